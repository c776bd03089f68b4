"""GPU: kick-drift-kick through a leaf plan with every step chosen on the device -- nbx_leaf_plan_step_kdk_adaptive, _get_step_clock and
_get_step_history (csrc/state_kernels.hip: step_controller_kernel, kick_drift_slots_clock_kernel; csrc/leaf_plan_api.hip:
plan_run_adaptive) through the C ABI, with the conventions of tests/test_gpu_tree_kdk.py.

Inputs, unless a test says otherwise, are contracting_bodies: n bodies of fp32 values in the unit cube (square) with masses around 1 / n
and velocities -(x - centre), 2 % of that at random on top, under a weak coupling G = 1e-5 and softening 1/64.  The velocities
shrink the cloud by the factor 1 - dt per step whatever the forces do, the largest acceleration grows as its size to the power -2
(Newton) or -3 (the tree codes' leaf law), and so the loop has to choose a different dt at nearly every step -- also with pow2, where
three different steps need a_max to change 16-fold.  c = 0.16 a_max(0), which makes the first raw step 0.4 and every later one about
0.6 x the one before (0.75 x or more with pow2); dt_max = 4, dt_min = 1/256, 16 steps.  (leaves.adaptive_leapfrog_spec run on these inputs at n = 2 .. 1000 chose
at least 3 different steps in every case, 4 or more with pow2 off.)  What is judged
bit for bit is judged with np.array_equal; the specification is leaves.choose_step / adaptive_leapfrog_spec, and the eccentric binary
and its certificate are tests/test_adaptive_step_cpu.py's."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_adaptive_step_cpu import BIN_C, BIN_DT_MAX, BIN_DT_MIN, BIN_EPS, BIN_EXTRA, BIN_FACTOR, BIN_G, BIN_PERIOD, binary_system
from test_gpu_tree_kdk import NBX_ERR_INVALID, NBX_ERR_STATE, ROOT, _with_bodies_left_out, downloaded, status

pytestmark = pytest.mark.gpu
N, DEPTH, THETA, EPS, G = 20000, 3, 0.5, 1.0 / 64, 1.0e-5
DT_MIN, DT_MAX, STEPS = 1.0 / 256, 4.0, 16
INF = float("inf")


def contracting_bodies(n, dim, seed=0):
    rng = np.random.default_rng(1000 * dim + seed + n)
    x = rng.uniform(0.0, 1.0, size=(n, dim))
    v = -(x - 0.5) * (1.0 + 0.02 * rng.normal(size=(n, dim)))
    m = rng.uniform(0.5, 1.5, size=(n, 1)) / n
    return np.ascontiguousarray(np.hstack([x, v, m]).astype(np.float32).astype(np.float64))


def law_of(nbx, law):
    return nbx.LAW_NEWTON if law == "newton" else nbx.LAW_TREE_LEAF


SHAPES = {   # name: (n, how the plan is made, rebuild_every)
    "n1": (1, "all_pairs", 0), "n2": (2, "all_pairs", 0), "n256": (256, "all_pairs", 0), "n257": (257, "all_pairs", 0),
    "left_out": (1000, "left_out", 0),
    "octree": (N, "octree", 0), "octree_rebuild1": (N, "octree", 1), "octree_rebuild3": (N, "octree", 3), "adaptive32_rebuild3": (N, "adaptive", 3),
}


def make_plan(nbx, c, b, how):
    n, dim = b.shape[0], (b.shape[1] - 1) // 2
    if how == "octree":
        p = nbx.LeafPlan.from_octree(c, DEPTH, THETA)
    elif how == "adaptive":
        p = nbx.LeafPlan.from_octree_adaptive(c, 10, 32, THETA)
    elif how == "left_out":
        p = nbx.LeafPlan(n, dim, *_with_bodies_left_out(nbx, b, dim)[0])
    else:
        p = nbx.LeafPlan(n, dim, *nbx.leaves.all_pairs_leaves(n, 64))
    if how in ("octree", "adaptive"):
        p.set_far_order(nbx.FAR_QUADRUPOLE)
    p.set_softening(EPS)
    return p


def accel_length_for(p, c, code):
    """c with raw = 0.4 at the start, from the plan's own largest acceleration there (an evaluation moves nothing)"""
    p.forces_ctx(c, code, G, fetch=False)
    a0 = p.max_accel()
    return 0.16 * a0 if a0 > 0 else 1.0


def replay(nbx, p, c, code, a_hist, dt_hist, rebuild_every, t_start, t_end):
    """the recorded steps spelled out with forces_ctx and kick_drift2; returns t by the rule and the a_max seen at every evaluation"""
    t, prev, seen = t_start, 0.0, []
    for e, dt in enumerate(dt_hist):
        if rebuild_every > 0 and e % rebuild_every == 0:
            p.rebuild(c)
        p.forces_ctx(c, code, G, fetch=False)
        seen.append(p.max_accel())
        if e == len(dt_hist) - 1:
            assert dt == 0.0
            if prev != 0.0:
                p.kick_drift2(c, 0.5 * prev, 0.0)
            break
        t = t_end if dt >= t_end - t else t + dt
        p.kick_drift2(c, 0.5 * prev + 0.5 * dt, dt)
        prev = dt
    return t, np.array(seen)


# ---- 1: replay, bit for bit -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pow2", (False, True))
@pytest.mark.parametrize("law", ("newton", "tree_leaf"))
@pytest.mark.parametrize("dim", (3, 2))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_replay_bit_for_bit(nbx, shape, dim, law, pow2):
    """An adaptive call on context A; on context B, with an equal plan, the history's steps spelled out.  Bodies, get_forces(), the
    structure and the clock's t are the same bits, and max_accel() at every evaluation on B is the recorded a_max.  The history holds at
    least three different steps and neither clamp everywhere -- except at n = 1, where no pair exists, a_max is 0 at every evaluation
    and every step is dt_max by the rule: that is what is asserted there."""
    n, how, every = SHAPES[shape]
    code = law_of(nbx, law)
    b0 = contracting_bodies(n, dim)
    with nbx.Context(n, dim) as ca, nbx.Context(n, dim) as cb:
        ca.upload(b0); cb.upload(b0)
        with make_plan(nbx, ca, b0, how) as pa, make_plan(nbx, cb, b0, how) as pb:
            c = accel_length_for(pa, ca, code)
            clock = pa.step_kdk_adaptive(ca, code, G, c, DT_MIN, DT_MAX, max_steps=STEPS, rebuild_every=every, pow2=pow2)
            a_hist, dt_hist = pa.step_history()
            assert clock.status == 0 and clock.finished == 0 and clock.steps == STEPS and clock.evaluations == STEPS + 1 == a_hist.size
            assert clock.dt_last == dt_hist[-2] and clock.a_max_last == a_hist[-1] and dt_hist[-1] == 0.0
            t, seen = replay(nbx, pb, cb, code, a_hist, dt_hist, every, 0.0, INF)
            ga, gb = downloaded(ca, b0), downloaded(cb, b0)
            fa, fb = pa.get_forces(), pb.get_forces()
            if how in ("octree", "adaptive"):
                assert all(np.array_equal(x, y) for x, y in zip(pa.structure(), pb.structure()))
                assert pa.softening == EPS and pa.far_order == 1
    dts = dt_hist[:-1]
    print(f"{shape} {dim}D {law} pow2={pow2}: a_max {a_hist.min():.3e}..{a_hist.max():.3e}, dt {dts.min():.4g}..{dts.max():.4g}, {np.unique(dts).size} different")
    assert np.array_equal(seen, a_hist)
    assert np.array_equal(ga, gb) and np.array_equal(fa, fb) and clock.t == t
    assert not np.array_equal(ga[:, :dim], b0[:, :dim])
    if n == 1:
        assert not a_hist.any() and (dts == DT_MAX).all()
        return
    assert not np.array_equal(ga[:, dim:2 * dim], b0[:, dim:2 * dim]), "coupling too weak to test anything"
    assert np.unique(dts).size >= 3 and not (dts == DT_MIN).all() and not (dts == DT_MAX).all()
    assert (dts >= DT_MIN).all() and (dts <= DT_MAX).all()
    if how == "left_out":
        out = _with_bodies_left_out(nbx, b0, dim)[1]
        assert out.size == 37 and np.array_equal(ga[out, dim:2 * dim], b0[out, dim:2 * dim]) and not fa[out].any()


# ---- 2: the device's choice is the specification's -----------------------------------------------------------------------------------

@pytest.mark.parametrize("law", ("newton", "tree_leaf"))
@pytest.mark.parametrize("dim", (3, 2))
def test_the_choice_is_the_specification(nbx, dim, law):
    """24 steps at n = 257.  pow2 off: choose_step of the recorded a_max is the recorded dt within 2 ulp (whether it was exact is
    printed).  pow2 on: no recorded raw lies within 4 ulp of a boundary dt_max 2^-j, and then every dt is the specification's exactly."""
    n, code, steps = 257, law_of(nbx, law), 24
    b0 = contracting_bodies(n, dim)
    for pow2 in (False, True):
        with nbx.Context(n, dim) as c, make_plan(nbx, c, b0, "all_pairs") as p:
            c.upload(b0)
            k = accel_length_for(p, c, code)
            clock = p.step_kdk_adaptive(c, code, G, k, DT_MIN, DT_MAX, max_steps=steps, pow2=pow2)
            a_hist, dt_hist = p.step_history()
        assert clock.steps == steps and a_hist.size == steps + 1
        a, dts = a_hist[:-1], dt_hist[:-1]
        want = np.array([nbx.leaves.choose_step(x, k, DT_MIN, DT_MAX, pow2) for x in a])
        assert np.unique(dts).size >= 3
        if not pow2:
            ulps = np.abs(dts - want) / np.spacing(want)
            print(f"{dim}D {law}: choose_step against the device: largest difference {ulps.max():.0f} ulp, exact = {bool((dts == want).all())}")
            assert (ulps <= 2).all()
        else:
            raw = np.sqrt(k / a)
            bounds = DT_MAX / 2.0 ** np.arange(0, 8)
            assert (np.abs(raw[:, None] - bounds[None, :]) > 4 * np.spacing(raw)[:, None]).all(), "a raw step on a boundary: choose another input"
            j = np.log2(DT_MAX / dts)
            assert np.array_equal(j, np.round(j)) and np.array_equal(dts, DT_MAX / 2.0 ** j)
            assert np.array_equal(dts, want)


# ---- 3: equal clamps are the fixed-step loops ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,every", (("n257", 0), ("octree", 0), ("octree", 2), ("adaptive", 1)))
def test_equal_clamps_give_the_bits_of_the_fixed_step_loops(nbx, shape, every):
    """dt_min == dt_max == dt, t_end = inf, max_steps = n against step_kdk / step_octree_kdk(rebuild_every): bodies, get_forces() and
    the structure bit for bit, with pow2 on and off."""
    dim, dt, steps = 3, 0.125, 4
    n, how = (257, "all_pairs") if shape == "n257" else (N, shape)
    b0 = contracting_bodies(n, dim)
    got = {}
    for kind in ("fixed", False, True):
        with nbx.Context(n, dim) as c:
            c.upload(b0)
            with make_plan(nbx, c, b0, how) as p:
                if kind == "fixed":
                    (p.step_octree_kdk(c, nbx.LAW_NEWTON, G, dt, steps, every) if every else p.step_kdk(c, nbx.LAW_NEWTON, G, dt, steps))
                else:
                    clock = p.step_kdk_adaptive(c, nbx.LAW_NEWTON, G, 1.0e-3, dt, dt, max_steps=steps, rebuild_every=every, pow2=kind)
                    assert clock.steps == steps and clock.t == steps * dt and clock.finished == 0 and (p.step_history()[1][:-1] == dt).all()
                got[kind] = (downloaded(c, b0), p.get_forces()) + (p.structure() if how != "all_pairs" else ())
    for kind in (False, True):
        assert all(np.array_equal(x, y) for x, y in zip(got[kind], got["fixed"])), f"pow2 = {kind}"
    assert not np.array_equal(got["fixed"][0][:, :6], b0[:, :6])


# ---- 4: landing on t_end ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,every,max_steps", (("n257", 0, 200), ("octree", 0, 40), ("octree", 3, 40), ("adaptive", 1, 40)))
@pytest.mark.parametrize("pow2", (False, True))
def test_landing_on_t_end(nbx, shape, every, max_steps, pow2):
    """t_end = 0.7 with max_steps well above what is needed: the clock stands at t_end bit for bit, finished, in fewer steps; only the
    landing step may be below dt_min; and bodies, get_forces(), structure and history are those of a second run whose max_steps is the
    number of steps taken -- the evaluations queued behind the stop (up to 200 here, past several of the loop's looks) changed
    nothing."""
    dim, t_start, t_end = 3, 0.125, 0.7
    n, how = (257, "all_pairs") if shape == "n257" else (N, shape)
    b0 = contracting_bodies(n, dim)
    got = {}
    for run in ("long", "exact"):
        with nbx.Context(n, dim) as c:
            c.upload(b0)
            with make_plan(nbx, c, b0, how) as p:
                k = accel_length_for(p, c, nbx.LAW_NEWTON) / 4.0                         # raw = 0.2 at the start: several steps to t_end
                cap = max_steps if run == "long" else got["long"][0].steps
                clock = p.step_kdk_adaptive(c, nbx.LAW_NEWTON, G, k, 0.02, DT_MAX, t_end=t_end, max_steps=cap, rebuild_every=every, t_start=t_start, pow2=pow2)
                got[run] = (clock, downloaded(c, b0), p.get_forces(), *p.step_history()) + (p.structure() if how != "all_pairs" else ())
    clock, _, _, a_hist, dt_hist = got["long"][:5]
    dts = dt_hist[:-1]
    print(f"{shape} every {every} pow2={pow2}: {clock.steps} steps, dt {dts.min():.4g}..{dts.max():.4g}, landing step {dts[-1]:.4g}")
    assert clock.t == t_end and clock.finished == 1 and clock.status == 0 and 3 <= clock.steps < max_steps
    assert clock.evaluations == clock.steps + 1 == a_hist.size and dt_hist[-1] == 0.0
    assert (dts[:-1] >= 0.02).all() and dts[-1] > 0 and abs(dts.sum() - (t_end - t_start)) <= 4 * dts.size * np.spacing(t_end)
    other = got["exact"][0]
    assert (other.t, other.steps, other.evaluations, other.finished, other.dt_last, other.a_max_last) == (clock.t, clock.steps, clock.evaluations, 1, clock.dt_last, clock.a_max_last)
    assert all(np.array_equal(x, y) for x, y in zip(got["long"][1:], got["exact"][1:]))


# ---- 5: chaining -----------------------------------------------------------------------------------------------------------------------

def test_chained_calls_against_one_call(nbx):
    """3 + 3 steps (the second call starting at the first's t) against 6 in one call, n = 257.  The second call's opening evaluation
    sees the positions of the first call's closing one, so sums, a_max and dt are the same bits; what differs is the joint: one call
    makes v + A (0.5 p + 0.5 d) there, two calls (v + A (0.5 p)) + A (0.5 d).  With u = 2^-53 each product and each sum rounds once, so
    the two differ by at most 2 u (|v| + |A| (p + d)) + u |v| <= 4 u V per component, V = max(|v|) over the run's ends, |A| (p + d) <=
    2 |dv| being covered by V up to the same factor.  The K = 3 kicks behind the joint add the same products to velocities one rounding
    apart, each sum rounding again: |dv| <= (4 + K) u V.  The drifts carry it into x: |dx| <= (4 + K) u V T + K u X over the remaining
    time T.  Bounds asserted: 2 x those, per body with the largest-component norms."""
    n, dim, K = 257, 3, 3
    b0 = contracting_bodies(n, dim)
    u = 2.0 ** -53
    runs = {}
    for name in ("one", "two"):
        with nbx.Context(n, dim) as c, make_plan(nbx, c, b0, "all_pairs") as p:
            c.upload(b0)
            k = accel_length_for(p, c, nbx.LAW_NEWTON)
            if name == "one":
                clock = p.step_kdk_adaptive(c, nbx.LAW_NEWTON, G, k, DT_MIN, DT_MAX, max_steps=2 * K)
                hist = p.step_history()[1][:-1]
            else:
                first = p.step_kdk_adaptive(c, nbx.LAW_NEWTON, G, k, DT_MIN, DT_MAX, max_steps=K)
                h1 = p.step_history()[1][:-1]
                clock = p.step_kdk_adaptive(c, nbx.LAW_NEWTON, G, k, DT_MIN, DT_MAX, max_steps=K, t_start=first.t)
                hist = np.concatenate([h1, p.step_history()[1][:-1]])
                assert clock.steps == K and first.steps == K
            runs[name] = (downloaded(c, b0), clock.t, hist)
    (one, t1, h_one), (two, t2, h_two) = runs["one"], runs["two"]
    assert np.allclose(h_one, h_two, rtol=1e-12, atol=0.0) and abs(t1 - t2) <= 1e-12 * t1
    v = slice(dim, 2 * dim)
    V = np.maximum(np.abs(b0[:, v]).max(axis=1), np.abs(one[:, v]).max(axis=1))
    X = np.abs(one[:, :dim]).max(axis=1)
    T = h_one[K:].sum()
    dv = np.abs(one[:, v] - two[:, v]).max(axis=1)
    dx = np.abs(one[:, :dim] - two[:, :dim]).max(axis=1)
    bound_v = 2 * (4 + K) * u * V
    bound_x = 2 * ((4 + K) * u * V * T + K * u * X)
    print(f"chained against one call: dv / bound {float((dv / bound_v).max()):.3f}, dx / bound {float((dx / bound_x).max()):.3f}, bodies that differ {int((dv > 0).sum())}")
    assert (dv <= bound_v).all() and (dx <= bound_x).all()
    assert np.abs(one[:, v] - b0[:, v]).max() > 1e6 * bound_v.max(), "coupling too weak to test anything"


# ---- 6: the eccentric binary -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra", (0, BIN_EXTRA))
@pytest.mark.parametrize("pow2", (False, True))
@pytest.mark.parametrize("c", BIN_C)
def test_eccentric_binary(nbx, c, pow2, extra):
    """tests/test_adaptive_step_cpu.py's binary, alone and among 256 light distant bodies, one period in chained one-step calls with the
    energy by plan.energy at every end: the adaptive loop's worst |E / E0 - 1| is at least 10 x below step_kdk's with the same calls,
    steps and evaluations.  (The specification's figures are in that module's docstring.)"""
    b0 = binary_system(extra)
    n = b0.shape[0]
    assert (b0[:, -1] > 0).all()
    worst = {}
    steps = 0
    for scheme in ("adaptive", "fixed"):
        with nbx.Context(n, 3) as ctx, nbx.LeafPlan(n, 3, *nbx.leaves.all_pairs_leaves(n, 64)) as p:
            ctx.upload(b0)
            p.set_softening(BIN_EPS)
            e0 = sum(p.energy(ctx, nbx.LAW_NEWTON, BIN_G))
            worst[scheme] = 0.0
            if scheme == "adaptive":
                t = 0.0
                while True:
                    clock = p.step_kdk_adaptive(ctx, nbx.LAW_NEWTON, BIN_G, c, BIN_DT_MIN, BIN_DT_MAX, t_end=BIN_PERIOD, max_steps=1, t_start=t, pow2=pow2)
                    assert clock.status == 0
                    steps += clock.steps
                    t = clock.t
                    worst[scheme] = max(worst[scheme], abs(sum(p.energy(ctx, nbx.LAW_NEWTON, BIN_G)) / e0 - 1.0))
                    if clock.finished:
                        break
                    assert steps < 2000
                assert t == BIN_PERIOD
            else:
                for _ in range(steps):
                    p.step_kdk(ctx, nbx.LAW_NEWTON, BIN_G, BIN_PERIOD / steps, 1)
                    worst[scheme] = max(worst[scheme], abs(sum(p.energy(ctx, nbx.LAW_NEWTON, BIN_G)) / e0 - 1.0))
    print(f"binary n = {n}, c = {c:g}, pow2 = {pow2}: {steps} steps, worst |E/E0 - 1| adaptive {worst['adaptive']:.3e}, fixed {worst['fixed']:.3e}, "
          f"ratio {worst['fixed'] / worst['adaptive']:.1f}")
    assert e0 < 0
    assert BIN_FACTOR * worst["adaptive"] <= worst["fixed"]


# ---- 7: an a_max that is not finite ----------------------------------------------------------------------------------------------------

def test_an_acceleration_that_is_not_finite_stops_the_loop(nbx):
    """One NaN position, uploaded (a value, not a fault): status 1 at the first evaluation, no entry in the history, and positions and
    velocities are the uploaded bits.  After one good step of the same plan on good bodies the NaN is met at the second evaluation: the
    loop stops before that kick, so the velocities are those of a replay that leaves the closing half-kick out."""
    n, dim = 64, 3
    b0 = contracting_bodies(n, dim)
    bad = b0.copy()
    bad[n // 2, 1] = np.nan
    with nbx.Context(n, dim) as c, make_plan(nbx, c, b0, "all_pairs") as p:
        c.upload(bad)
        clock = p.step_kdk_adaptive(c, nbx.LAW_NEWTON, G, 1.0, DT_MIN, DT_MAX, max_steps=5)
        a_hist, dt_hist = p.step_history()
        g = downloaded(c, bad)
        assert clock.status == 1 and clock.steps == 0 and clock.evaluations == 1 and clock.finished == 0 and clock.t == 0.0
        assert not np.isfinite(clock.a_max_last) and a_hist.size == 0 and dt_hist.size == 0
        assert np.array_equal(g.view(np.uint64), bad.view(np.uint64))
        c.upload(b0)                                                     # the plan and its clock are good for the next call
        clock = p.step_kdk_adaptive(c, nbx.LAW_NEWTON, G, 1.0, DT_MIN, DT_MAX, max_steps=2)
        assert clock.status == 0 and clock.steps == 2 and p.step_history()[0].size == 3


# ---- 8: refusals and observers ---------------------------------------------------------------------------------------------------------

def test_refusals(nbx):
    """Every refusal of the header, with a plan and two contexts at hand; a refused call launches nothing."""
    n, dim = 64, 3
    b = contracting_bodies(n, dim)
    lib = nbx.load_library()
    with nbx.LeafPlan(n, dim, *nbx.leaves.all_pairs_leaves(n, 8)) as plan, nbx.Context(n, dim) as c, nbx.Context(n + 1, dim) as wrong, nbx.Context(n, dim) as empty:
        c.upload(b)
        wrong.upload(contracting_bodies(n + 1, dim))
        good = plan.forces_ctx(c, nbx.LAW_TREE_LEAF, G)
        assert status(nbx, plan.step_clock) == NBX_ERR_STATE and status(nbx, plan.step_history) == NBX_ERR_STATE

        def call(ctx=c, law=nbx.LAW_TREE_LEAF, max_steps=2, every=0, **change):
            kw = dict(accel_length=1.0e-3, dt_min=0.01, dt_max=0.1, t_start=0.0, t_end=INF, pow2=0, reserved=0)
            kw.update(change)
            k = nbx.StepControl(**kw)
            return lib.nbx_leaf_plan_step_kdk_adaptive(plan.h, ctx.h if ctx is not None else None, law, G, ctypes.byref(k), max_steps, every)

        for change in (dict(accel_length=0.0), dict(accel_length=INF), dict(accel_length=np.nan), dict(dt_min=0.0), dict(dt_min=0.2), dict(dt_min=np.nan), dict(dt_max=INF),
                       dict(t_start=INF), dict(t_start=np.nan), dict(t_end=np.nan), dict(t_end=-INF), dict(pow2=2), dict(reserved=1)):
            assert call(**change) == NBX_ERR_INVALID, change
        assert call(law=4) == NBX_ERR_INVALID and call(law=-1) == NBX_ERR_INVALID
        assert call(max_steps=-1) == NBX_ERR_INVALID and call(max_steps=(1 << 20) + 1) == NBX_ERR_INVALID and call(every=-1) == NBX_ERR_INVALID
        assert call(ctx=None) == NBX_ERR_INVALID and call(ctx=wrong) == NBX_ERR_INVALID
        assert lib.nbx_leaf_plan_step_kdk_adaptive(plan.h, c.h, nbx.LAW_TREE_LEAF, G, None, 2, 0) == NBX_ERR_INVALID
        assert call(ctx=empty) == NBX_ERR_STATE                                  # nothing uploaded
        assert call(every=1) == NBX_ERR_STATE                                    # not an octree plan
        assert call(law=nbx.LAW_NEWTON) == NBX_ERR_STATE                         # no softening length
        assert status(nbx, plan.step_clock) == NBX_ERR_STATE, "a refused call leaves no clock"
        assert np.array_equal(plan.get_forces(), good) and np.array_equal(downloaded(c, b), b)
        assert call(max_steps=0) == 0 and np.array_equal(downloaded(c, b), b)    # does nothing
        assert status(nbx, plan.step_clock) == NBX_ERR_STATE
        assert call() == 0
        assert plan.step_clock().steps == 2 and not np.array_equal(downloaded(c, b)[:, :dim], b[:, :dim])
        count = ctypes.c_size_t(0)
        one_a, one_dt = np.full(2, -1.0), np.full(2, -1.0)
        assert lib.nbx_leaf_plan_get_step_history(plan.h, one_a.ctypes.data, one_dt.ctypes.data, 1, ctypes.byref(count)) == 0
        assert count.value == 3 and one_a[0] > 0 and one_dt[0] > 0 and one_a[1] == -1.0 and one_dt[1] == -1.0, "capacity bounds what is written"
        assert lib.nbx_leaf_plan_get_step_history(plan.h, None, None, 0, None) == NBX_ERR_INVALID and lib.nbx_leaf_plan_get_step_clock(plan.h, None) == NBX_ERR_INVALID


def test_observers_and_the_fixed_step_loop_afterwards(nbx):
    """energy() between two adaptive calls changes no later bit; and after an adaptive call step_kdk on that plan gives the bits of a
    fresh plan from the same state."""
    n, dim = 257, 3
    b0 = contracting_bodies(n, dim)
    ends = []
    for observe in (False, True):
        with nbx.Context(n, dim) as c, make_plan(nbx, c, b0, "all_pairs") as p:
            c.upload(b0)
            k = accel_length_for(p, c, nbx.LAW_NEWTON)
            first = p.step_kdk_adaptive(c, nbx.LAW_NEWTON, G, k, DT_MIN, DT_MAX, max_steps=3)
            if observe:
                p.energy(c, nbx.LAW_NEWTON, G)
                assert p.max_accel() == first.a_max_last
                assert p.step_clock().t == first.t
            second = p.step_kdk_adaptive(c, nbx.LAW_NEWTON, G, k, DT_MIN, DT_MAX, max_steps=3, t_start=first.t, pow2=True)
            middle = downloaded(c, b0)
            p.step_kdk(c, nbx.LAW_NEWTON, G, 0.01, 2)
            ends.append((second.t, middle, downloaded(c, b0), p.get_forces(), *p.step_history()))
    assert ends[0][0] == ends[1][0] and all(np.array_equal(x, y) for x, y in zip(ends[0][1:], ends[1][1:]))
    with nbx.Context(n, dim) as c, make_plan(nbx, c, b0, "all_pairs") as fresh:
        c.upload(ends[0][1])                                                     # fp64 bodies in: the fp32 copies are rounded from them as the drift does
        fresh.step_kdk(c, nbx.LAW_NEWTON, G, 0.01, 2)
        assert np.array_equal(downloaded(c, b0), ends[0][2]) and np.array_equal(fresh.get_forces(), ends[0][3])


# ---- 9: the harness --------------------------------------------------------------------------------------------------------------------

def test_harness_runs_the_tree_with_steps_chosen_on_the_device(tmp_path):
    """nbody_sim -m t --law newton --integrator kdka --accel-length 4 --dt 1 --dt-min 0.01 --steps 8 --energy-every 4 on the 20,000-body
    Plummer sphere of tests/test_gpu_tree_kdk.py's harness test: every step row carries `_kdka` and no other row does, a line behind
    each gives the steps taken, t and the range of dt, and the Newtonian rows' energy lines come at the ends of chained calls of 4
    steps.  The same command without the new options prints the parent's rows and no word of this."""
    sim = os.path.join(ROOT, "nbody_sim")
    assert os.path.exists(sim)
    common = ["-N", "20000", "-m", "t", "--init", "plummer", "--G", "0.1", "--far-order", "1", "--leaf-cap", "32", "--law", "newton", "--softening", "2048",
              "--steps", "8", "--energy-every", "4", "--dt", "1"]

    def run(name, extra):
        cwd = tmp_path / name
        cwd.mkdir()
        p = subprocess.run([sim] + common + extra, cwd=cwd, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        found = [os.path.join(d, f_) for d, _, files in os.walk(cwd) for f_ in files if f_.endswith(".csv")]
        return p.stdout, [line.split(",")[0] for path in sorted(found) for line in open(path) if line.startswith("BarnesHut_HIP")]

    parents = ["BarnesHut_HIP_adaptive", "BarnesHut_HIP_adaptive_steps", "BarnesHut_HIP_adaptive_quad", "BarnesHut_HIP_adaptive_steps_quad",
               "BarnesHut_HIP_adaptive_newton", "BarnesHut_HIP_adaptive_newton_steps", "BarnesHut_HIP_adaptive_newton_quad", "BarnesHut_HIP_adaptive_newton_quad_steps"]
    plain_out, plain_rows = run("kd", [])
    out, rows = run("kdka", ["--integrator", "kdka", "--accel-length", "4", "--dt-min", "0.01"])
    assert plain_rows == parents, plain_rows
    assert "kdka" not in plain_out and "Adaptive steps" not in plain_out and "chosen on the device" not in plain_out
    assert rows == [r + "_kdka" if "_steps" in r else r for r in parents], rows
    summary = [line for line in out.splitlines() if line.startswith("Adaptive steps: ")]
    assert len(summary) == 4 and len(out.splitlines()) == len(plain_out.splitlines()) + 4, out
    for line in summary:
        assert line.startswith("Adaptive steps: 8 taken, t = "), line
        t = float(line.split("t = ")[1].split(",")[0])
        lo, hi = (float(x) for x in line.split(", dt ")[1].split(",")[0].split(" .. "))
        assert 0.01 <= lo <= hi <= 1.0 and 8 * lo <= t * (1 + 1e-9) and t <= 8 * hi * (1 + 1e-9), line
    start = out.index("softened Newtonian law")
    energy = [line for line in out[start:].splitlines() if line.startswith("step ")]
    assert [line.split()[1] for line in energy] == ["0", "4", "8"] * 2 and all("E = " in line for line in energy), out
    for line in energy:
        assert float(line.split("E = ")[1].split()[0]) < 0, line
        if not line.startswith("step 0 "):
            assert float(line.split("|dE/E0| = ")[1].split()[0]) < 1e-2 and "2K/|U| " in line and float(line.split("  t = ")[1]) > 0, line
    assert out.count("steps chosen on the device") == 4
    refused = subprocess.run([sim] + common + ["--integrator", "kdka"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert refused.returncode == 1 and "--accel-length" in refused.stderr
