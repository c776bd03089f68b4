"""GPU: the all-pairs context's kick-drift-kick with every step chosen on the device -- nbx_ctx_max_accel, nbx_ctx_step_kdk_adaptive,
nbx_ctx_get_step_clock and nbx_ctx_get_step_history (csrc/state_kernels.hip: ctx_accel_max_kernel, kick_drift_clock_kernel and the plan's
step_controller_kernel; csrc/nbx_api.hip: the driver and its window) through the C ABI, by the conventions of
tests/test_gpu_adaptive_step.py, whose cases these are for the context.

Laws: "reference" (the reference's r^-4 form), "soft" (the same, softened) and "newton" (attractive, softened), crossed with D = 3, 2.

Inputs, unless a test says otherwise, are shrinking_cloud: n bodies of fp32 values in a cube of side 65,536 whose lowest corner is at
32,768 in every coordinate, masses around 1 / n, velocities -(x - centre) with 1e-4 of that at random on top, under a coupling that
bends no path before the cloud has all but collapsed.  The cloud's size goes as 1 - t until then, so the largest acceleration grows as that to the power
-3 (Newton: -2) and the loop has to choose a different dt nearly every time; c = 0.16 a_max(0) makes the first raw step 0.4, and the
steps add up to t near 1, where the cloud is smallest.  Up to t = 2.5 every coordinate stays above 16,384, the bound below
which the unsoftened fast path looks for close pairs: no body is ever a close-set candidate, so the context's asynchronous look at its
close-set counters cannot pick different kernels in two runs that are compared bit for bit (the softened laws have no close set).

What is judged bit for bit is judged with np.array_equal.  The specification is leaves.choose_step / adaptive_leapfrog_spec with
tests/test_ctx_adaptive_step_cpu.py's ctx_accel_fn; the eccentric binary and its certificate are tests/test_adaptive_step_cpu.py's."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from test_adaptive_step_cpu import BIN_C, BIN_DT_MAX, BIN_DT_MIN, BIN_EPS, BIN_EXTRA, BIN_FACTOR, BIN_G, BIN_PERIOD, binary_system
from test_ctx_adaptive_step_cpu import LAWS, ctx_accel_fn
from test_gpu_tree_kdk import NBX_ERR_INVALID, NBX_ERR_STATE, ROOT, downloaded, status

pytestmark = pytest.mark.gpu
LOW, SIDE = 32768.0, 65536.0
CLOUD_EPS = 1.0                                                    # the softened laws' length on the cloud: far below every distance met
CLOUD_G = {"reference": 1.0e8, "soft": 1.0e8, "newton": 1.0e4}     # weak couplings: a(0) ~ 1e-2 against velocities of 3e4
DT_MIN, DT_MAX, STEPS = 1.0 / 256, 0.5, 16
INF = float("inf")


def shrinking_cloud(n, dim, seed=0):
    rng = np.random.default_rng(1000 * dim + seed + n)
    x = LOW + SIDE * rng.uniform(0.0, 1.0, size=(n, dim))
    v = -(x - (LOW + 0.5 * SIDE)) * (1.0 + 1.0e-4 * rng.normal(size=(n, dim)))
    m = rng.uniform(0.5, 1.5, size=(n, 1)) / n
    return np.ascontiguousarray(np.hstack([x, v, m]).astype(np.float32).astype(np.float64))


def set_law(nbx, c, law, eps=CLOUD_EPS):
    if law != "reference":
        c.set_softening(eps)
    if law == "newton":
        c.set_law(nbx.FORCE_LAW_NEWTON)


def context(nbx, b, law, eps=CLOUD_EPS):
    c = nbx.Context(b.shape[0], (b.shape[1] - 1) // 2)
    c.upload(b)
    set_law(nbx, c, law, eps)
    return c


def accel_length_for(c, G, factor=0.16):
    """c with raw = sqrt(factor) at the start, from the context's own largest acceleration there (an evaluation moves nothing)"""
    c.compute_accel()
    a0 = c.max_accel(G)
    return factor * a0 if a0 > 0 else 1.0


def replay(c, G, dt_hist, t_start=0.0, t_end=INF):
    """the recorded steps spelled out with compute_accel and kick_drift2; returns t by the rule and the a_max seen at every evaluation"""
    t, prev, seen = t_start, 0.0, []
    for e, dt in enumerate(dt_hist):
        c.compute_accel()
        seen.append(c.max_accel(G))
        if e == len(dt_hist) - 1:
            assert dt == 0.0
            if prev != 0.0:
                c.kick_drift2(0.5 * prev, 0.0, G)
            break
        t = t_end if dt >= t_end - t else t + dt
        c.kick_drift2(0.5 * prev + 0.5 * dt, dt, G)
        prev = dt
    return t, np.array(seen)


# ---- 1: the maximum is the maximum -----------------------------------------------------------------------------------------------------

PAIR_M, PAIR_GAP, PAIR_EPS = 1.0e6, 16.0, 4.0


def cloud_with_a_heavy_pair(n, dim, first):
    """shrinking_cloud's positions at rest with masses around 1, and bodies first, first + 1 made a pair of mass 1e6 each, 16 apart
    along x: their acceleration (~1e6 / 16^3 per unit G) is far above what anything does to a light body thousands away"""
    b = shrinking_cloud(n, dim, seed=first)
    b[:, dim:2 * dim] = 0.0
    b[:, -1] = np.float32(1.0) * (b[:, -1] * n).astype(np.float32)
    b[first + 1, :dim] = b[first, :dim]
    b[first + 1, 0] += PAIR_GAP
    b[[first, first + 1], -1] = PAIR_M
    return np.ascontiguousarray(b.astype(np.float32).astype(np.float64))


def pairs_for(n):
    return sorted({p for p in (0, 255, n - 2, 4095) if 0 <= p and p + 1 < n})


def assert_is_the_maximum(c, b, G, pair, what):
    """max_accel against max_l |F_l| / m_l of get_forces.  Roundings (u = 2^-53, relative): F_k = -((G m) A_k) carries 2; its square 1
    more on top of twice that (5 u), the D - 1 additions 2, the root halves it and adds 1 (4.5 u), the division by m 1 (5.5 u); the
    device's |G| sqrt(sum A_k^2) carries 1 + 2, halved, + 1, + 1 = 3.5 u.  Together 9 u; the issue's bound 16 u is asserted."""
    dim = (b.shape[1] - 1) // 2
    got = c.max_accel(G)
    mag = np.sqrt((c.forces(G) ** 2).sum(axis=1)) / b[:c.count, -1] if c.count else np.zeros(0)
    want = float(mag.max()) if mag.size else 0.0
    assert want > 0 and abs(got - want) <= 16 * 2.0 ** -53 * want, f"{what}: {got!r} against {want!r}"
    assert int(np.argmax(mag)) in pair, f"{what}: the largest acceleration is body {int(np.argmax(mag))}'s, not the pair's"
    assert dim in (2, 3)


MODES = ("default", "plain", "guarded", "strict")


def set_mode(nbx, c, mode):
    if mode == "plain":
        c.set_refine(0.0, 0.0)
    elif mode == "guarded":
        c.set_tuning(0, nbx.variants().index("lds_t1_w8_exact_u8"))
    elif mode == "strict":
        c.set_tuning(0, nbx.variants().index("strict_f64_t4"))


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("dim", (3, 2))
@pytest.mark.parametrize("n", (2, 257, 4097, 8193))
def test_the_maximum_is_the_maximum(nbx, n, dim, law):
    """The heavy pair at {0, 1}, {255, 256}, {n - 2, n - 1} and {4095, 4096} -- edges of waves, workgroups and the 4,096 pad -- wherever
    n has room for it, under the default variant (mixed mode), plain fp32, the guarded fallback and the strict fp64 variant (the
    softened laws run their fast kernel whatever is asked for): max_accel is the largest |F| / m of get_forces to 16 x 2^-53 and the
    body that owns it is a member of the pair."""
    G = 1.0e-3
    for mode in MODES:
        with nbx.Context(n, dim) as c:
            for first in pairs_for(n):
                b = cloud_with_a_heavy_pair(n, dim, first)
                c.upload(b)
                set_law(nbx, c, law, PAIR_EPS)
                set_mode(nbx, c, mode)
                if law == "reference" and mode in ("guarded", "strict"):
                    assert c.effective_tuning()[0] == ("lds_t1_w8_exact_u8" if mode == "guarded" else "strict_f64_t4")
                c.compute_accel()
                assert_is_the_maximum(c, b, G, (first, first + 1), f"n={n} D={dim} {law} {mode} pair at {first}")
                assert np.array_equal(downloaded(c, b), b), "an observer"


@pytest.mark.parametrize("dim", (3, 2))
def test_the_maximum_over_the_symmetric_pass_planes(nbx, dim):
    """n = 65,536 is 8 super-blocks: the default run takes the symmetric pass, whose S + K slots of two planes are what is summed."""
    n, G = 65536, 1.0e-3
    first = 40000
    b = cloud_with_a_heavy_pair(n, dim, first)
    with nbx.Context(n, dim) as c:
        c.upload(b)
        assert c.effective_tuning()[0] == "sympk3l_t8_w3"
        c.compute_accel()
        assert c.effective_tuning()[0] == "sympk3l_t8_w3" and c.effective_tuning()[1] >= 8
        assert_is_the_maximum(c, b, G, (first, first + 1), f"symmetric pass D={dim}")


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("dim", (3, 2))
def test_the_maximum_of_each_shard_of_a_two_shard_context(nbx, dim, law):
    """LOCAL + REMOTE on each of two shards on one device: each shard's max_accel is the maximum over its own rows -- the pair's on the
    shard that holds it, a light body's on the other -- and before the LOCAL pass the call is refused."""
    n, G, first = 4097, 1.0e-3, 100                              # shard_len 2049: the pair lives on shard 0
    b = cloud_with_a_heavy_pair(n, dim, first)
    seen = []
    for shard in (0, 1):
        with nbx.Context(n, dim, 0, 2, shard) as c:
            c.upload(b)
            set_law(nbx, c, law, PAIR_EPS)
            assert status(nbx, lambda: c.max_accel(G)) == NBX_ERR_STATE
            c.compute_accel(nbx.SRC_LOCAL)
            c.compute_accel(nbx.SRC_REMOTE)
            lo = shard * c.shard_len
            rows = b[lo:lo + c.count]
            mag = np.sqrt((c.forces(G) ** 2).sum(axis=1)) / rows[:, -1]
            got = c.max_accel(G)
            assert abs(got - mag.max()) <= 16 * 2.0 ** -53 * mag.max()
            assert (int(np.argmax(mag)) + lo in (first, first + 1)) == (shard == 0)
            seen.append(got)
    assert seen[0] > 1.0e3 * seen[1] > 0


def test_an_empty_shard_has_no_acceleration(nbx):
    b = cloud_with_a_heavy_pair(2, 3, 0)
    with nbx.Context(2, 3, 0, 4, 3) as c:                        # shard_len 1: shards 2 and 3 are empty
        assert c.count == 0
        c.upload(b)
        c.compute_accel()
        assert c.max_accel(1.0) == 0.0


# ---- 2: equal clamps give the fixed loop's bits ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("dim", (3, 2))
@pytest.mark.parametrize("n", (257, 4097))
def test_equal_clamps_give_the_bits_of_step_kdk(nbx, n, dim, law):
    """dt_min == dt_max == dt, t_end = inf, 5 steps against nbx_ctx_step_kdk: bodies and get_forces bit for bit, pow2 on and off"""
    dt, steps, G = 0.125, 5, CLOUD_G[law]
    b0 = shrinking_cloud(n, dim)
    got = {}
    for kind in ("fixed", False, True):
        with context(nbx, b0, law) as c:
            if kind == "fixed":
                c.step_kdk(dt, steps, G)
            else:
                clock = c.step_kdk_adaptive(1.0e-3, dt, dt, max_steps=steps, pow2=kind, G=G)
                assert clock.steps == steps and clock.t == steps * dt and clock.finished == 0 and clock.status == 0 and clock.evaluations == steps + 1
                assert (c.step_history()[1][:-1] == dt).all()
            got[kind] = (downloaded(c, b0), c.forces(G))
    for kind in (False, True):
        assert all(np.array_equal(x, y) for x, y in zip(got[kind], got["fixed"])), f"pow2 = {kind}"
    assert not np.array_equal(got["fixed"][0][:, :dim], b0[:, :dim])
    assert not np.array_equal(got["fixed"][0][:, dim:2 * dim], b0[:, dim:2 * dim]), "coupling too weak to test anything"


# ---- 3: replay, bit for bit ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pow2", (False, True))
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("n,dim", ((257, 3), (257, 2), (2, 3), (4097, 3)))
def test_replay_bit_for_bit(nbx, n, dim, law, pow2):
    """An adaptive call on context A; on context B the history's steps spelled out with compute_accel and kick_drift2.  Bodies,
    get_forces and the clock's t are the same bits, max_accel at every evaluation on B is the recorded a_max, and every recorded dt is
    leaves.choose_step of the recorded a_max bit for bit.  The history holds at least three different steps and neither clamp
    everywhere."""
    G = CLOUD_G[law]
    b0 = shrinking_cloud(n, dim)
    with context(nbx, b0, law) as ca, context(nbx, b0, law) as cb:
        k = accel_length_for(ca, G)
        clock = ca.step_kdk_adaptive(k, DT_MIN, DT_MAX, max_steps=STEPS, pow2=pow2, G=G)
        a_hist, dt_hist = ca.step_history()
        assert clock.status == 0 and clock.finished == 0 and clock.steps == STEPS and clock.evaluations == STEPS + 1 == a_hist.size
        assert clock.dt_last == dt_hist[-2] and clock.a_max_last == a_hist[-1] and dt_hist[-1] == 0.0
        t, seen = replay(cb, G, dt_hist)
        ga, gb = downloaded(ca, b0), downloaded(cb, b0)
        fa, fb = ca.forces(G), cb.forces(G)
    dts = dt_hist[:-1]
    print(f"n={n} {dim}D {law} pow2={pow2}: a_max {a_hist.min():.3e}..{a_hist.max():.3e}, dt {dts.min():.4g}..{dts.max():.4g}, {np.unique(dts).size} different")
    assert np.array_equal(seen, a_hist)
    assert np.array_equal(ga, gb) and np.array_equal(fa, fb) and clock.t == t
    assert not np.array_equal(ga[:, :dim], b0[:, :dim]) and not np.array_equal(ga[:, dim:2 * dim], b0[:, dim:2 * dim])
    want = np.array([nbx.leaves.choose_step(x, k, DT_MIN, DT_MAX, pow2) for x in a_hist[:-1]])
    assert np.array_equal(dts, want)
    assert np.unique(dts).size >= 3 and not (dts == DT_MIN).all() and not (dts == DT_MAX).all()
    assert (dts >= DT_MIN).all() and (dts <= DT_MAX).all()


# ---- 4: against the specification ------------------------------------------------------------------------------------------------------

SPEC_CASES = {"reference": (0.0, 1.0e24), "soft": (50.0, 1.0e24), "newton": (2.0e4, 1.0e22)}   # law: (softening, coupling / oracle.G)


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("dim", (3, 2))
def test_against_the_specification(nbx, oracle, dim, law):
    """tests/test_gpu_softening.py's kick-drift-kick case (n = 600 generated bodies, a coupling strong enough to bend the orbits, dt
    around 2) with the steps chosen on the device, against the recorded steps run in fp64 numpy over all pairs (ctx_accel_fn of positions
    rounded to fp32, as the device's are): that test's tolerances, velocities atol = 2e-5 dv, positions rtol = 1e-9."""
    n, steps = 600, 5
    eps, gs = SPEC_CASES[law]
    G = oracle.G * gs
    b0 = oracle.round_inputs_to_f32(oracle.generate(35 + dim, n, dim))
    with context(nbx, b0, law, eps) as c:
        k = accel_length_for(c, G, factor=1.0)                                   # raw = 1 at the start
        clock = c.step_kdk_adaptive(k, 0.25, 2.0, max_steps=steps, G=G)
        a_hist, dt_hist = c.step_history()
        got = downloaded(c, b0)
    assert clock.steps == steps and clock.status == 0
    accel = ctx_accel_fn(G, eps, law)
    ref, prev = b0.copy(), 0.0
    for e, dt in enumerate(dt_hist):
        a = accel(oracle.round_inputs_to_f32(ref))
        if e == steps:
            ref[:, dim:2 * dim] += a * (0.5 * prev)
            break
        ref[:, dim:2 * dim] += a * (0.5 * prev + 0.5 * dt)
        ref[:, :dim] += ref[:, dim:2 * dim] * dt
        prev = dt
    dv = np.abs(ref[:, dim:2 * dim] - b0[:, dim:2 * dim]).max()
    err_v = np.abs(got[:, dim:2 * dim] - ref[:, dim:2 * dim]).max()
    print(f"{dim}D {law}: dt {dt_hist[:-1].min():.4g}..{dt_hist[:-1].max():.4g}, dv {dv:.3e}, largest velocity error {err_v:.3e} = {err_v / dv:.2e} dv")
    assert dv > 1e-3
    assert np.allclose(got[:, dim:2 * dim], ref[:, dim:2 * dim], rtol=0, atol=2e-5 * dv)
    assert np.allclose(got[:, :dim], ref[:, :dim], rtol=1e-9, atol=0)
    assert (dt_hist[:-1] > 0.25).all() and (dt_hist[:-1] < 2.0).all(), "a step on a clamp: the device chose nothing"


# ---- 5: landing on t_end, and the window -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pow2", (False, True))
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("dim", (3, 2))
def test_landing_on_t_end(nbx, dim, law, pow2):
    """t_end = 0.7 with max_steps = 200, far more than needed: the clock stands at t_end bit for bit, finished; only the landing step
    may be below dt_min; evaluations == steps + 1; and bodies, get_forces and history are those of a second run whose max_steps is
    the number of steps taken -- what was queued behind the stop changed nothing."""
    n, t_start, t_end, G = 257, 0.125, 0.7, CLOUD_G[law]
    b0 = shrinking_cloud(n, dim)
    got = {}
    for run in ("long", "exact"):
        with context(nbx, b0, law) as c:
            k = accel_length_for(c, G) / 4.0                                         # raw = 0.2 at the start: several steps to t_end
            cap = 200 if run == "long" else got["long"][0].steps
            clock = c.step_kdk_adaptive(k, 0.02, DT_MAX, t_end=t_end, max_steps=cap, t_start=t_start, pow2=pow2, G=G)
            got[run] = (clock, downloaded(c, b0), c.forces(G), *c.step_history())
    clock, _, _, a_hist, dt_hist = got["long"]
    dts = dt_hist[:-1]
    print(f"{dim}D {law} pow2={pow2}: {clock.steps} steps, dt {dts.min():.4g}..{dts.max():.4g}, landing step {dts[-1]:.4g}")
    assert clock.t == t_end and clock.finished == 1 and clock.status == 0 and 3 <= clock.steps < 200
    assert clock.evaluations == clock.steps + 1 == a_hist.size and dt_hist[-1] == 0.0
    assert (dts[:-1] >= 0.02).all() and dts[-1] > 0 and abs(dts.sum() - (t_end - t_start)) <= 4 * dts.size * np.spacing(t_end)
    other = got["exact"][0]
    assert (other.t, other.steps, other.evaluations, other.finished, other.dt_last, other.a_max_last) == (clock.t, clock.steps, clock.evaluations, 1, clock.dt_last, clock.a_max_last)
    assert all(np.array_equal(x, y) for x, y in zip(got["long"][1:], got["exact"][1:]))


WINDOW_CHILD = r"""
import hashlib, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import nbody_amd as nbx
from test_gpu_ctx_adaptive_step import window_digest
print("digest", window_digest(nbx))
"""


def window_digest(nbx):
    """the landing run of test_landing_on_t_end and a run stopped by max_steps, all laws, D = 3 and 2, as one hash over bodies, forces,
    histories and clocks"""
    h = hashlib.sha256()
    for dim in (3, 2):
        for law in LAWS:
            G = CLOUD_G[law]
            b0 = shrinking_cloud(257, dim)
            for t_end, cap in ((0.7, 200), (INF, 7)):
                with context(nbx, b0, law) as c:
                    k = accel_length_for(c, G) / 4.0
                    clock = c.step_kdk_adaptive(k, 0.02, DT_MAX, t_end=t_end, max_steps=cap, t_start=0.125, G=G)
                    assert clock.finished == (1 if t_end == 0.7 else 0) and clock.steps >= 3
                    for part in (downloaded(c, b0), c.forces(G), *c.step_history()):
                        h.update(np.ascontiguousarray(part).tobytes())
                    h.update(repr((clock.t, clock.dt_last, clock.a_max_last, clock.steps, clock.evaluations, clock.finished, clock.status)).encode())
    return h.hexdigest()


def test_the_results_do_not_depend_on_the_window(nbx):
    """The same runs in child processes with NBODY_HIP_STEP_WINDOW = 1 (the synchronous loop), 2 and 64 (everything queued at once for
    max_steps = 7; 63 evaluations behind the stop for the landing run) and in this process with the library's own window: identical
    bits, clocks and histories."""
    here = window_digest(nbx)
    for w in ("1", "2", "64"):
        p = subprocess.run([sys.executable, "-c", WINDOW_CHILD, ROOT], env=dict(os.environ, NBODY_HIP_STEP_WINDOW=w), capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        assert p.stdout.split("digest ")[1].strip() == here, f"window {w}"


# ---- 6: chained calls against one call -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("law", LAWS)
def test_chained_calls_against_one_call(nbx, law):
    """3 + 3 steps (the second call starting at the first's t) against 6 in one call, n = 257, by the bound derived in
    tests/test_gpu_adaptive_step.py's test of this name, whose argument does not know where the sums come from: the second call's
    opening evaluation sees the positions of the first call's closing one, so sums, a_max and dt are the same bits, and at the joint
    one call makes v + A (0.5 p + 0.5 d) where two make (v + A (0.5 p)) + A (0.5 d).  With u = 2^-53 that is at most 4 u V per component,
    V = max |v| over the run's ends; the K = 3 kicks behind the joint add (4 + K) u V in all, and the drifts carry it into x:
    |dx| <= (4 + K) u V T + K u X over the remaining time T.  Asserted: 2 x those, per body with the largest-component norms."""
    n, dim, K, G = 257, 3, 3, CLOUD_G[law]
    b0 = shrinking_cloud(n, dim)
    u = 2.0 ** -53
    runs = {}
    for name in ("one", "two"):
        with context(nbx, b0, law) as c:
            k = accel_length_for(c, G)
            if name == "one":
                clock = c.step_kdk_adaptive(k, DT_MIN, DT_MAX, max_steps=2 * K, G=G)
                hist = c.step_history()[1][:-1]
            else:
                first = c.step_kdk_adaptive(k, DT_MIN, DT_MAX, max_steps=K, G=G)
                h1 = c.step_history()[1][:-1]
                clock = c.step_kdk_adaptive(k, DT_MIN, DT_MAX, max_steps=K, t_start=first.t, G=G)
                hist = np.concatenate([h1, c.step_history()[1][:-1]])
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
    print(f"{law}: chained against one call: dv / bound {float((dv / bound_v).max()):.3f}, dx / bound {float((dx / bound_x).max()):.3f}, bodies that differ {int((dv > 0).sum())}")
    assert (dv <= bound_v).all() and (dx <= bound_x).all()
    assert np.abs(one[:, v] - b0[:, v]).max() > 1e6 * bound_v.max(), "coupling too weak to test anything"


# ---- 7: the eccentric binary -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra", (0, BIN_EXTRA))
@pytest.mark.parametrize("pow2", (False, True))
@pytest.mark.parametrize("c", BIN_C)
def test_eccentric_binary(nbx, c, pow2, extra):
    """tests/test_adaptive_step_cpu.py's binary, alone (n = 2) and among 256 light distant bodies, under the Newtonian law: one period in
    chained one-step calls with Context.energy at every end.  The adaptive loop's worst |E / E0 - 1| is at least BIN_FACTOR (10) below
    step_kdk's with the same calls, steps and evaluations.  (The specification's figures are that module's docstring's; the certificate
    for this path is tests/test_ctx_adaptive_step_cpu.py's.)"""
    b0 = binary_system(extra)
    n = b0.shape[0]
    worst = {}
    steps = 0
    for scheme in ("adaptive", "fixed"):
        with context(nbx, b0, "newton", BIN_EPS) as ctx:
            e0 = sum(ctx.energy(BIN_G))
            worst[scheme] = 0.0
            if scheme == "adaptive":
                t = 0.0
                while True:
                    clock = ctx.step_kdk_adaptive(c, BIN_DT_MIN, BIN_DT_MAX, t_end=BIN_PERIOD, max_steps=1, t_start=t, pow2=pow2, G=BIN_G)
                    assert clock.status == 0
                    steps += clock.steps
                    t = clock.t
                    worst[scheme] = max(worst[scheme], abs(sum(ctx.energy(BIN_G)) / e0 - 1.0))
                    if clock.finished:
                        break
                    assert steps < 2000
                assert t == BIN_PERIOD
            else:
                for _ in range(steps):
                    ctx.step_kdk(BIN_PERIOD / steps, 1, BIN_G)
                    worst[scheme] = max(worst[scheme], abs(sum(ctx.energy(BIN_G)) / e0 - 1.0))
    print(f"binary n = {n}, c = {c:g}, pow2 = {pow2}: {steps} steps, worst |E/E0 - 1| adaptive {worst['adaptive']:.3e}, fixed {worst['fixed']:.3e}, "
          f"ratio {worst['fixed'] / worst['adaptive']:.1f}")
    assert e0 < 0
    assert BIN_FACTOR * worst["adaptive"] <= worst["fixed"]


# ---- 8: an a_max that is not finite ----------------------------------------------------------------------------------------------------

def test_an_acceleration_that_is_not_finite_stops_the_loop(nbx):
    """One NaN coordinate under the Newtonian law, uploaded: a value, never an index -- pack_kernel converts and compares it (a NaN is no
    close-set candidate and fails the extent test, which picks the two-reciprocal kernel), and the softened fast kernel, which runs no
    close-set pass, addresses its tiles and planes by thread, workgroup and tile numbers alone.  status 1 at the first evaluation, no
    entry in the history, positions and velocities are the uploaded bits, and the context is good for the next call."""
    n, dim, G = 64, 3, CLOUD_G["newton"]
    b0 = shrinking_cloud(n, dim)
    bad = b0.copy()
    bad[n // 2, 1] = np.nan
    with context(nbx, bad, "newton") as c:
        clock = c.step_kdk_adaptive(1.0, DT_MIN, DT_MAX, max_steps=5, G=G)
        a_hist, dt_hist = c.step_history()
        g = downloaded(c, bad)
        assert clock.status == 1 and clock.steps == 0 and clock.evaluations == 1 and clock.finished == 0 and clock.t == 0.0
        assert not np.isfinite(clock.a_max_last) and a_hist.size == 0 and dt_hist.size == 0
        assert not np.isfinite(c.max_accel(G))
        assert np.array_equal(g.view(np.uint64), bad.view(np.uint64))
        c.upload(b0)
        clock = c.step_kdk_adaptive(1.0, DT_MIN, DT_MAX, max_steps=2, G=G)
        assert clock.status == 0 and clock.steps == 2 and c.step_history()[0].size == 3


# ---- 9: refusals and observers ---------------------------------------------------------------------------------------------------------

def test_refusals(nbx):
    """Every refusal of the header with contexts at hand; a refused call launches nothing and leaves no clock."""
    n, dim, G = 64, 3, CLOUD_G["reference"]
    b = shrinking_cloud(n, dim)
    lib = nbx.load_library()
    with nbx.Context(n, dim) as c, nbx.Context(n, dim) as empty, nbx.Context(n, dim, 0, 2, 0) as sharded:
        c.upload(b)
        sharded.upload(b)
        assert status(nbx, lambda: c.max_accel(G)) == NBX_ERR_STATE                  # no accelerations yet
        c.compute_accel()
        good = c.forces(G)
        assert status(nbx, c.step_clock) == NBX_ERR_STATE and status(nbx, c.step_history) == NBX_ERR_STATE

        def call(ctx=c, max_steps=2, **change):
            kw = dict(accel_length=1.0e-3, dt_min=0.01, dt_max=0.1, t_start=0.0, t_end=INF, pow2=0, reserved=0)
            kw.update(change)
            k = nbx.StepControl(**kw)
            return lib.nbx_ctx_step_kdk_adaptive(ctx.h if ctx is not None else None, G, ctypes.byref(k), max_steps)

        for change in (dict(accel_length=0.0), dict(accel_length=INF), dict(accel_length=np.nan), dict(dt_min=0.0), dict(dt_min=0.2), dict(dt_min=np.nan), dict(dt_max=INF),
                       dict(t_start=INF), dict(t_start=np.nan), dict(t_end=np.nan), dict(t_end=-INF), dict(pow2=2), dict(reserved=1)):
            assert call(**change) == NBX_ERR_INVALID, change
        assert call(max_steps=-1) == NBX_ERR_INVALID and call(max_steps=(1 << 20) + 1) == NBX_ERR_INVALID
        assert call(ctx=None) == NBX_ERR_INVALID
        assert lib.nbx_ctx_step_kdk_adaptive(c.h, G, None, 2) == NBX_ERR_INVALID
        assert lib.nbx_ctx_max_accel(c.h, G, None) == NBX_ERR_INVALID and lib.nbx_ctx_max_accel(None, G, None) == NBX_ERR_INVALID
        assert call(ctx=empty) == NBX_ERR_STATE                                      # nothing uploaded
        assert call(ctx=sharded) == NBX_ERR_STATE                                    # n_shards != 1
        c.set_law(nbx.FORCE_LAW_NEWTON)
        assert call() == NBX_ERR_STATE                                               # what compute_accel refuses: no softening length
        c.set_law(nbx.FORCE_LAW_REFERENCE)
        assert status(nbx, c.step_clock) == NBX_ERR_STATE, "a refused call leaves no clock"
        c.compute_accel()
        assert np.array_equal(c.forces(G), good) and np.array_equal(downloaded(c, b), b)
        assert call(max_steps=0) == 0 and np.array_equal(downloaded(c, b), b)        # does nothing
        assert status(nbx, c.step_clock) == NBX_ERR_STATE
        assert call() == 0
        assert c.step_clock().steps == 2 and not np.array_equal(downloaded(c, b)[:, :dim], b[:, :dim])
        count = ctypes.c_size_t(0)
        one_a, one_dt = np.full(2, -1.0), np.full(2, -1.0)
        assert lib.nbx_ctx_get_step_history(c.h, one_a.ctypes.data, one_dt.ctypes.data, 1, ctypes.byref(count)) == 0
        assert count.value == 3 and one_a[0] > 0 and one_dt[0] > 0 and one_a[1] == -1.0 and one_dt[1] == -1.0, "capacity bounds what is written"
        assert lib.nbx_ctx_get_step_history(c.h, None, None, 0, None) == NBX_ERR_INVALID and lib.nbx_ctx_get_step_clock(c.h, None) == NBX_ERR_INVALID


@pytest.mark.parametrize("law", LAWS)
def test_observers_and_the_fixed_step_loops_afterwards(nbx, law):
    """max_accel, energy and step_clock between two adaptive calls change no later bit; and after an adaptive call step_kdk and step
    on that context give the bits of a fresh context uploaded with the downloaded state."""
    n, dim, G = 257, 3, CLOUD_G[law]
    b0 = shrinking_cloud(n, dim)
    ends = []
    for observe in (False, True):
        with context(nbx, b0, law) as c:
            k = accel_length_for(c, G)
            first = c.step_kdk_adaptive(k, DT_MIN, DT_MAX, max_steps=3, G=G)
            if observe:
                c.energy(G)
                assert c.max_accel(G) == first.a_max_last
                assert c.step_clock().t == first.t
            second = c.step_kdk_adaptive(k, DT_MIN, DT_MAX, max_steps=3, t_start=first.t, pow2=True, G=G)
            middle = downloaded(c, b0)
            c.step_kdk(0.01, 2, G)
            after_kdk = downloaded(c, b0)
            c.step(0.01, 2, G)
            ends.append((second.t, middle, after_kdk, downloaded(c, b0), *c.step_history()))
    assert ends[0][0] == ends[1][0] and all(np.array_equal(x, y) for x, y in zip(ends[0][1:], ends[1][1:]))
    with context(nbx, ends[0][1], law) as fresh:                                     # fp64 bodies in: the fp32 copies are rounded from them as the drift does
        fresh.step_kdk(0.01, 2, G)
        assert np.array_equal(downloaded(fresh, b0), ends[0][2])
        fresh.step(0.01, 2, G)
        assert np.array_equal(downloaded(fresh, b0), ends[0][3])


# ---- 10: the harness -------------------------------------------------------------------------------------------------------------------

def test_harness_runs_the_all_pairs_loop_with_steps_chosen_on_the_device(tmp_path):
    """nbody_sim -N 4096 -m g --init plummer --law newton --softening 2048 --integrator kdka --accel-length 4 --dt 1 --dt-min 0.01
    --steps 8 --energy-every 4: the row carries `_kdka`, one `Adaptive steps: 8 taken` line gives t and the range of dt within
    [dt_min, dt], and the energy lines at 0, 4, 8 carry t.  The same command without the new options prints the fixed-step loop's row and
    lines and no word of this."""
    sim = os.path.join(ROOT, "nbody_sim")
    assert os.path.exists(sim)
    common = ["-N", "4096", "-m", "g", "--init", "plummer", "--seed", "5", "--G", "0.1", "--law", "newton", "--softening", "2048", "--steps", "8", "--energy-every", "4", "--dt", "1"]

    def run(name, extra):
        cwd = tmp_path / name
        cwd.mkdir()
        p = subprocess.run([sim] + common + extra, cwd=cwd, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        found = [os.path.join(d, f_) for d, _, files in os.walk(cwd) for f_ in files if f_.endswith(".csv")]
        return p.stdout, [line.split(",")[0] for path in sorted(found) for line in open(path) if line.startswith("Leapfrog_HIP")]

    plain_out, plain_rows = run("kdk", ["--integrator", "kdk"])
    out, rows = run("kdka", ["--integrator", "kdka", "--accel-length", "4", "--dt-min", "0.01"])
    assert plain_rows == ["Leapfrog_HIP_8steps"] and rows == ["Leapfrog_HIP_8steps_kdka"], (plain_rows, rows)
    assert "kdka" not in plain_out and "Adaptive steps" not in plain_out and "chosen on the device" not in plain_out and "  t = " not in plain_out
    summary = [line for line in out.splitlines() if line.startswith("Adaptive steps: ")]
    assert len(summary) == 1 and len(out.splitlines()) == len(plain_out.splitlines()) + 1, out
    line = summary[0]
    assert line.startswith("Adaptive steps: 8 taken, t = "), line
    t = float(line.split("t = ")[1].split(",")[0])
    lo, hi = (float(x) for x in line.split(", dt ")[1].split(",")[0].split(" .. "))
    assert 0.01 <= lo <= hi <= 1.0 and 8 * lo <= t * (1 + 1e-9) and t <= 8 * hi * (1 + 1e-9), line
    energy = [x for x in out.splitlines() if x.startswith("step ")]
    assert [x.split()[1] for x in energy] == ["0", "4", "8"] and all("E = " in x for x in energy), out
    ts = [float(x.split("  t = ")[1]) for x in energy[1:]]
    assert 0 < ts[0] < ts[1] == pytest.approx(t, rel=1e-9)
    for x in energy:
        assert float(x.split("E = ")[1].split()[0]) < 0, x
        if not x.startswith("step 0 "):
            assert float(x.split("|dE/E0| = ")[1].split()[0]) < 1e-2 and "2K/|U| " in x, x
    assert out.count("steps chosen on the device") == 1
