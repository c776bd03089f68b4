"""GPU: kick-drift-kick through a leaf plan -- nbx_leaf_plan_kick_drift2, _step_kdk, _step_octree_kdk and _max_accel
(csrc/state_kernels.hip: kick_drift_slots_kernel, slot_accel_max_kernel; csrc/leaf_plan_api.hip) through the C ABI.

Inputs, unless a test says otherwise, are those of tests/test_gpu_newton_tree.py::test_stepping: 20,000 generated bodies, an octree of
depth 3 at theta 0.5 built on the device, far order 1, EPS = 32768, G = oracle.G * 1e24, dt = 1.5.  What is judged bit for bit is
judged with np.array_equal; the one comparison with the oracle's helpers takes over test_stepping's per-body bound; the order of
convergence is judged against leaves.leapfrog_spec on the system tests/test_leapfrog_spec_cpu.py chose on the CPU."""
import os
import subprocess

import numpy as np
import pytest

from oracle_lib import TOL_BACKWARD_SMALL_N
from test_gpu_newton_tree import EPS, _far_case
from test_leapfrog_spec_cpu import KDK_DT, KDK_EPS, KDK_G, KDK_N, KDK_STEPS, all_pairs_accel, kdk_system, position_error

pytestmark = pytest.mark.gpu
NBX_ERR_INVALID, NBX_ERR_STATE = 1, 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, DEPTH, THETA, DT = 20000, 3, 0.5, 1.5


def status(nbx, call):
    with pytest.raises(nbx.NbxError) as e:
        call()
    return e.value.status


def bodies_of(oracle, dim, n=N):
    """_far_case's bodies (the same generator call), without its specification terms"""
    return oracle.round_inputs_to_f32(oracle.generate(50 + dim, n, dim))


def newton_octree(nbx, c, depth=DEPTH, capacity=0):
    p = nbx.LeafPlan.from_octree_adaptive(c, 10, capacity, THETA) if capacity else nbx.LeafPlan.from_octree(c, depth, THETA)
    p.set_far_order(nbx.FAR_QUADRUPOLE)
    p.set_softening(EPS)
    return p


def downloaded(c, like):
    out = like.copy()
    c.download(out)
    return out


# ---- 1: equal steps give the existing kernel's bits -----------------------------------------------------------------------------

@pytest.mark.parametrize("law", ("newton", "tree_leaf"))
@pytest.mark.parametrize("n", (N, 257, 1))
def test_equal_steps_give_the_bits_of_kick_drift(nbx, oracle, n, law):
    """kick_drift2(dt, dt) against kick_drift(dt), two contexts and two plans: the same bodies bit for bit.  N = 257 and N = 1 are the
    tile edges of the 256-lane grid (one lane in the second workgroup; one lane in all)."""
    dim = 3
    b0 = bodies_of(oracle, dim, n)
    code = nbx.LAW_NEWTON if law == "newton" else nbx.LAW_TREE_LEAF
    G = oracle.G * (1e24 if law == "newton" else 1e26)
    def make(c):                                                   # the octree at N = 20,000; below, leaves of 64 with every leaf on every list
        if n == N:
            return newton_octree(nbx, c)
        p = nbx.LeafPlan(n, dim, *nbx.leaves.all_pairs_leaves(n, 64))
        p.set_softening(EPS)
        return p

    with nbx.Context(n, dim) as ca, nbx.Context(n, dim) as cb:
        ca.upload(b0); cb.upload(b0)
        with make(ca) as pa, make(cb) as pb:
            for _ in range(2):                                    # the second round starts from moved bodies
                pa.forces_ctx(ca, code, G, fetch=False)
                pa.kick_drift(ca, DT)
                pb.forces_ctx(cb, code, G, fetch=False)
                pb.kick_drift2(cb, DT, DT)
            ga, gb = downloaded(ca, b0), downloaded(cb, b0)
    assert np.array_equal(ga, gb)
    assert not np.array_equal(ga[:, :dim], b0[:, :dim])
    if n > 1:
        assert not np.array_equal(ga[:, dim:2 * dim], b0[:, dim:2 * dim]), "coupling too weak to test anything"


@pytest.mark.parametrize("n", (257, 1))
def test_a_zero_step_of_kick_drift_changes_nothing(nbx, oracle, n):
    """kick_drift(0) runs the drifting kernel like every other step (it reads and writes the positions): the bodies downloaded are
    the uploaded bits, and a following kick_drift2(dt, dt) gives the bits of the same call on a second plan and context that
    skipped the zero step."""
    dim = 3
    b0 = bodies_of(oracle, dim, n)
    G = oracle.G * 1e26
    with nbx.Context(n, dim) as ca, nbx.Context(n, dim) as cb:
        ca.upload(b0); cb.upload(b0)
        with nbx.LeafPlan(n, dim, *nbx.leaves.all_pairs_leaves(n, 64)) as pa, nbx.LeafPlan(n, dim, *nbx.leaves.all_pairs_leaves(n, 64)) as pb:
            pa.forces_ctx(ca, nbx.LAW_TREE_LEAF, G, fetch=False)
            pa.kick_drift(ca, 0.0)
            assert np.array_equal(downloaded(ca, b0), b0)
            pa.kick_drift2(ca, DT, DT)
            pb.forces_ctx(cb, nbx.LAW_TREE_LEAF, G, fetch=False)
            pb.kick_drift2(cb, DT, DT)
            ga, gb = downloaded(ca, b0), downloaded(cb, b0)
    assert np.array_equal(ga, gb)
    assert not np.array_equal(ga[:, :dim], b0[:, :dim])


# ---- 2: unequal steps against the oracle's helpers ------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", (3, 2))
def test_unequal_steps_against_the_oracle(nbx, oracle, dim):
    """kick_drift2(0.75, 1.5) against oracle.update_body_velocities(f, 0.75) then update_body_positions(1.5) fed the specification's
    forces: test_stepping's per-body velocity bound 1.25 (TOL_BACKWARD_SMALL_N S_i + E_i) dt_kick / m_i, positions to that bound x
    dt_drift; the median |dv| is more than 100 x the bound."""
    dk, dd = 0.75, 1.5
    b0, leaves, cells, far, T = _far_case(nbx, oracle, dim, DEPTH, THETA)
    G = oracle.G * 1e24
    with nbx.Context(N, dim) as c:
        c.upload(b0)
        with newton_octree(nbx, c) as p:
            assert np.array_equal(p.structure()[0], np.asarray(leaves[0])), "the device tree is the specification's"
            p.forces_ctx(c, nbx.LAW_NEWTON, G, fetch=False)
            p.kick_drift2(c, dk, dd)
            g = downloaded(c, b0)
    gm = G * b0[:, -1]
    f = np.ascontiguousarray(gm[:, None] * (T["near"] + T["F0"] + T["C"]))
    allowed = np.abs(gm) * (TOL_BACKWARD_SMALL_N * (T["S_near"] + T["S0"] + T["SC"]) + T["E0"] + T["E1"])
    ref = b0.copy()
    oracle.update_body_velocities(ref, f, dk)
    oracle.update_body_positions(ref, dd)
    v = slice(dim, 2 * dim)
    bound = 1.25 * allowed / b0[:, -1] * dk
    err = np.linalg.norm(g[:, v] - ref[:, v], axis=1)
    moved = np.linalg.norm(ref[:, v] - b0[:, v], axis=1)
    print(f"kick_drift2({dk}, {dd}) in {dim}D: velocity error / bound = {float((err / bound).max()):.3f}, median |dv| / bound = {float(np.median(moved / bound)):.1e}")
    assert np.median(moved / bound) > 100.0, "coupling too weak to test anything"
    assert (err <= bound).all(), f"velocity error {float((err / bound).max()):.2f} x the per-body bound"
    assert np.allclose(g[:, :dim], ref[:, :dim], rtol=1e-9, atol=dd * float(bound.max()))
    # the drift used dt_drift, not dt_kick: a drift by 0.75 would be off by |v| 0.75
    assert not np.allclose(g[:, :dim], b0[:, :dim] + ref[:, v] * dk, rtol=1e-9, atol=dd * float(bound.max()))
    assert np.array_equal(g[:, -1], b0[:, -1])


# ---- 3: the pure kick -----------------------------------------------------------------------------------------------------------

def test_a_pure_kick_touches_no_position(nbx, oracle):
    """kick_drift2(dt, 0): the downloaded positions are the uploaded bits, the velocities moved; the next forces_ctx gives the previous
    evaluation's bits and the octree stands unchanged; the context's own accelerations stay valid (its bodies have not moved) --
    until a real drift."""
    dim = 3
    b0 = bodies_of(oracle, dim)
    G = oracle.G * 1e24
    with nbx.Context(N, dim) as c:
        c.upload(b0)
        c.compute_accel()
        fa = c.forces(G)
        with newton_octree(nbx, c) as p:
            s0 = p.structure()
            f0 = p.forces_ctx(c, nbx.LAW_NEWTON, G)
            p.kick_drift2(c, DT, 0.0)
            g = downloaded(c, b0)
            assert np.array_equal(g[:, :dim], b0[:, :dim]) and np.array_equal(g[:, -1], b0[:, -1])
            assert not np.array_equal(g[:, dim:2 * dim], b0[:, dim:2 * dim])
            assert np.array_equal(c.forces(G), fa), "the context's accelerations survive a pure kick"
            assert np.array_equal(p.get_forces(), f0)
            assert np.array_equal(p.forces_ctx(c, nbx.LAW_NEWTON, G), f0)
            assert all(np.array_equal(x, y) for x, y in zip(p.structure(), s0))
            p.kick_drift2(c, DT, DT)                                # a real drift does invalidate the context's own accelerations
            assert status(nbx, lambda: c.forces(G)) == NBX_ERR_STATE
            assert not np.array_equal(downloaded(c, b0)[:, :dim], b0[:, :dim])


# ---- 4: bodies in no leaf ---------------------------------------------------------------------------------------------------------

def _with_bodies_left_out(nbx, b, dim, left_out=37):
    lo, lb, so, ss = nbx.leaves.uniform_grid_leaves(b, dim, 2)
    keep = lo[-1] - left_out                                       # the last slots' bodies end up in no leaf
    return (np.minimum(lo, keep), lb[:keep], so, ss), np.setdiff1d(np.arange(b.shape[0]), lb[:keep])


def test_bodies_in_no_leaf_only_drift(nbx, oracle):
    """A hand-made structure that leaves 37 bodies out: under kick_drift2(0.75, 1.5) they move by exactly v * 1.5 and their velocities
    keep their bits; the others are kicked."""
    dim, dk, dd = 3, 0.75, 1.5
    b0 = bodies_of(oracle, dim)
    leaves, out = _with_bodies_left_out(nbx, b0, dim)
    assert out.size == 37
    with nbx.LeafPlan(N, dim, *leaves) as p, nbx.Context(N, dim) as c:
        c.upload(b0)
        p.forces_ctx(c, nbx.LAW_TREE_LEAF, oracle.G * 1e26, fetch=False)
        p.kick_drift2(c, dk, dd)
        g = downloaded(c, b0)
    v = slice(dim, 2 * dim)
    assert np.array_equal(g[out, v], b0[out, v])
    assert np.array_equal(g[out, :dim], b0[out, :dim] + b0[out, v] * dd)
    inside = np.setdiff1d(np.arange(N), out)
    assert (np.abs(g[inside, v] - b0[inside, v]).max(axis=1) > 0).mean() > 0.99, "coupling too weak to test anything"
    assert np.array_equal(g[inside, :dim], b0[inside, :dim] + g[inside, v] * dd)


# ---- 5, 6: the step loops against the calls spelled out -----------------------------------------------------------------------------

def _spelled_out(nbx, p, c, G, dt, nsteps, rebuild_every):
    """F K(dt/2) D(dt) [F K(dt) D(dt)]^(n-1) F K(dt/2) from forces_ctx / kick_drift2, a rebuild before evaluation e when asked for"""
    for e in range(nsteps + 1):
        if rebuild_every > 0 and e % rebuild_every == 0:
            p.rebuild(c)
        p.forces_ctx(c, nbx.LAW_NEWTON, G, fetch=False)
        p.kick_drift2(c, 0.5 * dt if e in (0, nsteps) else dt, dt if e < nsteps else 0.0)


@pytest.mark.parametrize("dim", (3, 2))
def test_step_kdk_equals_the_sequence_spelled_out(nbx, oracle, dim):
    """step_kdk(dt, 3) against forces_ctx(fetch=False) / kick_drift2 spelled out: bodies and get_forces() bit for bit; nsteps = 0
    does nothing."""
    b0 = bodies_of(oracle, dim)
    G = oracle.G * 1e24
    with nbx.Context(N, dim) as ca, nbx.Context(N, dim) as cb:
        ca.upload(b0); cb.upload(b0)
        with newton_octree(nbx, ca) as pa, newton_octree(nbx, cb) as pb:
            pb.step_kdk(cb, nbx.LAW_NEWTON, G, DT, 0)
            assert np.array_equal(downloaded(cb, b0), b0)
            _spelled_out(nbx, pa, ca, G, DT, 3, 0)
            pb.step_kdk(cb, nbx.LAW_NEWTON, G, DT, 3)
            ga, gb = downloaded(ca, b0), downloaded(cb, b0)
            assert np.array_equal(ga, gb)
            assert np.array_equal(pa.get_forces(), pb.get_forces())
            assert not np.array_equal(ga[:, dim:2 * dim], b0[:, dim:2 * dim]) and not np.array_equal(ga[:, :dim], b0[:, :dim])
            # the plan holds the sums of the final positions: a fresh evaluation of the context as it stands gives the same forces
            assert np.array_equal(pb.forces_ctx(cb, nbx.LAW_NEWTON, G), pa.get_forces())


@pytest.mark.parametrize("capacity", (0, 32))
def test_step_octree_kdk_equals_the_sequence_spelled_out(nbx, oracle, capacity):
    """step_octree_kdk(dt, 3, 1) and (dt, 4, 2) against rebuild + forces_ctx + kick_drift2 spelled out, on the fixed tree and on the
    adaptive one (capacity 32); softening and far order survive; rebuild_every = 0 equals step_kdk."""
    dim = 3
    b0 = bodies_of(oracle, dim)
    G = oracle.G * 1e24
    for nsteps, every in ((3, 1), (4, 2), (3, 0)):
        with nbx.Context(N, dim) as ca, nbx.Context(N, dim) as cb:
            ca.upload(b0); cb.upload(b0)
            with newton_octree(nbx, ca, capacity=capacity) as pa, newton_octree(nbx, cb, capacity=capacity) as pb:
                if every:
                    _spelled_out(nbx, pa, ca, G, DT, nsteps, every)
                else:
                    pa.step_kdk(ca, nbx.LAW_NEWTON, G, DT, nsteps)
                pb.step_octree_kdk(cb, nbx.LAW_NEWTON, G, DT, nsteps, every)
                assert pb.softening == EPS and pb.far_order == 1
                ga, gb = downloaded(ca, b0), downloaded(cb, b0)
                assert np.array_equal(ga, gb), f"bodies after step_octree_kdk(dt, {nsteps}, {every})"
                assert np.array_equal(pa.get_forces(), pb.get_forces())
                assert all(np.array_equal(x, y) for x, y in zip(pa.structure(), pb.structure()))
                assert not np.array_equal(ga[:, dim:2 * dim], b0[:, dim:2 * dim])


# ---- 7: the order of convergence on the device ---------------------------------------------------------------------------------------

def test_order_of_convergence_on_the_device(nbx):
    """tests/test_leapfrog_spec_cpu.py's system through a plan with every leaf on every list (all pairs direct: only the fp32 pair terms
    differ from the specification).  step_kdk and step at dt and dt/2 against the fp64 specification at dt/64: the error ratio is > 3
    for kick-drift-kick and < 2.6 for kick-drift, the midpoints between the first- and second-order values; and the kick-drift-kick
    error at dt/2 is at least 100 x the device-against-specification difference at equal dt, so fp32 noise decides nothing."""
    b0 = kdk_system()
    accel = all_pairs_accel(KDK_G, KDK_EPS)
    ref = nbx.leaves.leapfrog_spec(b0, accel, KDK_DT / 64, KDK_STEPS * 64, "kdk")
    err, dev = {}, {}
    with nbx.LeafPlan(KDK_N, 3, *nbx.leaves.all_pairs_leaves(KDK_N, 16)) as p:
        p.set_softening(KDK_EPS)
        for scheme in ("kdk", "kd"):
            for halvings in (0, 1):
                dt, nsteps = KDK_DT / 2 ** halvings, KDK_STEPS * 2 ** halvings
                with nbx.Context(KDK_N, 3) as c:
                    c.upload(b0)
                    (p.step_kdk if scheme == "kdk" else p.step)(c, nbx.LAW_NEWTON, KDK_G, dt, nsteps)
                    dev[scheme, halvings] = downloaded(c, b0)
                err[scheme, halvings] = position_error(dev[scheme, halvings], ref)
    noise = position_error(dev["kdk", 1], nbx.leaves.leapfrog_spec(b0, accel, KDK_DT / 2, KDK_STEPS * 2, "kdk"))
    print(f"position errors against the specification at dt/64: kdk {err['kdk', 0]:.3e} (dt) {err['kdk', 1]:.3e} (dt/2), kd {err['kd', 0]:.3e} (dt) "
          f"{err['kd', 1]:.3e} (dt/2); device against specification at dt/2: {noise:.3e}")
    assert err["kdk", 0] / err["kdk", 1] > 3.0
    assert err["kd", 0] / err["kd", 1] < 2.6
    assert err["kdk", 1] >= 100.0 * noise


# ---- 8: reversal on the device ---------------------------------------------------------------------------------------------------------

def test_reversal_on_the_device(nbx, oracle):
    """On a standing structure step_kdk(dt, n) then step_kdk(-dt, n) returns at least 1000 x closer to the start than step(dt, n);
    step(-dt, n), relative to the distance travelled."""
    dim, n = 3, 4
    b0 = bodies_of(oracle, dim)
    G = oracle.G * 1e24
    back = {}
    for scheme in ("kdk", "kd"):
        with nbx.Context(N, dim) as c:
            c.upload(b0)
            with newton_octree(nbx, c) as p:
                step = p.step_kdk if scheme == "kdk" else p.step
                step(c, nbx.LAW_NEWTON, G, DT, n)
                there = downloaded(c, b0)
                step(c, nbx.LAW_NEWTON, G, -DT, n)
                again = downloaded(c, b0)
        travelled = np.linalg.norm(there[:, :dim] - b0[:, :dim], axis=1).max()
        back[scheme] = float(np.linalg.norm(again[:, :dim] - b0[:, :dim], axis=1).max() / travelled)
        assert travelled > 0
    print(f"return distance / distance travelled after {n} + {n} steps: kdk {back['kdk']:.3e}, kd {back['kd']:.3e}, ratio {back['kd'] / max(back['kdk'], 1e-300):.3e}")
    assert 1000.0 * back["kdk"] <= back["kd"]


# ---- 9: the largest acceleration -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", (3, 2))
def test_max_accel(nbx, oracle, dim):
    """max_accel() is max_i |F_i| / m_i of get_forces() to 1e-12 relative, also after a step_kdk (the sums are the final positions');
    NBX_ERR_STATE before any evaluation; an observer: get_forces() and a following kick_drift give the bits they would have given."""
    b0 = bodies_of(oracle, dim)
    G = oracle.G * 1e24
    assert (b0[:, -1] > 0).all()

    def from_forces(f):
        return float((np.linalg.norm(f, axis=1) / b0[:, -1]).max())

    with nbx.Context(N, dim) as ca, nbx.Context(N, dim) as cb:
        ca.upload(b0); cb.upload(b0)
        with newton_octree(nbx, ca) as pa, newton_octree(nbx, cb) as pb:
            assert status(nbx, pa.max_accel) == NBX_ERR_STATE
            fa = pa.forces_ctx(ca, nbx.LAW_NEWTON, G)
            pb.forces_ctx(cb, nbx.LAW_NEWTON, G, fetch=False)
            a = pa.max_accel()
            assert a > 0 and abs(a - from_forces(fa)) <= 1e-12 * a
            assert pa.max_accel() == a
            assert np.array_equal(pa.get_forces(), fa)
            pa.kick_drift(ca, DT)
            pb.kick_drift(cb, DT)
            assert np.array_equal(downloaded(ca, b0), downloaded(cb, b0)), "max_accel must not change what kick_drift does"
            pa.step_kdk(ca, nbx.LAW_NEWTON, G, DT, 2)
            a2 = pa.max_accel()
            assert a2 != a and abs(a2 - from_forces(pa.get_forces())) <= 1e-12 * a2
            pa.rebuild(ca)
            assert status(nbx, pa.max_accel) == NBX_ERR_STATE, "a rebuilt plan holds no evaluation"


def test_max_accel_leaves_out_bodies_in_no_leaf(nbx, oracle):
    """On a hand-made structure that leaves 37 bodies out (their slot is 0xffffffff: the kernel must not follow it) the maximum is the
    one over the bodies in leaves."""
    dim = 3
    b0 = bodies_of(oracle, dim)
    leaves, out = _with_bodies_left_out(nbx, b0, dim)
    G = oracle.G * 1e26
    with nbx.LeafPlan(N, dim, *leaves) as p, nbx.Context(N, dim) as c:
        c.upload(b0)
        f = p.forces_ctx(c, nbx.LAW_TREE_LEAF, G)
        a = p.max_accel()
    assert not f[out].any()
    inside = np.setdiff1d(np.arange(N), out)
    want = float((np.linalg.norm(f[inside], axis=1) / b0[inside, -1]).max())
    assert a > 0 and abs(a - want) <= 1e-12 * a


# ---- 10: refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals(nbx, oracle):
    """Newton without a softening length is NBX_ERR_STATE from both step calls and launches nothing; negative counts are
    NBX_ERR_INVALID; rebuilding steps on a plan not built from an octree are NBX_ERR_STATE; kick_drift2 before any evaluation, or with
    another context than the evaluation's, is NBX_ERR_STATE."""
    n, dim = 64, 3
    b = oracle.round_inputs_to_f32(oracle.generate(7, n, dim))
    leaves = nbx.leaves.all_pairs_leaves(n, 8)
    with nbx.LeafPlan(n, dim, *leaves) as plan, nbx.Context(n, dim) as c, nbx.Context(n, dim) as other:
        c.upload(b); other.upload(b)
        assert status(nbx, lambda: plan.kick_drift2(c, 1.0, 1.0)) == NBX_ERR_STATE
        good = plan.forces_ctx(c, nbx.LAW_TREE_LEAF, oracle.G)
        assert status(nbx, lambda: plan.step_kdk(c, nbx.LAW_NEWTON, oracle.G, 1.0, 1)) == NBX_ERR_STATE
        assert status(nbx, lambda: plan.step_octree_kdk(c, nbx.LAW_NEWTON, oracle.G, 1.0, 1, 0)) == NBX_ERR_STATE
        assert np.array_equal(plan.get_forces(), good), "a refused step launches nothing"
        assert np.array_equal(downloaded(c, b), b)
        assert status(nbx, lambda: plan.step_kdk(c, nbx.LAW_TREE_LEAF, oracle.G, 1.0, -1)) == NBX_ERR_INVALID
        assert status(nbx, lambda: plan.step_octree_kdk(c, nbx.LAW_TREE_LEAF, oracle.G, 1.0, -1, 0)) == NBX_ERR_INVALID
        assert status(nbx, lambda: plan.step_octree_kdk(c, nbx.LAW_TREE_LEAF, oracle.G, 1.0, 1, -1)) == NBX_ERR_INVALID
        assert status(nbx, lambda: plan.step_kdk(c, 4, oracle.G, 1.0, 1)) == NBX_ERR_INVALID
        assert status(nbx, lambda: plan.step_octree_kdk(c, nbx.LAW_TREE_LEAF, oracle.G, 1.0, 1, 1)) == NBX_ERR_STATE
        assert status(nbx, lambda: plan.kick_drift2(other, 1.0, 1.0)) == NBX_ERR_STATE
        assert np.array_equal(plan.get_forces(), good) and np.array_equal(downloaded(c, b), b) and np.array_equal(downloaded(other, b), b)
        plan.step_octree_kdk(c, nbx.LAW_TREE_LEAF, oracle.G, 1.0, 1, 0)          # without rebuilds any plan will do
        assert not np.array_equal(downloaded(c, b)[:, :dim], b[:, :dim])


# ---- 11: a Plummer sphere in equilibrium ---------------------------------------------------------------------------------------------

def test_plummer_sphere_stays_in_equilibrium_under_kick_drift_kick(nbx):
    """tests/test_gpu_newton_tree.py's Plummer sphere (N = 32,768, a = 1e5, M = 1e12, G = 0.1, eps = 2048, dt = 0.5, adaptive octree of
    capacity 32 at theta 0.5 and order 1, rebuilt before every evaluation, 200 steps = one dynamical time) under step_octree_kdk, with
    that test's caps: E0 < 0, 2K/|U| within 0.9..1.1, the half-mass radius within 5 %, |dE/E0| <= 1e-2 -- caps against gross failure,
    not measurements.  The drifts of both integrators are printed, by the context's all-pairs energy and by the plan's own; neither
    is asserted to be the smaller: at this dt the tree's force error may dominate both."""
    n, G, dt, eps, a = 32768, 0.1, 0.5, 2048.0, 1.0e5
    b = nbx.plummer_bodies(n, 3, seed=5, a=a, total_mass=1.0e12, G=G)
    r_half0 = np.median(np.linalg.norm(b[:, :3] - 5.0e6, axis=1))
    drift, virial, r_half1 = {}, {}, {}
    for scheme in ("kdk", "kd"):
        with nbx.Context(n, 3) as c:
            c.upload(b)
            c.set_softening(eps)                                    # for nbx_ctx_energy only
            c.set_law(nbx.FORCE_LAW_NEWTON)
            ke0, pe0 = c.energy(G)
            e0 = ke0 + pe0
            virial[scheme] = [2 * ke0 / abs(pe0)]
            drift[scheme, "all pairs"] = drift[scheme, "tree"] = 0.0
            with nbx.LeafPlan.from_octree_adaptive(c, 10, 32, 0.5) as plan:
                plan.set_far_order(nbx.FAR_QUADRUPOLE)
                plan.set_softening(eps)
                kt0, pt0 = plan.energy(c, nbx.LAW_NEWTON, G)
                for _ in range(4):
                    (plan.step_octree_kdk if scheme == "kdk" else plan.step_octree)(c, nbx.LAW_NEWTON, G, dt, 50, 1)
                    ke, pe = c.energy(G)
                    kt, pt = plan.energy(c, nbx.LAW_NEWTON, G)
                    drift[scheme, "all pairs"] = max(drift[scheme, "all pairs"], abs(ke + pe - e0) / abs(e0))
                    drift[scheme, "tree"] = max(drift[scheme, "tree"], abs(kt + pt - kt0 - pt0) / abs(kt0 + pt0))
                    virial[scheme].append(2 * ke / abs(pe))
            r_half1[scheme] = np.median(np.linalg.norm(downloaded(c, b)[:, :3] - 5.0e6, axis=1))
    print(f"\nNewtonian Plummer through the tree N={n}, dt={dt}: E0 = {e0:.4e}; max |dE/E0| over t_dyn by the all-pairs energy: kdk "
          f"{drift['kdk', 'all pairs']:.3e}, kd {drift['kd', 'all pairs']:.3e}; by the tree's energy: kdk {drift['kdk', 'tree']:.3e}, kd {drift['kd', 'tree']:.3e}; "
          f"kdk virial 2K/|U| {min(virial['kdk']):.3f}..{max(virial['kdk']):.3f}, half-mass radius {r_half0:.0f} -> {r_half1['kdk']:.0f}")
    assert e0 < 0
    assert 0.9 < min(virial["kdk"]) and max(virial["kdk"]) < 1.1
    assert abs(r_half1["kdk"] - r_half0) < 0.05 * r_half0
    assert drift["kdk", "all pairs"] <= 1e-2


# ---- 12: the harness -------------------------------------------------------------------------------------------------------------------

def test_harness_runs_the_tree_under_kick_drift_kick(tmp_path):
    """nbody_sim -m t --law newton --integrator kdk --steps 8 --energy-every 4 on the 20,000-body Plummer sphere of
    tests/test_gpu_newton_tree.py's harness test: every step row carries `_kdk` and no other row does, and the energy lines parse.  The
    same command without --integrator prints the rows and as many lines as it always has: the names below are the parent's."""
    sim = os.path.join(ROOT, "nbody_sim")
    assert os.path.exists(sim)
    common = ["-N", "20000", "-m", "t", "--init", "plummer", "--G", "0.1", "--far-order", "1", "--leaf-cap", "32", "--law", "newton", "--softening", "2048",
              "--steps", "8", "--energy-every", "4"]

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
    out, rows = run("kdk", ["--integrator", "kdk"])
    assert plain_rows == parents, plain_rows
    assert "kdk" not in plain_out and "kick-drift-kick" not in plain_out
    assert rows == [r + "_kdk" if "_steps" in r else r for r in parents], rows
    assert len(out.splitlines()) == len(plain_out.splitlines())
    start = out.index("softened Newtonian law")
    energy = [line for line in out[start:].splitlines() if line.startswith("step ")]
    assert len(energy) == 6 and all("E = " in line for line in energy), out                    # steps 0, 4, 8 at each order
    for line in energy:
        e = float(line.split("E = ")[1].split()[0])
        assert e < 0, line
        if not line.startswith("step 0 "):
            assert float(line.split("|dE/E0| = ")[1].split()[0]) < 1e-2 and "2K/|U| " in line, line
    assert out.count("(kick-drift-kick)") == 4
