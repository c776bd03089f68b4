"""GPU: softened Newtonian gravity on a leaf plan (NBX_LAW_NEWTON with nbx_leaf_plan_set_softening; csrc/leaf_plan_api.hip, csrc/leaf_pair_kernel.hip,
csrc/leaf_far_kernel.hip) through the C ABI.

References.  The near field on complete structures is judged against the project's all-pairs checker of the context's Newtonian law,
oracle.force_rows_softened(newton=True), with assert_force_parity.  Everything else is judged against the law's fp64 specification in
nbody_amd.leaves: near_sums for the leaf sums, far_sums(law="newton") for the far cells at either order.

Every softening length here is a power of two, so eps^2 is exact in fp32 and the device's rho^2 = r^2 + eps^2 is the specification's
up to the rounding of the sum.

Tolerance of the far-field tests: TOL_BACKWARD_SMALL_N S_i + E_i, the form of tests/test_gpu_far_quadrupole.py, re-derived for this law.
  S_i = G |m_i| [ sum_j |m_j| r / rho^3  (near_sums' magnitude sums)  +  sum_c M_c R / rho^3  +  sum_c |C_c| ]: every term is made and
  summed in fp32.
  E_i, what the specification does not contain, is the rounding of a cell's record to fp32.  The pseudo-body: f(R) = R / rho^3 has the
  Jacobian I / rho^3 - 3 R R^T / rho^5, of norm <= (1 + 3) / rho^3 (r <= rho), so a centre of mass moved by
  eps_c = sqrt(D) 2^-23 |com_c|_inf changes the term by at most 4 M_c eps_c / rho^3.  The correction
      C_c = M_c [ -(3/2) t R / rho^5 + (15/2) R (R^T q R) / rho^7 - 3 q R / rho^5 ],   t = tr(q), q positive semi-definite (masses >= 0):
      (3/2) t R / rho^5              has a derivative bounded by  (3/2) (1 + 5) t / rho^5      =  9 t / rho^5,
      (15/2) R (R^T q R) / rho^7     by                           (15/2) (1 + 2 + 7) t / rho^5 = 75 t / rho^5,
      3 q R / rho^5                  by                           3 (1 + 5) t / rho^5          = 18 t / rho^5,
  102 M_c t eps_c / rho^5 together; C_c is linear in q, whose entries and trace are rounded to fp32 (u = 2^-24 + 2^-40, as there):
  M_c (3/2 + 15/2 + 3) u t r / rho^5 <= 12 M_c t u / rho^4.  So
      E_i = G |m_i| sum_c M_c [ 4 eps_c / rho^3 + t_c (102 eps_c / rho^5 + 12 u / rho^4) ]      (the second part at order 1 only),
  which is the issue's derivation, confirmed term by term.
"""
import contextlib
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle_lib import KAPPA_WELL, TOL_BACKWARD_SMALL_N, TOL_REL, assert_force_parity
from test_gpu_leaf_plan_device import _structure

pytestmark = pytest.mark.gpu
NBX_ERR_INVALID, NBX_ERR_STATE = 1, 5
EPS = 32768.0                       # 2^15 on the generator's 1e7 box: far below a leaf's side, eps^2 exact in fp32
U_Q = 2.0 ** -24 + 2.0 ** -40
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((3, 3, 0.5), (3, 4, 0.7), (2, 4, 0.5))


@contextlib.contextmanager
def planner(which):
    before = os.environ.get("NBODY_HIP_LEAF_PLANNER")
    os.environ["NBODY_HIP_LEAF_PLANNER"] = which
    try:
        yield
    finally:
        if before is None:
            del os.environ["NBODY_HIP_LEAF_PLANNER"]
        else:
            os.environ["NBODY_HIP_LEAF_PLANNER"] = before


def through_both_planners(nbx, b, dim, leaves, G, eps=EPS):
    """plan.forces under the new law through the host and the device planner: the same bits; (forces, info of the layout)."""
    f, info = None, None
    for which in ("host", "device"):
        with planner(which), nbx.LeafPlan(b.shape[0], dim, *leaves) as plan:
            assert plan.softening == 0.0
            plan.set_softening(eps)
            assert plan.softening == eps
            got = plan.forces(b, nbx.LAW_NEWTON, G)
            if f is None:
                f, info = got, plan.info()
            assert np.array_equal(got, f), f"{which} planner"
            assert plan.info() == info
    return f, info


# ---- the near field -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _checker_case(oracle, dim):
    """6,000 generated bodies with one coincident pair, and the all-pairs checker's forces and magnitude sums: once per dimension."""
    b = oracle.round_inputs_to_f32(oracle.generate(90 + dim, 6000, dim))
    b[11, :dim] = b[10, :dim]
    b = np.ascontiguousarray(b)
    ref, S = oracle.force_rows_softened(b, EPS, newton=True)
    return b, ref, S


@pytest.mark.parametrize("leaf_size", (32, 8, 4, 3))
@pytest.mark.parametrize("dim", (3, 2))
def test_near_field_against_the_checker(nbx, oracle, dim, leaf_size):
    """Every leaf on every list: the leaf sums are the all-pairs sums of the context's Newtonian law.  32-body leaves run one leaf per
    two-wave workgroup, 8-body leaves the packed waves, 4- and 3-body leaves the packed class whose lane pairs share their loads
    through DPP (3: an odd leaf, every leaf ends in a pad).  The coincident pair and every body with itself add exactly 0."""
    b, ref, S = _checker_case(oracle, dim)
    f, info = through_both_planners(nbx, b, dim, nbx.leaves.all_pairs_leaves(6000, leaf_size), oracle.G)
    print(f"D={dim} leaves of {leaf_size}: layout (slots, runs, workgroups, waves) = {info}")
    e = assert_force_parity(f, ref, S, f"all pairs through leaves of {leaf_size}, D={dim}")
    print(f"D={dim} leaves of {leaf_size}: {e}")


def _ragged_cases():
    """tests/test_gpu_leaf_plan_device.py::test_ragged_structures_word_for_word's shapes, drawn in its order from its generator (seed 9)
    and built with its structure seeds (100 + the case's index there), so that they are those structures word for word; and one more
    with every packed width."""
    rng = np.random.default_rng(9)
    cases = {
        "tiny_mixed": (100, rng.integers(0, 12, 3000).tolist(), lambda t: [3, 9, 27, 0, 14][t % 5]),     # every packed class, empty leaves, empty lists
        "fmm_sized": (101, rng.integers(1, 90, 500).tolist(), lambda t: [5, 40, 1][t % 3]),              # two-wave workgroups, cut pieces
        "long_lists": (103, rng.integers(1, 9, 400).tolist(), lambda t: [70, 130, 40][t % 3]),           # > 32 runs: one-leaf workgroups next to packed waves
        "big_leaves": (104, rng.integers(100, 300, 60).tolist(), lambda t: 7),                           # several workgroups per leaf
    }
    # mostly small leaves (the mean stays below 8), some of up to 31 bodies
    cases["wide_mixed"] = (310, rng.choice([0, 1, 2, 3, 5, 7, 13, 15, 16, 25, 31], 2500, p=[.05, .1, .15, .2, .2, .1, .05, .05, .04, .03, .03]).tolist(),
                           lambda t: [5, 11, 2, 0][t % 4])
    return cases


@pytest.mark.parametrize("dim", (3, 2))
@pytest.mark.parametrize("shape", ("tiny_mixed", "fmm_sized", "long_lists", "big_leaves", "wide_mixed"))
def test_ragged_structures(nbx, oracle, dim, shape):
    """Structures of mixed leaf sizes (packed waves of every width, one-leaf workgroups beside them in one fused launch, two-wave
    workgroups with cut pieces, leaves split over several workgroups, odd-sized and empty leaves, empty lists, repeated list entries)
    against near_sums: |dF_i| <= TOL_BACKWARD_SMALL_N G |m_i| S_i; bodies in no leaf and targets without sources get exact zeros."""
    seed, sizes, list_len = _ragged_cases()[shape]
    leaves, n = _structure(seed, sizes, list_len)
    b = oracle.round_inputs_to_f32(oracle.generate(95 + dim, n, dim))
    f, info = through_both_planners(nbx, b, dim, leaves, oracle.G)
    sums, S = nbx.leaves.near_sums(b, dim, *leaves, EPS)
    gm = oracle.G * b[:, -1]
    ref, S = gm[:, None] * sums, np.abs(gm) * S
    assert np.isfinite(f).all()
    in_leaf = np.zeros(n, dtype=bool)
    in_leaf[np.asarray(leaves[1])] = True
    assert (~in_leaf).sum() >= 11 and not f[~in_leaf].any(), "bodies in no leaf get exact zeros"
    assert not f[S == 0].any(), "targets without sources get exact zeros"
    live = S > 0
    err = np.sqrt(((f - ref) ** 2).sum(axis=1))
    worst = float((err[live] / S[live]).max())
    print(f"{shape} D={dim}: layout {info}, {int(live.sum())} live targets, backward error {worst:.2e} (bound {TOL_BACKWARD_SMALL_N:.0e})")
    assert (err[live] <= TOL_BACKWARD_SMALL_N * S[live]).all(), f"{shape}: backward error {worst:.3e}"


# ---- the far field ------------------------------------------------------------------------------------------------------------

def octree(nbx, b, dim, depth, theta):
    r = nbx.leaves.octree_cells(b, dim, depth, theta)
    return r[:4], r[4:6], r[6:8]


def newton_far_terms(nbx, b, dim, leaves, far, mom, eps):
    """Per body and per unit G |m_i|: the far sums at order 0 and the corrections' sum (vectors), their magnitude sums, and the two
    parts of E_i of the module docstring."""
    mass, com, Q = mom
    assert (b[:, -1] >= 0.0).all(), "the bound assumes a positive semi-definite q"
    lo, lb = np.asarray(leaves[0], dtype=np.int64), np.asarray(leaves[1], dtype=np.int64)
    fo, fc = np.asarray(far[0], dtype=np.int64), np.asarray(far[1], dtype=np.int64)
    eps_c = np.sqrt(dim) * 2.0 ** -23 * np.abs(com).max(axis=1)
    t = Q[:, :dim].sum(axis=1) / np.where(mass != 0.0, mass, 1.0)
    n = b.shape[0]
    F0, C, S0, SC, E0, E1 = np.zeros((n, dim)), np.zeros((n, dim)), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for tl in range(lo.size - 1):
        ids, c = lb[lo[tl]:lo[tl + 1]], fc[fo[tl]:fo[tl + 1]]
        c = c[mass[c] != 0.0]
        if not ids.size or not c.size:
            continue
        R = com[None, c, :] - b[ids, None, :dim]
        r2 = (R * R).sum(axis=2)
        rho2 = r2 + eps * eps
        rho3 = rho2 * np.sqrt(rho2)
        F0[ids] = ((mass[c] / rho3)[..., None] * R).sum(axis=1)
        S0[ids] = (mass[c] * np.sqrt(r2) / rho3).sum(axis=1)
        corr = nbx.leaves.far_correction(R, mass[None, c], Q[None, c, :], law="newton", eps=eps)
        C[ids] = corr.sum(axis=1)
        SC[ids] = np.sqrt((corr * corr).sum(axis=2)).sum(axis=1)
        E0[ids] = (4.0 * mass[c] * eps_c[c] / rho3).sum(axis=1)
        E1[ids] = (mass[c] * t[c] * (102.0 * eps_c[c] / (rho3 * rho2) + 12.0 * U_Q / rho2 ** 2)).sum(axis=1)
    return F0, C, S0, SC, E0, E1


@functools.lru_cache(maxsize=None)
def _far_case(nbx, oracle, dim, depth, theta):
    """20,000 generated bodies, their octree, and the specification's near and far terms: once per shape."""
    b = oracle.round_inputs_to_f32(oracle.generate(50 + dim, 20000, dim))
    leaves, cells, far = octree(nbx, b, dim, depth, theta)
    mom = nbx.leaves.cell_moments(b, dim, leaves[0], leaves[1], *cells)
    near, S_near = nbx.leaves.near_sums(b, dim, *leaves, EPS)
    F0, C, S0, SC, E0, E1 = newton_far_terms(nbx, b, dim, leaves, far, mom, EPS)
    # far_sums is the specification the issue names; newton_far_terms restates it for the bound's sake: they must agree
    for order, want in ((0, F0), (1, F0 + C)):
        spec = nbx.leaves.far_sums(b, dim, leaves[0], leaves[1], *cells, *far, order=order, moments=mom, law="newton", eps=EPS)
        assert (np.abs(spec - want).max(axis=1) <= 1e-13 * (S0 + SC)).all()      # the same terms, summed in another order
    return b, leaves, cells, far, dict(near=near, S_near=S_near, F0=F0, C=C, S0=S0, SC=SC, E0=E0, E1=E1)


def assert_far_parity(f, ref, S, E, what):
    """tests/test_gpu_far_quadrupole.py's assert_far_parity."""
    assert f.shape == ref.shape and np.isfinite(f).all(), what
    dF = np.sqrt(((f - ref) ** 2).sum(axis=1))
    nF = np.sqrt((ref ** 2).sum(axis=1))
    live = S > 0
    assert not f[~live].any(), f"{what}: bodies without any counted pair must get exactly zero"
    worst = float((dF[live] / (TOL_BACKWARD_SMALL_N * S[live] + E[live])).max()) if live.any() else 0.0
    print(f"{what}: backward error / bound = {worst:.3f}, largest E_i / S_i = {float((E[live] / S[live]).max()) if live.any() else 0.0:.2e}")
    assert (dF[live] <= TOL_BACKWARD_SMALL_N * S[live] + E[live]).all(), f"{what}: backward error {worst:.2f} x the bound"
    well = live & (nF > 0) & (S <= KAPPA_WELL * nF)
    if well.any():
        rel = dF[well] / nF[well]
        assert (rel <= TOL_REL + E[well] / nF[well]).all(), f"{what}: relative error {float(rel.max()):.3e} on well-conditioned bodies"


@pytest.mark.parametrize("order", (0, 1))
@pytest.mark.parametrize("dim,depth,theta", SHAPES)
def test_far_field_against_the_specification(nbx, oracle, dim, depth, theta, order):
    """Near + far at orders 0 and 1 on the octree of 20,000 generated bodies against near_sums + far_sums(law="newton"), bound
    TOL_BACKWARD_SMALL_N S_i + E_i (module docstring).  At order 1 the correction itself must be far above the tolerance, or the test
    shows nothing."""
    b, leaves, cells, far, T = _far_case(nbx, oracle, dim, depth, theta)
    n, G = b.shape[0], oracle.G
    with nbx.LeafPlan(n, dim, *leaves) as plan:
        plan.set_softening(EPS)
        plan.set_cells(*cells, *far)
        plan.set_far_order(order)
        f = plan.forces(b, nbx.LAW_NEWTON, G)
    gm = G * b[:, -1]
    ref = gm[:, None] * (T["near"] + T["F0"] + (T["C"] if order else 0.0))
    S = np.abs(gm) * (T["S_near"] + T["S0"] + (T["SC"] if order else 0.0))
    E = np.abs(gm) * (T["E0"] + (T["E1"] if order else 0.0))
    what = f"Newton order {order}, octree depth {depth} theta {theta} D={dim}"
    assert_far_parity(f, ref, S, E, what)
    if order:
        size = np.sqrt(((gm[:, None] * T["C"]) ** 2).sum(axis=1)) / np.sqrt((f ** 2).sum(axis=1))
        print(f"{what}: median |correction| / |F| = {float(np.median(size)):.2e}")
        assert np.median(size) > 10 * TOL_BACKWARD_SMALL_N


def test_every_way_in_gives_the_same_bits(nbx, oracle):
    """Order 1 under the new law through host bodies, resident bodies, and sums left on the device followed by get_forces; the
    softening length set before set_cells and set_far_order (host planner) and after both (device planner): the same bits."""
    dim, depth, theta = SHAPES[0]
    b, leaves, cells, far, _ = _far_case(nbx, oracle, dim, depth, theta)
    n, G, f = b.shape[0], oracle.G, None
    for which in ("host", "device"):
        with planner(which), nbx.LeafPlan(n, dim, *leaves) as plan:
            if which == "host":
                plan.set_softening(EPS)
            plan.set_cells(*cells, *far)
            plan.set_far_order(nbx.FAR_QUADRUPOLE)
            if which == "device":
                plan.set_softening(EPS)
            assert plan.softening == EPS and plan.far_order == 1
            got = plan.forces(b, nbx.LAW_NEWTON, G)
            if f is None:
                f = got
            assert np.array_equal(got, f), f"host bodies, {which} planner"
            with nbx.Context(n, dim) as c:
                c.upload(b)
                assert np.array_equal(plan.forces_ctx(c, nbx.LAW_NEWTON, G), f), f"resident bodies, {which} planner"
                plan.forces_ctx(c, nbx.LAW_NEWTON, G, fetch=False)
                assert np.array_equal(plan.get_forces(), f), f"sums left on the device, {which} planner"
            plan.set_cells(*cells, *far)                              # the cells again: the softening length is the plan's
            assert plan.softening == EPS
            assert np.array_equal(plan.forces(b, nbx.LAW_NEWTON, G), f), f"after set_cells, {which} planner"
            # another softening length gives other forces, and the first one gives the first ones again
            plan.set_softening(2.0 * EPS)
            assert not np.array_equal(plan.forces(b, nbx.LAW_NEWTON, G), f)
            plan.set_softening(EPS)
            assert np.array_equal(plan.forces(b, nbx.LAW_NEWTON, G), f)


def test_the_reference_laws_are_untouched(nbx, oracle):
    """Laws 0, 1 and 2 at orders 0 and 1: a plan with a softening length set and a plan never told give the same bits."""
    dim, depth, theta = SHAPES[0]
    b, leaves, cells, far, _ = _far_case(nbx, oracle, dim, depth, theta)
    n = b.shape[0]
    with nbx.LeafPlan(n, dim, *leaves) as told, nbx.LeafPlan(n, dim, *leaves) as never:
        told.set_softening(EPS)
        for p in (told, never):
            p.set_cells(*cells, *far)
        for order in (0, 1):
            told.set_far_order(order)
            never.set_far_order(order)
            for law in (nbx.LAW_BRUTE, nbx.LAW_TREE_LEAF, nbx.LAW_FMM_P2P):
                want = never.forces(b, law, oracle.G)
                assert want.any()
                assert np.array_equal(told.forces(b, law, oracle.G), want), (law, order)
        assert never.softening == 0.0


# ---- trees built on the device --------------------------------------------------------------------------------------------------

def test_device_trees(nbx, oracle):
    """from_octree on generated bodies and from_octree_adaptive (capacity 16) on a 20,000-body Plummer sphere under the new law, at
    both orders: the bits of a plan made from the same eight arrays on the host; the adaptive tree's forces are also held to
    near_sums + far_sums(law="newton") on that structure, bound TOL_BACKWARD_SMALL_N S_i + E_i (module docstring)."""
    n, dim, G = 20000, 3, 0.1
    cases = (("from_octree", oracle.round_inputs_to_f32(oracle.generate(53, n, dim)), lambda c: nbx.LeafPlan.from_octree(c, 4, 0.5)),
             ("from_octree_adaptive", oracle.round_inputs_to_f32(np.ascontiguousarray(nbx.plummer_bodies(n, dim, seed=3, G=G))),
              lambda c: nbx.LeafPlan.from_octree_adaptive(c, 10, 16, 0.5)))
    for what, b, make in cases:
        with nbx.Context(n, dim) as c:
            c.upload(b)
            with make(c) as plan:
                plan.set_softening(2048.0)
                f0 = plan.forces_ctx(c, nbx.LAW_NEWTON, G)
                plan.set_far_order(nbx.FAR_QUADRUPOLE)
                f1 = plan.forces_ctx(c, nbx.LAW_NEWTON, G)
                arrays = plan.structure()
            assert np.isfinite(f1).all() and not np.array_equal(f0, f1), what
            with nbx.LeafPlan(n, dim, *arrays[:4]) as ref:
                ref.set_cells(*arrays[4:])
                ref.set_softening(2048.0)
                assert np.array_equal(ref.forces_ctx(c, nbx.LAW_NEWTON, G), f0), f"{what}: order 0 on the host arrays"
                ref.set_far_order(nbx.FAR_QUADRUPOLE)
                assert np.array_equal(ref.forces_ctx(c, nbx.LAW_NEWTON, G), f1), f"{what}: order 1 on the host arrays"
                assert np.array_equal(ref.forces(b, nbx.LAW_NEWTON, G), f1), f"{what}: host bodies"
        if what == "from_octree_adaptive":
            # ... and the adaptive tree's forces against the specification on the structure the device built
            eps = 2048.0
            leaves, cells, far = arrays[:4], arrays[4:6], arrays[6:8]
            mom = nbx.leaves.cell_moments(b, dim, leaves[0], leaves[1], *cells)
            near, S_near = nbx.leaves.near_sums(b, dim, *leaves, eps)
            F0, C, S0, SC, E0, E1 = newton_far_terms(nbx, b, dim, leaves, far, mom, eps)
            gm = G * b[:, -1]
            for order, f in ((0, f0), (1, f1)):
                spec = nbx.leaves.far_sums(b, dim, leaves[0], leaves[1], *cells, *far, order=order, moments=mom, law="newton", eps=eps)
                assert (np.abs(spec - (F0 + order * C)).max(axis=1) <= 1e-13 * (S0 + SC)).all()
                assert_far_parity(f, gm[:, None] * (near + spec), np.abs(gm) * (S_near + S0 + order * SC), np.abs(gm) * (E0 + order * E1),
                                  f"adaptive tree (capacity 16) on a Plummer sphere, Newton order {order}")


def test_stepping(nbx, oracle):
    """step_octree(LAW_NEWTON) for 3 steps, rebuilding every step, equals rebuild + forces_ctx + kick_drift bit for bit, and the
    softening length survives the rebuilds.  One step agrees with the oracle's update_body_velocities / update_body_positions fed the
    specification's forces: per-body velocity bound 1.25 (TOL_BACKWARD_SMALL_N S_i + E_i) dt / m_i, positions to that bound x dt (the
    form of tests/test_gpu_far_field.py's stepping test)."""
    n, dim, depth, theta, dt, steps = 20000, 3, 3, 0.5, 1.5, 3
    b0, leaves, cells, far, T = _far_case(nbx, oracle, dim, depth, theta)
    G = oracle.G * 1e24
    ga, gb, g1 = b0.copy(), b0.copy(), b0.copy()
    with nbx.Context(n, dim) as ca, nbx.Context(n, dim) as cb, nbx.Context(n, dim) as c1:
        for c in (ca, cb, c1):
            c.upload(b0)
        with nbx.LeafPlan.from_octree(ca, depth, theta) as pa, nbx.LeafPlan.from_octree(cb, depth, theta) as pb, \
                nbx.LeafPlan.from_octree(c1, depth, theta) as p1:
            for p in (pa, pb, p1):
                p.set_far_order(nbx.FAR_QUADRUPOLE)
                p.set_softening(EPS)
            for _ in range(steps):
                pa.rebuild(ca)
                assert pa.softening == EPS
                pa.forces_ctx(ca, nbx.LAW_NEWTON, G, fetch=False)
                pa.kick_drift(ca, dt)
            pb.step_octree(cb, nbx.LAW_NEWTON, G, dt, steps, 1)
            assert pb.softening == EPS and pb.far_order == 1
            ca.download(ga); cb.download(gb)
            assert np.array_equal(ga, gb), f"bodies after {steps} steps"
            assert np.array_equal(pa.get_forces(), pb.get_forces())
            assert not np.array_equal(ga[:, dim:2 * dim], b0[:, dim:2 * dim]), "coupling too weak to test anything"
            assert np.array_equal(p1.structure()[0], np.asarray(leaves[0])), "the device tree is the specification's"
            p1.step_octree(c1, nbx.LAW_NEWTON, G, dt, 1, 1)
            c1.download(g1)
    gm = G * b0[:, -1]
    f = np.ascontiguousarray(gm[:, None] * (T["near"] + T["F0"] + T["C"]))
    allowed = np.abs(gm) * (TOL_BACKWARD_SMALL_N * (T["S_near"] + T["S0"] + T["SC"]) + T["E0"] + T["E1"])
    ref = b0.copy()
    oracle.update_body_velocities(ref, f, dt)
    oracle.update_body_positions(ref, dt)
    v = slice(dim, 2 * dim)
    bound = 1.25 * allowed / b0[:, -1] * dt
    err = np.linalg.norm(g1[:, v] - ref[:, v], axis=1)
    moved = np.linalg.norm(ref[:, v] - b0[:, v], axis=1)
    print(f"one Newtonian step: velocity error / bound = {float((err / bound).max()):.3f}, median |dv| / bound = {float(np.median(moved / bound)):.1e}")
    assert np.median(moved / bound) > 100.0, "coupling too weak to test anything"
    assert (err <= bound).all(), f"velocity error {float((err / bound).max()):.2f} x the per-body bound"
    assert np.allclose(g1[:, :dim], ref[:, :dim], rtol=1e-9, atol=dt * float(bound.max()))
    assert np.array_equal(g1[:, -1], b0[:, -1])


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals(nbx, oracle):
    """Newton without a softening length is NBX_ERR_STATE from every evaluation; softening lengths outside {0} U [1e-6, 1e15] are
    NBX_ERR_INVALID and leave the plan's value alone; a mass of 1e8 with eps = 1e15 is refused at evaluation (m / eps^3 underflows),
    from host bodies and from a context alike; the one-shot call refuses law 3."""
    n, dim = 64, 3
    b = oracle.round_inputs_to_f32(oracle.generate(7, n, dim))
    leaves = nbx.leaves.all_pairs_leaves(n, 8)

    def status(call):
        with pytest.raises(nbx.NbxError) as e:
            call()
        return e.value.status

    with nbx.LeafPlan(n, dim, *leaves) as plan, nbx.Context(n, dim) as c:
        c.upload(b)
        good = plan.forces(b, nbx.LAW_TREE_LEAF, oracle.G)
        assert status(lambda: plan.forces(b, nbx.LAW_NEWTON, oracle.G)) == NBX_ERR_STATE
        assert status(lambda: plan.forces_ctx(c, nbx.LAW_NEWTON, oracle.G)) == NBX_ERR_STATE
        assert status(lambda: plan.step(c, nbx.LAW_NEWTON, oracle.G, 1.0, 1)) == NBX_ERR_STATE
        assert status(lambda: plan.step_octree(c, nbx.LAW_NEWTON, oracle.G, 1.0, 1, 0)) == NBX_ERR_STATE
        assert status(lambda: plan.time_kernel(nbx.LAW_NEWTON, 2)) == NBX_ERR_STATE
        assert status(lambda: plan.forces(b, 4, oracle.G)) == NBX_ERR_INVALID
        assert np.array_equal(plan.get_forces(), good), "a refused evaluation launches nothing"
        plan.set_softening(64.0)
        for bad in (1.0e-7, 1.0e16, -1.0, float("nan"), float("inf")):
            assert status(lambda: plan.set_softening(bad)) == NBX_ERR_INVALID
            assert plan.softening == 64.0
        ok = plan.forces(b, nbx.LAW_NEWTON, oracle.G)
        assert np.isfinite(ok).all() and ok.any()
        assert plan.time_kernel(nbx.LAW_NEWTON, 2) >= 0.0
        # m / eps^3 = 1e8 / 1e45 underflows fp32's normal range
        heavy = b.copy()
        heavy[:, -1] = 1.0e6
        heavy[3, -1] = 1.0e8
        plan.set_softening(1.0e15)
        assert status(lambda: plan.forces(heavy, nbx.LAW_NEWTON, oracle.G)) == NBX_ERR_INVALID
        c.upload(heavy)
        assert status(lambda: plan.forces_ctx(c, nbx.LAW_NEWTON, oracle.G)) == NBX_ERR_INVALID
        assert status(lambda: plan.step(c, nbx.LAW_NEWTON, oracle.G, 1.0, 1)) == NBX_ERR_INVALID
        # ... and overflows it at the other end of the range
        plan.set_softening(1.0e-6)
        heavy[3, -1] = 1.0e21
        assert status(lambda: plan.forces(heavy, nbx.LAW_NEWTON, oracle.G)) == NBX_ERR_INVALID
        plan.set_softening(0.0)
        assert plan.softening == 0.0
        assert status(lambda: plan.forces(b, nbx.LAW_NEWTON, oracle.G)) == NBX_ERR_STATE
        assert np.array_equal(plan.forces(b, nbx.LAW_TREE_LEAF, oracle.G), good)
    assert status(lambda: nbx.leaf_pair_forces_hip(b, *leaves, law=nbx.LAW_NEWTON, G=oracle.G)) == NBX_ERR_INVALID


# ---- a Plummer sphere in equilibrium through the tree -----------------------------------------------------------------------------

def test_plummer_sphere_stays_in_equilibrium_through_the_tree(nbx):
    """tests/test_gpu_softening.py's Newtonian Plummer sphere through the adaptive tree: N = 32,768, a = 1e5, M = 1e12, G = 0.1
    (t_dyn = 100), eps = 2048, dt = 0.5, adaptive octree (max depth 10, capacity 32, theta 0.5, order 1) rebuilt every step, 200 steps =
    one dynamical time; the energy is the context's (nbx_ctx_energy under the Newtonian law), every 50 steps.  E0 < 0, 2K/|U| within
    0.9..1.1 and the half-mass radius within 5 %: the bounds of the brute-force test.  |dE/E0| <= 1e-2 is a cap against gross failure,
    not a measurement: a wrong sign or a dropped far pass moves E by order 1, force errors of ~1e-4 acting coherently for a dynamical
    time by ~1e-3 at worst.  The same steps run on a brute-force context; both drifts are printed (profiles/r12/newton_tree.txt)."""
    n, G, dt, eps, a = 32768, 0.1, 0.5, 2048.0, 1.0e5
    b = nbx.plummer_bodies(n, 3, seed=5, a=a, total_mass=1.0e12, G=G)
    r_half0 = np.median(np.linalg.norm(b[:, :3] - 5.0e6, axis=1))
    drift = {}
    with nbx.Context(n, 3) as c, nbx.Context(n, 3) as brute:
        for ctx in (c, brute):
            ctx.upload(b)
            ctx.set_softening(eps)                                  # on the tree's context: for nbx_ctx_energy only
            ctx.set_law(nbx.FORCE_LAW_NEWTON)
        ke0, pe0 = c.energy(G)
        e0 = ke0 + pe0
        assert brute.energy(G) == (ke0, pe0)
        virial = [2 * ke0 / abs(pe0)]
        drift["tree"], drift["brute"] = 0.0, 0.0
        with nbx.LeafPlan.from_octree_adaptive(c, 10, 32, 0.5) as plan:
            plan.set_far_order(nbx.FAR_QUADRUPOLE)
            plan.set_softening(eps)
            for _ in range(4):
                plan.step_octree(c, nbx.LAW_NEWTON, G, dt, 50, 1)
                ke, pe = c.energy(G)
                drift["tree"] = max(drift["tree"], abs(ke + pe - e0) / abs(e0))
                virial.append(2 * ke / abs(pe))
                brute.step(dt, 50, G)
                kb, pb = brute.energy(G)
                drift["brute"] = max(drift["brute"], abs(kb + pb - e0) / abs(e0))
            assert plan.softening == eps and plan.far_order == 1
        cur = b.copy()
        c.download(cur)
    r_half1 = np.median(np.linalg.norm(cur[:, :3] - 5.0e6, axis=1))
    print(f"\nNewtonian Plummer through the tree N={n}: E0 = {e0:.4e}, max |dE/E0| over t_dyn: tree {drift['tree']:.3e}, brute force "
          f"{drift['brute']:.3e}; virial 2K/|U| {min(virial):.3f}..{max(virial):.3f}, half-mass radius {r_half0:.0f} -> {r_half1:.0f}")
    assert e0 < 0
    assert 0.9 < min(virial) and max(virial) < 1.1
    assert abs(r_half1 - r_half0) < 0.05 * r_half0
    assert drift["tree"] <= 1e-2


# ---- the C++ layer and the harness --------------------------------------------------------------------------------------------

def test_cpp_layer_and_harness(tmp_path):
    """nbody_sim -m t --law newton --softening 2048 on a 20,000-body Plummer sphere through the adaptive tree (host/leaf_pairs_hip.cpp's
    Newtonian calls and BarnesHutNewtonHip): the reference-law rows at both orders are there and their CSV is byte for byte that of a
    run without the two flags, apart from the time column; behind them the BarnesHut_HIP_adaptive_newton and ..._newton_quad rows, the
    second with the smaller median error against the all-pairs forces of the same law; and the step loop's energy lines."""
    sim = os.path.join(ROOT, "nbody_sim")
    assert os.path.exists(sim)
    common = ["-N", "20000", "-m", "t", "-a", "1", "--init", "plummer", "--G", "0.1", "--far-order", "1", "--leaf-cap", "32", "--steps", "4",
              "--energy-every", "2"]

    def run(name, extra):
        cwd = tmp_path / name
        cwd.mkdir()
        p = subprocess.run([sim] + common + extra, cwd=cwd, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        found = [os.path.join(d, f_) for d, _, files in os.walk(cwd) for f_ in files if f_.endswith(".csv")]
        rows = [line.rstrip("\n").split(",") for path in sorted(found) for line in open(path) if line.startswith("BarnesHut_HIP")]
        return p.stdout, rows, p.stderr

    def without_time(rows):
        return [",".join(r[:3] + r[4:]) for r in rows]

    plain_out, plain_rows, _ = run("plain", [])
    out, rows, err_text = run("newton", ["--law", "newton", "--softening", "2048"])
    reference_law = [r for r in rows if "newton" not in r[0]]
    assert {"BarnesHut_HIP_adaptive", "BarnesHut_HIP_adaptive_quad"} <= {r[0] for r in reference_law}, out
    assert all("newton" not in r[0] for r in plain_rows) and "Newtonian" not in plain_out
    assert without_time(reference_law) == without_time(plain_rows), "the reference-law rows must not notice the two flags"
    names = [r[0] for r in rows if "newton" in r[0] and not r[0].endswith("_steps")]
    assert names == ["BarnesHut_HIP_adaptive_newton", "BarnesHut_HIP_adaptive_newton_quad"], out + err_text
    err = [[float(v.split()[-1]) for v in line.split(":")[1].split(",")] for line in out.splitlines() if line.startswith("Newtonian relative force error")]
    print(f"\nnbody_sim --law newton through the tree: relative error (median, p99) at orders 0 and 1: {err}")
    assert len(err) == 2 and err[1][0] < err[0][0], "the _quad row must be the more accurate one"
    start = out.index("softened Newtonian law")
    energy = [line for line in out[start:].splitlines() if line.startswith("step ")]
    assert len(energy) == 6 and all("E = " in line for line in energy), out                   # steps 0, 2, 4 at each order
    assert all("|dE/E0| = " in line and "2K/|U| " in line for line in energy if not line.startswith("step 0 ")), out + err_text
