"""GPU: the potential through a leaf plan (nbx_leaf_plan_potentials, _energy, _get_potentials; csrc/leaf_phi_kernel.hip,
csrc/leaf_plan_api.hip) through the C ABI.

Reference: the fp64 specification in nbody_amd.leaves (near_potentials, far_potentials, far_potential_correction), which
tests/test_tree_potential_cpu.py ties to the laws' force terms, to an exact cluster potential and to a direct all-pairs sum.  Totals are
also held against code that shares nothing with it: the oracle's energy and the context's all-pairs nbx_ctx_energy.

Every softening length here is a power of two, so eps^2 is exact in fp32.

Per-body bound, per unit G m_i:  |dphi_i| <= TOL_BACKWARD_SMALL_N S_i + E_i.
  S_i is the sum of the magnitudes of every term of phi_i (near pairs, cells' monopoles, cells' corrections): each is made and summed
  in fp32, at most 248 of them between flushes into fp64.
  E_i is what the specification does not contain, the rounding of a cell's record to fp32.  With eps_c = sqrt(D) 2^-23 |com_c|_inf (how
  far the fp32 centre of mass can lie from the fp64 one) and u = 2^-24 + 2^-40 (the rounding of q's entries and trace):
    monopole.   NEWTON: grad (1 / rho) = R / rho^3, of norm r / rho^3 <= 1 / rho^2.  Reference: grad (1 / (2 r^2)) = R / r^4, norm 1 / r^3.
    correction, NEWTON: C = M [ -t / (2 rho^3) + (3/2) R^T q R / rho^5 ], t = tr q, q positive semi-definite (masses >= 0), |q R| <= t r:
                |grad t / (2 rho^3)| = (3/2) t r / rho^5 <= (3/2) t / rho^4;
                |grad (3/2) R^T q R / rho^5| <= (3/2) [ 2 |q R| / rho^5 + 5 R^T q R r / rho^7 ] <= (3 + 15/2) t / rho^4:   12 t / rho^4 together.
                linear in q: |C| <= M t (1/2 + 3/2) / rho^3, so rounding q costs 2 u M t / rho^3.
    correction, reference: C = M [ -t / (2 r^4) + 2 R^T q R / r^6 ]:
                |grad t / (2 r^4)| = 2 t / r^5;  |grad 2 R^T q R / r^6| <= 2 [ 2 t / r^5 + 6 t / r^5 ] = (4 + 12) t / r^5:   18 t / r^5 together.
                linear in q: |C| <= M t (1/2 + 2) / r^4, so rounding q costs 2.5 u M t / r^4.
      NEWTON:     E_i = sum_c M_c [ eps_c / rho^2 + t_c (12 eps_c / rho^4 + 2 u / rho^3) ]
      reference:  E_i = sum_c M_c [ eps_c / r^3   + t_c (18 eps_c / r^5   + 2.5 u / r^4) ]      (the t_c part at order 1 only)
  which is the issue's derivation, confirmed term by term.
Totals: |dU| <= (G / 2) sum_i |m_i| (TOL_BACKWARD_SMALL_N S_i + E_i).
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from oracle_lib import TOL_BACKWARD_SMALL_N
from test_gpu_leaf_plan_device import _structure
from test_gpu_newton_tree import SHAPES, _ragged_cases, octree, planner

pytestmark = pytest.mark.gpu
NBX_ERR_INVALID, NBX_ERR_STATE = 1, 5
EPS = 32768.0                       # 2^15 on the generator's 1e7 box
EPS_SMALL = 2.0 ** -6               # the self-term test: m_i / eps dwarfs the rest of phi_i
U_Q = 2.0 ** -24 + 2.0 ** -40
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAWS = ("newton", "brute", "tree_leaf")


def law_id(nbx, law):
    return {"newton": nbx.LAW_NEWTON, "brute": nbx.LAW_BRUTE, "tree_leaf": nbx.LAW_TREE_LEAF}[law]


def potentials_through_both_planners(nbx, b, dim, leaves, law, eps):
    """plan.potentials through the host and the device planner: the same bits."""
    phi = None
    for which in ("host", "device"):
        with planner(which), nbx.LeafPlan(b.shape[0], dim, *leaves) as plan:
            if law == "newton":
                plan.set_softening(eps)
            got = plan.potentials(b, law_id(nbx, law))
            if phi is None:
                phi = got
            assert np.array_equal(got, phi), f"{which} planner"
            assert np.array_equal(plan.get_potentials(), phi)
    return phi


def assert_phi_parity(phi, ref, S, E, what, in_leaf=None):
    assert phi.shape == ref.shape and np.isfinite(phi).all(), what
    live = S > 0
    assert not phi[~live].any(), f"{what}: bodies without any counted term must get exactly zero"
    if in_leaf is not None:
        assert not phi[~in_leaf].any(), f"{what}: bodies in no leaf get exact zeros"
    bound = TOL_BACKWARD_SMALL_N * S + E
    err = np.abs(phi - ref)
    worst = float((err[live] / bound[live]).max()) if live.any() else 0.0
    print(f"{what}: {int(live.sum())} live targets, |dphi| / bound = {worst:.3f}")
    assert (err[live] <= bound[live]).all(), f"{what}: {worst:.2f} x the bound"


# ---- 1, 2: the near field ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _complete_case(nbx, oracle, dim, law, eps):
    """6,000 generated bodies with one coincident pair and the specification's potential on COMPLETE lists -- which does not depend on how
    the bodies are cut into leaves (tests/test_tree_potential_cpu.py::test_partition): computed once, through leaves of 32."""
    b = oracle.round_inputs_to_f32(oracle.generate(90 + dim, 6000, dim))
    b[11, :dim] = b[10, :dim]
    b = np.ascontiguousarray(b)
    ref, S = nbx.leaves.near_potentials(b, dim, *nbx.leaves.all_pairs_leaves(6000, 32), law, eps)
    return b, ref, S


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("leaf_size", (32, 8, 4, 3))
@pytest.mark.parametrize("dim", (3, 2))
def test_near_field_on_complete_lists(nbx, oracle, dim, leaf_size, law):
    """Every leaf on every list, leaves of 32 (one-leaf workgroups of two waves), 8, 4 and 3 bodies (the packed classes; 3: every leaf
    ends in a pad), both planners, against near_potentials.  The coincident pair is counted under NEWTON and skipped under the others."""
    b, ref, S = _complete_case(nbx, oracle, dim, law, EPS)
    phi = potentials_through_both_planners(nbx, b, dim, nbx.leaves.all_pairs_leaves(6000, leaf_size), law, EPS)
    assert_phi_parity(phi, ref, S, np.zeros_like(S), f"{law} D={dim}, complete lists through leaves of {leaf_size}")


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("dim", (3, 2))
@pytest.mark.parametrize("shape", ("tiny_mixed", "fmm_sized", "long_lists", "big_leaves", "wide_mixed"))
def test_near_field_on_ragged_structures(nbx, oracle, dim, shape, law):
    """tests/test_gpu_newton_tree.py::test_ragged_structures' structures (every packed class, empty leaves and lists, more than 32 runs,
    two-wave workgroups with cut pieces, several workgroups per leaf, repeated list entries) against near_potentials."""
    seed, sizes, list_len = _ragged_cases()[shape]
    leaves, n = _structure(seed, sizes, list_len)
    b = oracle.round_inputs_to_f32(oracle.generate(95 + dim, n, dim))
    phi = potentials_through_both_planners(nbx, b, dim, leaves, law, EPS)
    ref, S = nbx.leaves.near_potentials(b, dim, *leaves, law, EPS)
    in_leaf = np.zeros(n, dtype=bool)
    in_leaf[np.asarray(leaves[1])] = True
    assert (~in_leaf).sum() >= 11
    assert_phi_parity(phi, ref, S, np.zeros_like(S), f"{law} {shape} D={dim}", in_leaf)


@pytest.mark.parametrize("leaf_size", (32, 8, 3))
@pytest.mark.parametrize("dim", (3, 2))
def test_self_term(nbx, oracle, dim, leaf_size):
    """The same bodies at eps = 2^-6 under NEWTON.  m_i / eps exceeds the rest of phi_i by orders of magnitude: a self term that is
    summed and subtracted afterwards, or excluded by distance, cannot meet the bound -- and the coincident pair's m_j / eps must be there."""
    b, ref, S = _complete_case(nbx, oracle, dim, "newton", EPS_SMALL)
    self_term = b[:, -1] / EPS_SMALL
    others = np.delete(np.arange(6000), (10, 11))
    assert np.median(self_term[others] / S[others]) > 1e3, "the self term must dwarf the sum, or the test shows nothing"
    assert ref[10] >= b[11, -1] / EPS_SMALL and ref[11] >= b[10, -1] / EPS_SMALL
    phi = potentials_through_both_planners(nbx, b, dim, nbx.leaves.all_pairs_leaves(6000, leaf_size), "newton", EPS_SMALL)
    assert_phi_parity(phi, ref, S, np.zeros_like(S), f"self term, D={dim}, leaves of {leaf_size}")
    assert abs(phi[10] - ref[10]) <= TOL_BACKWARD_SMALL_N * S[10] and phi[10] >= 0.999 * b[11, -1] / EPS_SMALL


# ---- 3: totals against independent code --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", (3, 2))
def test_totals_against_independent_code(nbx, oracle, dim):
    """Complete lists: U under BRUTE against oracle.energy's potential to the 2e-6 relative that tests/test_gpu_energy.py grants
    nbx_ctx_energy; U under NEWTON against Context.energy (law and softening set on the context) to twice that; K against
    Context.energy's to 1e-13 relative."""
    n = 3000
    b = oracle.round_inputs_to_f32(oracle.generate(12, n, dim))
    b[10, :dim] = b[11, :dim]
    ke_ref, pe_ref = oracle.energy(b)
    with nbx.Context(n, dim) as c, nbx.LeafPlan(n, dim, *nbx.leaves.all_pairs_leaves(n, 32)) as plan:
        c.upload(b)
        ke_ctx, pe_ctx = c.energy(oracle.G)
        ke, pe = plan.energy(c, nbx.LAW_BRUTE, oracle.G)
        print(f"D={dim} BRUTE: U_tree {pe:.12e}, oracle {pe_ref:.12e}, rel {abs(pe - pe_ref) / abs(pe_ref):.2e}; K rel {abs(ke - ke_ctx) / ke_ctx:.2e}")
        assert abs(ke - ke_ctx) <= 1e-13 * ke_ctx and abs(ke - ke_ref) <= 1e-13 * ke_ref
        assert abs(pe - pe_ref) <= 2e-6 * abs(pe_ref)
        c.set_softening(EPS)
        c.set_law(nbx.FORCE_LAW_NEWTON)
        plan.set_softening(EPS)
        ke_n, pe_n = c.energy(oracle.G)
        ke2, pe2 = plan.energy(c, nbx.LAW_NEWTON, oracle.G)
        print(f"D={dim} NEWTON: U_tree {pe2:.12e}, context {pe_n:.12e}, rel {abs(pe2 - pe_n) / abs(pe_n):.2e}")
        assert pe2 < 0 and abs(pe2 - pe_n) <= 4e-6 * abs(pe_n)
        assert abs(ke2 - ke_n) <= 1e-13 * ke_n
        # the reduction is the per-body potentials': U = s (G / 2) sum m_i phi_i
        phi = plan.get_potentials()
        assert abs(-0.5 * oracle.G * float((b[:, -1] * phi).sum()) - pe2) <= 1e-12 * abs(pe2)


# ---- 4: the far field --------------------------------------------------------------------------------------------------------------

def far_terms(nbx, b, dim, leaves, far, mom, law, eps):
    """Per body and per unit G m_i: the far cells' monopole potentials and corrections (sums and magnitude sums) and the two parts of E_i
    of the module docstring."""
    mass, com, Q = mom
    assert (b[:, -1] >= 0.0).all(), "the bound assumes a positive semi-definite q"
    newton = law == "newton"
    lo, lb = np.asarray(leaves[0], dtype=np.int64), np.asarray(leaves[1], dtype=np.int64)
    fo, fc = np.asarray(far[0], dtype=np.int64), np.asarray(far[1], dtype=np.int64)
    eps_c = np.sqrt(dim) * 2.0 ** -23 * np.abs(com).max(axis=1)
    t = Q[:, :dim].sum(axis=1) / np.where(mass != 0.0, mass, 1.0)
    n = b.shape[0]
    P0, C, S0, SC, E0, E1 = (np.zeros(n) for _ in range(6))
    for tl in range(lo.size - 1):
        ids, c = lb[lo[tl]:lo[tl + 1]], fc[fo[tl]:fo[tl + 1]]
        c = c[mass[c] != 0.0]
        if not ids.size or not c.size:
            continue
        R = com[None, c, :] - b[ids, None, :dim]
        r2 = (R * R).sum(axis=2)
        corr = nbx.leaves.far_potential_correction(R, mass[None, c], Q[None, c, :], law, eps)
        if newton:
            rho2 = r2 + eps * eps
            rho = np.sqrt(rho2)
            mono = mass[c] / rho
            E0[ids] = (mass[c] * eps_c[c] / rho2).sum(axis=1)
            E1[ids] = (mass[c] * t[c] * (12.0 * eps_c[c] / rho2 ** 2 + 2.0 * U_Q / (rho2 * rho))).sum(axis=1)
        else:
            assert (r2 >= 1e-9).all()
            r = np.sqrt(r2)
            mono = 0.5 * mass[c] / r2
            E0[ids] = (mass[c] * eps_c[c] / (r2 * r)).sum(axis=1)
            E1[ids] = (mass[c] * t[c] * (18.0 * eps_c[c] / (r2 * r2 * r) + 2.5 * U_Q / r2 ** 2)).sum(axis=1)
        P0[ids], S0[ids] = mono.sum(axis=1), np.abs(mono).sum(axis=1)
        C[ids], SC[ids] = corr.sum(axis=1), np.abs(corr).sum(axis=1)
    return dict(P0=P0, C=C, S0=S0, SC=SC, E0=E0, E1=E1)


def spec_terms(nbx, b, dim, leaves, cells, far, law, eps):
    """near_potentials + far_terms, and far_potentials (the specification the header names) checked against the latter."""
    mom = nbx.leaves.cell_moments(b, dim, leaves[0], leaves[1], *cells)
    near, S_near = nbx.leaves.near_potentials(b, dim, *leaves, law, eps)
    T = far_terms(nbx, b, dim, leaves, far, mom, law, eps)
    for order in (0, 1):
        spec, S = nbx.leaves.far_potentials(b, dim, leaves[0], leaves[1], *cells, *far, order=order, law=law, eps=eps, moments=mom)
        assert (np.abs(spec - (T["P0"] + order * T["C"])) <= 1e-13 * (T["S0"] + T["SC"])).all()
        assert (S <= (T["S0"] + order * T["SC"]) * (1 + 1e-12)).all()
    T.update(near=near, S_near=S_near)
    return T


def ref_at(T, order):
    return (T["near"] + T["P0"] + order * T["C"], T["S_near"] + T["S0"] + order * T["SC"], T["E0"] + order * T["E1"])


@functools.lru_cache(maxsize=None)
def _far_case(nbx, oracle, dim, depth, theta, law):
    """20,000 generated bodies, their octree and the specification's terms: once per shape and law."""
    b = oracle.round_inputs_to_f32(oracle.generate(50 + dim, 20000, dim))
    leaves, cells, far = octree(nbx, b, dim, depth, theta)
    return b, leaves, cells, far, spec_terms(nbx, b, dim, leaves, cells, far, law, EPS)


@pytest.mark.parametrize("law", ("newton", "tree_leaf"))
@pytest.mark.parametrize("dim,depth,theta", SHAPES)
def test_far_field_against_the_specification(nbx, oracle, dim, depth, theta, law):
    """Near + far at orders 0 and 1 on octrees of 20,000 generated bodies against the specification.  At order 1 the correction must stand
    far above the bound or the test shows nothing: a median |C_i| / (TOL phi_i) >= 100 for the reference law in 3D and for both laws in 2D.
    Under NEWTON in 3D an isotropic q contributes nothing (1 / rho is harmonic at eps = 0), the median is only 6 - 16; those two shapes are
    still held to the bound, and their discriminating case is test_far_field_of_rods."""
    b, leaves, cells, far, T = _far_case(nbx, oracle, dim, depth, theta, law)
    n = b.shape[0]
    got = {}
    with nbx.LeafPlan(n, dim, *leaves) as plan:
        plan.set_softening(EPS)
        plan.set_cells(*cells, *far)
        for order in (0, 1):
            plan.set_far_order(order)
            got[order] = plan.potentials(b, law_id(nbx, law))
            ref, S, E = ref_at(T, order)
            assert_phi_parity(got[order], ref, S, E, f"{law} order {order}, octree depth {depth} theta {theta} D={dim}")
    ref1, _, _ = ref_at(T, 1)
    size = np.abs(T["C"]) / (TOL_BACKWARD_SMALL_N * np.abs(ref1))
    print(f"{law} D={dim} depth {depth} theta {theta}: median |C_i| / (TOL phi_i) = {float(np.median(size)):.1f}, 10th percentile {float(np.percentile(size, 10)):.1f}")
    assert not np.array_equal(got[0], got[1])
    if not (law == "newton" and dim == 3):
        assert np.median(size) >= 100.0


def _rod_case(nbx, dim):
    """Cells whose bodies lie along a line: 24 rods of 16 bodies and length L = 1e4 along x, one leaf and one cell each; per rod four
    single-body target leaves ON ITS AXIS at 3 - 6 rod lengths from its centre, whose far list is that rod's cell alone.  Behind the
    targets: single-body source leaves (a cell with Q = 0) and massless leaves (a cell with M = 0) for the fallbacks."""
    rng = np.random.default_rng(17)
    L, n_rods, per_rod = 1.0e4, 24, 16
    rows, sizes = [], []
    centres = rng.uniform(-4.0e5, 4.0e5, (n_rods, dim))
    for k in range(n_rods):
        x = np.zeros((per_rod, dim))
        x[:, 0] = np.linspace(-0.5 * L, 0.5 * L, per_rod)
        rows.append(np.concatenate([centres[k] + x, np.zeros((per_rod, dim)), rng.uniform(1e3, 1e5, (per_rod, 1))], axis=1))
        sizes.append(per_rod)
    targets_of = []
    for k in range(n_rods):
        mine = []
        for d in np.linspace(3.0, 6.0, 4) * (1 if k % 2 else -1):
            p = centres[k].copy()
            p[0] += d * L
            rows.append(np.concatenate([p, np.zeros(dim), [1.0e4]])[None, :])
            mine.append(len(sizes))
            sizes.append(1)
        targets_of.append(mine)
    b = np.ascontiguousarray(np.concatenate(rows).astype(np.float32).astype(np.float64))
    n = b.shape[0]
    lo = np.concatenate([[0], np.cumsum(sizes)])
    lb = np.arange(n)
    nl = len(sizes)
    near_off, near_src = np.arange(nl + 1), np.arange(nl)                     # every leaf: itself
    cell_first, cell_count = np.arange(n_rods), np.ones(n_rods, dtype=np.int64)
    far_lists = [[] for _ in range(nl)]
    for k in range(n_rods):
        for t in targets_of[k]:
            far_lists[t] = [k]
    far_off = np.concatenate([[0], np.cumsum([len(f) for f in far_lists])])
    far_cells = np.concatenate([np.asarray(f, dtype=np.int64) for f in far_lists])
    targets = np.concatenate(targets_of)
    return b, (lo, lb, near_off, near_src), (cell_first, cell_count), (far_off, far_cells), lo[targets]


@pytest.mark.parametrize("dim", (3, 2))
def test_far_field_of_rods(nbx, dim):
    """NEWTON's discriminating case: on the axis of a rod the correction is M t / rho^3, about (L^2 / 12) / d^2 of the monopole.  Checked
    with the specification on the CPU first: the correction exceeds 100 x the bound for EVERY target; then the device is held to the bound
    at both orders, and order 0 must MISS the order-1 specification."""
    eps = 64.0
    b, leaves, cells, far, tgt = _rod_case(nbx, dim)
    T = spec_terms(nbx, b, dim, leaves, cells, far, "newton", eps)
    ref1, S1, E1 = ref_at(T, 1)
    bound1 = TOL_BACKWARD_SMALL_N * S1 + E1
    ratio = np.abs(T["C"][tgt]) / bound1[tgt]
    print(f"rods D={dim}: |C_i| / bound over {tgt.size} targets: min {float(ratio.min()):.0f}, median {float(np.median(ratio)):.0f}")
    assert (ratio > 100.0).all()
    with nbx.LeafPlan(b.shape[0], dim, *leaves) as plan:
        plan.set_softening(eps)
        plan.set_cells(*cells, *far)
        for order in (0, 1):
            plan.set_far_order(order)
            phi = plan.potentials(b, nbx.LAW_NEWTON)
            ref, S, E = ref_at(T, order)
            assert_phi_parity(phi, ref, S, E, f"rods D={dim} order {order}")
            if order == 0:
                assert (np.abs(phi[tgt] - ref1[tgt]) > 50.0 * bound1[tgt]).all(), "order 0 must not pass for order 1"


@pytest.mark.parametrize("law", ("newton", "tree_leaf"))
def test_massless_cells_and_the_zero_q_fallback(nbx, law):
    """Cells of one body have Q = 0, so their q record is all zeros: order 1 gives exactly the monopole's bits.  Massless cells at the end
    of the far lists add exactly nothing."""
    dim, rng = 3, np.random.default_rng(23)
    n_t, n_s, n_z = 70, 300, 40
    n = n_t + n_s + n_z
    b = np.zeros((n, 7))
    b[:n_t, :3] = rng.uniform(-1e5, 1e5, (n_t, 3))
    b[n_t:, :3] = rng.uniform(4e5, 9e5, (n_s + n_z, 3))
    b[:, -1] = rng.uniform(1e3, 1e6, n)
    b[n_t + n_s:, -1] = 0.0
    b = np.ascontiguousarray(b.astype(np.float32).astype(np.float64))
    lo = np.concatenate([[0, n_t], n_t + 1 + np.arange(n_s + n_z)])            # leaf 0: the targets; then one leaf per source body
    nl = lo.size - 1
    leaves = (lo, np.arange(n), np.arange(nl + 1), np.arange(nl))
    cell_first, cell_count = 1 + np.arange(n_s + n_z), np.ones(n_s + n_z, dtype=np.int64)

    def far(with_massless):
        k = n_s + (n_z if with_massless else 0)
        return np.concatenate([[0], np.full(nl, k)]), np.arange(k)

    got = {}
    with nbx.LeafPlan(n, dim, *leaves) as plan:
        plan.set_softening(64.0)
        for with_massless in (False, True):
            plan.set_cells(cell_first, cell_count, *far(with_massless))
            for order in (0, 1):
                plan.set_far_order(order)
                got[with_massless, order] = plan.potentials(b, law_id(nbx, law))
    assert got[False, 0][:n_t].all() and not got[False, 0][n_t:].any()
    for key in ((False, 1), (True, 0), (True, 1)):
        assert np.array_equal(got[key], got[False, 0]), key
    near, S_near = nbx.leaves.near_potentials(b, dim, *leaves, law, 64.0)
    T = far_terms(nbx, b, dim, leaves, far(True), nbx.leaves.cell_moments(b, dim, lo, leaves[1], cell_first, cell_count), law, 64.0)
    assert not T["C"].any()
    assert_phi_parity(got[True, 1], near + T["P0"], S_near + T["S0"], T["E0"], f"{law}: single-body and massless cells")


# ---- 5, 6, 7: every way in, the observer, trees built on the device ----------------------------------------------------------------

def test_every_way_in_gives_the_same_bits(nbx, oracle):
    """potentials(b) on host bodies, energy(ctx) + get_potentials() on the same bodies uploaded, and a plan from from_octree against a plan
    made from structure()'s eight arrays: the same bits, at order 1 under both law families."""
    dim, depth, theta = SHAPES[0]
    n = 20000
    b = oracle.round_inputs_to_f32(oracle.generate(50 + dim, n, dim))
    with nbx.Context(n, dim) as c:
        c.upload(b)
        with nbx.LeafPlan.from_octree(c, depth, theta) as dev:
            arrays = dev.structure()
            with nbx.LeafPlan(n, dim, *arrays[:4]) as host:
                host.set_cells(*arrays[4:])
                for p in (dev, host):
                    p.set_far_order(nbx.FAR_QUADRUPOLE)
                    p.set_softening(EPS)
                for law in (nbx.LAW_NEWTON, nbx.LAW_TREE_LEAF):
                    want = host.potentials(b, law)
                    assert want.all()
                    assert np.array_equal(host.get_potentials(), want)
                    for what, p in (("device tree", dev), ("host arrays", host)):
                        ke, pe = p.energy(c, law, oracle.G)
                        assert np.array_equal(p.get_potentials(), want), f"{what}: resident bodies, law {law}"
                        assert abs(-0.5 * oracle.G * float((b[:, -1] * want).sum()) - pe) <= 1e-12 * abs(pe)
                    assert np.array_equal(dev.potentials(b, law), want), f"device tree: host bodies, law {law}"


@pytest.mark.parametrize("order", (0, 1))
def test_observer(nbx, oracle, order):
    """On a device octree plan get_forces() before and after energy() are the same bits, and step_octree for 6 steps with an energy() call
    between every two steps leaves the downloaded bodies bit-identical to the run without the calls."""
    dim, depth, theta, n, dt = 3, 3, 0.5, 20000, 1.5
    b = oracle.round_inputs_to_f32(oracle.generate(53, n, dim))
    G = oracle.G * 1e24
    out = []
    for look in (False, True):
        with nbx.Context(n, dim) as c:
            c.upload(b)
            with nbx.LeafPlan.from_octree(c, depth, theta) as plan:
                plan.set_far_order(order)
                plan.set_softening(EPS)
                f = plan.forces_ctx(c, nbx.LAW_NEWTON, G)
                if look:
                    ke, pe = plan.energy(c, nbx.LAW_NEWTON, G)
                    assert ke >= 0 and pe < 0
                    assert np.array_equal(plan.get_forces(), f), "energy() must leave the last evaluation's sums alone"
                    plan.energy(c, nbx.LAW_TREE_LEAF, G)                  # another law: still an observer
                    assert np.array_equal(plan.get_forces(), f)
                    plan.potentials(b[::-1].copy(), nbx.LAW_NEWTON)        # other host bodies: the masses of the last evaluation stay
                    assert np.array_equal(plan.get_forces(), f)
                for _ in range(3):
                    plan.step_octree(c, nbx.LAW_NEWTON, G, dt, 2, 1)
                    if look:
                        plan.energy(c, nbx.LAW_NEWTON, G)
                g = b.copy()
                c.download(g)
                out.append((g, plan.get_forces()))
    if order == 0:
        # host bodies: the masses of the last force evaluation live in the plan's staged copy, which a potential call of other bodies
        # must not touch
        other = b.copy()
        other[:, -1] *= 3.0
        with nbx.LeafPlan(n, dim, *octree(nbx, b, dim, depth, theta)[0]) as plan:
            f = plan.forces(b, nbx.LAW_TREE_LEAF, G)
            plan.potentials(other, nbx.LAW_TREE_LEAF)
            assert np.array_equal(plan.get_forces(), f)
    assert not np.array_equal(out[0][0][:, dim:2 * dim], b[:, dim:2 * dim]), "coupling too weak to test anything"
    assert np.array_equal(out[0][0], out[1][0]), "bodies after 6 steps"
    assert np.array_equal(out[0][1], out[1][1])


def _direct_sample(b, dim, rows, law, eps):
    """phi of the bodies `rows` by a direct all-pairs fp64 sum."""
    x, m = b[:, :dim], b[:, -1]
    out = np.zeros(rows.size)
    for i0 in range(0, rows.size, 256):
        r = rows[i0:i0 + 256]
        r2 = ((x[None, :, :] - x[r, None, :]) ** 2).sum(axis=2)
        if law == "newton":
            w = m[None, :] / np.sqrt(r2 + eps * eps)
            w[np.arange(r.size), r] = 0.0
        else:
            keep = r2 >= 1e-9
            w = np.where(keep, 0.5 * m[None, :] / np.where(keep, r2, 1.0), 0.0)
        out[i0:i0 + 256] = w.sum(axis=1)
    return out


@pytest.mark.parametrize("law", ("newton", "tree_leaf"))
@pytest.mark.parametrize("tree", ("from_octree", "from_octree_adaptive"))
def test_device_trees(nbx, oracle, tree, law):
    """from_octree on generated bodies and from_octree_adaptive (Plummer sphere, capacity 32) at N = 20,000 against the specification on the
    structure read back, at both orders; and, for 2,000 bodies, against a direct all-pairs fp64 sum: median and p99 relative error are
    printed, and order 1's median must be below order 0's (not asserted of the total U: the per-body errors cancel differently)."""
    n, dim, G, eps = 20000, 3, 0.1, 2048.0
    if tree == "from_octree":
        b = oracle.round_inputs_to_f32(oracle.generate(53, n, dim))
        make = lambda c: nbx.LeafPlan.from_octree(c, 4, 0.5)
    else:
        b = oracle.round_inputs_to_f32(np.ascontiguousarray(nbx.plummer_bodies(n, dim, seed=3, G=G)))
        make = lambda c: nbx.LeafPlan.from_octree_adaptive(c, 10, 32, 0.5)
    got, U = {}, {}
    with nbx.Context(n, dim) as c:
        c.upload(b)
        with make(c) as plan:
            plan.set_softening(eps)
            for order in (0, 1):
                plan.set_far_order(order)
                _, U[order] = plan.energy(c, law_id(nbx, law), G)
                got[order] = plan.get_potentials()
            arrays = plan.structure()
    leaves, cells, far = arrays[:4], arrays[4:6], arrays[6:8]
    T = spec_terms(nbx, b, dim, leaves, cells, far, law, eps)
    rows = np.arange(0, n, 10)
    exact = _direct_sample(b, dim, rows, law, eps)
    med = {}
    for order in (0, 1):
        ref, S, E = ref_at(T, order)
        assert_phi_parity(got[order], ref, S, E, f"{tree} {law} order {order}")
        bound_U = 0.5 * G * float((np.abs(b[:, -1]) * (TOL_BACKWARD_SMALL_N * S + E)).sum())
        U_spec = -0.5 * G * float((b[:, -1] * ref).sum())
        assert abs(U[order] - U_spec) <= bound_U, f"{tree} {law} order {order}: U {U[order]:.9e} against {U_spec:.9e}"
        rel = np.abs(got[order][rows] - exact) / np.abs(exact)
        med[order] = float(np.median(rel))
        print(f"{tree} {law} order {order}: relative error against all pairs, median {med[order]:.2e}, p99 {float(np.percentile(rel, 99)):.2e}")
    assert med[1] < med[0]


# ---- 8: refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals(nbx, oracle):
    """Every refusal of the header; after each the plan still evaluates forces to the bits it gave before."""
    n, dim = 64, 3
    b = oracle.round_inputs_to_f32(oracle.generate(7, n, dim))
    leaves = nbx.leaves.all_pairs_leaves(n, 8)
    L = nbx.load_library()

    def status(call):
        with pytest.raises(nbx.NbxError) as e:
            call()
        return e.value.status

    with nbx.LeafPlan(n, dim, *leaves) as plan, nbx.Context(n, dim) as c, nbx.Context(n, dim) as empty, nbx.Context(n, 2) as flat, \
            nbx.Context(n + 1, dim) as bigger, nbx.Context(n, dim, n_shards=2, shard=0) as sharded:
        c.upload(b)
        good = plan.forces(b, nbx.LAW_TREE_LEAF, oracle.G)
        out = np.zeros(n)

        def still_good():
            assert np.array_equal(plan.get_forces(), good)
            assert np.array_equal(plan.forces(b, nbx.LAW_TREE_LEAF, oracle.G), good)

        assert status(plan.get_potentials) == NBX_ERR_STATE                      # before the first potential call
        for law in (nbx.LAW_FMM_P2P, 4, -1):
            assert status(lambda: plan.potentials(b, law)) == NBX_ERR_INVALID
            assert status(lambda: plan.energy(c, law, oracle.G)) == NBX_ERR_INVALID
        still_good()
        assert status(lambda: plan.potentials(b, nbx.LAW_NEWTON)) == NBX_ERR_STATE           # eps = 0
        assert status(lambda: plan.energy(c, nbx.LAW_NEWTON, oracle.G)) == NBX_ERR_STATE
        assert status(lambda: plan.energy(empty, nbx.LAW_TREE_LEAF, oracle.G)) == NBX_ERR_STATE   # nothing uploaded
        still_good()
        for wrong in (flat, bigger, sharded):
            assert status(lambda: plan.energy(wrong, nbx.LAW_TREE_LEAF, oracle.G)) == NBX_ERR_INVALID
        assert L.nbx_leaf_plan_potentials(plan.h, None, 56, nbx.LAW_TREE_LEAF, out.ctypes.data) == NBX_ERR_INVALID
        assert L.nbx_leaf_plan_potentials(plan.h, b.ctypes.data, 56, nbx.LAW_TREE_LEAF, None) == NBX_ERR_INVALID
        assert L.nbx_leaf_plan_potentials(plan.h, b.ctypes.data, 48, nbx.LAW_TREE_LEAF, out.ctypes.data) == NBX_ERR_INVALID   # stride < sizeof(Body<3>)
        assert L.nbx_leaf_plan_potentials(plan.h, b.ctypes.data, 60, nbx.LAW_TREE_LEAF, out.ctypes.data) == NBX_ERR_INVALID   # not a multiple of 8
        assert L.nbx_leaf_plan_energy(plan.h, None, nbx.LAW_TREE_LEAF, 1.0, None, None) == NBX_ERR_INVALID
        assert L.nbx_leaf_plan_get_potentials(plan.h, None) == NBX_ERR_INVALID
        assert status(plan.get_potentials) == NBX_ERR_STATE                      # still none went through
        still_good()
        # the max|m| / eps^3 rule of the force evaluations
        heavy = b.copy()
        heavy[:, -1] = 1.0e6
        heavy[3, -1] = 1.0e8
        plan.set_softening(1.0e15)
        assert status(lambda: plan.potentials(heavy, nbx.LAW_NEWTON)) == NBX_ERR_INVALID
        plan.set_softening(1.0e-6)
        heavy[3, -1] = 1.0e21
        assert status(lambda: plan.potentials(heavy, nbx.LAW_NEWTON)) == NBX_ERR_INVALID
        plan.set_softening(64.0)
        still_good()
        # ... and the calls go through: either out pointer may be NULL
        phi = plan.potentials(b, nbx.LAW_NEWTON)
        assert phi.all() and np.array_equal(plan.get_potentials(), phi)
        assert L.nbx_leaf_plan_energy(plan.h, c.h, nbx.LAW_NEWTON, oracle.G, None, None) == 0
        assert np.array_equal(plan.get_potentials(), phi)
        still_good()


# ---- 9: the C++ layer and the harness ----------------------------------------------------------------------------------------------

def test_cpp_layer_and_harness(tmp_path):
    """nbody_sim -m t --law newton --energy-every 10 --energy-tree prints an E_tree line behind each energy line (BarnesHutNewtonHip's
    tree_energy); the potentials of the two are within 1e-3 relative -- a cap against gross failure, not a measurement; the measured
    difference is printed.  Without --energy-tree stdout has the format it had: the non-timing fields of the two runs are the same."""
    sim = os.path.join(ROOT, "nbody_sim")
    assert os.path.exists(sim)
    common = ["-N", "8192", "-m", "t", "--init", "plummer", "--leaf-cap", "32", "--far-order", "1", "--law", "newton", "--softening", "2048", "--G", "0.1",
              "--steps", "20", "--energy-every", "10", "--seed", "5"]     # a fixed seed: the two runs are compared

    def run(name, extra):
        cwd = tmp_path / name
        cwd.mkdir()
        p = subprocess.run([sim] + common + extra, cwd=cwd, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        return p.stdout

    def without_times(text):
        keep = []
        for line in text.splitlines():
            if "E_tree" in line or "Run ID: " in line:                            # the tagged lines; the run's time stamp
                continue
            if line.startswith("Time taken") or " ms per step" in line:
                line = line.split(":")[0]
            keep.append(line)
        return keep

    plain, tagged = run("plain", []), run("tree", ["--energy-tree"])
    assert "E_tree" not in plain
    assert without_times(tagged) == without_times(plain), "without the tagged lines the output is the one it was"
    lines = tagged.splitlines()
    pairs = [(lines[i - 1], line) for i, line in enumerate(lines) if "E_tree" in line]
    assert len(pairs) == 6, tagged                                               # steps 0, 10, 20 at each order
    worst = 0.0
    for allpairs, tree in pairs:
        assert allpairs.startswith("step ") and "  E = " in allpairs and tree.split("  E_tree")[0] == allpairs.split("  E = ")[0]
        pot = [float(re.search(r"potential (-?[0-9.eE+-]+)", s).group(1)) for s in (allpairs, tree)]
        kin = [float(re.search(r"kinetic (-?[0-9.eE+-]+)", s).group(1)) for s in (allpairs, tree)]
        assert pot[0] < 0 and abs(pot[1] - pot[0]) <= 1e-3 * abs(pot[0]), (allpairs, tree)
        assert abs(kin[1] - kin[0]) <= 1e-9 * kin[0]
        assert "|U_tree - U| / |U| = " in tree
        worst = max(worst, abs(pot[1] - pot[0]) / abs(pot[0]))
    print(f"\nnbody_sim --energy-tree: largest |U_tree - U_allpairs| / |U| over {len(pairs)} looks = {worst:.3e}")
