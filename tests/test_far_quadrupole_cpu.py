"""CPU: the second-order term of the far field (NBX_FAR_QUADRUPOLE, include/nbody_hip.h) -- its fp64 specification in
nbody_amd.leaves (cell_moments, far_correction, far_sums), which the GPU tests hold the kernels to, and the three ABI entries.

Nothing here needs a device: the expansion's order, the moments against extended-precision sums, the accuracy the term buys
against the oracle's all-pairs sums, and what the library answers without a plan."""
import ctypes
import os

import numpy as np
import pytest

MIN_GAIN = 8.0      # order 1 against order 0, median and p99 on the uniform 3D inputs: see test_accuracy_gain_on_uniform_3d


def expansion_residuals(nbx, dim, seed=5):
    """Relative residual (rms over 16 directions) of the monopole and of monopole + far_correction against the direct sum over one
    random cell of 50 bodies, at 10, 20 and 40 cell radii from its centre of mass."""
    rng = np.random.default_rng(seed)
    x, m = rng.uniform(-1.0, 1.0, (50, dim)), rng.uniform(1.0, 10.0, 50)
    b = np.zeros((50, 2 * dim + 1))
    b[:, :dim], b[:, -1] = x, m
    M, com, Q = nbx.leaves.cell_moments(b, dim, [0, 50], np.arange(50), [0], [1])
    radius = float(np.sqrt(((x - com[0]) ** 2).sum(axis=1)).max())
    u = rng.normal(size=(16, dim))
    u /= np.sqrt((u * u).sum(axis=1))[:, None]
    mono, quad = [], []
    for k in (10.0, 20.0, 40.0):
        p = com[0] - k * radius * u                                   # targets; R = com - p
        d = x[None, :, :] - p[:, None, :]
        exact = (m[None, :, None] * d / (d * d).sum(axis=2)[..., None] ** 2).sum(axis=1)
        R = com[0] - p
        f0 = M[0] * R / (R * R).sum(axis=1)[:, None] ** 2
        f1 = f0 + nbx.leaves.far_correction(R, M[0], Q[0])
        norm = np.sqrt((exact ** 2).sum())
        mono.append(float(np.sqrt(((f0 - exact) ** 2).sum()) / norm))
        quad.append(float(np.sqrt(((f1 - exact) ** 2).sum()) / norm))
    return mono, quad


@pytest.mark.parametrize("dim", (2, 3))
def test_order_of_the_expansion(nbx, dim):
    """Per doubling of the distance the monopole's residual falls ~4x (the missing term is second order), with far_correction ~8x
    (the missing term is third order); measured 3.5-3.7 and 7.3-7.6 when the formula was derived."""
    mono, quad = expansion_residuals(nbx, dim)
    print(f"D={dim}: monopole residuals {mono}, with the correction {quad}")
    for a, b in ((0, 1), (1, 2)):
        assert mono[a] / mono[b] > 3.0, (mono[a] / mono[b])
        assert quad[a] / quad[b] > 6.0, (quad[a] / quad[b])
        assert quad[a] < mono[a] and quad[b] < mono[b]


def longdouble_moments(b, dim, lo, lb, cf, cc):
    """The sums of leaves.cell_moments written out again, in np.longdouble."""
    L = np.longdouble
    pairs = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)) if dim == 3 else ((0, 0), (1, 1), (0, 1))
    M, com, Q = np.zeros(len(cf), dtype=L), np.zeros((len(cf), dim), dtype=L), np.zeros((len(cf), len(pairs)), dtype=L)
    for c in range(len(cf)):
        ids = lb[lo[cf[c]]:lo[cf[c] + cc[c]]]
        m, x = b[ids, -1].astype(L), b[ids, :dim].astype(L)
        M[c] = m.sum()
        if M[c] == 0:
            continue
        com[c] = (m[:, None] * x).sum(axis=0) / M[c]
        s = x - com[c]
        Q[c] = [(m * s[:, i] * s[:, j]).sum() for i, j in pairs]
    return M, com, Q


@pytest.mark.parametrize("dim,depth", ((3, 3), (2, 4)))
def test_cell_moments_against_longdouble(nbx, oracle, dim, depth):
    """|dQ_ab| <= 2^-24 tr(Q) per cell on the octree of 20,000 generated bodies; a one-body cell has Q == 0 exactly; a massless cell
    gives zeros."""
    b = oracle.round_inputs_to_f32(oracle.generate(60 + dim, 20000, dim))
    r = nbx.leaves.octree_cells(b, dim, depth, 0.5)
    lo, lb = r[0].astype(np.int64), r[1].astype(np.int64)
    one = int(lb[lo[7]])
    b[lb[lo[3]:lo[5]], -1] = 0.0                                           # two massless leaves: cells -2 and -1
    nl = lo.size - 1
    cf = np.concatenate([r[4], [3, 4]]).astype(np.int64)
    cc = np.concatenate([r[5], [2, 1]]).astype(np.int64)
    M, com, Q = nbx.leaves.cell_moments(b, dim, lo, lb, cf, cc)
    ML, comL, QL = longdouble_moments(b, dim, lo, lb, cf, cc)
    assert Q.dtype == np.float64 and Q.shape == (cf.size, dim * (dim + 1) // 2)
    tr = QL[:, :dim].sum(axis=1)
    live = tr > 0
    assert live.sum() > 100
    assert (np.abs(Q - QL) <= 2.0 ** -24 * tr[:, None]).all(), float((np.abs(Q - QL) / np.maximum(tr, 1e-300)[:, None]).max())
    print(f"D={dim}: largest |dQ| / tr(Q) = {float((np.abs(Q - QL)[live] / tr[live, None]).max()):.2e} (bound {2.0 ** -24:.2e})")
    assert not M[-2:].any() and not com[-2:].any() and not Q[-2:].any(), "massless cells give zeros"
    M1, com1, Q1 = nbx.leaves.cell_moments(b[one:one + 1], dim, [0, 1], [0], [0], [1])
    assert M1[0] == b[one, -1] and np.array_equal(com1[0], b[one, :dim]) and not Q1.any(), "a one-body cell has Q == 0 exactly"
    assert nl > 100


def tree_errors(nbx, oracle, b, dim, structure):
    """Relative error of near (direct, fp64) + far (order 0 and 1) against the oracle's all-pairs sums, per body."""
    lo, lb, so, ss = (np.asarray(a, dtype=np.int64) for a in structure[:4])
    G = oracle.G
    near = np.zeros((b.shape[0], dim))
    for t in range(lo.size - 1):
        ids = lb[lo[t]:lo[t + 1]]
        src = np.concatenate([lb[lo[s]:lo[s + 1]] for s in ss[so[t]:so[t + 1]]])
        d = b[None, src, :dim] - b[ids, None, :dim]
        r2 = (d * d).sum(axis=2)
        w = np.where(r2 > 0, b[None, src, -1] / np.where(r2 > 0, r2, 1.0) ** 2, 0.0)
        near[ids] = (w[..., None] * d).sum(axis=1)
    mom = nbx.leaves.cell_moments(b, dim, lo, lb, structure[4], structure[5])
    ref = oracle.brute_force_omp_2(b)                                        # F_i = -G m_i sum_j m_j d / r^4 (methods.cpp:131)
    out = []
    for order in (0, 1):
        far = nbx.leaves.far_sums(b, dim, lo, lb, *structure[4:], order=order, moments=mom)
        f = -G * b[:, -1:] * (near + far)
        out.append(np.sqrt(((f - ref) ** 2).sum(axis=1)) / np.sqrt((ref ** 2).sum(axis=1)))
    return out


def gains(e0, e1):
    return float(np.median(e0) / np.median(e1)), float(np.percentile(e0, 99) / np.percentile(e1, 99))


@pytest.mark.parametrize("theta", (0.5, 0.7))
def test_accuracy_gain_on_uniform_3d(nbx, oracle, theta):
    """N = 4,096 generated bodies, depth 3: the median and the 99th percentile of the relative error against all-pairs sums are at
    least MIN_GAIN times smaller at order 1 than at order 0.
    Measured with the oracle's generator (seed 71), order 0 -> order 1, median / p99:
        theta 0.5: 1.54e-3 -> 5.58e-5 (27.6x) / 8.75e-3 -> 4.88e-4 (17.9x)
        theta 0.7: 3.31e-3 -> 1.49e-4 (22.2x) / 1.91e-2 -> 1.31e-3 (14.5x)
    Every ratio is at least 11, so the factor is the 8 the feature was specified with (it would have been half the smallest ratio
    otherwise).  All 4,096 bodies improve."""
    b = oracle.round_inputs_to_f32(oracle.generate(71, 4096, 3))
    e0, e1 = tree_errors(nbx, oracle, b, 3, nbx.leaves.octree_cells(b, 3, 3, theta))
    gm, gp = gains(e0, e1)
    print(f"uniform 3D theta {theta}: median {np.median(e0):.2e} -> {np.median(e1):.2e} ({gm:.1f}x), "
          f"p99 {np.percentile(e0, 99):.2e} -> {np.percentile(e1, 99):.2e} ({gp:.1f}x), improved bodies {float((e1 < e0).mean()):.3f}")
    assert gm >= MIN_GAIN and gp >= MIN_GAIN


def test_accuracy_improves_in_2d_and_on_a_plummer_sphere(nbx, oracle):
    """The same comparison on a 2D quadtree (depth 4) and on a Plummer sphere through the adaptive octree (capacity 16): printed,
    and asserted only to improve."""
    b2 = oracle.round_inputs_to_f32(oracle.generate(72, 4096, 2))
    bp = oracle.round_inputs_to_f32(np.ascontiguousarray(nbx.plummer_bodies(4096, 3, seed=3)))
    cases = (("uniform 2D depth 4 theta 0.5", b2, 2, nbx.leaves.octree_cells(b2, 2, 4, 0.5)),
             ("Plummer adaptive depth 8 capacity 16 theta 0.5", bp, 3, nbx.leaves.adaptive_octree_cells(bp, 3, 8, 16, 0.5)))
    for what, b, dim, structure in cases:
        e0, e1 = tree_errors(nbx, oracle, b, dim, structure)
        gm, gp = gains(e0, e1)
        print(f"{what}: median {np.median(e0):.2e} -> {np.median(e1):.2e} ({gm:.1f}x), p99 {np.percentile(e0, 99):.2e} -> "
              f"{np.percentile(e1, 99):.2e} ({gp:.1f}x)")
        assert gm > 1.0 and gp > 1.0, what


def test_abi_entries_and_python_members(nbx):
    """The three entry points are exported and typed, a null plan is NBX_ERR_INVALID with the argument named, and LeafPlan carries
    set_far_order, far_order and get_cell_quadrupoles."""
    typed = {name: (res, args) for name, res, args in nbx.ABI}
    assert typed["nbx_leaf_plan_set_far_order"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    assert typed["nbx_leaf_plan_get_far_order"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)])
    assert typed["nbx_leaf_plan_get_cell_quadrupoles"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    lib = nbx.load_library()
    order = ctypes.c_int(7)
    for rc in (lib.nbx_leaf_plan_set_far_order(None, 1), lib.nbx_leaf_plan_get_far_order(None, ctypes.byref(order)),
               lib.nbx_leaf_plan_get_cell_quadrupoles(None, None)):
        assert rc == 1
        assert b"plan" in lib.nbx_last_error_detail()
    assert order.value == 7
    assert (nbx.FAR_MONOPOLE, nbx.FAR_QUADRUPOLE) == (0, 1)
    assert callable(nbx.LeafPlan.set_far_order) and callable(nbx.LeafPlan.get_cell_quadrupoles)
    assert isinstance(nbx.LeafPlan.far_order, property)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbody_hip.h")).read()
    assert "enum { NBX_FAR_MONOPOLE = 0, NBX_FAR_QUADRUPOLE = 1 };" in header
