"""CPU: softened Newtonian gravity on a leaf plan (NBX_LAW_NEWTON, include/nbody_hip.h) -- its fp64 specification in
nbody_amd.leaves (far_correction and far_sums with law="newton", near_sums), which tests/test_gpu_newton_tree.py holds the kernels
to, and the two ABI entries.

Nothing here needs a device: the order of the softened kernel's expansion, the accuracy its second-order term buys against all-pairs
Newtonian sums, the defaults of far_correction / far_sums (today's arrays, bit for bit), and what the library answers without a
plan."""
import ctypes
import os

import numpy as np
import pytest

# order 1 against order 0, median and p99 of the relative error: half the smallest ratio measured per dimension (table in
# test_accuracy_gain), and more than 1 in any case
MIN_GAIN_3D = 1.8
MIN_GAIN_2D = 4.7
EPS_CASES = (1.0e4, 3.0e5)          # softening lengths on the generator's 1e7 box: far below and about a leaf's side


def newton_residuals(nbx, dim, eps_in_radii, seed=5):
    """test_far_quadrupole_cpu.expansion_residuals for the softened kernel: relative residual (rms over 16 directions) of the
    monopole M R / rho^3 and of monopole + far_correction(law="newton") against the direct sum over one random cell of 50 bodies, at
    10, 20 and 40 cell radii from its centre of mass; eps = eps_in_radii x the cell's radius."""
    rng = np.random.default_rng(seed)
    x, m = rng.uniform(-1.0, 1.0, (50, dim)), rng.uniform(1.0, 10.0, 50)
    b = np.zeros((50, 2 * dim + 1))
    b[:, :dim], b[:, -1] = x, m
    M, com, Q = nbx.leaves.cell_moments(b, dim, [0, 50], np.arange(50), [0], [1])
    radius = float(np.sqrt(((x - com[0]) ** 2).sum(axis=1)).max())
    eps = eps_in_radii * radius
    u = rng.normal(size=(16, dim))
    u /= np.sqrt((u * u).sum(axis=1))[:, None]
    mono, quad = [], []
    for k in (10.0, 20.0, 40.0):
        p = com[0] - k * radius * u                                   # targets; R = com - p
        d = x[None, :, :] - p[:, None, :]
        exact = (m[None, :, None] * d / ((d * d).sum(axis=2) + eps * eps)[..., None] ** 1.5).sum(axis=1)
        R = com[0] - p
        f0 = M[0] * R / ((R * R).sum(axis=1) + eps * eps)[:, None] ** 1.5
        f1 = f0 + nbx.leaves.far_correction(R, M[0], Q[0], law="newton", eps=eps)
        norm = np.sqrt((exact ** 2).sum())
        mono.append(float(np.sqrt(((f0 - exact) ** 2).sum()) / norm))
        quad.append(float(np.sqrt(((f1 - exact) ** 2).sum()) / norm))
    return mono, quad


@pytest.mark.parametrize("eps_in_radii", (0.0, 1.0))
@pytest.mark.parametrize("dim", (2, 3))
def test_order_of_the_expansion(nbx, dim, eps_in_radii):
    """Per doubling of the distance the monopole's residual falls ~4x (the missing term is second order), with the Newtonian
    far_correction ~8x (the missing term is third order), unsoftened and with eps = the cell's radius."""
    mono, quad = newton_residuals(nbx, dim, eps_in_radii)
    print(f"D={dim} eps={eps_in_radii} radii: monopole residuals {mono}, with the correction {quad}")
    for a, b in ((0, 1), (1, 2)):
        assert mono[a] / mono[b] > 3.0, (mono[a] / mono[b])
        assert quad[a] / quad[b] > 6.0, (quad[a] / quad[b])
    assert all(q < m for q, m in zip(quad, mono)), "the term must improve every distance"


def all_pairs_newton(b, dim, eps):
    """sum_j m_j d / (r^2 + eps^2)^(3/2) for every body, fp64 numpy, in row blocks."""
    x, m = b[:, :dim], b[:, -1]
    out = np.zeros((b.shape[0], dim))
    for i0 in range(0, b.shape[0], 256):
        d = x[None, :, :] - x[i0:i0 + 256, None, :]
        rho2 = (d * d).sum(axis=2) + eps * eps
        out[i0:i0 + 256] = ((m[None, :] / (rho2 * np.sqrt(rho2)))[..., None] * d).sum(axis=1)
    return out


def newton_tree_errors(nbx, b, dim, structure, eps):
    """Relative error of near_sums + far_sums(law="newton") at orders 0 and 1 against the all-pairs sums, per body."""
    ref = all_pairs_newton(b, dim, eps)
    near, _ = nbx.leaves.near_sums(b, dim, *structure[:4], eps)
    mom = nbx.leaves.cell_moments(b, dim, structure[0], structure[1], structure[4], structure[5])
    out = []
    for order in (0, 1):
        f = near + nbx.leaves.far_sums(b, dim, structure[0], structure[1], *structure[4:], order=order, moments=mom, law="newton", eps=eps)
        out.append(np.sqrt(((f - ref) ** 2).sum(axis=1)) / np.sqrt((ref ** 2).sum(axis=1)))
    return out


@pytest.fixture(scope="module")
def generated(oracle):
    return {dim: oracle.round_inputs_to_f32(oracle.generate(70 + dim, 4096, dim)) for dim in (2, 3)}


@pytest.mark.parametrize("theta", (0.5, 0.7))
@pytest.mark.parametrize("dim,depth", ((3, 3), (2, 4)))
def test_accuracy_gain(nbx, generated, dim, depth, theta):
    """N = 4,096 generated bodies (the oracle's generator, seeds 73 and 72), depth 3 in 3D and 4 in 2D: near + far in numpy against
    numpy all-pairs Newtonian sums; order 1 against order 0 at the median and at the 99th percentile of the relative error.
    The gain in 3D is smaller than under the reference law: a uniformly filled cube has almost no traceless quadrupole, and
    Newton's monopole is already good.
    Measured, order 0 -> order 1, median / p99:
        D=3 theta 0.5 eps 1e4: 5.07e-4 -> 9.13e-5 (5.6x) / 2.92e-3 -> 4.30e-4 (6.8x)
        D=3 theta 0.5 eps 3e5: 5.33e-4 -> 9.49e-5 (5.6x) / 3.17e-3 -> 4.41e-4 (7.2x)
        D=3 theta 0.7 eps 1e4: 1.05e-3 -> 2.86e-4 (3.7x) / 4.91e-3 -> 1.30e-3 (3.8x)
        D=3 theta 0.7 eps 3e5: 1.11e-3 -> 2.95e-4 (3.7x) / 4.92e-3 -> 1.30e-3 (3.8x)
        D=2 theta 0.5 eps 1e4: 2.46e-3 -> 5.89e-5 (41.7x) / 2.74e-2 -> 8.97e-4 (30.5x)
        D=2 theta 0.5 eps 3e5: 5.60e-3 -> 1.40e-4 (40.0x) / 2.76e-2 -> 1.48e-3 (18.7x)
        D=2 theta 0.7 eps 1e4: 5.23e-3 -> 1.92e-4 (27.2x) / 5.40e-2 -> 3.07e-3 (17.6x)
        D=2 theta 0.7 eps 3e5: 1.14e-2 -> 4.36e-4 (26.1x) / 5.94e-2 -> 6.18e-3 (9.6x)
    The smallest ratio is 3.7 in 3D and 9.6 in 2D; MIN_GAIN_3D and MIN_GAIN_2D are half of those, rounded down."""
    b = generated[dim]
    structure = nbx.leaves.octree_cells(b, dim, depth, theta)
    floor = MIN_GAIN_3D if dim == 3 else MIN_GAIN_2D
    assert floor > 1.0
    for eps in EPS_CASES:
        e0, e1 = newton_tree_errors(nbx, b, dim, structure, eps)
        gm, gp = float(np.median(e0) / np.median(e1)), float(np.percentile(e0, 99) / np.percentile(e1, 99))
        print(f"D={dim} theta {theta} eps {eps:.0e}: {np.median(e0):.2e} -> {np.median(e1):.2e} ({gm:.1f}x) / "
              f"{np.percentile(e0, 99):.2e} -> {np.percentile(e1, 99):.2e} ({gp:.1f}x)")
        assert gm >= floor and gp >= floor, (dim, theta, eps, gm, gp)


def _far_correction_today(R, M, Q):
    """leaves.far_correction as it stood before the Newtonian law, restated."""
    dim = R.shape[-1]
    pairs = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)) if dim == 3 else ((0, 0), (1, 1), (0, 1))
    M, Q = np.asarray(M, dtype=R.dtype), np.asarray(Q, dtype=R.dtype)
    live = M != 0
    q = Q / np.where(live, M, 1)[..., None]
    r2 = (R * R).sum(axis=-1)
    tr = q[..., 0] + q[..., 1] + (q[..., 2] if dim == 3 else 0)
    qR = np.zeros(np.broadcast(R, q[..., :1]).shape, dtype=R.dtype)
    for k, (a, b) in enumerate(pairs):
        qR[..., a] += q[..., k] * R[..., b]
        if a != b:
            qR[..., b] += q[..., k] * R[..., a]
    RqR = (R * qR).sum(axis=-1)
    scalar = -2 * tr / r2 + 12 * RqR / r2 ** 2
    out = (M / r2 ** 2)[..., None] * (R * scalar[..., None] - 4 * qR / r2[..., None])
    return np.where(live[..., None], out, 0)


def _far_sums_today(b, dim, lo, lb, mom, fo, fc, order):
    """leaves.far_sums as it stood before the Newtonian law, restated."""
    M, com, Q = mom
    out = np.zeros((b.shape[0], dim))
    for t in range(lo.size - 1):
        ids, c = lb[lo[t]:lo[t + 1]], fc[fo[t]:fo[t + 1]]
        c = c[M[c] != 0]
        if not ids.size or not c.size:
            continue
        R = com[None, c, :] - b[ids, None, :dim]
        r2 = (R * R).sum(axis=2)
        term = (M[c] / r2 ** 2)[..., None] * R
        if order == 1:
            term = term + _far_correction_today(R, M[None, c], Q[None, c, :])
        out[ids] = term.sum(axis=1)
    return out


@pytest.mark.parametrize("dim,depth", ((3, 3), (2, 4)))
def test_defaults_are_unchanged(nbx, generated, dim, depth):
    """far_correction and far_sums called as before (no law, no eps), and with law="reference" spelled out, give today's arrays."""
    b = generated[dim]
    s = nbx.leaves.octree_cells(b, dim, depth, 0.5)
    lo, lb, fo, fc = (np.asarray(a, dtype=np.int64) for a in (s[0], s[1], s[6], s[7]))
    mom = nbx.leaves.cell_moments(b, dim, lo, lb, s[4], s[5])
    rng = np.random.default_rng(3)
    R = rng.uniform(5.0, 9.0, (40, dim)) * rng.choice((-1.0, 1.0), (40, dim))
    M, Q = rng.uniform(0.0, 3.0, 40) * (rng.uniform(size=40) > 0.2), rng.uniform(-1.0, 1.0, (40, dim * (dim + 1) // 2))
    want = _far_correction_today(R, M, Q)
    assert np.array_equal(nbx.leaves.far_correction(R, M, Q), want)
    assert np.array_equal(nbx.leaves.far_correction(R, M, Q, law="reference", eps=7.0), want), "the reference law never reads eps"
    assert not np.array_equal(nbx.leaves.far_correction(R, M, Q, law="newton", eps=0.0), want)
    for order in (0, 1):
        want = _far_sums_today(b, dim, lo, lb, mom, fo, fc, order)
        assert np.abs(want).max() > 0
        assert np.array_equal(nbx.leaves.far_sums(b, dim, lo, lb, s[4], s[5], fo, fc, order=order), want), order
        assert np.array_equal(nbx.leaves.far_sums(b, dim, lo, lb, s[4], s[5], fo, fc, order, mom, "reference", 5.0), want), order
    with pytest.raises(ValueError):
        nbx.leaves.far_sums(b, dim, lo, lb, s[4], s[5], fo, fc, law="plummer")


def test_near_sums_is_the_all_pairs_sum_on_a_complete_structure(nbx, generated):
    """Every leaf on every list: near_sums is the all-pairs Newtonian sum; a body in no leaf and a coincident pair get what the law
    says (zeros; no contribution)."""
    b = generated[3][:700].copy()
    b[11, :3] = b[10, :3]                                             # a coincident pair: adds exactly 0 to each other
    leaves = nbx.leaves.all_pairs_leaves(700, 33)
    sums, S = nbx.leaves.near_sums(b, 3, *leaves, 2048.0)
    ref = all_pairs_newton(b, 3, 2048.0)
    assert np.allclose(sums, ref, rtol=1e-12, atol=0.0) and (S > 0).all()
    # the last body taken out of its leaf: no target any more (zeros) and no source either
    lo, lb, so, ss = (np.asarray(a).copy() for a in leaves)
    lo[-1] -= 1
    sums2, S2 = nbx.leaves.near_sums(b, 3, lo, lb[:-1], so, ss, 2048.0)
    assert not sums2[699].any() and S2[699] == 0.0, "a body in no leaf gets zeros"
    assert np.allclose(sums2[:699], all_pairs_newton(b[:699], 3, 2048.0), rtol=1e-12, atol=0.0)


def test_abi_entries_and_python_members(nbx):
    """The two entry points are exported and typed, a null plan is NBX_ERR_INVALID with the argument named, LAW_NEWTON is 3, LeafPlan
    carries set_softening and the softening property, and the ABI version is still 5."""
    typed = {name: (res, args) for name, res, args in nbx.ABI}
    assert typed["nbx_leaf_plan_set_softening"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double])
    assert typed["nbx_leaf_plan_get_softening"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)])
    lib = nbx.load_library()
    eps = ctypes.c_double(7.0)
    for rc in (lib.nbx_leaf_plan_set_softening(None, 1.0), lib.nbx_leaf_plan_get_softening(None, ctypes.byref(eps))):
        assert rc == 1
        assert b"plan" in lib.nbx_last_error_detail()
    assert eps.value == 7.0
    assert nbx.LAW_NEWTON == 3 and (nbx.LAW_BRUTE, nbx.LAW_TREE_LEAF, nbx.LAW_FMM_P2P) == (0, 1, 2)
    assert callable(nbx.LeafPlan.set_softening) and isinstance(nbx.LeafPlan.softening, property)
    assert lib.nbx_abi_version() == 5
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbody_hip.h")).read()
    assert "NBX_LAW_NEWTON = 3 };" in header
    assert "int nbx_leaf_plan_set_softening(nbx_leaf_plan* plan, double epsilon);" in header
    assert "int nbx_leaf_plan_get_softening(const nbx_leaf_plan* plan, double* epsilon);" in header
    # the one-shot call has no plan to carry a softening length: law 3 is refused before anything else is looked at
    b = np.zeros((2, 7))
    z = np.zeros(2, dtype=np.uint32)
    rc = lib.nbx_leaf_pair_forces(b.ctypes.data, 2, 3, 56, z.ctypes.data, z.ctypes.data, 0, z.ctypes.data, z.ctypes.data, 3, 1.0, 0, b.ctypes.data, None)
    assert rc == 1 and b"NBX_LAW_NEWTON" in lib.nbx_last_error_detail()
