"""CPU: the fp64 specification of the potential through a leaf plan (nbody_amd.leaves.near_potentials, far_potential_correction,
far_potentials) and the three entry points' place in the C ABI (nbx_leaf_plan_potentials, _energy, _get_potentials).

The specification is what tests/test_gpu_tree_potential.py holds csrc/leaf_phi_kernel.hip to, so it is itself checked here against
things it shares nothing with: the laws' force terms (its gradient), the exact potential of a cluster (its order), and a direct
all-pairs sum (its partition of the sources)."""
import ctypes

import numpy as np
import pytest

from test_capi_cpu import _no_gpu, declared_symbols

NEW = ("nbx_leaf_plan_energy", "nbx_leaf_plan_get_potentials", "nbx_leaf_plan_potentials")
NBX_ERR_INVALID = 1


def _cluster(rng, dim):
    """40 bodies of masses 0.5-2 in a box, their moments about the centre of mass, and the cluster's radius."""
    x = rng.uniform(-1.0, 1.0, (40, dim))
    m = rng.uniform(0.5, 2.0, 40)
    M = m.sum()
    com = (m[:, None] * x).sum(axis=0) / M
    s = x - com
    pairs = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)) if dim == 3 else ((0, 0), (1, 1), (0, 1))
    Q = np.array([(m * s[:, a] * s[:, b]).sum() for a, b in pairs])
    return x, m, M, com, Q, float(np.linalg.norm(s, axis=1).max())


def _exact(x, m, p, newton, eps):
    r2 = ((x - p) ** 2).sum(axis=1)
    return (m / np.sqrt(r2 + eps * eps)).sum() if newton else (0.5 * m / r2).sum()


def _monopole_via_far_potentials(leaves, M, com, p, law, eps):
    """far_potentials' cell term at order 0 for ONE target at p and one cell (M, com): a two-leaf structure, leaf 0 the target."""
    dim = p.size
    b = np.zeros((2, 2 * dim + 1))
    b[0, :dim], b[0, -1] = p, 1.0
    b[1, :dim], b[1, -1] = com, M
    nq = dim * (dim + 1) // 2
    phi, S = leaves.far_potentials(b, dim, [0, 1, 2], [0, 1], [1], [1], [0, 1, 1], [0], order=0, law=law, eps=eps,
                                   moments=(np.array([M]), com[None, :], np.zeros((1, nq))))
    assert S[0] == abs(phi[0]) and phi[1] == 0.0
    return phi[0]


@pytest.mark.parametrize("eps", (0.0, 0.3))
@pytest.mark.parametrize("law", ("newton", "reference"))
@pytest.mark.parametrize("dim", (2, 3))
def test_gradient(nbx, dim, law, eps):
    """The central difference (step 2^-16 r) of far_potentials' cell term at order 0 and of far_potential_correction is M R w' (the
    force passes' monopole term) and leaves.far_correction, to 1e-6 of the larger magnitude: truncation <= (h / r)^2 7 8 9 / 6 = 2e-8,
    rounding ~1e-11.  Targets at 8 - 64 cell radii."""
    leaves = nbx.leaves
    rng = np.random.default_rng(100 * dim + (law == "newton") + int(10 * eps))
    newton = law == "newton"
    e = eps if newton else 0.0                     # the reference laws have no softening
    for _ in range(6):
        x, m, M, com, Q, radius = _cluster(rng, dim)
        for dist in (8.0, 20.0, 64.0):
            u = rng.normal(size=dim)
            p = com + dist * radius * u / np.linalg.norm(u)
            R = com - p
            r = np.linalg.norm(R)
            h = 2.0 ** -16 * r
            g0, g1 = np.zeros(dim), np.zeros(dim)
            for k in range(dim):
                d = np.zeros(dim)
                d[k] = h
                g0[k] = (_monopole_via_far_potentials(leaves, M, com, p + d, law, e) - _monopole_via_far_potentials(leaves, M, com, p - d, law, e)) / (2 * h)
                g1[k] = (leaves.far_potential_correction(com - (p + d), M, Q, law, e) - leaves.far_potential_correction(com - (p - d), M, Q, law, e)) / (2 * h)
            rho2 = r * r + e * e
            want0 = M * R / (rho2 * np.sqrt(rho2)) if newton else M * R / r ** 4
            want1 = leaves.far_correction(R, M, Q, law, e) if newton else leaves.far_correction(R, M, Q)
            for got, want in ((g0, want0), (g1, want1)):
                scale = max(np.abs(got).max(), np.abs(want).max())
                assert scale > 0 and np.abs(got - want).max() <= 1e-6 * scale, (dim, law, eps, dist, got, want)


@pytest.mark.parametrize("eps", (0.0, 0.3))
@pytest.mark.parametrize("law", ("newton", "reference"))
@pytest.mark.parametrize("dim", (2, 3))
def test_expansion_order(nbx, dim, law, eps):
    """The residual against the exact cluster potential, relative, per doubling of the distance over 32 -> 64 -> 128 radii: it falls
    by 3.5 - 4.6 at order 0 (asymptotically 4: the quadrupole is left out) and by 6.5 - 9.5 at order 1 (asymptotically 8)."""
    leaves = nbx.leaves
    rng = np.random.default_rng(7 + dim)
    newton = law == "newton"
    e = eps if newton else 0.0
    for _ in range(4):
        x, m, M, com, Q, radius = _cluster(rng, dim)
        u = rng.normal(size=dim)
        u /= np.linalg.norm(u)
        res = {0: [], 1: []}
        for dist in (32.0, 64.0, 128.0):
            p = com + dist * radius * u
            exact = _exact(x, m, p, newton, e)
            mono = _monopole_via_far_potentials(leaves, M, com, p, law, e)
            corr = float(leaves.far_potential_correction(com - p, M, Q, law, e))
            res[0].append(abs(mono - exact) / exact)
            res[1].append(abs(mono + corr - exact) / exact)
        for order, (lo, hi) in ((0, (3.5, 4.6)), (1, (6.5, 9.5))):
            ratios = [res[order][i] / res[order][i + 1] for i in range(2)]
            assert all(lo <= q <= hi for q in ratios), (dim, law, eps, order, ratios, res[order])


def _direct(b, dim, law, eps):
    x, m = b[:, :dim], b[:, -1]
    r2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
    if law == "newton":
        w = m[None, :] / np.sqrt(r2 + eps * eps)
        np.fill_diagonal(w, 0.0)
    else:
        keep = r2 >= (1e-10 if law == "brute" else 1e-9)
        w = np.where(keep, 0.5 * m[None, :] / np.where(keep, r2, 1.0), 0.0)
    return w.sum(axis=1), np.abs(w).sum(axis=1)


@pytest.mark.parametrize("law,eps", (("newton", 0.25), ("brute", 0.0), ("tree_leaf", 0.0)))
@pytest.mark.parametrize("dim", (2, 3))
def test_partition(nbx, dim, law, eps):
    """octree_cells / adaptive_octree_cells at theta = 0 put every leaf on every near list: near_potentials is then a direct all-pairs
    fp64 sum to 1e-12 relative per body -- a coincident pair included (counted as m_j / eps under NEWTON, skipped under the others) and
    every body listed in its own leaf (never counted)."""
    leaves = nbx.leaves
    rng = np.random.default_rng(30 + dim)
    n = 700
    b = np.zeros((n, 2 * dim + 1))
    b[:, :dim] = rng.uniform(-100.0, 100.0, (n, dim))
    b[:, -1] = rng.uniform(0.5, 2.0, n)
    b[41, :dim] = b[40, :dim]
    want, S_want = _direct(b, dim, law, eps)
    if law == "newton":
        assert want[40] >= b[41, -1] / eps and want[41] >= b[40, -1] / eps
    for what, arrays in (("fixed", leaves.octree_cells(b, dim, 3, 0.0)), ("adaptive", leaves.adaptive_octree_cells(b, dim, 6, 12, 0.0))):
        assert arrays[6][-1] == 0, "theta = 0 accepts nothing: no far entries"
        phi, S = leaves.near_potentials(b, dim, *arrays[:4], law, eps)
        assert np.abs(phi - want).max() <= 1e-12 * np.abs(want).max() and (np.abs(phi - want) <= 1e-12 * S_want).all(), what
        assert np.allclose(S, S_want, rtol=1e-12, atol=0.0)
        fphi, fS = leaves.far_potentials(b, dim, arrays[0], arrays[1], *arrays[4:], order=1, law=law, eps=eps)
        assert not fphi.any() and not fS.any()
    with pytest.raises(ValueError):
        leaves.near_potentials(b, dim, *arrays[:4], "fmm_p2p", 0.0)


def test_abi(nbx):
    """The three names are declared, bound and exported; null arguments are NBX_ERR_INVALID; without a device the calls fail loudly;
    the ABI version stays 5."""
    decl = declared_symbols()
    bound = {name: (res, args) for name, res, args in nbx.ABI}
    lib = ctypes.CDLL(nbx.LIB_PATH)
    for name in NEW:
        assert name in decl and name in bound and hasattr(lib, name), name
    assert len(bound["nbx_leaf_plan_potentials"][1]) == 5 and len(bound["nbx_leaf_plan_energy"][1]) == 6 and len(bound["nbx_leaf_plan_get_potentials"][1]) == 2
    for m in ("potentials", "energy", "get_potentials"):
        assert callable(getattr(nbx.LeafPlan, m))
    L = nbx.load_library()
    assert L.nbx_abi_version() == 5
    out = np.zeros(4)
    ke, pe = ctypes.c_double(), ctypes.c_double()
    assert L.nbx_leaf_plan_potentials(None, out.ctypes.data, 56, nbx.LAW_TREE_LEAF, out.ctypes.data) == NBX_ERR_INVALID
    assert L.nbx_leaf_plan_energy(None, None, nbx.LAW_TREE_LEAF, 1.0, ctypes.byref(ke), ctypes.byref(pe)) == NBX_ERR_INVALID
    assert L.nbx_leaf_plan_get_potentials(None, out.ctypes.data) == NBX_ERR_INVALID
    if _no_gpu(nbx):
        # no plan can be made without a device, so no potential call can be reached: the failure is loud, there is no CPU fallback
        b = np.zeros((4, 7))
        b[:, -1] = 1.0
        with pytest.raises(nbx.NbxError) as e:
            with nbx.LeafPlan(4, 3, *nbx.leaves.all_pairs_leaves(4, 2)) as plan:
                plan.potentials(b, nbx.LAW_TREE_LEAF)
        assert e.value.status == 2 and "no CPU fallback" in str(e.value)
