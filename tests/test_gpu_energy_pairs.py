"""GPU: the all-pairs energy (nbx_ctx_energy / nbx_node_energy: potential_kernel<D, SOFT>, energy_partials_kernel) pair by pair at
every edge of its tiling, on the inputs of tests/energy_case.py (the certificate that a single wrong pair term cannot pass these
checks is asserted in tests/test_energy_case_cpu.py):

  1. sparse-mass probes, one per placement class (two entries of a tile; one lane's two targets; neighbouring workgroups; tile and
     workgroup edges; a slice edge beside a chunk edge; the same local index in different shards; the first and last body of
     ragged and padded shards), under the reference law, the softened law at eps below and above the separations and the
     Newtonian law, D = 2 and 3: EVERY SHARD'S share by itself, then the sum;
  2. the same placements with two heavy bodies exactly coincident, just below and just above the reference's skip threshold;
  3. dense inputs on partitions with one-body and empty shards: every share, a one-body share being one body's phi;
  4. bit-exact repeatability and independence from the force path.

Tolerances (energy_case.PE_TOL, SMALL_SHARE_TOL, KE_TOL, derived there): potential 2e-6 relative -- the project's energy tolerance;
shares of fewer than 64 bodies the worst case of one fp32 tile sum, (256 + 8) 2^-24 = 1.57e-5; a share that holds no heavy body
is an absolute zero; kinetic 1e-13."""
import numpy as np
import pytest

import energy_case as ec

pytestmark = pytest.mark.gpu

PROBE_LAWS = (("reference", 0.0), ("softened", ec.EPS_BELOW), ("softened", ec.EPS_ABOVE), ("newton", ec.EPS_BELOW))
PAIR_LAWS = (("reference", 0.0), ("softened", ec.PAIR_EPS_BELOW), ("softened", ec.PAIR_EPS_ABOVE), ("newton", ec.PAIR_EPS_BELOW))


def _set_law(c, nbx, law, eps):
    c.set_law(nbx.FORCE_LAW_REFERENCE)                      # (the Newtonian law refuses eps = 0: leave it first)
    c.set_softening(eps)
    if law == "newton":
        c.set_law(nbx.FORCE_LAW_NEWTON)


def _device_shares(nbx, b, n_shards, laws, G):
    """{(law, eps): [n_shards, 2]}: every shard's (kinetic, potential), one context per shard, all laws on the same upload."""
    n, dim = b.shape[0], (b.shape[1] - 1) // 2
    lay, cnts = ec.layout(n, n_shards), ec.counts(n, n_shards)
    out = {k: np.zeros((n_shards, 2)) for k in laws}
    for g in range(n_shards):
        with nbx.Context(n, dim, n_shards=n_shards, shard=g) as c:
            assert (c.shard_len, c.shard_pad, c.count) == (lay["shard_len"], lay["pad"], cnts[g]), "energy_case.layout is not the library's"
            c.upload(b)
            for law, eps in laws:
                _set_law(c, nbx, law, eps)
                out[(law, eps)][g] = c.energy(G)
    return out


def _check_shares(got, ref, tols, total_tol, what, worst):
    """got, ref: [n_shards, 2].  Every shard's potential to its tolerance (absolute zero where the reference is), the sum to
    total_tol, kinetic energies to KE_TOL; the largest error / tolerance goes into worst[0]."""
    for g in range(ref.shape[0]):
        assert abs(got[g, 0] - ref[g, 0]) <= ec.KE_TOL * ref[g, 0], f"{what}: kinetic share of shard {g}: {got[g, 0]!r} != {ref[g, 0]!r}"
        if ref[g, 1] == 0.0:
            assert got[g, 1] == 0.0, f"{what}: shard {g} holds nothing that weighs: its share must be 0, not {got[g, 1]!r}"
        else:
            r = abs(got[g, 1] - ref[g, 1]) / (tols[g] * abs(ref[g, 1]))
            worst[0] = max(worst[0], r)
            assert r <= 1.0, f"{what}: potential share of shard {g}: {got[g, 1]!r} != {ref[g, 1]!r}: {r:.3g} tolerances of {tols[g]:.3g}"
    ke, pe, ke_ref, pe_ref = got[:, 0].sum(), got[:, 1].sum(), ref[:, 0].sum(), ref[:, 1].sum()
    assert abs(ke - ke_ref) <= ec.KE_TOL * ke_ref, f"{what}: kinetic energy {ke!r} != {ke_ref!r}"
    if pe_ref == 0.0:
        assert pe == 0.0, f"{what}: potential energy {pe!r} must be 0"
    else:
        r = abs(pe - pe_ref) / (total_tol * abs(pe_ref))
        worst[0] = max(worst[0], r)
        assert r <= 1.0, f"{what}: potential energy {pe!r} != {pe_ref!r}: {r:.3g} tolerances of {total_tol:.3g}"


@pytest.mark.parametrize("dim", (3, 2))
@pytest.mark.parametrize("name", list(ec.PROBES))
def test_sparse_probe_every_share_and_the_sum(nbx, oracle, name, dim):
    n, n_shards, heavy = ec.PROBES[name]
    b = ec.probe_bodies(name, dim)
    got = _device_shares(nbx, b, n_shards, PROBE_LAWS, oracle.G)
    refs = ec.shares_of_laws(b, n_shards, PROBE_LAWS, oracle.G)
    worst = [0.0]
    for law, eps in PROBE_LAWS:
        ref = refs[(law, eps)]
        assert np.count_nonzero(ref[:, 1]) == len(set(ec.places(n, n_shards, heavy).shard))
        _check_shares(got[(law, eps)], ref, [ec.PE_TOL] * n_shards, ec.PE_TOL,
                      f"{name} {dim}D {law} eps={eps:g}; heavy bodies {ec.report(n, n_shards, heavy)}", worst)
    print(f"\n{name} {dim}D: worst potential error / tolerance {worst[0]:.3g}")


@pytest.mark.parametrize("dim", (3, 2))
@pytest.mark.parametrize("name", list(ec.PAIR_PROBES))
def test_coincident_and_threshold_pairs(nbx, oracle, name, dim):
    """Two heavy bodies 0, 83 and 84 fp32 spacings apart at coordinate 1 (r^2 = 0, 0.979e-10, 1.003e-10).  Reference law: the first two
    contribute exactly nothing -- the energy is that of the input with either body massless, 0 --, the third its G m m / (2 r^2);
    the softened laws count all three, the coincident pair as m m / eps^2 (m m / eps)."""
    n, n_shards, ia, ib = ec.PAIR_PROBES[name]
    worst = [0.0]
    for sep in ec.SEPARATIONS:
        b = ec.pair_bodies(name, sep, dim)
        got = _device_shares(nbx, b, n_shards, PAIR_LAWS, oracle.G)
        refs = ec.shares_of_laws(b, n_shards, PAIR_LAWS, oracle.G)
        for law, eps in PAIR_LAWS:
            ref = refs[(law, eps)]
            assert (ref[:, 1].sum() != 0.0) == (law != "reference" or sep == "above")
            _check_shares(got[(law, eps)], ref, [ec.PE_TOL] * n_shards, ec.PE_TOL,
                          f"{name} {sep} {dim}D {law} eps={eps:g}; the pair {ec.report(n, n_shards, (ia, ib))}", worst)
        if sep != "above":                                  # the skipped pair's comparison input, on the device as well: 0 == 0
            for m in ("A", "B"):
                lone = _device_shares(nbx, ec.pair_bodies(name, sep, dim, massless=m), n_shards, PAIR_LAWS[:2], oracle.G)
                for k in PAIR_LAWS[:2]:
                    assert not lone[k][:, 1].any(), f"{name} {sep} {dim}D: one massive body alone has no potential energy under {k}"
                assert np.array_equal(lone[PAIR_LAWS[0]][:, 1], got[PAIR_LAWS[0]][:, 1]), f"{name} {sep} {dim}D: body {m} massless"
    print(f"\n{name} {dim}D: worst potential error / tolerance {worst[0]:.3g}")


@pytest.mark.parametrize("dim", (3, 2))
@pytest.mark.parametrize("name", list(ec.DENSE))
def test_dense_shares_one_body_and_empty_shards_among_them(nbx, oracle, name, dim):
    """Every shard's share of a dense input.  Shares of >= 64 bodies: 2e-6.  Smaller ones, down to the ONE-BODY share (a single
    phi_i seen through the API): the worst-case bound of the kernel's fp32 level, (kTile + 8) 2^-24 = 1.57e-5 -- a sequential sum
    of 256 non-negative terms per tile.  The bound is not tightened to what is observed; the observed ratio to it is printed
    (DESIGN.md section 4 records the figures of the run that introduced this test)."""
    n, n_shards = ec.DENSE[name][:2]
    assert oracle.G == ec.G_REFERENCE
    b = ec.dense_bodies(name, dim)
    cnts = ec.counts(n, n_shards)
    tols = [ec.share_tolerance(c) for c in cnts]
    total_tol = ec.PE_TOL if n >= ec.SMALL_SHARE_BODIES else ec.SMALL_SHARE_TOL
    got = _device_shares(nbx, b, n_shards, PROBE_LAWS, oracle.G)
    refs = ec.shares_of_laws(b, n_shards, PROBE_LAWS, oracle.G)     # every r^2 once, for all four laws
    worst, worst_one = [0.0], 0.0
    for law, eps in PROBE_LAWS:
        ref = refs[(law, eps)]
        for g, c in enumerate(cnts):
            if c == 0:
                assert ref[g, 0] == 0.0 and ref[g, 1] == 0.0
            if c == 1:
                worst_one = max(worst_one, abs(got[(law, eps)][g, 1] - ref[g, 1]) / (ec.SMALL_SHARE_TOL * abs(ref[g, 1])))
        _check_shares(got[(law, eps)], ref, tols, total_tol, f"{name} {dim}D {law} eps={eps:g}, shard sizes {cnts}", worst)
    print(f"\n{name} {dim}D: shard sizes {cnts}; worst potential error / tolerance {worst[0]:.3g}"
          + (f"; one-body shares: worst error / (264 * 2^-24) = {worst_one:.3g}" if 1 in cnts else ""))


# ---- structure-independence: bit-exact ---------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@pytest.mark.parametrize("dim", (3, 2))
def test_energy_is_repeatable_and_leaves_the_force_path_alone(nbx, oracle, dim):
    n, dt = 3000, 2.0
    G = oracle.G * 1e24                                     # strong enough for one step to move the bodies
    b = ec.generated(n, dim, 58)
    for law, eps in PROBE_LAWS[:2] + PROBE_LAWS[3:]:
        stepped = []
        for with_energy in (False, True):
            with nbx.Context(n, dim) as c:
                c.upload(b)
                _set_law(c, nbx, law, eps)
                if with_energy:
                    e0 = c.energy(G)
                    assert np.array_equal(_bits(e0), _bits(c.energy(G))), f"{law}: energy() twice"
                    c.compute_accel()
                    f0 = c.forces(G)
                    assert np.array_equal(_bits(e0), _bits(c.energy(G))), f"{law}: energy() after a force evaluation"
                    assert np.array_equal(_bits(f0), _bits(c.forces(G))), f"{law}: forces() after energy()"
                c.step(dt, 1, G)
                out = b.copy()
                c.download(out)
                stepped.append(out)
        assert np.abs(stepped[0][:, dim:2 * dim] - b[:, dim:2 * dim]).max() > 0.0 and not np.array_equal(stepped[0][:, :dim], b[:, :dim])
        assert np.array_equal(_bits(stepped[0]), _bits(stepped[1])), f"{law}: a step after energy() differs from the step without it"


@pytest.mark.parametrize("ranks,dim", ((2, 3), (4, 3), (4, 2)))
def test_node_energy_is_the_sum_of_its_ranks_shares(nbx, oracle, ranks, dim):
    """nbx_node_energy on virtual ranks of device 0 against plain sharded contexts: the same bits, the ranks added in rank order."""
    n = 3001
    b = ec.generated(n, dim, 59)
    for law, eps in (PROBE_LAWS[0], PROBE_LAWS[1], PROBE_LAWS[3]):
        want = np.zeros(2)
        for row in _device_shares(nbx, b, ranks, ((law, eps),), oracle.G)[(law, eps)]:
            want += row
        with nbx.Node(n, dim, [0] * ranks) as node:
            node.upload(b)
            if law != "reference":
                node.set_softening(eps)
            if law == "newton":
                node.set_law(nbx.FORCE_LAW_NEWTON)
            got = node.energy(oracle.G)
            again = node.energy(oracle.G)
        assert np.array_equal(_bits(got), _bits(want)), f"{ranks} ranks {law}: node {got!r}, contexts {tuple(want)!r}"
        assert np.array_equal(_bits(got), _bits(again))
        ref = ec.shares(b, 1, law, eps, oracle.G)[0]
        assert abs(got[0] - ref[0]) <= 1e-13 * ref[0] and abs(got[1] - ref[1]) <= ec.PE_TOL * abs(ref[1])
