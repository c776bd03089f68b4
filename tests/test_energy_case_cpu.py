"""CPU: the inputs of the pair-by-pair energy tests (tests/energy_case.py) are what they claim to be.  The certificate -- a kernel
with one modelled fault (a pair counted from one side, a wrong own-entry exclusion, a misplaced skip rule, a tile lost at a
slice or chunk edge, rotated shares) misses the tolerances of tests/test_gpu_energy_pairs.py by a factor of 100 or more on every
probe it touches, 10 or more for a single term of a one-body share -- is asserted from the fp64 specification alone; the
specification is pinned to the oracle's energies; where() is pinned to hand-worked cases and to a port of the kernel's own
index expressions."""
import numpy as np
import pytest

import energy_case as ec

FLOOR, FLOOR_ONE_BODY = 100.0, 10.0
PROBE_LAWS = (("reference", 0.0), ("softened", ec.EPS_BELOW), ("softened", ec.EPS_ABOVE), ("newton", ec.EPS_BELOW))
PAIR_LAWS = (("reference", 0.0), ("softened", ec.PAIR_EPS_BELOW), ("softened", ec.PAIR_EPS_ABOVE), ("newton", ec.PAIR_EPS_BELOW))


def _worst(models, ref, **kw):
    return {f: min((ec.miss(s, ref, **kw), label) for label, s in variants) for f, variants in models.items()}


def test_where_reproduces_hand_worked_cases():
    P = ec.Place
    assert ec.layout(12000, 3) == {"shard_len": 4000, "pad": 4096, "tiles_per_chunk": 16, "tiles_per_split": 3}
    assert ec.where(12000, 3, 3839) == P(shard=0, local=3839, tile=14, entry=255, slice=4, wg=7, q=0)     # last tile of slice 4
    assert ec.where(12000, 3, 3840) == P(shard=0, local=3840, tile=15, entry=0, slice=5, wg=7, q=1)       # first tile of slice 5
    assert ec.where(12000, 3, 3999) == P(shard=0, local=3999, tile=15, entry=159, slice=5, wg=7, q=1)     # last body of chunk 0
    assert ec.where(12000, 3, 4000) == P(shard=1, local=0, tile=16, entry=0, slice=5, wg=0, q=0)          # chunk 1, same slice
    assert ec.where(12000, 3, 4511) == P(shard=1, local=511, tile=17, entry=255, slice=5, wg=0, q=1)
    assert ec.where(12000, 3, 4512) == P(shard=1, local=512, tile=18, entry=0, slice=6, wg=1, q=0)
    assert ec.where(12000, 3, 8356) == P(shard=2, local=356, tile=33, entry=100, slice=11, wg=0, q=1)
    assert ec.layout(3000, 1)["tiles_per_split"] == 1
    assert ec.where(3000, 1, 517) == P(shard=0, local=517, tile=2, entry=5, slice=2, wg=1, q=0)
    assert ec.where(3000, 1, 773) == P(shard=0, local=773, tile=3, entry=5, slice=3, wg=1, q=1)
    assert ec.layout(12298, 3) == {"shard_len": 4100, "pad": 8192, "tiles_per_chunk": 32, "tiles_per_split": 6}
    assert ec.where(12298, 3, 12297) == P(shard=2, local=4097, tile=80, entry=1, slice=13, wg=8, q=0)
    assert ec.counts(12298, 3) == [4100, 4100, 4098] and ec.counts(4795, 8) == [600] * 7 + [595]
    assert ec.layout(8195, 1) == {"shard_len": 8195, "pad": 12288, "tiles_per_chunk": 48, "tiles_per_split": 3}
    assert ec.where(8195, 1, 8194) == P(shard=0, local=8194, tile=32, entry=2, slice=10, wg=16, q=0)
    assert ec.layout(57, 8)["shard_len"] == 8 and ec.counts(57, 8) == [8] * 7 + [1]
    assert ec.where(57, 8, 56) == P(shard=7, local=0, tile=112, entry=0, slice=14, wg=0, q=0)
    assert ec.counts(5, 8) == [1] * 5 + [0] * 3
    assert ec.layout(8192, 1)["pad"] == 8192 and ec.layout(4097, 1)["pad"] == 8192 and ec.layout(1, 8)["pad"] == 4096
    assert ec.SMALL_SHARE_TOL == 264 * 2.0 ** -24 and ec.PE_TOL == 2e-6


def _kernel_index_logic(n, n_shards, i, chunk_test=True, q_test=True):
    """potential_kernel's index expressions for target body i, restated line by line: the workgroups (bx, by) of i's shard walk the
    virtual tile list slice by slice (TileWalk::seek / next), `rel = w.k - bx * TPL` in unsigned arithmetic, `own_tile = chunk ==
    tgt_chunk && rel < TPL`, the excluded entry `q == rel && j == tid`.  Returns (slots visited as [(chunk, local)] with repeats,
    excluded bodies).  chunk_test / q_test = False leave that comparison out: the mutations of fault models 2 and 3."""
    lay, p = ec.layout(n, n_shards), ec.where(n, n_shards, i)
    tpc, tps, TPL = lay["tiles_per_chunk"], lay["tiles_per_split"], 2
    total = n_shards * tpc
    bx, tid = p.wg, p.entry
    tiles, excluded = [], []
    for by in range(ec.PHI_SLICES):
        t, t_end = by * tps, min(by * tps + tps, total)
        vc, k = divmod(t, tpc)                                    # seek
        while t < t_end:
            rel = (k - bx * TPL) % (1 << 32)
            own_tile = (vc == p.shard or not chunk_test) and rel < TPL
            tiles.append((vc, k))
            if own_tile and (p.q == rel or not q_test):
                local = k * ec.K_TILE + tid
                if local < lay["shard_len"] and vc * lay["shard_len"] + local < n:
                    excluded.append(vc * lay["shard_len"] + local)
            t += 1
            k += 1                                                # next
            if k == tpc:
                k, vc = 0, vc + 1
    return tiles, sorted(excluded)


@pytest.mark.parametrize("name", list(ec.PROBES) + list(ec.PAIR_PROBES))
def test_kernel_index_logic_and_its_mutations_are_what_the_fault_models_say(name):
    """The restated index logic visits every tile of every chunk exactly once and excludes body i alone; without the chunk
    comparison it excludes the same local index in every shard, without the q comparison body i +- 256 of the workgroup: the
    pairs fault models 2 and 3 take away."""
    spec = ec.PROBES.get(name) or ec.PAIR_PROBES[name]
    n, n_shards, heavy = spec[0], spec[1], (spec[2] if name in ec.PROBES else spec[2:])
    lay = ec.layout(n, n_shards)
    P = ec.places(n, n_shards, heavy)
    for a, i in enumerate(heavy):
        tiles, excluded = _kernel_index_logic(n, n_shards, i)
        assert sorted(tiles) == [(c, k) for c in range(n_shards) for k in range(lay["tiles_per_chunk"])]
        assert excluded == [i]
        _, no_chunk = _kernel_index_logic(n, n_shards, i, chunk_test=False)
        want = sorted(g * lay["shard_len"] + int(P.local[a]) for g in range(n_shards) if g * lay["shard_len"] + int(P.local[a]) < n)
        assert no_chunk == want
        _, no_q = _kernel_index_logic(n, n_shards, i, q_test=False)
        twin = i + ec.K_TILE * (1 - 2 * int(P.q[a]))
        assert no_q == sorted(j for j in (i, twin) if int(P.shard[a]) * lay["shard_len"] <= j < min(n, (int(P.shard[a]) + 1) * lay["shard_len"]))
    # ... and the fault models drop exactly those pairs among the heavy bodies
    b = ec.probe_bodies(name, 3) if name in ec.PROBES else ec.pair_bodies(name, "above", 3)
    ref, models = ec.fault_models(b, n_shards, "softened", 1.0e-3)
    T, _ = ec.pair_terms(b, heavy, heavy, "softened", 1.0e-3)
    f = ec.pe_factor("softened", ec.G_REFERENCE)
    for fault, kw in (("own_tile_without_chunk_test", {"chunk_test": False}), ("own_tile_without_q_test", {"q_test": False})):
        Tm = T.copy()
        for a, i in enumerate(heavy):
            for j in _kernel_index_logic(n, n_shards, i, **kw)[1]:
                if j in heavy:
                    Tm[a, list(heavy).index(j)] = 0.0
        want = np.array([(f * b[list(heavy), -1] * Tm.sum(1))[P.shard == g].sum() for g in range(n_shards)])
        if np.array_equal(Tm, T):
            assert fault not in models
        else:
            assert len(models[fault]) == 1 and np.allclose(models[fault][0][1], want, rtol=1e-14, atol=0)


def test_every_fault_model_applies_to_some_probe():
    seen = set()
    for name, (n, n_shards, heavy) in ec.PROBES.items():
        for law, eps in PROBE_LAWS:
            seen |= set(ec.fault_models(ec.probe_bodies(name, 3), n_shards, law, eps)[1])
    assert seen == set(ec.FAULTS) - {"skip_under_softened_law", "no_skip_under_reference_law"}     # (those: the threshold pairs)
    applies = {}
    for name, (n, n_shards, ia, ib) in ec.PAIR_PROBES.items():
        for law, eps in PAIR_LAWS:
            for f in ec.fault_models(ec.pair_bodies(name, "below", 3), n_shards, law, eps)[1]:
                applies.setdefault(f, set()).add(name)
    assert applies["skip_under_softened_law"] == applies["no_skip_under_reference_law"] == set(ec.PAIR_PROBES)
    assert applies["own_tile_without_chunk_test"] == {"pair_same_local"} and applies["own_tile_without_q_test"] == {"pair_lane"}
    # the placement classes: what each probe's name promises
    P = {name: ec.places(n, g, heavy) for name, (n, g, heavy) in ec.PROBES.items()}
    assert len(set(P["one_tile"].tile)) == 1 and len(set(P["one_tile_sharded"].tile)) == 1
    for name in ("lane_pair", "lane_pair_sharded"):
        p = P[name]
        assert (p.shard[0], p.wg[0], p.entry[0]) == (p.shard[1], p.wg[1], p.entry[1]) and (p.q[0], p.q[1]) == (0, 1)
    for name in ("next_workgroup", "next_workgroup_sharded"):
        p = P[name]
        assert len(set(p.entry)) == 1 and len(set(p.q)) == 1 and list(p.wg) == [0, 1, 2] and len(set(p.shard)) == 1
    for name, first in (("tile_and_workgroup_edges", 0), ("tile_and_workgroup_edges_sharded", 32)):
        p = P[name]
        assert list(p.entry) == [255, 0, 255, 0] and list(p.tile - first) == [0, 1, 1, 2] and list(p.wg) == [0, 0, 0, 1]
    p = P["slice_edges_one_shard"]
    assert list(p.tile) == [2, 3, 5, 6] and list(p.slice) == [0, 1, 1, 2] and list(p.entry) == [255, 0, 255, 0]
    p = P["slice_edge_into_chunk_edge"]
    assert list(p.tile) == [14, 15, 16] and list(p.slice) == [4, 5, 5] and list(p.shard) == [0, 0, 1]
    p = P["chunk_edge_out_of_slice"]
    assert list(p.tile) == [15, 17, 18] and list(p.slice) == [5, 5, 6] and list(p.shard) == [0, 1, 1]
    p = P["same_local_index"]
    assert list(p.shard) == [0, 1, 2] and list(p.local) == [100, 100, 356]
    p = P["same_local_index_minus"]
    assert list(p.shard) == [0, 1, 2] and list(p.local) == [356, 100, 100]
    for name in ("ends_padded_to_8192", "ends_eight_shards", "ends_one_shard"):
        n, g, heavy = ec.PROBES[name]
        assert heavy[0] == 0 and heavy[-1] == n - 1 and ec.counts(n, g)[-1] % 64 != 0
    assert ec.layout(*ec.PROBES["ends_padded_to_8192"][:2])["pad"] == 8192 and ec.layout(*ec.PROBES["ends_padded_to_8192"][:2])["tiles_per_split"] >= 2


@pytest.mark.parametrize("name", list(ec.PROBES))
def test_fault_margins_and_pair_shares_of_the_sparse_probes(name):
    n, n_shards, heavy = ec.PROBES[name]
    assert 2 <= len(heavy) <= 8 and n <= 8195 or (n_shards <= 8 and 4096 <= ec.layout(n, n_shards)["pad"] <= 8192)
    print(f"\n{name}: n={n}, {n_shards} shard(s); heavy {ec.report(n, n_shards, heavy)}")
    for dim in (2, 3):
        b = ec.probe_bodies(name, dim)
        assert ec.is_f32_input(b, dim) and sorted(np.flatnonzero(b[:, -1])) == sorted(heavy)
        for law, eps in PROBE_LAWS:
            sep = np.sqrt(ec.pair_terms(b, heavy, heavy, law, eps)[1][np.triu_indices(len(heavy), 1)])
            assert ec.EPS_BELOW < 0.02 * sep.min() and ec.EPS_ABOVE > 20 * sep.max()
            share = ec.pair_shares(b, law, eps)
            assert len(share) == len(heavy) * (len(heavy) - 1) // 2 and min(share.values()) >= 0.01, (dim, law, eps, share)
            ref, models = ec.fault_models(b, n_shards, law, eps)
            assert np.allclose(ref, ec.shares(b, n_shards, law, eps)[:, 1], rtol=1e-14, atol=0)
            worst = _worst(models, ref)
            print(f"    {dim}D {law:9s} eps={eps:g}: smallest pair share {min(share.values()):.3f}; error / tolerance: "
                  + ", ".join(f"{f} {w:.3g}" for f, (w, _) in worst.items()))
            assert "one_sided" in worst and ("self_term_included" in worst) == (law != "reference")
            for f, (w, label) in worst.items():
                assert w >= FLOOR, (name, dim, law, eps, f, label, w)


@pytest.mark.parametrize("name", list(ec.PAIR_PROBES))
def test_fault_margins_of_the_coincident_and_threshold_pairs(name):
    n, n_shards, ia, ib = ec.PAIR_PROBES[name]
    for dim in (2, 3):
        for sep, dx in ec.SEPARATIONS.items():
            b = ec.pair_bodies(name, sep, dim)
            assert ec.is_f32_input(b, dim) and list(np.flatnonzero(b[:, -1])) == [ia, ib]
            d = b[ib, :dim] - b[ia, :dim]
            assert np.count_nonzero(d) == (sep != "coincident") and d.sum() == dx and b[ia, :dim].min() == 1.0
            r2_f32 = float(np.float32(np.float32(d.sum()) * np.float32(d.sum())))
            assert (r2_f32 < ec.R2_SKIP) == ((d * d).sum() < ec.R2_SKIP) == (sep != "above")
            for law, eps in PAIR_LAWS:
                ref, models = ec.fault_models(b, n_shards, law, eps)
                worst = _worst(models, ref)
                counted = law != "reference" or sep == "above"
                assert (ref.sum() != 0.0) == counted
                if counted:
                    assert "one_sided" in worst
                    # the pair's term is the whole energy: m_i m_j u(r^2), with the API's factor
                    u = 1.0 / (dx * dx + eps * eps) if law != "newton" else 1.0 / np.sqrt(dx * dx + eps * eps)
                    want = 2 * ec.pe_factor(law, ec.G_REFERENCE) * ec.HEAVY_MASSES[0] * ec.HEAVY_MASSES[1] * u
                    assert abs(ref.sum() - want) <= 1e-14 * abs(want)
                else:
                    assert list(worst) == ["no_skip_under_reference_law"]
                    for m in ("A", "B"):                          # ... as if one of the two had no mass
                        assert not ec.shares(ec.pair_bodies(name, sep, dim, massless=m), n_shards, law, eps)[:, 1].any()
                assert ("skip_under_softened_law" in worst) == (law != "reference" and sep != "above")
                for f, (w, label) in worst.items():
                    assert w >= FLOOR, (name, sep, dim, law, eps, f, label, w)


@pytest.mark.parametrize("name", [k for k in ec.DENSE if 1 in ec.counts(*ec.DENSE[k][:2])])
def test_no_term_of_a_one_body_share_is_too_small_to_see(name):
    """A one-body shard's share is that body's phi: a single term missing from it (and a tile lost at a slice or chunk edge,
    where one applies) must miss the worst-case tolerance of a single fp32 sum by a factor of 10 or more."""
    n, n_shards = ec.DENSE[name][:2]
    cnts, sl = ec.counts(n, n_shards), ec.layout(n, n_shards)["shard_len"]
    assert 1 in cnts and (name != "n5_g8" or 0 in cnts)
    for dim in (2, 3):
        b = ec.dense_bodies(name, dim)
        assert ec.is_f32_input(b, dim) and (b[:, -1] > 0).all()
        for law, eps in PROBE_LAWS:
            full = ec.shares(b, n_shards, law, eps)[:, 1]
            least = float("inf")
            for g in (g for g, c in enumerate(cnts) if c == 1):
                ref, models = ec.fault_models(b, n_shards, law, eps, rows=[g * sl])
                assert abs(ref[g] - full[g]) <= 1e-14 * abs(full[g]) and ec.share_tolerance(1) == ec.SMALL_SHARE_TOL
                assert len(models["one_sided"]) == n - 1
                for f in ec.DROPPED_TERM_FAULTS:
                    for label, s in models.get(f, []):
                        w = abs(s[g] - ref[g]) / (ec.SMALL_SHARE_TOL * abs(ref[g]))
                        least = min(least, w)
                        assert w >= FLOOR_ONE_BODY, (name, dim, law, eps, g, f, label, w)
            print(f"\n{name} {dim}D {law} eps={eps:g}: smallest dropped term / tolerance {least:.3g}")


@pytest.mark.parametrize("dim", (3, 2))
def test_the_specification_is_the_oracles_energy(oracle, dim):
    assert oracle.G == ec.G_REFERENCE
    inputs = [(name, ec.probe_bodies(name, dim), spec[1], PROBE_LAWS) for name, spec in ec.PROBES.items()]
    inputs += [(f"{name} {sep}", ec.pair_bodies(name, sep, dim), spec[1], PAIR_LAWS) for name, spec in ec.PAIR_PROBES.items() for sep in ec.SEPARATIONS]
    inputs += [(name, ec.dense_bodies(name, dim), spec[1], PROBE_LAWS) for name, spec in ec.DENSE.items()]
    for k, (name, b, n_shards, laws) in enumerate(inputs):
        assert np.array_equal(b, oracle.round_inputs_to_f32(b))
        if b.shape[0] > 8195:                                    # the oracle is O(N^2) over the massless bodies too: the 12,000-body
            laws = (laws[k % 4], laws[(k + dim - 1) % 4])        # inputs take two of the four settings each, in rotation
        for law, eps in laws:
            ke_ref, pe_ref = oracle.energy(b) if law == "reference" else oracle.energy_softened(b, eps, newton=(law == "newton"))
            s = ec.shares(b, n_shards, law, eps, oracle.G)
            assert s.shape == (n_shards, 2)
            assert abs(s[:, 0].sum() - ke_ref) <= 1e-12 * ke_ref and abs(s[:, 1].sum() - pe_ref) <= 1e-12 * abs(pe_ref), (name, law, eps)
            assert (pe_ref < 0) == (law == "newton" and pe_ref != 0)
            if b.shape[0] < 8195 or law == "reference":          # per_body_phi is the same specification, body by body
                per_body = ec.pe_factor(law, oracle.G) * b[:, -1] * ec.per_body_phi(b, law, eps)
                sl = ec.layout(b.shape[0], n_shards)["shard_len"]
                for g in range(n_shards):
                    assert abs(per_body[g * sl:(g + 1) * sl].sum() - s[g, 1]) <= 1e-13 * abs(s[g, 1]), (name, law, eps, g)
