"""CPU: the conditions tests/test_gpu_close_cells.py rests on -- the inputs of close_cells_case.py really put a pair across
every boundary of the sorted-cell refinement, with r^2 well inside each kind's range, and bad_targets() (the definition of
the close-set list) counts exactly the planted bodies."""
import numpy as np
import pytest

import close_cells_case as ccc

PINNED = {3: (9469, 156), 2: (9089, 48)}        # bodies, bad targets = 2 * (3 listed kinds * neighbour directions)


@pytest.fixture(scope="module", params=(3, 2))
def case(request, oracle):
    dim = request.param
    b, pairs = ccc.build(dim, oracle.generate(500 + dim, ccc.n_bodies(dim), dim))
    return dim, b, pairs, ccc.bad_targets(b[:, :dim], dim)


def test_every_direction_and_kind_is_planted_across_its_corner(case):
    dim, b, pairs, _ = case
    pos = b[:, :dim]
    assert np.array_equal(pos, pos.astype(np.float32)) and np.array_equal(b[:, -1], b[:, -1].astype(np.float32))
    assert len(pairs) == len(ccc.KINDS) * (3 ** dim - 1)
    assert {(tuple(p["direction"][:dim]), str(p["kind"])) for p in pairs} == {(d, k) for d in ccc.directions(dim) for k in ccc.KINDS}
    cp, cq = ccc.cell_of(pos[pairs["p"]]), ccc.cell_of(pos[pairs["q"]])
    assert np.array_equal(cq - cp, pairs["direction"][:, :dim]), "a pair does not sit in the neighbour cells it was planted for"
    # ... around the recorded corner: the lower of the two cells is corner - 1 on a straddled axis
    d = pairs["direction"][:, :dim]
    assert np.array_equal(np.minimum(cp, cq), pairs["corner"][:, :dim] - (d != 0))
    # mid-cell on the other axes, the same fp32 value for both bodies
    frac = pos[pairs["p"]] * ccc.INV_H - cp
    assert np.allclose(frac[d == 0], ccc.MID, atol=1e-3) and np.array_equal(pos[pairs["p"]][d == 0], pos[pairs["q"]][d == 0])
    # corners at coordinate 0 (cells -1 | 0) for every direction and every kind, and cells at negative coordinates
    zero = pairs[pairs["zero_corner"]]
    assert {tuple(p["direction"][:dim]) for p in zero} == set(ccc.directions(dim)) and {str(k) for k in zero["kind"]} == set(ccc.KINDS)
    for p in zero:
        a = int(np.flatnonzero(p["direction"][:dim])[0])
        assert p["corner"][a] == 0 and {ccc.cell_of(pos[p["p"]])[a], ccc.cell_of(pos[p["q"]])[a]} == {-1, 0}
    assert (np.maximum(cp, cq) < -1).all(axis=1).any(), "no pair with negative cell indices on every axis"
    for kind in ccc.KINDS:
        assert (np.minimum(cp, cq)[pairs["kind"] == kind] < -1).any()


def test_planted_r2_ranges(case):
    dim, b, pairs, _ = case
    r2 = ccc.pair_r2_f32(b[:, :dim], pairs["p"], pairs["q"])
    assert np.array_equal(r2, ccc.pair_r2_f32(b[:, :dim], pairs["q"], pairs["p"]))
    for kind in ccc.KINDS:
        lo, hi = ccc.R2_RANGE[kind]
        got = r2[pairs["kind"] == kind]
        assert lo <= got.min() and got.max() <= hi, (kind, got.min(), got.max())
    # 20 % clear of both thresholds, whatever the order of the fp32 operations
    r2_64 = ((b[pairs["q"], :dim] - b[pairs["p"], :dim]) ** 2).sum(axis=1)
    for x in (ccc.SKIP_R2, float(ccc.BAD_R2)):
        assert (np.abs(r2 - x) >= 0.2 * x).all() and (np.abs(r2_64 - x) >= 0.2 * x).all()
    assert np.abs(r2 / r2_64 - 1).max() < 1e-6


def test_isolation_and_background(case):
    dim, b, pairs, bad = case
    pos = b[:, :dim]
    planted = np.concatenate([pairs["p"], pairs["q"]])
    partner = np.concatenate([pairs["q"], pairs["p"]])
    for i, j in zip(planted, partner):
        r = np.sqrt(((pos - pos[i]) ** 2).sum(axis=1))
        r[[i, j]] = np.inf
        assert r.min() >= 0.01, (i, r.min())
    back = np.ones(b.shape[0], dtype=bool)
    back[planted] = False
    assert back.sum() == ccc.n_background(dim)
    assert not bad[back].any(), "a background body owns a close pair"
    for i in np.flatnonzero(back)[::97]:
        r = np.sqrt(((pos[back] - pos[i]) ** 2).sum(axis=1))
        assert np.sort(r)[1] >= 0.06 - 1e-6


def test_the_count_is_exact(case):
    dim, b, pairs, bad = case
    assert (b.shape[0], int(bad.sum())) == PINNED[dim]
    assert int(bad.sum()) == ccc.expected_bad(pairs)
    for kind in ccc.KINDS:
        assert bad[ccc.rows_of_kind(pairs, kind)].all() == ccc.LISTED[kind] and bad[ccc.rows_of_kind(pairs, kind)].any() == ccc.LISTED[kind]
    # restricted to some targets, the definition is the same rows of the full answer
    rows = np.arange(b.shape[0] // 3, 2 * b.shape[0] // 3)
    assert np.array_equal(ccc.bad_targets(b[:, :dim], dim, rows), bad[rows])


def test_definition_on_known_answers():
    f32 = np.float32
    one = float(np.nextafter(f32(1), f32(2))) - 1.0
    p = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0],                   # exact duplicates: r^2 = 0, not bad
                  [2.0, 2.0, 2.0], [2.0 + 2 * one, 2.0, 2.0],          # one fp32 step at 2.0: r^2 = 5.7e-14, bad
                  [3.0, 3.0, 3.0], [3.0, 3.0 + 9.0e-4, 3.0],           # r^2 = 8.1e-7: bad
                  [4.0, 4.0, 4.0], [4.0, 4.0, 4.0 + 1.1e-3]],          # r^2 = 1.21e-6: not bad
                 dtype=np.float32)
    assert ccc.bad_targets(p, 3).tolist() == [False, False, True, True, True, True, False, False]
    assert ccc.bad_targets(p[:, :2], 2).tolist() == [False, False, True, True, True, True, False, False]


def test_compared_sums_are_well_conditioned(case):
    """What the GPU test compares at rtol = 2e-5 per component (counted pairs) and at 1e-4 of the force (skipped pairs) must
    be a statement about the close-set path, not about cancellation in the lattice's pull: the suite holds every kernel to a
    backward error of 4e-6 of the magnitude sum at this size (oracle_lib.TOL_BACKWARD_SMALL_N), which is 2e-5 of a component
    whose terms cancel to no less than 1/5 of their magnitude sum, and 1e-4 of a force that cancels to no less than 1/25."""
    dim, b, pairs, _ = case
    pos, mass = b[:, :dim], b[:, -1]
    for p in pairs:
        for i in (p["p"], p["q"]):
            comp, vec = ccc.pull_condition(pos[i], pos, mass)
            if p["kind"] == "counted":
                assert all(comp[a] <= 5.0 for a in range(dim) if not p["direction"][a]), (p, comp)
            if p["kind"] == "skipped":
                assert vec <= 25.0 / 4, (p, vec)


@pytest.mark.parametrize("n_shards", (2, 3))
def test_shard_order_splits_every_second_pair(case, n_shards):
    dim, b, pairs, bad = case
    n = b.shape[0]
    order, moved = ccc.shard_order(pairs, n, n_shards)
    L = -(-n // n_shards)
    split = moved["p"] // L != moved["q"] // L
    assert np.array_equal(split, [ccc.split_pair(t) for t in range(len(pairs))]) and split.sum() * 2 == len(pairs)
    assert split[moved["zero_corner"]].any() and not split[moved["zero_corner"]].all()
    for kind in ccc.KINDS:                       # every kind, and every direction, both within a shard and across shards
        assert split[moved["kind"] == kind].any() and not split[moved["kind"] == kind].all()
    assert {tuple(d) for d in moved["direction"][split]} | {tuple(d) for d in moved["direction"][~split]} == {tuple(d) for d in pairs["direction"]}
    assert np.array_equal(b[order][moved["p"]], b[pairs["p"]]) and np.array_equal(b[order][moved["q"]], b[pairs["q"]])


def test_other_inputs(oracle):
    """The remaining inputs of the GPU tests: pinned counts and the properties their docstrings promise."""
    for dim in (3, 2):
        n = ccc.n_bodies(dim)
        # candidates x candidates on the same pairs: candidates <= 1/16
        b, pairs = ccc.build_with_far_shell(dim, oracle.generate(510 + dim, 14000, dim))
        cand = (np.abs(b[:, :dim]).min(axis=1) < 16384.0).sum()
        assert b.shape[0] == 14000 and cand * 16 <= b.shape[0] and not b[:, dim:2 * dim].any()
        assert ccc.bad_targets(b[:, :dim], dim).sum() == PINNED[dim][1] == ccc.expected_bad(pairs)
        assert np.array_equal(ccc.cell_of(b[pairs["q"], :dim]) - ccc.cell_of(b[pairs["p"], :dim]), pairs["direction"][:, :dim])
        for p in pairs[pairs["kind"] == "counted"]:
            for i in (p["p"], p["q"]):
                comp, _ = ccc.pull_condition(b[i, :dim], b[:, :dim], b[:, -1])
                assert all(comp[a] <= 5.0 for a in range(dim) if not p["direction"][a])
        # one equal-key run longer than a sort tile
        b, pairs, dup, (p, q) = ccc.build_equal_keys(dim, oracle.generate(520 + dim, n + 5002, dim))
        bad = ccc.bad_targets(b[:, :dim], dim)
        cells = ccc.cell_of(b[np.concatenate([dup, [p, q]]), :dim])
        assert dup.size == 5000 and (cells == cells[0]).all() and (b[dup, :dim] == b[dup[0], :dim]).all()
        assert not bad[dup].any() and bad[p] and bad[q] and bad.sum() == PINNED[dim][1] + 2
        assert 1.2e-10 <= ccc.pair_r2_f32(b[:, :dim], [p], [q])[0] <= 3.0e-10
        assert np.sqrt(((b[p, :dim] - b[dup[0], :dim]) ** 2).sum()) >= 1.2e-3
        comp, _ = ccc.pull_condition(b[p, :dim], b[:, :dim], b[:, -1])
        assert comp.max() <= 5.0
        # the 1/8 rule
        for n_pairs in (512, 513):
            b = ccc.build_eighth(dim, oracle.generate(530 + dim, 8192, dim), n_pairs)
            bad = ccc.bad_targets(b[:, :dim], dim)
            assert b.shape[0] == 8192 and bad.sum() == 2 * n_pairs and bad[:2 * n_pairs].all()
            assert (np.abs(b[:, :dim]).max() < 16384.0) and np.unique(b[:, :dim], axis=0).shape[0] == 8192
        assert 1024 * 8 <= 8192 < 1026 * 8
        # range ends
        b, pairs, extra = ccc.build_range_ends(dim, oracle.generate(540 + dim, n + 8, dim))
        bad = ccc.bad_targets(b[:, :dim], dim)
        assert bad.sum() == PINNED[dim][1] + 8 and bad[extra.ravel()].all()
        x = b[extra, 0].astype(np.float32)
        assert sorted(np.abs(x).max(axis=1).tolist()) == [float(np.nextafter(np.float32(v), np.float32(0))) for v in (8192, 8192, 16384, 16384)]
        assert (np.abs(x[:, 0] - x[:, 1]) == np.spacing(np.abs(x).min(axis=1))).all() and (x[0::2] > 0).all() and (x[1::2] < 0).all()
