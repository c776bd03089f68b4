"""CPU: the input of the multi-rank exchange tests (tests/exchange_case.py) is what it claims to be.  The certificate -- a
stale, early, frozen or partly stale copy of any rank's chunk in any other rank's buffer misses the project's tolerances by a
factor of 100 or more, in velocity and in potential energy -- is asserted on every shape, law and scheme the GPU tests run; the
specification it rests on is pinned to the oracle's helpers; and the generated-only input those tests used to rest on is
shown to certify nothing."""
import numpy as np
import pytest

import exchange_case as ec

FLOOR = 100.0
# planted rows and ordered rank pairs per case: 2 k^2 and k (k - 1) for k non-empty shards
COUNTS = {"r2": (8, 2), "r3_2d": (18, 6), "r8": (128, 56), "r4_short": (32, 12), "softened": (8, 2), "newton": (32, 12),
          "dist2": (8, 2), "dist3_2d": (18, 6), "gloo2": (8, 2), "gloo3_2d": (18, 6)}


# (the one-process-per-rank GPU cases, dist*, step kick-drift only)
@pytest.mark.parametrize("name,scheme", [(name, scheme) for name in sorted(ec.CASES) for scheme in ("kd", "kdk")
                                         if not (name.startswith("dist") and scheme == "kdk")])
def test_certificate_holds_on_every_shape_the_gpu_tests_use(name, scheme):
    c = ec.CASES[name]
    m = ec.case_margins(name, scheme)
    pairs = ec.ordered_pairs(c["n"], c["ranks"])
    print(f"\n{name} {scheme} ({c['ranks']} ranks, n={c['n']}, {c['dim']}D, {c['law']}): moved {m['moved']:.4g}, U {m['pe_total']:.4g}; "
          "minimum over the rank pairs of error / tolerance [velocity, position, potential energy]")
    for f in ec.FAULTS:
        assert sorted(m[f]["pairs"]) == sorted(pairs)
        print(f"    {f:10s} {m[f]['vel']:9.0f} {m[f]['pos']:9.0f} {m[f]['pe']:9.0f}")
    for f in ec.FAULTS:
        assert m[f]["vel"] >= FLOOR and m[f]["pe"] >= FLOOR, (name, scheme, f, m[f]["vel"], m[f]["pe"])


@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_planted_rows_and_rank_pairs_are_pinned(name):
    c = ec.CASES[name]
    n, dim, ranks = c["n"], c["dim"], c["ranks"]
    lay = ec.planted_layout(n, dim, ranks)
    rows = ec.planted_rows(n, dim, ranks)
    pairs = ec.ordered_pairs(n, ranks)
    assert (len(rows), len(pairs)) == COUNTS[name] and len(set(rows)) == len(rows)
    bounds = ec.shard_bounds(n, ranks)
    shard_of = lambda i: next(g for g, (lo, hi) in enumerate(bounds) if lo <= i < hi)
    # the first and the last row of every shard is a mover, and every other shard reads it through a probe of its own
    assert sorted(m[0] for m in lay["movers"]) == sorted([lo for lo, hi in bounds] + [hi - 1 for lo, hi in bounds])
    for row, q in lay["movers"]:
        readers = sorted(r for prow, r, mrow in lay["probes"] if mrow == row)
        assert shard_of(row) == q and readers == [g for g in range(ranks) if g != q]
    for prow, r, mrow in lay["probes"]:
        lo, hi = bounds[r]
        assert shard_of(prow) == r and lo < prow < hi - 1
        if hi - lo >= 2 * ec.EDGE_ROWS + 2 * (ranks - 1):        # (every GPU shape; the 300-body gloo shapes are shorter)
            assert lo + ec.EDGE_ROWS <= prow < hi - ec.EDGE_ROWS   # outside the rows of late_head / late_tail
    b = ec.case_bodies(name)
    assert np.array_equal(b[:, :dim], b[:, :dim].astype(np.float32)) and np.array_equal(b[:, -1], b[:, -1].astype(np.float32))
    assert np.array_equal(b[rows, dim:2 * dim], b[rows, dim:2 * dim].astype(np.float32))
    x = b[rows, :dim]
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)) + 1e9 * np.eye(len(rows))
    assert d.min() >= 0.999 * ec.PLANTED_SEP and b[:, :dim].min() > 0
    assert np.array_equal(ec.case_bodies(name), b)                                      # the same bodies in every process


def test_a_case_that_cannot_host_the_planted_rows_fails_loudly():
    with pytest.raises(ValueError):
        ec.moving_pairs(9, 3, 8, 1)                  # shards of two rows, the last of one
    with pytest.raises(ValueError):
        ec.moving_pairs(8 * 15 + 1, 3, 8, 1)         # sixteen rows per shard, but the last shard holds nine
    with pytest.raises(ValueError):
        ec.moving_pairs(8 * 15, 3, 8, 1)             # fifteen rows per shard, sixteen to plant
    assert ec.moving_pairs(8 * 16, 3, 8, 1).shape == (128, 7)
    with pytest.raises(ValueError):
        ec.moving_pairs(4000, 3, 9, 1)               # eight probes behind one mover: 3D has seven places
    with pytest.raises(ValueError):
        ec.moving_pairs(4000, 2, 5, 1)               # 2D has three
    lay = ec.planted_layout(7, 3, 1)                  # one rank: no exchange, nothing planted
    assert lay == {"movers": [], "probes": []} and ec.ordered_pairs(7, 1) == []
    assert ec.ordered_pairs(5, 8) == [(r, q) for r in range(5) for q in range(5) if r != q]   # empty ranks are no readers


def test_generated_bodies_alone_certify_nothing():
    """Why the planted groups exist: on the generated bodies the multi-rank tests stepped before (eight ranks, a 2,000-body
    stand-in for their 9,000), one rank reading one other rank's chunk one step late stays inside the velocity tolerance for
    most rank pairs -- the smallest error over the 56 pairs is a few hundredths of it."""
    n, dim, ranks = 2000, 3, 8
    b = ec.bodies_by_name("generated", n, dim, ranks, 31)
    m = ec.fault_margins(b, dim, ranks, ec.STEPS, ec.DT, ec.G_REFERENCE * 1e24, "kd", targets="all", faults=("late",))
    vel = np.array([v[0] for v in m["late"]["pairs"].values()])
    print(f"\ngenerated only, {ranks} ranks, n={n}: late copy, error / tolerance over {vel.size} rank pairs: min {vel.min():.3g}, "
          f"median {np.median(vel):.3g}, max {vel.max():.3g}; caught {int((vel > 1).sum())}")
    assert vel.size == 56 and vel.min() < 1.0 and (vel > 1).sum() < vel.size
    assert m["late"]["vel"] == vel.min()


@pytest.mark.parametrize("dim", (3, 2))
def test_trajectory_spec_is_the_oracles_helpers_composed_the_same_way(oracle, dim):
    n, steps, dt, gs, eps = 160, 3, 2.0, 1e24, 700.0
    b = ec.moving_pairs(n, dim, 2, 5)
    G = oracle.G * gs

    def force(cur, law):
        r = oracle.round_inputs_to_f32(cur)
        if law == "reference":
            return oracle.brute_force_seq(r) * gs
        return oracle.force_rows_softened(r, eps, newton=(law == "newton"))[0] * gs

    for law in ("reference", "softened", "newton"):
        for scheme in ("kd", "kdk"):
            cur = b.copy()
            for _ in range(steps):
                if scheme == "kd":
                    oracle.update_body_velocities(cur, np.ascontiguousarray(force(cur, law)), dt)
                    oracle.update_body_positions(cur, dt)
                else:
                    oracle.update_body_velocities(cur, np.ascontiguousarray(force(cur, law)), dt / 2)
                    oracle.update_body_positions(cur, dt)
                    oracle.update_body_velocities(cur, np.ascontiguousarray(force(cur, law)), dt / 2)
            got = ec.trajectory_spec(b, dim, steps, dt, G, scheme, law, eps)[-1]
            dv = np.abs(cur[:, dim:2 * dim] - b[:, dim:2 * dim]).max()
            assert dv > 1.0
            assert np.abs(got[:, dim:2 * dim] - cur[:, dim:2 * dim]).max() <= 1e-12 * dv, (law, scheme)
            assert np.allclose(got[:, :dim], cur[:, :dim], rtol=1e-12, atol=0), (law, scheme)
            assert np.array_equal(got[:, -1], b[:, -1])
            r32 = oracle.round_inputs_to_f32(cur)
            ke_ref, pe_ref = oracle.energy(r32) if law == "reference" else oracle.energy_softened(r32, eps, newton=(law == "newton"))
            ke, pe = ec.energy_spec(cur, dim, G, law, eps)
            assert abs(ke - ke_ref) <= 1e-12 * ke_ref and abs(pe - pe_ref * gs) <= 1e-12 * abs(pe_ref * gs), (law, scheme)
