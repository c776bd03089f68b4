"""GPU: the symmetric own-shard force pass with TWO VISITORS PER LANE (csrc/force_sym_kernel.hip, D = 3): a float2 holds the
same position p of two consecutive 64-visitor groups of a chunk (.x: group 2j, .y: group 2j + 1) against one home body.
What the layout distinguishes, and the smallest shard of each:

  padded shard   shape
  16,384         B = 2: the antipodal block only
  20,480         B = 3, ragged last super-block
  65,536         B = 8, S = 64: one pair of groups per chunk
  73,728         B = 9, odd
  532,480        B = 65, S = 32: two pairs of groups per chunk (level 2's order across the pairs shows)

Three layers, with the bounds of tests/test_gpu_sym_large.py and no others:
  1. a sparse-mass probe (tests/sym_probe.py's plan, placement report and fp64 reference) with a heavy body in EVERY group of a
     chunk -- both halves of a lane pair, both pairs where a chunk has two -- at three positions of the rotation: all raw
     accelerations against fp64 numpy under (T1) TOL_BACKWARD and (T3) TOL_REL for kappa <= 4 (mixed mode: every body);
  2. every body of uniform inputs against the strict fp64 kernel (tests/all_bodies.py);
  3. a planted sub-threshold pair whose bodies are the two halves of ONE lane pair."""
import numpy as np
import pytest

import all_bodies
import sym_probe
from oracle_lib import KAPPA_WELL, TOL_BACKWARD, TOL_REL, assert_force_parity

pytestmark = pytest.mark.gpu

SYM = "sympk3l_t8_w3"
PADS = (16384, 20480, 65536, 73728, 532480)
SHAPES = {16384: (2, 64, 2), 20480: (3, 64, 2), 65536: (8, 64, 2), 73728: (9, 64, 2), 532480: (65, 32, 4)}   # B, S, groups per chunk


def _norm(a):
    return np.sqrt((a * a).sum(axis=1))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _heavy(pad, n):
    """One heavy body in every group of the slice's chunk, in super-blocks 0, 1, K and B - 1 (a different slice in each: first,
    last without a pad body, middle), at a position of the rotation that differs from group to group; and the last valid body."""
    p = sym_probe.plan(pad)
    length = sym_probe.SUPER // p["S"]
    assert p["chunks"] == 1 and length == p["gc"] * sym_probe.GROUP
    out = {n - 1}
    for j, block in enumerate(dict.fromkeys((0, 1 % p["B"], p["K"], p["B"] - 1))):
        valid = min(sym_probe.SUPER, n - block * sym_probe.SUPER)
        slices = valid // length                         # slices without a pad body
        assert slices >= 1
        s = (0, slices - 1, slices // 2)[j % 3]
        for g in range(p["gc"]):
            out.add(block * sym_probe.SUPER + s * length + g * sym_probe.GROUP + (5 + 19 * g + 7 * j) % sym_probe.GROUP)
    return np.array(sorted(out), dtype=np.int64)


@pytest.mark.parametrize("pad", PADS)
def test_sparse_mass_probe_with_a_heavy_body_in_every_group_of_a_chunk(nbx, oracle, pad):
    names = nbx.variants()
    p = sym_probe.plan(pad)
    assert (p["B"], p["S"], p["gc"]) == SHAPES[pad], p
    n = sym_probe.body_count(pad)
    heavy = _heavy(pad, n)
    groups = {(int(i) // sym_probe.SUPER, (int(i) % sym_probe.SUPER) // sym_probe.GROUP % p["gc"]) for i in heavy[:-1]}
    assert heavy.size <= 64 and heavy.max() == n - 1 and len(groups) == (heavy.size - 1), "one heavy body per (block, group of the chunk)"
    assert {g for _, g in groups} == set(range(p["gc"])), "both halves of a lane pair, and both pairs where there are two"
    b = oracle.generate(700 + pad % 97, n, 3)
    m = b[heavy, -1].copy()
    b[:, -1] = 0.0
    b[heavy, -1] = m
    b = oracle.round_inputs_to_f32(b)
    ref, mag = sym_probe.reference(b, heavy)
    nref = _norm(ref)
    assert np.isfinite(ref).all() and (nref > 0).all()
    well = mag <= KAPPA_WELL * nref
    massless = b[:, -1] == 0.0
    where = lambda idx: [(int(i), sym_probe.where(pad, int(i))) for i in idx[:12]]
    with nbx.Context(n, 3) as c:
        c.upload(b)
        c.set_tuning(0, names.index(SYM))
        assert c.effective_tuning() == (SYM, p["slots"]), (c.effective_tuning(), p)
        for mixed in (False, True):
            c.set_refine(1.0e-5 if mixed else 0.0)
            c.compute_accel()
            a, f = c.accel().T.astype(np.float64), c.forces()
            assert a.shape == ref.shape and np.isfinite(a).all() and np.isfinite(f).all()
            d = _norm(a - ref)
            back, rel = d / mag, d / nref
            print(f"\nprobe pad={pad} {'mixed' if mixed else 'plain'}: max backward {back.max():.3e}, max rel (kappa <= 4) "
                  f"{rel[well].max():.3e}, max rel {rel.max():.3e}, share kappa > 4 {float((~well).mean()):.4f}")
            bad = np.flatnonzero(back > TOL_BACKWARD)
            assert bad.size == 0, f"(T1) pad={pad} mixed={mixed}: worst {back.max():.3e}; {bad.size} bodies, first (block, slice, chunk, home pass) {where(bad)}; heavy {where(heavy)}"
            bad = np.flatnonzero((rel > TOL_REL) & (well | mixed))
            assert bad.size == 0, f"(T3) pad={pad} mixed={mixed}: worst {rel[bad].max():.3e}; {bad.size} bodies, first {where(bad)}; heavy {where(heavy)}"
            assert not f[massless].any(), "a massless body feels no force"
            assert np.abs(f[~massless]).max() > 0.0


@pytest.mark.parametrize("pad", (65536, 532480))
def test_every_body_against_the_strict_kernel(nbx, oracle, pad):
    """Uniform seeded bodies, all of them against the strict fp64 kernel: (T1) in plain fp32, nobody over 1e-5 in mixed mode."""
    b = oracle.round_inputs_to_f32(oracle.generate(3, pad, 3))
    rec = all_bodies.survey(nbx, oracle, b, f"uniform 3D N={pad:,} (seed 3), symmetric pass, two visitors per lane", variant=SYM)
    all_bodies.write_record(rec, "accuracy_all_bodies_sym_pairs.jsonl")
    print("\n", {k: rec[k] for k in ("n", "default_variant", "default_kernel_ms", "mixed_kernel_ms", "sigma_needed")}, rec["default"], rec["mixed"])
    assert rec["default_variant"] == SYM
    assert rec["default"]["max_backward"] <= TOL_BACKWARD
    assert rec["mixed"]["n_over_tol"] == 0 and rec["mixed"]["tolerance"] == 1.0e-5, rec["mixed"]
    assert rec["mixed"]["max_rel"] <= 1.0e-5


def test_planted_pair_in_the_two_halves_of_one_lane_pair(nbx, oracle):
    """N = 65,536 (B = 8, S = 64: a slice is one chunk of two groups).  One pair at r^2 = 2.3e-13, below the reference's skip
    threshold: position 37 of groups 0 and 1 of slice 9 of super-block 5, so every workgroup (A, 9) with A != 5 that meets block
    5 carries the two bodies in the .x and .y halves of one lane's registers, and block 5 meets them at home and as its own
    visitors.  Both are close-set targets: all planes of both are replaced by the guarded evaluation.  A plane left behind
    would carry the pair's 1/r^4 = 1.9e25 term: the oracle's rows of both bodies (which skip the pair) and of a sample decide."""
    n, dim = 65536, 3
    p = sym_probe.plan(n)
    assert (p["S"], p["gc"]) == (64, 2)
    first = 5 * sym_probe.SUPER + 9 * (sym_probe.SUPER // p["S"]) + 37
    pair = np.array([first, first + sym_probe.GROUP])
    assert sym_probe.where(n, int(pair[0]))[:3] == sym_probe.where(n, int(pair[1]))[:3] == (5, 9, 0)
    b = oracle.generate(305, n, dim)
    b[pair[0], :3] = (3.0, 5.0e6, 5.0e6)
    b[pair[1], :3] = (3.0 + 4.8e-7, 5.0e6, 5.0e6)
    b = oracle.round_inputs_to_f32(b)
    r2 = float(((b[pair[0], :3] - b[pair[1], :3]) ** 2).sum())
    assert 0.0 < r2 < 1.0e-10
    rows = np.unique(np.concatenate((np.random.default_rng(11).integers(0, n, 1100), pair, [n - 1])))
    assert rows.size >= 1024 and np.isin(pair, rows).all()
    ref, S = oracle.force_rows_omp_2(b, rows), oracle.force_magnitude_sums(b, rows)
    with nbx.Context(n, dim) as c:
        c.upload(b)
        c.set_tuning(0, nbx.variants().index(SYM))
        assert c.effective_tuning() == (SYM, p["slots"])
        for tol in (0.0, 1.0e-5):
            c.set_refine(tol)
            c.compute_accel()
            f, a = c.forces(oracle.G), c.accel()
            assert np.isfinite(f).all() and np.isfinite(a).all()
            assert_force_parity(f[rows], ref, S, f"{SYM} planted lane pair tol={tol}", n_sources=n)
            if tol:
                assert np.isinf(c.aux()[pair]).all(), "a close-set target keeps no spread sum"
            c.compute_accel()
            assert np.array_equal(_bits(f), _bits(c.forces(oracle.G))) and np.array_equal(_bits(a), _bits(c.accel())), \
                f"planted lane pair tol={tol}: the same launch twice"
