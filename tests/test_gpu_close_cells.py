"""GPU: the close-set classification against its definition, at every boundary of the sorted-cell refinement
(csrc/close_hash.hip) and of the rules around it.

The fast force kernels carry no per-pair guard: they are right only because every target with a partner at
0 < r^2 < 1e-6 is listed and handed to the guarded close-set workgroups.  The inputs of close_cells_case.py put a pair
across every one of the 3^D - 1 neighbour-cell boundaries (at the origin and at negative cells too); the list is checked
through its length (nbx_ctx_close_set_mode against close_cells_case.bad_targets) and through the forces of the bodies for
which a missed listing shows: a counted pair at r^2 = 1.7e-10 is off by 2 kTiny / r^2 >= 4.7e-5 when it is not listed,
a skipped pair (r^2 = 4e-11) by orders of magnitude.  tests/test_close_cells_cpu.py asserts what these checks rest on.

Variants are run in plain fp32 (set_refine(0)): mixed mode re-evaluates every listed target in fp64 and would stand in
front of the close-set workgroups' own sums.  The default tuning runs in the default (mixed) precision as well."""
import numpy as np
import pytest

import close_cells_case as ccc
from oracle_lib import assert_force_parity

pytestmark = pytest.mark.gpu

RTOL_COUNTED = 2.0e-5       # test_gpu_parity.test_fast_path_boundary_pairs' bound; the guarded path is good to ~1e-6
RTOL_SKIPPED = 1.0e-4       # the partner contributes nothing


class Case:
    def __init__(self, oracle, b, pairs, dim):
        self.b, self.pairs, self.dim, self.n = b, pairs, dim, b.shape[0]
        self.ref = oracle.brute_force_seq(b)
        self.S = oracle.force_magnitude_sums(b)
        self.bad = ccc.bad_targets(b[:, :dim], dim)
        self.counted = ccc.rows_of_kind(pairs, "counted")
        self.skipped = ccc.rows_of_kind(pairs, "skipped")


@pytest.fixture(scope="module")
def cells(oracle):
    """build() for D = 3 and 2 with the oracle's forces, computed once and left unchanged."""
    out = {}
    for dim in (3, 2):
        b, pairs = ccc.build(dim, oracle.generate(500 + dim, ccc.n_bodies(dim), dim))
        out[dim] = Case(oracle, b, pairs, dim)
    return out


def check_forces(f, case, what, lo=0, extra_counted=()):
    """The three force assertions on rows lo .. lo + len(f) of the case: parity over all of them; every body of a counted
    pair per component at 2e-5; on every body of a skipped pair the partner contributes nothing."""
    hi = lo + f.shape[0]
    ref, S = case.ref[lo:hi], case.S[lo:hi]
    counted = np.concatenate([case.counted, np.asarray(extra_counted, dtype=np.int64)])
    counted = counted[(counted >= lo) & (counted < hi)] - lo
    skipped = case.skipped[(case.skipped >= lo) & (case.skipped < hi)] - lo
    worst_c = max((float(np.abs(f[i] / ref[i] - 1).max()) for i in counted), default=0.0)
    worst_s = max((float(np.linalg.norm(f[i] - ref[i]) / np.linalg.norm(ref[i])) for i in skipped), default=0.0)
    print(f"{what}: counted bodies {counted.size}, worst component error {worst_c:.3e}; skipped bodies {skipped.size}, worst error {worst_s:.3e}")
    for i in counted:
        assert np.allclose(f[i], ref[i], rtol=RTOL_COUNTED, atol=0), (what, "counted", int(i) + lo, f[i], ref[i])
    for i in skipped:
        assert np.linalg.norm(f[i] - ref[i]) <= RTOL_SKIPPED * np.linalg.norm(ref[i]), (what, "skipped", int(i) + lo, f[i], ref[i])
    assert_force_parity(f, ref, S, what, n_sources=case.n)


def run_variants(nbx, oracle, c, case, what, extra_counted=()):
    """Every fast* / sym* variant that keeps its name on this input in plain fp32, then the default tuning in the default
    precision; each evaluated twice (same bits)."""
    tol, sigma = nbx.get_default_refine()
    ran = []
    for v, name in list(enumerate(nbx.variants())) + [(-1, "default")]:
        if v >= 0 and not name.startswith(("fast", "sym")):
            continue
        c.set_tuning(0, v)
        c.set_refine(0.0 if v >= 0 else tol, 0.0 if v >= 0 else sigma)
        if v >= 0 and c.effective_tuning()[0] != name:
            assert name.startswith("sym"), f"{what}: the fast variant {name} must run itself here, not {c.effective_tuning()[0]}"
            continue
        c.compute_accel()
        f = c.forces(oracle.G)
        check_forces(f, case, f"{what}, {name}", extra_counted=extra_counted)
        c.compute_accel()
        assert np.array_equal(f, c.forces(oracle.G)), f"{what}, {name}: a second evaluation gives other bits"
        ran.append(name)
    assert sum(n.startswith("fast") for n in ran) >= 3 and ran[-1] == "default", ran
    return ran


@pytest.mark.parametrize("dim", (3, 2))
def test_every_neighbour_cell(nbx, oracle, cells, dim):
    """One pair across each of the 26 (8) neighbour-cell boundaries, for each kind: the sorted-cell list has exactly the
    definition's length, and every body whose listing shows in its force has the guarded sum's force."""
    case = cells[dim]
    with nbx.Context(case.n, dim) as c:
        c.upload(case.b)
        mode, _, bad = c.close_set_mode()
        print(f"D={dim}: n={case.n} mode {mode}, bad targets {bad} (definition {int(case.bad.sum())})")
        assert mode == "sorted_cells" and int(case.bad.sum()) == ccc.expected_bad(case.pairs)
        # a wrong list shows twice, in its length and in the forces: report both before failing
        problems = [] if bad == int(case.bad.sum()) else [f"{bad} bad targets listed, the definition gives {int(case.bad.sum())}"]
        try:
            run_variants(nbx, oracle, c, case, f"every neighbour cell D={dim}")
        except AssertionError as e:
            problems.append(str(e))
        assert not problems, "\n".join(problems)
        assert c.close_set_mode()[0] == "sorted_cells"


@pytest.mark.parametrize("n_shards", (2, 3))
@pytest.mark.parametrize("dim", (3, 2))
def test_neighbour_cells_across_shards(nbx, oracle, cells, dim, n_shards):
    """The same bodies reordered so that every second pair has its bodies in different shards: each shard's probe counts its
    own targets against ALL bodies, and LOCAL + REMOTE passes give the listed bodies the guarded sum."""
    case = cells[dim]
    order, moved = ccc.shard_order(case.pairs, case.n, n_shards)
    sh = Case.__new__(Case)
    sh.b, sh.pairs, sh.dim, sh.n = np.ascontiguousarray(case.b[order]), moved, dim, case.n
    sh.ref, sh.S, sh.bad = case.ref[order], case.S[order], case.bad[order]    # per-body quantities: the order of the sources moves the oracle's fp64 sums by ~1e-16
    sh.counted, sh.skipped = ccc.rows_of_kind(moved, "counted"), ccc.rows_of_kind(moved, "skipped")
    tol, sigma = nbx.get_default_refine()
    seen = 0
    for r in range(n_shards):
        with nbx.Context(sh.n, dim, n_shards=n_shards, shard=r) as c:
            c.upload(sh.b)
            lo = r * c.shard_len
            want = int(sh.bad[lo:lo + c.count].sum())
            mode, _, bad = c.close_set_mode()
            print(f"D={dim} shard {r}/{n_shards}: mode {mode}, bad targets {bad} (definition {want})")
            assert mode == "sorted_cells" and bad == want
            seen += bad
            for refine in ((0.0, 0.0), (tol, sigma)):
                c.set_refine(*refine)
                c.compute_accel(nbx.SRC_LOCAL)
                c.compute_accel(nbx.SRC_REMOTE)
                check_forces(c.forces(oracle.G), sh, f"D={dim} shard {r}/{n_shards} refine={refine[0]:g}", lo=lo)
    assert seen == int(case.bad.sum())


@pytest.mark.parametrize("dim", (3, 2))
def test_both_classifiers_on_the_same_pairs(nbx, oracle, dim):
    """The planted cloud inside a shell of bodies at coordinates >= 1e5: candidates are 1/23 of the system, so
    refine_close_kernel (candidates x candidates) classifies the very same pairs.  Its count is read through the asynchronous
    poll of a run in which nothing moves."""
    b, pairs = ccc.build_with_far_shell(dim, oracle.generate(510 + dim, 14000, dim))
    case = Case(oracle, b, pairs, dim)
    n_cand = int((np.abs(b[:, :dim]).min(axis=1) < 16384.0).sum())
    with nbx.Context(case.n, dim) as c:
        c.upload(b)
        assert c.close_set_mode()[0] == "candidate_pairs"
        run_variants(nbx, oracle, c, case, f"candidate pairs D={dim}")
        assert c.close_set_mode()[0] == "candidate_pairs"
        # zero velocities and a coupling of 1e-20 of the reference's: 17 steps move no fp32 position
        G = oracle.G * 1.0e-20
        for _ in range(16):
            c.compute_accel()
            c.kick_drift(1.0, G)
        c.synchronize()                      # the counter copy issued by step 16 has landed
        c.compute_accel()
        c.kick_drift(1.0, G)                 # ... and this poll reads it
        mode, cand, bad = c.close_set_mode()
        cur = b.copy()
        c.download(cur)
        assert np.array_equal(cur[:, :dim].astype(np.float32), b[:, :dim].astype(np.float32)), "a position moved: the poll's count is of another input"
        print(f"D={dim}: poll saw {cand} candidates (input {n_cand}), {bad} bad targets (definition {int(case.bad.sum())})")
        assert mode == "candidate_pairs" and cand == n_cand
        assert bad == int(case.bad.sum()) == ccc.expected_bad(pairs)


@pytest.mark.parametrize("dim", (3, 2))
def test_a_long_run_of_equal_keys(nbx, oracle, dim):
    """5000 exact duplicates and a counted pair in ONE cell: an equal-key run of 5002, longer than a 4096-element tile of the
    radix sort, which the refinement's lower_bound + scan has to walk.  The duplicates (r^2 = 0) are not bad; the pair is."""
    b, pairs, dup, (p, q) = ccc.build_equal_keys(dim, oracle.generate(520 + dim, ccc.n_bodies(dim) + 5002, dim))
    case = Case(oracle, b, pairs, dim)
    lattice_part = ccc.expected_bad(pairs)
    assert not case.bad[dup].any() and int(case.bad.sum()) == lattice_part + 2
    with nbx.Context(case.n, dim) as c:
        c.upload(b)
        mode, _, bad = c.close_set_mode()
        print(f"D={dim}: n={case.n} mode {mode}, bad targets {bad} (definition {lattice_part} + 2)")
        assert mode == "sorted_cells" and bad == lattice_part + 2
        run_variants(nbx, oracle, c, case, f"equal keys D={dim}", extra_counted=(p, q))


@pytest.mark.parametrize("dim", (3, 2))
def test_the_eighth_rule_exactly(nbx, oracle, dim):
    """probe_bad * 8 > count demotes a shard to the guarded kernel: 1024 bad targets of 8192 stay on the fast path (and fill
    four list blocks of the close-set workgroups), 1026 do not."""
    tol, sigma = nbx.get_default_refine()
    for n_pairs, want_mode in ((512, "sorted_cells"), (513, "guarded_kernel")):
        b = ccc.build_eighth(dim, oracle.generate(530 + dim, 8192, dim), n_pairs)
        ref, S = oracle.brute_force_seq(b), oracle.force_magnitude_sums(b)
        assert int(ccc.bad_targets(b[:, :dim], dim).sum()) == 2 * n_pairs
        with nbx.Context(8192, dim) as c:
            c.upload(b)
            mode, _, bad = c.close_set_mode()
            print(f"D={dim}: {n_pairs} pairs: mode {mode}, bad targets {bad}, kernel {c.effective_tuning()[0]}")
            assert bad == 2 * n_pairs and mode == want_mode
            assert ("exact" in c.effective_tuning()[0]) == (want_mode == "guarded_kernel")
            for refine in ((0.0, 0.0), (tol, sigma)):
                c.set_refine(*refine)
                c.compute_accel()
                assert_force_parity(c.forces(oracle.G), ref, S, f"D={dim} {n_pairs} pairs refine={refine[0]:g}")


@pytest.mark.parametrize("dim", (3, 2))
def test_range_ends(nbx, oracle, dim):
    """Pairs one fp32 step apart just below |x| = 8192 and 16384, both signs, in a small-coordinate cloud: cell indices up to
    8.4e6 (and down to -8.4e6), fp32 spacing up to 2^-10 = 9.77e-4 -- r^2 = 9.54e-7, the largest listed r^2 there is."""
    b, pairs, extra = ccc.build_range_ends(dim, oracle.generate(540 + dim, ccc.n_bodies(dim) + 8, dim))
    case = Case(oracle, b, pairs, dim)
    assert case.bad[extra.ravel()].all() and int(case.bad.sum()) == ccc.expected_bad(pairs) + 8
    with nbx.Context(case.n, dim) as c:
        c.upload(b)
        mode, _, bad = c.close_set_mode()
        print(f"D={dim}: mode {mode}, bad targets {bad} (definition {int(case.bad.sum())})")
        assert mode == "sorted_cells" and bad == int(case.bad.sum())
        run_variants(nbx, oracle, c, case, f"range ends D={dim}")
