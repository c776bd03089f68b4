"""GPU: the symmetric own-shard force pass (variant sympk3l_t8_w3, csrc/force_sym_kernel.hip) by the helpers and bounds of
tests/test_gpu_parity.py and tests/test_gpu_fullsize.py: every pair evaluated once and used for both bodies must give what
the one-sided kernels give -- the reference's forces within (T1)/(T2)/(T3) of oracle_lib, its skip rule for every pair,
bit-identical repeats and graph replays, and the mixed mode's every-body bound at the benchmark's size."""
import numpy as np
import pytest

import all_bodies
from oracle_lib import TOL_BACKWARD, assert_force_parity, assert_plain_relative

pytestmark = pytest.mark.gpu

SYM, ONE_SIDED = "sympk3l_t8_w3", "fastpk3l_t8_w3_u4"


def _v(nbx, name):
    return nbx.variants().index(name)


def _inputs(oracle, seed, n, dim):
    return oracle.round_inputs_to_f32(oracle.generate(seed, n, dim))


def _norm(a):
    return np.sqrt((a * a).sum(axis=1))


@pytest.mark.parametrize("dim", (3, 2))
@pytest.mark.parametrize("n", (1, 2, 3, 255, 257, 1024, 1025, 4096))
def test_below_two_super_blocks_the_context_keeps_the_one_sided_kernel(nbx, oracle, dim, n):
    b = _inputs(oracle, 100 + n, n, dim)
    ref, S = oracle.brute_force_seq(b), oracle.force_magnitude_sums(b)
    with nbx.Context(n, dim) as c:
        c.upload(b)
        c.set_tuning(0, _v(nbx, SYM))
        assert c.effective_tuning()[0] == SYM
        c.compute_accel()
        f = c.forces(oracle.G)
        assert_force_parity(f, ref, S, f"{SYM} D={dim} N={n}")
        c.set_tuning(0, _v(nbx, ONE_SIDED))
        c.compute_accel()
        assert np.array_equal(f, c.forces(oracle.G)), "no symmetric decomposition: the same kernel must have run"


@pytest.mark.parametrize("dim", (3, 2))
def test_every_force_at_n65536(nbx, oracle, dim):
    """All 65,536 forces against the oracle (B = 8 super-blocks: the antipodal rule, four reaction slots), plain fp32 and the
    default precision, the same launch twice, and against the one-sided kernel per body."""
    n = 65536
    b = _inputs(oracle, 2, n, dim)
    ref, S = oracle.brute_force_omp_2(b), oracle.force_magnitude_sums(b)
    with nbx.Context(n, dim) as c:
        c.upload(b)
        assert c.effective_tuning()[0] == SYM, "a single shard of 8 super-blocks: the default run takes the symmetric pass"
        c.set_tuning(0, _v(nbx, SYM))
        assert c.effective_tuning() == (SYM, 68)
        c.compute_accel()
        f = c.forces(oracle.G)
        e = assert_force_parity(f, ref, S, f"{SYM} full N=65,536 D={dim}")
        worst = assert_plain_relative(f, ref, f"{SYM} full N=65,536 D={dim}")
        print(f"\n{SYM} N=65,536 D={dim}: max |da|/|a| = {worst:.3e}, {e}")
        assert oracle.compute_accuracy(f, ref) == 100.0
        total = np.abs(f).sum(axis=0)
        assert (np.abs(f.sum(axis=0)) <= 1e-5 * total).all(), "Newton's third law"
        c.compute_accel()
        assert np.array_equal(f, c.forces(oracle.G)), "same launch twice must be bit-identical"
        c.set_refine(0.0)
        c.compute_accel()
        plain = c.forces(oracle.G)
        assert_force_parity(plain, ref, S, f"{SYM} plain fp32 N=65,536 D={dim}")
        c.compute_accel()
        assert np.array_equal(plain, c.forces(oracle.G))
        c.set_tuning(0, _v(nbx, ONE_SIDED))
        c.compute_accel()
        d = _norm(plain - c.forces(oracle.G))
        assert (d <= 2.0 * TOL_BACKWARD * S).all(), "per body: two summation orders of the same terms"


@pytest.mark.parametrize("n,dim", ((12289, 3), (20000, 3), (28000, 2), (40000, 3)))
def test_ragged_and_odd_decompositions(nbx, oracle, n, dim):
    """B = 2 (only the antipodal block), 3 (odd, ragged last block), 4 (even, ragged), 5 (odd): the full array against the oracle."""
    b = _inputs(oracle, 7 + n, n, dim)
    ref, S = oracle.brute_force_omp_2(b), oracle.force_magnitude_sums(b)
    with nbx.Context(n, dim) as c:
        c.upload(b)
        c.set_tuning(0, _v(nbx, SYM))
        for tol in (0.0, 1.0e-5):
            c.set_refine(tol)
            c.compute_accel()
            f = c.forces(oracle.G)
            assert_force_parity(f, ref, S, f"{SYM} N={n} D={dim} tol={tol}")
            c.compute_accel()
            assert np.array_equal(f, c.forces(oracle.G))


def test_planted_coincident_and_sub_threshold_pairs(nbx, oracle):
    """The planted pairs of test_fast_path_close_set_semantics, in one super-block and across super-blocks and slices."""
    n, dim = 40000, 3
    b = oracle.generate(91, n, dim)
    b[:1500, 0] = 1.0 + 8000.0 * (b[:1500, 0] / 1e7)          # 7.5 % of the first super-block near the x = 0 plane
    b[200, :3] = (3.0, 5.0e6, 5.0e6)
    b[30001, :3] = (3.0 + 4.8e-7, 5.0e6, 5.0e6)               # 2 ulp apart, three super-blocks away: r^2 = 2.3e-13 -> skipped
    b[300, :3] = (100.0, 2.0e6, 2.0e6)
    b[301, :3] = (100.0 + 7.7e-6, 2.0e6, 2.0e6)               # r^2 = 5.9e-11 -> skipped
    b[17002, :3] = (100.0 + 1.6e-5, 2.0e6, 2.0e6)             # r^2 = 2.6e-10 from body 300 -> counted
    b[5000:5004, :3] = b[4999, :3]                            # exact duplicates in one home pass
    b[25000:25003, :3] = b[4999, :3]                          # ... and in another super-block
    b[6000, :3] = (9000.0, 9000.0, 9000.0)
    b[39001, :3] = (9000.0 + 9.765625e-4, 9000.0, 9000.0)     # closest possible pair outside the close set
    b = oracle.round_inputs_to_f32(b)
    ref, S = oracle.brute_force_seq(b), oracle.force_magnitude_sums(b)
    with nbx.Context(n, dim) as c:
        c.upload(b)
        c.set_tuning(0, _v(nbx, SYM))
        assert c.effective_tuning()[0] == SYM
        for tol in (0.0, 1.0e-5):
            c.set_refine(tol)
            c.compute_accel()
            f = c.forces(oracle.G)
            assert np.isfinite(f).all()
            assert_force_parity(f, ref, S, f"{SYM} planted pairs tol={tol}")
            c.compute_accel()
            assert np.array_equal(f, c.forces(oracle.G)), "bit-reproducible despite the atomically built list"


def test_graph_replayed_steps_equal_eager_steps(nbx, oracle):
    for n, dim in ((20000, 3), (16000, 2)):
        b = _inputs(oracle, 46, n, dim)
        b[:, :dim] = b[:, :dim] / 50.0           # pull part of the system into the candidate region
        b = oracle.round_inputs_to_f32(b)
        eager, graph = b.copy(), b.copy()
        Gs = oracle.G * 1e22
        with nbx.Context(n, dim) as c:
            c.upload(b)
            c.set_tuning(0, _v(nbx, SYM))
            assert c.effective_tuning()[0] == SYM
            for _ in range(12):
                c.compute_accel()
                c.kick_drift(1.5, Gs)
            c.download(eager)
        with nbx.Context(n, dim) as c:
            c.upload(b)
            c.set_tuning(0, _v(nbx, SYM))
            c.step(1.5, 7, Gs)
            c.step(1.5, 5, Gs)                   # second call reuses the instantiated graph
            c.download(graph)
        assert np.array_equal(eager, graph)
        assert np.abs(eager[:, dim:2 * dim] - b[:, dim:2 * dim]).max() > 0


def test_single_shard_pass_against_eight_shards_of_the_one_sided_kernels(nbx, oracle):
    n, dim = 65536, 3
    b = _inputs(oracle, 12, n, dim)
    S = oracle.force_magnitude_sums(b)
    with nbx.Context(n, dim) as c:
        c.upload(b)
        c.set_tuning(0, _v(nbx, SYM))
        c.compute_accel()
        f = c.forces(oracle.G)
    parts = []
    for r in range(8):
        with nbx.Context(n, dim, n_shards=8, shard=r) as c:
            c.upload(b)
            assert c.effective_tuning()[0] == ONE_SIDED, "multi-shard contexts keep today's kernels"
            c.compute_accel(nbx.SRC_LOCAL)
            c.compute_accel(nbx.SRC_REMOTE)
            parts.append(c.forces(oracle.G))
    d = _norm(f - np.concatenate(parts))
    assert (d <= 2.0 * TOL_BACKWARD * S).all(), f"worst {float((d / S).max()):.3e} of S_i"


def test_every_body_at_n1048576_in_mixed_mode(nbx, oracle):
    """The benchmark's size: every body against the strict fp64 kernel (tests/all_bodies.py), nobody over 1e-5."""
    n = 1 << 20
    b = _inputs(oracle, 3, n, 3)
    rec = all_bodies.survey(nbx, oracle, b, "uniform 3D N=2^20 (BASELINE config 3 input, seed 3), symmetric pass", variant=SYM)
    all_bodies.write_record(rec, "accuracy_all_bodies_sym.jsonl")
    print("\n", {k: rec[k] for k in ("default_variant", "default_kernel_ms", "mixed_kernel_ms", "mixed_refine_ms", "sigma_needed")},
          rec["default"], rec["mixed"])
    assert rec["default_variant"] == SYM
    assert rec["mixed"]["n_over_tol"] == 0 and rec["mixed"]["tolerance"] == 1.0e-5, rec["mixed"]
    assert rec["mixed"]["max_rel"] <= 1.0e-5
    assert rec["default"]["max_backward"] <= TOL_BACKWARD
