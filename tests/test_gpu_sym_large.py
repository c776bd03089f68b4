"""GPU: the symmetric own-shard force pass (csrc/force_sym_kernel.hip) on shards above 2^20 bodies, where its decomposition
(csrc/sym_plan.h) takes shapes no other test launches: more than one visitor chunk per slice and block (the kernel's prefetch
across chunks of one block, the reuse of the waves' visitor slots, reaction rows written at chunk c > 0), slices of 4,096 and
8,192 bodies (S = 2, 1), 128 slots = 256 planes (the most the consumers take), a plane array above 4 GiB, the edge of the
default selection and the silent fallback past 255 super-blocks.  Shapes: the table of tests/sym_probe.py, pinned to the header
by tests/test_sym_plan_cpu.py.  Three layers:

  1. a sparse-mass probe (tests/sym_probe.py) at all seven shapes, D = 3 and 2, plain and mixed: every raw acceleration is a
     sum of <= 19 terms, compared with fp64 numpy for ALL bodies under (T1) and (T3) of oracle_lib -- no other tolerance;
  2. every body of uniform inputs against the strict fp64 kernel (tests/all_bodies.py), the protocol of
     tests/test_gpu_sym.py::test_every_body_at_n1048576_in_mixed_mode;
  3. the edges: default selection, the fallback, eager / graph stepping on 256 planes against the oracle's helpers, and a
     planted sub-threshold pair whose 256 planes the close set replaces.

One context is alive at a time (about 15 GiB at the largest shape)."""
import subprocess
import sys

import numpy as np
import pytest

import all_bodies
import sym_probe
from oracle_lib import KAPPA_WELL, TOL_BACKWARD, TOL_REL, assert_force_parity

pytestmark = pytest.mark.gpu

SYM, DPP, ONE_SIDED = "sympk3l_t8_w3", "sympk3l_t8_w3_dpp", "fastpk3l_t8_w3_u4"
TIMES = "sym_large_times.jsonl"


def _v(nbx, name):
    return nbx.variants().index(name)


def _norm(a):
    return np.sqrt((a * a).sum(axis=1))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert np.array_equal(_bits(a), _bits(b)), f"{what}: {int((_bits(a) != _bits(b)).sum())} of {a.size} values differ"


def _uniform(oracle, seed, pad, dim):
    return oracle.round_inputs_to_f32(oracle.generate(seed, sym_probe.body_count(pad), dim))


def _slots(pad):
    """S + K of the shard by the rule of sym_plan.h, stated without the library, and by the table."""
    B = -(-pad // 8192)
    K, S = B // 2, 128
    while S > 1 and (S + K > 128 or B * S > 4096):
        S //= 2
    row = sym_probe.TABLE.get(pad)
    assert row is None or (row[0], row[1], row[2], row[6]) == (B, S, K, S + K), (pad, row, B, S, K)
    return S + K


def _evaluate(c, mixed):
    c.compute_accel()
    out = {"accel": c.accel(), "forces": c.forces()}
    if mixed:
        out["Q"] = c.aux()
    return out


def _where_report(pad, idx, heavy):
    """The failing bodies by (super-block, slice, chunk, home pass): what a reader needs to find the kernel's fault."""
    at = [sym_probe.where(pad, int(i)) for i in idx[:12]]
    blocks = np.unique(np.asarray(idx) // sym_probe.SUPER)
    return (f"{len(idx)} bodies in {blocks.size} super-blocks (first {blocks[:16].tolist()}); first bodies {list(map(int, idx[:12]))} at "
            f"(block, slice, chunk, home pass) {at}; heavy bodies at {[sym_probe.where(pad, int(i)) for i in heavy]}")


def run_probe(nbx, oracle, pad, dim):
    """Layer 1 at one shard size.  Returns the record it printed."""
    names = nbx.variants()
    p = sym_probe.plan(pad)
    b, heavy = sym_probe.sparse_bodies(oracle, 500 + dim, pad, dim)
    n = b.shape[0]
    assert (n + 4095) // 4096 * 4096 == pad and n % 4096 != 0
    ref, mag = sym_probe.reference(b, heavy)
    nref = _norm(ref)
    # self-check on the host: every body has an acceleration to be compared with
    assert np.isfinite(ref).all() and (nref > 0).all() and heavy.size <= 64
    well = mag <= KAPPA_WELL * nref
    massless = b[:, -1] == 0.0
    rec = dict(what="sparse-mass probe", pad=pad, n=n, dim=dim, heavy=int(heavy.size), share_kappa_gt_4=float((~well).mean()), plan=p)
    with nbx.Context(n, dim) as c:
        c.upload(b)
        for mixed in (False, True):
            c.set_refine(1.0e-5 if mixed else 0.0)
            mode = "mixed" if mixed else "plain"
            got = {}
            for name in (SYM, DPP):
                c.set_tuning(0, names.index(name))
                rec.setdefault("variant_slots", c.effective_tuning())
                assert c.effective_tuning() == (name, p["slots"]), (c.effective_tuning(), p)
                c.kernel_time()
                first, second = _evaluate(c, mixed), _evaluate(c, mixed)
                rec[f"{name}_{mode}_kernel_ms"] = c.kernel_time()[0]   # mean of the two launches
                for k in first:
                    _same(first[k], second[k], f"{name} pad={pad} D={dim} {mode}: {k}, the same launch twice")
                got[name] = first
            for k in got[SYM]:
                _same(got[SYM][k], got[DPP][k], f"pad={pad} D={dim} {mode}: {k}, LDS rotation against DPP rotation")
            a = got[SYM]["accel"].T.astype(np.float64)
            f = got[SYM]["forces"]
            assert a.shape == ref.shape and np.isfinite(a).all() and np.isfinite(f).all()
            d = _norm(a - ref)
            back, rel = d / mag, d / nref
            rec[mode] = dict(max_backward=float(back.max()), max_rel_kappa_le_4=float(rel[well].max()), max_rel=float(rel.max()))
            print(f"\nprobe pad={pad} D={dim} {mode}: {rec['variant_slots']} {rec[mode]}")
            bad = np.flatnonzero(back > TOL_BACKWARD)
            assert bad.size == 0, f"(T1) pad={pad} D={dim} {mode}: worst {back.max():.3e} of sum_j |a_ij|; {_where_report(pad, bad, heavy)}"
            bad = np.flatnonzero((rel > TOL_REL) & (well | mixed))
            assert bad.size == 0, f"(T3) pad={pad} D={dim} {mode}: worst {rel[bad].max():.3e}; {_where_report(pad, bad, heavy)}"
            assert not f[massless].any(), "a massless body feels no force"
            assert np.abs(f[~massless]).max() > 0.0 and np.abs(a).max() > 0.0
    all_bodies.write_record(rec, TIMES)
    return rec


@pytest.mark.parametrize("dim", (3, 2))
@pytest.mark.parametrize("pad", sym_probe.PADS)
def test_sparse_mass_probe_meets_every_pair_once(nbx, oracle, pad, dim):
    """(T1) |da_i| <= TOL_BACKWARD sum_j |a_ij| for every body; (T3) |da_i| <= TOL_REL |a_i| where kappa_i <= 4 and, in mixed
    mode, for every body; the same launch twice and both rotations bit for bit; massless bodies feel exactly nothing."""
    cov = sym_probe.coverage(pad, sym_probe.body_count(pad), sym_probe.heavy_indices(pad, sym_probe.body_count(pad)))
    assert all(cov.values()), cov
    assert sym_probe.plan(pad)["slots"] == _slots(pad)
    run_probe(nbx, oracle, pad, dim)


def test_sparse_mass_probe_at_one_chunk_per_slice(nbx, oracle):
    """The same probe at pad 2^20 (B = 128, S = 32, one chunk per slice, 96 slots), the shape the other tests of the pass run:
    a fault that the probe finds above 2^20 bodies and not here lies in the walk over the chunks of a slice."""
    pad = 1 << 20
    p = sym_probe.plan(pad)
    assert (p["chunks"], p["slots"]) == (1, 96) and p["slots"] == _slots(pad)
    run_probe(nbx, oracle, pad, 3)


@pytest.mark.parametrize("pad,dim", ((1052672, 3), (2035712, 3), (2088960, 3), (2035712, 2)))
def test_every_body_against_the_strict_kernel(nbx, oracle, pad, dim):
    """Uniform seeded bodies, every one of them against the strict fp64 kernel: (T1) in plain fp32, nobody over 1e-5 in mixed
    mode (T3) -- the project's contract, first measured for this pass above 2^20 bodies here."""
    b = _uniform(oracle, 3, pad, dim)
    rec = all_bodies.survey(nbx, oracle, b, f"uniform {dim}D N={b.shape[0]:,} (pad {pad:,}, seed 3), symmetric pass", variant=SYM)
    rec["pad"] = pad
    all_bodies.write_record(rec, "accuracy_all_bodies_sym.jsonl")
    print("\n", {k: rec[k] for k in ("n", "dim", "default_variant", "default_kernel_ms", "mixed_kernel_ms", "mixed_refine_ms", "sigma_needed")},
          rec["default"], rec["mixed"])
    assert rec["default_variant"] == SYM
    assert rec["default"]["max_backward"] <= TOL_BACKWARD
    assert rec["mixed"]["n_over_tol"] == 0 and rec["mixed"]["tolerance"] == 1.0e-5, rec["mixed"]
    assert rec["mixed"]["max_rel"] <= 1.0e-5


def _compute_units():
    """The device's CU count from torch, in a child process: this one keeps a single HIP runtime."""
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return int(out.stdout.split()[-1])


def test_default_selection_follows_the_workgroup_count(nbx, oracle):
    """Tuning untouched: the symmetric pass where its B x S workgroups are at least two per CU, the one-sided kernel elsewhere
    (on 256 CUs: up to pad 2,035,712 with 996 workgroups; not at 2,048,000 with 500) and where there is no plan."""
    cus = _compute_units()
    seen = {}
    for pad in sym_probe.TABLE:
        p = sym_probe.plan(pad)
        want = SYM if p is not None and p["B"] * p["S"] >= 2 * cus else ONE_SIDED
        with nbx.Context(sym_probe.body_count(pad), 3) as c:
            c.upload(_uniform(oracle, 9, pad, 3))
            seen[pad] = c.effective_tuning()
            assert seen[pad][0] == want, (pad, cus, p, seen[pad])
            assert want != SYM or seen[pad][1] == _slots(pad), (pad, seen[pad])
            assert want != SYM or seen[pad][1] * 2 <= 256, "two planes per slot, 256 planes at most"
    print(f"\n{cus} CUs: defaults {seen}")
    assert seen[sym_probe.PADS[0]][0] == SYM or cus > 1032, "the first shape has 2,064 workgroups"


def test_past_255_super_blocks_the_context_keeps_the_one_sided_kernel(nbx, oracle):
    pad = sym_probe.PAD_NO_PLAN
    b = _uniform(oracle, 4, pad, 3)
    with nbx.Context(b.shape[0], 3) as c:
        c.upload(b)
        c.set_tuning(0, _v(nbx, ONE_SIDED))
        name, slices = c.effective_tuning()
        assert name == ONE_SIDED
        c.compute_accel()
        want = c.forces(oracle.G)
        c.set_tuning(0, _v(nbx, SYM))
        assert c.effective_tuning() == (SYM, slices), "the name as asked, the slice count of the kernel that runs"
        c.compute_accel()
        _same(c.forces(oracle.G), want, "no symmetric decomposition: the same kernel must have run")
        assert np.isfinite(want).all() and np.abs(want).max() > 0.0


def test_eager_and_graph_steps_on_256_planes(nbx, oracle):
    """Pad 2,035,712, D = 3: 128 slots.  Three eager steps = step(2) + step(1) bit for bit; four more = step(4), whose steps
    are graph replays; and the first step against the oracle's update_body_velocities / update_body_positions fed the device's
    forces, under the rule tests/test_gpu_parity.py holds kick_drift to: rtol 1e-14, atol 0 on positions and velocities.  The
    device's integrator is the reference's arithmetic in fp64, operation by operation and without contraction, on the very
    forces it exports, so a kick that cancels most of a velocity leaves no room for more than that either."""
    pad, dim, dt = 2035712, 3, 1.5
    b = _uniform(oracle, 46, pad, dim)
    b[:, :dim] = b[:, :dim] / 50.0           # pull part of the system into the candidate region
    b = oracle.round_inputs_to_f32(b)
    n = b.shape[0]
    Gs = oracle.G * 1e22
    first, eager3, eager7, graph3, graph7 = (b.copy() for _ in range(5))
    with nbx.Context(n, dim) as c:
        c.upload(b)
        c.set_tuning(0, _v(nbx, SYM))
        assert c.effective_tuning() == (SYM, 128)
        for step in range(7):
            c.compute_accel()
            if step == 0:
                f = c.forces(Gs)
            c.kick_drift(dt, Gs)
            if step in (0, 2):
                c.download(first if step == 0 else eager3)
        c.download(eager7)
        assert c.effective_tuning() == (SYM, 128)
    with nbx.Context(n, dim) as c:
        c.upload(b)
        c.set_tuning(0, _v(nbx, SYM))
        c.step(dt, 2, Gs)
        c.step(dt, 1, Gs)
        c.download(graph3)
        c.step(dt, 4, Gs)                    # from four steps on: a captured step, replayed
        c.download(graph7)
    assert np.array_equal(eager3, graph3), "three eager steps against step(2) + step(1)"
    assert np.array_equal(eager7, graph7), "seven eager steps against step(2) + step(1) + step(4)"
    assert np.abs(eager3[:, dim:2 * dim] - b[:, dim:2 * dim]).max() > 0, "the velocities must have moved"
    assert np.isfinite(f).all()
    want = b.copy()
    oracle.update_body_velocities(want, np.ascontiguousarray(f), dt)
    oracle.update_body_positions(want, dt)
    rows = np.unique(np.concatenate((np.random.default_rng(5).integers(0, n, 4096), [0, n - 1])))
    assert rows.size >= 1024
    dv = np.abs(f[rows] / b[rows, -1:] * dt)
    v_rel = np.abs(first[rows, dim:2 * dim] / want[rows, dim:2 * dim] - 1.0).max()
    x_rel = np.abs(first[rows, :dim] / want[rows, :dim] - 1.0).max()
    print(f"\nfirst step on {rows.size} rows against the oracle's helpers: worst relative difference v {v_rel:.3e}, x {x_rel:.3e}; "
          f"median |dv| / |v| {float(np.median(dv / np.abs(b[rows, dim:2 * dim]))):.3e}")
    assert np.allclose(first[rows, :dim], want[rows, :dim], rtol=1e-14, atol=0)
    assert np.allclose(first[rows, dim:2 * dim], want[rows, dim:2 * dim], rtol=1e-14, atol=0)
    assert (dv > 1e-12 * np.abs(b[rows, dim:2 * dim])).mean() > 0.9, "coupling too weak to test the kick"
    assert np.array_equal(first[:, -1], b[:, -1])


def test_planted_sub_threshold_pair_on_256_planes(nbx, oracle):
    """Pad 2,088,960 (S = 1, K = 127): one pair at r^2 = 2.3e-13, below the reference's skip threshold, in super-blocks 0
    and 200.  Both bodies are close-set targets: scatter_close_kernel replaces all 256 planes of each by the guarded
    evaluation.  A plane it left behind would carry the pair's 1/r^4 = 1.9e25 term: the oracle's rows of both bodies (which
    skip the pair) and of a sample of the others decide."""
    pad, dim = 2088960, 3
    b = oracle.generate(303, sym_probe.body_count(pad), dim)
    n = b.shape[0]
    pair = np.array([200, 200 * 8192 + 4567])
    b[pair[0], :3] = (3.0, 5.0e6, 5.0e6)
    b[pair[1], :3] = (3.0 + 4.8e-7, 5.0e6, 5.0e6)
    b = oracle.round_inputs_to_f32(b)
    r2 = float(((b[pair[0], :3] - b[pair[1], :3]) ** 2).sum())
    assert 0.0 < r2 < 1.0e-10 and pair[1] // 8192 == 200
    rows = np.unique(np.concatenate((np.random.default_rng(11).integers(0, n, 1100), pair, [n - 1])))
    assert rows.size >= 1024 and np.isin(pair, rows).all()
    ref, S = oracle.force_rows_omp_2(b, rows), oracle.force_magnitude_sums(b, rows)
    with nbx.Context(n, dim) as c:
        c.upload(b)
        c.set_tuning(0, _v(nbx, SYM))
        assert c.effective_tuning() == (SYM, 128)
        for tol in (0.0, 1.0e-5):
            c.set_refine(tol)
            c.compute_accel()
            f = c.forces(oracle.G)
            assert np.isfinite(f).all() and np.isfinite(c.accel()).all()
            assert_force_parity(f[rows], ref, S, f"{SYM} planted pair pad={pad} tol={tol}", n_sources=n)
            if tol:
                assert np.isinf(c.aux()[pair]).all(), "a close-set target keeps no spread sum"
            c.compute_accel()
            _same(f, c.forces(oracle.G), f"planted pair tol={tol}: the same launch twice")
