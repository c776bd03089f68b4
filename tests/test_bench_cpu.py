"""bench.py's record-keeping, checked without a GPU: the committed PMC profile resolves for the kernel the default run launches
(a hand-kept name table went stale and the driver's line carried traffic: null), and a plain
`python bench.py --gpus N` starts its ranks as a child process instead of exiting with a usage line (weak #6)."""
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import nbody_amd as nbx  # noqa: E402


def _default_variant_name():
    lib = nbx.load_library()
    return lib.nbx_variant_name(lib.nbx_default_variant()).decode()


def test_library_reports_the_default_kernels_symbol_without_a_device():
    sym = bench.launched_kernel_symbol(_default_variant_name(), 3, 1.0e-5)
    assert sym.startswith("void nbx::(anonymous namespace)::accel_fast3l_kernel<3, ") and sym.endswith(">(nbx::KArgs)"), sym
    plain = bench.launched_kernel_symbol(_default_variant_name(), 3, 0.0)
    assert plain != sym and "accel_fast3l_kernel<3, " in plain
    assert "accel_fast3l_kernel<2, " in bench.launched_kernel_symbol(_default_variant_name(), 2, 1.0e-5)
    # a variant without a mixed-mode build runs its plain kernel whatever the tolerance
    assert "accel_f64_kernel<3, " in bench.launched_kernel_symbol("strict_f64_t4", 3, 1.0e-5)


def test_committed_pmc_profile_resolves_for_the_default_run():
    launched = bench.launched_kernel_symbol(_default_variant_name(), 3, 1.0e-5)
    found = None
    for rnd in bench.PROFILE_ROUNDS:
        path = os.path.join(ROOT, "profiles", rnd, "pmc_force_kernel.json")
        if not os.path.exists(path):
            continue
        t = bench.pmc_traffic(json.load(open(path)), launched)
        if t is not None:
            found = (rnd, t)
            break
    assert found, f"no profiles/<round>/pmc_force_kernel.json of '{launched}' in {bench.PROFILE_ROUNDS}"
    rnd, t = found
    algorithmic = 28.0 * (1 << 20)
    # the {hi, lo} planes of the fp64 slice sums: ~19x the compulsory 29.4 MB, 0.07 ms at 8 TB/s
    assert 5.0 * algorithmic < t["bytes"] < 40.0 * algorithmic, (rnd, t)
    assert 1.8 < t["f_fetch"] < 2.1 and 0.95 < t["f_write"] < 1.05, t


def test_a_profile_of_another_kernel_is_refused():
    path = os.path.join(ROOT, "profiles", "r4", "pmc_force_kernel.json")
    pmc = json.load(open(path))
    assert bench.pmc_traffic(pmc, "void nbx::(anonymous namespace)::accel_fast3l_kernel<3, 4, 3, 4, 64, 1, 0>(nbx::KArgs)") is None


def test_plain_gpus_n_starts_the_ranks_as_a_child_process():
    """No GPU here: each rank must get as far as bench.py's own 'needs a GPU' exit -- proof that `--gpus 2` without a launcher
    started two ranks under torch.distributed.run (it used to exit 1 with a usage line before importing anything)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--bodies", "4096"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "must be launched with" not in p.stderr
    assert p.stderr.count("bench.py needs a GPU") >= 2, p.stderr[-2000:]


def test_cpu_baseline_leg_runs_its_solvers_in_child_processes(reference_library):
    """bench.py's cpu_baseline on a small sample: the reference's object code, one fresh process per thread count (OpenMP sizes its
    pool at start-up), both solvers reported in ordered pairs per second, the --cpu-baseline-n override honoured."""
    out = bench.cpu_baseline(8192, 3, 1, budget_s=0.05, n_sample=3000)
    assert out["kind"] == "reference" and out["cores"] >= 1 and out["value"] > 0
    assert [r["n"] for r in out["all_runs"]][:2] == [3000, 3000]
    assert {r["solver"] for r in out["all_runs"]} == {"brute_force_omp_n_body_2<3>", "brute_force_omp_n_body_1<3>"}
    assert "first 3000 bodies" in out["sample"]


class _OneRank:
    """The calls dump_outputs makes on a one-rank system: layout.bounds, gather_bodies (state), compute_forces and forces."""

    def __init__(self, state, forces):
        self.state, self.f, self.computed = state, forces, False
        self.layout = types.SimpleNamespace(bounds=lambda: (0, state.shape[0]))

    def gather_bodies(self, bodies):
        return self.state.copy()

    def compute_forces(self):
        self.computed = True

    def forces(self, G):
        assert self.computed
        return self.f.copy()


def _dump(tmp_path, n, dim):
    import numpy as np
    rng = np.random.default_rng(7)
    state, forces = rng.standard_normal((n, 2 * dim + 1)), rng.standard_normal((n, dim))
    out = tmp_path / f"dump_{n}_{dim}"
    bench.dump_outputs(str(out), _OneRank(state, forces), state, 1.0, dim, 1, 0, None)
    return out, state, forces


def test_dump_outputs_writes_the_whole_state_when_it_fits(tmp_path):
    import numpy as np
    out, state, forces = _dump(tmp_path, 5000, 3)
    assert sorted(os.listdir(out)) == ["forces.npy", "positions.npy", "velocities.npy"]
    for name, want in (("positions", state[:, :3]), ("velocities", state[:, 3:6]), ("forces", forces)):
        got = np.load(out / f"{name}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, want)


def test_dump_outputs_of_2_to_the_20_bodies_is_a_fixed_sample_within_64_mb(tmp_path):
    import numpy as np
    n = 1 << 20
    out, state, forces = _dump(tmp_path, n, 3)
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 * 10**6
    rows = np.load(out / "rows.npy")
    assert rows.dtype == np.float64 and rows.size > n // 2 and np.all(np.diff(rows) > 0)
    idx = rows.astype(np.int64)
    assert np.array_equal(np.load(out / "forces.npy"), forces[idx])
    assert np.array_equal(np.load(out / "positions.npy"), state[idx, :3])
    again, _, _ = _dump(tmp_path / "again", n, 3)
    assert np.array_equal(np.load(again / "rows.npy"), rows)       # the same rows from run to run
