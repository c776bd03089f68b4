"""GPU: kick-drift-kick with block time steps (nbx_ctx_step_kdk_block) against its fp64 specification,
blocksteps.block_leapfrog_spec fed the all-pairs sums of positions rounded to fp32 (as the device's sources are).

What must be EQUAL: the history (n_active, dn), pair_terms, the clock's counts and the final levels -- every level choice is a
comparison of sqrt(c / a_i) with a step, and the specification's choices keep a margin of 1e-4 from every threshold (asserted here, on
the very runs compared; tests/test_block_steps_cpu.py has the certificate), two orders above what the fp32 sums can move a_i by.
What must be CLOSE: positions and velocities.  The tolerance for the eccentric binary is 4 times the deviation that
nbx_ctx_step_kdk_adaptive (pow2) -- the same pair arithmetic and sources, another summation order and step sequence -- shows from
leaves.adaptive_leapfrog_spec on the same system and c, measured with tests/measure/block_steps.py (profiles/r19/block_steps.txt):

    PARENT_DEVIATION below, max over bodies and components of |device - specification|, (positions, velocities), with and without
    the 256 extra bodies alike:  c = 4e-3: (1.188e-06, 1.137e-06);  c = 1e-3: (1.468e-07, 1.562e-07);  c = 2.5e-4: (1.815e-07, 1.340e-07)
    -- the same digits from a build of the parent commit.  The block loop's own deviations, as measured: (8.458e-07, 8.150e-07),
    (1.147e-07, 1.372e-07), (1.175e-07, 7.017e-08).
"""
import os
import subprocess

import numpy as np
import pytest

from test_adaptive_step_cpu import BIN_C, BIN_DT_MAX, BIN_EPS, BIN_EXTRA, BIN_G, BIN_PERIOD, binary_system
from test_block_steps_cpu import (BIN_BLOCKS, BIN_LEVELS, MARGIN, THREE_BLOCKS, THREE_CONTROL, THREE_EPS, THREE_G, binary_block_control, rows_accel_fn,
                                  three_level_system)
from test_ctx_adaptive_step_cpu import kinetic_plus_newton_potential

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (extra, c) -> (positions, velocities): nbx_ctx_step_kdk_adaptive(pow2) against adaptive_leapfrog_spec over one period
PARENT_DEVIATION = {
    (0, 4.0e-3): (1.188e-06, 1.137e-06), (0, 1.0e-3): (1.468e-07, 1.562e-07), (0, 2.5e-4): (1.815e-07, 1.340e-07),
    (256, 4.0e-3): (1.188e-06, 1.137e-06), (256, 1.0e-3): (1.468e-07, 1.562e-07), (256, 2.5e-4): (1.815e-07, 1.340e-07),
}


def rounded(accel):
    """the device's sources are the fp32 roundings of its fp64 positions"""
    return lambda b, active: accel(b.astype(np.float32).astype(np.float64), active)


def context(nbx, b, law, eps):
    c = nbx.Context(b.shape[0], (b.shape[1] - 1) // 2)
    c.upload(b)
    c.set_softening(eps)
    if law == "newton":
        c.set_law(nbx.FORCE_LAW_NEWTON)
    return c


def downloaded(c, b0):
    got = b0.copy()
    c.download(got)
    return got


def assert_same_bookkeeping(c, clock, spec_clock, spec_history, spec_levels):
    n_active, dn = c.block_history()
    assert np.array_equal(n_active, spec_history[:, 0]) and np.array_equal(dn, spec_history[:, 1])
    assert np.array_equal(c.block_levels(), spec_levels)
    for name in ("ticks", "pair_terms", "substeps", "evaluations", "deepest_level", "finished", "status"):
        assert getattr(clock, name) == spec_clock[name], name
    assert clock.t == spec_clock["t"]


# ---- levels = 0 ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("law", ("soft", "newton"))
@pytest.mark.parametrize("dim", (3, 2))
def test_levels_zero_is_the_fixed_step_loop(nbx, oracle, dim, law):
    """tests/test_gpu_softening.py's kick-drift-kick case (600 generated bodies, dt = 2, 5 steps, a coupling strong enough to bend the
    orbits) with a softening length, levels = 0: leaves.leapfrog_spec's fixed-step kick-drift-kick, to that test's tolerances --
    velocities atol = 2e-5 dv, positions rtol = 1e-9."""
    n, steps, dt = 600, 5, 2.0
    eps, gs = (50.0, 1e24) if law == "soft" else (2.0e4, 1e22)                  # tests/test_gpu_ctx_adaptive_step.py's SPEC_CASES
    G = oracle.G * gs
    b0 = oracle.round_inputs_to_f32(oracle.generate(35 + dim, n, dim))
    accel = rounded(rows_accel_fn(G, eps, law))
    ref = nbx.leaves.leapfrog_spec(b0, lambda b: accel(b, np.arange(n)), dt, steps, "kdk")
    spec = nbx.blocksteps.block_leapfrog_spec(b0, accel, dict(accel_length=1.0, dt_max=dt, levels=0), steps, 1 << 20)
    assert np.array_equal(spec[0], ref)
    with context(nbx, b0, law, eps) as c:
        clock = c.step_kdk_block(1.0, dt, 0, steps, G=G)
        assert_same_bookkeeping(c, clock, spec[1], spec[2], spec[3])
        got = downloaded(c, b0)
        lib = nbx.load_library()
        out = np.zeros((n, dim))
        assert lib.nbx_ctx_get_forces(c.h, G, out.ctypes.data) == 5              # NBX_ERR_STATE: no valid accelerations afterwards
    dv = np.abs(ref[:, dim:2 * dim] - b0[:, dim:2 * dim]).max()
    err_v = np.abs(got[:, dim:2 * dim] - ref[:, dim:2 * dim]).max()
    print(f"{dim}D {law}: dv {dv:.3e}, largest velocity error {err_v:.3e} = {err_v / dv:.2e} dv")
    assert dv > 1e-3
    assert np.allclose(got[:, dim:2 * dim], ref[:, dim:2 * dim], rtol=0, atol=2e-5 * dv)
    assert np.allclose(got[:, :dim], ref[:, :dim], rtol=1e-9, atol=0)


# ---- the eccentric binary ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra", (0, BIN_EXTRA))
@pytest.mark.parametrize("c", BIN_C)
def test_eccentric_binary(nbx, c, extra):
    b0 = binary_system(extra)
    n = b0.shape[0]
    accel = rounded(rows_accel_fn(BIN_G, BIN_EPS, "newton"))
    ref, spec_clock, spec_history, spec_levels, margin = nbx.blocksteps.block_leapfrog_spec(b0, accel, binary_block_control(c), BIN_BLOCKS, 1 << 20)
    assert margin >= MARGIN and spec_clock["finished"] == 1
    e0_spec = kinetic_plus_newton_potential(b0, BIN_G, BIN_EPS)
    figure = abs(kinetic_plus_newton_potential(ref, BIN_G, BIN_EPS) / e0_spec - 1.0)
    with context(nbx, b0, "newton", BIN_EPS) as ctx:
        e0 = sum(ctx.energy(BIN_G))
        clock = ctx.step_kdk_block(c, BIN_DT_MAX, BIN_LEVELS, BIN_BLOCKS, G=BIN_G)
        assert_same_bookkeeping(ctx, clock, spec_clock, spec_history, spec_levels)
        e1 = sum(ctx.energy(BIN_G))
        got = downloaded(ctx, b0)
    assert clock.t == BIN_PERIOD and clock.finished == 1
    error = abs(e1 / e0 - 1.0)
    dev_x, dev_v = np.abs(got[:, :3] - ref[:, :3]).max(), np.abs(got[:, 3:6] - ref[:, 3:6]).max()
    tol_x, tol_v = (4.0 * d for d in PARENT_DEVIATION[(extra, c)])
    print(f"binary n = {n}, c = {c:g}: {clock.substeps} substeps, pair terms {clock.pair_terms} (shared step: {len(spec_history) * n * n}), deepest level "
          f"{clock.deepest_level}, |E/E0 - 1| device {error:.3e}, specification {figure:.3e}; deviation x {dev_x:.3e} (bound {tol_x:.3e}), v {dev_v:.3e} (bound {tol_v:.3e})")
    assert e0 < 0 and error <= 1.5 * figure
    assert dev_x <= tol_x and dev_v <= tol_v


# ---- three populated levels ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("build", ("short", "long", "default"))
@pytest.mark.parametrize("dim", (3, 2))
def test_three_populated_levels(nbx, monkeypatch, dim, build):
    """A random 600-body system with one tight pair: the histories, the levels and the clocks are equal, whichever build of the list
    kernel evaluates the active bodies."""
    if build != "default":
        monkeypatch.setenv("NBODY_HIP_ACTIVE_LONG_LIST", {"short": str(1 << 31), "long": "1"}[build])
    b0 = three_level_system(dim)
    accel = rounded(rows_accel_fn(THREE_G, THREE_EPS, "newton"))
    ref, spec_clock, spec_history, spec_levels, margin = nbx.blocksteps.block_leapfrog_spec(b0, accel, THREE_CONTROL, THREE_BLOCKS, 1 << 20)
    assert margin >= MARGIN and len(np.unique(spec_levels)) >= 3 and len(np.unique(spec_history[:, 0])) >= 3
    with context(nbx, b0, "newton", THREE_EPS) as c:
        clock = c.step_kdk_block(THREE_CONTROL["accel_length"], THREE_CONTROL["dt_max"], THREE_CONTROL["levels"], THREE_BLOCKS, G=THREE_G)
        assert_same_bookkeeping(c, clock, spec_clock, spec_history, spec_levels)
        got = downloaded(c, b0)
    dv = np.abs(ref[:, dim:2 * dim] - b0[:, dim:2 * dim]).max()
    err_v, err_x = np.abs(got[:, dim:2 * dim] - ref[:, dim:2 * dim]).max(), np.abs(got[:, :dim] - ref[:, :dim]).max()
    print(f"three levels D = {dim}, {build}: {clock.substeps} substeps, margin {margin:.2e}, velocity error {err_v / dv:.2e} dv, position error {err_x:.2e}")
    assert np.isfinite(got).all()


# ---- the cap, a replay, a later call ---------------------------------------------------------------------------------------------------

def test_the_cap_stops_the_loop_with_status_2(nbx):
    b0 = three_level_system(3)
    accel = rounded(rows_accel_fn(THREE_G, THREE_EPS, "newton"))
    cap = 7
    ref, spec_clock, spec_history, spec_levels, _ = nbx.blocksteps.block_leapfrog_spec(b0, accel, THREE_CONTROL, THREE_BLOCKS, cap)
    assert spec_clock["status"] == 2 and spec_clock["substeps"] == cap
    with context(nbx, b0, "newton", THREE_EPS) as c:
        clock = c.step_kdk_block(THREE_CONTROL["accel_length"], THREE_CONTROL["dt_max"], THREE_CONTROL["levels"], THREE_BLOCKS, max_substeps=cap, G=THREE_G)
        assert clock.status == 2 and clock.finished == 0 and clock.substeps == cap and clock.evaluations == cap + 1
        assert_same_bookkeeping(c, clock, spec_clock, spec_history, spec_levels)
        assert c.step_kdk_block(THREE_CONTROL["accel_length"], THREE_CONTROL["dt_max"], THREE_CONTROL["levels"], 0, G=THREE_G) is None   # n_blocks = 0 does nothing
        assert c.block_clock().substeps == cap


@pytest.mark.parametrize("window", (None, "1", "64"))
def test_two_identical_calls_give_identical_bits(nbx, monkeypatch, window):
    """... and the results do not depend on the window of looks at `stopped`."""
    if window:
        monkeypatch.setenv("NBODY_HIP_STEP_WINDOW", window)
    b0 = three_level_system(3)
    runs = []
    for _ in range(2):
        with context(nbx, b0, "newton", THREE_EPS) as c:
            clock = c.step_kdk_block(THREE_CONTROL["accel_length"], THREE_CONTROL["dt_max"], THREE_CONTROL["levels"], THREE_BLOCKS, G=THREE_G)
            runs.append((downloaded(c, b0), c.block_history(), c.block_levels(), (clock.t, clock.ticks, clock.pair_terms, clock.substeps)))
            if not runs[1:]:
                # a later call on the same context starts from fresh levels: it is the call a fresh context makes from these bodies
                mid = runs[0][0]
                c.step_kdk_block(THREE_CONTROL["accel_length"], THREE_CONTROL["dt_max"], THREE_CONTROL["levels"], 1, G=THREE_G)
                again = (downloaded(c, b0), c.block_history(), c.block_levels())
                with context(nbx, mid, "newton", THREE_EPS) as fresh:
                    fresh.step_kdk_block(THREE_CONTROL["accel_length"], THREE_CONTROL["dt_max"], THREE_CONTROL["levels"], 1, G=THREE_G)
                    assert np.array_equal(again[0], downloaded(fresh, mid)) and np.array_equal(again[2], fresh.block_levels())
                    assert all(np.array_equal(x, y) for x, y in zip(again[1], fresh.block_history()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][2], runs[1][2]) and runs[0][3] == runs[1][3]
    assert all(np.array_equal(x, y) for x, y in zip(runs[0][1], runs[1][1]))
    _digests.append(runs[0][0].tobytes())
    assert len(set(_digests)) == 1                               # the same bits under every window


_digests = []


def test_a_sum_that_is_not_finite_stops_the_loop(nbx):
    """One NaN coordinate, uploaded: every sum is NaN, the first evaluation sets status 1 and nobody is kicked."""
    b0 = three_level_system(3, n=40)
    b0[5, 0] = np.nan
    with context(nbx, b0, "newton", THREE_EPS) as c:
        clock = c.step_kdk_block(THREE_CONTROL["accel_length"], THREE_CONTROL["dt_max"], THREE_CONTROL["levels"], 1, G=THREE_G)
        assert clock.status == 1 and clock.finished == 0 and clock.substeps == 0 and clock.evaluations == 1 and clock.ticks == 0
        got = downloaded(c, b0)
        assert len(c.block_history()[0]) == 0
    keep = np.arange(40) != 5
    assert np.array_equal(got[keep], b0[keep])


def test_refusals_on_a_context(nbx):
    b0 = three_level_system(3, n=40)
    lib = nbx.load_library()
    import ctypes
    k = nbx.BlockControl(1e-3, 0.1, 0.0, 4, 0)
    clock = nbx.BlockClock()
    with nbx.Context(40, 3) as c:
        assert lib.nbx_ctx_step_kdk_block(c.h, 1.0, ctypes.byref(k), 1, 8) == 5          # nothing uploaded
        c.upload(b0)
        assert lib.nbx_ctx_step_kdk_block(c.h, 1.0, ctypes.byref(k), 1, 8) == 5          # softening 0
        c.set_softening(THREE_EPS)
        assert lib.nbx_ctx_get_block_clock(c.h, ctypes.byref(clock)) == 5                # no call yet
        assert lib.nbx_ctx_step_kdk_block(c.h, 1.0, ctypes.byref(k), 0, 8) == 0 and lib.nbx_ctx_get_block_clock(c.h, ctypes.byref(clock)) == 5
        assert lib.nbx_ctx_step_kdk_block(c.h, 1.0, ctypes.byref(k), 1, 8) == 0 and lib.nbx_ctx_get_block_clock(c.h, ctypes.byref(clock)) == 0
    with nbx.Context(40, 3, n_shards=2, shard=0) as c:
        c.upload(b0)
        c.set_softening(THREE_EPS)
        assert lib.nbx_ctx_step_kdk_block(c.h, 1.0, ctypes.byref(k), 1, 8) == 5


# ---- the harness -------------------------------------------------------------------------------------------------------------------

def test_harness_row(tmp_path):
    """nbody_sim -N 4096 -m g --init plummer --law newton --softening 2048 --integrator kdkb --accel-length 4 --levels 6 --dt 4 --steps 4
    --energy-every 2: the row is Leapfrog_HIP_4blocks_kdkb, one `Block steps:` line gives the substeps, t = 16, the pair terms next to a
    shared step's and the deepest level, and the energy lines at 0, 2, 4 show a bound system whose energy holds."""
    sim = os.path.join(ROOT, "nbody_sim")
    assert os.path.exists(sim)
    cmd = [sim, "-N", "4096", "-m", "g", "--init", "plummer", "--seed", "5", "--G", "0.1", "--law", "newton", "--softening", "2048", "--steps", "4",
           "--energy-every", "2", "--dt", "4", "--integrator", "kdkb", "--accel-length", "4", "--levels", "6"]
    p = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    found = [os.path.join(d, f_) for d, _, files in os.walk(tmp_path) for f_ in files if f_.endswith(".csv")]
    rows = [line.split(",")[0] for path in sorted(found) for line in open(path) if line.startswith("Leapfrog_HIP")]
    assert rows == ["Leapfrog_HIP_4blocks_kdkb"], rows
    summary = [line for line in p.stdout.splitlines() if line.startswith("Block steps: ")]
    assert len(summary) == 1, p.stdout
    line = summary[0]
    substeps = int(line.split("Block steps: ")[1].split(" substeps")[0])
    t = float(line.split("t = ")[1].split(",")[0])
    terms = int(line.split("pair terms ")[1].split(" ")[0])
    shared = int(line.split("a shared step: ")[1].split(",")[0])
    deepest = int(line.split("deepest level ")[1].split(" ")[0])
    assert t == 16.0 and 4 <= substeps <= 4 << 6 and 0 <= deepest <= 6
    assert shared == (substeps + 2) * 4096 * 4096 and 2 * 2 * 4096 * 4096 <= terms <= shared      # two calls: two closing evaluations
    energy = [x for x in p.stdout.splitlines() if x.startswith("step ")]
    assert [x.split()[1] for x in energy] == ["0", "2", "4"] and all("E = " in x for x in energy), p.stdout
    for x in energy:
        assert float(x.split("E = ")[1].split()[0]) < 0, x
        if not x.startswith("step 0 "):
            assert float(x.split("|dE/E0| = ")[1].split()[0]) < 1e-2, x
