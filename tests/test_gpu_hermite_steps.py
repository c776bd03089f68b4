"""GPU: the fourth-order Hermite scheme with block time steps (nbx_ctx_step_hermite_block) against its fp64 specification,
hermite.hermite_block_spec fed hermite.accel_jerk_rows of the predicted positions and velocities rounded to fp32 (as the device's
sources are).

What must be EQUAL: the history (n_active, dn), pair_terms, the clock's counts and the final levels, on runs whose choices keep a
margin of 1e-2 from every threshold (asserted here, on the very runs compared; tests/test_hermite_cpu.py has the certificate and
says why equality is asked over two blocks of the eccentric binary and not over a period).
What must be CLOSE: positions and velocities of the levels = 0 runs.  The tolerance is 4 times the deviation that
nbx_ctx_step_kdk_block(levels = 0) of the parent commit -- the same pair arithmetic and sources, second order -- shows from
blocksteps.block_leapfrog_spec on the same systems, measured with tests/measure/hermite_steps.py deviation
(profiles/r20/hermite_block.txt):

    PARENT_DEVIATION below, max over bodies and components of |device - specification|, (positions, velocities):
    (3, soft): (5.248e-06, 1.084e-06);  (3, newton): (7.228e-05, 1.447e-05);  (2, soft): (1.443e-06, 2.881e-07);
    (2, newton): (8.597e-05, 1.632e-05) -- against displacements of 1.0e+02 to 2.4e+02 and velocity changes of 0.45 to 31.
    This loop's own deviations from its specification, as measured:
    (3, soft): (5.255e-06, 1.084e-06);  (3, newton): (7.211e-05, 1.447e-05);  (2, soft): (1.444e-06, 2.881e-07);
    (2, newton): (8.502e-05, 1.632e-05): 0.99 to 1.00 of the parent's, the bound being 4.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_adaptive_step_cpu import BIN_DT_MAX, BIN_EPS, BIN_EXTRA, BIN_G, BIN_PERIOD, binary_system
from test_block_steps_cpu import BIN_BLOCKS, BIN_LEVELS, THREE_CONTROL, THREE_EPS, THREE_G, three_level_system
from test_ctx_adaptive_step_cpu import kinetic_plus_newton_potential
from test_hermite_cpu import BIN_ETA_START, EQUAL_BLOCKS, EQUAL_ETAS, EQUAL_MARGIN, PAIRED, accel_jerk_fn, binary_hermite_control, binary_hermite_run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (dim, law) -> (positions, velocities): nbx_ctx_step_kdk_block(levels = 0) against block_leapfrog_spec, 600 bodies, 5 steps of dt = 2
PARENT_DEVIATION = {
    (3, "soft"): (5.248e-06, 1.084e-06), (3, "newton"): (7.228e-05, 1.447e-05),
    (2, "soft"): (1.443e-06, 2.881e-07), (2, "newton"): (8.597e-05, 1.632e-05),
}
THREE_HERMITE = dict(eta=0.02, dt_max=THREE_CONTROL["dt_max"], levels=THREE_CONTROL["levels"])


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


def binary_step(c, eta, n_blocks, **more):
    return c.step_hermite_block(eta, BIN_DT_MAX, BIN_LEVELS, n_blocks, G=BIN_G, eta_start=BIN_ETA_START, **more)


def three_step(c, n_blocks=1, **more):
    return c.step_hermite_block(THREE_HERMITE["eta"], THREE_HERMITE["dt_max"], THREE_HERMITE["levels"], n_blocks, G=THREE_G, **more)


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
def test_levels_zero_is_the_shared_step_hermite_loop(nbx, oracle, dim, law):
    """tests/test_gpu_block_steps.py's levels = 0 systems: 600 generated bodies, dt = 2, 5 steps, a coupling strong enough to bend the
    orbits."""
    n, steps, dt = 600, 5, 2.0
    eps, gs = (50.0, 1e24) if law == "soft" else (2.0e4, 1e22)
    G = oracle.G * gs
    b0 = oracle.round_inputs_to_f32(oracle.generate(35 + dim, n, dim))
    spec = nbx.hermite.hermite_block_spec(b0, accel_jerk_fn(nbx, G, eps, law, rounded=True), dict(eta=0.02, dt_max=dt, levels=0), steps, 1 << 20)
    ref = spec[0]
    with context(nbx, b0, law, eps) as c:
        clock = c.step_hermite_block(0.02, dt, 0, steps, G=G)
        assert_same_bookkeeping(c, clock, spec[1], spec[2], spec[3])
        assert clock.evaluations == clock.substeps + 1 == steps + 1
        got = downloaded(c, b0)
        out = np.zeros((n, dim))
        assert nbx.load_library().nbx_ctx_get_forces(c.h, ctypes.c_double(G), out.ctypes.data) == 5   # NBX_ERR_STATE: no valid accelerations afterwards
    dev_x, dev_v = np.abs(got[:, :dim] - ref[:, :dim]).max(), np.abs(got[:, dim:2 * dim] - ref[:, dim:2 * dim]).max()
    tol_x, tol_v = (4.0 * d for d in PARENT_DEVIATION[(dim, law)])
    dv = np.abs(ref[:, dim:2 * dim] - b0[:, dim:2 * dim]).max()
    print(f"{dim}D {law}: deviation x {dev_x:.3e} (bound {tol_x:.3e}), v {dev_v:.3e} (bound {tol_v:.3e}); the run changes v by up to {dv:.3e}")
    assert dv > 1e-3 and np.isfinite(got).all()
    assert dev_x <= tol_x and dev_v <= tol_v


# ---- the eccentric binary ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eta", EQUAL_ETAS)
def test_two_blocks_of_the_binary_equal_the_specification(nbx, eta):
    b0 = binary_system(BIN_EXTRA)
    ref, spec_clock, spec_history, spec_levels, margin = binary_hermite_run(nbx, BIN_EXTRA, eta, EQUAL_BLOCKS, rounded=True)
    assert margin >= EQUAL_MARGIN and spec_clock["finished"] == 1 and spec_clock["deepest_level"] >= 2
    with context(nbx, b0, "newton", BIN_EPS) as c:
        clock = binary_step(c, eta, EQUAL_BLOCKS)
        assert_same_bookkeeping(c, clock, spec_clock, spec_history, spec_levels)
        got = downloaded(c, b0)
    dev_x, dev_v = np.abs(got[:2, :3] - ref[:2, :3]).max(), np.abs(got[:2, 3:6] - ref[:2, 3:6]).max()
    print(f"binary, {EQUAL_BLOCKS} blocks, eta = {eta:g}: {clock.substeps} substeps, margin {margin:.3e}, deepest level {clock.deepest_level}, "
          f"the pair's deviation x {dev_x:.3e}, v {dev_v:.3e}")
    assert np.isfinite(got).all()


@pytest.mark.parametrize("extra", (0, BIN_EXTRA))
@pytest.mark.parametrize("eta", [eta for eta, _ in PAIRED])
def test_eccentric_binary_over_one_period(nbx, eta, extra):
    b0 = binary_system(extra)
    n = b0.shape[0]
    ref, spec_clock, spec_history, spec_levels, margin = binary_hermite_run(nbx, extra, eta, BIN_BLOCKS, rounded=True)
    assert spec_clock["finished"] == 1
    e0_spec = kinetic_plus_newton_potential(b0, BIN_G, BIN_EPS)
    figure = abs(kinetic_plus_newton_potential(ref, BIN_G, BIN_EPS) / e0_spec - 1.0)
    with context(nbx, b0, "newton", BIN_EPS) as c:
        e0 = sum(c.energy(BIN_G))
        clock = binary_step(c, eta, BIN_BLOCKS)
        e1 = sum(c.energy(BIN_G))                                 # straight after: the corrected state at one time
        got = downloaded(c, b0)
    assert clock.finished == 1 and clock.status == 0 and clock.t == BIN_PERIOD and clock.evaluations == clock.substeps + 1
    error = abs(e1 / e0 - 1.0)
    off = abs(clock.pair_terms / spec_clock["pair_terms"] - 1.0)
    print(f"binary n = {n}, eta = {eta:g}: {clock.substeps} substeps (specification {spec_clock['substeps']}), pair terms {clock.pair_terms} "
          f"({off:.2%} from the specification's), deepest level {clock.deepest_level}, |E/E0 - 1| device {error:.3e}, specification {figure:.3e}")
    assert e0 < 0 and np.isfinite(got).all()
    assert error <= 1.5 * figure
    assert off <= 0.01


# ---- the cap, a replay, a later call ---------------------------------------------------------------------------------------------------

def test_the_cap_stops_the_loop_with_status_2(nbx):
    """The binary's two-block run, cut after 3 substeps: the prefix of a run whose margin is certified."""
    b0 = binary_system(BIN_EXTRA)
    cap, eta = 3, EQUAL_ETAS[0]
    fn = accel_jerk_fn(nbx, BIN_G, BIN_EPS, "newton", rounded=True)
    ref, spec_clock, spec_history, spec_levels, margin = nbx.hermite.hermite_block_spec(b0, fn, binary_hermite_control(eta), EQUAL_BLOCKS, cap)
    assert spec_clock["status"] == 2 and spec_clock["substeps"] == cap and margin >= EQUAL_MARGIN
    with context(nbx, b0, "newton", BIN_EPS) as c:
        clock = binary_step(c, eta, EQUAL_BLOCKS, max_substeps=cap)
        assert clock.status == 2 and clock.finished == 0 and clock.substeps == cap and clock.evaluations == cap + 1
        assert_same_bookkeeping(c, clock, spec_clock, spec_history, spec_levels)
        assert binary_step(c, eta, 0) is None                     # n_blocks = 0 does nothing
        assert c.block_clock().substeps == cap
        # the bodies are at their own times, and the fp32 sources are their roundings again: what a fresh context holds
        got = downloaded(c, b0)
        c.compute_accel_active([0, 1, 2])
        here = c.forces_active(BIN_G)
        with context(nbx, got, "newton", BIN_EPS) as fresh:
            fresh.compute_accel_active([0, 1, 2])
            assert np.array_equal(here, fresh.forces_active(BIN_G))
    assert np.isfinite(got).all() and not np.array_equal(got[:2], b0[:2])


@pytest.mark.parametrize("window", (None, "1", "64"))
def test_two_identical_calls_give_identical_bits(nbx, monkeypatch, window):
    """... and the results do not depend on the window of looks at `stopped`."""
    if window:
        monkeypatch.setenv("NBODY_HIP_STEP_WINDOW", window)
    b0 = three_level_system(3)
    runs = []
    for _ in range(2):
        with context(nbx, b0, "newton", THREE_EPS) as c:
            clock = three_step(c)
            assert clock.finished == 1 and clock.status == 0 and clock.deepest_level >= 2
            runs.append((downloaded(c, b0), c.block_history(), c.block_levels(), (clock.t, clock.ticks, clock.pair_terms, clock.substeps)))
            if not runs[1:]:
                # a later call on the same context starts afresh: it is the call a fresh context makes from these bodies
                mid = runs[0][0]
                three_step(c)
                again = (downloaded(c, b0), c.block_history(), c.block_levels())
                with context(nbx, mid, "newton", THREE_EPS) as fresh:
                    three_step(fresh)
                    assert np.array_equal(again[0], downloaded(fresh, mid)) and np.array_equal(again[2], fresh.block_levels())
                    assert all(np.array_equal(x, y) for x, y in zip(again[1], fresh.block_history()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][2], runs[1][2]) and runs[0][3] == runs[1][3]
    assert all(np.array_equal(x, y) for x, y in zip(runs[0][1], runs[1][1]))
    assert not np.array_equal(runs[0][0], b0)
    _digests.append(runs[0][0].tobytes())
    assert len(set(_digests)) == 1                               # the same bits under every window


_digests = []


def test_a_kick_drift_kick_call_after_a_hermite_call_is_a_fresh_contexts(nbx):
    b0 = three_level_system(3)
    kdk = lambda c: c.step_kdk_block(THREE_CONTROL["accel_length"], THREE_CONTROL["dt_max"], THREE_CONTROL["levels"], 1, G=THREE_G)
    with context(nbx, b0, "newton", THREE_EPS) as c:
        three_step(c)
        mid = downloaded(c, b0)
        clock = kdk(c)
        after = (downloaded(c, b0), c.block_history(), c.block_levels(), (clock.t, clock.ticks, clock.pair_terms, clock.substeps, clock.evaluations))
    with context(nbx, mid, "newton", THREE_EPS) as fresh:
        clock = kdk(fresh)
        assert np.array_equal(after[0], downloaded(fresh, mid)) and np.array_equal(after[2], fresh.block_levels())
        assert all(np.array_equal(x, y) for x, y in zip(after[1], fresh.block_history()))
        assert after[3] == (clock.t, clock.ticks, clock.pair_terms, clock.substeps, clock.evaluations)


def test_a_sum_that_is_not_finite_stops_the_loop(nbx):
    """One NaN coordinate, uploaded: every sum is NaN, evaluation 0 sets status 1 and no body is changed."""
    b0 = three_level_system(3, n=40)
    b0[5, 0] = np.nan
    with context(nbx, b0, "newton", THREE_EPS) as c:
        clock = three_step(c)
        assert clock.status == 1 and clock.finished == 0 and clock.substeps == 0 and clock.evaluations == 1 and clock.ticks == 0
        got = downloaded(c, b0)
        assert len(c.block_history()[0]) == 0
    assert np.array_equal(got, b0, equal_nan=True)


def test_refusals_on_a_context(nbx):
    b0 = three_level_system(3, n=40)
    lib = nbx.load_library()
    k = nbx.HermiteControl(0.02, 0.01, 0.1, 0.0, 4, 0)
    clock = nbx.BlockClock()
    with nbx.Context(40, 3) as c:
        assert lib.nbx_ctx_step_hermite_block(c.h, 1.0, ctypes.byref(k), 1, 8) == 5      # nothing uploaded
        c.upload(b0)
        assert lib.nbx_ctx_step_hermite_block(c.h, 1.0, ctypes.byref(k), 1, 8) == 5      # softening 0
        c.set_softening(THREE_EPS)
        assert lib.nbx_ctx_get_block_clock(c.h, ctypes.byref(clock)) == 5                # no call yet
        assert lib.nbx_ctx_step_hermite_block(c.h, 1.0, ctypes.byref(k), 0, 8) == 0 and lib.nbx_ctx_get_block_clock(c.h, ctypes.byref(clock)) == 5
        assert lib.nbx_ctx_step_hermite_block(c.h, 1.0, ctypes.byref(k), 1, 8) == 0 and lib.nbx_ctx_get_block_clock(c.h, ctypes.byref(clock)) == 0
        bad = nbx.HermiteControl(0.0, 0.01, 0.1, 0.0, 4, 0)
        assert lib.nbx_ctx_step_hermite_block(c.h, 1.0, ctypes.byref(bad), 1, 8) == 1 and "eta" in lib.nbx_last_error_detail().decode()
    with nbx.Context(40, 3, n_shards=2, shard=0) as c:
        c.upload(b0)
        c.set_softening(THREE_EPS)
        assert lib.nbx_ctx_step_hermite_block(c.h, 1.0, ctypes.byref(k), 1, 8) == 5


# ---- the harness -------------------------------------------------------------------------------------------------------------------

def test_harness_row(tmp_path):
    """nbody_sim -N 4096 -m g --init plummer --law newton --softening 2048 --integrator h4b --eta 0.02 --levels 6 --dt 4 --steps 4
    --energy-every 2: the row is Hermite_HIP_4blocks_h4b, one `Block steps:` line gives the substeps, t = 16, the pair terms next to a
    shared step's and the deepest level, and the energy lines at 0, 2, 4 show a bound system whose energy holds."""
    sim = os.path.join(ROOT, "nbody_sim")
    assert os.path.exists(sim)
    cmd = [sim, "-N", "4096", "-m", "g", "--init", "plummer", "--seed", "5", "--G", "0.1", "--law", "newton", "--softening", "2048", "--steps", "4",
           "--energy-every", "2", "--dt", "4", "--integrator", "h4b", "--eta", "0.02", "--levels", "6"]
    p = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    found = [os.path.join(d, f_) for d, _, files in os.walk(tmp_path) for f_ in files if f_.endswith(".csv")]
    rows = [line.split(",")[0] for path in sorted(found) for line in open(path) if line.startswith(("Leapfrog_HIP", "Hermite_HIP"))]
    assert rows == ["Hermite_HIP_4blocks_h4b"], rows
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
