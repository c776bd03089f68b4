"""CPU: forces on a list of targets and kick-drift-kick with block time steps -- nbx_ctx_compute_accel_active, _get_forces_active,
nbx_ctx_step_kdk_block, _get_block_clock, _get_block_history, _get_block_levels -- as far as they can be judged without a device: the
six names in the header, the version script, the library and capi.py; every refusal that is decided before a device is needed; the
invariants of the fp64 specification (blocksteps.block_leapfrog_spec); and the certificate of tests/test_gpu_block_steps.py on
tests/test_adaptive_step_cpu.py's eccentric binary: the choices keep a margin that the device's fp32 sums cannot cross, the energy
error is that of the shared-step loop, and the pair terms are at least 8 times fewer."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

from test_adaptive_step_cpu import BIN_C, BIN_DT_MAX, BIN_DT_MIN, BIN_EPS, BIN_EXTRA, BIN_G, BIN_PERIOD, binary_system
from test_ctx_adaptive_step_cpu import ctx_accel_fn, kinetic_plus_newton_potential

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nbx_ctx_compute_accel_active", "nbx_ctx_get_forces_active", "nbx_ctx_step_kdk_block", "nbx_ctx_get_block_clock",
         "nbx_ctx_get_block_history", "nbx_ctx_get_block_levels")
NBX_ERR_INVALID = 1
BIN_LEVELS, BIN_BLOCKS = 16, 8
MARGIN = 1.0e-4


def rows_accel_fn(G, eps, law):
    """accel_rows_fn of blocksteps.block_leapfrog_spec for the all-pairs context: ctx_accel_fn's sums for the rows `active` only."""
    def accel(b, active):
        dim = (b.shape[1] - 1) // 2
        d = b[None, :, :dim] - b[active, None, :dim]
        rho2 = (d * d).sum(axis=2) + eps * eps
        w = b[None, :, -1] / (rho2 * rho2 if law == "soft" else rho2 * np.sqrt(rho2))
        w[np.arange(len(active)), active] = 0.0
        return (-G if law == "soft" else G) * (w[..., None] * d).sum(axis=1)
    return accel


def binary_block_control(c, **more):
    return dict(accel_length=c, dt_max=BIN_DT_MAX, levels=BIN_LEVELS, **more)


_runs = {}


def binary_block_run(nbx, extra, c):
    """The specification on the binary over one period, computed once per (extra, c)."""
    if (extra, c) not in _runs:
        _runs[(extra, c)] = nbx.blocksteps.block_leapfrog_spec(binary_system(extra), rows_accel_fn(BIN_G, BIN_EPS, "newton"), binary_block_control(c),
                                                               BIN_BLOCKS, 1 << 20)
    return _runs[(extra, c)]


# ---- the names -----------------------------------------------------------------------------------------------------------------------

def test_the_six_names_are_in_every_layer(nbx):
    header = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    script = open(os.path.join(ROOT, "nbody-simulation-parallel_amd", "csrc", "libnbody_hip.map")).read()
    patterns = [p.strip() for p in script.split("global:")[1].split("local:")[0].replace("\n", " ").split(";") if p.strip()]
    assert all(any(fnmatch.fnmatchcase(name, p) for p in patterns) for name in NAMES), patterns
    exported = subprocess.run(["nm", "-D", "--defined-only", nbx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    table = {row[0] for row in nbx.capi.ABI}
    lib = nbx.load_library()
    for name in NAMES:
        assert name in exported and name in table and getattr(lib, name) is not None, name
    for name in ("compute_accel_active", "forces_active", "step_kdk_block", "block_clock", "block_history", "block_levels"):
        assert callable(getattr(nbx.Context, name)), name
    assert lib.nbx_abi_version() == 5
    assert ctypes.sizeof(nbx.BlockControl) == 32 and ctypes.sizeof(nbx.BlockClock) == 48


# ---- refusals that need no device ----------------------------------------------------------------------------------------------------

def test_refusals_are_decided_before_a_device_is_needed(nbx):
    """On a machine without a GPU no context can exist, so every call here has a null context: the control and the counts are judged
    first (the detail text says which check refused), then the null handle."""
    lib = nbx.load_library()
    good = dict(accel_length=1.0e-3, dt_max=0.1, t_start=0.0, levels=4, reserved=0)

    def call(n_blocks=2, max_substeps=64, null_control=False, **change):
        k = nbx.BlockControl(**dict(good, **change))
        rc = lib.nbx_ctx_step_kdk_block(None, 1.0, None if null_control else ctypes.byref(k), n_blocks, max_substeps)
        return rc, lib.nbx_last_error_detail().decode()

    assert call() == (NBX_ERR_INVALID, "ctx is null")                            # a good control: the null handle is what is refused
    assert call(n_blocks=0) == (NBX_ERR_INVALID, "ctx is null") and call(max_substeps=0) == (NBX_ERR_INVALID, "ctx is null")
    assert call(levels=0)[1] == "ctx is null" and call(levels=20)[1] == "ctx is null" and call(t_start=-3.0)[1] == "ctx is null"
    assert call(null_control=True) == (NBX_ERR_INVALID, "null argument")
    bad = (dict(accel_length=0.0), dict(accel_length=-1.0), dict(accel_length=np.inf), dict(accel_length=np.nan),
           dict(dt_max=0.0), dict(dt_max=-0.1), dict(dt_max=np.inf), dict(dt_max=np.nan), dict(t_start=np.inf), dict(t_start=np.nan),
           dict(levels=-1), dict(levels=21), dict(reserved=1))
    for change in bad:
        rc, why = call(**change)
        assert rc == NBX_ERR_INVALID and why and why not in ("ctx is null", "null argument"), change
    rc, why = call(n_blocks=-1)
    assert rc == NBX_ERR_INVALID and "n_blocks" in why
    for max_substeps in (-1, (1 << 20) + 1):
        rc, why = call(max_substeps=max_substeps)
        assert rc == NBX_ERR_INVALID and "max_substeps" in why
    targets = (ctypes.c_uint32 * 2)(0, 1)
    out, clock, count = (ctypes.c_double * 6)(*([7.0] * 6)), nbx.BlockClock(), ctypes.c_size_t(7)
    assert lib.nbx_ctx_compute_accel_active(None, targets, 2) == NBX_ERR_INVALID and lib.nbx_ctx_compute_accel_active(None, None, 0) == NBX_ERR_INVALID
    assert lib.nbx_ctx_get_forces_active(None, 1.0, out) == NBX_ERR_INVALID and list(out) == [7.0] * 6
    assert lib.nbx_ctx_get_block_clock(None, ctypes.byref(clock)) == NBX_ERR_INVALID and lib.nbx_ctx_get_block_clock(None, None) == NBX_ERR_INVALID
    assert lib.nbx_ctx_get_block_history(None, None, None, 0, ctypes.byref(count)) == NBX_ERR_INVALID and count.value == 7
    levels = (ctypes.c_int32 * 2)(7, 7)
    assert lib.nbx_ctx_get_block_levels(None, levels) == NBX_ERR_INVALID and list(levels) == [7, 7]


def test_harness_refusals_at_the_command_line(nbx, tmp_path):
    sim = os.path.join(ROOT, "nbody_sim")
    base = [sim, "-N", "64", "-m", "g", "--steps", "4", "--integrator", "kdkb"]
    ok = ["--accel-length", "1", "--softening", "0.5"]
    for missing in ([], ["--accel-length", "1"], ["--softening", "0.5"], ok + ["--levels", "21"], ok + ["--levels", "-1"]):
        p = subprocess.run(base + missing, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "--accel-length" in p.stderr and "--softening" in p.stderr and "--levels" in p.stderr, p.stderr
    for where in (["--gpus", "2"], ["--devices", "0,0"]):
        p = subprocess.run(base + ok + where, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "--gpus" in p.stderr and "kdkb" in p.stderr, p.stderr
    for methods in ("a", "t", "gt"):
        p = subprocess.run([sim, "-N", "64", "-m", methods, "--steps", "4", "--integrator", "kdkb"] + ok, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "kdkb" in p.stderr
    p = subprocess.run([sim, "-N", "64", "-m", "g", "--steps", "4", "--integrator", "kdkc"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "kdkb" in p.stderr


# ---- the specification ---------------------------------------------------------------------------------------------------------------

def test_want_level_takes_the_first_halving_that_fits(nbx):
    want = nbx.blocksteps.want_level
    c, dt_max = 1.0e-2, 1.0
    assert want(0.0, c, dt_max, 5) == (0, np.inf)
    for j in range(6):
        a = c / (dt_max * 2.0 ** -j) ** 2                        # raw = dt_max 2^-j up to rounding: a little more or less acceleration decides
        assert want(a * (1 - 1e-9), c, dt_max, 5)[0] == j and want(a * (1 + 1e-9), c, dt_max, 5)[0] == min(j + 1, 5)
        assert want(a * (1 + 1e-9), c, dt_max, 5)[1] < 1e-8
    assert want(1.0e30, c, dt_max, 5)[0] == 5 and want(1.0e30, c, dt_max, 0)[0] == 0
    w, m = want(c / 0.3 ** 2, c, dt_max, 5)                      # raw = 0.3: between 0.5 and 0.25
    assert w == 2 and m == pytest.approx(0.3 / 0.25 - 1.0)


THREE_SEED = {3: 6, 2: 7}


def three_level_system(dim, n=600):
    """A random system with one heavy pair: the pair, its neighbourhood and the field populate different levels.  The pair's
    separation is 0.04 at coordinates of order 1: an fp32 position moves it by 1.5e-6 of itself, so what the device's fp32 sources do
    to an acceleration stays two orders below the 1e-4 margin asserted of every choice.  (A pair 0.004 apart is moved by 1.5e-5 and a
    choice flipped on the device; with noise of 1e-5 on the specification's accelerations it flips there too.)  The seeds are ones
    whose runs keep the margin, populate at least three levels and drift by more than one length."""
    rng = np.random.default_rng(THREE_SEED[dim])
    b = np.zeros((n, 2 * dim + 1))
    b[:, :dim] = rng.uniform(-1.0, 1.0, size=(n, dim))
    b[:, dim:2 * dim] = 0.05 * rng.normal(size=(n, dim))
    b[:, -1] = rng.uniform(0.5, 1.5, size=n) / n
    b[1, :dim] = b[0, :dim] + 0.04 * np.eye(dim)[0]
    b[0, -1] = b[1, -1] = 0.5
    return np.ascontiguousarray(b.astype(np.float32).astype(np.float64))


THREE_G, THREE_EPS = 1.0, 2.0e-3
THREE_CONTROL = dict(accel_length=2.0e-4, dt_max=1.0 / 64, levels=6)
THREE_BLOCKS = 1


@pytest.mark.parametrize("dim", (3, 2))
def test_ticks_are_a_multiple_of_every_present_step_and_all_are_active_at_the_end(nbx, dim):
    b0 = three_level_system(dim)
    L = THREE_CONTROL["levels"]
    seen = []

    def watched(b, active):
        seen.append(np.array(active))
        return rows_accel_fn(THREE_G, THREE_EPS, "newton")(b, active)

    # the invariant is checked from outside: replay the history's T against the levels after every evaluation
    b, clock, history, levels, margin = nbx.blocksteps.block_leapfrog_spec(b0, watched, THREE_CONTROL, THREE_BLOCKS, 1 << 20)
    assert clock["finished"] == 1 and clock["status"] == 0 and clock["ticks"] == THREE_BLOCKS << L and clock["t"] == THREE_BLOCKS * THREE_CONTROL["dt_max"]
    assert history[:, 1].sum() == THREE_BLOCKS << L and history[-1, 1] == 0 and (history[:-1, 1] > 0).all()
    assert len(seen) == len(history) == clock["evaluations"] == clock["substeps"] + 1
    assert seen[0].size == seen[-1].size == b0.shape[0]                      # all active at T = 0 and at T_end
    assert [s.size for s in seen] == list(history[:, 0]) and clock["pair_terms"] == int(history[:, 0].sum()) * b0.shape[0]
    assert all((np.diff(s) > 0).all() for s in seen)                          # ascending
    T = np.concatenate([[0], np.cumsum(history[:, 1])])[:-1]
    for t, dn in zip(T, history[:, 1]):
        assert dn == 0 or (t % dn == 0 and dn & (dn - 1) == 0)               # the drift is the smallest step present, aligned
    assert len(np.unique(history[:-1, 1])) >= 2 and clock["deepest_level"] >= 2
    assert len(np.unique(levels)) >= 3, np.unique(levels)                     # three populated levels at the end
    assert np.isfinite(b).all()


def test_a_body_is_evaluated_exactly_when_its_own_step_ends(nbx):
    """Replay: from the recorded actives and the rule's level changes, body i is active at T iff T is a multiple of its step."""
    b0 = three_level_system(3)
    L = THREE_CONTROL["levels"]
    accel = rows_accel_fn(THREE_G, THREE_EPS, "newton")
    log = []

    def watched(b, active):
        log.append(np.array(active))
        return accel(b, active)

    _, clock, history, levels, _ = nbx.blocksteps.block_leapfrog_spec(b0, watched, THREE_CONTROL, 1, 1 << 20)
    T, last = 0, np.zeros(b0.shape[0], dtype=np.int64)
    gaps = [set() for _ in range(b0.shape[0])]
    for active, dn in zip(log, history[:, 1]):
        for i in active:
            if T:
                gaps[i].add(T - last[i])
            last[i] = T
        T += int(dn)
    assert T == 1 << L and (last == T).all()
    assert all(g & (g - 1) == 0 and g <= 1 << L for s in gaps for g in s)    # every body's steps are powers of two ticks
    assert max(len(s) for s in gaps) >= 2                                      # some body changed its level


@pytest.mark.parametrize("dim", (3, 2))
def test_levels_zero_is_the_fixed_step_kick_drift_kick_bit_for_bit(nbx, dim):
    b0 = three_level_system(dim, n=40)
    accel = rows_accel_fn(THREE_G, THREE_EPS, "newton")
    dt, steps = 1.0 / 128, 5
    got, clock, history, levels, margin = nbx.blocksteps.block_leapfrog_spec(b0, accel, dict(accel_length=1.0, dt_max=dt, levels=0), steps, 1 << 20)
    want = nbx.leaves.leapfrog_spec(b0, lambda b: accel(b, np.arange(b.shape[0])), dt, steps, "kdk")
    assert np.array_equal(got, want)
    assert clock["substeps"] == steps and clock["evaluations"] == steps + 1 and clock["finished"] == 1 and (levels == 0).all()
    assert (history[:, 0] == 40).all() and list(history[:, 1]) == [1] * steps + [0]


def test_the_cap_and_a_sum_that_is_not_finite(nbx):
    b0 = three_level_system(3, n=40)
    accel = rows_accel_fn(THREE_G, THREE_EPS, "newton")
    full = nbx.blocksteps.block_leapfrog_spec(b0, accel, THREE_CONTROL, 1, 1 << 20)
    assert full[1]["substeps"] > 3
    b, clock, history, levels, _ = nbx.blocksteps.block_leapfrog_spec(b0, accel, THREE_CONTROL, 1, 3)
    assert clock["status"] == 2 and clock["finished"] == 0 and clock["substeps"] == 3 and clock["evaluations"] == 4
    assert np.array_equal(history[:3], full[2][:3]) and history[3, 1] == 0 and history[3, 0] == full[2][3, 0]
    b, clock, history, levels, _ = nbx.blocksteps.block_leapfrog_spec(b0, accel, THREE_CONTROL, 1, 0)
    assert clock["status"] == 2 and clock["substeps"] == 0 and np.array_equal(b[:, :3], b0[:, :3]) and not np.array_equal(b[:, 3:6], b0[:, 3:6])
    calls = []

    def poisoned(b, active):
        calls.append(1)
        a = accel(b, active)
        if len(calls) == 3:
            a[0, 0] = np.nan
        return a

    b, clock, history, levels, _ = nbx.blocksteps.block_leapfrog_spec(b0, poisoned, THREE_CONTROL, 1, 1 << 20)
    assert clock["status"] == 1 and clock["evaluations"] == 3 and clock["substeps"] == 2 and len(history) == 2 and np.isfinite(b).all()
    b, clock, history, levels, margin = nbx.blocksteps.block_leapfrog_spec(b0, accel, THREE_CONTROL, 0, 5)
    assert np.array_equal(b, b0) and clock["evaluations"] == 0 and len(history) == 0
    with pytest.raises(ValueError):
        nbx.blocksteps.block_leapfrog_spec(b0, accel, dict(THREE_CONTROL, levels=21), 1, 5)


@pytest.mark.parametrize("dim", (3, 2))
def test_three_level_system_keeps_the_margin(nbx, dim):
    """tests/test_gpu_block_steps.py compares the device's history with this run's: no choice may sit within 1e-4 of a threshold."""
    _, clock, history, levels, margin = nbx.blocksteps.block_leapfrog_spec(three_level_system(dim), rows_accel_fn(THREE_G, THREE_EPS, "newton"),
                                                                          THREE_CONTROL, THREE_BLOCKS, 1 << 20)
    print(f"three levels, D = {dim}: {clock['substeps']} substeps, margin {margin:.3e}, levels {np.bincount(levels)}")
    assert margin >= MARGIN


# ---- the certificate of the GPU test ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra", (0, BIN_EXTRA))
@pytest.mark.parametrize("c", BIN_C)
def test_eccentric_binary_certificate(nbx, c, extra):
    b0 = binary_system(extra)
    n = b0.shape[0]
    b, clock, history, levels, margin = binary_block_run(nbx, extra, c)
    assert clock["finished"] == 1 and clock["status"] == 0 and clock["t"] == BIN_PERIOD and clock["ticks"] == BIN_BLOCKS << BIN_LEVELS
    e0 = kinetic_plus_newton_potential(b0, BIN_G, BIN_EPS)
    block = abs(kinetic_plus_newton_potential(b, BIN_G, BIN_EPS) / e0 - 1.0)
    shared_rows, shared_clock, shared_history = nbx.leaves.adaptive_leapfrog_spec(
        b0, ctx_accel_fn(BIN_G, BIN_EPS, "newton"), dict(accel_length=c, dt_min=BIN_DT_MIN, dt_max=BIN_DT_MAX, pow2=True, t_end=BIN_PERIOD), 1 << 20)
    assert shared_clock["finished"] == 1
    shared = abs(kinetic_plus_newton_potential(shared_rows, BIN_G, BIN_EPS) / e0 - 1.0)
    shared_terms = len(shared_history) * n * n
    ratio = shared_terms / clock["pair_terms"]
    print(f"binary n = {n}, c = {c:g}: {clock['substeps']} substeps, margin {margin:.3e}, pair terms {clock['pair_terms']} against {shared_terms} "
          f"(ratio {ratio:.1f}), |E/E0 - 1| block {block:.3e}, shared pow2 {shared:.3e}")
    assert margin >= MARGIN
    assert block <= 2.0 * shared
    if extra:
        assert ratio >= 8.0
