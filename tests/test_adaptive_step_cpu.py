"""CPU: leaves.choose_step and leaves.adaptive_leapfrog_spec, the fp64 specification of nbx_leaf_plan_step_kdk_adaptive (kick-drift-kick
through a leaf plan with every step chosen on the device), the certificate of the GPU energy test, and the three new entry points'
argument checks without a device.

The eccentric binary (binary_system) is chosen HERE and tests/test_gpu_adaptive_step.py runs the same one through a plan: masses 1 and
1, G = 1, semi-major axis 1, eccentricity 0.9, softening 1e-3, started at apocentre, dt_max = T / 8, one period T = 2 pi / sqrt(2).
Positions, velocities and masses are fp32 values, so the device's inputs are the specification's.  With 256 light (1e-12), distant
(~1e3) bodies at rest around it the system has n = 258 and the same orbit.

Measured with the specification, sampled after every step (chained one-step calls), worst |E / E0 - 1| over the period, adaptive
against fixed-step kick-drift-kick with the same number of steps (n = 2; n = 258 agrees to the digits shown):
    c = 4e-3     pow2 off:  71 steps 1.5e-01 against 6.7e+00 (43 x)     pow2 on: 104 steps 7.5e-02 against 3.3e+00 (43 x)
    c = 1e-3     pow2 off: 141 steps 3.8e-02 against 1.3e+00 (35 x)     pow2 on: 207 steps 1.6e-02 against 6.9e-01 (45 x)
    c = 2.5e-4   pow2 off: 281 steps 9.3e-03 against 6.4e-01 (69 x)     pow2 on: 416 steps 3.8e-03 against 4.9e-01 (130 x)
The factor 10 asserted below is the condition the issue sets, not one of these measurements."""
import ctypes

import numpy as np
import pytest

from test_leapfrog_spec_cpu import KDK_DT, KDK_EPS, KDK_G, KDK_STEPS, all_pairs_accel, kdk_system, position_error

BIN_G, BIN_EPS, BIN_ECC, BIN_EXTRA = 1.0, 1.0e-3, 0.9, 256
BIN_PERIOD = 2.0 * np.pi / np.sqrt(2.0)                            # a = 1, G (m1 + m2) = 2
BIN_DT_MAX = BIN_PERIOD / 8
BIN_DT_MIN = BIN_DT_MAX / 65536                                    # 2^-16: a power of two below dt_max, so pow2 can reach it exactly
BIN_C = (4.0e-3, 1.0e-3, 2.5e-4)
BIN_FACTOR = 10.0                                                  # adaptive must beat fixed steps by this much: the issue's condition


def binary_system(extra=0):
    """Body<3> rows: the binary at apocentre (separation 1.9 along x, relative speed sqrt(2 (2 / 1.9 - 1)) along y), then `extra` bodies
    of mass 1e-12 at rest on a shell of radius ~1e3.  Every entry is an fp32 value; no mass is 0."""
    r, v = 1.0 + BIN_ECC, np.sqrt(2.0 * (2.0 / (1.0 + BIN_ECC) - 1.0))
    rows = [[-r / 2, 0, 0, 0, -v / 2, 0, 1.0], [r / 2, 0, 0, 0, v / 2, 0, 1.0]]
    if extra:
        rng = np.random.default_rng(23)
        d = rng.normal(size=(extra, 3))
        d *= rng.uniform(900.0, 1100.0, size=(extra, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
        rows += [[*p, 0, 0, 0, 1.0e-12] for p in d]
    return np.ascontiguousarray(np.array(rows, dtype=np.float64).astype(np.float32).astype(np.float64))


def binary_control(c, pow2, **more):
    return dict(accel_length=c, dt_min=BIN_DT_MIN, dt_max=BIN_DT_MAX, pow2=pow2, **more)


def pair_functions(G, eps):
    """(accel_fn, energy_fn) of Body<3> rows under the softened Newtonian law, fp64: all_pairs_accel's sum and K + U with every pair
    once.  Both come from one distance matrix, kept for the positions last seen: the closing evaluation of a chained call, the energy
    at its end and the opening evaluation of the next call all see the same positions."""
    seen = {}

    def pairs(b):
        key = b[:, :3].tobytes()
        if seen.get("key") != key:
            d = b[None, :, :3] - b[:, None, :3]
            rho2 = (d * d).sum(axis=2) + eps * eps
            m = b[:, -1]
            seen["key"] = key
            seen["accel"] = G * ((m[None, :] / (rho2 * np.sqrt(rho2)))[..., None] * d).sum(axis=1)
            seen["potential"] = -G * float((m[:, None] * m[None, :] / np.sqrt(rho2))[np.triu_indices(b.shape[0], 1)].sum())
        return seen

    def energy(b):
        return float(0.5 * (b[:, -1] * (b[:, 3:6] ** 2).sum(axis=1)).sum()) + pairs(b)["potential"]

    return (lambda b: pairs(b)["accel"]), energy


def worst_energy_errors(nbx, b0, c, pow2):
    """(steps, worst |E/E0 - 1| adaptive, the same for fixed steps of T / steps): one period in chained one-step calls, the energy
    taken at every synchronised end"""
    accel, energy = pair_functions(BIN_G, BIN_EPS)
    e0 = energy(b0)
    b, t, steps, worst = b0, 0.0, 0, 0.0
    while True:
        b, clock, _ = nbx.leaves.adaptive_leapfrog_spec(b, accel, binary_control(c, pow2, t_start=t, t_end=BIN_PERIOD), 1)
        steps += clock["steps"]
        t = clock["t"]
        worst = max(worst, abs(energy(b) / e0 - 1.0))
        if clock["finished"]:
            break
        assert steps < 100000
    assert t == BIN_PERIOD
    f, fixed = b0, 0.0
    for _ in range(steps):
        f = nbx.leaves.leapfrog_spec(f, accel, BIN_PERIOD / steps, 1, "kdk")
        fixed = max(fixed, abs(energy(f) / e0 - 1.0))
    return steps, worst, fixed


# ---- choose -----------------------------------------------------------------------------------------------------------------------

def test_choose_honours_both_clamps(nbx):
    choose = nbx.leaves.choose_step
    assert choose(0.0, 1.0, 0.25, 2.0) == 2.0 and choose(0.0, 1.0, 0.25, 2.0, True) == 2.0       # a_max = 0: raw = +inf
    assert choose(1.0e-30, 1.0, 0.25, 2.0) == 2.0                                                # raw above dt_max
    assert choose(1.0e30, 1.0, 0.25, 2.0) == 0.25 and choose(1.0e30, 1.0, 0.25, 2.0, True) == 0.25
    assert choose(4.0, 1.0, 0.25, 2.0) == 0.5 and choose(1.0, 2.25, 0.25, 2.0) == 1.5            # in between: sqrt(c / a_max)
    assert choose(1.0, 1.0, 0.3, 0.3) == 0.3 and choose(1.0, 1.0, 0.3, 0.3, True) == 0.3         # equal clamps


def test_choose_pow2_takes_the_first_halving_that_fits(nbx):
    """dt_max 2^-j with the smallest j for which dt <= raw, or the last one whose dt is not below dt_min"""
    choose = nbx.leaves.choose_step
    rng = np.random.default_rng(3)
    dt_max, dt_min = 0.75, 0.75 / 40.0                                # dt_min is no halving of dt_max: the smallest dt is dt_max / 32
    for a_max in np.concatenate([10.0 ** rng.uniform(-4, 6, size=400), [1.0 / 0.75 ** 2, 4.0 / 0.75 ** 2]]):
        raw = np.sqrt(1.0 / a_max)
        d = choose(a_max, 1.0, dt_min, dt_max, True)
        j = np.log2(dt_max / d)
        assert j == int(j) and d == dt_max / 2 ** int(j) and d >= dt_min
        j = int(j)
        assert d <= raw or 0.5 * d < dt_min                          # it fits, or it cannot be halved again
        assert j == 0 or 2.0 * d > raw                                # the halving before it did not fit
    assert choose(1.0 / 0.75 ** 2, 1.0, dt_min, dt_max, True) == 0.75   # d == raw is not halved


# ---- landing ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pow2", (False, True))
def test_landing_on_t_end(nbx, pow2):
    b, accel = kdk_system(), all_pairs_accel(KDK_G, KDK_EPS)
    t_start, t_end, dt_min = 0.1, 1.0, 0.05
    control = dict(accel_length=0.01, dt_min=dt_min, dt_max=0.25, t_start=t_start, t_end=t_end, pow2=pow2)
    rows, clock, hist = nbx.leaves.adaptive_leapfrog_spec(b, accel, control, 1000)
    assert clock["t"] == t_end and clock["finished"] == 1 and clock["status"] == 0
    assert clock["steps"] == hist.shape[0] - 1 < 1000 and clock["evaluations"] == hist.shape[0]
    dts = hist[:-1, 1]
    assert hist[-1, 1] == 0.0 and (dts[:-1] >= dt_min).all() and (dts <= 0.25).all() and dts[-1] > 0
    assert abs(dts.sum() - (t_end - t_start)) <= 4 * dts.size * np.spacing(t_end)
    assert not np.array_equal(rows[:, :6], b[:, :6]) and np.array_equal(b, kdk_system())
    # the same call capped at the steps taken ends in the same state, not finished by the clock's reckoning only if t fell short
    again, clock2, hist2 = nbx.leaves.adaptive_leapfrog_spec(b, accel, control, clock["steps"])
    assert np.array_equal(again, rows) and np.array_equal(hist2, hist) and clock2 == clock
    # t_start at or past t_end: one evaluation, no step, no kick
    rows0, clock0, hist0 = nbx.leaves.adaptive_leapfrog_spec(b, accel, dict(control, t_start=1.0), 5)
    assert np.array_equal(rows0, b) and clock0["steps"] == 0 and clock0["finished"] == 1 and hist0.shape == (1, 2)
    rows0, clock0, hist0 = nbx.leaves.adaptive_leapfrog_spec(b, accel, control, 0)
    assert np.array_equal(rows0, b) and clock0["evaluations"] == 0 and hist0.shape == (0, 2)


def test_equal_clamps_are_the_fixed_step_loop(nbx):
    """dt_min == dt_max == dt and t_end = inf: leapfrog_spec(..., "kdk") bit for bit, because 0.5 dt + 0.5 dt == dt"""
    b, accel = kdk_system(), all_pairs_accel(KDK_G, KDK_EPS)
    for pow2 in (False, True):
        rows, clock, hist = nbx.leaves.adaptive_leapfrog_spec(b, accel, dict(accel_length=3.0, dt_min=KDK_DT, dt_max=KDK_DT, pow2=pow2), KDK_STEPS)
        assert np.array_equal(rows, nbx.leaves.leapfrog_spec(b, accel, KDK_DT, KDK_STEPS, "kdk"))
        assert clock["steps"] == KDK_STEPS and clock["finished"] == 0 and clock["t"] == KDK_STEPS * KDK_DT
        assert (hist[:-1, 1] == KDK_DT).all() and hist[-1, 1] == 0.0


def test_an_acceleration_that_is_not_finite_stops_the_loop(nbx):
    b, accel = kdk_system(), all_pairs_accel(KDK_G, KDK_EPS)
    bad = b.copy()
    bad[5, 0] = np.nan
    rows, clock, hist = nbx.leaves.adaptive_leapfrog_spec(bad, accel, dict(accel_length=0.01, dt_min=0.01, dt_max=0.25), 4)
    assert clock["status"] == 1 and clock["steps"] == 0 and clock["evaluations"] == 1 and hist.shape == (0, 2)
    assert np.array_equal(rows, bad, equal_nan=True)
    # bodies in no leaf count 0 towards a_max and are not kicked
    mask = np.ones(b.shape[0], dtype=bool)
    mask[5] = False
    rows, clock, hist = nbx.leaves.adaptive_leapfrog_spec(b, accel, dict(accel_length=0.01, dt_min=0.01, dt_max=0.25), 2, in_leaf=mask)
    assert clock["status"] == 0 and np.array_equal(rows[5, 3:6], b[5, 3:6]) and not np.array_equal(rows[5, :3], b[5, :3])


# ---- the certificate of the GPU energy test ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra", (0, BIN_EXTRA))
@pytest.mark.parametrize("pow2", (False, True))
@pytest.mark.parametrize("c", BIN_C)
def test_eccentric_binary_certificate(nbx, c, pow2, extra):
    """One period of the module docstring's binary: the adaptive loop's worst synchronised energy error is at least 10 x below
    fixed-step kick-drift-kick's with the same number of steps."""
    b0 = binary_system(extra)
    assert (b0[:, -1] > 0).all()
    steps, worst, fixed = worst_energy_errors(nbx, b0, c, pow2)
    print(f"binary n = {b0.shape[0]}, c = {c:g}, pow2 = {pow2}: {steps} steps, worst |E/E0 - 1| adaptive {worst:.3e}, fixed {fixed:.3e}, ratio {fixed / worst:.1f}")
    assert BIN_FACTOR * worst <= fixed


def test_the_binary_uses_many_different_steps(nbx):
    _, clock, hist = nbx.leaves.adaptive_leapfrog_spec(binary_system(), all_pairs_accel(BIN_G, BIN_EPS), binary_control(1.0e-3, False, t_end=BIN_PERIOD), 100000)
    dts = hist[:-1, 1]
    assert clock["finished"] == 1 and dts.max() / dts.min() > 10.0 and dts.min() > BIN_DT_MIN and dts.max() < BIN_DT_MAX


# ---- second order -----------------------------------------------------------------------------------------------------------------

CONV_C, CONV_T_END, CONV_DT_MIN, CONV_DT_MAX = 0.02, 1.0, 1.0e-4, 0.5


def convergence_control(c, **more):
    return dict(accel_length=c, dt_min=CONV_DT_MIN, dt_max=CONV_DT_MAX, t_end=CONV_T_END, **more)


def test_second_order_convergence(nbx):
    """kdk_system to t = 1 with steps sqrt(c / a_max), no clamp active: dt goes as sqrt(c), so a second-order scheme's position error
    goes as c.  Against the specification at c / 4096 the error ratio from c to c / 4 and from c / 4 to c / 16 is 4 within 15 %: the
    specification itself showed 4.25 and 4.10 (errors 6.1e-3, 1.4e-3, 3.5e-4 with 8, 15 and 29 steps)."""
    b, accel = kdk_system(), all_pairs_accel(KDK_G, KDK_EPS)
    ref, clock, _ = nbx.leaves.adaptive_leapfrog_spec(b, accel, convergence_control(CONV_C / 4096), 100000)
    assert clock["finished"] == 1
    err = []
    for c in (CONV_C, CONV_C / 4, CONV_C / 16):
        rows, clock, hist = nbx.leaves.adaptive_leapfrog_spec(b, accel, convergence_control(c), 100000)
        dts = hist[:-2, 1]                                          # all but the landing step
        assert clock["finished"] == 1 and dts.min() > CONV_DT_MIN and dts.max() < CONV_DT_MAX and np.unique(dts).size > 3
        err.append(position_error(rows, ref))
        print(f"c = {c:g}: {clock['steps']} steps, position error {err[-1]:.3e}")
    print(f"ratios {err[0] / err[1]:.3f}, {err[1] / err[2]:.3f}")
    assert abs(err[0] / err[1] - 4.0) <= 0.6 and abs(err[1] / err[2] - 4.0) <= 0.6


# ---- the entry points without a device --------------------------------------------------------------------------------------------

def test_adaptive_entry_points_reject_bad_arguments_without_a_device(nbx):
    """Null arguments and every control field outside its range are NBX_ERR_INVALID before a device is touched.  The control is judged
    before the handles, so with null handles the detail text says which check refused."""
    lib = nbx.load_library()
    good = dict(accel_length=1.0e-3, dt_min=0.01, dt_max=0.1, t_start=0.0, t_end=np.inf, pow2=0, reserved=0)

    def call(law=1, max_steps=4, rebuild_every=0, null_control=False, **change):
        k = nbx.StepControl(**dict(good, **change))
        rc = lib.nbx_leaf_plan_step_kdk_adaptive(None, None, law, 1.0, None if null_control else ctypes.byref(k), max_steps, rebuild_every)
        return rc, lib.nbx_last_error_detail().decode()

    assert call() == (1, "null argument")                                        # a good control: the null handles are what is refused
    assert call(null_control=True)[0] == 1
    assert call(t_end=2.0)[1] == "null argument" and call(t_start=5.0, t_end=2.0)[1] == "null argument" and call(pow2=1)[1] == "null argument"
    bad = (dict(accel_length=0.0), dict(accel_length=-1.0), dict(accel_length=np.inf), dict(accel_length=np.nan),
           dict(dt_min=0.0), dict(dt_min=-0.01), dict(dt_min=np.nan), dict(dt_min=0.2), dict(dt_max=np.inf), dict(dt_max=np.nan), dict(dt_min=np.inf, dt_max=np.inf),
           dict(t_start=np.inf), dict(t_start=np.nan), dict(t_end=np.nan), dict(t_end=-np.inf), dict(pow2=2), dict(pow2=-1), dict(reserved=1))
    for change in bad:
        rc, why = call(**change)
        assert rc == 1 and why != "null argument" and why, change
    for kw in (dict(law=-1), dict(law=4), dict(max_steps=-1), dict(max_steps=(1 << 20) + 1), dict(rebuild_every=-1)):
        rc, why = call(**kw)
        assert rc == 1 and why != "null argument", kw
    clock, count = nbx.StepClock(), ctypes.c_size_t(7)
    assert lib.nbx_leaf_plan_get_step_clock(None, ctypes.byref(clock)) == 1 and lib.nbx_leaf_plan_get_step_clock(None, None) == 1
    assert lib.nbx_leaf_plan_get_step_history(None, None, None, 0, ctypes.byref(count)) == 1 and count.value == 7
    assert ctypes.sizeof(nbx.StepControl) == 48 and ctypes.sizeof(nbx.StepClock) == 40
    for name in ("step_kdk_adaptive", "step_clock", "step_history"):
        assert callable(getattr(nbx.LeafPlan, name))
