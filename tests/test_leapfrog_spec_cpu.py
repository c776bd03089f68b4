"""CPU: leaves.leapfrog_spec, the fp64 specification of the plan's two step loops (kick-drift: nbx_leaf_plan_step; kick-drift-kick:
nbx_leaf_plan_step_kdk), and the four kick-drift-kick entry points' argument checks without a device.

The system (kdk_system) is chosen HERE, on the CPU, and tests/test_gpu_tree_kdk.py runs the same one through a plan: 48 bodies of
mass 1/48 in a ball of radius 1 with velocities of ~0.35 per component, G = 1 (a dynamical time ~1), softening 1/4; one time unit in
steps of dt = 1/8.  Positions, velocities and masses are fp32 values, and the softening length is a power of two, so the device's
inputs are the specification's.  Measured here against the specification at dt/64: the largest position error is 4.1e-3 (dt) and
1.0e-3 (dt/2) for kick-drift-kick, ratio 4.06; 5.5e-2 and 2.8e-2 for kick-drift, ratio 1.97 -- both in the asymptotic range, and
the kick-drift-kick error at dt/2 is four orders above what fp32 pair terms can add (the GPU test's margin)."""
import ctypes

import numpy as np

KDK_N, KDK_G, KDK_EPS, KDK_DT, KDK_STEPS = 48, 1.0, 0.25, 0.125, 8


def kdk_system():
    """Body<3> rows of the module docstring's system, every entry an fp32 value; centre of mass and total momentum (nearly) zero."""
    rng = np.random.default_rng(11)
    x = rng.normal(size=(KDK_N, 3))
    x *= np.cbrt(rng.uniform(0.2, 1.0, size=(KDK_N, 1))) / np.linalg.norm(x, axis=1, keepdims=True)
    v = 0.35 * rng.normal(size=(KDK_N, 3))
    x -= x.mean(axis=0)
    v -= v.mean(axis=0)
    b = np.hstack([x, v, np.full((KDK_N, 1), 1.0 / KDK_N)])
    return np.ascontiguousarray(b.astype(np.float32).astype(np.float64))


def all_pairs_accel(G, eps):
    """accel_fn of leapfrog_spec: the softened Newtonian sum over all pairs, a_i = G sum_j m_j d / (r^2 + eps^2)^(3/2), fp64."""
    def accel(b):
        dim = (b.shape[1] - 1) // 2
        d = b[None, :, :dim] - b[:, None, :dim]
        rho2 = (d * d).sum(axis=2) + eps * eps
        return G * ((b[None, :, -1] / (rho2 * np.sqrt(rho2)))[..., None] * d).sum(axis=1)
    return accel


def position_error(got, ref):
    return float(np.linalg.norm(got[:, :3] - ref[:, :3], axis=1).max())


def test_order_of_convergence(nbx):
    """Position error at dt and dt/2 against the specification at dt/64 (kick-drift-kick, whose own error there is 1/4096 of the one at
    dt): the ratio is 4 +- 10 % for kick-drift-kick and 2 +- 15 % for kick-drift."""
    b, accel, spec = kdk_system(), all_pairs_accel(KDK_G, KDK_EPS), nbx.leaves.leapfrog_spec
    ref = spec(b, accel, KDK_DT / 64, KDK_STEPS * 64, "kdk")
    ratio = {}
    for scheme in ("kdk", "kd"):
        e1 = position_error(spec(b, accel, KDK_DT, KDK_STEPS, scheme), ref)
        e2 = position_error(spec(b, accel, KDK_DT / 2, KDK_STEPS * 2, scheme), ref)
        ratio[scheme] = e1 / e2
        print(f"{scheme}: position error {e1:.3e} at dt = {KDK_DT}, {e2:.3e} at dt / 2, ratio {e1 / e2:.3f}")
    assert abs(ratio["kdk"] - 4.0) <= 0.4
    assert abs(ratio["kd"] - 2.0) <= 0.3
    assert np.array_equal(b, kdk_system()), "leapfrog_spec leaves its input alone"


def test_reversal(nbx):
    """n kick-drift-kick steps and n more with -dt return positions and velocities to 1e-12 relative; kick-drift ends at least 1e6
    times further away."""
    b, accel, spec = kdk_system(), all_pairs_accel(KDK_G, KDK_EPS), nbx.leaves.leapfrog_spec
    scale = np.abs(b[:, :6]).max()
    back = {}
    for scheme in ("kdk", "kd"):
        there = spec(b, accel, KDK_DT, KDK_STEPS, scheme)
        assert position_error(there, b) > 0.1
        again = spec(there, accel, -KDK_DT, KDK_STEPS, scheme)
        back[scheme] = float(np.abs(again[:, :6] - b[:, :6]).max()) / scale
        assert np.array_equal(again[:, -1], b[:, -1])
    print(f"return distance / scale: kdk {back['kdk']:.3e}, kd {back['kd']:.3e}")
    assert back["kdk"] <= 1e-12
    assert back["kd"] >= 1e6 * back["kdk"] and back["kd"] >= 1e-6


def test_merged_kicks_equal_the_textbook_form(nbx):
    """K(dt/2) D(dt) K(dt/2) per step, two evaluations' worth of half-kicks written out, against leapfrog_spec's merged form: the same
    to rounding (v + a dt/2 + a dt/2 against v + a dt)."""
    b, accel = kdk_system(), all_pairs_accel(KDK_G, KDK_EPS)
    t = b.copy()
    for _ in range(KDK_STEPS):
        t[:, 3:6] += accel(t) * (0.5 * KDK_DT)
        t[:, :3] += t[:, 3:6] * KDK_DT
        t[:, 3:6] += accel(t) * (0.5 * KDK_DT)
    got = nbx.leaves.leapfrog_spec(b, accel, KDK_DT, KDK_STEPS, "kdk")
    assert np.allclose(got, t, rtol=0.0, atol=1e-13 * np.abs(t[:, :6]).max())
    assert not np.array_equal(got[:, :6], b[:, :6])
    one = nbx.leaves.leapfrog_spec(b, accel, KDK_DT, 1, "kdk")       # a single step has nothing to merge: the textbook form's bits
    t = b.copy()
    t[:, 3:6] += accel(t) * (0.5 * KDK_DT)
    t[:, :3] += t[:, 3:6] * KDK_DT
    t[:, 3:6] += accel(t) * (0.5 * KDK_DT)
    assert np.array_equal(one, t)
    assert np.array_equal(nbx.leaves.leapfrog_spec(b, accel, KDK_DT, 0, "kdk"), b)
    for bad in (lambda: nbx.leaves.leapfrog_spec(b, accel, KDK_DT, 1, "dkd"), lambda: nbx.leaves.leapfrog_spec(b, accel, KDK_DT, -1, "kd")):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("leapfrog_spec must refuse an unknown scheme and a negative step count")


def test_kdk_entry_points_reject_null_arguments_without_a_device(nbx):
    """nbx_leaf_plan_kick_drift2, _step_kdk, _step_octree_kdk and _max_accel return NBX_ERR_INVALID for null arguments before they touch
    a device (the pattern of test_capi_cpu.py::test_new_entry_points_validate_and_fail_loudly_without_a_device)."""
    lib = nbx.load_library()
    a = ctypes.c_double(-1.0)
    calls = ((lib.nbx_leaf_plan_kick_drift2, (None, None, 1.0, 1.0)), (lib.nbx_leaf_plan_step_kdk, (None, None, 1, 1.0, 1.0, 1)),
             (lib.nbx_leaf_plan_step_octree_kdk, (None, None, 1, 1.0, 1.0, 1, 1)), (lib.nbx_leaf_plan_max_accel, (None, ctypes.byref(a))),
             (lib.nbx_leaf_plan_max_accel, (None, None)))
    for fn, args in calls:
        assert fn(*args) == 1, fn.__name__
        assert lib.nbx_last_error_detail()
    assert a.value == -1.0, "a refused call writes nothing"
    for name in ("kick_drift2", "step_kdk", "step_octree_kdk", "max_accel"):
        assert callable(getattr(nbx.LeafPlan, name))
