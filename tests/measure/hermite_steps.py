"""Accelerations with jerks on a list of targets and the fourth-order Hermite loop, measured (profiles/r20/hermite_block.txt).
    python tests/measure/hermite_steps.py deviation
    python tests/measure/hermite_steps.py jerk      [--n N] [--long-list T]
    python tests/measure/hermite_steps.py threshold [--n N]
    python tests/measure/hermite_steps.py substep   [--n N]
    python tests/measure/hermite_steps.py binary    [--n N] [--eta E] [--c C]
    python tests/measure/hermite_steps.py parent    [--repo DIR] [--n N]
`deviation`: what tests/test_gpu_hermite_steps.py's tolerance is made of -- nbx_ctx_step_kdk_block(levels = 0) on the 600 generated
bodies of its levels = 0 case against blocksteps.block_leapfrog_spec fed the same sums of fp32-rounded positions: max over bodies and
components of |device - specification|, positions and velocities, per (dim, law); next to it nbx_ctx_step_hermite_block's own
deviation from hermite.hermite_block_spec where this library has it (a build of the parent commit, --repo DIR, prints the first
only).  `jerk`: ms of one evaluation of n_active listed targets (random, distinct) with the jerk next to nbx_ctx_compute_accel_active
on the same context, softened Newtonian law, uniform bodies with velocities; five warm runs each, the best printed (the upload of
the list is included in both).  `threshold`: list lengths around the long-list threshold under each build of the jerk kernel.
`substep`: ms per substep of the Hermite loop on the eccentric binary among N - 2 field bodies (the field never becomes active between
the ends: the bookkeeping and a two-target evaluation).  `binary`: wall time, pair terms and energy error of that system over one
period, Hermite (--eta) against kick-drift-kick block steps (--c).  `parent`: nbx_ctx_step, _step_kdk, _step_kdk_adaptive and
_step_kdk_block for alternating processes of this commit and a build of the parent commit (--repo DIR)."""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("deviation", "jerk", "threshold", "substep", "binary", "parent"))
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--eta", type=float, default=0.02)
ap.add_argument("--c", type=float, default=2.5e-4)
ap.add_argument("--long-list", default="")
ap.add_argument("--repo", default="")
a = ap.parse_args()
here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, a.repo or here)
sys.path.insert(0, os.path.join(here, "tests"))
import numpy as np, nbody_amd as nbx
fmt = lambda ts: " ".join("%.3f" % t for t in ts)


def wall(c, f):
    c.synchronize(); t0 = time.perf_counter(); f(); c.synchronize(); return (time.perf_counter() - t0) * 1e3


def uniform(n, seed=77):
    b = nbx.generate.uniform_bodies(n, 3, seed)
    rng = np.random.default_rng(seed)
    b[:, 3:6] = rng.normal(size=(n, 3))
    return np.ascontiguousarray(b.astype(np.float32).astype(np.float64))


def newton_context(b, eps, long_list=None):
    if long_list is None or long_list == "":
        os.environ.pop("NBODY_HIP_ACTIVE_LONG_LIST", None)
    else:
        os.environ["NBODY_HIP_ACTIVE_LONG_LIST"] = str(long_list)
    c = nbx.Context(b.shape[0], 3)
    c.upload(b); c.set_softening(eps); c.set_law(nbx.FORCE_LAW_NEWTON); c.synchronize()
    return c


def field_binary(n_field, seed=23):
    """tests/test_adaptive_step_cpu.py's binary among n_field light bodies at rest on its shell"""
    from test_adaptive_step_cpu import BIN_ECC
    r, v = 1.0 + BIN_ECC, np.sqrt(2.0 * (2.0 / (1.0 + BIN_ECC) - 1.0))
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_field, 3))
    d *= rng.uniform(900.0, 1100.0, size=(n_field, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    rows = np.zeros((n_field + 2, 7))
    rows[0] = [-r / 2, 0, 0, 0, -v / 2, 0, 1.0]
    rows[1] = [r / 2, 0, 0, 0, v / 2, 0, 1.0]
    rows[2:, :3], rows[2:, 6] = d, 1.0e-12
    return np.ascontiguousarray(rows.astype(np.float32).astype(np.float64))


if a.mode == "deviation":
    from oracle_lib import Oracle
    from test_block_steps_cpu import rows_accel_fn
    oracle = Oracle()
    n, steps, dt = 600, 5, 2.0
    for dim in (3, 2):
        for law in ("soft", "newton"):
            eps, gs = (50.0, 1e24) if law == "soft" else (2.0e4, 1e22)
            G = oracle.G * gs
            b0 = oracle.round_inputs_to_f32(oracle.generate(35 + dim, n, dim))
            accel = rows_accel_fn(G, eps, law)
            ref = nbx.blocksteps.block_leapfrog_spec(b0, lambda b, act: accel(b.astype(np.float32).astype(np.float64), act),
                                                     dict(accel_length=1.0, dt_max=dt, levels=0), steps, 1 << 20)[0]
            line = []
            for kind in ("kdk", "hermite"):
                if kind == "hermite" and not hasattr(nbx.Context, "step_hermite_block"):
                    continue
                with nbx.Context(n, dim) as c:
                    c.upload(b0); c.set_softening(eps)
                    if law == "newton":
                        c.set_law(nbx.FORCE_LAW_NEWTON)
                    if kind == "kdk":
                        c.step_kdk_block(1.0, dt, 0, steps, G=G)
                        want = ref
                    else:
                        c.step_hermite_block(0.02, dt, 0, steps, G=G)
                        fn = lambda rows, act: nbx.hermite.accel_jerk_rows(rows.astype(np.float32).astype(np.float64), act, G, eps, law)
                        want = nbx.hermite.hermite_block_spec(b0, fn, dict(eta=0.02, dt_max=dt, levels=0), steps, 1 << 20)[0]
                    got = b0.copy(); c.download(got)
                line.append("%s (%.3e, %.3e)" % (kind, np.abs(got[:, :dim] - want[:, :dim]).max(), np.abs(got[:, dim:2 * dim] - want[:, dim:2 * dim]).max()))
            dx, dv = np.abs(ref[:, :dim] - b0[:, :dim]).max(), np.abs(ref[:, dim:2 * dim] - b0[:, dim:2 * dim]).max()
            print("(%d, %r): " % (dim, law) + ", ".join(line) + "   # the run moves x by up to %.3e, v by up to %.3e" % (dx, dv), flush=True)
    sys.exit(0)

n = a.n
eps = 2048.0

if a.mode in ("jerk", "threshold"):
    b = uniform(n)
    rng = np.random.default_rng(3)
    if a.mode == "jerk":
        lengths = [m for m in (1, 64, 4096, 65536) if m < n] + [n]
        builds = [a.long_list or None]
    else:
        lengths = [m for m in (256, 512, 1024, 2048, 4096, 8192, 16384, 32768) if m <= n]
        builds = [str(1 << 31), "1"]
    for build in builds:
        with newton_context(b, eps, long_list=build) as c:
            row = []
            for m in lengths:
                t = rng.permutation(n)[:m].astype(np.uint32)
                c.compute_accel_jerk_active(t); c.compute_accel_active(t)
                jerk = min(wall(c, lambda: c.compute_accel_jerk_active(t)) for _ in range(5))
                plain = min(wall(c, lambda: c.compute_accel_active(t)) for _ in range(5))
                row.append("%d: %.3f (%.3f)" % (m, jerk, plain))
            print("N %d, long-list threshold %s: ms with the jerk (nbx_ctx_compute_accel_active), upload included | " % (n, build or "default") + " | ".join(row), flush=True)
    sys.exit(0)

if a.mode == "substep":
    from test_adaptive_step_cpu import BIN_DT_MAX, BIN_EPS, BIN_G
    fb = field_binary(n - 2)
    with newton_context(fb, BIN_EPS) as c:
        for name, run in (("Hermite eta %g" % a.eta, lambda: c.step_hermite_block(a.eta, BIN_DT_MAX, 16, 1, G=BIN_G)),
                          ("kick-drift-kick c %g" % a.c, lambda: c.step_kdk_block(a.c, BIN_DT_MAX, 16, 1, G=BIN_G))):
            c.upload(fb); run()
            ts, subs = [], 0
            for _ in range(3):
                c.upload(fb)
                ts.append(wall(c, run))
                subs = c.block_clock().substeps
            print("N %d binary, one block of dt_max, %s: %d substeps, ms per call %s -> ms per substep %s" % (n, name, subs, fmt(ts), fmt([t / max(subs, 1) for t in ts])), flush=True)
    sys.exit(0)

if a.mode == "binary":
    from test_adaptive_step_cpu import BIN_DT_MAX, BIN_EPS, BIN_G
    fb = field_binary(n - 2)
    for name, run in (("Hermite, eta = %g" % a.eta, lambda c: c.step_hermite_block(a.eta, BIN_DT_MAX, 16, 8, G=BIN_G)),
                      ("kick-drift-kick block steps, c = %g" % a.c, lambda c: c.step_kdk_block(a.c, BIN_DT_MAX, 16, 8, G=BIN_G))):
        with newton_context(fb, BIN_EPS) as c:
            e0 = sum(c.energy(BIN_G))
            t = wall(c, lambda: run(c))
            k = c.block_clock()
            e = abs(sum(c.energy(BIN_G)) / e0 - 1.0)
        print("N %d binary, one period, %s: %.1f ms, %d substeps, pair terms %d, deepest level %d, finished %d, |E/E0 - 1| %.3e" % (
            n, name, t, k.substeps, k.pair_terms, k.deepest_level, k.finished, e), flush=True)
    sys.exit(0)

if a.mode == "parent":
    b = uniform(n)
    K = 200 if n <= 4096 else 50 if n <= 65536 else 3
    G, dt = nbx.REFERENCE_G, 1.0
    name = os.path.basename(os.path.abspath(a.repo or here))
    os.environ.pop("NBODY_HIP_STEP_WINDOW", None)
    with nbx.Context(n, 3) as c:
        c.upload(b); c.synchronize()
        c.step(dt, 5, G)
        kd = min(wall(c, lambda: c.step(dt, K, G)) / K for _ in range(2))
        kdk = min(wall(c, lambda: c.step_kdk(dt, K, G)) / K for _ in range(2))
        ada = min(wall(c, lambda: c.step_kdk_adaptive(1.0, dt, dt, max_steps=K, G=G)) / K for _ in range(2))
    with newton_context(b, eps) as c:
        c.step_kdk_block(1.0, dt, 0, 2, G=G)
        blk = min(wall(c, lambda: c.step_kdk_block(1.0, dt, 0, K, G=G)) / K for _ in range(2))
    print("N %d (%s), ms per step: ctx.step %.4f | ctx.step_kdk %.4f | ctx.step_kdk_adaptive %.4f | ctx.step_kdk_block(levels = 0) %.4f" % (n, name, kd, kdk, ada, blk), flush=True)
