"""Forces on a list of targets and kick-drift-kick with block time steps, measured (profiles/r19/block_steps.txt).
    python tests/measure/block_steps.py deviation
    python tests/measure/block_steps.py active    [--n N] [--long-list T]
    python tests/measure/block_steps.py threshold [--n N]
    python tests/measure/block_steps.py window    [--n N]
    python tests/measure/block_steps.py substep   [--n N]
    python tests/measure/block_steps.py binary    [--n N] [--c C] [--block-only]
    python tests/measure/block_steps.py parent    [--repo DIR] [--n N]
`deviation`: what tests/test_gpu_block_steps.py's tolerance is made of -- nbx_ctx_step_kdk_adaptive (pow2) on the eccentric binary
over one period against leaves.adaptive_leapfrog_spec fed the same sums of fp32-rounded positions: max over bodies and components of
|device - specification|, positions and velocities, per (extra bodies, c).  `active`: ms of one evaluation of n_active listed targets
(random, distinct) next to nbx_ctx_compute_accel on the same context, softened Newtonian law, uniform bodies; five warm runs each,
the best printed.  `threshold`: the same list lengths around the long-list threshold under each build.  `window`: a block-step call
whose stop comes early (n_blocks = 1, levels = 0), per NBODY_HIP_STEP_WINDOW.  `substep`: ms per substep with an empty force
evaluation's worth of bookkeeping -- levels = 0 against nbx_ctx_step_kdk, whose difference at large N is the bookkeeping plus the list
kernels' distance from K1.  `binary`: wall time of the eccentric binary among N field bodies over one period, block steps against
nbx_ctx_step_kdk_adaptive (pow2).  `parent`: nbx_ctx_step, _step_kdk and _step_kdk_adaptive for alternating processes of this commit
and a build of the parent commit (--repo DIR)."""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("deviation", "active", "threshold", "window", "substep", "binary", "parent"))
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--c", type=float, default=2.5e-4)
ap.add_argument("--long-list", default="")
ap.add_argument("--repo", default="")
ap.add_argument("--block-only", action="store_true")
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
    b[:, :3] = b[:, :3].astype(np.float32)
    return np.ascontiguousarray(b)


def newton_context(b, eps, long_list=None, window=None):
    for name, v in (("NBODY_HIP_ACTIVE_LONG_LIST", long_list), ("NBODY_HIP_STEP_WINDOW", window)):
        if v is None or v == "":
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)
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
    from test_adaptive_step_cpu import BIN_C, BIN_DT_MAX, BIN_DT_MIN, BIN_EPS, BIN_EXTRA, BIN_G, BIN_PERIOD, binary_system
    from test_ctx_adaptive_step_cpu import ctx_accel_fn
    accel = ctx_accel_fn(BIN_G, BIN_EPS, "newton")
    for extra in (0, BIN_EXTRA):
        for c_len in BIN_C:
            b0 = binary_system(extra)
            ref, clock, hist = nbx.leaves.adaptive_leapfrog_spec(b0, lambda b: accel(b.astype(np.float32).astype(np.float64)),
                                                                 dict(accel_length=c_len, dt_min=BIN_DT_MIN, dt_max=BIN_DT_MAX, pow2=True, t_end=BIN_PERIOD), 1 << 20)
            with newton_context(b0, BIN_EPS) as c:
                k = c.step_kdk_adaptive(c_len, BIN_DT_MIN, BIN_DT_MAX, t_end=BIN_PERIOD, pow2=True, G=BIN_G)
                got = b0.copy(); c.download(got)
                same = np.array_equal(c.step_history()[1], hist[:, 1])
            print("(%d, %g): (%.3e, %.3e),   # %d steps, device %d, same steps: %s" % (extra, c_len, np.abs(got[:, :3] - ref[:, :3]).max(),
                  np.abs(got[:, 3:6] - ref[:, 3:6]).max(), clock["steps"], k.steps, same), flush=True)
    sys.exit(0)

n = a.n
eps = 2048.0

if a.mode in ("active", "threshold"):
    b = uniform(n)
    rng = np.random.default_rng(3)
    if a.mode == "active":
        lengths = [m for m in (1, 64, 4096, 65536) if m < n] + [n]
        builds = [a.long_list or None]
    else:
        lengths = [m for m in (256, 512, 1024, 2048, 4096, 8192, 16384, 32768) if m <= n]
        builds = [str(1 << 31), "1"]
    for build in builds:
        with newton_context(b, eps, long_list=build) as c:
            c.compute_accel(); full = min(wall(c, c.compute_accel) for _ in range(5))
            row = []
            for m in lengths:
                t = rng.permutation(n)[:m].astype(np.uint32)
                c.compute_accel_active(t)
                best = min(wall(c, lambda: c.compute_accel_active(t)) for _ in range(5))
                row.append("%d: %.3f" % (m, best))
            print("N %d, long-list threshold %s: nbx_ctx_compute_accel %.3f ms | active (upload included) ms " % (n, build or "default", full) + " | ".join(row), flush=True)
    sys.exit(0)

if a.mode == "window":
    b = uniform(n)
    for w in (1, 2, 4, 8, 16, 64):
        with newton_context(b, eps, window=w) as c:
            run = lambda: c.step_kdk_block(1.0, 1.0, 0, 4, max_substeps=64, G=nbx.REFERENCE_G)
            run()
            ts = [wall(c, run) for _ in range(5)]
        print("N %d, 4 substeps then the stop (max_substeps 64), W = %d: ms per call %s" % (n, w, fmt(ts)), flush=True)
    sys.exit(0)

if a.mode == "substep":
    b = uniform(n)
    K = 20 if n <= 65536 else 3
    with newton_context(b, eps) as c, newton_context(b, eps) as f:
        c.step_kdk_block(1.0, 1.0, 0, 2, G=nbx.REFERENCE_G); f.step_kdk(1.0, 2, nbx.REFERENCE_G)
        blk = [wall(c, lambda: c.step_kdk_block(1.0, 1.0, 0, K, G=nbx.REFERENCE_G)) / (K + 1) for _ in range(5)]
        kdk = [wall(f, lambda: f.step_kdk(1.0, K, nbx.REFERENCE_G)) / (K + 1) for _ in range(5)]
    print("N %d, %d steps a run, ms per evaluation: step_kdk_block(levels = 0) %s | step_kdk %s" % (n, K, fmt(blk), fmt(kdk)), flush=True)
    # the bookkeeping alone: a system whose field never becomes active between the ends -- two heavy bodies, levels deep
    fb = field_binary(n - 2)
    from test_adaptive_step_cpu import BIN_DT_MAX, BIN_EPS, BIN_G
    with newton_context(fb, BIN_EPS) as c:
        c.step_kdk_block(a.c, BIN_DT_MAX, 16, 1, G=BIN_G)
        ts, subs = [], 0
        for _ in range(3):
            ts.append(wall(c, lambda: c.step_kdk_block(a.c, BIN_DT_MAX, 16, 1, G=BIN_G)))
            subs = c.block_clock().substeps
    print("N %d binary, one block of dt_max, c = %g: %d substeps, ms per call %s -> ms per substep %s" % (n, a.c, subs, fmt(ts), fmt([t / max(subs, 1) for t in ts])), flush=True)
    sys.exit(0)

if a.mode == "binary":
    from test_adaptive_step_cpu import BIN_DT_MAX, BIN_DT_MIN, BIN_EPS, BIN_G, BIN_PERIOD
    fb = field_binary(n - 2)
    with newton_context(fb, BIN_EPS) as c:
        e0 = sum(c.energy(BIN_G))
        t_blk = wall(c, lambda: c.step_kdk_block(a.c, BIN_DT_MAX, 16, 8, G=BIN_G))
        k = c.block_clock()
        e_blk = abs(sum(c.energy(BIN_G)) / e0 - 1.0)
    print("N %d binary, c = %g, block steps: %.1f ms, %d substeps, %d evaluations, pair terms %d (shared step %d: %.1f x), deepest level %d, |E/E0 - 1| %.3e" % (
        n, a.c, t_blk, k.substeps, k.evaluations, k.pair_terms, (k.substeps + 1) * n * n, (k.substeps + 1) * n * n / k.pair_terms, k.deepest_level, e_blk), flush=True)
    if a.block_only:
        sys.exit(0)
    with newton_context(fb, BIN_EPS) as c:
        e0 = sum(c.energy(BIN_G))
        t_ad = wall(c, lambda: c.step_kdk_adaptive(a.c, BIN_DT_MIN, BIN_DT_MAX, t_end=BIN_PERIOD, pow2=True, G=BIN_G))
        k = c.step_clock()
        e_ad = abs(sum(c.energy(BIN_G)) / e0 - 1.0)
    print("N %d binary, c = %g, nbx_ctx_step_kdk_adaptive (pow2): %.1f ms, %d steps, |E/E0 - 1| %.3e -> block steps %.1f x faster" % (n, a.c, t_ad, k.steps, e_ad, t_ad / t_blk), flush=True)
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
    print("N %d (%s), ms per step: ctx.step %.4f | ctx.step_kdk %.4f | ctx.step_kdk_adaptive %.4f" % (n, name, kd, kdk, ada), flush=True)
