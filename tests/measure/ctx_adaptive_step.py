"""The all-pairs context's kick-drift-kick with the step chosen on the device (nbx_ctx_step_kdk_adaptive) next to the loops it joins.
    python tests/measure/ctx_adaptive_step.py window [--n N] [--steps K]
    python tests/measure/ctx_adaptive_step.py waste  [--n N]
    python tests/measure/ctx_adaptive_step.py host   [--n N] [--steps K]
    python tests/measure/ctx_adaptive_step.py parent [--repo DIR] [--n N] [--steps K]
    python tests/measure/ctx_adaptive_step.py trace  [--n N] [--steps K]
    python tests/measure/ctx_adaptive_step.py energy
Bodies: the reference's uniform bodies, D = 3, default (mixed) mode, reference law, G the reference's, dt = 1.
`window`: the controller's price and the choice of W -- the adaptive loop with dt_min == dt_max (the fixed-step trajectory, bit for bit)
in contexts made with NBODY_HIP_STEP_WINDOW = 1, 2, 4, 8 against nbx_ctx_step_kdk in the same process, K steps a run, runs alternating,
five each, warm; ms per step, every run printed.  `waste`: what lies behind a stop -- a call with max_steps = 16 whose t_end is
reached by its first step, per window, against step_kdk of one step.  `host`: what the loop replaces -- per step get_forces, the maximum
on the host, kick_drift2 -- against the adaptive loop choosing the same way.  `parent`: the loops both commits have (nbx_ctx_step,
nbx_ctx_step_kdk, the plan's step_kdk_adaptive), for alternating processes of this commit and a build of the parent commit
(--repo DIR); it touches nothing the parent lacks.  `trace`: K adaptive steps and K step_kdk steps and nothing else, to be run under a
kernel trace.  `energy`: a cold 32,768-body Plummer sphere (velocities x 0.1: a collapse) under the all-pairs Newtonian law over one
dynamical time, ten readings of Context.energy: the adaptive loop against step_kdk with the same number of steps and evaluations."""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("window", "waste", "host", "parent", "trace", "energy"))
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--steps", type=int, default=0)
ap.add_argument("--repo", default="")
a = ap.parse_args()
here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, a.repo or here)
import numpy as np, nbody_amd as nbx
INF = float("inf")
fmt = lambda ts: " ".join("%.3f" % t for t in ts)

if a.mode == "energy":
    n, G, eps, t_end, readings = 32768, 0.1, 2048.0, 100.0, 10
    b = nbx.plummer_bodies(n, 3, seed=5, a=1.0e5, total_mass=1.0e12, G=G)
    b[:, 3:6] *= 0.1
    for c_len, dt_max in ((2.0, 4.0), (0.5, 4.0)):
        with nbx.Context(n, 3) as c, nbx.Context(n, 3) as c2:
            for ctx in (c, c2):
                ctx.upload(b); ctx.set_softening(eps); ctx.set_law(nbx.FORCE_LAW_NEWTON)
            e0 = sum(c.energy(G))
            worst, steps, evals, lo, hi, t = 0.0, [], 0, INF, 0.0, 0.0
            for r in range(readings):
                k = c.step_kdk_adaptive(c_len, dt_max / 1024, dt_max, t_end=t_end * (r + 1) / readings, max_steps=1 << 16, t_start=t, G=G)
                d = c.step_history()[1][:-1]
                t, evals = k.t, evals + k.evaluations
                steps.append(k.steps); lo, hi = min(lo, d.min()), max(hi, d.max())
                worst = max(worst, abs(sum(c.energy(G)) - e0) / abs(e0))
            assert k.finished and k.status == 0
            fixed, fevals, dt = 0.0, 0, t_end / sum(steps)
            for r in range(readings):
                c2.step_kdk(dt, steps[r], G)
                fevals += steps[r] + 1
                fixed = max(fixed, abs(sum(c2.energy(G)) - e0) / abs(e0))
        print("cold N %d, t = %g, c = %g, dt_max = %g: adaptive %d steps, %d evaluations, dt %.4g .. %.4g, max |dE/E0| %.3e | step_kdk dt %.4g, %d evaluations, max |dE/E0| %.3e" % (
            n, t_end, c_len, dt_max, sum(steps), evals, lo, hi, worst, dt, fevals, fixed), flush=True)
    sys.exit(0)

n, dim, G, dt = a.n, 3, nbx.REFERENCE_G, 1.0
K = a.steps or (200 if n <= 4096 else 50 if n <= 65536 else 3)
b = nbx.generate.uniform_bodies(n, dim, 77)
b[:, :dim] = b[:, :dim].astype(np.float32)
b = np.ascontiguousarray(b)
name = os.path.basename(os.path.abspath(a.repo or here))


def make(window=None):
    if window is None:
        os.environ.pop("NBODY_HIP_STEP_WINDOW", None)
    else:
        os.environ["NBODY_HIP_STEP_WINDOW"] = str(window)        # read when the context is created
    c = nbx.Context(n, dim)
    c.upload(b); c.synchronize()
    return c


def wall(c, f):
    c.synchronize(); t0 = time.perf_counter(); f(); c.synchronize(); return (time.perf_counter() - t0) * 1e3


if a.mode == "parent":
    with make() as c:
        c.step(dt, 5, G)
        kd = [wall(c, lambda: c.step(dt, K, G)) / K for _ in range(2)]
        kdk = [wall(c, lambda: c.step_kdk(dt, K, G)) / K for _ in range(2)]
        m = min(n, 65536)
        with nbx.Context(m, dim) as c2:
            c2.upload(b[:m])
            with nbx.LeafPlan.from_octree(c2, 4, 0.5) as plan:
                plan.set_softening(2048.0)
                plan.step_kdk_adaptive(c2, 1, G, 1.0, dt, dt, max_steps=5)
                pa = [wall(c2, lambda: plan.step_kdk_adaptive(c2, 1, G, 1.0, dt, dt, max_steps=50)) / 50 for _ in range(2)]
    print("N %d (%s): ctx.step ms %s | ctx.step_kdk ms %s | plan.step_kdk_adaptive (N %d) ms %s" % (n, name, fmt(kd), fmt(kdk), m, fmt(pa)), flush=True)
    sys.exit(0)

if a.mode == "trace":
    with make() as c:
        c.step_kdk_adaptive(1.0, dt, dt, max_steps=K, G=G)
        c.step_kdk(dt, K, G)
        c.synchronize()
    sys.exit(0)

if a.mode == "host":
    with make() as c, make() as h:
        c.compute_accel(); h.compute_accel()
        c_len = 0.16 * c.max_accel(G)
        lo, hi = 0.05, 4.0

        def host_loop():
            prev = 0.0
            for _ in range(K):
                f = h.forces(G)                                    # 24 B x N over the host link, and a synchronisation
                a_max = float(np.sqrt((f * f).sum(axis=1) / (b[:, -1] ** 2)).max())
                step = nbx.leaves.choose_step(a_max, c_len, lo, hi)
                h.kick_drift2(0.5 * prev + 0.5 * step, step, G)
                h.compute_accel()
                prev = step
            h.kick_drift2(0.5 * prev, 0.0, G)

        device_loop = lambda: c.step_kdk_adaptive(c_len, lo, hi, max_steps=K, G=G)
        host_loop(); device_loop()
        rec = {"host": [], "device": []}
        for _ in range(5):
            rec["host"].append(wall(h, host_loop) / K)
            rec["device"].append(wall(c, device_loop) / K)
    print("N %d, %d steps a run, ms per step: get_forces + numpy max + kick_drift2 %s | nbx_ctx_step_kdk_adaptive %s" % (n, K, fmt(rec["host"]), fmt(rec["device"])), flush=True)
    sys.exit(0)

windows = (1, 2, 4, 8)
ctxs = {w: make(w) for w in windows}
fixed = make()
try:
    if a.mode == "window":
        run = {w: (lambda w=w: ctxs[w].step_kdk_adaptive(1.0, dt, dt, max_steps=K, G=G)) for w in windows}
        for w in windows:
            run[w]()
        fixed.step_kdk(dt, K, G)
        rec = {k: [] for k in ("kdk",) + windows}
        for _ in range(5):
            rec["kdk"].append(wall(fixed, lambda: fixed.step_kdk(dt, K, G)) / K)
            for w in windows:
                rec[w].append(wall(ctxs[w], run[w]) / K)
        print("N %d, %d steps a run, ms per step: step_kdk %s | " % (n, K, fmt(rec["kdk"])) + " | ".join("W=%d %s" % (w, fmt(rec[w])) for w in windows), flush=True)
    else:
        run = {w: (lambda w=w: ctxs[w].step_kdk_adaptive(1.0, dt, dt, t_end=dt, max_steps=16, G=G)) for w in windows}
        for w in windows:
            run[w]()
        fixed.step_kdk(dt, 1, G)
        rec = {k: [] for k in ("kdk",) + windows}
        for _ in range(3):
            rec["kdk"].append(wall(fixed, lambda: fixed.step_kdk(dt, 1, G)))
            for w in windows:
                rec[w].append(wall(ctxs[w], run[w]))
        print("N %d, one step then the stop (max_steps 16), ms per call: step_kdk of one step %s | " % (n, fmt(rec["kdk"])) + " | ".join("W=%d %s" % (w, fmt(rec[w])) for w in windows), flush=True)
finally:
    for c in list(ctxs.values()) + [fixed]:
        c.close()
