"""Kick-drift-kick with the step chosen on the device (nbx_leaf_plan_step_kdk_adaptive) next to the fixed-step loops.
    python tests/measure/adaptive_step.py cost <plummer|uniform> [--n N]
    python tests/measure/adaptive_step.py parent <plummer|uniform> [--repo DIR] [--n N]
    python tests/measure/adaptive_step.py buys <plummer|cold> [--dt DT] [--c C]
uniform: LeafPlan.from_octree at depth 6 (N = 2^20) under the tree-leaf law; plummer: from_octree_adaptive(max depth 10, capacity 32)
under the Newtonian law, eps 2048, G 0.1; theta 0.5, far order 0.  `cost`: the controller's price -- the adaptive loop with dt_min ==
dt_max (the fixed-step trajectory, bit for bit) against step_kdk on the standing structure (50 steps) and step_octree_kdk rebuilding
every step (20 steps), warm, ms per step, twice each, alternating.  `parent`: the loops both commits have (step, step_kdk,
step_octree_kdk, one forces_ctx), for alternating processes of this commit and a build of the parent commit (--repo DIR); it touches
nothing the parent lacks.  `buys`: the 32,768-body Plummer sphere of tests/measure/tree_kdk.py (`cold`: its velocities times 0.1, a
collapse) over one dynamical time, adaptive tree of capacity 32, order 1, rebuilt before every evaluation: max |dE/E0| by the
context's all-pairs energy, ten readings, of the adaptive loop at --c with dt_max = --dt, and of step_octree_kdk with the same number
of steps and readings; the dt range the device chose."""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("cost", "parent", "buys"))
ap.add_argument("init", choices=("plummer", "uniform", "cold"))
ap.add_argument("--n", type=int, default=0)
ap.add_argument("--dt", type=float, default=4.0)
ap.add_argument("--c", type=float, default=2.0)
ap.add_argument("--repo", default="")
a = ap.parse_args()
here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, a.repo or here)
import numpy as np, nbody_amd as nbx
dim, theta, eps = 3, 0.5, 2048.0
TREE_LEAF, NEWTON = 1, 3
INF = float("inf")

if a.mode == "buys":
    n, G = 32768, 0.1
    b = nbx.plummer_bodies(n, 3, seed=5, a=1.0e5, total_mass=1.0e12, G=G)
    if a.init == "cold":
        b[:, 3:6] *= 0.1
    t_end, readings = 100.0, 10
    out = {}
    with nbx.Context(n, 3) as c, nbx.Context(n, 3) as c2:
        for ctx in (c, c2):
            ctx.upload(b); ctx.set_softening(eps); ctx.set_law(nbx.FORCE_LAW_NEWTON)
        e0 = sum(c.energy(G))
        with nbx.LeafPlan.from_octree_adaptive(c, 10, 32, theta) as plan:
            plan.set_far_order(1); plan.set_softening(eps)
            worst, steps, evals, lo, hi, t = 0.0, [], 0, INF, 0.0, 0.0
            for r in range(readings):
                k = plan.step_kdk_adaptive(c, NEWTON, G, a.c, a.dt / 1024, a.dt, t_end=t_end * (r + 1) / readings, max_steps=1 << 16, rebuild_every=1, t_start=t)
                d = plan.step_history()[1][:-1]
                t, evals = k.t, evals + k.evaluations
                steps.append(k.steps); lo, hi = min(lo, d.min()), max(hi, d.max())
                worst = max(worst, abs(sum(c.energy(G)) - e0) / abs(e0))
            assert k.finished and k.status == 0
        with nbx.LeafPlan.from_octree_adaptive(c2, 10, 32, theta) as plan:
            plan.set_far_order(1); plan.set_softening(eps)
            fixed, fevals = 0.0, 0
            dt = t_end / sum(steps)
            for r in range(readings):
                plan.step_octree_kdk(c2, NEWTON, G, dt, steps[r], 1)
                fevals += steps[r] + 1
                fixed = max(fixed, abs(sum(c2.energy(G)) - e0) / abs(e0))
    print("%s N %d, t = %g, c = %g, dt_max = %g: adaptive %d steps, %d evaluations, dt %.4g .. %.4g, max |dE/E0| %.3e | step_octree_kdk dt %.4g, %d evaluations, max |dE/E0| %.3e" % (
        a.init, n, t_end, a.c, a.dt, sum(steps), evals, lo, hi, worst, dt, fevals, fixed), flush=True)
    sys.exit(0)

plummer = a.init == "plummer"
law, G, dt = (NEWTON, 0.1, 0.5) if plummer else (TREE_LEAF, 4.471e-21, 1.0)
n = a.n or (1 << 20)
b = nbx.generate.plummer_bodies(n, dim, 1, G=G) if plummer else nbx.generate.uniform_bodies(n, dim, 77)
b[:, :dim] = b[:, :dim].astype(np.float32)
b = np.ascontiguousarray(b)
depth = 0
while depth < 10 and n / 2.0 ** (depth * dim) > 16.0:
    depth += 1
name = os.path.basename(os.path.abspath(a.repo or here))
with nbx.Context(n, dim) as c:
    c.upload(b); c.synchronize()
    def wall(f):
        c.synchronize(); t0 = time.perf_counter(); f(); c.synchronize(); return (time.perf_counter() - t0) * 1e3
    with (nbx.LeafPlan.from_octree_adaptive(c, 10, 32, theta) if plummer else nbx.LeafPlan.from_octree(c, depth, theta)) as plan:
        plan.set_softening(eps)
        plan.step_octree_kdk(c, law, G, dt, 5, 1)                   # warm
        fmt = lambda ts: " ".join("%.3f" % t for t in ts)
        if a.mode == "parent":
            kd = [wall(lambda: plan.step(c, law, G, dt, 50)) / 50 for _ in range(2)]
            kdk = [wall(lambda: plan.step_kdk(c, law, G, dt, 50)) / 50 for _ in range(2)]
            c.upload(b); plan.rebuild(c)
            rebuilt = [wall(lambda: plan.step_octree_kdk(c, law, G, dt, 20, 1)) / 20 for _ in range(2)]
            plan.forces_ctx(c, law, G, fetch=False)
            ev = [wall(lambda: plan.forces_ctx(c, law, G, fetch=False)) for _ in range(3)]
            print("%s N %d (%s): step ms %s | step_kdk ms %s | step_octree_kdk ms %s | forces_ctx ms %s" % (a.init, n, name, fmt(kd), fmt(kdk), fmt(rebuilt), fmt(ev)), flush=True)
        else:
            def adaptive(steps, every):
                plan.step_kdk_adaptive(c, law, G, 1.0, dt, dt, max_steps=steps, rebuild_every=every)   # returns the clock: one synchronising read-back per call
            adaptive(5, 1)
            rec = {k: [] for k in ("kdk", "kdka", "okdk", "okdka")}
            for _ in range(2):
                c.upload(b); plan.rebuild(c)
                rec["kdk"].append(wall(lambda: plan.step_kdk(c, law, G, dt, 50)) / 50)
                c.upload(b); plan.rebuild(c)
                rec["kdka"].append(wall(lambda: adaptive(50, 0)) / 50)
                c.upload(b); plan.rebuild(c)
                rec["okdk"].append(wall(lambda: plan.step_octree_kdk(c, law, G, dt, 20, 1)) / 20)
                c.upload(b); plan.rebuild(c)
                rec["okdka"].append(wall(lambda: adaptive(20, 1)) / 20)
            print("%s N %d, ms per step: step_kdk %s | adaptive, dt_min = dt_max %s | step_octree_kdk %s | adaptive rebuilding every step %s" % (
                a.init, n, fmt(rec["kdk"]), fmt(rec["kdka"]), fmt(rec["okdk"]), fmt(rec["okdka"])), flush=True)
