"""Kick-drift-kick through a leaf plan (nbx_leaf_plan_step_octree_kdk) next to kick-drift (nbx_leaf_plan_step_octree).
    python tests/measure/tree_kdk.py kdk <plummer|uniform> [--n N] [--steps K]
    python tests/measure/tree_kdk.py parent <plummer|uniform> [--repo DIR] [--n N]
    python tests/measure/tree_kdk.py drift plummer [--dt DT]
uniform: LeafPlan.from_octree at depth 6 (N = 2^20) under the tree-leaf law; plummer: from_octree_adaptive(max depth 10, capacity
32) under the Newtonian law, eps 2048, G 0.1; theta 0.5.  `kdk`: per far order 0 and 1, K steps (default 100) rebuilding every step,
warm, ms per step of either loop, twice each, alternating -- kick-drift-kick makes K + 1 evaluations and rebuilds for K steps -- and
max_accel's wall time.  `parent`: the loops both commits have (step on the standing structure, step_octree, one timed forces_ctx), for
alternating processes of this commit and a build of the parent commit (--repo DIR); it touches nothing the parent lacks.  `drift`: the
Plummer sphere of tests/test_gpu_tree_kdk.py (N = 32,768) over one dynamical time at --dt (default 2): max |dE/E0| of either loop by
the context's all-pairs energy and by the plan's own."""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("kdk", "parent", "drift"))
ap.add_argument("init", choices=("plummer", "uniform"))
ap.add_argument("--n", type=int, default=0)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--dt", type=float, default=2.0)
ap.add_argument("--repo", default="")
a = ap.parse_args()
here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, a.repo or here)
import numpy as np, nbody_amd as nbx
dim, theta, eps = 3, 0.5, 2048.0
TREE_LEAF, NEWTON = 1, 3
plummer = a.init == "plummer"
law, G, dt = (NEWTON, 0.1, 0.5) if plummer else (TREE_LEAF, 4.471e-21, 1.0)


def make(c, n):
    depth = 0
    while depth < 10 and n / 2.0 ** (depth * dim) > 16.0:
        depth += 1
    p = nbx.LeafPlan.from_octree_adaptive(c, 10, 32, theta) if plummer else nbx.LeafPlan.from_octree(c, depth, theta)
    p.set_softening(eps)
    return p


if a.mode == "drift":
    n, G, dt = 32768, 0.1, a.dt
    b = nbx.plummer_bodies(n, 3, seed=5, a=1.0e5, total_mass=1.0e12, G=G)
    chunk = max(1, int(round(25.0 / dt)))                          # four energy readings over t_dyn = 100
    for scheme in ("kd", "kdk"):
        with nbx.Context(n, 3) as c:
            c.upload(b); c.set_softening(eps); c.set_law(nbx.FORCE_LAW_NEWTON)
            e0 = sum(c.energy(G))
            with nbx.LeafPlan.from_octree_adaptive(c, 10, 32, theta) as plan:
                plan.set_far_order(1); plan.set_softening(eps)
                t0 = sum(plan.energy(c, NEWTON, G))
                worst, worst_tree = 0.0, 0.0
                for _ in range(4):
                    (plan.step_octree_kdk if scheme == "kdk" else plan.step_octree)(c, NEWTON, G, dt, chunk, 1)
                    worst = max(worst, abs(sum(c.energy(G)) - e0) / abs(e0))
                    worst_tree = max(worst_tree, abs(sum(plan.energy(c, NEWTON, G)) - t0) / abs(t0))
        print("plummer N %d dt %g, %d steps, %s: max |dE/E0| all-pairs energy %.3e, tree energy %.3e" % (n, dt, 4 * chunk, scheme, worst, worst_tree), flush=True)
    sys.exit(0)

n = a.n or (1 << 20)
b = nbx.generate.plummer_bodies(n, dim, 1, G=G) if plummer else nbx.generate.uniform_bodies(n, dim, 77)
b[:, :dim] = b[:, :dim].astype(np.float32)
b = np.ascontiguousarray(b)
with nbx.Context(n, dim) as c:
    c.upload(b); c.synchronize()
    def wall(f):
        c.synchronize(); t0 = time.perf_counter(); f(); c.synchronize(); return (time.perf_counter() - t0) * 1e3
    with make(c, n) as plan:
        if a.mode == "parent":
            plan.step_octree(c, law, G, dt, 5, 1)                   # warm
            standing = [wall(lambda: plan.step(c, law, G, dt, 50)) / 50 for _ in range(2)]
            c.upload(b); plan.rebuild(c)
            rebuilt = [wall(lambda: plan.step_octree(c, law, G, dt, 20, 1)) / 20 for _ in range(2)]
            plan.forces_ctx(c, law, G, fetch=False)
            ev = [wall(lambda: plan.forces_ctx(c, law, G, fetch=False)) for _ in range(3)]
            print("%s N %d (%s): step ms %s | step_octree ms %s | forces_ctx ms %s" % (
                a.init, n, os.path.basename(os.path.abspath(a.repo or here)), " ".join("%.3f" % t for t in standing), " ".join("%.3f" % t for t in rebuilt),
                " ".join("%.3f" % t for t in ev)), flush=True)
        else:
            for order in (0, 1):
                plan.set_far_order(order)
                c.upload(b); plan.rebuild(c)
                plan.step_octree(c, law, G, dt, 10, 1)              # warm
                rec = {"kd": [], "kdk": []}
                for _ in range(2):
                    for scheme in ("kd", "kdk"):
                        c.upload(b); plan.rebuild(c)
                        f = plan.step_octree_kdk if scheme == "kdk" else plan.step_octree
                        rec[scheme].append(wall(lambda: f(c, law, G, dt, a.steps, 1)) / a.steps)
                amax = [wall(plan.max_accel) for _ in range(3)]
                print("%s N %d order %d, %d steps rebuilding every step, ms per step: step_octree %s | step_octree_kdk %s | max_accel ms %s (a_max %.4e)" % (
                    a.init, n, order, a.steps, " ".join("%.3f" % t for t in rec["kd"]), " ".join("%.3f" % t for t in rec["kdk"]),
                    " ".join("%.3f" % t for t in amax), plan.max_accel()), flush=True)
