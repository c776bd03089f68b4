"""Softened Newtonian gravity on a leaf plan (NBX_LAW_NEWTON) next to the tree-leaf law, in one process on one plan.
    python tests/measure/newton_tree.py time <plummer|uniform> [--n N] [--eps E] [--reps R]
    python tests/measure/newton_tree.py accuracy <plummer|uniform> [--n N] [--eps E]
    python tests/measure/newton_tree.py step <plummer|uniform> [--repo DIR] [--n N]
uniform: LeafPlan.from_octree at depth 6 (N = 2^20; the harness default); plummer: from_octree_adaptive(max depth 10, capacity 32);
theta 0.5.  `time` (default N = 2^20) prints, per far order 0 and 1: the pair kernel under TREE_LEAF and under NEWTON from
nbx_leaf_plan_time_kernel (alternating, three times each), the moments and far-pass times of a timed evaluation under either law, and
step_octree(10 steps, rebuilding every step) per step under either law.  `accuracy` (default N = 131,072): median and 99th
percentile of the relative error of every body against the context's all-pairs forces of the same law (nbx_ctx_get_forces).
`step` is the default-law record of tests/measure/far_order.py (order 0: moments / pair / far and the step with rebuild), for
alternating processes of this commit and a build of the parent commit (--repo DIR); it touches nothing the parent lacks."""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("time", "accuracy", "step"))
ap.add_argument("init", choices=("plummer", "uniform"))
ap.add_argument("--n", type=int, default=0)
ap.add_argument("--eps", type=float, default=2048.0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--repo", default="")
a = ap.parse_args()
here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, a.repo or here)
import numpy as np, nbody_amd as nbx
dim, theta = 3, 0.5
n = a.n or ((1 << 17) if a.mode == "accuracy" else (1 << 20))
G = 0.1 if a.init == "plummer" else 4.471e-21
b = nbx.generate.plummer_bodies(n, dim, 1, G=G) if a.init == "plummer" else nbx.generate.uniform_bodies(n, dim, 77)
b[:, :dim] = b[:, :dim].astype(np.float32)
b = np.ascontiguousarray(b)
depth = 0
while depth < 10 and n / 2.0 ** (depth * dim) > 16.0:
    depth += 1
what = "adaptive capacity 32 max_depth 10" if a.init == "plummer" else "fixed depth %d" % depth
TREE_LEAF, NEWTON = 1, 3


def make(c):
    return nbx.LeafPlan.from_octree_adaptive(c, 10, 32, theta) if a.init == "plummer" else nbx.LeafPlan.from_octree(c, depth, theta)


with nbx.Context(n, dim) as c:
    c.upload(b); c.synchronize()
    def wall(f):
        c.synchronize(); t0 = time.perf_counter(); f(); c.synchronize(); return (time.perf_counter() - t0) * 1e3
    if a.mode == "step":
        with make(c) as plan:
            nl, near, nc, far = plan.structure_sizes()
            plan.forces_ctx(c, TREE_LEAF, G, fetch=False)
            pair_ms = plan.forces_ctx(c, TREE_LEAF, G, fetch=False, timed=True)
            info = plan.cell_info()
            steps = [wall(lambda: plan.step_octree(c, TREE_LEAF, G, 1.0, 10, 1)) / 10 for _ in range(2)]
            print("%s %s TREE_LEAF order 0 (%s): leaves %d near %d cells %d far %d | evaluation ms: moments %.3f pair %.3f far %.3f | step with rebuild ms: %s"
                  % (a.init, what, os.path.basename(os.path.abspath(a.repo or here)), nl, near, nc, far, info[2], pair_ms, info[3],
                     " ".join("%.3f" % t for t in steps)), flush=True)
    elif a.mode == "time":
        with make(c) as plan:
            plan.set_softening(a.eps)
            nl, near, nc, far = plan.structure_sizes()
            print("%s %s N %d eps %g: leaves %d near %d cells %d far %d; layout %s" % (a.init, what, n, a.eps, nl, near, nc, far, plan.info()), flush=True)
            for order in (0, 1):
                plan.set_far_order(order)
                rec = {}
                for law in (TREE_LEAF, NEWTON):
                    plan.forces_ctx(c, law, G, fetch=False)
                    plan.forces_ctx(c, law, G, fetch=False, timed=True)
                    rec[law] = plan.cell_info()[2:]
                plan.forces_ctx(c, TREE_LEAF, G, fetch=False)
                pair = {TREE_LEAF: [], NEWTON: []}
                for _ in range(3):
                    for law in (TREE_LEAF, NEWTON):
                        pair[law].append(plan.time_kernel(law, a.reps))
                print("  order %d pair kernel ms (time_kernel, %d reps): TREE_LEAF %s | NEWTON %s" % (
                    order, a.reps, " ".join("%.4f" % t for t in pair[TREE_LEAF]), " ".join("%.4f" % t for t in pair[NEWTON])), flush=True)
                print("  order %d moments / far ms: TREE_LEAF %.3f / %.3f | NEWTON %.3f / %.3f" % (order, *rec[TREE_LEAF], *rec[NEWTON]), flush=True)
                state = b.copy()
                steps = {}
                for law in (TREE_LEAF, NEWTON):
                    steps[law] = []
                    for _ in range(2):
                        c.upload(state); plan.rebuild(c)
                        steps[law].append(wall(lambda: plan.step_octree(c, law, G, 0.5, 10, 1)) / 10)
                print("  order %d step with rebuild ms: TREE_LEAF %s | NEWTON %s" % (
                    order, " ".join("%.3f" % t for t in steps[TREE_LEAF]), " ".join("%.3f" % t for t in steps[NEWTON])), flush=True)
                c.upload(state); plan.rebuild(c)
    else:
        c.set_softening(a.eps)
        c.set_law(nbx.FORCE_LAW_NEWTON)
        c.compute_accel()
        ref = c.forces(G)
        with make(c) as plan:
            plan.set_softening(a.eps)
            for order in (0, 1):
                plan.set_far_order(order)
                f = plan.forces_ctx(c, NEWTON, G)
                e = np.sqrt(((f - ref) ** 2).sum(axis=1)) / np.sqrt((ref ** 2).sum(axis=1))
                print("%s %s N %d eps %g NEWTON order %d theta %.1f: relative error against the all-pairs forces median %.3e p99 %.3e max %.3e"
                      % (a.init, what, n, a.eps, order, theta, np.median(e), np.percentile(e, 99), e.max()), flush=True)
