"""The adaptive octree built on the device against the fixed-depth one at N = 2^20 (3D, theta 0.5, law TREE_LEAF).
    python tools/time_octree_adaptive.py <plummer|uniform> <leaf_capacity> [--depth D] [--repo DIR] [--reps K]
leaf_capacity > 0: LeafPlan.from_octree_adaptive(ctx, D (default 10), leaf_capacity, theta); leaf_capacity = 0: LeafPlan.from_octree
at depth D (default: the harness default, at most 16 bodies per cell on average) -- with --repo DIR the package and its library come
from another checkout, e.g. a build of the parent commit.  One process prints one record: the structure's sizes, K rebuilds (wall
time of the call and the synchronisation behind it), one timed evaluation split into moments / pair / far (device events), and
step_octree(10 steps, rebuild_every = 1) per step.  Run the configurations in alternating processes
(profiles/r9/adaptive_octree.txt)."""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("init", choices=("plummer", "uniform"))
ap.add_argument("leaf_capacity", type=int)
ap.add_argument("--depth", type=int, default=0)
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--theta", type=float, default=0.5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
a = ap.parse_args()
sys.path.insert(0, a.repo)
import numpy as np, nbody_amd as nbx
n, dim, G = a.n, 3, 4.471e-21
b = nbx.generate.plummer_bodies(n, dim, 1) if a.init == "plummer" else nbx.generate.uniform_bodies(n, dim, 77)
b[:, :dim] = b[:, :dim].astype(np.float32)
fmt = lambda ts: " ".join("%.3f" % t for t in ts)
if a.leaf_capacity > 0:
    depth = a.depth or 10
    make = lambda c: nbx.LeafPlan.from_octree_adaptive(c, depth, a.leaf_capacity, a.theta)
    what = "adaptive capacity %d max_depth %d" % (a.leaf_capacity, depth)
else:
    depth = a.depth
    while not a.depth and depth < 10 and n / 2.0 ** (depth * dim) > 16.0:
        depth += 1
    make = lambda c: nbx.LeafPlan.from_octree(c, depth, a.theta)
    what = "fixed depth %d" % depth
with nbx.Context(n, dim) as c:
    c.upload(b); c.synchronize()
    def wall(f):
        c.synchronize(); t0 = time.perf_counter(); r = f(); c.synchronize(); return (time.perf_counter() - t0) * 1e3, r
    t_first, plan = wall(lambda: make(c))
    nl, near, nc, far = plan.structure_sizes()
    sizes = np.diff(plan.structure()[0].astype(np.int64))
    rebuilds = [wall(lambda: plan.rebuild(c))[0] for _ in range(a.reps)]
    plan.forces_ctx(c, 1, G, fetch=False)
    pair_ms = plan.forces_ctx(c, 1, G, fetch=False, timed=True)
    info = plan.cell_info()
    steps = [wall(lambda: plan.step_octree(c, 1, G, 1.0, 10, 1))[0] / 10 for _ in range(2)]
    print("%s %s (%s): leaves %d largest %d near %d cells %d far %d | first build %.2f | rebuild ms: %s | evaluation ms: moments %.3f pair %.3f far %.3f | step with rebuild ms: %s"
          % (a.init, what, os.path.basename(os.path.abspath(a.repo)), nl, int(sizes.max()), near, nc, far, t_first, fmt(rebuilds), info[2], pair_ms, info[3], fmt(steps)), flush=True)
    plan.close()
