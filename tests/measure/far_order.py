"""The far field's order (nbx_leaf_plan_set_far_order) at N = 2^20 (3D, law TREE_LEAF): cost per pass and per step, and accuracy.
    python tests/measure/far_order.py time <plummer|uniform> <order> <theta> [--repo DIR] [--n N]
    python tests/measure/far_order.py accuracy <plummer|uniform> [--n N] [--rows K]
uniform: LeafPlan.from_octree at the harness default depth (6 at N = 2^20, 5 at 131,072); plummer: from_octree_adaptive(max depth 10,
capacity 32).  `time` prints one record per process: the structure's sizes, one timed evaluation split into moments / pair / far
(device events, after an untimed one), and step_octree(10 steps, rebuild_every = 1) per step, twice.  With --repo DIR the package
and its library come from another checkout (a build of the parent commit; order must then be 0 and is not set).  Run the
configurations in alternating processes (profiles/r11/quadrupole.txt).  `accuracy` prints the median and 99th percentile of the
relative force error of K sampled rows against fp64 all-pairs sums (oracle/liboracle.so) at order 0, theta 0.5 and at order 1 for a
range of theta, default N = 131,072."""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("time", "accuracy"))
ap.add_argument("init", choices=("plummer", "uniform"))
ap.add_argument("order", type=int, nargs="?", default=0)
ap.add_argument("theta", type=float, nargs="?", default=0.5)
ap.add_argument("--n", type=int, default=0)
ap.add_argument("--rows", type=int, default=4096)
ap.add_argument("--repo", default="")
a = ap.parse_args()
here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, a.repo or here)
import numpy as np, nbody_amd as nbx
dim, G = 3, 4.471e-21
n = a.n or ((1 << 20) if a.mode == "time" else (1 << 17))
b = nbx.generate.plummer_bodies(n, dim, 1) if a.init == "plummer" else nbx.generate.uniform_bodies(n, dim, 77)
b[:, :dim] = b[:, :dim].astype(np.float32)
depth = 0
while depth < 10 and n / 2.0 ** (depth * dim) > 16.0:
    depth += 1


def make(c, theta):
    return nbx.LeafPlan.from_octree_adaptive(c, 10, 32, theta) if a.init == "plummer" else nbx.LeafPlan.from_octree(c, depth, theta)


what = "adaptive capacity 32 max_depth 10" if a.init == "plummer" else "fixed depth %d" % depth
if a.mode == "time":
    with nbx.Context(n, dim) as c:
        c.upload(b); c.synchronize()
        def wall(f):
            c.synchronize(); t0 = time.perf_counter(); r = f(); c.synchronize(); return (time.perf_counter() - t0) * 1e3, r
        plan = make(c, a.theta)
        if not a.repo:
            plan.set_far_order(a.order)
        elif a.order:
            sys.exit("--repo runs another checkout's order 0 only")
        nl, near, nc, far = plan.structure_sizes()
        plan.forces_ctx(c, 1, G, fetch=False)
        pair_ms = plan.forces_ctx(c, 1, G, fetch=False, timed=True)
        info = plan.cell_info()
        steps = [wall(lambda: plan.step_octree(c, 1, G, 1.0, 10, 1))[0] / 10 for _ in range(2)]
        print("%s %s order %d theta %.2f (%s): leaves %d near %d cells %d far %d | evaluation ms: moments %.3f pair %.3f far %.3f | step with rebuild ms: %s"
              % (a.init, what, a.order, a.theta, os.path.basename(os.path.abspath(a.repo or here)), nl, near, nc, far, info[2], pair_ms, info[3],
                 " ".join("%.3f" % t for t in steps)), flush=True)
        plan.close()
else:
    sys.path.insert(0, os.path.join(here, "tests"))
    from oracle_lib import Oracle
    oracle = Oracle()
    rows = np.sort(np.random.default_rng(11).choice(n, min(a.rows, n), replace=False))
    b = np.ascontiguousarray(b)
    ref = -oracle.force_rows_omp_2(b, rows)                          # the oracle's brute force pushes, the tree law pulls
    with nbx.Context(n, dim) as c:
        c.upload(b)
        for order, theta in ((0, 0.5), (1, 0.5), (1, 0.6), (1, 0.7), (1, 0.8), (1, 0.9), (1, 1.0), (1, 1.1), (1, 1.2)):
            with make(c, theta) as plan:
                plan.set_far_order(order)
                f = plan.forces_ctx(c, 1, oracle.G)[rows]
                nl, near, nc, far = plan.structure_sizes()
            e = np.sqrt(((f - ref) ** 2).sum(axis=1)) / np.sqrt((ref ** 2).sum(axis=1))
            print("%s %s N %d order %d theta %.1f: relative error median %.3e p99 %.3e max %.3e | near %d far %d entries"
                  % (a.init, what, n, order, theta, np.median(e), np.percentile(e, 99), e.max(), near, far), flush=True)
