"""The octree built on the device against the host-array path at N = 2^20 (uniform bodies, seed 77, 3D, theta 0.5).
    python tools/time_octree_device.py octree <depth> [--check] [--save FILE] [--reps K]
        wall time of LeafPlan.from_octree and of K rebuilds, of step_octree with rebuild_every = 1 against 0, the shader clock;
        --check compares the structure with leaves.octree_cells word for word (44 s at depth 6), --save writes it as .npz
    python tools/time_octree_device.py host <depth> --load FILE [--repo DIR] [--reps K]
        wall time of nbx_leaf_plan_create + nbx_leaf_plan_set_cells fed the ready host arrays of FILE; --repo imports the
        package (and its library) from another checkout, e.g. a build of the parent commit
Run the two in alternating processes (profiles/r7/octree_device.txt)."""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("octree", "host"))
ap.add_argument("depth", type=int)
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--theta", type=float, default=0.5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--check", action="store_true")
ap.add_argument("--save")
ap.add_argument("--load")
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
a = ap.parse_args()
sys.path.insert(0, a.repo)
import numpy as np, nbody_amd as nbx
NAMES = ("leaf_offsets", "leaf_bodies", "list_offsets", "list_sources", "cell_first_leaf", "cell_leaf_count", "far_offsets", "far_cells")
n, dim, G = a.n, 3, 4.471e-21
b = nbx.uniform_bodies(n, dim, 77)
fmt = lambda ts: " ".join("%.3f" % t for t in ts)
with nbx.Context(n, dim) as c:
    c.upload(b); c.synchronize()
    def wall(f):
        c.synchronize(); t0 = time.perf_counter(); r = f(); c.synchronize(); return (time.perf_counter() - t0) * 1e3, r
    c.enable_clock_stamps(True); c.compute_accel(); c.synchronize()
    print("shader clock before:", c.shader_clock())
    if a.mode == "octree":
        t_first, plan = wall(lambda: nbx.LeafPlan.from_octree(c, a.depth, a.theta))
        print("depth %d: %s leaves / near entries / cells / far entries" % (a.depth, plan.structure_sizes()))
        print("from_octree (first in the process: allocations) %.3f ms" % t_first)
        plan.close()
        t_again, plan = wall(lambda: nbx.LeafPlan.from_octree(c, a.depth, a.theta))
        print("from_octree (parked blocks) %.3f ms" % t_again)
        print("rebuild x %d: %s ms" % (a.reps, fmt(wall(lambda: plan.rebuild(c))[0] for _ in range(a.reps))))
        print("forces_ctx (timed), near kernel ms:", plan.forces_ctx(c, 1, G, fetch=False, timed=True), "cell_info:", plan.cell_info())
        for every in (0, 1, 0, 1):
            print("step_octree(10 steps, rebuild_every = %d): %.3f ms per step" % (every, wall(lambda: plan.step_octree(c, 1, G, 1.0, 10, every))[0] / 10))
        c.upload(b)
        plan.rebuild(c)
        s = plan.structure()
        if a.check:
            t0 = time.perf_counter()
            want = nbx.leaves.octree_cells(b, dim, a.depth, a.theta)
            print("host builder leaves.octree_cells: %.1f s" % (time.perf_counter() - t0))
            for name, g, w in zip(NAMES, s, want):
                assert np.array_equal(g, w), name
            print("structure equals the host builder's word for word")
        if a.save:
            np.savez(a.save, **dict(zip(NAMES, s)))
        plan.close()
    else:
        z = np.load(a.load)
        s = [np.ascontiguousarray(z[k]) for k in NAMES]
        def make():
            p = nbx.LeafPlan(n, dim, *s[:4]); p.set_cells(*s[4:]); return p
        ts = []
        for _ in range(a.reps + 1):
            t, p = wall(make)
            ts.append(t); p.close()
        print("depth %d host arrays: create + set_cells, first %.3f ms, then %s ms" % (a.depth, ts[0], fmt(ts[1:])))
    c.compute_accel(); c.synchronize()
    print("shader clock after:", c.shader_clock())
