"""The energy through a leaf plan's tree (nbx_leaf_plan_energy) against the same plan's force evaluation and against the all-pairs
diagnostic it replaces (nbx_ctx_energy), at N = 2^20, theta 0.5, 3D.
    python tools/time_tree_energy.py <plummer|uniform> [--reps K] [--n N] [--repo DIR] [--profile]
uniform: fixed depth 6; plummer: adaptive, capacity 32, max depth 10.  Laws NEWTON (softening a power of two) and TREE_LEAF, far
orders 0 and 1.  Per case, warm, in one process, host clock around the synchronising call: K times LeafPlan.energy, K times the plan's
force evaluation (forces_ctx without fetch + synchronise: moments + pair + far), and |U_tree - U_allpairs| / |U|; per law once
Context.energy.  With --repo DIR the package and its library come from another checkout, e.g. a build of the parent commit, which has no
energy through the tree: the force evaluations alone are timed (run the two in alternating processes).  --profile: three energy looks
per case and nothing else, for one kernel trace of its own.  profiles/r13/tree_energy.txt has the figures."""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("init", choices=("plummer", "uniform"))
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--theta", type=float, default=0.5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--profile", action="store_true")
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
a = ap.parse_args()
sys.path.insert(0, a.repo)
import numpy as np, nbody_amd as nbx
n, dim, G = a.n, 3, 0.1
if a.init == "plummer":
    b, eps, what = nbx.generate.plummer_bodies(n, dim, 5, G=G), 512.0, "Plummer sphere, adaptive octree (capacity 32, max depth 10)"
    make = lambda c: nbx.LeafPlan.from_octree_adaptive(c, 10, 32, a.theta)
else:
    b, eps, what = nbx.generate.uniform_bodies(n, dim, 77), 4096.0, "uniform box, octree of depth 6"
    make = lambda c: nbx.LeafPlan.from_octree(c, 6, a.theta)
b[:, :dim] = b[:, :dim].astype(np.float32)
fmt = lambda ts: "%.3f-%.3f" % (min(ts), max(ts))
has_energy = hasattr(nbx.LeafPlan, "energy")
print("%s, N = %d, theta %.2f (%s)" % (what, n, a.theta, os.path.basename(os.path.abspath(a.repo))), flush=True)
with nbx.Context(n, dim) as c:
    c.upload(b); c.synchronize()
    def wall(f):
        c.synchronize(); t0 = time.perf_counter(); r = f(); c.synchronize(); return (time.perf_counter() - t0) * 1e3, r
    with make(c) as plan:
        nl, near, nc, far = plan.structure_sizes()
        print("  leaves %d, near entries %d, cells %d, far entries %d" % (nl, near, nc, far), flush=True)
        plan.set_softening(eps)
        for law_name, law in (("NEWTON", nbx.LAW_NEWTON), ("TREE_LEAF", nbx.LAW_TREE_LEAF)):
            if law == nbx.LAW_NEWTON:
                c.set_softening(eps); c.set_law(nbx.FORCE_LAW_NEWTON)
            else:
                c.set_law(nbx.FORCE_LAW_REFERENCE); c.set_softening(0.0)
            if not a.profile:
                c.energy(G)
                ctx_ms = [wall(lambda: c.energy(G)) for _ in range(2)]
                u_all = ctx_ms[-1][1][1]
                print("  %s: nbx_ctx_energy (all pairs) ms: %s" % (law_name, fmt([t for t, _ in ctx_ms])), flush=True)
            for order in (0, 1):
                plan.set_far_order(order)
                if a.profile:
                    for _ in range(3):
                        plan.energy(c, law, G)
                    continue
                plan.forces_ctx(c, law, G, fetch=False); c.synchronize()
                force_ms = [wall(lambda: plan.forces_ctx(c, law, G, fetch=False))[0] for _ in range(a.reps)]
                line = "  %s order %d: force evaluation ms %s" % (law_name, order, fmt(force_ms))
                if has_energy:
                    plan.energy(c, law, G)
                    looks = [wall(lambda: plan.energy(c, law, G)) for _ in range(a.reps)]
                    u_tree = looks[-1][1][1]
                    line += " | energy through the tree ms %s | |U_tree - U_allpairs| / |U| = %.2e" % (
                        fmt([t for t, _ in looks]), abs(abs(u_tree) - abs(u_all)) / abs(u_all))
                print(line, flush=True)
