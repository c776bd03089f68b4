"""TEST INFRASTRUCTURE, run as a program by tests/test_gpu_exchange.py: R sharded contexts stepped by hand on device 0 with
the position exchange done by this file's own torch copies.  A process of its own because torch has to initialise the GPU
before the HIP library does (as in the one-process-per-rank workers); the pytest process has long loaded the library.

    python tests/exchange_hand_ranks.py JOBS.json RESULTS.json
JOBS: [[case name, scheme, fault or null, stale_energy]], fault = [class, reader, source]; RESULTS: one
{"dv", "dx", "rke", "rpe"} per job -- error / tolerance of velocities, positions, kinetic and potential energy against the
specification (tests/exchange_case.py)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import exchange_case as ec


def set_law(obj, nbx, c):
    if c["eps"] > 0:
        obj.set_softening(c["eps"])
    obj.set_law(nbx.FORCE_LAW_NEWTON if c["law"] == "newton" else nbx.FORCE_LAW_REFERENCE)


def ratios(got, states, dim, steps, vel_tol=ec.VEL_TOL):
    """(moved, velocity error / tolerance, position error / tolerance) of a final state against the specification's."""
    ref = states[-1]
    moved = ec.moved_of(states, dim)
    assert moved > 1e-6, "coupling too weak to move the bodies measurably"
    dv = np.abs(got[:, dim:2 * dim] - ref[:, dim:2 * dim]).max() / (vel_tol * moved)
    dx = (np.abs(got[:, :dim] - ref[:, :dim]) / (ec.POS_RTOL * np.abs(ref[:, :dim]) + vel_tol * moved * ec.DT * steps)).max()
    return moved, float(dv), float(dx)


def energy_ratios(ke, pe, got, c, G):
    ke_ref, pe_ref = ec.energy_spec(got, c["dim"], G, c["law"], c["eps"])
    return float(abs(ke - ke_ref) / (1e-12 * ke_ref)), float(abs(pe - pe_ref) / (ec.PE_TOL * abs(pe_ref)))


class HandRanks:
    """R sharded contexts on device 0, each with exchange buffers of its own in torch memory and a torch stream of its own
    (what HipShardBackend sets up per process).  The exchange is done here: after every drift a rank keeps a copy of its own
    chunk (state e), and before a REMOTE pass the reader's buffer receives every other rank's chunk of the evaluation's state
    -- or, for the one (reader, source) pair of `fault`, the rows and the state exchange_case.faulty_view names."""

    def __init__(self, nbx, b, c):
        import torch
        self.torch, self.nbx, self.b, self.c = torch, nbx, b, c
        self.R, self.dim, n = c["ranks"], c["dim"], b.shape[0]
        self.bounds = ec.shard_bounds(n, self.R)
        dev = torch.device("cuda", 0)
        self.ctx, self.pos, self.mass, self.stream = [], [], [], []
        for r in range(self.R):
            ctx = nbx.Context(n, self.dim, device=0, n_shards=self.R, shard=r)
            self.ctx.append(ctx)
            self.pos.append(torch.zeros((self.R, self.dim, ctx.shard_pad), dtype=torch.float32, device=dev))
            self.mass.append(torch.zeros((self.R, ctx.shard_pad), dtype=torch.float32, device=dev))
            self.stream.append(torch.cuda.Stream(device=dev))
            ctx.set_gather_buffers(self.pos[r].data_ptr(), self.mass[r].data_ptr())
            ctx.set_stream(self.stream[r].cuda_stream)
        torch.cuda.synchronize(dev)                          # the zero fills are done before the contexts' streams write
        facts = [self.ctx[r].upload_shard(np.ascontiguousarray(b[lo:hi])) for r, (lo, hi) in enumerate(self.bounds)]
        for r in range(self.R):
            for q in range(self.R):
                if q != r:
                    self.mass[r][q].copy_(self.mass[q][q])
                    self.pos[r][q].copy_(self.pos[q][q])
        torch.cuda.synchronize(dev)
        for ctx in self.ctx:
            ctx.upload_finish(max(f[0] for f in facts), max(f[1] for f in facts))
            set_law(ctx, nbx, c)
        self.hist = [[self.pos[q][q].clone()] for q in range(self.R)]     # hist[q][e]: q's own chunk at state e
        torch.cuda.synchronize(dev)

    def close(self):
        self.torch.cuda.synchronize()
        for ctx in self.ctx:
            ctx.close()

    def _exchange(self, r, e, n_evals, n_states, fault):
        torch = self.torch
        for q in range(self.R):
            if q == r:
                continue
            self.stream[r].wait_stream(self.stream[q])       # q's copies of its states were made on q's stream
            with torch.cuda.stream(self.stream[r]):
                self.pos[r][q].copy_(self.hist[q][e])
                if fault is not None and fault[1:] == (r, q):
                    lo, hi = self.bounds[q]
                    k, rows = ec.faulty_view(fault[0], e, n_evals, n_states, hi - lo)
                    if k != e:
                        self.pos[r][q][:, rows].copy_(self.hist[q][k][:, rows])

    def run(self, scheme, steps, G, fault=None, stale_energy=False):
        """Steps all ranks; fault = (class, reader, source) or None.  Returns (bodies, kinetic, potential); stale_energy: the
        energy sum's own exchange leaves the reader's copy of the source chunk as the fault class says."""
        torch, nbx = self.torch, self.nbx
        evals = ec._evaluations(steps, scheme)
        reader = fault[1] if fault else self.R - 1
        order = [r for r in range(self.R) if r != reader] + [reader]      # the reader last: an early copy exists by then
        for e, (hk, hd) in enumerate(evals):
            for ctx in self.ctx:
                ctx.compute_accel(nbx.SRC_LOCAL)
            for r in order:
                self._exchange(r, e, len(evals), e + 2 if hd else e + 1, fault if r == reader else None)
                self.ctx[r].compute_accel(nbx.SRC_REMOTE)
                if scheme == "kd":
                    self.ctx[r].kick_drift(ec.DT, G)
                else:
                    self.ctx[r].kick_drift2(hk * ec.DT, hd * ec.DT, G)
                if hd:
                    with torch.cuda.stream(self.stream[r]):
                        self.hist[r].append(self.pos[r][r].clone())
        ke = pe = 0.0
        for r in range(self.R):
            self._exchange(r, steps, steps + 1, steps + 1, fault if (stale_energy and r == reader) else None)
            a, p = self.ctx[r].energy(G)
            ke, pe = ke + a, pe + p
        got = np.array(self.b)
        for ctx in self.ctx:
            ctx.download(got)
        torch.cuda.synchronize()
        return got, ke, pe



def main(jobs_path, results_path):
    import torch
    torch.zeros(1, device="cuda:0")                          # torch first, then the library (see the module docstring)
    import nbody_amd as nbx
    nbx.load_library()
    with open(jobs_path) as f:
        jobs = json.load(f)
    cache, out = {}, []
    for name, scheme, fault, stale_energy in jobs:
        c = ec.CASES[name]
        if (name, scheme) not in cache:
            b = ec.case_bodies(name)
            G = ec.G_REFERENCE * c["gscale"]
            cache[(name, scheme)] = (b, ec.trajectory_spec(b, c["dim"], c["steps"], ec.DT, G, scheme, c["law"], c["eps"]), G)
        b, states, G = cache[(name, scheme)]
        ranks = HandRanks(nbx, b, c)
        try:
            got, ke, pe = ranks.run(scheme, c["steps"], G, tuple(fault) if fault else None, stale_energy)
        finally:
            ranks.close()
        assert np.isfinite(got).all() and np.isfinite([ke, pe]).all(), (name, scheme, fault)
        _, dv, dx = ratios(got, states, c["dim"], c["steps"])
        rke, rpe = energy_ratios(ke, pe, got, c, G)
        out.append({"dv": dv, "dx": dx, "rke": rke, "rpe": rpe})
    with open(results_path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
