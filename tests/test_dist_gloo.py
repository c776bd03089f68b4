"""CPU: the N>1 path (nbody-simulation-parallel_amd/dist.py + sharding.py) over gloo, world_size 2
and 3, with the numpy shard double in place of the HIP back end.  Checks the shard partition, the
exchange/compute ordering (a stale remote chunk would show at once: G is scaled so forces bend the
orbits), ragged last shards, and that the gathered state equals the oracle's leapfrog."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n, dim, steps, dt, gscale, outdir, case="generated"):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import nbody_amd
        from cpu_shard_double import CpuShardDouble
        from oracle_lib import Oracle
        o = Oracle()
        if case == "generated":
            bodies = o.round_inputs_to_f32(o.generate(77, n, dim))
        else:
            from exchange_case import bodies_by_name
            bodies = bodies_by_name(case, n, dim, world, 77)  # by name: "moving_pairs" (tests/exchange_case.py)
        pkg = nbody_amd.package
        layout = pkg.sharding.ShardLayout(n_total=n, n_shards=world, shard=rank, dim=dim)
        be = CpuShardDouble(bodies, layout)
        sysm = pkg.dist.ShardedNBody(be, layout)
        # exchange self-check (what bench.py --gpus N runs first on a multi-GPU node): clean pass, then a
        # deliberately broken transport must be caught
        clean = sysm.verify_exchange(bodies)
        real_start = be.start_exchange
        be.start_exchange = lambda group: None           # a collective that delivers nothing
        broken = sysm.verify_exchange(bodies)
        be.start_exchange = real_start
        assert sysm.verify_exchange(bodies) == 0           # and the buffers are whole again
        # a collective that RAISES on one rank only: every rank must still meet in the bookkeeping (through the rendezvous
        # store, a transport of its own) and every rank must end with ExchangeError -- nobody retries on a communicator that may be wedged
        raised = 0
        if world > 1:
            sysc = pkg.dist.ShardedNBody(be, layout, check_store=dist.distributed_c10d._get_default_store())
            real_finish = be.finish_exchange

            def finish_raising_on_rank0(work):
                real_finish(work)
                if rank == 0:
                    raise RuntimeError("injected: the collective reported an error on this rank")
            be.finish_exchange = finish_raising_on_rank0
            try:
                sysc.verify_exchange(bodies)
            except pkg.dist.ExchangeError:
                raised = 1
            be.finish_exchange = real_finish
            assert sysc.verify_exchange(bodies) == 0
        del be.calls[:]
        sysm.compute_forces()
        f0 = sysm.forces(o.G * gscale)
        sysm.step(dt, o.G * gscale, steps)
        final = sysm.gather_bodies(bodies)
        ncalls = len(be.calls)
        ke, pe = sysm.energy(o.G * gscale)
        # kick-drift-kick form from the same state, on a copy of the back end's state
        be2 = CpuShardDouble(bodies, layout)
        sys2 = pkg.dist.ShardedNBody(be2, layout)
        sys2.step_kdk(dt, o.G * gscale, steps)
        final_kdk = sys2.gather_bodies(bodies)
        lo, hi = layout.bounds()
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), f0=f0, final=final, lo=lo, hi=hi, calls=np.array(be.calls[:ncalls]),
                 energy=np.array([ke, pe]), verify=np.array([clean, broken, raised]), final_kdk=final_kdk)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,dim,case", [(2, 300, 3, "generated"), (3, 301, 2, "generated"), (2, 1, 3, "generated"),
                                              (2, 300, 3, "moving_pairs"), (3, 301, 2, "moving_pairs")],
                         ids=["2-300-3", "3-301-2", "2-1-3", "2-300-3-moving_pairs", "3-301-2-moving_pairs"])
def test_sharded_steps_match_oracle(tmp_path, oracle, world, n, dim, case):
    import nbody_amd  # noqa: F401  (fails early if the package is broken)
    steps, dt, gscale = 4, 2.0, 1e24
    mp.spawn(_worker, args=(world, _free_port(), n, dim, steps, dt, gscale, str(tmp_path), case), nprocs=world, join=True)
    if case == "generated":
        bodies = oracle.round_inputs_to_f32(oracle.generate(77, n, dim))
    else:
        from exchange_case import bodies_by_name
        bodies = bodies_by_name(case, n, dim, world, 77)
    ref_f0 = oracle.brute_force_seq(bodies) * gscale
    # host loop from the oracle's leaves, forces taken on the fp32-rounded positions like the device path
    ref = bodies.copy()
    for _ in range(steps):
        f = oracle.brute_force_seq(oracle.round_inputs_to_f32(ref)) * gscale
        oracle.update_body_velocities(ref, np.ascontiguousarray(f), dt)
        oracle.update_body_positions(ref, dt)
    scale = np.abs(ref_f0).max() if n > 1 else 1.0
    finals = []
    for r in range(world):
        z = np.load(os.path.join(tmp_path, f"rank{r}.npz"))
        lo, hi = int(z["lo"]), int(z["hi"])
        assert z["f0"].shape == (hi - lo, dim)
        if hi > lo:
            assert np.abs(z["f0"] - ref_f0[lo:hi]).max() <= 1e-9 * max(scale, 1e-300)
        finals.append(z["final"])
        others = n - (hi - lo)
        assert z["verify"][0] == 0 and (z["verify"][1] == dim * (world * n - n) if world > 1 else z["verify"][1] == 0), z["verify"]
        assert z["verify"][2] == (1 if world > 1 else 0), "an exchange that raises on one rank must raise ExchangeError on every rank"
        calls = list(z["calls"])
        per = ["exchange", "local", "remote"] if world > 1 else ["exchange", "local"]
        assert calls == per + (per + ["kick_drift"]) * steps, "exchange must precede the local pass every step"
    for fin in finals[1:]:
        assert np.array_equal(fin, finals[0]), "every rank must assemble the same state"
    # whole-system energy, identical on every rank, equals the oracle's on the final state
    if n > 1:
        fin32 = oracle.round_inputs_to_f32(finals[0])
        fin32[:, dim:2 * dim] = finals[0][:, dim:2 * dim]
        ke_ref, pe_ref = oracle.energy(fin32)
        for r in range(world):
            e = np.load(os.path.join(tmp_path, f"rank{r}.npz"))["energy"]
            assert abs(e[0] - ke_ref) <= 1e-12 * abs(ke_ref) and abs(e[1] - pe_ref * gscale) <= 1e-9 * abs(pe_ref * gscale)
    # kick-drift-kick: the oracle's helpers composed the same way (half kick, drift, force, half kick)
    kref = bodies.copy()
    for _ in range(steps):
        f = oracle.brute_force_seq(oracle.round_inputs_to_f32(kref)) * gscale
        oracle.update_body_velocities(kref, np.ascontiguousarray(f), dt / 2)
        oracle.update_body_positions(kref, dt)
        f = oracle.brute_force_seq(oracle.round_inputs_to_f32(kref)) * gscale
        oracle.update_body_velocities(kref, np.ascontiguousarray(f), dt / 2)
    kd = np.load(os.path.join(tmp_path, "rank0.npz"))["final_kdk"]
    if n > 1:
        dvk = np.abs(kref[:, dim:2 * dim] - bodies[:, dim:2 * dim]).max()
        assert np.allclose(kd[:, dim:2 * dim], kref[:, dim:2 * dim], rtol=0, atol=1e-7 * dvk)   # merged half-kicks: (a+b)*dt vs a*dt/2+b*dt/2
    assert np.allclose(kd[:, :dim], kref[:, :dim], rtol=1e-12, atol=0)
    d = dim
    if n > 1:
        moved = np.abs(ref[:, d:2 * d] - bodies[:, d:2 * d]).max()
        assert moved > 1e-6, "coupling too weak to move the bodies measurably"
        assert np.allclose(finals[0][:, d:2 * d], ref[:, d:2 * d], rtol=0, atol=1e-7 * moved)
    assert np.allclose(finals[0][:, :d], ref[:, :d], rtol=1e-12, atol=0)
    assert np.array_equal(finals[0][:, -1], bodies[:, -1])


def test_shard_layout_logic():
    import nbody_amd
    SL = nbody_amd.package.sharding.ShardLayout
    L = SL(n_total=1 << 20, n_shards=8, shard=3, dim=3)
    assert L.shard_len == 131072 and L.shard_pad == 131072 and L.bounds() == (393216, 524288) and L.count == 131072
    assert L.pos_all_shape() == (8, 3, 131072) and L.interactions_per_step() == 131072 * (1 << 20)
    R = SL(n_total=10, n_shards=4, shard=3, dim=2)       # ragged: shards of 3,3,3,1
    assert R.shard_len == 3 and R.shard_pad == 4096 and R.bounds() == (9, 10) and R.count == 1
    E = SL(n_total=2, n_shards=4, shard=3, dim=2)        # more ranks than bodies
    assert E.count == 0 and E.bounds() == (2, 2)
    assert sum(SL(1001, 7, g, 3).count for g in range(7)) == 1001
    for bad in (dict(n_total=4, n_shards=0, shard=0, dim=3), dict(n_total=4, n_shards=2, shard=2, dim=3),
                dict(n_total=4, n_shards=1, shard=0, dim=4)):
        with pytest.raises(ValueError):
            SL(**bad)
