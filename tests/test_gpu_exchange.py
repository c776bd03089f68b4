"""GPU: multi-rank stepping on an input that cannot hide a stale position exchange (tests/exchange_case.py; the certificate
is asserted in tests/test_exchange_case_cpu.py): one rank reading another rank's chunk one step late, one step early, never
refreshed, or late in its first or last 64 rows misses the tolerances below by a factor of 100 or more, for every pair of ranks.

 (a) nbx_node_step / nbx_node_step_kdk / nbx_node_energy on virtual ranks of device 0, against the fp64 specification;
 (b) the same step loops driven by hand over plain sharded contexts (LOCAL pass, exchange, REMOTE pass, kick / drift), the
     exchange being this file's own torch copies: the right schedule passes (a)'s checks, and a reader handed a wrong copy of
     one chunk -- valid positions of another step, nothing else -- fails them by the factor the certificate predicts.

Tolerances (the multi-rank tests' own): velocities atol 3e-5 * moved, positions rtol 1e-9 + 3e-5 * moved * dt * steps,
kinetic energy 1e-12 and potential energy 3e-6 relative; kick-drift-kick node against a single context 2e-5 * dv."""
import functools

import numpy as np
import pytest

import exchange_case as ec
from exchange_hand_ranks import energy_ratios as _energy_ratios, ratios as _ratios, set_law as _set_law

pytestmark = pytest.mark.gpu
FLOOR = 100.0


@functools.lru_cache(maxsize=None)
def _case(name, scheme):
    """(bodies, states of the specification, G) of a shared case, computed once."""
    c = ec.CASES[name]
    b = ec.case_bodies(name)
    G = ec.G_REFERENCE * c["gscale"]
    states = ec.trajectory_spec(b, c["dim"], c["steps"], ec.DT, G, scheme, c["law"], c["eps"])
    for s in states:
        s.setflags(write=False)
    b.setflags(write=False)
    return b, states, G


# ---- (a) the node layer ------------------------------------------------------------------------------------------------

NODE_CASES = [(name, scheme, None) for name in ("r2", "r3_2d", "r8", "r4_short", "softened", "newton") for scheme in ("kd", "kdk")]
NODE_CASES += [("r3_2d", "kd", 0.0), ("r3_2d", "kdk", 0.0)]      # plain fp32 beside the default mixed mode (refine 1e-5)


@pytest.mark.parametrize("name,scheme,refine", NODE_CASES)
def test_node_steps_match_the_specification(nbx, name, scheme, refine):
    c = ec.CASES[name]
    n, dim, ranks, steps = c["n"], c["dim"], c["ranks"], c["steps"]
    b, states, G = _case(name, scheme)
    with nbx.Node(n, dim, [0] * ranks) as node:
        node.upload(np.array(b))
        _set_law(node, nbx, c)
        if refine is not None:
            node.set_refine(refine)
        assert node.verify_exchange() == 0
        getattr(node, "step" if scheme == "kd" else "step_kdk")(ec.DT, steps, G)
        got = np.array(b)
        node.download(got)
        ke, pe = node.energy(G)
    moved, dv, dx = _ratios(got, states, dim, steps)
    rke, rpe = _energy_ratios(ke, pe, got, c, G)
    print(f"\nnode {name} {scheme} refine={refine}: moved {moved:.4g}; error / tolerance: velocity {dv:.3g}, position {dx:.3g}, "
          f"kinetic {rke:.3g}, potential {rpe:.3g}")
    assert dv <= 1.0 and dx <= 1.0
    assert rke <= 1.0 and rpe <= 1.0
    assert np.array_equal(got[:, -1], b[:, -1])
    if scheme == "kdk":                                      # LOCAL + REMOTE sums on the ranks against one ALL sum
        one = np.array(b)
        with nbx.Context(n, dim) as ctx:
            ctx.upload(np.array(b))
            _set_law(ctx, nbx, c)
            if refine is not None:
                ctx.set_refine(refine)
            ctx.step_kdk(ec.DT, steps, G)
            ctx.download(one)
        dvk = np.abs(one[:, dim:2 * dim] - b[:, dim:2 * dim]).max()
        assert np.allclose(got[:, dim:2 * dim], one[:, dim:2 * dim], rtol=0, atol=2e-5 * dvk)
        assert np.allclose(got[:, :dim], one[:, :dim], rtol=1e-9, atol=2e-5 * dvk * ec.DT * steps)


# ---- (b) ranks driven by hand ------------------------------------------------------------------------------------------

RIGHT = [("r2", "kd"), ("r2", "kdk"), ("r3_2d", "kd"), ("r3_2d", "kdk"), ("r4_short", "kd"), ("r4_short", "kdk"),
         ("softened", "kd"), ("newton", "kdk")]
WRONG = [("r2", "kd"), ("r3_2d", "kd"), ("r3_2d", "kdk")]


def _fault_jobs(name, scheme):
    R = ec.CASES[name]["ranks"]
    return [(name, scheme, (f, r, q), f == "late") for r, q in ((0, R - 1), (R - 1, 0)) for f in ec.FAULTS]


@pytest.fixture(scope="module")
def hand_results(nbx, tmp_path_factory):
    """Every hand-driven run of this file, in ONE child process (tests/exchange_hand_ranks.py says why a child): the right
    schedule on RIGHT, and on WRONG every fault class at (reader, source) = (0, R - 1) and (R - 1, 0)."""
    import json
    import os
    import subprocess
    import sys
    jobs = [(name, scheme, None, False) for name, scheme in RIGHT]
    for name, scheme in WRONG:
        jobs += _fault_jobs(name, scheme)
    d = tmp_path_factory.mktemp("hand_ranks")
    with open(d / "jobs.json", "w") as f:
        json.dump(jobs, f)
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "exchange_hand_ranks.py")
    p = subprocess.run([sys.executable, helper, str(d / "jobs.json"), str(d / "results.json")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with open(d / "results.json") as f:
        res = json.load(f)
    return {(j[0], j[1], j[2]): r for j, r in zip(jobs, res)}


@pytest.mark.parametrize("name,scheme", RIGHT)
def test_hand_driven_ranks_with_the_right_schedule_match_the_specification(hand_results, name, scheme):
    """LOCAL pass, exchange, REMOTE pass, kick / drift on plain sharded contexts -- the one-process-per-rank data flow without
    torch.distributed; kick-drift-kick over LOCAL + REMOTE has no other test."""
    r = hand_results[(name, scheme, None)]
    dv, dx, rke, rpe = r["dv"], r["dx"], r["rke"], r["rpe"]
    print(f"\nhand-driven {name} {scheme}: error / tolerance: velocity {dv:.3g}, position {dx:.3g}, kinetic {rke:.3g}, potential {rpe:.3g}")
    assert dv <= 1.0 and dx <= 1.0 and rke <= 1.0 and rpe <= 1.0


@pytest.mark.parametrize("name,scheme", WRONG)
def test_a_wrong_copy_of_one_chunk_fails_the_checks_by_the_certified_factor(hand_results, name, scheme):
    """The checks above CAN fail: for every fault class, at (reader, source) = (0, R - 1) and (R - 1, 0), the reader is handed
    a wrong copy of the source's chunk (valid positions of another step, inside this test's own buffers).  Each run misses the
    velocity tolerance by >= 100 tolerances, the late run the potential energy's as well -- beside what the certificate predicts
    (the certificate steps the reader's planted rows only and leaves everything else exact: a lower bound, usually close)."""
    c = ec.CASES[name]
    R = c["ranks"]
    predicted = ec.case_margins(name, scheme)
    print(f"\nwrong copies, {name} {scheme}: observed error / tolerance (certificate's prediction)")
    for r, q in ((0, R - 1), (R - 1, 0)):
        for f in ec.FAULTS:
            res = hand_results[(name, scheme, (f, r, q))]
            dv, dx, rpe = res["dv"], res["dx"], res["rpe"]
            pv, px, ppe = predicted[f]["pairs"][(r, q)]
            line = f"    {f:10s} reader {r} source {q}: velocity {dv:9.0f} ({pv:9.0f})  position {dx:9.0f} ({px:9.0f})"
            if f == "late":
                line += f"  potential energy {rpe:9.0f} ({ppe:9.0f})"
            print(line)
            assert dv >= FLOOR, (f, r, q, dv)
            assert pv >= FLOOR, (f, r, q, pv)
            if f == "late":
                assert rpe >= FLOOR and ppe >= FLOOR, (f, r, q, rpe, ppe)
