"""TEST INFRASTRUCTURE (plain numpy: no device, no oracle library): an input on which a stale position exchange between
ranks cannot hide, the fp64 specification of the step loops, and the certificate that says so.

moving_pairs      generated bodies with planted groups.  Row 0 and row count - 1 of every non-empty shard q become MOVERS
                  (mass 4e7, speed 300); behind each mover, at rest, stands one PROBE (mass 2.25e6) of every other shard r,
                  2,100 away at first and 3,600 after four steps of dt = 2.  The force on r's probe therefore depends strongly
                  on WHERE q's first (last) row is believed to be: a copy of q's chunk that is one step old, one step ahead,
                  never refreshed, or old in its first or last rows only changes that distance by 13 % or more -- for every
                  ordered pair (r, q).
trajectory_spec   kick-drift and kick-drift-kick in fp64 with the sources rounded to fp32 every evaluation, as the device holds
                  them; the reference law, the softened law and the softened Newtonian law.
fault_margins     for every ordered pair (r, q) and every fault class (FAULTS): by how many tolerances a run in which rank r
                  reads q's chunk as the fault says misses the project's checks.  A certificate >= 100 is a property of the
                  INPUT, established from the specification alone; the GPU tests then run on such inputs only.

The tolerances are the ones the multi-rank tests use: velocities atol = 3e-5 * moved (moved = the largest velocity change of
the run), positions rtol 1e-9 + 3e-5 * moved * dt * steps, potential energy 3e-6 relative.
"""
import numpy as np

import nbody_amd

R2_SKIP = 1e-10                      # the reference law's skip threshold (methods.cpp:24)
FAULTS = ("late", "early", "frozen", "late_last", "late_head", "late_tail")
EDGE_ROWS = 64                       # late_head / late_tail: the first / last rows of the chunk that arrive one step late
VEL_TOL, POS_RTOL, PE_TOL = 3e-5, 1e-9, 3e-6
MOVER_MASS, PROBE_MASS = 4.0e7, 2.25e6
PLANTED_SEP = 2000.0                 # the unit of a group's geometry (_probe_offsets): the least distance between two of its probes
PLANTED_SPEED = 300.0                # of a mover: 600 = 0.3 units per step at dt = 2
GROUP_LO, GROUP_HI = 36000.0, 124000.0    # group centres, per coordinate: above kCloseCoord (16384); fp32 spacing there 2^-7
GROUP_MIN_DISTANCE = 30000.0              # movers of two groups: far enough that their mutual energy does not answer to a late copy


def shard_bounds(n, ranks):
    """[(lo, hi)] per rank: ShardLayout's contiguous split, shard_len = ceil(n / ranks)."""
    sl = -(-n // ranks)
    return [(min(n, g * sl), min(n, g * sl + sl)) for g in range(ranks)]


def live_shards(n, ranks):
    return [g for g, (lo, hi) in enumerate(shard_bounds(n, ranks)) if hi > lo]


def ordered_pairs(n, ranks):
    """Every ordered pair (reader r, source q) of non-empty shards."""
    live = live_shards(n, ranks)
    return [(r, q) for r in live for q in live if r != q]


def _probe_offsets(dim):
    """Where the probes stand BEHIND a mover, in units of PLANTED_SEP (first component: along the mover's velocity): one unit
    off the axis and 0.3 units behind, and one on the axis a whole unit behind.  The mover leaves them at 0.3 units per
    step: every mover-probe distance grows monotonically, so a copy of the mover's place that is old looks nearer and one
    that is early looks farther, by 13 % or more per step at the end.  The probes, pushed by the mover, drift backwards and
    apart: an old copy of a PROBE also looks nearer to everything in its group -- every term of the energy sum errs one way."""
    if dim == 2:
        return np.array([(-0.3, 1.0), (-0.3, -1.0), (-1.0, 0.0)])
    return np.array([(-0.3, np.cos(np.pi * j / 3.0), np.sin(np.pi * j / 3.0)) for j in range(6)] + [(-1.0, 0.0, 0.0)])


def planted_layout(n, dim, ranks):
    """Where moving_pairs plants: {'movers': [(row, shard)], 'probes': [(row, reader shard, mover row)]}.  With k non-empty
    shards every shard hosts 2 movers (its first and last row) and 2 (k - 1) probes (rows spread between them): 2 k rows.  A
    shard too short for that, or more shards than the probe directions allow, is refused: such a case certifies nothing."""
    bounds, live = shard_bounds(n, ranks), live_shards(n, ranks)
    k = len(live)
    if k < 2:
        return {"movers": [], "probes": []}
    if k - 1 > len(_probe_offsets(dim)):
        raise ValueError(f"moving_pairs: {k} shards need {k - 1} probes behind a mover; {dim}D has room for {len(_probe_offsets(dim))}")
    per = 2 * (k - 1)
    movers, probes, used = [], [], {g: 0 for g in live}
    for g in live:
        lo, hi = bounds[g]
        if hi - lo < 2 + per:
            raise ValueError(f"moving_pairs: shard {g} has {hi - lo} rows, fewer than the {2 + per} planted ones (n={n}, ranks={ranks})")
    for q in live:
        for row in (bounds[q][0], bounds[q][1] - 1):
            movers.append((row, q))
            for r in live:
                if r != q:
                    lo, hi = bounds[r]       # between the first and last EDGE_ROWS rows where the shard is long enough for that
                    edge = EDGE_ROWS if hi - lo - 2 * EDGE_ROWS >= per else 1
                    probes.append((lo + edge + (used[r] * (hi - lo - 2 * edge)) // per, r, row))
                    used[r] += 1
    return {"movers": movers, "probes": probes}


def planted_rows(n, dim, ranks):
    lay = planted_layout(n, dim, ranks)
    return sorted([m[0] for m in lay["movers"]] + [p[0] for p in lay["probes"]])


def moving_pairs(n, dim, ranks, seed, background_mass=1.0):
    """float64 [n, 2 dim + 1] bodies: uniform_bodies(n, dim, seed) with positions and masses rounded to fp32 and the rows of
    planted_layout replaced (see the module docstring); every planted coordinate, velocity and mass is an fp32 number.
    background_mass scales the generated masses: under the Newtonian law the potential falls off as 1/r and the sum over
    the generated pairs, millions of units apart, would bury any group's share of it (the tests use 0.05 there)."""
    b = nbody_amd.uniform_bodies(n, dim, seed)
    b[:, -1] *= background_mass
    b[:, :dim] = b[:, :dim].astype(np.float32)
    b[:, -1] = b[:, -1].astype(np.float32)
    lay = planted_layout(n, dim, ranks)
    rng = np.random.default_rng(1000003 * seed + 7919 * ranks + n)
    offs = _probe_offsets(dim)
    centres = []
    for row, q in lay["movers"]:
        apart, tries = GROUP_MIN_DISTANCE, 0
        while True:
            c = rng.uniform(GROUP_LO, GROUP_HI, size=dim)
            if all(np.sqrt(((c - o) ** 2).sum()) >= apart for o in centres):
                break
            tries += 1
            if tries % 500 == 0:
                apart *= 0.9                                  # a crowded box: settle for less (the certificate decides anyway)
        centres.append(c)
        frame, _ = np.linalg.qr(rng.normal(size=(dim, dim)))   # columns: the velocity's direction, then the rest of the frame
        vel = (PLANTED_SPEED * frame[:, 0]).astype(np.float32)
        mine = [p for p in lay["probes"] if p[2] == row]
        b[row, :dim] = c.astype(np.float32)
        b[row, dim:2 * dim] = vel
        b[row, -1] = MOVER_MASS
        for j, (prow, _, _) in enumerate(mine):
            b[prow, :dim] = (c + PLANTED_SEP * (frame @ offs[j])).astype(np.float32)
            b[prow, dim:2 * dim] = 0.0
            b[prow, -1] = PROBE_MASS
    return b


# ---- the specification -------------------------------------------------------------------------------------------------

def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _accel(tx, sx, sm, law, eps, block=256):
    """sum_j m_j (s_j - t_i) w(r^2) for every target row, fp64, in row blocks.  w = 1/r^4 with the reference's skip
    (law 'reference'), 1/(r^2+eps^2)^2 ('softened'), 1/(r^2+eps^2)^(3/2) ('newton'; the caller flips the sign)."""
    out = np.zeros_like(tx)
    e2 = eps * eps
    for i in range(0, tx.shape[0], block):
        d = sx[None, :, :] - tx[i:i + block, None, :]
        r2 = (d ** 2).sum(-1)
        if law == "reference":
            ok = r2 >= R2_SKIP
            w = np.where(ok, sm[None, :] / np.where(ok, r2, 1.0) ** 2, 0.0)
        elif law == "softened":
            w = sm[None, :] / (r2 + e2) ** 2
        elif law == "newton":
            w = np.where(r2 > 0.0, sm[None, :] / (r2 + e2) ** 1.5, 0.0)
        else:
            raise ValueError(law)
        out[i:i + block] = (w[:, :, None] * d).sum(1)
    return out


def _phi(tx, sx, sm, law, eps, block=256):
    """sum_j m_j u(r^2) per target: u = 1/r^2 (skip below R2_SKIP), 1/(r^2+eps^2), or 1/sqrt(r^2+eps^2) without the self term."""
    out = np.zeros(tx.shape[0])
    e2 = eps * eps
    for i in range(0, tx.shape[0], block):
        r2 = ((sx[None, :, :] - tx[i:i + block, None, :]) ** 2).sum(-1)
        if law == "reference":
            ok = r2 >= R2_SKIP
            u = np.where(ok, 1.0 / np.where(ok, r2, 1.0), 0.0)
        elif law == "softened":
            u = np.where(r2 > 0.0, 1.0 / (r2 + e2), 0.0)    # (self term out; distinct coincident bodies are not in these inputs)
        else:
            u = np.where(r2 > 0.0, 1.0 / np.sqrt(r2 + e2), 0.0)
        out[i:i + block] = (u * sm[None, :]).sum(1)
    return out


def _sign(law):
    return 1.0 if law == "newton" else -1.0                 # F_i = sign * G m_i * _accel


def _evaluations(steps, scheme):
    """(kick dt factor, drift dt factor) of every force evaluation: kick-drift has `steps`, kick-drift-kick `steps + 1`
    (opening half kick, merged full kicks, closing half kick without a drift)."""
    if scheme == "kd":
        return [(1.0, 1.0)] * steps
    if scheme == "kdk":
        return [(0.5 if e in (0, steps) else 1.0, 1.0 if e < steps else 0.0) for e in range(steps + 1)] if steps > 0 else []
    raise ValueError(scheme)


def trajectory_spec(b, dim, steps, dt, G, scheme="kd", law="reference", eps=0.0):
    """[steps + 1] states (bodies arrays; [0] is the input): x and v in fp64, every force from the positions and masses
    rounded to fp32.  'kd': v += (F/m) dt; x += v dt.  'kdk': v += (F/m) dt/2; x += v dt; v += (F'/m) dt/2."""
    cur = np.array(b, dtype=np.float64)
    m32 = _f32(cur[:, -1])
    states = [cur.copy()]
    s = _sign(law)

    def kick(h):
        x32 = _f32(cur[:, :dim])
        F = (s * G * cur[:, -1])[:, None] * _accel(x32, x32, m32, law, eps)
        cur[:, dim:2 * dim] += (F / cur[:, -1][:, None]) * h

    for _ in range(steps):
        if scheme == "kd":
            kick(dt)
            cur[:, :dim] += cur[:, dim:2 * dim] * dt
        elif scheme == "kdk":
            kick(0.5 * dt)
            cur[:, :dim] += cur[:, dim:2 * dim] * dt
            kick(0.5 * dt)
        else:
            raise ValueError(scheme)
        states.append(cur.copy())
    return states


def energy_spec(state, dim, G, law="reference", eps=0.0):
    """(kinetic, potential) of a state as the device defines it: positions and masses rounded to fp32, velocities and the
    masses of the prefactors in fp64.  U = sum_{i<j} G m m / (2 r^2) (reference, softened) or -sum G m m / sqrt(r^2+eps^2)."""
    x32, m32 = _f32(state[:, :dim]), _f32(state[:, -1])
    m = state[:, -1]
    ke = float((0.5 * m * (state[:, dim:2 * dim] ** 2).sum(1)).sum())
    phi = _phi(x32, x32, m32, law, eps)
    pe = float((m * phi).sum()) * (-0.5 * G if law == "newton" else 0.25 * G)
    return ke, pe


def moved_of(states, dim):
    return float(np.abs(states[-1][:, dim:2 * dim] - states[0][:, dim:2 * dim]).max())


# ---- the certificate ---------------------------------------------------------------------------------------------------

def faulty_view(fault, e, n_evals, n_states, rows):
    """What a reader holds of a source chunk of `rows` rows at evaluation e (of n_evals) under `fault`, state e being the
    correct answer and n_states states existing (early: no state further on, no hazard).  Returns (state index of the wrong
    rows, slice of the wrong rows); rows outside the slice are correct."""
    whole = slice(0, rows)
    if fault == "late":
        return (e - 1 if e >= 1 else e), whole
    if fault == "early":
        return (e + 1 if e + 1 < n_states else e), whole
    if fault == "frozen":
        return 0, whole
    if fault == "late_last":
        return (e - 1 if e == n_evals - 1 and e >= 1 else e), whole
    if fault == "late_head":
        return (e - 1 if e >= 1 else e), slice(0, min(EDGE_ROWS, rows))
    if fault == "late_tail":
        return (e - 1 if e >= 1 else e), slice(max(0, rows - EDGE_ROWS), rows)
    raise ValueError(fault)


def fault_margins(b, dim, ranks, steps, dt, G, scheme="kd", law="reference", eps=0.0, targets="planted", faults=FAULTS,
                  vel_tol=VEL_TOL):
    """For every fault class: the minimum over all ordered pairs (r, q) of non-empty shards of
         vel = max |dv| / (vel_tol * moved),   pos = max (|dx| / (POS_RTOL |x| + vel_tol * moved * dt * steps)),
         pe  = |dU| / (PE_TOL * |U|)
    of a run in which rank r reads q's chunk as the fault says and everything else is right.  Rank r's targets are stepped
    again from the input against the specification's stored positions (the other ranks see correct data, and the feedback
    through r's own displacement on them is second order); targets='planted' steps only r's planted rows -- the maximum over
    fewer bodies, a lower bound of the margin --, 'all' every row of the shard.  dU: the reader's share of the potential
    energy of the final state, summed with q's chunk as the fault leaves it (early: q one step further).
    Returns {fault: {'vel', 'pos', 'pe', 'pairs': {(r, q): (vel, pos, pe)}}} and, under 'moved' / 'pe_total', the scales."""
    n = b.shape[0]
    states = trajectory_spec(b, dim, steps + 1, dt, G, scheme, law, eps)      # one state further: the early class's future
    hist = [_f32(s[:, :dim]) for s in states]
    ref = states[steps]
    m32 = _f32(b[:, -1])
    moved = moved_of(states[:steps + 1], dim)
    pe_total = energy_spec(ref, dim, G, law, eps)[1]
    evals = _evaluations(steps, scheme)
    bounds = shard_bounds(n, ranks)
    planted = planted_rows(n, dim, ranks)
    sgn = _sign(law)
    pe_factor = -0.5 * G if law == "newton" else 0.25 * G
    out = {f: {"pairs": {}} for f in faults}
    for r, q in ordered_pairs(n, ranks):
        (rlo, rhi), (qlo, qhi) = bounds[r], bounds[q]
        if targets == "planted":
            rows = np.array([i for i in planted if rlo <= i < rhi], dtype=np.int64)
        else:
            rows = np.arange(rlo, rhi)
        m = b[rows, -1]
        for f in faults:
            x, v = b[rows, :dim].copy(), b[rows, dim:2 * dim].copy()
            for e, (hk, hd) in enumerate(evals):
                k, sl = faulty_view(f, e, len(evals), steps + 1, qhi - qlo)
                src = hist[e].copy()
                src[rows] = _f32(x)
                src[qlo:qhi][sl] = hist[k][qlo:qhi][sl]
                a = _accel(_f32(x), src, m32, law, eps)
                v += ((sgn * G * m)[:, None] * a / m[:, None]) * (hk * dt)
                x += v * (hd * dt)
            dv = np.abs(v - ref[rows, dim:2 * dim]).max()
            dx = (np.abs(x - ref[rows, :dim]) / (POS_RTOL * np.abs(ref[rows, :dim]) + vel_tol * moved * dt * steps)).max()
            # the energy sum of the final state with q's chunk as the fault leaves it in r's buffer
            k, sl = faulty_view(f, steps, steps + 1, steps + 2, qhi - qlo)
            all_r = np.arange(rlo, rhi)
            tx = hist[steps][all_r]
            good = _phi(tx, hist[steps][qlo:qhi][sl], m32[qlo:qhi][sl], law, eps)
            bad = _phi(tx, hist[k][qlo:qhi][sl], m32[qlo:qhi][sl], law, eps)
            dU = pe_factor * float((b[all_r, -1] * (bad - good)).sum())
            out[f]["pairs"][(r, q)] = (dv / (vel_tol * moved), dx, abs(dU) / (PE_TOL * abs(pe_total)))
    for f in faults:
        vals = np.array(list(out[f]["pairs"].values())).reshape(-1, 3)
        for j, key in enumerate(("vel", "pos", "pe")):
            out[f][key] = float(vals[:, j].min()) if vals.size else float("inf")
    out["moved"], out["pe_total"] = moved, pe_total
    return out


# ---- the cases the tests share ------------------------------------------------------------------------------------------

G_REFERENCE = 4.471e-21              # nbody-sim-new/utils.h:21
STEPS, DT = 4, 2.0
# name: ranks, n, dim, seed, steps, law, eps, G scale, background_mass.  The four shapes of tests/test_gpu_exchange.py (two
# ranks; three ranks in 2D with a ragged split; eight ranks; a last rank three rows short), the laws at one shape each, and
# the one-process-per-rank cases of tests/test_gpu_dist.py (three steps there) and tests/test_dist_gloo.py.
CASES = {
    "r2":        dict(ranks=2, n=1500, dim=3, seed=31, steps=STEPS, law="reference", eps=0.0, gscale=1e24, background_mass=1.0),
    "r3_2d":     dict(ranks=3, n=1027, dim=2, seed=31, steps=STEPS, law="reference", eps=0.0, gscale=1e24, background_mass=1.0),
    "r8":        dict(ranks=8, n=2053, dim=3, seed=31, steps=STEPS, law="reference", eps=0.0, gscale=1e24, background_mass=1.0),
    "r4_short":  dict(ranks=4, n=1021, dim=3, seed=31, steps=STEPS, law="reference", eps=0.0, gscale=1e24, background_mass=1.0),
    "softened":  dict(ranks=2, n=1500, dim=3, seed=31, steps=STEPS, law="softened", eps=500.0, gscale=1e24, background_mass=1.0),
    "newton":    dict(ranks=4, n=1021, dim=3, seed=31, steps=STEPS, law="newton", eps=500.0, gscale=4e20, background_mass=0.05),
    "dist2":     dict(ranks=2, n=1500, dim=3, seed=77, steps=3, law="reference", eps=0.0, gscale=1e24, background_mass=1.0),
    "dist3_2d":  dict(ranks=3, n=1027, dim=2, seed=77, steps=3, law="reference", eps=0.0, gscale=1e24, background_mass=1.0),
    "gloo2":     dict(ranks=2, n=300, dim=3, seed=77, steps=STEPS, law="reference", eps=0.0, gscale=1e24, background_mass=1.0),
    "gloo3_2d":  dict(ranks=3, n=301, dim=2, seed=77, steps=STEPS, law="reference", eps=0.0, gscale=1e24, background_mass=1.0),
}


def case_bodies(name):
    c = CASES[name]
    return moving_pairs(c["n"], c["dim"], c["ranks"], c["seed"], c["background_mass"])


def case_margins(name, scheme, **kw):
    c = CASES[name]
    return fault_margins(case_bodies(name), c["dim"], c["ranks"], c["steps"], DT, G_REFERENCE * c["gscale"], scheme, c["law"], c["eps"], **kw)


def bodies_by_name(name, n, dim, ranks, seed):
    """Inputs of the one-process-per-rank workers, by name (spawn arguments stay picklable and small)."""
    if name == "moving_pairs":
        return moving_pairs(n, dim, ranks, seed)
    if name == "generated":
        b = nbody_amd.uniform_bodies(n, dim, seed)
        b[:, :dim] = b[:, :dim].astype(np.float32)
        b[:, -1] = b[:, -1].astype(np.float32)
        return b
    raise ValueError(name)
