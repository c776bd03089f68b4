"""Kick-drift-kick with block (hierarchical) time steps: the fp64 numpy specification of nbx_ctx_step_kdk_block (include/nbody_hip.h
has the rule), next to leaves.leapfrog_spec and adaptive_leapfrog_spec.

Body i steps by dt_max / 2^level_i.  Every body drifts on the smallest step present; accelerations are computed only for the bodies
whose own step ends (the active ones), from ALL bodies' current positions.  Time is counted in ticks of dt_max / 2^L, so every
comparison of times is an integer one."""
import numpy as np


def want_level(a, accel_length: float, dt_max: float, levels: int):
    """(w, margin) of one body's choice.  raw = sqrt(accel_length / a), +inf when a == 0; w = 0; d = dt_max; while d > raw and w <
    levels: d = 0.5 d, w += 1 -- the per-body form of leaves.choose_step's pow2 choice.  margin = min over j = 0 .. levels of
    |raw / (dt_max 2^-j) - 1| (inf when raw is): how far the choice is from flipping."""
    a, c, d = np.float64(a), np.float64(accel_length), np.float64(dt_max)
    raw = np.float64(np.inf) if a == 0.0 else np.sqrt(c / a)
    w = 0
    while d > raw and w < levels:
        d = np.float64(0.5) * d
        w += 1
    if not np.isfinite(raw):
        return w, np.inf
    steps = np.float64(dt_max) * np.float64(2.0) ** -np.arange(levels + 1, dtype=np.float64)
    return w, float(np.abs(raw / steps - 1.0).min())


def block_leapfrog_spec(bodies: np.ndarray, accel_rows_fn, control: dict, n_blocks: int, max_substeps: int):
    """nbx_ctx_step_kdk_block in fp64 numpy.  bodies: Body<D> rows (position[D], velocity[D], mass); accel_rows_fn(rows, active) ->
    a[len(active), D], the accelerations F_i / m_i (G and sign included) of the bodies `active` (ascending indices) from all rows as
    they stand; control: a dict with accel_length, dt_max, levels and optionally t_start (0).  Returns (rows, clock, history, levels,
    margin): the new rows; clock, a dict with the fields of nbx_block_clock; history, an integer array [k, 2] of the recorded
    (n_active, dn); the bodies' final levels; margin, the smallest |raw / (dt_max 2^-j) - 1| over every choice made.
        T = 0; all active
        for every evaluation:  any |a_i| not finite -> status 1, stop, no kick
                               active i: first evaluation: new = want, kick = 0.5 dt_new
                                         later: new = want if deeper; one level up if want is higher and T % 2^(L-old+1) == 0; else old
                                                (at T_end: old); kick = 0.5 dt_old + (0 at T_end, else 0.5 dt_new)
                                         v_i += a_i kick
                               record (n_active, dn); T == T_end -> finished, stop; substeps == max_substeps -> status 2, stop
                               dn = 2^(L - deepest level present); x += v (dn tick) for all; T += dn"""
    c, dt_max, L = float(control["accel_length"]), float(control["dt_max"]), int(control["levels"])
    t_start = float(control.get("t_start", 0.0))
    if not (c > 0 and np.isfinite(c) and dt_max > 0 and np.isfinite(dt_max) and np.isfinite(t_start) and 0 <= L <= 20):
        raise ValueError("control outside the ranges of nbx_block_control")
    if n_blocks < 0 or not 0 <= max_substeps <= 1 << 20:
        raise ValueError("n_blocks must be >= 0 and max_substeps in [0, 1 << 20]")
    b = np.array(bodies, dtype=np.float64, copy=True)
    n = b.shape[0]
    dim = (b.shape[1] - 1) // 2
    x, v = b[:, :dim], b[:, dim:2 * dim]
    level = np.zeros(n, dtype=np.int32)
    clock = {"t": t_start, "ticks": 0, "pair_terms": 0, "substeps": 0, "evaluations": 0, "deepest_level": 0, "finished": 0, "status": 0}
    history, margin = [], np.inf
    if n_blocks == 0:
        return b, clock, np.zeros((0, 2), dtype=np.int64), level, margin
    half = np.float64(0.5)
    step_of = np.float64(dt_max) * np.float64(2.0) ** -np.arange(L + 1, dtype=np.float64)   # dt_l, exact
    tick = step_of[L]
    T, T_end, first = 0, n_blocks << L, True
    active = np.arange(n)
    while True:
        a = np.asarray(accel_rows_fn(b, active), dtype=np.float64).reshape(active.size, dim)
        mag = np.sqrt((a * a).sum(axis=1))
        clock["evaluations"] += 1
        if not np.isfinite(mag).all():
            clock["status"] = 1
            break
        closing = T == T_end
        kick = np.empty(active.size, dtype=np.float64)
        for r, i in enumerate(active):
            old = int(level[i])
            w, m = want_level(mag[r], c, dt_max, L)
            margin = min(margin, m)
            if first:
                new = w
                kick[r] = half * step_of[new]
            else:
                if closing:
                    new = old
                elif w > old:
                    new = w
                elif w < old and old > 0 and T % (1 << (L - old + 1)) == 0:
                    new = old - 1
                else:
                    new = old
                kick[r] = half * step_of[old] if closing else half * step_of[old] + half * step_of[new]
            level[i] = new
        v[active] += a * kick[:, None]
        first = False
        deepest = int(level.max()) if n else 0
        clock["deepest_level"] = max(clock["deepest_level"], deepest)
        clock["pair_terms"] += int(active.size) * n
        capped = not closing and clock["substeps"] == max_substeps
        dn = 0 if closing or capped else 1 << (L - deepest)
        history.append((int(active.size), dn))
        if closing:
            clock["finished"] = 1
            break
        if capped:
            clock["status"] = 2
            break
        x += v * (np.float64(dn) * tick)
        T += dn
        clock["substeps"] += 1
        active = np.flatnonzero(T % (1 << (L - level.astype(np.int64))) == 0)
    clock.update(t=float(np.float64(t_start) + np.float64(T) * tick), ticks=T)
    return b, clock, np.array(history, dtype=np.int64).reshape(-1, 2), level, float(margin)


def shared_step_pair_terms(history, n: int) -> int:
    """What the same substeps cost when every body is evaluated at each: (substeps + 1) n^2, the all-pairs count of a shared step as
    small as the smallest present -- the figure a block run's pair_terms is compared with."""
    return int(len(history)) * n * n
