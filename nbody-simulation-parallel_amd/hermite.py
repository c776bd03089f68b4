"""Fourth-order Hermite with block (hierarchical) time steps: the fp64 numpy specification of nbx_ctx_step_hermite_block and of the
sums of nbx_ctx_compute_accel_jerk_active (include/nbody_hip.h has the rule), next to blocksteps.block_leapfrog_spec.

Body i steps by dt_max / 2^level_i and holds (x, v, a, j) at its own time t_i.  All bodies are predicted to the current time;
accelerations and jerks are computed only for the bodies whose own step ends (the active ones), from ALL bodies' predicted positions
and velocities, and those bodies are corrected.  Time is counted in ticks of dt_max / 2^L."""
import numpy as np


def accel_jerk_rows(rows: np.ndarray, active, G: float, eps: float, law: str):
    """(a, j, S_a, S_j) of the bodies `active` from all `rows` (Body<D>: position[D], velocity[D], mass) as they stand, fp64:
        a_r = g sum_j m_j w d,   j_r = g sum_j m_j w [dv - p (d.dv) / rho^2 d],   d = x_j - x_r, dv = v_j - v_r, rho^2 = r^2 + eps^2, w = rho^-p
    with p = 4, g = -G for law "soft" (the softened reference law) and p = 3, g = G for "newton": the accelerations F / m of the
    context's kicks and their time derivatives along straight paths.  The row's own term is left out (it is an exact zero).
    S_a = |G| sum_j m_j w |d| and S_j = |G| sum_j m_j w |dv| (1 + p r^2 / rho^2) bound the magnitudes of the terms: the scales of the
    device's rounding errors."""
    b = np.asarray(rows, dtype=np.float64)
    active = np.asarray(active, dtype=np.int64)
    dim = (b.shape[1] - 1) // 2
    p = 4.0 if law == "soft" else 3.0
    d = b[None, :, :dim] - b[active, None, :dim]
    dv = b[None, :, dim:2 * dim] - b[active, None, dim:2 * dim]
    r2 = (d * d).sum(axis=2)
    rho2 = r2 + eps * eps
    w = b[None, :, -1] / (rho2 * rho2 if law == "soft" else rho2 * np.sqrt(rho2))
    w[np.arange(active.size), active] = 0.0
    rv = (d * dv).sum(axis=2)
    g = -G if law == "soft" else G
    a = g * (w[..., None] * d).sum(axis=1)
    j = g * (w[..., None] * (dv - (p * rv / rho2)[..., None] * d)).sum(axis=1)
    S_a = abs(G) * (np.abs(w) * np.sqrt(r2)).sum(axis=1)
    S_j = abs(G) * (np.abs(w) * np.sqrt((dv * dv).sum(axis=2)) * (1.0 + p * r2 / rho2)).sum(axis=1)
    return a, j, S_a, S_j


def _norms(u):
    """|u_r| with the squares added in component order, as the device adds them"""
    s = np.zeros(u.shape[0], dtype=np.float64)
    for k in range(u.shape[1]):
        s = s + u[:, k] * u[:, k]
    return np.sqrt(s)


def hermite_block_spec(bodies: np.ndarray, accel_jerk_fn, control: dict, n_blocks: int, max_substeps: int):
    """nbx_ctx_step_hermite_block in fp64 numpy.  bodies: Body<D> rows; accel_jerk_fn(rows, active) -> (a, j, ...), each
    [len(active), D], of the bodies `active` (ascending indices) from all rows as they stand -- the rows it is handed hold the
    PREDICTED positions and velocities (accel_jerk_rows with G, eps and law bound is one); control: a dict with eta, dt_max, levels
    and optionally eta_start (0.01) and t_start (0).  Returns what blocksteps.block_leapfrog_spec returns: (rows, clock, history,
    levels, margin), margin the smallest |raw / (dt_max 2^-j) - 1| over every choice made.
        evaluation 0, all bodies: level = want(eta_start |a| / |j|), t_i = 0
        after every evaluation: record (n_active, dn); T == T_end -> finished, stop; substeps == max_substeps -> status 2, stop
                                dn = 2^(L - deepest level present); T += dn
        predict all to T; (a1, j1) of the active; any component not finite -> status 1, stop, nobody corrected
        correct the active over h = their own step; raw by Aarseth's criterion; the level rule of the kick-drift-kick loop"""
    eta, dt_max, L = float(control["eta"]), float(control["dt_max"]), int(control["levels"])
    eta_start, t_start = float(control.get("eta_start", 0.01)), float(control.get("t_start", 0.0))
    if not (eta > 0 and np.isfinite(eta) and eta_start > 0 and np.isfinite(eta_start) and dt_max > 0 and np.isfinite(dt_max)
            and np.isfinite(t_start) and 0 <= L <= 20):
        raise ValueError("control outside the ranges of nbx_hermite_control")
    if n_blocks < 0 or not 0 <= max_substeps <= 1 << 20:
        raise ValueError("n_blocks must be >= 0 and max_substeps in [0, 1 << 20]")
    b = np.array(bodies, dtype=np.float64, copy=True)
    n = b.shape[0]
    dim = (b.shape[1] - 1) // 2
    x, v = b[:, :dim], b[:, dim:2 * dim]
    a, j = np.zeros((n, dim)), np.zeros((n, dim))
    t_i = np.zeros(n, dtype=np.int64)
    level = np.zeros(n, dtype=np.int32)
    clock = {"t": t_start, "ticks": 0, "pair_terms": 0, "substeps": 0, "evaluations": 0, "deepest_level": 0, "finished": 0, "status": 0}
    history, margin = [], np.inf
    if n_blocks == 0:
        return b, clock, np.zeros((0, 2), dtype=np.int64), level, margin
    f = np.float64
    step_of = f(dt_max) * f(2.0) ** -np.arange(L + 1, dtype=np.float64)   # dt_l, exact
    tick = step_of[L]
    T, T_end, first = 0, n_blocks << L, True
    active = np.arange(n)
    rows = b.copy()                                                       # what the evaluation sees: the predicted state
    with np.errstate(all="ignore"):
        while True:
            out = accel_jerk_fn(rows, active)
            a1 = np.asarray(out[0], dtype=np.float64).reshape(active.size, dim)
            j1 = np.asarray(out[1], dtype=np.float64).reshape(active.size, dim)
            clock["evaluations"] += 1
            if not (np.isfinite(a1).all() and np.isfinite(j1).all()):
                clock["status"] = 1
                break
            closing = T == T_end
            na, nj = _norms(a1), _norms(j1)
            if first:
                raw = np.where(nj == 0.0, np.inf, (f(eta_start) * na) / np.where(nj == 0.0, 1.0, nj))
            else:
                h = step_of[level[active]][:, None]
                h2 = h * h
                h3 = h2 * h
                a0, j0, v0, x0 = a[active], j[active], v[active], x[active]
                da = a0 - a1
                v1 = (v0 + (f(0.5) * h) * (a0 + a1)) + (h2 / f(12.0)) * (j0 - j1)
                x1 = (x0 + (f(0.5) * h) * (v0 + v1)) + (h2 / f(12.0)) * da
                a2 = (f(-6.0) * da - h * (f(4.0) * j0 + f(2.0) * j1)) / h2
                a3 = (f(12.0) * da + (f(6.0) * h) * (j0 + j1)) / h3
                a2e = a2 + h * a3
                n2, n3 = _norms(a2e), _norms(a3)
                den = nj * n3 + n2 * n2
                raw = np.where(den == 0.0, np.inf, np.sqrt((f(eta) * (na * n2 + nj * nj)) / np.where(den == 0.0, 1.0, den)))
                v[active], x[active] = v1, x1
            a[active], j[active], t_i[active] = a1, j1, T
            for r, i in enumerate(active):
                old = int(level[i])
                w, m = _want_raw(raw[r], dt_max, L)
                margin = min(margin, m)
                if first:
                    new = w
                elif closing:
                    new = old
                elif w > old:
                    new = w
                elif w < old and old > 0 and T % (1 << (L - old + 1)) == 0:
                    new = old - 1
                else:
                    new = old
                level[i] = new
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
            T += dn
            clock["substeps"] += 1
            h = ((T - t_i).astype(np.float64) * tick)[:, None]
            h2 = h * h
            rows = b.copy()
            rows[:, :dim] = ((x + v * h) + a * (f(0.5) * h2)) + j * ((h2 * h) / f(6.0))
            rows[:, dim:2 * dim] = (v + a * h) + j * (f(0.5) * h2)
            active = np.flatnonzero(T % (1 << (L - level.astype(np.int64))) == 0)
    clock.update(t=float(f(t_start) + f(T) * tick), ticks=T)
    return b, clock, np.array(history, dtype=np.int64).reshape(-1, 2), level, float(margin)


def _want_raw(raw, dt_max: float, levels: int):
    """(w, margin) of one choice from the raw step itself: blocksteps.want_level's halvings and margin"""
    raw, d = np.float64(raw), np.float64(dt_max)
    w = 0
    while d > raw and w < levels:
        d = np.float64(0.5) * d
        w += 1
    if not np.isfinite(raw):
        return w, np.inf
    steps = np.float64(dt_max) * np.float64(2.0) ** -np.arange(levels + 1, dtype=np.float64)
    return w, float(np.abs(raw / steps - 1.0).min())
