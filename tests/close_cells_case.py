"""Inputs that put a close pair across EVERY boundary of the sorted-cell refinement (csrc/close_hash.hip), and the
definition of the list that refinement has to produce (test input only: numpy, no GPU, no oracle).

The refinement bins candidates into cells of edge h = 2^-9 and looks for partners at 0 < r^2 < 1e-6 in the 3^D cells
around a target.  build() plants, on a jittered lattice that has no close pair of its own, one pair for every neighbour
direction (26 in 3D, 8 in 2D) and every kind of KINDS: the two bodies sit on opposite sides of a cell corner along the
direction's non-zero axes (separation split evenly over them) and mid-cell (0.37 h) on the others.

  kind          separation   r^2 (fp32)          what must happen
  skipped       6.5e-6       2e-11 .. 8e-11      listed; contributes nothing (the reference skips r^2 < 1e-10)
  counted       1.3e-5       1.2e-10 .. 3e-10    listed; unlisted, the fast kernel's bias 2 kTiny / r^2 is >= 4.7e-5
  listed_only   6.0e-4       2.4e-7 .. 8e-7      listed (no visible effect on the forces: only the count sees it)
  outside       1.15e-3      > 1.2e-6            NOT listed, although the partner sits in an adjacent cell

Every planted r^2 stays 20 % away from 1e-10 and from 1e-6, so the order of the fp32 operations decides no case.

bad_targets() is the definition itself: body i is bad iff some j has 0 < r^2 < 1e-6, r^2 in fp32 in the kernels' order."""
import itertools

import numpy as np

H = 2.0 ** -9                       # cell edge of the sorted-cell refinement
INV_H = 512.0
BAD_R2 = np.float32(1.0e-6)         # kBadR2
SKIP_R2 = 1.0e-10                   # the reference's skip rule
MID = 0.37                          # position inside the cell on the axes a pair does not straddle

KINDS = ("skipped", "counted", "listed_only", "outside")
SEPARATION = {"skipped": 6.5e-6, "counted": 1.3e-5, "listed_only": 6.0e-4, "outside": 1.15e-3}
R2_RANGE = {"skipped": (2.0e-11, 8.0e-11), "counted": (1.2e-10, 3.0e-10), "listed_only": (2.4e-7, 8.0e-7),
            "outside": (1.2e-6, 1.5e-6)}
LISTED = {"skipped": True, "counted": True, "listed_only": True, "outside": False}

SPACING, JITTER = 0.1, 0.02         # background lattice: no two of its bodies nearer than 0.1 - 2 * 0.02 = 0.06
LATTICE_SIDE = {3: 21, 2: 95}       # 21^3 bodies in [-1, 1]^3; 95^2 bodies at the same spacing in [-4.7, 4.7]^2
PLANT_HALF = 10                     # planted pairs stay inside the lattice cells of [-1, 1]^D in both dimensions

PAIR_DTYPE = np.dtype([("p", np.int64), ("q", np.int64), ("kind", "U12"), ("direction", np.int64, (3,)),
                       ("corner", np.int64, (3,)), ("zero_corner", np.bool_)])


def directions(dim):
    return [d for d in itertools.product((-1, 0, 1), repeat=dim) if any(d)]


def n_background(dim):
    return LATTICE_SIDE[dim] ** dim


def n_bodies(dim):
    return n_background(dim) + 2 * len(KINDS) * len(directions(dim))


def lattice(dim, rng, keep=None):
    """Jittered lattice, fp64; keep = number of sites kept (an evenly spaced subset) or None for all."""
    side = LATTICE_SIDE[dim]
    half = (side - 1) // 2
    axes = [np.arange(-half, half + 1, dtype=np.float64) * SPACING] * dim
    g = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, dim)
    g = g + rng.uniform(-JITTER, JITTER, size=g.shape)
    if keep is not None:
        g = g[np.linspace(0, g.shape[0] - 1, keep).astype(np.int64)]
    return g


KAPPA_COMPONENT = 3.0               # plant_pairs: off-axis components of the background's pull on a counted pair
KAPPA_VECTOR = 6.0                  # ... and the background's whole pull on a skipped pair (sum |t_j| / |sum t_j|)


def pull_condition(at, pos, mass):
    """Conditioning of the pull of bodies (pos, mass) on a body at `at` under the reference's pair law t_j = m_j d_j / r_j^4:
    (per component sum_j |t_jk| / |sum_j t_jk|, of the vector sum_j |t_j| / |sum_j t_j|).  fp64; bodies nearer than 1e-5 (the
    body itself, its partner) are left out."""
    d = pos - at
    r2 = (d * d).sum(axis=1)
    far = r2 >= 1.0e-9
    t = (mass[far] / r2[far] ** 2)[:, None] * d[far]
    return np.abs(t).sum(axis=0) / np.abs(t.sum(axis=0)), np.sqrt((t * t).sum(axis=1)).sum() / np.sqrt((t.sum(axis=0) ** 2).sum())


def plant_pairs(dim, rng, back, back_mass, planted_mass):
    """(positions [2 * pairs, dim] fp64, pair table with p / q as indices into those positions).

    A pair's partner adds nothing to the force components along the axes it does not straddle (both bodies sit at 0.37 h
    there), and nothing at all when the pair is skipped: those numbers are sums over the other bodies, which cancel at most
    places between lattice sites.  A comparison at rtol = 2e-5 per component is only a statement about the close-set path
    where that sum is well conditioned, so a counted or skipped pair moves on to the next free lattice cell until it is
    (pull_condition over the lattice and every other planted body)."""
    dirs = directions(dim)
    n_pairs = len(KINDS) * len(dirs)
    pos = np.zeros((2 * n_pairs, dim))
    pairs = np.zeros(n_pairs, dtype=PAIR_DTYPE)
    # the middle of a lattice cell is >= 0.05 - JITTER = 0.03 per axis from every lattice body; one pair per lattice cell
    cells = np.stack(np.meshgrid(*[np.arange(-PLANT_HALF, PLANT_HALF)] * dim, indexing="ij"), -1).reshape(-1, dim)
    cells = cells[rng.permutation(cells.shape[0])]
    centres = np.full((n_pairs, dim), np.inf)
    placed = np.zeros(2 * n_pairs, dtype=bool)
    state = {"next": 0}

    def well_conditioned(t):
        kind, d = str(pairs[t]["kind"]), pairs[t]["direction"][:dim]
        if kind not in ("counted", "skipped"):
            return True
        others = placed.copy()
        others[2 * t:2 * t + 2] = False
        comp, vec = pull_condition((pos[2 * t] + pos[2 * t + 1]) / 2, np.concatenate([back, pos[others]]),
                                   np.concatenate([back_mass, planted_mass[others]]))
        return vec <= KAPPA_VECTOR if kind == "skipped" else all(comp[a] <= KAPPA_COMPONENT for a in range(dim) if not d[a])

    def place(t):
        d, kind = pairs[t]["direction"][:dim], str(pairs[t]["kind"])
        straddled = [a for a in range(dim) if d[a]]
        centres[t] = np.inf
        while True:
            centre = (cells[state["next"]] + 0.5) * SPACING
            state["next"] += 1
            if pairs[t]["zero_corner"]:
                centre[straddled[0]] = 0.0       # the pair's cells are -1 and 0 there: floorf of a negative, wrapped index
            if np.abs(centres - centre).max(axis=1).min() < 0.05:
                continue
            corner = np.rint(centre * INV_H).astype(np.int64)
            delta = SEPARATION[kind] / np.sqrt(len(straddled))
            for a in range(dim):
                if d[a]:
                    pos[2 * t, a] = corner[a] * H - d[a] * delta / 2
                    pos[2 * t + 1, a] = corner[a] * H + d[a] * delta / 2
                else:
                    pos[2 * t, a] = pos[2 * t + 1, a] = (corner[a] + MID) * H
            if well_conditioned(t):
                break
        centres[t] = centre
        pairs[t]["corner"][:dim] = corner
        placed[2 * t:2 * t + 2] = True

    for di, d in enumerate(dirs):
        for ki, kind in enumerate(KINDS):
            t = di * len(KINDS) + ki
            pairs[t]["p"], pairs[t]["q"], pairs[t]["kind"] = 2 * t, 2 * t + 1, kind
            pairs[t]["direction"][:dim] = d
            pairs[t]["zero_corner"] = (di + ki) % 2 == 0     # every direction and every kind gets corners at coordinate 0
    for t in range(n_pairs):
        place(t)
    for _ in range(50):                          # a pair planted later changes the pull on its neighbours: settle
        moved = [t for t in range(n_pairs) if not well_conditioned(t)]
        for t in moved:
            place(t)
        if not moved:
            break
    assert not moved, "no well-conditioned placement found"
    return pos, pairs


def _finish(template, pos, dim):
    b = np.ascontiguousarray(template[:pos.shape[0]].copy())
    assert b.shape == (pos.shape[0], 2 * dim + 1), "template: oracle.generate(seed, n_bodies, dim)"
    b[:, :dim] = pos.astype(np.float32)
    b[:, -1] = b[:, -1].astype(np.float32)
    return b


def build(dim, template, seed=7, keep_background=None):
    """(bodies [n, 2 dim + 1] fp64 holding fp32-representable positions and masses, pair table).

    template: oracle.generate(seed, n, dim) with n >= the rows needed -- its masses and velocities are kept.  The planted bodies
    are spread evenly through the array (never two partners next to each other), the lattice fills the rest."""
    rng = np.random.default_rng(seed)
    back = lattice(dim, rng, keep_background)
    n_planted = 2 * len(KINDS) * len(directions(dim))
    n = back.shape[0] + n_planted
    slots = np.linspace(3, n - 4, n_planted).astype(np.int64)            # strictly increasing: n >> planted bodies
    is_planted = np.zeros(n, dtype=bool)
    is_planted[slots] = True
    order = rng.permutation(n_planted)                                    # planted body order[k] goes to slots[k]
    where = np.empty(n_planted, dtype=np.int64)
    where[order] = slots
    mass = template[:n, -1].astype(np.float32).astype(np.float64)
    planted, pairs = plant_pairs(dim, rng, back, mass[~is_planted], mass[where])
    pos = np.zeros((n, dim))
    pos[where] = planted
    pos[~is_planted] = back
    pairs["p"], pairs["q"] = where[pairs["p"]], where[pairs["q"]]
    return _finish(template, pos, dim), pairs


def pair_r2_f32(pos_f32, i, j):
    """r^2 of bodies i and j (index arrays) as the kernels compute it: dx * dx, then fma with dy, then fma with dz, in fp32."""
    p = np.asarray(pos_f32, dtype=np.float32)
    d = (p[j] - p[i]).astype(np.float32)
    r2 = (d[..., 0] * d[..., 0]).astype(np.float32)
    for a in range(1, p.shape[1]):
        da = d[..., a].astype(np.float64)
        r2 = (da * da + r2.astype(np.float64)).astype(np.float32)   # the product is exact in fp64: one rounding, as an fma
    return r2


def bad_targets(pos_f32, dim, targets=None, block=512):
    """bool[len(targets)]: target i is bad iff some body j of pos_f32 has 0 < r^2 < 1e-6 (targets: default all bodies).

    All pairs, in blocks of rows.  The only shortcut: a block of targets (taken in the order of their x) is compared with the
    bodies whose x lies within 1.1e-3 of the block's range -- r^2 >= dx^2, so nothing beyond can be below 1e-6."""
    p = np.ascontiguousarray(np.asarray(pos_f32)[:, :dim], dtype=np.float32)
    assert np.array_equal(p, np.asarray(pos_f32)[:, :dim]), "positions must be fp32-representable"
    targets = np.arange(p.shape[0]) if targets is None else np.asarray(targets, dtype=np.int64)
    by_x = np.argsort(p[:, 0], kind="stable")
    xs = p[by_x, 0].astype(np.float64)
    targets_by_x = targets[np.argsort(p[targets, 0], kind="stable")]
    bad_of = np.zeros(p.shape[0], dtype=bool)
    for lo in range(0, targets_by_x.size, block):
        rows = targets_by_x[lo:lo + block]
        t = p[rows]
        w = by_x[np.searchsorted(xs, float(t[0, 0]) - 1.1e-3):np.searchsorted(xs, float(t[-1, 0]) + 1.1e-3, side="right")]
        s = p[w]
        d = s[None, :, 0] - t[:, None, 0]
        r2 = d * d
        for a in range(1, dim):
            da = (s[None, :, a] - t[:, None, a]).astype(np.float64)
            r2 = (da * da + r2.astype(np.float64)).astype(np.float32)   # one rounding of the exact sum: an fma
        bad_of[rows] = ((r2 > 0) & (r2 < BAD_R2)).any(axis=1)
    return bad_of[targets]


def cell_of(pos_f32):
    """Integer cell coordinates as hash_keys_kernel computes them: floorf(x * 512) in fp32 (the scaling is exact)."""
    return np.floor(np.asarray(pos_f32, dtype=np.float32) * np.float32(INV_H)).astype(np.int64)


def rows_of_kind(pairs, kind):
    sel = pairs[pairs["kind"] == kind]
    return np.concatenate([sel["p"], sel["q"]])


def expected_bad(pairs):
    return 2 * int(sum(LISTED[k] for k in pairs["kind"]))


def split_pair(t):
    """Every second pair of the table is split over two shards: per kind, directions 2, 3, 6, 7, ... or the others, so that
    every kind and both kinds of corner (at coordinate 0 or not) occur split and unsplit."""
    return (t % len(KINDS) + t // len(KINDS) // 2) % 2 == 1


def shard_order(pairs, n, n_shards, seed=11):
    """Permutation `order` (new row k holds old row order[k]) after which every second planted pair has its two bodies in
    different shards of an n_shards split; returns (order, pair table in the new numbering)."""
    rng = np.random.default_rng(seed)
    L = -(-n // n_shards)
    sizes = [max(0, min(L, n - s * L)) for s in range(n_shards)]
    members = [[] for _ in range(n_shards)]
    planted = np.zeros(n, dtype=bool)
    for t, pr in enumerate(pairs):
        s = (t // 2) % n_shards
        members[s].append(int(pr["p"]))
        members[(s + 1) % n_shards if split_pair(t) else s].append(int(pr["q"]))
        planted[[pr["p"], pr["q"]]] = True
    rest = iter(np.flatnonzero(~planted))
    order = []
    for s in range(n_shards):
        m = members[s] + [int(next(rest)) for _ in range(sizes[s] - len(members[s]))]
        order += [m[k] for k in rng.permutation(len(m))]
    order = np.array(order, dtype=np.int64)
    assert order.size == n and np.array_equal(np.sort(order), np.arange(n))
    new_of_old = np.empty(n, dtype=np.int64)
    new_of_old[order] = np.arange(n)
    moved = pairs.copy()
    moved["p"], moved["q"] = new_of_old[pairs["p"]], new_of_old[pairs["q"]]
    return order, moved


# ---- the other inputs of tests/test_gpu_close_cells.py ------------------------------------------------------------------

def far_shell(n, dim, rng):
    """n bodies at coordinates >= 1e5 on every axis (no close-set candidates), on a lattice of spacing 64: no close pair."""
    side = int(np.ceil(n ** (1.0 / dim)))
    g = np.stack(np.meshgrid(*[np.arange(side, dtype=np.float64)] * dim, indexing="ij"), -1).reshape(-1, dim)[:n]
    return 1.0e5 + 64.0 * g + rng.uniform(-8.0, 8.0, size=g.shape)


def build_with_far_shell(dim, template, keep_background=400, n_total=14000, seed=7):
    """The planted cloud of build() on a thinned lattice, surrounded by bodies at coordinates >= 1e5, so that candidates are
    <= 1/16 of the system and the library checks candidates x candidates (refine_close_kernel) on the very same pairs."""
    near, pairs = build(dim, template, seed=seed, keep_background=keep_background)
    rng = np.random.default_rng(seed + 1)
    n_far = n_total - near.shape[0]
    assert near.shape[0] * 16 <= n_total
    pos = np.concatenate([near[:, :dim], far_shell(n_far, dim, rng)])
    b = _finish(template, pos, dim)
    b[:, dim:2 * dim] = 0.0          # nothing moves: the asynchronous poll must see the uploaded positions
    return b, pairs


def counted_pair_at(centre, dim):
    """Two positions 1.3e-5 apart along x around `centre` (inside one cell when centre is mid-cell)."""
    p, q = np.array(centre, dtype=np.float64), np.array(centre, dtype=np.float64)
    p[0] -= SEPARATION["counted"] / 2
    q[0] += SEPARATION["counted"] / 2
    return p, q


def build_equal_keys(dim, template, duplicates=5000, seed=7):
    """build()'s system plus `duplicates` exact copies of one point and a counted pair in the SAME cell, 1.2e-3 away from the
    point: an equal-key run of duplicates + 2, longer than one 4096-element tile of the radix sort.
    Returns (bodies, pair table, rows of the duplicates, (p, q) of the extra pair)."""
    near, pairs = build(dim, template, seed=seed)
    n0 = near.shape[0]
    # the middle of the lattice cell around (1.25, 1.25, ...): beyond the planted pairs (|x| <= 1), in 3D beyond the lattice too
    cell = np.full(dim, int(1.25 * INV_H))
    point = (cell + 0.15) * H
    centre = (cell + 0.45) * H                                          # off the duplicates on every axis: no component of
    centre[0] = (cell[0] + 0.80) * H                                    # their pull vanishes; >= 0.71 h = 1.4e-3 from them
    p, q = counted_pair_at(centre, dim)
    pos = np.concatenate([near[:, :dim], np.repeat(point[None], duplicates, axis=0), p[None], q[None]])
    b = _finish(template, pos, dim)
    return b, pairs, np.arange(n0, n0 + duplicates), (n0 + duplicates, n0 + duplicates + 1)


def build_eighth(dim, template, n_pairs, n=8192):
    """n bodies on a lattice of spacing 0.1 (every coordinate small: all are candidates), the first 2 * n_pairs of them
    forming isolated listed-only pairs along x: exactly 2 * n_pairs bad targets."""
    side = int(np.ceil((n - n_pairs) ** (1.0 / dim)))
    g = np.stack(np.meshgrid(*[np.arange(side, dtype=np.float64)] * dim, indexing="ij"), -1).reshape(-1, dim)
    g = (g - side // 2) * SPACING + 0.013                               # off the cell corners, both signs
    site = g[:n - n_pairs]
    pos = np.empty((n, dim))
    pos[:n_pairs] = site[:n_pairs]
    pos[n_pairs:2 * n_pairs] = site[:n_pairs]
    pos[n_pairs:2 * n_pairs, 0] += SEPARATION["listed_only"]
    pos[2 * n_pairs:] = site[n_pairs:]
    return _finish(template, pos, dim)


def build_range_ends(dim, template, seed=7):
    """build()'s cloud plus pairs ONE fp32 step apart just below |x| = 8192 and 16384 on both signs (the other coordinates
    small): cell indices up to 8.4e6, fp32 spacing 2^-11 and 2^-10 -- so r^2 = 2.4e-7 and 9.5e-7.
    Returns (bodies, pair table, rows [k, 2] of the extra pairs)."""
    near, pairs = build(dim, template, seed=seed)
    f32 = np.float32
    extra = []
    for k, edge in enumerate((8192.0, -8192.0, 16384.0, -16384.0)):
        a = np.nextafter(f32(edge), f32(0))
        b_ = np.nextafter(a, f32(0))
        other = [(1.2 + 0.05 * k + 0.011 * ax) for ax in range(1, dim)]
        extra += [[float(a)] + other, [float(b_)] + other]
    pos = np.concatenate([near[:, :dim], np.array(extra)])
    n0 = near.shape[0]
    return _finish(template, pos, dim), pairs, np.arange(n0, n0 + len(extra)).reshape(-1, 2)
