"""TEST INFRASTRUCTURE (plain numpy: no device, no oracle library): inputs on which a single wrong PAIR TERM of the all-pairs
energy (nbx_ctx_energy / nbx_node_energy: potential_kernel<D, SOFT> and energy_partials_kernel) cannot hide, the fp64
specification of what the API returns, and the fault models that say so.

On a dense input one pair is ~2/N^2 of the total, far below the 2e-6 the totals are compared to.  Here all masses are zero but
those of two to four HEAVY bodies, so every pair is a sizeable part of the answer, and the heavy bodies stand where the kernel's
tiling has an edge:

where             shard, local index, source tile of the virtual tile list, entry, source slice, target workgroup and q (which of a
                  lane's two targets) of body i -- the library's own rules (shard_len = ceil(N / G), pad = next multiple of 4,096,
                  256-body tiles, 16 slices of G * pad / 4096 tiles, 512 targets per workgroup); the GPU test asserts shard_len
                  and pad against Context before it trusts this copy.
per_body_phi      phi_i = sum_{j != i} m_j u(r_ij^2) in fp64 on fp32-representable inputs, the self term left out BY INDEX only:
                  u = 1/r^2, skipped for r^2 < 1e-10 ('reference'); 1/(r^2 + eps^2) ('softened'); 1/sqrt(r^2 + eps^2) ('newton').
shares            per-shard (kinetic, potential) as the API returns them: sum over the shard's bodies of m v^2 / 2 and of
                  (G m / 4) phi ('newton': -(G m / 2) phi); shares_of_laws: the same for several laws from one pass over the pairs.
PROBES            sparse-mass probes, one per placement class (the name says what it distinguishes).
PAIR_PROBES       two heavy bodies of classes 2, 5 and 6 exactly coincident, just below and just above the skip threshold.
DENSE             generated bodies with every mass kept, on partitions with one-body and empty shards.
fault_models      the per-shard potential shares a kernel with ONE modelled fault would return (FAULTS below).
miss              by how many tolerances a set of shares misses the checks of tests/test_gpu_energy_pairs.py.
"""
import collections

import numpy as np

import nbody_amd

K_TILE = 256                         # sources per LDS tile (kTile)
PAD_QUANTUM = 4096                   # a shard's slots: shard_len rounded up to this (kPadQuantum)
PHI_SLICES = 16                      # source slices of one potential launch (kPhiSlices)
WG_TARGETS = 512                     # targets per workgroup: 256 lanes, two targets (q = 0, 1) per lane
R2_SKIP = 1e-10                      # the reference law's skip threshold (methods.cpp:24)
G_REFERENCE = 4.471e-21              # nbody-sim-new/utils.h:21

# The two tolerances of the potential energy (relative), and the kinetic one.
#   PE_TOL        the project's existing energy tolerance.  On a sparse probe the kernel's own arithmetic stays inside it: at most
#                 8 non-zero terms per tile, each with <= 3 roundings in r^2, one add of eps^2, a 1-ulp v_rcp_f32 / v_rsq_f32, an
#                 fma, and one cast of the slice sum: <= 16 u ~ 1e-6 (u = 2^-24).  On a dense share of >= 64 bodies the errors of
#                 the bodies' sums average out as they do in the 3,000-body totals this tolerance comes from.
#   SMALL_SHARE_TOL  worst case of the kernel's fp32 level, a sequential sum of K_TILE non-negative terms per tile: (K_TILE - 1) u
#                 from the adds and <= 8 u per term and for the cast, relative to the sum because every term has one sign.  A
#                 share is a sum of m_i phi_i of one sign again, so the bound holds for a share of ANY number of bodies; it is
#                 used where nothing averages: shares of fewer than 64 bodies, the one-body share (a single phi_i) among them.
PE_TOL = 2e-6
SMALL_SHARE_TOL = (K_TILE + 8) * 2.0 ** -24
SMALL_SHARE_BODIES = 64
KE_TOL = 1e-13

Place = collections.namedtuple("Place", "shard local tile entry slice wg q")


def layout(n, n_shards):
    """shard_len, pad, tiles per chunk and tiles per source slice of an n-body system on n_shards shards."""
    shard_len = -(-n // n_shards)
    pad = max(PAD_QUANTUM, -(-shard_len // PAD_QUANTUM) * PAD_QUANTUM)
    assert (n_shards * pad) % (PHI_SLICES * K_TILE) == 0
    return {"shard_len": shard_len, "pad": pad, "tiles_per_chunk": pad // K_TILE, "tiles_per_split": n_shards * pad // (PHI_SLICES * K_TILE)}


def counts(n, n_shards):
    sl = layout(n, n_shards)["shard_len"]
    return [max(0, min(sl, n - g * sl)) for g in range(n_shards)]


def places(n, n_shards, idx):
    """where() for an index array: a Place of int64 arrays."""
    lay = layout(n, n_shards)
    idx = np.asarray(idx, dtype=np.int64)
    assert ((idx >= 0) & (idx < n)).all()
    shard = idx // lay["shard_len"]
    local = idx - shard * lay["shard_len"]
    tile = shard * lay["tiles_per_chunk"] + local // K_TILE
    return Place(shard, local, tile, local % K_TILE, tile // lay["tiles_per_split"], local // WG_TARGETS, (local % WG_TARGETS) // K_TILE)


def where(n, n_shards, i):
    """Place(shard, local, tile, entry, slice, wg, q) of body i: as a SOURCE it is entry `entry` of tile `tile` of the virtual tile
    list, read by the workgroups of source slice `slice`; as a TARGET it is lane `entry`'s q-th body in workgroup `wg` of its shard."""
    return Place(*(int(v[0]) for v in places(n, n_shards, [i])))


def report(n, n_shards, idx):
    """For failure messages: body -> its Place, as text."""
    return "; ".join(f"{int(i)}: " + " ".join(f"{k}={v}" for k, v in where(n, n_shards, int(i))._asdict().items()) for i in idx)


# ---- the specification -------------------------------------------------------------------------------------------------

def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def is_f32_input(b, dim):
    return bool(np.array_equal(b[:, :dim], _f32(b[:, :dim])) and np.array_equal(b[:, -1], _f32(b[:, -1])))


def _u(r2, law, eps):
    """The pair weight u(r^2) of a law; the reference law's skipped pairs weigh nothing."""
    e2 = eps * eps
    if law == "reference":
        ok = r2 >= R2_SKIP
        return np.where(ok, 1.0 / np.where(ok, r2, 1.0), 0.0)
    assert eps > 0.0, "the softened laws need a softening length"
    if law == "softened":
        return 1.0 / (r2 + e2)
    if law == "newton":
        return 1.0 / np.sqrt(r2 + e2)
    raise ValueError(law)


def pair_terms(b, rows, cols, law, eps):
    """(T, r2): T[a, c] = m_cols[c] u(r^2) of target rows[a] and source cols[c], 0 where rows[a] == cols[c]; r2 beside it."""
    dim = (b.shape[1] - 1) // 2
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    r2 = np.zeros((rows.size, cols.size))
    for k in range(dim):                                     # (x, y, z in turn, as the oracle adds them)
        d = b[cols, k][None, :] - b[rows, k][:, None]
        r2 += d * d
    T = b[cols, -1][None, :] * _u(r2, law, eps)
    T[rows[:, None] == cols[None, :]] = 0.0
    return T, r2


def per_body_phi(b, law, eps=0.0, rows=None, block=512):
    """phi_i for the given rows (all bodies when None), fp64.  Massless sources are left out: their term is an exact zero under
    every law (finite weight, or skipped)."""
    dim = (b.shape[1] - 1) // 2
    assert is_f32_input(b, dim), "positions and masses must be fp32 numbers: the device holds them as such"
    rows = np.arange(b.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    cols = np.flatnonzero(b[:, -1] != 0.0)
    out = np.zeros(rows.size)
    for lo in range(0, rows.size, block):
        out[lo:lo + block] = pair_terms(b, rows[lo:lo + block], cols, law, eps)[0].sum(1)
    return out


def pe_factor(law, G):
    return -0.5 * G if law == "newton" else 0.25 * G


def _by_shard(values, n, n_shards):
    sl = layout(n, n_shards)["shard_len"]
    return np.array([values[g * sl:min(n, g * sl + sl)].sum() for g in range(n_shards)])


def shares_of_laws(b, n_shards, laws, G=G_REFERENCE, block=1024):
    """{(law, eps): [n_shards, 2]}: every shard's (kinetic, potential) as nbx_ctx_energy returns it, for several laws at once.
    phi of the massive bodies as in per_body_phi, with every r^2 computed once: a block of pairs (I, J >= I) serves phi[I], and
    transposed phi[J], under all the laws (a dense 8,195-body input costs a second, not one per law and side)."""
    n, dim = b.shape[0], (b.shape[1] - 1) // 2
    assert is_f32_input(b, dim), "positions and masses must be fp32 numbers: the device holds them as such"
    m = b[:, -1]
    ke = _by_shard(0.5 * m * (b[:, dim:2 * dim] ** 2).sum(1), n, n_shards)
    live = np.flatnonzero(m != 0.0)
    x, ml = b[live, :dim], m[live]
    phi = {k: np.zeros(live.size) for k in laws}
    for lo in range(0, live.size, block):
        I = slice(lo, lo + block)
        for lo2 in range(lo, live.size, block):
            J = slice(lo2, lo2 + block)
            r2 = np.zeros((x[I].shape[0], x[J].shape[0]))
            for k in range(dim):
                d = x[J, k][None, :] - x[I, k][:, None]
                r2 += d * d
            for law, eps in laws:
                U = _u(r2, law, eps)
                if lo2 == lo:
                    np.fill_diagonal(U, 0.0)                  # self, by index
                    phi[(law, eps)][I] += U @ ml[J]
                else:
                    phi[(law, eps)][I] += U @ ml[J]
                    phi[(law, eps)][J] += ml[I] @ U
    out = {}
    for law, eps in laws:
        pe = np.zeros(n)
        pe[live] = pe_factor(law, G) * ml * phi[(law, eps)]
        out[(law, eps)] = np.stack((ke, _by_shard(pe, n, n_shards)), axis=1)
    return out


def shares(b, n_shards, law, eps=0.0, G=G_REFERENCE):
    """[n_shards, 2]: every shard's (kinetic, potential) as nbx_ctx_energy returns it."""
    return shares_of_laws(b, n_shards, ((law, eps),), G)[(law, eps)]


# ---- inputs ------------------------------------------------------------------------------------------------------------

HEAVY_MASSES = (4.0e7, 2.5e7, 3.25e7, 2.0e7)     # fp32 numbers, all different: a term weighed with the wrong body's mass shows
CLUSTER_CENTRE, CLUSTER_RADIUS = 5.0e6, 1.0e5    # the heavy bodies of a sparse probe stand 1e5 ... 3e5 apart
EPS_BELOW, EPS_ABOVE = 1.0e3, 1.0e7              # softening lengths below and above every such separation


def generated(n, dim, seed):
    """uniform_bodies with positions and masses rounded to fp32 (velocities stay fp64, as the device keeps them)."""
    b = nbody_amd.uniform_bodies(n, dim, seed)
    b[:, :dim] = _f32(b[:, :dim])
    b[:, -1] = _f32(b[:, -1])
    return b


# name: (n, n_shards, heavy bodies).  3 shards of 4,000 bodies: pad 4,096, 16 tiles per chunk, 3 tiles per slice; slice 4 is
# tiles 12-14, slice 5 tiles 15, 16, 17 and straddles the chunks 0 | 1 between tiles 15 and 16.
PROBES = collections.OrderedDict((
    # 1. two (three) entries of one tile: first, middle, last entry
    ("one_tile",          (3000, 1, (7, 130, 255))),
    ("one_tile_sharded",  (12000, 3, (4000 + 768 + 7, 4000 + 768 + 130, 4000 + 1023))),
    # 2. i and i + 256: one lane's two targets, and the body the own-tile index test must NOT exclude
    ("lane_pair",         (3000, 1, (517, 773, 2000))),
    ("lane_pair_sharded", (12000, 3, (8000 + 517, 8000 + 773))),
    # 3. i and i + 512: same lane and q, neighbouring workgroups
    ("next_workgroup",    (3000, 1, (5, 517, 1029))),
    ("next_workgroup_sharded", (12000, 3, (4000 + 5, 4000 + 517, 4000 + 1029))),
    # 4. entries 255 | 256 of adjacent tiles, 511 | 512 across a workgroup
    ("tile_and_workgroup_edges", (3000, 1, (255, 256, 511, 512))),
    ("tile_and_workgroup_edges_sharded", (12000, 3, (8000 + 255, 8000 + 256, 8000 + 511, 8000 + 512))),
    # 5. either side of a slice boundary (tiles 14 | 15), inside the slice that straddles a chunk boundary (15 | 16), and out of
    #    it again (17 | 18)
    ("slice_edge_into_chunk_edge", (12000, 3, (3839, 3840, 4000))),
    ("chunk_edge_out_of_slice",    (12000, 3, (3999, 4000 + 511, 4000 + 512))),
    #    ... and the slice edges of ONE shard of 8,195 bodies (padded to 12,288: 3 tiles per slice): tiles 2 | 3, and 5 | 6
    ("slice_edges_one_shard",      (8195, 1, (767, 768, 1535, 1536))),
    # 6. different shards at the same local index, and at local index +- 256
    ("same_local_index",       (12000, 3, (100, 4000 + 100, 8000 + 356))),
    ("same_local_index_minus", (12000, 3, (356, 4000 + 100, 8000 + 100))),
    # 7. body 0 and body n - 1.  Shards of 4,100 slots padded to 8,192 (6 tiles per slice), the last one holding 4,098 bodies
    #    (count % 64 = 2: body n - 1 is lane 1 of a two-lane last workgroup of the reduction); eight shards of 600, the last of
    #    595 (count % 64 = 19); one shard just past 8,192 (padded to 12,288, count % 64 = 3)
    ("ends_padded_to_8192",   (3 * 4100 - 2, 3, (0, 4099, 3 * 4100 - 3))),
    ("ends_eight_shards",     (8 * 600 - 5, 8, (0, 599, 8 * 600 - 6))),
    ("ends_one_shard",        (8195, 1, (0, 4097, 8194))),
))


def probe_bodies(name, dim):
    """Generated bodies, every mass zero but the probe's heavy bodies, which stand on a small irregular polygon (3D: a helix)
    so that no pair of them is a negligible part of the energy under any law (pair_shares; asserted on the CPU)."""
    n, n_shards, heavy = PROBES[name]
    b = generated(n, dim, 40 + list(PROBES).index(name))
    b[:, -1] = 0.0
    for k, i in enumerate(heavy):
        ang = 2.0 * np.pi * k / len(heavy) + 0.3
        rad = CLUSTER_RADIUS * (1.0 + 0.15 * k)
        x = [CLUSTER_CENTRE + rad * np.cos(ang), CLUSTER_CENTRE + rad * np.sin(ang), CLUSTER_CENTRE + 0.2 * CLUSTER_RADIUS * k]
        b[i, :dim] = _f32(x[:dim])
        b[i, -1] = HEAVY_MASSES[k]
    return b


# Threshold pairs.  Body A keeps its generated coordinates but for one axis, where it stands at 1.0; B is A moved along that axis
# by k * 2^-23 (the fp32 spacing in [1, 2)): both coordinates are fp32 numbers, the kernel's dx is exact, dy = dz = 0, and its
# r^2 is the fp32 rounding of dx * dx.  84 and 83 spacings are the nearest separations on either side of sqrt(1e-10).
SPACING = 2.0 ** -23
SEPARATIONS = collections.OrderedDict((("coincident", 0.0), ("below", 83 * SPACING), ("above", 84 * SPACING)))
PAIR_EPS_BELOW, PAIR_EPS_ABOVE = 1.0e-6, 1.0e-3  # softening lengths below and above 1e-5 (1e-6: the API's smallest)
for _name, _dx in SEPARATIONS.items():           # fp64 and fp32 agree about the side of the threshold, by 1e-3 relative or more
    _r2, _r2f = _dx * _dx, float(np.float32(np.float32(_dx) * np.float32(_dx)))
    assert float(np.float32(1.0 + _dx)) == 1.0 + _dx and float(np.float32(_dx)) == _dx
    if _name == "above":
        assert _r2 >= R2_SKIP * (1 + 1e-3) and _r2f >= R2_SKIP * (1 + 1e-3)
    else:
        assert _r2 <= R2_SKIP * (1 - 1e-3) and _r2f <= R2_SKIP * (1 - 1e-3)
assert SEPARATIONS["below"] > PAIR_EPS_BELOW and SEPARATIONS["above"] < PAIR_EPS_ABOVE

# name: (n, n_shards, A, B), the placement classes 2, 5 and 6 of PROBES
PAIR_PROBES = collections.OrderedDict((
    ("pair_lane",          (3000, 1, 517, 773)),
    ("pair_slice_edge",    (12000, 3, 3839, 3840)),
    ("pair_chunk_edge",    (12000, 3, 3999, 4000)),
    ("pair_same_local",    (12000, 3, 100, 4000 + 100)),
    ("pair_local_plus_256", (12000, 3, 356, 8000 + 100)),
))


def pair_bodies(name, separation, dim, massless=None):
    """The two-heavy-body input of a threshold pair; massless='A' / 'B' takes that body's mass away (the comparison input)."""
    n, n_shards, ia, ib = PAIR_PROBES[name]
    k = list(PAIR_PROBES).index(name)
    axis = k % dim
    b = generated(n, dim, 70 + k)
    b[:, -1] = 0.0
    b[ia, axis] = 1.0
    b[ib, :dim] = b[ia, :dim]
    b[ib, axis] = 1.0 + SEPARATIONS[separation]
    b[ia, -1], b[ib, -1] = HEAVY_MASSES[0], HEAVY_MASSES[1]
    if massless is not None:
        b[{"A": ia, "B": ib}[massless], -1] = 0.0
    return b


# name: (n, n_shards, seed of the 2D input, seed of the 3D input).  57 on 8: seven shards of 8 and ONE-BODY shard 7; 5 on 8:
# five one-body shards and three empty ones; 8,195 on 3: shards of 2,732, 2,732 and 2,731 (ragged last workgroups).  The seeds
# of the first two are chosen by the certificate (tests/test_energy_case_cpu.py): no term of a one-body share is too small to see.
DENSE = collections.OrderedDict((
    ("n57_g8",   (57, 8, 7, 5)),
    ("n5_g8",    (5, 8, 1, 1)),
    ("n8195_g3", (8195, 3, 21, 21)),
))


def dense_bodies(name, dim):
    n, n_shards, s2, s3 = DENSE[name]
    return generated(n, dim, s2 if dim == 2 else s3)


def share_tolerance(count):
    """Relative tolerance of a shard's potential share (see PE_TOL / SMALL_SHARE_TOL above)."""
    return PE_TOL if count >= SMALL_SHARE_BODIES else SMALL_SHARE_TOL


# ---- fault models ------------------------------------------------------------------------------------------------------

FAULTS = ("one_sided", "own_tile_without_chunk_test", "own_tile_without_q_test", "self_term_included", "skip_under_softened_law",
          "no_skip_under_reference_law", "last_tile_of_slice_dropped", "first_tile_of_chunk_dropped", "shares_rotated")
DROPPED_TERM_FAULTS = ("one_sided", "last_tile_of_slice_dropped", "first_tile_of_chunk_dropped")


def fault_models(b, n_shards, law, eps=0.0, G=G_REFERENCE, rows=None):
    """{fault: [(label, potential shares [n_shards])]}: what the shards would return with ONE fault in the kernel, everything else
    exact.  rows: the targets whose phi is modelled (default: the massive bodies; a massless body's phi never shows).  Only
    variants that change a term are listed: a fault that does not touch this input is absent (it 'does not apply').

      one_sided                    one pair counted from one side only: a single term m_j u_ij missing from phi_i (one variant per term)
      own_tile_without_chunk_test  softened laws: the own-entry exclusion hits the same LOCAL index in every shard
      own_tile_without_q_test      softened laws: it hits entry tid of both tiles of the workgroup: body i +- 256 as well
      self_term_included           softened laws: no exclusion at all: m_i u(0) joins phi_i
      skip_under_softened_law      the reference's r^2 < 1e-10 rule applied where it has no place
      no_skip_under_reference_law  ... and not applied where it belongs (a coincident pair: infinite)
      last_tile_of_slice_dropped   every slice ends one tile early
      first_tile_of_chunk_dropped  the walk loses the first tile of a chunk it steps into (a slice that starts there seeks it)
      shares_rotated               every shard returns its neighbour's share"""
    n = b.shape[0]
    cols = np.flatnonzero(b[:, -1] != 0.0)
    rows = cols if rows is None else np.asarray(rows, dtype=np.int64)
    T, r2 = pair_terms(b, rows, cols, law, eps)
    pr, pc = places(n, n_shards, rows), places(n, n_shards, cols)
    tps = layout(n, n_shards)["tiles_per_split"]
    soft = law != "reference"
    is_self = rows[:, None] == cols[None, :]
    f = pe_factor(law, G)

    def to_shares(Tm):
        with np.errstate(invalid="ignore"):
            per_row = f * b[rows, -1] * Tm.sum(1)
        return np.array([per_row[pr.shard == g].sum() for g in range(n_shards)])

    ref = to_shares(T)
    out = {}

    def add(fault, label, Tm):
        if not np.array_equal(Tm, T):
            out.setdefault(fault, []).append((label, to_shares(Tm)))

    def without(mask):
        return np.where(mask, 0.0, T)

    for a, c in zip(*np.nonzero(T)):
        Tm = T.copy()
        Tm[a, c] = 0.0
        add("one_sided", f"phi[{rows[a]}] without body {cols[c]}", Tm)
    if soft:
        same_local = pr.local[:, None] == pc.local[None, :]
        other_shard = pr.shard[:, None] != pc.shard[None, :]
        add("own_tile_without_chunk_test", "same local index, another shard", without(same_local & other_shard))
        lane_twin = ~other_shard & (pr.wg[:, None] == pc.wg[None, :]) & (pr.entry[:, None] == pc.entry[None, :]) & (pr.q[:, None] != pc.q[None, :])
        add("own_tile_without_q_test", "the lane's other target", without(lane_twin))
        add("self_term_included", "self", np.where(is_self, (b[cols, -1] * _u(np.zeros(1), law, eps))[None, :], T))
        add("skip_under_softened_law", "r^2 < 1e-10", without(~is_self & (r2 < R2_SKIP)))
    else:
        with np.errstate(divide="ignore"):
            add("no_skip_under_reference_law", "r^2 < 1e-10", np.where(~is_self & (r2 < R2_SKIP), b[cols, -1][None, :] / r2, T))
    add("last_tile_of_slice_dropped", "tile % tiles_per_split == tiles_per_split - 1", without((pc.tile % tps == tps - 1)[None, :] & ~is_self))
    stepped_into = (pc.shard >= 1) & (pc.local < K_TILE) & (pc.tile % tps != 0)
    add("first_tile_of_chunk_dropped", "tile 0 of a chunk >= 1, inside a slice", without(stepped_into[None, :] & ~is_self))
    if n_shards > 1 and not np.array_equal(np.roll(ref, 1), ref):
        out["shares_rotated"] = [("share[r] <- share[r - 1]", np.roll(ref, 1))]
    return ref, out


def miss(got, ref, tols=None, total_tol=PE_TOL):
    """By how many tolerances the potential shares `got` miss the checks against `ref`: the largest, over the shards and their
    sum (total_tol; None: the shards only), of |got - ref| / (tolerance * |ref|); a share that must be an absolute zero misses
    by infinity if it is not.  tols: per shard (default PE_TOL each, the sparse probes' tolerance)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    worst = 0.0
    tols = [PE_TOL] * ref.size if tols is None else tols
    checks = [(got[g], ref[g], tols[g]) for g in range(ref.size)]
    if total_tol is not None:
        checks.append((got.sum(), ref.sum(), total_tol))
    for x, r, tol in checks:
        if not np.isfinite(x):
            return float("inf")
        if x != r:
            worst = max(worst, float("inf") if r == 0.0 else abs(x - r) / (tol * abs(r)))
    return worst


def pair_shares(b, law, eps=0.0):
    """Every heavy pair's part of the potential energy: {(i, j): (m_i T_ij + m_j T_ji) / sum}, i < j."""
    cols = np.flatnonzero(b[:, -1] != 0.0)
    T, _ = pair_terms(b, cols, cols, law, eps)
    W = b[cols, -1][:, None] * T
    tot = W.sum()
    return {(int(cols[a]), int(cols[c])): float((W[a, c] + W[c, a]) / tot) for a in range(cols.size) for c in range(a + 1, cols.size)}
