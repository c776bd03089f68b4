"""Leaf lists for the leaf-pair direct-sum entry point (nbx_leaf_pair_forces).

The reference's tree codes build their leaves by recursive subdivision and collect, per leaf, the adjacent
leaves whose bodies are summed directly (FMM neighbour lists: nbody-sim-new/fmm.cpp:455-476,
fmm_parlay.cpp:369-390).  The device entry point takes that structure as two CSR arrays; this module builds the
simplest instance of it -- a fixed-depth subdivision of the bounding box (a uniform grid of 2^depth cells per
axis; the non-empty cells are the leaves) with the 3^D adjacent cells as each leaf's list -- for tests, examples
and timing.  Pure integer/numpy host logic; any other tree can feed the same arrays."""
from __future__ import annotations

import numpy as np


def uniform_grid_leaves(bodies: np.ndarray, dim: int, depth: int):
    """Returns (leaf_offsets, leaf_bodies, list_offsets, list_sources), all uint32.
    Leaf = non-empty cell of the 2^depth-per-axis grid over the bodies' bounding box (padded by 1 %, like the
    reference's root box, fmm.cpp:386-387); list = the leaf itself first, then its non-empty adjacent cells."""
    pos = np.asarray(bodies)[:, :dim]
    n = pos.shape[0]
    g = 1 << depth
    if n == 0:
        z = np.zeros(1, dtype=np.uint32)
        return z, np.zeros(0, dtype=np.uint32), z.copy(), np.zeros(0, dtype=np.uint32)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    centre, half = (lo + hi) / 2.0, max(float((hi - lo).max()) / 2.0 * 1.01, 1e-300)
    cell = np.clip(np.floor((pos - (centre - half)) / (2.0 * half) * g).astype(np.int64), 0, g - 1)
    key = np.zeros(n, dtype=np.int64)
    for d in range(dim):
        key = key * g + cell[:, d]
    order = np.argsort(key, kind="stable")
    keys, first = np.unique(key[order], return_index=True)
    leaf_offsets = np.append(first, n).astype(np.uint32)
    leaf_bodies = order.astype(np.uint32)
    # decode the cell coordinates of every leaf and look its 3^dim neighbours up (keys is sorted: a binary search per neighbour cell)
    coords = np.zeros((keys.size, dim), dtype=np.int64)
    rest = keys.copy()
    for d in range(dim - 1, -1, -1):
        coords[:, d] = rest % g
        rest //= g
    offs = np.stack(np.meshgrid(*[np.arange(-1, 2)] * dim, indexing="ij"), -1).reshape(-1, dim)
    offs = np.concatenate([np.zeros((1, dim), dtype=offs.dtype), offs[np.any(offs != 0, axis=1)]])   # own bodies first (fmm_parlay.cpp:973-974)
    found = np.full((keys.size, offs.shape[0]), -1, dtype=np.int64)
    for c, o in enumerate(offs):
        nb = coords + o
        inside = np.all((nb >= 0) & (nb < g), axis=1)
        k = np.zeros(keys.size, dtype=np.int64)
        for d in range(dim):
            k = k * g + nb[:, d]
        at = np.minimum(np.searchsorted(keys, k), keys.size - 1)
        hit = inside & (keys[at] == k)
        found[hit, c] = at[hit]
    present = found >= 0
    list_offsets = np.concatenate([[0], np.cumsum(present.sum(axis=1))])
    list_sources = found[present]                                    # row-major: every leaf's cells in the order of `offs`
    return (leaf_offsets, leaf_bodies, np.asarray(list_offsets, dtype=np.uint32), np.asarray(list_sources, dtype=np.uint32))


def all_pairs_leaves(n: int, leaf_size: int):
    """Contiguous leaves of `leaf_size` bodies, every leaf on every list: the leaf-pair sum then equals the
    all-pairs sum (used to tie the leaf kernel to the brute-force oracle)."""
    n_leaves = max(1, -(-n // leaf_size))
    leaf_offsets = np.minimum(np.arange(n_leaves + 1) * leaf_size, n).astype(np.uint32)
    leaf_bodies = np.arange(n, dtype=np.uint32)
    list_offsets = (np.arange(n_leaves + 1) * n_leaves).astype(np.uint32)
    list_sources = np.tile(np.arange(n_leaves, dtype=np.uint32), n_leaves)
    return leaf_offsets, leaf_bodies, list_offsets, list_sources


def median_split_leaves(bodies: np.ndarray, dim: int, max_leaf_size: int = 16, reach: float = 1.0):
    """Leaves the way the reference's BVH makes them -- BVH<D>::build_recursive (nbody-sim-new/bvh.cpp:34-73): split the bodies at
    the median along the longest axis of their bounding box until a node holds at most max_leaf_size (methods.h:57: 16) -- with a
    near-field list per leaf: the leaf itself first, then every other leaf whose bounding box comes within `reach` x the leaf's own
    box diagonal of its box (box-to-box distance, the kind of acceptance test a traversal applies).  Leaves come out in tree
    order (depth first, lower half first), which keeps spatial neighbours close in leaf order.  Host-side numpy; a stand-in for a
    tree builder in tests and timing, not a port of the reference's pointer tree."""
    pos = np.asarray(bodies)[:, :dim]
    n = pos.shape[0]
    if n == 0:
        z = np.zeros(1, dtype=np.uint32)
        return z, np.zeros(0, dtype=np.uint32), z.copy(), np.zeros(0, dtype=np.uint32)
    # level by level: the nodes of a level have at most two different sizes (a node of s bodies splits into s // 2 and s - s // 2),
    # and all nodes of one size are split in one batched call
    order = np.arange(n)
    nodes = np.array([[0, n]], dtype=np.int64)              # [lo, hi) of the current level's nodes, in tree order
    done = []
    while nodes.size:
        size = nodes[:, 1] - nodes[:, 0]
        leaf = size <= max_leaf_size
        done.append(nodes[leaf])
        nodes = nodes[~leaf]
        size = size[~leaf]
        nxt = np.empty((2 * nodes.shape[0], 2), dtype=np.int64)
        for s_ in np.unique(size):
            sel = np.nonzero(size == s_)[0]
            at = nodes[sel, 0][:, None] + np.arange(s_)[None, :]          # [k, s] positions in `order`
            idx = order[at]
            p = pos[idx]                                                # [k, s, dim]
            axis = np.argmax(p.max(axis=1) - p.min(axis=1), axis=1)     # longest axis of every node's box
            val = np.take_along_axis(p, axis[:, None, None], axis=2)[:, :, 0]
            mid = int(s_) // 2
            part = np.argpartition(val, mid, axis=1)
            order[at] = np.take_along_axis(idx, part, axis=1)
            nxt[2 * sel, 0] = nodes[sel, 0]; nxt[2 * sel, 1] = nodes[sel, 0] + mid          # lower half first
            nxt[2 * sel + 1, 0] = nodes[sel, 0] + mid; nxt[2 * sel + 1, 1] = nodes[sel, 1]
        nodes = nxt
    leaves = np.concatenate(done)
    leaves = leaves[np.argsort(leaves[:, 0], kind="stable")]
    leaf_offsets = np.append(leaves[:, 0], n).astype(np.uint32)
    nl = leaves.shape[0]
    sorted_pos = pos[order]
    bmin = np.minimum.reduceat(sorted_pos, leaves[:, 0], axis=0)
    bmax = np.maximum.reduceat(sorted_pos, leaves[:, 0], axis=0)
    diag = np.linalg.norm(bmax - bmin, axis=1)
    centre = 0.5 * (bmin + bmax)
    from scipy.spatial import cKDTree
    # candidates by centre distance (a superset: box gap >= centre distance - the two half diagonals), then the exact box-to-box
    # distance.  Leaves are put into buckets of like diagonal (ratio 1.25) and every pair of buckets is queried once with the
    # radius its largest members need -- the result is arrays (a ball query per leaf returns Python lists: slow for a million bodies)
    half = 0.5 * diag
    d_min = max(float(diag.min()), 1e-300 + float(diag.max()) * 1e-6)
    bucket = np.floor(np.log(np.maximum(diag, d_min) / d_min) / np.log(1.25)).astype(np.int64)
    ids_of = [np.nonzero(bucket == b_)[0] for b_ in np.unique(bucket)]
    trees = [cKDTree(centre[ids]) for ids in ids_of]
    rows_parts, c_parts = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for ia, ta in zip(ids_of, trees):
        for ib, tb in zip(ids_of, trees):
            found = ta.sparse_distance_matrix(tb, float((0.5 + reach) * diag[ia].max() + half[ib].max()), output_type="ndarray")
            rows_parts.append(ia[found["i"]])
            c_parts.append(ib[found["j"]])
    rows, c = np.concatenate(rows_parts), np.concatenate(c_parts)
    other = c != rows
    rows, c = rows[other], c[other]
    gap = np.maximum(0.0, np.maximum(bmin[c] - bmax[rows], bmin[rows] - bmax[c]))
    near = np.sqrt((gap * gap).sum(axis=1)) <= reach * diag[rows]
    rows, c = rows[near], c[near]
    by_leaf = np.lexsort((c, rows))                          # every leaf's neighbours in ascending order
    rows, c = rows[by_leaf], c[by_leaf]
    counts = np.bincount(rows, minlength=nl)
    list_offsets = np.concatenate([[0], np.cumsum(counts + 1)])
    list_sources = np.empty(int(list_offsets[-1]), dtype=np.int64)
    list_sources[list_offsets[:-1]] = np.arange(nl)          # the leaf itself first
    rank = np.arange(rows.size) - np.repeat(np.cumsum(counts) - counts, counts)
    list_sources[list_offsets[rows] + 1 + rank] = c
    return (leaf_offsets, order.astype(np.uint32), np.asarray(list_offsets, dtype=np.uint32), np.asarray(list_sources, dtype=np.uint32))


def _morton_keys(cell: np.ndarray, dim: int, depth: int) -> np.ndarray:
    """Morton (Z-order) key of integer cell coordinates: bit b of axis d lands at bit b * dim + (dim - 1 - d)."""
    key = np.zeros(cell.shape[0], dtype=np.int64)
    for bit in range(depth):
        for d in range(dim):
            key |= ((cell[:, d] >> bit) & 1) << (bit * dim + (dim - 1 - d))
    return key


def _morton_coords(keys: np.ndarray, dim: int, level: int) -> np.ndarray:
    out = np.zeros((keys.size, dim), dtype=np.int64)
    for bit in range(level):
        for d in range(dim):
            out[:, d] |= ((keys >> (bit * dim + (dim - 1 - d))) & 1) << bit
    return out


def octree_cells(bodies: np.ndarray, dim: int, depth: int, theta: float, chunk_leaves: int = 16384):
    """A fixed-depth octree (quadtree in 2D) with near AND far lists, for nbx_leaf_plan_set_cells.  Returns
    (leaf_offsets, leaf_bodies, list_offsets, list_sources, cell_first_leaf, cell_leaf_count, far_offsets, far_cells), all uint32.
    Leaves: the non-empty cells of the 2^depth grid over the 1 %-padded bounding box (as uniform_grid_leaves), in MORTON order, so
    that every node of the tree is a contiguous range of leaves.  Cells: the non-empty nodes of levels 1 .. depth, level by level
    (the last `n_leaves` cells are the leaves themselves).  Per target leaf a top-down walk (octree.cpp:129-151's acceptance
    test on boxes): a node goes to the far list when side(node) < theta * gap, gap = the box-to-box distance between the leaf's
    grid box and the node's grid box -- so every body of an accepted node is farther than side / theta from every body of the
    leaf; a leaf-level node that is not accepted goes to the near list, the leaf itself first.  theta = 0 accepts nothing.
    The walk is level-synchronous over a frontier of (leaf, node) pairs, `chunk_leaves` target leaves at a time (memory)."""
    pos = np.asarray(bodies)[:, :dim]
    n = pos.shape[0]
    u32 = lambda a: np.asarray(a, dtype=np.uint32)
    none = np.zeros(0, dtype=np.uint32)
    if n == 0:
        z = np.zeros(1, dtype=np.uint32)
        return z, none, z.copy(), none.copy(), none.copy(), none.copy(), z.copy(), none.copy()
    g = 1 << depth
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    centre, half = (lo + hi) / 2.0, max(float((hi - lo).max()) / 2.0 * 1.01, 1e-300)
    cell = np.clip(np.floor((pos - (centre - half)) / (2.0 * half) * g).astype(np.int64), 0, g - 1)
    key = _morton_keys(cell, dim, depth)
    order = np.argsort(key, kind="stable")
    keys, first = np.unique(key[order], return_index=True)
    nl = keys.size
    leaf_offsets = np.append(first, n)
    # the non-empty nodes of every level: keys (sorted), leaf ranges, coordinates, children (a contiguous range of the next level)
    lv_keys, lv_first, lv_count, lv_coords, lv_base = {}, {}, {}, {}, {}
    base = 0
    for L in range(1, depth + 1):
        kl, f, c = np.unique(keys >> (dim * (depth - L)), return_index=True, return_counts=True)
        lv_keys[L], lv_first[L], lv_count[L], lv_coords[L], lv_base[L] = kl, f, c, _morton_coords(kl, dim, L), base
        base += kl.size
    child_first, child_count = {}, {}
    for L in range(1, depth):
        child_first[L] = np.searchsorted(lv_keys[L + 1], lv_keys[L] << dim)
        child_count[L] = np.searchsorted(lv_keys[L + 1], (lv_keys[L] + 1) << dim) - child_first[L]
    q = lv_coords[depth] if depth >= 1 else np.zeros((nl, dim), dtype=np.int64)
    near_t, near_s, far_t, far_c = [], [], [], []
    for t0 in range(0, nl, max(1, int(chunk_leaves))):
        t1 = min(nl, t0 + max(1, int(chunk_leaves)))
        if depth == 0:                                             # one leaf, no levels below the root: itself
            near_t.append(np.arange(t0, t1)); near_s.append(np.arange(t0, t1))
            continue
        n1 = lv_keys[1].size
        t = np.repeat(np.arange(t0, t1, dtype=np.int64), n1)
        node = np.tile(np.arange(n1, dtype=np.int64), t1 - t0)
        ft, fc = [], []
        for L in range(1, depth + 1):
            s = depth - L
            blo = lv_coords[L][node] << s
            qt = q[t]
            gap = np.maximum(0, np.maximum(blo - (qt + 1), qt - (blo + (1 << s))))
            acc = float(1 << s) < theta * np.sqrt((gap * gap).sum(axis=1).astype(np.float64))
            ft.append(t[acc]); fc.append(lv_base[L] + node[acc])
            t, node = t[~acc], node[~acc]
            if L == depth:
                break
            cnt = child_count[L][node]
            start = np.repeat(np.cumsum(cnt) - cnt, cnt)
            kid = np.repeat(child_first[L][node], cnt) + (np.arange(int(cnt.sum()), dtype=np.int64) - start)
            t, node = np.repeat(t, cnt), kid
        by = np.lexsort((node, node != t, t))                      # per leaf: itself first, then the others in Morton order
        near_t.append(t[by]); near_s.append(node[by])
        ft, fc = np.concatenate(ft), np.concatenate(fc)
        by = np.argsort(ft, kind="stable")                         # per leaf: coarse levels first, Morton order within a level
        far_t.append(ft[by]); far_c.append(fc[by])
    near_t, near_s = np.concatenate(near_t), np.concatenate(near_s)
    list_offsets = np.concatenate([[0], np.cumsum(np.bincount(near_t, minlength=nl))])
    if far_t:
        far_t, far_c = np.concatenate(far_t), np.concatenate(far_c)
    else:
        far_t = far_c = np.zeros(0, dtype=np.int64)
    far_offsets = np.concatenate([[0], np.cumsum(np.bincount(far_t, minlength=nl))])
    if depth >= 1:
        cell_first = np.concatenate([lv_first[L] for L in range(1, depth + 1)])
        cell_count = np.concatenate([lv_count[L] for L in range(1, depth + 1)])
    else:
        cell_first = cell_count = none
    return (u32(leaf_offsets), u32(order), u32(list_offsets), u32(near_s), u32(cell_first), u32(cell_count), u32(far_offsets), u32(far_c))


def adaptive_octree_cells(bodies: np.ndarray, dim: int, max_depth: int, leaf_capacity: int, theta: float, chunk_leaves: int = 16384):
    """An ADAPTIVE octree (quadtree in 2D) with near and far lists: the eight uint32 arrays of octree_cells, for
    nbx_leaf_plan_set_cells, and the specification of nbx_leaf_plan_create_octree_adaptive.  Root box, cells at `max_depth`, Morton
    keys and the stable body order are those of octree_cells(depth = max_depth).  A node is a key prefix at level L <= max_depth; the
    root is split when max_depth >= 1 and (leaf_capacity == 0 or n > leaf_capacity); a node of level L >= 1 exists when it is not
    empty and its parent is split; an existing node is a LEAF at L == max_depth or, for leaf_capacity > 0, when it holds at most
    leaf_capacity bodies, and is split otherwise.  Leaves are numbered in Morton order (every node is a contiguous leaf range); cells
    are the existing nodes of levels 1 .. max_depth, level by level, Morton order within a level -- every leaf is one of them.
    The walk of target leaf t uses the leaf's OWN node box: in units of the finest grid gap_d = max(0, node_lo - (t_lo + t_side),
    t_lo - (node_lo + node_side)), and a node is accepted (far list: coarse levels first, Morton order within a level) when
    float(node_side) < theta * sqrt(sum gap_d^2); a node that is not accepted goes to the near list when it is a leaf (t first, the
    others in leaf order) and is opened otherwise.  leaf_capacity = 0 gives octree_cells(depth = max_depth) word for word; an unsplit
    root gives one leaf, its near list itself, and no cells."""
    if not 0 <= int(max_depth) <= 10 or int(leaf_capacity) < 0 or not (theta >= 0.0 and np.isfinite(theta)):
        raise ValueError("max_depth in [0, 10], leaf_capacity >= 0, theta finite and >= 0")
    pos = np.asarray(bodies)[:, :dim]
    n, depth, cap = pos.shape[0], int(max_depth), int(leaf_capacity)
    u32 = lambda a: np.asarray(a, dtype=np.uint32)
    none = np.zeros(0, dtype=np.uint32)
    if n == 0:
        z = np.zeros(1, dtype=np.uint32)
        return z, none, z.copy(), none.copy(), none.copy(), none.copy(), z.copy(), none.copy()
    g = 1 << depth
    lo, hi = pos.min(axis=0), pos.max(axis=0)                      # root box and cells: octree_cells's expressions
    centre, half = (lo + hi) / 2.0, max(float((hi - lo).max()) / 2.0 * 1.01, 1e-300)
    cell = np.clip(np.floor((pos - (centre - half)) / (2.0 * half) * g).astype(np.int64), 0, g - 1)
    key = _morton_keys(cell, dim, depth)
    order = np.argsort(key, kind="stable")
    if not (depth >= 1 and (cap == 0 or n > cap)):                 # the root is not split
        return u32([0, n]), u32(order), u32([0, 1]), u32([0]), none, none.copy(), u32([0, 0]), none.copy()
    keys, first = np.unique(key[order], return_index=True)         # the finest level's runs
    nr = keys.size
    run_off = np.append(first, n)
    # every run's leaf level: the first level whose node holds at most `cap` bodies, else max_depth
    run_level = np.full(nr, depth, dtype=np.int64)
    if cap > 0:
        for L in range(depth - 1, 0, -1):                          # coarser levels overwrite finer ones: the first such level stays
            _, f, inv = np.unique(keys >> (dim * (depth - L)), return_index=True, return_inverse=True)
            count = run_off[np.append(f[1:], nr)] - run_off[f]
            small = count[inv] <= cap
            run_level[small] = L
    shift = dim * (depth - run_level)
    start = np.ones(nr, dtype=bool)
    start[1:] = (keys[1:] >> shift[1:]) != (keys[:-1] >> shift[1:])
    lead = np.nonzero(start)[0]
    nl = lead.size
    leaf_offsets, leaf_key, leaf_level = np.append(run_off[lead], n), keys[lead], run_level[lead]
    # the existing nodes of every level: keys (sorted), leaf ranges, coordinates, leaf or split, children (a range of the next level)
    lv_keys, lv_first, lv_count, lv_coords, lv_base, lv_leaf = {}, {}, {}, {}, {}, {}
    leaf_cell = np.zeros(nl, dtype=np.int64)                       # a leaf's own node within its level
    base = 0
    for L in range(1, depth + 1):
        s = dim * (depth - L)
        under = np.nonzero(leaf_level >= L)[0]
        kl, f = np.unique(leaf_key[under] >> s, return_index=True)
        fl = under[f]
        lv_keys[L], lv_first[L], lv_coords[L], lv_base[L] = kl, fl, _morton_coords(kl, dim, L), base
        lv_count[L] = np.searchsorted(leaf_key, (kl + 1) << s) - fl
        lv_leaf[L] = leaf_level[fl] == L
        leaf_cell[fl[lv_leaf[L]]] = np.nonzero(lv_leaf[L])[0]
        base += kl.size
    child_first, child_count = {}, {}
    for L in range(1, depth):
        child_first[L] = np.searchsorted(lv_keys[L + 1], lv_keys[L] << dim)
        child_count[L] = np.searchsorted(lv_keys[L + 1], (lv_keys[L] + 1) << dim) - child_first[L]
    t_side = np.int64(1) << (depth - leaf_level)                   # the target boxes, in units of the finest grid
    t_lo = np.zeros((nl, dim), dtype=np.int64)
    for L in range(1, depth + 1):
        at = np.nonzero(leaf_level == L)[0]
        t_lo[at] = lv_coords[L][leaf_cell[at]] << (depth - L)
    near_t, near_s, far_t, far_c = [], [], [], []
    for t0 in range(0, nl, max(1, int(chunk_leaves))):
        t1 = min(nl, t0 + max(1, int(chunk_leaves)))
        n1 = lv_keys[1].size
        t = np.repeat(np.arange(t0, t1, dtype=np.int64), n1)
        node = np.tile(np.arange(n1, dtype=np.int64), t1 - t0)
        ft, fc, nt, ns = [], [], [], []
        for L in range(1, depth + 1):
            s = depth - L
            blo = lv_coords[L][node] << s
            qlo, qs = t_lo[t], t_side[t][:, None]
            gap = np.maximum(0, np.maximum(blo - (qlo + qs), qlo - (blo + (1 << s))))
            acc = float(1 << s) < theta * np.sqrt((gap * gap).sum(axis=1).astype(np.float64))
            ft.append(t[acc]); fc.append(lv_base[L] + node[acc])
            t, node = t[~acc], node[~acc]
            is_leaf = lv_leaf[L][node]
            nt.append(t[is_leaf]); ns.append(lv_first[L][node[is_leaf]])
            t, node = t[~is_leaf], node[~is_leaf]
            if L == depth or t.size == 0:
                break
            cnt = child_count[L][node]
            begin = np.repeat(np.cumsum(cnt) - cnt, cnt)
            kid = np.repeat(child_first[L][node], cnt) + (np.arange(int(cnt.sum()), dtype=np.int64) - begin)
            t, node = np.repeat(t, cnt), kid
        nt, ns = np.concatenate(nt), np.concatenate(ns)
        by = np.lexsort((ns, ns != nt, nt))                        # per leaf: itself first, then the others in leaf order
        near_t.append(nt[by]); near_s.append(ns[by])
        ft, fc = np.concatenate(ft), np.concatenate(fc)
        by = np.argsort(ft, kind="stable")                         # per leaf: coarse levels first, Morton order within a level
        far_t.append(ft[by]); far_c.append(fc[by])
    near_t, near_s = np.concatenate(near_t), np.concatenate(near_s)
    far_t, far_c = np.concatenate(far_t), np.concatenate(far_c)
    list_offsets = np.concatenate([[0], np.cumsum(np.bincount(near_t, minlength=nl))])
    far_offsets = np.concatenate([[0], np.cumsum(np.bincount(far_t, minlength=nl))])
    cell_first = np.concatenate([lv_first[L] for L in range(1, depth + 1)])
    cell_count = np.concatenate([lv_count[L] for L in range(1, depth + 1)])
    return (u32(leaf_offsets), u32(order), u32(list_offsets), u32(near_s), u32(cell_first), u32(cell_count), u32(far_offsets), u32(far_c))


# ---- the far field's second-order term: the fp64 specification of NBX_FAR_QUADRUPOLE (include/nbody_hip.h) --------------------
# Plain numpy, nothing shared with the device code: these are what the tests hold csrc/leaf_far_kernel.hip to.

def _quad_pairs(dim: int):
    """Index pairs (a, b) of the stored moments: xx, yy, zz, xy, xz, yz in 3D; xx, yy, xy in 2D."""
    return ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)) if dim == 3 else ((0, 0), (1, 1), (0, 1))


def cell_moments(bodies: np.ndarray, dim: int, leaf_offsets, leaf_bodies, cell_first_leaf, cell_leaf_count, dtype=np.float64):
    """(M[n_cells], com[n_cells, dim], Q[n_cells, dim (dim + 1) / 2]) of cells given as leaf ranges: total mass, centre of mass and
    the central second moments Q_ab = sum m_j s_a s_b, s = p_j - com, summed directly about the centre (nothing cancels), in `dtype`.
    A cell without mass (empty, or every body massless) gives zeros."""
    lo, lb = np.asarray(leaf_offsets, dtype=np.int64), np.asarray(leaf_bodies, dtype=np.int64)
    cf, cc = np.asarray(cell_first_leaf, dtype=np.int64), np.asarray(cell_leaf_count, dtype=np.int64)
    pairs = _quad_pairs(dim)
    M, com, Q = np.zeros(cf.size, dtype=dtype), np.zeros((cf.size, dim), dtype=dtype), np.zeros((cf.size, len(pairs)), dtype=dtype)
    x_all, m_all = np.asarray(bodies[:, :dim], dtype=dtype), np.asarray(bodies[:, -1], dtype=dtype)
    for c in range(cf.size):
        ids = lb[lo[cf[c]]:lo[cf[c] + cc[c]]]
        m = m_all[ids]
        M[c] = m.sum()
        if M[c] == 0:
            continue
        com[c] = (m[:, None] * x_all[ids]).sum(axis=0) / M[c]
        s = x_all[ids] - com[c]
        for k, (a, b) in enumerate(pairs):
            Q[c, k] = (m * s[:, a] * s[:, b]).sum()
    return M, com, Q


def far_correction(R: np.ndarray, M, Q: np.ndarray, law: str = "reference", eps: float = 0.0) -> np.ndarray:
    """What a cell of mass M and central second moments Q (stored order) adds to the monopole term M R / r^4 for a target at
    -R from its centre of mass (R = com - p_i), per unit G m_i:
        (M / r^4) [ R (-2 tr(q) / r^2 + 12 R^T q R / r^4) - 4 q R / r^2 ],   q = Q / M.
    law="newton" (NBX_LAW_NEWTON, softening length eps): what it adds to M R / rho^3, rho^2 = r^2 + eps^2 -- the second-order term of
    the softened kernel, exactly:
        (M / rho^3) [ R (-(3/2) tr(q) / rho^2 + (15/2) R^T q R / rho^4) - 3 q R / rho^2 ].
    R[..., dim], M[...], Q[..., dim (dim + 1) / 2] broadcast together; zeros where M == 0."""
    if law not in ("reference", "newton"):
        raise ValueError("law must be 'reference' or 'newton'")
    R = np.asarray(R)
    dim = R.shape[-1]
    pairs = _quad_pairs(dim)
    M = np.asarray(M, dtype=R.dtype)
    Q = np.asarray(Q, dtype=R.dtype)
    live = M != 0
    q = Q / np.where(live, M, 1)[..., None]
    r2 = (R * R).sum(axis=-1)
    tr = q[..., 0] + q[..., 1] + (q[..., 2] if dim == 3 else 0)
    qR = np.zeros(np.broadcast(R, q[..., :1]).shape, dtype=R.dtype)
    for k, (a, b) in enumerate(pairs):
        qR[..., a] += q[..., k] * R[..., b]
        if a != b:
            qR[..., b] += q[..., k] * R[..., a]
    RqR = (R * qR).sum(axis=-1)
    if law == "newton":
        rho2 = r2 + R.dtype.type(eps) ** 2
        scalar = -1.5 * tr / rho2 + 7.5 * RqR / rho2 ** 2
        out = (M / (rho2 * np.sqrt(rho2)))[..., None] * (R * scalar[..., None] - 3 * qR / rho2[..., None])
        return np.where(live[..., None], out, 0)
    scalar = -2 * tr / r2 + 12 * RqR / r2 ** 2
    out = (M / r2 ** 2)[..., None] * (R * scalar[..., None] - 4 * qR / r2[..., None])
    return np.where(live[..., None], out, 0)


def far_sums(bodies: np.ndarray, dim: int, leaf_offsets, leaf_bodies, cell_first_leaf, cell_leaf_count, far_offsets, far_cells,
             order: int = 0, moments=None, law: str = "reference", eps: float = 0.0) -> np.ndarray:
    """Every body's far sum per unit G m_i, fp64: sum over the cells c of its leaf's far list of M_c R / r^4 (order 0), plus
    far_correction (order 1); law="newton": of M_c R / (r^2 + eps^2)^(3/2) and that law's far_correction.  No special case of any
    law is applied: far pairs are far.  moments: cell_moments' result, if at hand."""
    if law not in ("reference", "newton"):
        raise ValueError("law must be 'reference' or 'newton'")
    lo, lb = np.asarray(leaf_offsets, dtype=np.int64), np.asarray(leaf_bodies, dtype=np.int64)
    fo, fc = np.asarray(far_offsets, dtype=np.int64), np.asarray(far_cells, dtype=np.int64)
    M, com, Q = moments if moments is not None else cell_moments(bodies, dim, lo, lb, cell_first_leaf, cell_leaf_count)
    out = np.zeros((bodies.shape[0], dim))
    for t in range(lo.size - 1):
        ids, c = lb[lo[t]:lo[t + 1]], fc[fo[t]:fo[t + 1]]
        c = c[M[c] != 0]
        if not ids.size or not c.size:
            continue
        R = com[None, c, :] - bodies[ids, None, :dim]
        r2 = (R * R).sum(axis=2)
        if law == "newton":
            rho2 = r2 + float(eps) ** 2
            term = (M[c] / (rho2 * np.sqrt(rho2)))[..., None] * R
        else:
            term = (M[c] / r2 ** 2)[..., None] * R
        if order == 1:
            term = term + (far_correction(R, M[None, c], Q[None, c, :], law, eps) if law == "newton" else far_correction(R, M[None, c], Q[None, c, :]))
        out[ids] = term.sum(axis=1)
    return out


def near_sums(bodies: np.ndarray, dim: int, leaf_offsets, leaf_bodies, list_offsets, list_sources, eps: float):
    """The leaf sums of NBX_LAW_NEWTON per unit G m_i, fp64, plain numpy: for every body i of target leaf t,
        sum over the bodies j of the leaves on t's list (in list order; a repeated leaf counts twice) of m_j d / (r^2 + eps^2)^(3/2),
    d = p_j - p_i.  Every pair counts; i == j and coincident bodies add exactly 0.  Returns (sums[n, dim], S[n]) with the
    magnitude sums S_i = sum |m_j| |d| / (r^2 + eps^2)^(3/2), the scale of a backward-error bound on the fp32 pair terms.  Bodies
    in no leaf get zeros."""
    lo, lb = np.asarray(leaf_offsets, dtype=np.int64), np.asarray(leaf_bodies, dtype=np.int64)
    so, ss = np.asarray(list_offsets, dtype=np.int64), np.asarray(list_sources, dtype=np.int64)
    x, m = np.asarray(bodies[:, :dim], dtype=np.float64), np.asarray(bodies[:, -1], dtype=np.float64)
    e2 = float(eps) ** 2
    out, S = np.zeros((bodies.shape[0], dim)), np.zeros(bodies.shape[0])
    for t in range(lo.size - 1):
        ids = lb[lo[t]:lo[t + 1]]
        if not ids.size or so[t + 1] == so[t]:
            continue
        src = np.concatenate([lb[lo[l]:lo[l + 1]] for l in ss[so[t]:so[t + 1]]])
        if not src.size:
            continue
        xi = [x[ids, k][:, None] for k in range(dim)]
        for j0 in range(0, src.size, 8192):                       # bounded temporaries: [targets, 8192] per component
            sj = src[j0:j0 + 8192]
            d = [x[sj, k][None, :] - xi[k] for k in range(dim)]
            r2 = d[0] * d[0]
            for k in range(1, dim):
                r2 += d[k] * d[k]
            rho2 = r2 + e2
            w = m[None, sj] / (rho2 * np.sqrt(rho2))
            for k in range(dim):
                out[ids, k] += np.einsum("ij,ij->i", w, d[k])
            S[ids] += np.einsum("ij,ij->i", np.abs(w), np.sqrt(r2))
    return out, S


# ---- the potential through a plan: the fp64 specification of nbx_leaf_plan_energy / _potentials (include/nbody_hip.h) ----------
# Plain numpy, nothing shared with the device code: these are what the tests hold csrc/leaf_phi_kernel.hip to.  The laws' sums
# (near_sums, far_sums, the kernels) are the gradients of these with respect to the target's position.

_POTENTIAL_LAWS = {"newton": None, "brute": 1e-10, "tree_leaf": 1e-9, "reference": 1e-9}   # r^2 below which the law skips a pair


def _potential_law(law: str):
    if law not in _POTENTIAL_LAWS:
        raise ValueError("law must be 'newton', 'brute', 'tree_leaf' or 'reference' (= 'tree_leaf'); NBX_LAW_FMM_P2P has no potential")
    return _POTENTIAL_LAWS[law]


def near_potentials(bodies: np.ndarray, dim: int, leaf_offsets, leaf_bodies, list_offsets, list_sources, law: str, eps: float = 0.0):
    """Every body's near potential per unit G m_i, fp64: for body i of target leaf t, the sum over the bodies j != i of the leaves on
    t's list (a repeated leaf counts twice) of m_j w(r_ij):
        law="newton":              w = 1 / sqrt(r^2 + eps^2); the body ITSELF is left out (by identity), a different body at the
                                   same position counts m_j / eps;
        law="brute" / "tree_leaf": w = 1 / (2 r^2); pairs with r^2 < 1e-10 / 1e-9 are left out (the body itself among them).
    Returns (phi[n], S[n]) with S_i the sum of the terms' magnitudes, the scale of a backward-error bound on the fp32 pair terms.
    Bodies in no leaf get zeros."""
    skip = _potential_law(law)
    lo, lb = np.asarray(leaf_offsets, dtype=np.int64), np.asarray(leaf_bodies, dtype=np.int64)
    so, ss = np.asarray(list_offsets, dtype=np.int64), np.asarray(list_sources, dtype=np.int64)
    x, m = np.asarray(bodies[:, :dim], dtype=np.float64), np.asarray(bodies[:, -1], dtype=np.float64)
    e2 = float(eps) ** 2
    phi, S = np.zeros(bodies.shape[0]), np.zeros(bodies.shape[0])
    for t in range(lo.size - 1):
        ids = lb[lo[t]:lo[t + 1]]
        if not ids.size or so[t + 1] == so[t]:
            continue
        src = np.concatenate([lb[lo[l]:lo[l + 1]] for l in ss[so[t]:so[t + 1]]])
        for j0 in range(0, src.size, 8192):                       # bounded temporaries: [targets, 8192]
            sj = src[j0:j0 + 8192]
            r2 = np.zeros((ids.size, sj.size))
            for k in range(dim):
                d = x[sj, k][None, :] - x[ids, k][:, None]
                r2 += d * d
            if skip is None:
                w = np.where(sj[None, :] == ids[:, None], 0.0, m[None, sj] / np.sqrt(np.where(sj[None, :] == ids[:, None], 1.0, r2 + e2)))
            else:
                keep = r2 >= skip
                w = np.where(keep, 0.5 * m[None, sj] / np.where(keep, r2, 1.0), 0.0)
            phi[ids] += w.sum(axis=1)
            S[ids] += np.abs(w).sum(axis=1)
    return phi, S


def _far_quadratic_form(R: np.ndarray, q: np.ndarray):
    """(tr q, R^T q R) for q in the stored order."""
    dim = R.shape[-1]
    tr = q[..., 0] + q[..., 1] + (q[..., 2] if dim == 3 else 0)
    RqR = 0
    for k, (a, b) in enumerate(_quad_pairs(dim)):
        RqR = RqR + (1 if a == b else 2) * q[..., k] * R[..., a] * R[..., b]
    return tr, RqR


def far_potential_correction(R: np.ndarray, M, Q: np.ndarray, law: str = "reference", eps: float = 0.0) -> np.ndarray:
    """What a cell of mass M and central second moments Q (stored order) adds to its monopole potential for a target at -R from its
    centre of mass (R = com - p_i), per unit G m_i, with q = Q / M and t = tr q:
        reference laws:  (M / (2 r^2)) [ -t / r^2 + 4 R^T q R / r^4 ]                 on top of M / (2 r^2)
        law="newton":    (M / rho) [ -t / (2 rho^2) + (3/2) R^T q R / rho^4 ]         on top of M / rho, rho^2 = r^2 + eps^2.
    Its gradient with respect to p_i is far_correction.  R[..., dim], M[...], Q[..., dim (dim + 1) / 2] broadcast together; zeros
    where M == 0.  No skip is applied here (far_potentials does)."""
    newton = _potential_law(law) is None
    R = np.asarray(R, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    live = M != 0
    q = Q / np.where(live, M, 1)[..., None]
    tr, RqR = _far_quadratic_form(R, q)
    r2 = (R * R).sum(axis=-1)
    if newton:
        rho2 = r2 + float(eps) ** 2
        out = (M / np.sqrt(rho2)) * (-0.5 * tr / rho2 + 1.5 * RqR / rho2 ** 2)
    else:
        out = (0.5 * M / r2) * (-tr / r2 + 4.0 * RqR / r2 ** 2)
    return np.where(live, out, 0.0)


def far_potentials(bodies: np.ndarray, dim: int, leaf_offsets, leaf_bodies, cell_first_leaf, cell_leaf_count, far_offsets, far_cells,
                   order: int = 0, law: str = "reference", eps: float = 0.0, moments=None):
    """Every body's far potential per unit G m_i, fp64: the sum over the cells c of its leaf's far list of M_c / (2 r^2) (reference
    laws) or M_c / sqrt(r^2 + eps^2) (law="newton"), plus far_potential_correction at order 1.  Where a reference law skips the pair
    with the pseudo-body (r^2 below its threshold) the whole term is 0; a massless cell adds 0.  Returns (phi[n], S[n]), S_i the sum
    of the terms' magnitudes.  moments: cell_moments' result, if at hand."""
    skip = _potential_law(law)
    lo, lb = np.asarray(leaf_offsets, dtype=np.int64), np.asarray(leaf_bodies, dtype=np.int64)
    fo, fc = np.asarray(far_offsets, dtype=np.int64), np.asarray(far_cells, dtype=np.int64)
    M, com, Q = moments if moments is not None else cell_moments(bodies, dim, lo, lb, cell_first_leaf, cell_leaf_count)
    phi, S = np.zeros(bodies.shape[0]), np.zeros(bodies.shape[0])
    for t in range(lo.size - 1):
        ids, c = lb[lo[t]:lo[t + 1]], fc[fo[t]:fo[t + 1]]
        c = c[M[c] != 0]
        if not ids.size or not c.size:
            continue
        R = com[None, c, :] - np.asarray(bodies[ids, None, :dim], dtype=np.float64)
        r2 = (R * R).sum(axis=2)
        if skip is None:
            term = M[None, c] / np.sqrt(r2 + float(eps) ** 2)
        else:
            term = 0.5 * M[None, c] / np.where(r2 >= skip, r2, 1.0)
        if order == 1:
            term = term + far_potential_correction(np.where((r2 > 0)[..., None], R, 1.0), M[None, c], Q[None, c, :], law, eps)
        if skip is not None:
            term = np.where(r2 >= skip, term, 0.0)
        phi[ids] = term.sum(axis=1)
        S[ids] = np.abs(term).sum(axis=1)
    return phi, S


# ---- the leapfrog through a plan: the fp64 specification of nbx_leaf_plan_step / _step_kdk (include/nbody_hip.h) ------------------

def leapfrog_spec(bodies: np.ndarray, accel_fn, dt: float, nsteps: int, scheme: str = "kdk") -> np.ndarray:
    """`nsteps` leapfrog steps of Body<D> rows (position[D], velocity[D], mass) in fp64 numpy; returns the new rows, `bodies` stays.
    accel_fn(rows) -> a[n, D], the accelerations F_i / m_i of the rows as they stand, G and sign included -- an all-pairs sum, or
    near_sums + far_sums through a structure, both fit.
        scheme="kd":   nsteps x { a; v += a dt; x += v dt } -- the reference helpers' order (nbx_leaf_plan_step): first order, and
                       v is half a step behind x in the second-order reading.
        scheme="kdk":  a K(dt/2) D(dt) [ a K(dt) D(dt) ]^(nsteps-1) a K(dt/2), adjacent half-kicks merged into one multiply by dt
                       (nbx_leaf_plan_step_kdk): nsteps + 1 evaluations, second order, time-reversible, x and v at one time."""
    if scheme not in ("kd", "kdk"):
        raise ValueError("scheme must be 'kd' or 'kdk'")
    if nsteps < 0:
        raise ValueError("nsteps must be >= 0")
    b = np.array(bodies, dtype=np.float64, copy=True)
    dim = (b.shape[1] - 1) // 2
    x, v = b[:, :dim], b[:, dim:2 * dim]                         # views: accel_fn sees the rows as they stand
    if nsteps == 0:
        return b
    if scheme == "kd":
        for _ in range(nsteps):
            v += np.asarray(accel_fn(b), dtype=np.float64) * dt
            x += v * dt
        return b
    for e in range(nsteps + 1):
        v += np.asarray(accel_fn(b), dtype=np.float64) * (0.5 * dt if e in (0, nsteps) else dt)
        if e < nsteps:
            x += v * dt
    return b


# ---- the variable-step leapfrog: the fp64 specification of nbx_leaf_plan_step_kdk_adaptive (include/nbody_hip.h) ------------------

def choose_step(a_max: float, accel_length: float, dt_min: float, dt_max: float, pow2: bool = False) -> float:
    """The step the adaptive loop chooses from the largest acceleration of an evaluation: raw = sqrt(accel_length / a_max), +inf for
    a_max == 0; clamped to [dt_min, dt_max], or with pow2 dt_max halved while it is above raw and the half is not below dt_min.  One
    fp64 division, one square root, comparisons and exact halvings: the device's operations in the device's order."""
    a_max, c = np.float64(a_max), np.float64(accel_length)
    dt_min, dt_max = np.float64(dt_min), np.float64(dt_max)
    raw = np.float64(np.inf) if a_max == 0.0 else np.sqrt(c / a_max)
    if pow2:
        d = dt_max
        while d > raw and np.float64(0.5) * d >= dt_min:
            d = np.float64(0.5) * d
        return float(d)
    return float(min(max(raw, dt_min), dt_max))


def adaptive_leapfrog_spec(bodies: np.ndarray, accel_fn, control: dict, max_steps: int, in_leaf=None):
    """nbx_leaf_plan_step_kdk_adaptive in fp64 numpy, next to leapfrog_spec and with its accel_fn.  control: a dict with accel_length,
    dt_min, dt_max and optionally t_start (0), t_end (inf), pow2 (False).  in_leaf: a mask of the bodies that belong to a leaf (all,
    if None); the others count 0 towards a_max, as on the device, where they have no sums.  Returns (rows, clock, history):
    the new rows; clock, a dict with the fields of nbx_step_clock; history, an array [k, 2] of the recorded (a_max, dt).
        t = t_start; prev = 0; steps = 0
        for every evaluation:  a_max not finite -> status 1, stop, no kick
                               t >= t_end or steps == max_steps -> v += a (0.5 prev); record (a_max, 0); stop
                               dt = choose_step(a_max); landing on t_end when dt >= t_end - t
                               v += a (0.5 prev + 0.5 dt); x += v dt; prev = dt; steps += 1; record (a_max, dt)"""
    if max_steps < 0:
        raise ValueError("max_steps must be >= 0")
    c, dt_min, dt_max = (float(control[k]) for k in ("accel_length", "dt_min", "dt_max"))
    t_start, t_end, pow2 = float(control.get("t_start", 0.0)), float(control.get("t_end", np.inf)), bool(control.get("pow2", False))
    if not (c > 0 and np.isfinite(c) and 0 < dt_min <= dt_max and np.isfinite(dt_max) and np.isfinite(t_start)) or np.isnan(t_end) or t_end == -np.inf:
        raise ValueError("control outside the ranges of nbx_step_control")
    b = np.array(bodies, dtype=np.float64, copy=True)
    dim = (b.shape[1] - 1) // 2
    x, v = b[:, :dim], b[:, dim:2 * dim]
    clock = {"t": t_start, "dt_last": 0.0, "a_max_last": 0.0, "steps": 0, "evaluations": 0, "finished": 0, "status": 0}
    history = []
    if max_steps == 0:
        return b, clock, np.zeros((0, 2))
    t, prev, steps = np.float64(t_start), np.float64(0.0), 0
    half = np.float64(0.5)
    while True:
        a = np.asarray(accel_fn(b), dtype=np.float64)
        mag = np.sqrt((a * a).sum(axis=1))
        if in_leaf is not None:
            mag = np.where(in_leaf, mag, 0.0)
        a_max = np.float64(np.nan) if np.isnan(mag).any() else np.float64(mag.max() if mag.size else 0.0)   # a NaN orders above infinity
        clock["evaluations"] += 1
        clock["a_max_last"] = float(a_max)
        if not np.isfinite(a_max):
            clock["status"] = 1
            break
        if in_leaf is not None:
            a = np.where(np.asarray(in_leaf)[:, None], a, 0.0)
        if t >= t_end or steps == max_steps:
            if prev != 0.0:
                v += a * (half * prev)
            history.append((float(a_max), 0.0))
            clock["finished"] = 1 if t >= t_end else 0
            break
        dt = np.float64(choose_step(a_max, c, dt_min, dt_max, pow2))
        if dt >= t_end - t:
            dt, t = np.float64(t_end - t), np.float64(t_end)
        else:
            t = t + dt
        v += a * (half * prev + half * dt)
        x += v * dt
        prev = dt
        steps += 1
        history.append((float(a_max), float(dt)))
    clock.update(t=float(t), dt_last=float(prev), steps=steps)
    return b, clock, np.array(history, dtype=np.float64).reshape(-1, 2)
