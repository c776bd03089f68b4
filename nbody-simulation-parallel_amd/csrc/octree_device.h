// octree_device.h -- the fixed-depth octree of leaves.octree_cells (host/leaf_pairs_hip.cpp build_octree_cells<D>) built ON THE
// DEVICE from a context's resident fp64 positions: the eight arrays of the host builder, word for word, without the bodies or the
// tree crossing PCIe (nbx_leaf_plan_create_octree, nbx_leaf_plan_rebuild_octree).
//
// The part above the __HIPCC__ guard is plain C++: the root box, the cell index and the Morton key in ONE definition that the
// device kernels and a g++ build (tests/test_octree_build_cpu.py, under ASan / UBSan) both compile.  It must round exactly like
// numpy's  clip(floor((x - (centre - half)) / (2 * half) * 2^depth), 0, 2^depth - 1):  the same fp64 operations in the same
// order, no contraction into fused multiply-adds (-ffp-contract=off for every unit that CALLS them), IEEE division.
//
//   stage (octree_device.hip)   kernels                                            host builder's counterpart (leaves.py)
//   bounding box, root box      ot_bbox_partial, ot_bbox_final                      pos.min / pos.max, centre, half
//   keys, order                 ot_keys, ceil(dim depth / 8) radix passes           _morton_keys, argsort(kind="stable")
//   leaves                      ot_flags, scan, ot_leaves                           np.unique(key[order], return_index)
//   levels 1 .. depth           per level ot_level_flags + scan; ot_level_bases,    np.unique(keys >> ..), searchsorted (children)
//                               ot_cells, ot_cell_ends, one radix pass (small | big)
//   walk, counting              ot_walk<false> (one lane per target leaf), 2 scans  the level-synchronous frontier
//   -- 64 bytes to the host: the counts size the plan's arena --
//   walk, filling               ot_walk<true>                                       lexsort / stable argsort of the frontier's output
//   far layout                  ot_far_blocks, radix passes by far-list length,     leaf_far.h plan_far
//                               ot_far_deal
// The ADAPTIVE tree of leaves.adaptive_octree_cells (nbx_leaf_plan_create_octree_adaptive) shares the first two stages, run at
// max_depth, and everything after the walk; between them (ota_* kernels):
//   leaf level of every run     per level ot_flags + scan, ota_node_starts,         np.unique(.., return_inverse), count <= capacity
//                               ota_run_level
//   leaves                      ota_leaf_flags, scan, ota_leaves                    runs of equal (leaf level, prefix)
//   existing nodes per level    per level ota_level_flags + scan; ot_level_bases,   np.unique over the leaves of level >= L
//                               ota_cells (count: a binary search), one radix pass
//   walk                        ot_walk<FILL, true>: stops at a leaf of any level,  the frontier with lv_leaf and the leaves' own boxes
//                               accepts_box with the target leaf's own side
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define NBX_OT_HD __host__ __device__
#else
#define NBX_OT_HD
#endif

namespace nbx_octree {

constexpr int kMaxDepth = 10;   // 3 x 10 key bits in a 32-bit word; the same bound holds in 2D

// the root box of the builder: origin = centre - half per axis, side = 2 * half
struct RootBox {
    double origin[3];
    double side;
};

// lo / hi: the bodies' bounding box (exact fp64 minima and maxima)
NBX_OT_HD inline RootBox root_box(const double* lo, const double* hi, int dim) {
    double widest = hi[0] - lo[0];
    for (int d = 1; d < dim; ++d) widest = (hi[d] - lo[d]) > widest ? (hi[d] - lo[d]) : widest;
    double half = widest / 2.0 * 1.01;
    half = half > 1e-300 ? half : 1e-300;
    RootBox b;
    for (int d = 0; d < 3; ++d) b.origin[d] = d < dim ? (lo[d] + hi[d]) / 2.0 - half : 0.0;
    b.side = 2.0 * half;
    return b;
}

// clip(floor((x - origin) / side * 2^depth), 0, 2^depth - 1)
NBX_OT_HD inline uint32_t cell_index(double x, double origin, double side, int depth) {
    const double g = (double)(1u << depth);
    const double t = floor((x - origin) / side * g);
    if (!(t > 0.0)) return 0u;                       // negative, zero, or not a number
    if (t >= g) return (1u << depth) - 1u;
    return (uint32_t)t;
}

// bit b of axis d lands at bit b * dim + (dim - 1 - d)
NBX_OT_HD inline uint32_t morton_key(const uint32_t* cell, int dim, int depth) {
    uint32_t key = 0;
    for (int bit = 0; bit < depth; ++bit)
        for (int d = 0; d < dim; ++d) key |= ((cell[d] >> bit) & 1u) << (bit * dim + (dim - 1 - d));
    return key;
}

// a node's coordinates from its key, packed 10 bits per axis (x | y << 10 | z << 20)
NBX_OT_HD inline uint32_t packed_coords(uint32_t key, int dim, int level) {
    uint32_t out = 0;
    for (int bit = 0; bit < level; ++bit)
        for (int d = 0; d < dim; ++d) out |= ((key >> (bit * dim + (dim - 1 - d))) & 1u) << (10 * d + bit);
    return out;
}

NBX_OT_HD inline uint32_t body_key(const double* x, const RootBox& box, int dim, int depth) {
    uint32_t cell[3] = {0u, 0u, 0u};
    for (int d = 0; d < dim; ++d) cell[d] = cell_index(x[d], box.origin[d], box.side, depth);
    return morton_key(cell, dim, depth);
}

// The acceptance test of the walk on integer boxes: q = the target leaf's cell, node = a level-L node's cell (s = depth - L).
NBX_OT_HD inline bool accepts(uint32_t q_packed, uint32_t node_packed, int dim, int s, double theta) {
    long long sum = 0;
    for (int d = 0; d < dim; ++d) {
        const long long q = (q_packed >> (10 * d)) & 1023u, blo = (long long)((node_packed >> (10 * d)) & 1023u) << s;
        long long gap = blo - (q + 1);
        const long long other = q - (blo + (1ll << s));
        gap = gap > other ? gap : other;
        gap = gap > 0 ? gap : 0;
        sum += gap * gap;
    }
    return (double)(1ll << s) < theta * sqrt((double)sum);
}

// The same test for a target that is a node of ANY level (the adaptive tree): t = the target leaf's cell at its own level, st =
// max_depth - that level, so its box is [t << st, (t << st) + 2^st) in units of the finest grid.  st = 0 is accepts().
NBX_OT_HD inline bool accepts_box(uint32_t t_packed, int st, uint32_t node_packed, int dim, int s, double theta) {
    long long sum = 0;
    for (int d = 0; d < dim; ++d) {
        const long long q = (long long)((t_packed >> (10 * d)) & 1023u) << st, blo = (long long)((node_packed >> (10 * d)) & 1023u) << s;
        long long gap = blo - (q + (1ll << st));
        const long long other = q - (blo + (1ll << s));
        gap = gap > other ? gap : other;
        gap = gap > 0 ? gap : 0;
        sum += gap * gap;
    }
    return (double)(1ll << s) < theta * sqrt((double)sum);
}

// The adaptive tree's root is split (otherwise: one leaf, no cells).  leaf_capacity = 0: the fixed-depth tree.
NBX_OT_HD inline bool root_is_split(size_t n, int max_depth, size_t leaf_capacity) { return max_depth >= 1 && (leaf_capacity == 0 || n > leaf_capacity); }

}  // namespace nbx_octree

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "leaf_far.h"

namespace nbx_octree {

// What the host reads back after the counting walk (one copy of 64 bytes): it sizes the plan's and the cells' arenas.
struct Counts {
    uint32_t bad;                    // a coordinate was not finite: nothing below means anything
    uint32_t n_leaves;
    uint32_t n_cells;
    uint32_t n_small;                // cells of <= nbx_far::kSmallCell leaves
    unsigned long long near_entries;
    unsigned long long far_entries;
    uint32_t far_blocks;             // waves of the far pass (leaf_far.h plan_far)
    uint32_t n;                      // the bodies (the sort's count word)
    uint32_t n_runs;                 // adaptive tree: the non-empty cells of the finest grid (its leaves are unions of them)
    uint32_t pad_[5];
};
static_assert(sizeof(Counts) == 64, "one cache line, copied back whole");

// The tree's own device block: everything whose size follows from n, dim and depth alone.  Offsets in bytes.
struct TreeLayout {
    size_t counts, box, partial, level_base;
    size_t key_a, key_b, val_a, val_b, hist, tile_sums, flags;
    size_t leaf_offsets, leaf_keys, list_offsets, far_offsets, near_cnt, far_cnt, level_far;
    size_t rank;                     // [depth + 1][nl_max + 1]: a leaf's node at every level
    size_t cell_first, cell_count, cell_coords, child_first, child_end, cell_key, cell_key2, cell_id, cells_split;
    size_t far_blk_cnt, far_blk_off;
    size_t run_off, run_keys, run_level, node_at, node_start, leaf_level;   // the adaptive tree only (0 otherwise)
    size_t total;
    size_t nl_max, cells_max;
};
TreeLayout make_tree_layout(size_t n, int dim, int depth, bool adaptive = false);

struct Tree {                        // device pointers into the tree block, for the plan to keep
    Counts* counts = nullptr;
    const uint32_t* leaf_offsets = nullptr;   // [n_leaves + 1]
    const uint32_t* leaf_bodies = nullptr;    // [n]
    const uint32_t* list_offsets = nullptr;   // [n_leaves + 1]
    const uint32_t* far_offsets = nullptr;    // [n_leaves + 1]
    const uint32_t* cell_first = nullptr;     // [n_cells]
    const uint32_t* cell_count = nullptr;     // [n_cells]
    const uint32_t* small_cells = nullptr;    // [n_small], then the big ones
};

// bounding box ... counting walk, and the counts into *counts_host (asynchronous; synchronise the stream before reading)
hipError_t enqueue_build(const double* x64, size_t pad, size_t n, int dim, int depth, double theta, char* block, const TreeLayout& L,
                         hipStream_t s, Counts* counts_host, Tree* tree);
// the filling walk: list_sources[near_entries], far_cells[far_entries]
hipError_t enqueue_fill(size_t n, int dim, int depth, double theta, char* block, const TreeLayout& L, uint32_t* list_sources, uint32_t* far_cells,
                        hipStream_t s);
// The ADAPTIVE tree (leaves.adaptive_octree_cells; leaf_capacity > 0, a layout made with adaptive = true): bounding box, keys, sort
// and finest runs as above at depth = max_depth; then per level the nodes' body counts from the runs' offsets, every run's leaf
// level, the leaves as runs of equal (level, prefix), the existing nodes per level, and the same walk stopping at a leaf of any
// level and testing with the target leaf's own box.  Everything downstream (enqueue_far_layout, the plan) is shared.
hipError_t enqueue_build_adaptive(const double* x64, size_t pad, size_t n, int dim, int max_depth, size_t leaf_capacity, double theta, char* block,
                                  const TreeLayout& L, hipStream_t s, Counts* counts_host, Tree* tree);
hipError_t enqueue_fill_adaptive(size_t n, int dim, int max_depth, size_t leaf_capacity, double theta, char* block, const TreeLayout& L,
                                 uint32_t* list_sources, uint32_t* far_cells, hipStream_t s);
// plan_far's blocks on the device (unit_off: the planner's padded slots): far_blocks of them, longest far list first; scratch:
// 4 x far_blocks words + one FarBlock array of the same length
size_t far_scratch_bytes(size_t far_blocks);
hipError_t enqueue_far_layout(const uint32_t* unit_off, const Counts& counts, char* block, const TreeLayout& L, nbx_far::FarBlock* blocks, char* scratch,
                              hipStream_t s);

}  // namespace nbx_octree
#endif
