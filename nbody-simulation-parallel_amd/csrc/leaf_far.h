// leaf_far.h -- the far field of a leaf plan (include/nbody_hip.h nbx_leaf_plan_set_cells): CELLS (contiguous ranges of leaves) whose
// total mass and centre of mass are recomputed on the device in every evaluation, and per target leaf a FAR LIST of cells that
// attract the leaf's bodies as one pseudo-body each (octree.cpp:129-151, bvh.cpp:203-239).
// This header is the host side: validation of the caller's arrays and the layout the kernels of leaf_far_kernel.hip follow.  The
// part above the __HIPCC__ guard is plain C++ (tests/test_far_field_cpu.py compiles it with g++ under ASan / UBSan).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace nbx_far {

constexpr uint32_t kFarTile = 256;         // cell records a wave stages in LDS at a time (4 KB); longer far lists go in chunks
constexpr uint32_t kFarMaxLanes = 16;      // lanes that share one target (they split the tile's records between them)
constexpr uint32_t kFarTilePad = 4 * kFarMaxLanes;   // massless records behind a tile's last one: the lane groups' shares are rounded up to an odd number of record pairs
constexpr uint32_t kSmallCell = 8;         // a cell of up to this many leaves is summed by ONE lane, a larger one by a workgroup
constexpr uint32_t kCellThreads = 256;     // lanes of the workgroup that sums one large cell
constexpr uint32_t kLeafLanes = 8;         // lanes that sum one leaf's slots

// One wave64 of the far pass: `count` consecutive targets (padded slots of ONE leaf) against the leaf's far list.
struct FarBlock {
    uint32_t first, count;      // targets: padded slots [first, first + count), count <= 64
    uint32_t far_lo, far_n;     // the leaf's far list: far_cells[far_lo .. far_lo + far_n)
};
static_assert(sizeof(FarBlock) == 16, "read with one 16-byte load");

struct FarPlan {
    std::vector<FarBlock> blocks;        // longest far list first
    std::vector<uint32_t> small_cells;   // cells of <= kSmallCell leaves (one lane each) ...
    std::vector<uint32_t> big_cells;     // ... and the others (one workgroup each)
    size_t far_entries = 0;
};

// Everything the kernels will follow is checked here, before anything is launched.  Returns nullptr, or why the arrays are refused.
inline const char* validate_cells(size_t n_leaves, const uint32_t* cell_first_leaf, const uint32_t* cell_leaf_count, size_t n_cells,
                                  const uint32_t* far_offsets, const uint32_t* far_cells) {
    if (n_cells > ((size_t)1 << 31)) return "too many cells";
    if (n_cells && (!cell_first_leaf || !cell_leaf_count)) return "null cell arrays";
    for (size_t c = 0; c < n_cells; ++c)
        if ((uint64_t)cell_first_leaf[c] + (uint64_t)cell_leaf_count[c] > (uint64_t)n_leaves) return "a cell's leaf range runs past n_leaves";
    if (!far_offsets) return (n_cells && n_leaves) ? "null far_offsets" : nullptr;   // no cells (or no leaves): nothing to name them
    if (!n_leaves) return nullptr;
    if (far_offsets[0] != 0) return "far_offsets must start at 0";
    for (size_t l = 0; l < n_leaves; ++l)
        if (far_offsets[l + 1] < far_offsets[l]) return "far_offsets must be non-decreasing";
    const size_t entries = far_offsets[n_leaves];
    if (entries > 0xfffffff0ull) return "far lists too long";
    if (entries && !far_cells) return "null far_cells";
    uint32_t largest = 0;                                    // no exit inside the loop: vectorised (10^8 entries at N = 2^20)
    for (size_t e = 0; e < entries; ++e) largest = far_cells[e] > largest ? far_cells[e] : largest;
    if (entries && largest >= n_cells) return "far_cells entry out of range";
    return nullptr;
}

// unit_off[n_leaves + 1]: first padded slot of every leaf (leaf_plan.h; a leaf of odd size ends in a massless pad slot, which the
// far pass treats as a target like the others: its terms are exact zeros).  The arrays must have passed validate_cells.
inline void plan_far(const uint32_t* unit_off, size_t n_leaves, const uint32_t* cell_leaf_count, size_t n_cells, const uint32_t* far_offsets,
                     FarPlan& out) {
    out.blocks.clear(); out.small_cells.clear(); out.big_cells.clear();
    out.far_entries = (n_cells && n_leaves && far_offsets) ? far_offsets[n_leaves] : 0;
    for (size_t c = 0; c < n_cells; ++c) (cell_leaf_count[c] <= kSmallCell ? out.small_cells : out.big_cells).push_back((uint32_t)c);
    if (!out.far_entries) return;
    for (size_t l = 0; l < n_leaves; ++l) {
        const uint32_t c = unit_off[l + 1] - unit_off[l], far_n = far_offsets[l + 1] - far_offsets[l];
        if (!c || !far_n) continue;
        const uint32_t groups = (c + 63u) / 64u;
        uint32_t f = unit_off[l];
        for (uint32_t g = 0; g < groups; ++g) {
            const uint32_t share = c / groups + (g < c % groups ? 1u : 0u);   // <= 64
            out.blocks.push_back(FarBlock{f, share, far_offsets[l], far_n});
            f += share;
        }
    }
    // longest first (workgroups are dispatched in index order: the launch then drains in a fraction of a mean wave's time), leaf
    // order among equals
    std::stable_sort(out.blocks.begin(), out.blocks.end(), [](const FarBlock& a, const FarBlock& b) { return a.far_n > b.far_n; });
}

}  // namespace nbx_far

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
namespace nbx_far {

// Device arrays of a plan's cells (one allocation) and what an evaluation's two passes read and write.
struct FarDevice {
    const float4* xp = nullptr;            // the plan's leaf-ordered source pairs
    const uint32_t* unit_off = nullptr;    // [n_leaves + 1]
    double* sums = nullptr;                // [dim][pslots] -- the far terms are ADDED behind the pair kernel
    uint32_t pslots = 0, n_leaves = 0, n_cells = 0, n_small = 0, n_big = 0, n_blocks = 0;
    const uint32_t* cell_first = nullptr;  // [n_cells]
    const uint32_t* cell_count = nullptr;  // [n_cells]
    const uint32_t* small_cells = nullptr; // [n_small]
    const uint32_t* big_cells = nullptr;   // [n_big]
    const uint32_t* far_cells = nullptr;   // [far_entries]
    const FarBlock* blocks = nullptr;      // [n_blocks]
    double* leaf_mom = nullptr;            // [n_leaves][4]: sum m, sum m x, sum m y, sum m z
    double* cell_mass = nullptr;           // [n_cells]       fp64 moments as the far pass used them, before the fp32 rounding
    double* cell_com = nullptr;            // [n_cells][dim]
    float4* cell_rec = nullptr;            // [n_cells] {x, y, z, M} fp32: the pseudo-bodies
    // ---- order 1 (NBX_FAR_QUADRUPOLE) only; a plan at order 0 leaves all of it null and its passes never look ----
    int order = 0;
    double* leaf_quad = nullptr;           // [n_leaves][6]: central second moments of a leaf about its OWN centre of mass (3D order; 2D uses xx, yy, xy)
    double* cell_quad = nullptr;           // [n_cells][dim (dim + 1) / 2] fp64 Q as the far pass used them, before the division by M and the fp32 rounding
    float4* cell_qrec = nullptr;           // [n_cells][quad_rec_vecs(dim)] fp32 q = Q / M and its trace, next to cell_rec
    // ---- NBX_LAW_NEWTON only: the plan's softening length squared, set per far pass (no other law reads it) ----
    float eps2 = 0.0f;
};

// The fp32 record of a cell's second moments, q = Q / M (all zeros: the cell attracts as its monopole alone):
//   3D: {xx, yy, zz, xy}, {xz, yz, tr q, 0} -- with cell_rec 48 bytes per cell, three 16-byte loads;   2D: {xx, yy, xy, tr q} -- 32 bytes.
constexpr uint32_t quad_rec_vecs(int dim) { return dim == 3 ? 2u : 1u; }
constexpr uint32_t quad_count(int dim) { return (uint32_t)(dim * (dim + 1) / 2); }

// per-leaf moments, then every cell's (fixed summation order, no atomics); at d.order == 1 the second moments behind them
hipError_t enqueue_moments(const FarDevice& d, int dim, hipStream_t s);
// the far terms of every target, added into d.sums (d.order: monopoles, or monopoles + the second-order term)
hipError_t enqueue_far(const FarDevice& d, int dim, int law, hipStream_t s);

}  // namespace nbx_far
#endif
