// octree_device.hip -- the kernels behind octree_device.h: a fixed-depth octree with near and far lists, built from resident
// fp64 positions on one stream.  Every kernel is launched for an upper bound known to the host (n, min(n, 2^(dim depth)) leaves,
// the cells of full levels) and reads its actual count from device memory, as the kernels of device_sort.h and
// leaf_plan_device.h do; the host reads 64 bytes back between the counting and the filling walk, and nothing else.
// Compiled with -ffp-contract=off: the cell index must round as the host builder's numpy expression does.
#include "octree_device.h"

#include <algorithm>
#include <cfloat>

#include "device_sort.h"

namespace nbx_octree {

namespace {
using namespace nbx_sort;

constexpr unsigned kBoxBlocks = 256;    // partial bounding boxes of the first reduction pass
constexpr unsigned kWalkLanes = 64;     // target leaves per workgroup of the walk: one wave

__device__ __forceinline__ void block_min_max(double* lo, double* hi, double (*slo)[256], double (*shi)[256], int dim) {
    for (int d = 0; d < dim; ++d) { slo[d][threadIdx.x] = lo[d]; shi[d][threadIdx.x] = hi[d]; }
    __syncthreads();
    for (unsigned w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w)
            for (int d = 0; d < dim; ++d) {
                slo[d][threadIdx.x] = fmin(slo[d][threadIdx.x], slo[d][threadIdx.x + w]);
                shi[d][threadIdx.x] = fmax(shi[d][threadIdx.x], shi[d][threadIdx.x + w]);
            }
        __syncthreads();
    }
    for (int d = 0; d < dim; ++d) { lo[d] = slo[d][0]; hi[d] = shi[d][0]; }
}

// partial[b] = {lo[3], hi[3]} of the bodies workgroup b strides over; a coordinate that is not finite sets Counts::bad
__global__ __launch_bounds__(256) void ot_bbox_partial_kernel(const double* __restrict__ x64, size_t pad, uint32_t n, int dim, double* __restrict__ partial,
                                                              Counts* C) {
    __shared__ double slo[3][256], shi[3][256];
    double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    bool bad = false;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u)
        for (int d = 0; d < dim; ++d) {
            const double x = x64[(size_t)d * pad + i];
            bad |= !(fabs(x) <= DBL_MAX);
            lo[d] = fmin(lo[d], x);
            hi[d] = fmax(hi[d], x);
        }
    if (bad) atomicOr(&C->bad, 1u);
    block_min_max(lo, hi, slo, shi, dim);
    if (threadIdx.x == 0)
        for (int d = 0; d < dim; ++d) { partial[blockIdx.x * 6u + d] = lo[d]; partial[blockIdx.x * 6u + 3u + d] = hi[d]; }
}

__global__ __launch_bounds__(256) void ot_bbox_final_kernel(const double* __restrict__ partial, unsigned blocks, int dim, RootBox* __restrict__ box) {
    __shared__ double slo[3][256], shi[3][256];
    double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    for (unsigned b = threadIdx.x; b < blocks; b += 256u)
        for (int d = 0; d < dim; ++d) { lo[d] = fmin(lo[d], partial[b * 6u + d]); hi[d] = fmax(hi[d], partial[b * 6u + 3u + d]); }
    block_min_max(lo, hi, slo, shi, dim);
    if (threadIdx.x == 0) *box = root_box(lo, hi, dim);
}

__global__ __launch_bounds__(256) void ot_keys_kernel(const double* __restrict__ x64, size_t pad, uint32_t n, int dim, int depth, const RootBox* __restrict__ box,
                                                      uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const RootBox b = *box;
    double x[3] = {0.0, 0.0, 0.0};
    for (int d = 0; d < dim; ++d) x[d] = x64[(size_t)d * pad + i];
    keys[i] = body_key(x, b, dim, depth);
    vals[i] = i;
}

// flag[i] = element i starts a run of equal (keys[i] >> shift); `count` elements
__global__ __launch_bounds__(256) void ot_flags_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ count, uint32_t capacity, int shift,
                                                       uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n = *count < capacity ? *count : capacity;
    if (i >= n) return;
    flags[i] = (i == 0u || (keys[i] >> shift) != (keys[i - 1u] >> shift)) ? 1u : 0u;
}

// the leaves: runs of equal keys among the sorted bodies.  rank = the exclusive scan of the run starts (rank[n] = their number)
__global__ __launch_bounds__(256) void ot_leaves_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ rank, uint32_t n,
                                                        uint32_t* __restrict__ leaf_offsets, uint32_t* __restrict__ leaf_keys, Counts* C) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (i == 0u) { const uint32_t nl = rank[n]; leaf_offsets[nl] = n; C->n_leaves = nl; }
    if (i == 0u || keys[i] != keys[i - 1u]) { leaf_offsets[rank[i]] = i; leaf_keys[rank[i]] = keys[i]; }
}

// level_base[L] = first cell of level L (levels 1 .. depth; level_base[depth + 1] = the number of cells)
__global__ void ot_level_bases_kernel(const uint32_t* __restrict__ rank, size_t rank_stride, int depth, uint32_t* __restrict__ level_base, Counts* C) {
    const uint32_t nl = C->n_leaves;
    uint32_t base = 0;
    level_base[0] = 0u;
    for (int L = 1; L <= depth; ++L) { level_base[L] = base; base += rank[(size_t)L * rank_stride + nl]; }
    level_base[depth + 1] = base;
    C->n_cells = base;
}

// one lane per (level, leaf): the leaf that starts a node of the level writes the node's cell
__global__ __launch_bounds__(256) void ot_cells_kernel(const uint32_t* __restrict__ leaf_keys, const uint32_t* __restrict__ rank, size_t rank_stride, int dim,
                                                       int depth, const uint32_t* __restrict__ level_base, const Counts* C, uint32_t* __restrict__ cell_first,
                                                       uint32_t* __restrict__ cell_coords, uint32_t* __restrict__ child_first) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const int L = (int)blockIdx.y + 1;
    if (i >= C->n_leaves) return;
    const int shift = dim * (depth - L);
    const uint32_t key = leaf_keys[i] >> shift;
    if (i != 0u && key == (leaf_keys[i - 1u] >> shift)) return;
    const uint32_t c = level_base[L] + rank[(size_t)L * rank_stride + i];
    cell_first[c] = i;
    cell_coords[c] = packed_coords(key, dim, L);
    child_first[c] = L < depth ? level_base[L + 1] + rank[(size_t)(L + 1) * rank_stride + i] : 0u;   // a node's first leaf starts a node of every finer level
}

// a cell's leaf count and the end of its children, from the next cell of its level; the key of the small | big partition
__global__ __launch_bounds__(256) void ot_cell_ends_kernel(const uint32_t* __restrict__ cell_first, const uint32_t* __restrict__ child_first, int depth,
                                                           const uint32_t* __restrict__ level_base, const Counts* C, uint32_t* __restrict__ cell_count,
                                                           uint32_t* __restrict__ child_end, uint32_t* __restrict__ cell_key, uint32_t* __restrict__ cell_id) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= C->n_cells) return;
    int L = 1;
    while (c >= level_base[L + 1]) ++L;
    const bool last = c + 1u == level_base[L + 1];
    const uint32_t count = (last ? C->n_leaves : cell_first[c + 1u]) - cell_first[c];
    cell_count[c] = count;
    child_end[c] = L < depth ? (last ? level_base[L + 2] : child_first[c + 1u]) : 0u;
    cell_key[c] = count > nbx_far::kSmallCell ? 1u : 0u;
    cell_id[c] = c;
}

__global__ void ot_small_count_kernel(const uint32_t* __restrict__ hist, uint32_t tiles, Counts* C) { C->n_small = hist[(size_t)1 * tiles]; }

struct WalkArgs {
    const Counts* C;
    const uint32_t* level_base;
    const uint32_t* leaf_offsets;
    const uint32_t* cell_coords;
    const uint32_t* child_first;
    const uint32_t* child_end;
    uint32_t* near_cnt;         // counting: out
    uint32_t* far_cnt;
    uint32_t* level_far;        // [depth][nl_max] far entries of a leaf per level (counting: out, filling: in)
    uint32_t* far_blk_cnt;
    const uint32_t* list_offsets;   // filling: in
    const uint32_t* far_offsets;
    uint32_t* list_sources;     // filling: out
    uint32_t* far_cells;
    Counts* totals;
    uint32_t nl_max;
    int dim, depth;
    double theta;
    const uint32_t* leaf_keys;      // the adaptive tree: a leaf's first finest key and its level
    const uint32_t* leaf_level;
};

// The walk of one target leaf per lane, depth first from the level-1 nodes: a node the acceptance test takes goes to the far list
// (its level's section: depth-first order within a level is Morton order), a leaf-level node it does not take goes to the near
// list (the leaf itself in front), any other node is opened.  No frontier is stored: FILL = false counts (near, far, far per
// level), FILL = true walks again and writes behind the offsets the counts gave.
// ADAPTIVE: leaves sit at any level.  A cell that is a leaf has child_end = 0 and its leaf in child_first; the target's box is the
// leaf's own node (accepts_box); a.depth = 0 stands for an unsplit root.
template <bool FILL, bool ADAPTIVE>
__global__ __launch_bounds__(kWalkLanes) void ot_walk_kernel(WalkArgs a) {
    __shared__ uint32_t cur[kMaxDepth + 1][kWalkLanes], end[kMaxDepth + 1][kWalkLanes], far_at[kMaxDepth + 1][kWalkLanes];
    const unsigned lane = threadIdx.x;
    const uint32_t t = blockIdx.x * kWalkLanes + lane;
    const uint32_t nl = a.C->n_leaves;
    const bool live = t < nl && a.C->bad == 0u;
    uint32_t near = 0, far = 0;
    if (live && a.depth == 0) {
        near = 1u;
        if (FILL) a.list_sources[a.list_offsets[t]] = t;
    } else if (live) {
        const int depth = a.depth, dim = a.dim;
        const uint32_t leaf_base = ADAPTIVE ? 0u : a.level_base[depth];
        const int st = ADAPTIVE ? depth - (int)a.leaf_level[t] : 0;
        const uint32_t q = ADAPTIVE ? packed_coords(a.leaf_keys[t] >> (dim * st), dim, depth - st) : a.cell_coords[leaf_base + t];
        uint32_t near_base = 0;
        if (FILL) {
            near_base = a.list_offsets[t];
            uint32_t at = a.far_offsets[t];
            for (int L = 1; L <= depth; ++L) { far_at[L][lane] = at; at += a.level_far[(size_t)(L - 1) * a.nl_max + t]; }
            near = 1u;                                  // the leaf itself takes the first place
        } else {
            for (int L = 1; L <= depth; ++L) far_at[L][lane] = 0u;
        }
        int L = 1;
        cur[1][lane] = a.level_base[1];
        end[1][lane] = a.level_base[2];
        while (L >= 1) {
            const uint32_t c = cur[L][lane];
            if (c == end[L][lane]) { --L; continue; }
            cur[L][lane] = c + 1u;
            const uint32_t stop = ADAPTIVE ? a.child_end[c] : 0u;
            if (ADAPTIVE ? accepts_box(q, st, a.cell_coords[c], dim, depth - L, a.theta) : accepts(q, a.cell_coords[c], dim, depth - L, a.theta)) {
                const uint32_t at = far_at[L][lane];
                far_at[L][lane] = at + 1u;
                if (FILL) a.far_cells[at] = c;
                else ++far;
            } else if (ADAPTIVE ? stop == 0u : L == depth) {
                const uint32_t leaf = ADAPTIVE ? a.child_first[c] : c - leaf_base;
                if (FILL) {
                    if (leaf == t) a.list_sources[near_base] = leaf;
                    else a.list_sources[near_base + near++] = leaf;
                } else {
                    ++near;
                }
            } else {
                const uint32_t first = a.child_first[c];
                ++L;
                cur[L][lane] = first;
                end[L][lane] = ADAPTIVE ? stop : a.child_end[c];
            }
        }
        if (!FILL)
            for (int K = 1; K <= depth; ++K) a.level_far[(size_t)(K - 1) * a.nl_max + t] = far_at[K][lane];
    }
    if (FILL) return;
    uint32_t groups = 0;
    if (live) {
        a.near_cnt[t] = near;
        a.far_cnt[t] = far;
        const uint32_t padded = (a.leaf_offsets[t + 1u] - a.leaf_offsets[t] + 1u) & ~1u;   // the planner's slots of this leaf
        groups = far ? (padded + 63u) / 64u : 0u;
        a.far_blk_cnt[t] = groups;
    }
    unsigned long long near_sum = near, far_sum = far;
    uint32_t group_sum = groups;
    for (int d = 32; d > 0; d >>= 1) {
        near_sum += __shfl_xor(near_sum, d);
        far_sum += __shfl_xor(far_sum, d);
        group_sum += __shfl_xor(group_sum, d);
    }
    if (lane == 0u && near_sum) {
        atomicAdd(&a.totals->near_entries, near_sum);
        atomicAdd(&a.totals->far_entries, far_sum);
        atomicAdd(&a.totals->far_blocks, group_sum);
    }
}

// ---- the adaptive tree ----
__global__ void ota_runs_done_kernel(Counts* C) { C->n_runs = C->n_leaves; }

// node_start[j] = the first run of the level's j-th node (node_at: the exclusive scan of the level's run starts); one past the last: n_runs
__global__ __launch_bounds__(256) void ota_node_starts_kernel(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ node_at, const Counts* C,
                                                              uint32_t capacity, uint32_t* __restrict__ node_start) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    const uint32_t nr = C->n_runs < capacity ? C->n_runs : capacity;
    if (r >= nr) return;
    if (flags[r]) node_start[node_at[r]] = r;
    if (r == 0u) node_start[node_at[nr]] = nr;
}

// a run without a leaf level yet (0) takes this level when its node here holds at most `cap` bodies
__global__ __launch_bounds__(256) void ota_run_level_kernel(const uint32_t* __restrict__ node_at, const uint32_t* __restrict__ node_start,
                                                            const uint32_t* __restrict__ run_off, const Counts* C, uint32_t capacity, uint32_t cap, uint32_t level,
                                                            uint32_t* __restrict__ run_level) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    const uint32_t nr = C->n_runs < capacity ? C->n_runs : capacity;
    if (r >= nr || run_level[r] != 0u) return;
    const uint32_t j = node_at[r + 1u] - 1u;      // the starts up to and including r, less one
    if (run_off[node_start[j + 1u]] - run_off[node_start[j]] <= cap) run_level[r] = level;
}

// a run starts a leaf when the run before it lies in another node of the run's leaf level (a node's runs share their leaf level);
// runs still without a level take `fallback`: max_depth, or 0 under an unsplit root
__global__ __launch_bounds__(256) void ota_leaf_flags_kernel(const uint32_t* __restrict__ run_keys, const Counts* C, uint32_t capacity, int dim, int depth,
                                                             uint32_t fallback, uint32_t* __restrict__ run_level, uint32_t* __restrict__ flags) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    const uint32_t nr = C->n_runs < capacity ? C->n_runs : capacity;
    if (r >= nr) return;
    uint32_t lv = run_level[r];
    if (lv == 0u) run_level[r] = lv = fallback;
    const int shift = dim * (depth - (int)lv);
    flags[r] = (r == 0u || (run_keys[r] >> shift) != (run_keys[r - 1u] >> shift)) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void ota_leaves_kernel(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ leaf_of, const uint32_t* __restrict__ run_off,
                                                         const uint32_t* __restrict__ run_keys, const uint32_t* __restrict__ run_level, uint32_t capacity,
                                                         uint32_t* __restrict__ leaf_offsets, uint32_t* __restrict__ leaf_keys, uint32_t* __restrict__ leaf_level,
                                                         Counts* C) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    const uint32_t nr = C->n_runs < capacity ? C->n_runs : capacity;
    if (r >= nr) return;
    if (r == 0u) { const uint32_t nl = leaf_of[nr]; leaf_offsets[nl] = C->n; C->n_leaves = nl; }
    if (flags[r]) { const uint32_t l = leaf_of[r]; leaf_offsets[l] = run_off[r]; leaf_keys[l] = run_keys[r]; leaf_level[l] = run_level[r]; }
}

// flag[i] = leaf i starts an EXISTING node of `level`: it lies at that level or below, and the leaf before it under another prefix
__global__ __launch_bounds__(256) void ota_level_flags_kernel(const uint32_t* __restrict__ leaf_keys, const uint32_t* __restrict__ leaf_level, const Counts* C,
                                                              uint32_t capacity, uint32_t level, int shift, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t nl = C->n_leaves < capacity ? C->n_leaves : capacity;
    if (i >= nl) return;
    flags[i] = (leaf_level[i] >= level && (i == 0u || (leaf_keys[i] >> shift) != (leaf_keys[i - 1u] >> shift))) ? 1u : 0u;
}

// one lane per (level, leaf): the leaf that starts an existing node of the level writes the node's cell.  Its leaves end where the
// sorted leaf keys leave the prefix (a binary search); a leaf cell keeps its leaf in child_first and 0 in child_end (a split node's
// children end past level_base[2] >= 1); a split node's children are the next level's nodes started within its leaves.
__global__ __launch_bounds__(256) void ota_cells_kernel(const uint32_t* __restrict__ leaf_keys, const uint32_t* __restrict__ leaf_level,
                                                        const uint32_t* __restrict__ rank, size_t rank_stride, int dim, int depth,
                                                        const uint32_t* __restrict__ level_base, const Counts* C, uint32_t* __restrict__ cell_first,
                                                        uint32_t* __restrict__ cell_count, uint32_t* __restrict__ cell_coords, uint32_t* __restrict__ child_first,
                                                        uint32_t* __restrict__ child_end, uint32_t* __restrict__ cell_key, uint32_t* __restrict__ cell_id) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t L = blockIdx.y + 1u, nl = C->n_leaves;
    if (i >= nl || leaf_level[i] < L) return;
    const int shift = dim * (depth - (int)L);
    const uint32_t key = leaf_keys[i] >> shift;
    if (i != 0u && key == (leaf_keys[i - 1u] >> shift)) return;
    const uint32_t past = (key + 1u) << shift;      // at most 2^(dim depth) <= 2^30
    uint32_t lo = i + 1u, hi = nl;                   // the first leaf whose key is >= past
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (leaf_keys[mid] < past) lo = mid + 1u; else hi = mid;
    }
    const uint32_t c = level_base[L] + rank[(size_t)L * rank_stride + i], count = lo - i;
    cell_first[c] = i;
    cell_count[c] = count;
    cell_coords[c] = packed_coords(key, dim, (int)L);
    if (leaf_level[i] == L) {
        child_first[c] = i;
        child_end[c] = 0u;
    } else {
        child_first[c] = level_base[L + 1u] + rank[(size_t)(L + 1u) * rank_stride + i];
        child_end[c] = level_base[L + 1u] + rank[(size_t)(L + 1u) * rank_stride + i + count];
    }
    cell_key[c] = count > nbx_far::kSmallCell ? 1u : 0u;
    cell_id[c] = c;
}

// leaf_far.h plan_far's blocks of one leaf per lane, in leaf order; the sort key puts the longest far list first
__global__ __launch_bounds__(256) void ot_far_blocks_kernel(const uint32_t* __restrict__ unit_off, const uint32_t* __restrict__ far_offsets,
                                                            const uint32_t* __restrict__ far_blk_cnt, const uint32_t* __restrict__ far_blk_off, const Counts* C,
                                                            uint32_t capacity, nbx_far::FarBlock* __restrict__ tmp, uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    const uint32_t l = blockIdx.x * 256u + threadIdx.x;
    if (l >= C->n_leaves) return;
    const uint32_t groups = far_blk_cnt[l];
    if (!groups) return;
    const uint32_t c = unit_off[l + 1u] - unit_off[l], far_lo = far_offsets[l], far_n = far_offsets[l + 1u] - far_lo;
    uint32_t f = unit_off[l], at = far_blk_off[l];
    for (uint32_t g = 0; g < groups && at < capacity; ++g, ++at) {
        const uint32_t share = c / groups + (g < c % groups ? 1u : 0u);
        tmp[at] = nbx_far::FarBlock{f, share, far_lo, far_n};
        key[at] = C->n_cells - far_n;      // a far list names every cell at most once
        val[at] = at;
        f += share;
    }
}

__global__ __launch_bounds__(256) void ot_far_deal_kernel(const nbx_far::FarBlock* __restrict__ tmp, const uint32_t* __restrict__ val, uint32_t n_blocks,
                                                          nbx_far::FarBlock* __restrict__ blocks) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_blocks) blocks[i] = tmp[val[i]];
}

inline uint32_t* words(char* block, size_t off) { return reinterpret_cast<uint32_t*>(block + off); }
inline unsigned grid_of(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

TreeLayout make_tree_layout(size_t n, int dim, int depth, bool adaptive) {
    TreeLayout L{};
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) / 256 * 256 + 256; return o; };
    const size_t grid_cells = (size_t)1 << (dim * depth);
    const size_t nl = std::min(n, grid_cells);
    size_t cells = 0;
    for (int lv = 1; lv <= depth; ++lv) cells += std::min(n, (size_t)1 << (dim * lv));
    L.nl_max = nl;
    L.cells_max = cells;
    const size_t far_blocks_max = nl + (n + nl) / 64 + 1;
    const size_t sort_cap = std::max(std::max(n + 1, cells), far_blocks_max);
    L.counts = take(sizeof(Counts));
    L.box = take(sizeof(RootBox));
    L.partial = take((size_t)kBoxBlocks * 6 * sizeof(double));
    L.level_base = take((kMaxDepth + 3) * 4);
    L.key_a = take((n + 1) * 4);
    L.key_b = take((n + 1) * 4);
    L.val_a = take((n + 1) * 4);
    L.val_b = take((n + 1) * 4);
    L.hist = take(nbx_sort::radix_temp_bytes((unsigned)sort_cap));
    L.tile_sums = take(((size_t)nbx_sort::scan_tiles((unsigned)sort_cap) + 2) * 4);
    L.flags = take((n + 1) * 4);
    L.leaf_offsets = take((nl + 1) * 4);
    L.leaf_keys = take((nl + 1) * 4);
    L.list_offsets = take((nl + 1) * 4);
    L.far_offsets = take((nl + 1) * 4);
    L.near_cnt = take((nl + 1) * 4);
    L.far_cnt = take((nl + 1) * 4);
    L.level_far = take(((size_t)depth * nl + 1) * 4);
    L.rank = take((size_t)(depth + 2) * (nl + 1) * 4);
    L.cell_first = take((cells + 1) * 4);
    L.cell_count = take((cells + 1) * 4);
    L.cell_coords = take((cells + 1) * 4);
    L.child_first = take((cells + 1) * 4);
    L.child_end = take((cells + 1) * 4);
    L.cell_key = take((cells + 1) * 4);
    L.cell_key2 = take((cells + 1) * 4);
    L.cell_id = take((cells + 1) * 4);
    L.cells_split = take((cells + 1) * 4);
    L.far_blk_cnt = take((nl + 1) * 4);
    L.far_blk_off = take((nl + 2) * 4);
    if (adaptive) {
        L.run_off = take((nl + 1) * 4);
        L.run_keys = take((nl + 1) * 4);
        L.run_level = take((nl + 1) * 4);
        L.node_at = take((nl + 2) * 4);
        L.node_start = take((nl + 2) * 4);
        L.leaf_level = take((nl + 1) * 4);
    }
    L.total = at;
    return L;
}

#define OT_TRY(expr) do { if ((e = (expr)) != hipSuccess) return e; } while (0)

hipError_t enqueue_build(const double* x64, size_t pad, size_t n, int dim, int depth, double theta, char* block, const TreeLayout& L, hipStream_t s,
                         Counts* counts_host, Tree* tree) {
    hipError_t e;
    const uint32_t n32 = (uint32_t)n, nl_max = (uint32_t)L.nl_max, cells_max = (uint32_t)L.cells_max;
    Counts* const C = reinterpret_cast<Counts*>(block + L.counts);
    RootBox* const box = reinterpret_cast<RootBox*>(block + L.box);
    double* const partial = reinterpret_cast<double*>(block + L.partial);
    Counts init{};
    init.n = n32;
    *counts_host = init;   // staged from here: the copy below may be asynchronous
    OT_TRY(hipMemcpyAsync(C, counts_host, sizeof(Counts), hipMemcpyHostToDevice, s));
    const dim3 blk(256);
    // bounding box, root box, keys
    hipLaunchKernelGGL(ot_bbox_partial_kernel, dim3(kBoxBlocks), blk, 0, s, x64, pad, n32, dim, partial, C);
    hipLaunchKernelGGL(ot_bbox_final_kernel, dim3(1), blk, 0, s, partial, kBoxBlocks, dim, box);
    uint32_t *keys = words(block, L.key_a), *vals = words(block, L.val_a), *keys2 = words(block, L.key_b), *vals2 = words(block, L.val_b);
    hipLaunchKernelGGL(ot_keys_kernel, dim3(grid_of(n)), blk, 0, s, x64, pad, n32, dim, depth, box, keys, vals);
    // stable LSD radix sort of (key, body): the body order of numpy's stable argsort
    const int passes = (dim * depth + 7) / 8;
    for (int p = 0; p < passes; ++p) {
        OT_TRY(radix_pass(keys, vals, keys2, vals2, &C->n, n32, 8 * p, words(block, L.hist), s));
        std::swap(keys, keys2);
        std::swap(vals, vals2);
    }
    // leaves: the runs of equal keys
    uint32_t* const flags = words(block, L.flags);
    uint32_t* const body_rank = keys2;   // the sort's spare key buffer
    hipLaunchKernelGGL(ot_flags_kernel, dim3(grid_of(n)), blk, 0, s, keys, &C->n, n32, 0, flags);
    OT_TRY(exclusive_scan(flags, body_rank, &C->n, n32, words(block, L.tile_sums), s));
    hipLaunchKernelGGL(ot_leaves_kernel, dim3(grid_of(n)), blk, 0, s, keys, body_rank, n32, words(block, L.leaf_offsets), words(block, L.leaf_keys), C);
    // the non-empty nodes of every level: a leaf's node index at level L is the scan of the level's run starts
    const size_t rank_stride = L.nl_max + 1;
    uint32_t* const rank = words(block, L.rank);
    for (int lv = 1; lv <= depth; ++lv) {
        hipLaunchKernelGGL(ot_flags_kernel, dim3(grid_of(nl_max)), blk, 0, s, words(block, L.leaf_keys), &C->n_leaves, nl_max, dim * (depth - lv), flags);
        OT_TRY(exclusive_scan(flags, rank + (size_t)lv * rank_stride, &C->n_leaves, nl_max, words(block, L.tile_sums), s));
    }
    hipLaunchKernelGGL(ot_level_bases_kernel, dim3(1), dim3(1), 0, s, rank, rank_stride, depth, words(block, L.level_base), C);
    if (depth >= 1) {
        hipLaunchKernelGGL(ot_cells_kernel, dim3(grid_of(nl_max), (unsigned)depth), blk, 0, s, words(block, L.leaf_keys), rank, rank_stride, dim, depth,
                           words(block, L.level_base), C, words(block, L.cell_first), words(block, L.cell_coords), words(block, L.child_first));
        hipLaunchKernelGGL(ot_cell_ends_kernel, dim3(grid_of(cells_max)), blk, 0, s, words(block, L.cell_first), words(block, L.child_first), depth,
                           words(block, L.level_base), C, words(block, L.cell_count), words(block, L.child_end), words(block, L.cell_key), words(block, L.cell_id));
        // small cells first, then the big ones, each in cell order: one stable pass over a one-bit key
        OT_TRY(radix_pass(words(block, L.cell_key), words(block, L.cell_id), words(block, L.cell_key2), words(block, L.cells_split), &C->n_cells, cells_max, 0,
                          words(block, L.hist), s));
        hipLaunchKernelGGL(ot_small_count_kernel, dim3(1), dim3(1), 0, s, words(block, L.hist), sort_tiles(cells_max), C);
    }
    // the counting walk and the offsets of both lists
    WalkArgs a{};
    a.C = C; a.level_base = words(block, L.level_base); a.leaf_offsets = words(block, L.leaf_offsets); a.cell_coords = words(block, L.cell_coords);
    a.child_first = words(block, L.child_first); a.child_end = words(block, L.child_end);
    a.near_cnt = words(block, L.near_cnt); a.far_cnt = words(block, L.far_cnt); a.level_far = words(block, L.level_far); a.far_blk_cnt = words(block, L.far_blk_cnt);
    a.totals = C; a.nl_max = nl_max; a.dim = dim; a.depth = depth; a.theta = theta;
    hipLaunchKernelGGL((ot_walk_kernel<false, false>), dim3((nl_max + kWalkLanes - 1u) / kWalkLanes), dim3(kWalkLanes), 0, s, a);
    OT_TRY(exclusive_scan(words(block, L.near_cnt), words(block, L.list_offsets), &C->n_leaves, nl_max, words(block, L.tile_sums), s));
    OT_TRY(exclusive_scan(words(block, L.far_cnt), words(block, L.far_offsets), &C->n_leaves, nl_max, words(block, L.tile_sums), s));
    OT_TRY(exclusive_scan(words(block, L.far_blk_cnt), words(block, L.far_blk_off), &C->n_leaves, nl_max, words(block, L.tile_sums), s));
    OT_TRY(hipGetLastError());
    OT_TRY(hipMemcpyAsync(counts_host, C, sizeof(Counts), hipMemcpyDeviceToHost, s));
    tree->counts = C;
    tree->leaf_offsets = words(block, L.leaf_offsets);
    tree->leaf_bodies = vals;
    tree->list_offsets = words(block, L.list_offsets);
    tree->far_offsets = words(block, L.far_offsets);
    tree->cell_first = words(block, L.cell_first);
    tree->cell_count = words(block, L.cell_count);
    tree->small_cells = words(block, L.cells_split);
    return hipSuccess;
}

hipError_t enqueue_fill(size_t n, int dim, int depth, double theta, char* block, const TreeLayout& L, uint32_t* list_sources, uint32_t* far_cells,
                        hipStream_t s) {
    (void)n;
    Counts* const C = reinterpret_cast<Counts*>(block + L.counts);
    WalkArgs a{};
    a.C = C; a.level_base = words(block, L.level_base); a.leaf_offsets = words(block, L.leaf_offsets); a.cell_coords = words(block, L.cell_coords);
    a.child_first = words(block, L.child_first); a.child_end = words(block, L.child_end);
    a.level_far = words(block, L.level_far);
    a.list_offsets = words(block, L.list_offsets); a.far_offsets = words(block, L.far_offsets);
    a.list_sources = list_sources; a.far_cells = far_cells;
    a.totals = C; a.nl_max = (uint32_t)L.nl_max; a.dim = dim; a.depth = depth; a.theta = theta;
    hipLaunchKernelGGL((ot_walk_kernel<true, false>), dim3(((unsigned)L.nl_max + kWalkLanes - 1u) / kWalkLanes), dim3(kWalkLanes), 0, s, a);
    return hipGetLastError();
}

hipError_t enqueue_build_adaptive(const double* x64, size_t pad, size_t n, int dim, int depth, size_t leaf_capacity, double theta, char* block,
                                  const TreeLayout& L, hipStream_t s, Counts* counts_host, Tree* tree) {
    hipError_t e;
    const uint32_t n32 = (uint32_t)n, nl_max = (uint32_t)L.nl_max, cells_max = (uint32_t)L.cells_max;
    const uint32_t cap = (uint32_t)std::min<size_t>(leaf_capacity, 0xffffffffu);
    const bool split = root_is_split(n, depth, leaf_capacity);
    Counts* const C = reinterpret_cast<Counts*>(block + L.counts);
    RootBox* const box = reinterpret_cast<RootBox*>(block + L.box);
    double* const partial = reinterpret_cast<double*>(block + L.partial);
    Counts init{};
    init.n = n32;
    *counts_host = init;
    OT_TRY(hipMemcpyAsync(C, counts_host, sizeof(Counts), hipMemcpyHostToDevice, s));
    const dim3 blk(256);
    // bounding box, root box, keys at max_depth, the stable sort: the fixed builder's stages
    hipLaunchKernelGGL(ot_bbox_partial_kernel, dim3(kBoxBlocks), blk, 0, s, x64, pad, n32, dim, partial, C);
    hipLaunchKernelGGL(ot_bbox_final_kernel, dim3(1), blk, 0, s, partial, kBoxBlocks, dim, box);
    uint32_t *keys = words(block, L.key_a), *vals = words(block, L.val_a), *keys2 = words(block, L.key_b), *vals2 = words(block, L.val_b);
    hipLaunchKernelGGL(ot_keys_kernel, dim3(grid_of(n)), blk, 0, s, x64, pad, n32, dim, depth, box, keys, vals);
    const int passes = (dim * depth + 7) / 8;
    for (int p = 0; p < passes; ++p) {
        OT_TRY(radix_pass(keys, vals, keys2, vals2, &C->n, n32, 8 * p, words(block, L.hist), s));
        std::swap(keys, keys2);
        std::swap(vals, vals2);
    }
    // the finest level's runs (the fixed tree's leaves)
    uint32_t* const flags = words(block, L.flags);
    uint32_t *const run_off = words(block, L.run_off), *const run_keys = words(block, L.run_keys), *const run_level = words(block, L.run_level);
    uint32_t *const node_at = words(block, L.node_at), *const node_start = words(block, L.node_start), *const leaf_level = words(block, L.leaf_level);
    hipLaunchKernelGGL(ot_flags_kernel, dim3(grid_of(n)), blk, 0, s, keys, &C->n, n32, 0, flags);
    OT_TRY(exclusive_scan(flags, keys2, &C->n, n32, words(block, L.tile_sums), s));
    hipLaunchKernelGGL(ot_leaves_kernel, dim3(grid_of(n)), blk, 0, s, keys, keys2, n32, run_off, run_keys, C);
    hipLaunchKernelGGL(ota_runs_done_kernel, dim3(1), dim3(1), 0, s, C);
    // every run's leaf level: the first level whose node holds at most `cap` bodies (node counts from the runs' offsets), else max_depth
    OT_TRY(hipMemsetAsync(run_level, 0, (L.nl_max + 1) * 4, s));
    if (split)
        for (int lv = 1; lv < depth; ++lv) {
            hipLaunchKernelGGL(ot_flags_kernel, dim3(grid_of(nl_max)), blk, 0, s, run_keys, &C->n_runs, nl_max, dim * (depth - lv), flags);
            OT_TRY(exclusive_scan(flags, node_at, &C->n_runs, nl_max, words(block, L.tile_sums), s));
            hipLaunchKernelGGL(ota_node_starts_kernel, dim3(grid_of(nl_max)), blk, 0, s, flags, node_at, C, nl_max, node_start);
            hipLaunchKernelGGL(ota_run_level_kernel, dim3(grid_of(nl_max)), blk, 0, s, node_at, node_start, run_off, C, nl_max, cap, (uint32_t)lv, run_level);
        }
    // the leaves: runs of equal (leaf level, prefix)
    hipLaunchKernelGGL(ota_leaf_flags_kernel, dim3(grid_of(nl_max)), blk, 0, s, run_keys, C, nl_max, dim, depth, split ? (uint32_t)depth : 0u, run_level, flags);
    OT_TRY(exclusive_scan(flags, node_at, &C->n_runs, nl_max, words(block, L.tile_sums), s));
    hipLaunchKernelGGL(ota_leaves_kernel, dim3(grid_of(nl_max)), blk, 0, s, flags, node_at, run_off, run_keys, run_level, nl_max, words(block, L.leaf_offsets),
                       words(block, L.leaf_keys), leaf_level, C);
    // the existing nodes of every level
    const size_t rank_stride = L.nl_max + 1;
    uint32_t* const rank = words(block, L.rank);
    for (int lv = 1; lv <= depth; ++lv) {
        hipLaunchKernelGGL(ota_level_flags_kernel, dim3(grid_of(nl_max)), blk, 0, s, words(block, L.leaf_keys), leaf_level, C, nl_max, (uint32_t)lv,
                           dim * (depth - lv), flags);
        OT_TRY(exclusive_scan(flags, rank + (size_t)lv * rank_stride, &C->n_leaves, nl_max, words(block, L.tile_sums), s));
    }
    hipLaunchKernelGGL(ot_level_bases_kernel, dim3(1), dim3(1), 0, s, rank, rank_stride, depth, words(block, L.level_base), C);
    if (split) {
        hipLaunchKernelGGL(ota_cells_kernel, dim3(grid_of(nl_max), (unsigned)depth), blk, 0, s, words(block, L.leaf_keys), leaf_level, rank, rank_stride, dim, depth,
                           words(block, L.level_base), C, words(block, L.cell_first), words(block, L.cell_count), words(block, L.cell_coords),
                           words(block, L.child_first), words(block, L.child_end), words(block, L.cell_key), words(block, L.cell_id));
        OT_TRY(radix_pass(words(block, L.cell_key), words(block, L.cell_id), words(block, L.cell_key2), words(block, L.cells_split), &C->n_cells, cells_max, 0,
                          words(block, L.hist), s));
        hipLaunchKernelGGL(ot_small_count_kernel, dim3(1), dim3(1), 0, s, words(block, L.hist), sort_tiles(cells_max), C);
    }
    // the counting walk and the offsets of both lists
    WalkArgs a{};
    a.C = C; a.level_base = words(block, L.level_base); a.leaf_offsets = words(block, L.leaf_offsets); a.cell_coords = words(block, L.cell_coords);
    a.child_first = words(block, L.child_first); a.child_end = words(block, L.child_end);
    a.near_cnt = words(block, L.near_cnt); a.far_cnt = words(block, L.far_cnt); a.level_far = words(block, L.level_far); a.far_blk_cnt = words(block, L.far_blk_cnt);
    a.totals = C; a.nl_max = nl_max; a.dim = dim; a.depth = split ? depth : 0; a.theta = theta;
    a.leaf_keys = words(block, L.leaf_keys); a.leaf_level = leaf_level;
    hipLaunchKernelGGL((ot_walk_kernel<false, true>), dim3((nl_max + kWalkLanes - 1u) / kWalkLanes), dim3(kWalkLanes), 0, s, a);
    OT_TRY(exclusive_scan(words(block, L.near_cnt), words(block, L.list_offsets), &C->n_leaves, nl_max, words(block, L.tile_sums), s));
    OT_TRY(exclusive_scan(words(block, L.far_cnt), words(block, L.far_offsets), &C->n_leaves, nl_max, words(block, L.tile_sums), s));
    OT_TRY(exclusive_scan(words(block, L.far_blk_cnt), words(block, L.far_blk_off), &C->n_leaves, nl_max, words(block, L.tile_sums), s));
    OT_TRY(hipGetLastError());
    OT_TRY(hipMemcpyAsync(counts_host, C, sizeof(Counts), hipMemcpyDeviceToHost, s));
    tree->counts = C;
    tree->leaf_offsets = words(block, L.leaf_offsets);
    tree->leaf_bodies = vals;
    tree->list_offsets = words(block, L.list_offsets);
    tree->far_offsets = words(block, L.far_offsets);
    tree->cell_first = words(block, L.cell_first);
    tree->cell_count = words(block, L.cell_count);
    tree->small_cells = words(block, L.cells_split);
    return hipSuccess;
}

hipError_t enqueue_fill_adaptive(size_t n, int dim, int depth, size_t leaf_capacity, double theta, char* block, const TreeLayout& L, uint32_t* list_sources,
                                 uint32_t* far_cells, hipStream_t s) {
    Counts* const C = reinterpret_cast<Counts*>(block + L.counts);
    WalkArgs a{};
    a.C = C; a.level_base = words(block, L.level_base); a.leaf_offsets = words(block, L.leaf_offsets); a.cell_coords = words(block, L.cell_coords);
    a.child_first = words(block, L.child_first); a.child_end = words(block, L.child_end);
    a.level_far = words(block, L.level_far);
    a.list_offsets = words(block, L.list_offsets); a.far_offsets = words(block, L.far_offsets);
    a.list_sources = list_sources; a.far_cells = far_cells;
    a.totals = C; a.nl_max = (uint32_t)L.nl_max; a.dim = dim; a.depth = root_is_split(n, depth, leaf_capacity) ? depth : 0; a.theta = theta;
    a.leaf_keys = words(block, L.leaf_keys); a.leaf_level = words(block, L.leaf_level);
    hipLaunchKernelGGL((ot_walk_kernel<true, true>), dim3(((unsigned)L.nl_max + kWalkLanes - 1u) / kWalkLanes), dim3(kWalkLanes), 0, s, a);
    return hipGetLastError();
}

size_t far_scratch_bytes(size_t far_blocks) { return 4 * ((far_blocks + 1) * 4 + 256) + (far_blocks + 1) * sizeof(nbx_far::FarBlock) + 256; }

hipError_t enqueue_far_layout(const uint32_t* unit_off, const Counts& counts, char* block, const TreeLayout& L, nbx_far::FarBlock* blocks, char* scratch,
                              hipStream_t s) {
    hipError_t e;
    const uint32_t nb = counts.far_blocks;
    if (!nb) return hipSuccess;
    Counts* const C = reinterpret_cast<Counts*>(block + L.counts);
    const size_t stride = ((size_t)nb + 1) * 4 + 256;
    uint32_t *key = words(scratch, 0), *val = words(scratch, stride), *key2 = words(scratch, 2 * stride), *val2 = words(scratch, 3 * stride);
    nbx_far::FarBlock* const tmp = reinterpret_cast<nbx_far::FarBlock*>(scratch + 4 * stride);
    hipLaunchKernelGGL(ot_far_blocks_kernel, dim3(grid_of(L.nl_max)), dim3(256), 0, s, unit_off, words(block, L.far_offsets), words(block, L.far_blk_cnt),
                       words(block, L.far_blk_off), C, nb, tmp, key, val);
    int bits = 1;
    while (bits < 32 && (counts.n_cells >> bits)) ++bits;
    for (int p = 0; p < (bits + 7) / 8; ++p) {
        OT_TRY(radix_pass(key, val, key2, val2, &C->far_blocks, nb, 8 * p, words(block, L.hist), s));
        std::swap(key, key2);
        std::swap(val, val2);
    }
    hipLaunchKernelGGL(ot_far_deal_kernel, dim3(grid_of(nb)), dim3(256), 0, s, tmp, val, nb, blocks);
    return hipGetLastError();
}
#undef OT_TRY

}  // namespace nbx_octree
