// leaf_far_kernel.hip -- the far field of a leaf plan: every cell's total mass and centre of mass from the positions as they stand
// (the moment pass), then, per target leaf, the pair law applied to the cells of its far list as pseudo-bodies (the far pass):
//   octree.cpp:129-151, bvh.cpp:203-239 -- a far node attracts a body as one body of the node's mass at its centre of mass.
// leaf_far.h has the layout both passes follow.
//
// Moment pass (fp64 from the fp32 slot values; fixed summation order, no atomics; the error does not grow with N):
//  * far_leaf_moments_kernel: kLeafLanes lanes per leaf stride over the leaf's padded slots (a pad is massless: exact zeros) and
//    meet in a fixed xor tree: {sum m, sum m x, sum m y, sum m z} per leaf.  m x is exact in fp64 (24 + 24 bits).
//  * far_small_cells_kernel: one lane per cell of <= kSmallCell leaves (at a 2^depth grid: every parent of leaves and every leaf).
//  * far_big_cells_kernel: one workgroup per larger cell (a child of the root spans an eighth of all leaves): its lanes stride over
//    the leaf range and meet in an LDS tree.
//  Both write the fp64 moments (for nbx_leaf_plan_get_cells) and the 16-byte fp32 pseudo-body {x, y, z, M}; a cell of mass 0 becomes
//  the pair kernels' pad body (massless, far away): its terms are exact zeros, never NaN (bvh.cpp:225 guards the same case).
//  At order 1 (NBX_FAR_QUADRUPOLE) three more kernels of the same shapes follow, for the central second moments Q_ab = sum m s_a s_b,
//  s = p - com, in the parallel-axis form (no term cancels; sum m x x^T - M c c^T is never formed):
//  * far_leaf_quad_kernel: Q_l about the leaf's OWN centre of mass, kLeafLanes lanes per leaf, the same xor tree;
//  * far_small_cells_quad_kernel / far_big_cells_quad_kernel: Q = sum_l [ Q_l + M_l (c_l - c)(c_l - c)^T ] over the cell's leaves, c the
//    cell's centre of mass that the kernels above have just written.
//  They write Q in fp64 (nbx_leaf_plan_get_cell_quadrupoles) and the fp32 record q = Q / M with its trace (leaf_far.h); the record is all
//  zeros -- the cell then attracts as its monopole alone -- when M == 0 or when any entry of q is not finite in fp32.
// Far pass: one wave64 per FarBlock (<= 64 targets of one leaf).  The wave walks the leaf's far list in tiles of kFarTile entries:
//  lanes load the indices coalesced and gather the 16-byte records (L2 hits: neighbouring leaves name the same cells) through
//  registers into LDS (two layouts, see far_kernel); a target is shared by P = min(64 / targets, kFarMaxLanes) lanes, lane group g takes
//  record pairs [g T, (g + 1) T) of the tile (T odd; two ds_read_b128 per pair, the lanes of a group read one address) on float2 values.  fp32 partial sums, flushed
//  into fp64 every <= 248 terms; the lane groups' fp64 sums meet in LDS in group order; one lane per target ADDS the result to the
//  plan's slot-ordered sums behind the pair kernel.  Every slot is written by one lane: no atomics.
//  The law's special cases are applied per pair with leaf_weight (leaf_law.h): the pair kernels' unguarded form needs every source mass
//  below 1.7e10 (m / kTiny^2 finite for a coincident source), and a cell's mass is not a body's: at N = 2^20 with the reference's masses a
//  child of the root weighs 6.5e12.
//  ORDER 1 adds the second-order term of the expansion of sum m_j (R + s_j) / |R + s_j|^4 about the centre of mass (the dipole vanishes):
//      (M / r^4) [ R (1 - 2 tr(q) / r^2 + 12 R^T q R / r^4) - 4 q R / r^2 ],   R = com - p_i, r^2 = |R|^2, q = Q / M.
//  The law is one power of r steeper than Newton's, d / r^4 is not a harmonic function's gradient in 3D: the full symmetric q is needed,
//  not the traceless one.  Evaluated with u = R / r^2 (|u| = 1 / r: nothing overflows, a pad's 1e18 included): q u, u^T q u, the scalar
//  1 + 12 u^T q u - 2 tr(q) / r^2, the direction scalar * R - 4 q u.  1 / r^2 is the reciprocal leaf_weight_ri took for the weight; where
//  the law skips or softens the pair it is 0 and the term is the monopole's, bit for bit.  The q records ride in a second LDS tile
//  (32 B per record in 3D, 16 B in 2D) in the same two layouts; everything else -- one wave per FarBlock, float2 arithmetic on two
//  records, the fp64 flush, the lane groups meeting in LDS in group order, one writer per slot -- is the monopole pass's.
//  Under NBX_LAW_NEWTON (m_j d / rho^3, rho^2 = r^2 + eps^2; leaf_law.h) the pseudo-body is a body like any other, and the second-order
//  term of sum m_j (R + s_j) / (|R + s_j|^2 + eps^2)^(3/2) is, exactly,
//      (M / rho^3) [ R (1 - (3/2) tr(q) / rho^2 + (15/2) R^T q R / rho^4) - 3 q R / rho^2 ]
//  -- the same expression with the coefficients (2, 12, 4) replaced by (3/2, 15/2, 3) and rho^2 in every denominator, u = R / rho^2
//  included; leaf_weight_ri hands back 1 / rho^2.
#include "leaf_far.h"
#include "leaf_law.h"

using namespace nbx_leaf;

namespace nbx_far {
namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
constexpr unsigned kFlushTerms = 248;

__global__ __launch_bounds__(256) void far_leaf_moments_kernel(const float* __restrict__ xp, const uint32_t* __restrict__ unit_off, uint32_t n_leaves,
                                                               int dim, double* __restrict__ leaf_mom) {
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t l = gid / kLeafLanes, k = gid % kLeafLanes;
    double m = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
    if (l < n_leaves) {
        const uint32_t lo = unit_off[l], hi = unit_off[l + 1];
        for (uint32_t p = lo + k; p < hi; p += kLeafLanes) {
            const float* __restrict__ o = xp + (size_t)(p >> 1) * 8u + (p & 1u);
            const double w = (double)o[6];
            m += w;
            mx += w * (double)o[0];
            my += w * (double)o[2];
            if (dim == 3) mz += w * (double)o[4];
        }
    }
    for (unsigned d = 1; d < kLeafLanes; d <<= 1) {       // every lane of the wave takes part; the order is fixed
        m += __shfl_xor(m, (int)d); mx += __shfl_xor(mx, (int)d); my += __shfl_xor(my, (int)d); mz += __shfl_xor(mz, (int)d);
    }
    if (l < n_leaves && k == 0u) {
        double* __restrict__ o = leaf_mom + (size_t)l * 4u;
        o[0] = m; o[1] = mx; o[2] = my; o[3] = mz;
    }
}

__device__ __forceinline__ void write_cell(const FarDevice& d, int dim, uint32_t c, double m, double mx, double my, double mz) {
    double cx = 0.0, cy = 0.0, cz = 0.0;
    float4 rec = make_float4(kFar, kFar, dim == 3 ? kFar : 0.0f, 0.0f);   // mass 0: the pad body
    if (m != 0.0) {
        cx = mx / m; cy = my / m; cz = dim == 3 ? mz / m : 0.0;
        rec = make_float4((float)cx, (float)cy, (float)cz, (float)m);
    }
    d.cell_mass[c] = m;
    d.cell_com[(size_t)c * dim] = cx;
    d.cell_com[(size_t)c * dim + 1] = cy;
    if (dim == 3) d.cell_com[(size_t)c * dim + 2] = cz;
    d.cell_rec[c] = rec;
}

__global__ __launch_bounds__(256) void far_small_cells_kernel(FarDevice d, int dim) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= d.n_small) return;
    const uint32_t c = d.small_cells[i];
    const uint32_t lo = d.cell_first[c], n = d.cell_count[c];
    double m = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
    for (uint32_t l = lo; l < lo + n; ++l) {
        const double* __restrict__ q = d.leaf_mom + (size_t)l * 4u;
        m += q[0]; mx += q[1]; my += q[2]; mz += q[3];
    }
    write_cell(d, dim, c, m, mx, my, mz);
}

__global__ __launch_bounds__(kCellThreads) void far_big_cells_kernel(FarDevice d, int dim) {
    __shared__ double red[4][kCellThreads];
    const uint32_t c = d.big_cells[blockIdx.x];
    const uint32_t lo = d.cell_first[c], n = d.cell_count[c];
    const uint32_t tid = threadIdx.x;
    double m = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
    for (uint32_t l = tid; l < n; l += kCellThreads) {
        const double* __restrict__ q = d.leaf_mom + (size_t)(lo + l) * 4u;
        m += q[0]; mx += q[1]; my += q[2]; mz += q[3];
    }
    red[0][tid] = m; red[1][tid] = mx; red[2][tid] = my; red[3][tid] = mz;
    __syncthreads();
    for (uint32_t h = kCellThreads / 2u; h >= 1u; h >>= 1) {
        if (tid < h) { red[0][tid] += red[0][tid + h]; red[1][tid] += red[1][tid + h]; red[2][tid] += red[2][tid + h]; red[3][tid] += red[3][tid + h]; }
        __syncthreads();
    }
    if (tid == 0u) write_cell(d, dim, c, red[0][0], red[1][0], red[2][0], red[3][0]);
}

// ---- order 1: central second moments.  Six running sums whatever the dimension (xx, yy, zz, xy, xz, yz; 2D leaves three at zero). ----
struct Quad { double xx = 0.0, yy = 0.0, zz = 0.0, xy = 0.0, xz = 0.0, yz = 0.0; };

__global__ __launch_bounds__(256) void far_leaf_quad_kernel(const float* __restrict__ xp, const uint32_t* __restrict__ unit_off, uint32_t n_leaves,
                                                            int dim, const double* __restrict__ leaf_mom, double* __restrict__ leaf_quad) {
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t l = gid / kLeafLanes, k = gid % kLeafLanes;
    Quad q;
    if (l < n_leaves) {
        const double* __restrict__ mo = leaf_mom + (size_t)l * 4u;
        const double m = mo[0];
        // a massless leaf: every term below is an exact zero whatever the centre
        const double cx = m != 0.0 ? mo[1] / m : 0.0, cy = m != 0.0 ? mo[2] / m : 0.0, cz = m != 0.0 ? mo[3] / m : 0.0;
        const uint32_t lo = unit_off[l], hi = unit_off[l + 1];
        for (uint32_t p = lo + k; p < hi; p += kLeafLanes) {
            const float* __restrict__ o = xp + (size_t)(p >> 1) * 8u + (p & 1u);
            const double w = (double)o[6];
            if (w == 0.0) continue;                      // a pad slot sits at 1e18: 0 * 1e36 is still zero, but keep it out of the sums' way
            const double sx = (double)o[0] - cx, sy = (double)o[2] - cy;
            q.xx += w * sx * sx; q.yy += w * sy * sy; q.xy += w * sx * sy;
            if (dim == 3) {
                const double sz = (double)o[4] - cz;
                q.zz += w * sz * sz; q.xz += w * sx * sz; q.yz += w * sy * sz;
            }
        }
    }
    for (unsigned d = 1; d < kLeafLanes; d <<= 1) {       // every lane of the wave takes part; the order is fixed
        q.xx += __shfl_xor(q.xx, (int)d); q.yy += __shfl_xor(q.yy, (int)d); q.zz += __shfl_xor(q.zz, (int)d);
        q.xy += __shfl_xor(q.xy, (int)d); q.xz += __shfl_xor(q.xz, (int)d); q.yz += __shfl_xor(q.yz, (int)d);
    }
    if (l < n_leaves && k == 0u) {
        double* __restrict__ o = leaf_quad + (size_t)l * 6u;
        o[0] = q.xx; o[1] = q.yy; o[2] = q.zz; o[3] = q.xy; o[4] = q.xz; o[5] = q.yz;
    }
}

// leaf l's share of a cell's Q about the cell's centre (cx, cy, cz): its own Q_l plus M_l (c_l - c)(c_l - c)^T
__device__ __forceinline__ void add_leaf_quad(Quad& a, const FarDevice& d, uint32_t l, double cx, double cy, double cz) {
    const double* __restrict__ mo = d.leaf_mom + (size_t)l * 4u;
    const double* __restrict__ lq = d.leaf_quad + (size_t)l * 6u;
    const double m = mo[0];
    double ex = 0.0, ey = 0.0, ez = 0.0;
    if (m != 0.0) { ex = mo[1] / m - cx; ey = mo[2] / m - cy; ez = mo[3] / m - cz; }
    a.xx += lq[0] + m * ex * ex; a.yy += lq[1] + m * ey * ey; a.zz += lq[2] + m * ez * ez;
    a.xy += lq[3] + m * ex * ey; a.xz += lq[4] + m * ex * ez; a.yz += lq[5] + m * ey * ez;
}

__device__ __forceinline__ void write_cell_quad(const FarDevice& d, int dim, uint32_t c, const Quad& Q) {
    const double M = d.cell_mass[c];
    double* __restrict__ o = d.cell_quad + (size_t)c * quad_count(dim);
    float q[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};               // xx, yy, zz, xy, xz, yz, tr
    if (M != 0.0) {
        const double src[7] = {Q.xx, Q.yy, Q.zz, Q.xy, Q.xz, Q.yz, Q.xx + Q.yy + Q.zz};
        bool finite = true;
        for (int k = 0; k < 7; ++k) {
            q[k] = (float)(src[k] / M);
            finite = finite && __builtin_isfinite(q[k]);
        }
        if (!finite)                                                  // mixed-sign masses, M near 0: the monopole alone, never a NaN
            for (int k = 0; k < 7; ++k) q[k] = 0.f;
    }
    if (M == 0.0) {                                                   // a massless cell reports zeros (masses that cancel exactly included)
        for (uint32_t k = 0; k < quad_count(dim); ++k) o[k] = 0.0;
    } else if (dim == 3) {
        o[0] = Q.xx; o[1] = Q.yy; o[2] = Q.zz; o[3] = Q.xy; o[4] = Q.xz; o[5] = Q.yz;
    } else {
        o[0] = Q.xx; o[1] = Q.yy; o[2] = Q.xy;
    }
    if (dim == 3) {
        d.cell_qrec[(size_t)c * 2u] = make_float4(q[0], q[1], q[2], q[3]);
        d.cell_qrec[(size_t)c * 2u + 1u] = make_float4(q[4], q[5], q[6], 0.f);
    } else {
        d.cell_qrec[c] = make_float4(q[0], q[1], q[3], q[6]);
    }
}

__global__ __launch_bounds__(256) void far_small_cells_quad_kernel(FarDevice d, int dim) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= d.n_small) return;
    const uint32_t c = d.small_cells[i];
    const uint32_t lo = d.cell_first[c], n = d.cell_count[c];
    const double cx = d.cell_com[(size_t)c * dim], cy = d.cell_com[(size_t)c * dim + 1], cz = dim == 3 ? d.cell_com[(size_t)c * dim + 2] : 0.0;
    Quad Q;
    for (uint32_t l = lo; l < lo + n; ++l) add_leaf_quad(Q, d, l, cx, cy, cz);
    write_cell_quad(d, dim, c, Q);
}

__global__ __launch_bounds__(kCellThreads) void far_big_cells_quad_kernel(FarDevice d, int dim) {
    __shared__ double red[6][kCellThreads];
    const uint32_t c = d.big_cells[blockIdx.x];
    const uint32_t lo = d.cell_first[c], n = d.cell_count[c];
    const uint32_t tid = threadIdx.x;
    const double cx = d.cell_com[(size_t)c * dim], cy = d.cell_com[(size_t)c * dim + 1], cz = dim == 3 ? d.cell_com[(size_t)c * dim + 2] : 0.0;
    Quad Q;
    for (uint32_t l = tid; l < n; l += kCellThreads) add_leaf_quad(Q, d, lo + l, cx, cy, cz);
    red[0][tid] = Q.xx; red[1][tid] = Q.yy; red[2][tid] = Q.zz; red[3][tid] = Q.xy; red[4][tid] = Q.xz; red[5][tid] = Q.yz;
    __syncthreads();
    for (uint32_t h = kCellThreads / 2u; h >= 1u; h >>= 1) {
        if (tid < h)
            for (int k = 0; k < 6; ++k) red[k][tid] += red[k][tid + h];
        __syncthreads();
    }
    if (tid == 0u) {
        Q.xx = red[0][0]; Q.yy = red[1][0]; Q.zz = red[2][0]; Q.xy = red[3][0]; Q.xz = red[4][0]; Q.yz = red[5][0];
        write_cell_quad(d, dim, c, Q);
    }
}

template <int D, int LAW, int ORDER>
__global__ __launch_bounds__(64) void far_kernel(FarDevice d) {
    __shared__ __attribute__((aligned(16))) float4 tile[kFarTile + kFarTilePad];
    __shared__ double osum[3][64];
    constexpr unsigned QV = quad_rec_vecs(D);                    // float4s of a cell's q record (leaf_far.h)
    float4* qtile = nullptr;
    if constexpr (ORDER == 1) {
        __shared__ __attribute__((aligned(16))) float4 qtile_lds[(kFarTile + kFarTilePad) * QV];
        qtile = qtile_lds;
    }
    const unsigned lane = threadIdx.x;
    const FarBlock b = d.blocks[blockIdx.x];
    const unsigned W = b.count;                                   // 1 .. 64 (plan_far)
    const unsigned fit = 64u / W;
    const unsigned P = fit < kFarMaxLanes ? fit : kFarMaxLanes;
    const unsigned g_raw = lane / W, t = lane - g_raw * W;
    const bool valid = g_raw < P;                                 // lanes left over compute along with group 0, unused
    const unsigned g = valid ? g_raw : 0u;
    const uint32_t pslot = b.first + t;                           // t < W: inside the block's targets
    const float* __restrict__ xf = reinterpret_cast<const float*>(d.xp) + (size_t)(pslot >> 1) * 8u + (pslot & 1u);
    const float ix = xf[0], iy = xf[2], iz = (D == 3) ? xf[4] : 0.0f;
    const f2 ix2 = {ix, ix}, iy2 = {iy, iy}, iz2 = {iz, iz};
    const float4 pad_rec = make_float4(kFar, kFar, (D == 3) ? kFar : 0.0f, 0.0f);
    const float eps2 = LAW == NBX_LAW_NEWTON ? d.eps2 : 0.0f;
    f2 ax = {0.f, 0.f}, ay = {0.f, 0.f}, az = {0.f, 0.f};
    double sx = 0.0, sy = 0.0, sz = 0.0;
    unsigned pending = 0;                                         // wave-uniform
    auto flush = [&]() {
        sx += (double)ax.x + (double)ax.y; sy += (double)ay.x + (double)ay.y;
        if (D == 3) sz += (double)az.x + (double)az.y;
        ax = ay = az = f2{0.f, 0.f};
        pending = 0;
    };
    const uint32_t* __restrict__ list = d.far_cells + b.far_lo;
    constexpr unsigned kPerLane = kFarTile / 64u;
    static_assert(kPerLane == 4, "the gather names four registers");
    // the gather of a tile: indices coalesced, then the records they name (every index was checked against n_cells by validate_cells)
    float4 r0 = pad_rec, r1 = pad_rec, r2_ = pad_rec, r3 = pad_rec;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 qr[kPerLane][QV];                                      // ORDER 1: the q records of the same four entries
    auto gather = [&](const uint32_t base) {
        const uint32_t e0 = base + lane, e1 = e0 + 64u, e2 = e0 + 128u, e3 = e0 + 192u;
        const uint32_t c0 = e0 < b.far_n ? list[e0] : 0xffffffffu, c1 = e1 < b.far_n ? list[e1] : 0xffffffffu;
        const uint32_t c2 = e2 < b.far_n ? list[e2] : 0xffffffffu, c3 = e3 < b.far_n ? list[e3] : 0xffffffffu;
        r0 = c0 != 0xffffffffu ? d.cell_rec[c0] : pad_rec;
        r1 = c1 != 0xffffffffu ? d.cell_rec[c1] : pad_rec;
        r2_ = c2 != 0xffffffffu ? d.cell_rec[c2] : pad_rec;
        r3 = c3 != 0xffffffffu ? d.cell_rec[c3] : pad_rec;
        if constexpr (ORDER == 1) {
            const uint32_t cs[kPerLane] = {c0, c1, c2, c3};
#pragma unroll
            for (unsigned j = 0; j < kPerLane; ++j)
#pragma unroll
                for (unsigned v = 0; v < QV; ++v) qr[j][v] = cs[j] != 0xffffffffu ? d.cell_qrec[(size_t)cs[j] * QV + v] : zero4;
        }
    };
    gather(0u);
    float* const tile_f = reinterpret_cast<float*>(tile);
    // Two tile layouts, chosen per wave.  Many targets (P <= 4 lanes each: a lane walks >= 32 pairs of a tile): records e and e + 1
    // become one SOURCE PAIR {xa,xb,ya,yb},{za,zb,ma,mb}, the pair kernels' layout, read with two ds_read_b128 straight into the
    // register pairs of the packed arithmetic (four ds_write_b32 per record to stage it).  Few targets (small leaves, P up to 16:
    // a lane walks 8 pairs): the records as they are, one ds_write_b128 each, and the loop picks the pairs' halves out of two
    // records (6 more moves per two terms).  Measured at N = 2^20 (profiles/r6/far_field.txt): the pair layout took the pass at 32-body
    // leaves from 0.77 to 0.66 ms; at 4-body leaves the pair layout for every wave cost 1.37 -> 1.68 ms.
    const bool pair_layout = P <= 4u;                             // wave-uniform
    float* const qtile_f = reinterpret_cast<float*>(qtile);
    // ORDER 1: two terms with their q (see the head of the file); ri = 0 leaves exactly the monopole's fma
    auto two_terms_quad = [&](const f2 sx2, const f2 sy2, const f2 sz2, const f2 sm2, const f2 qxx, const f2 qyy, const f2 qzz, const f2 qxy,
                              const f2 qxz, const f2 qyz, const f2 qtr) {
        if (pending + 2u > kFlushTerms) flush();
        const f2 dx = sx2 - ix2, dy = sy2 - iy2;
        const f2 dz = (D == 3) ? sz2 - iz2 : f2{0.f, 0.f};
        f2 r2 = dx * dx;
        r2 = __builtin_elementwise_fma(dy, dy, r2);
        if (D == 3) r2 = __builtin_elementwise_fma(dz, dz, r2);
        float ria, rib;
        const f2 w = {leaf_weight_ri<D, LAW>(r2.x, sm2.x, dx.x, dy.x, dz.x, ria, eps2), leaf_weight_ri<D, LAW>(r2.y, sm2.y, dx.y, dy.y, dz.y, rib, eps2)};
        const f2 ri = {ria, rib};
        const f2 ux = dx * ri, uy = dy * ri;
        f2 gx = qxx * ux, gy = qxy * ux, gz = {0.f, 0.f};        // g = q u
        gx = __builtin_elementwise_fma(qxy, uy, gx);
        gy = __builtin_elementwise_fma(qyy, uy, gy);
        f2 uz = {0.f, 0.f};
        if (D == 3) {
            uz = dz * ri;
            gx = __builtin_elementwise_fma(qxz, uz, gx);
            gy = __builtin_elementwise_fma(qyz, uz, gy);
            gz = qxz * ux;
            gz = __builtin_elementwise_fma(qyz, uy, gz);
            gz = __builtin_elementwise_fma(qzz, uz, gz);
        }
        f2 uqu = ux * gx;
        uqu = __builtin_elementwise_fma(uy, gy, uqu);
        if (D == 3) uqu = __builtin_elementwise_fma(uz, gz, uqu);
        // the term's three coefficients: of tr(q) / r^2, of u^T q u and of q u (d / r^4: 2, 12, 4; softened Newton: 3/2, 15/2, 3)
        constexpr float kTr = LAW == NBX_LAW_NEWTON ? 1.5f : 2.f, kUqu = LAW == NBX_LAW_NEWTON ? 7.5f : 12.f, kQu = LAW == NBX_LAW_NEWTON ? 3.f : 4.f;
        const f2 one = {1.f, 1.f}, twelve = {kUqu, kUqu}, m2 = {-kTr, -kTr}, m4 = {-kQu, -kQu};
        f2 sc = __builtin_elementwise_fma(m2 * qtr, ri, one);
        sc = __builtin_elementwise_fma(twelve, uqu, sc);
        const f2 vx = __builtin_elementwise_fma(sc, dx, m4 * gx), vy = __builtin_elementwise_fma(sc, dy, m4 * gy);
        ax = __builtin_elementwise_fma(w, vx, ax);
        ay = __builtin_elementwise_fma(w, vy, ay);
        if (D == 3) {
            const f2 vz = __builtin_elementwise_fma(sc, dz, m4 * gz);
            az = __builtin_elementwise_fma(w, vz, az);
        }
        pending += 2u;
    };
    auto two_terms = [&](const f2 sx2, const f2 sy2, const f2 sz2, const f2 sm2) {
        if (pending + 2u > kFlushTerms) flush();
        const f2 dx = sx2 - ix2, dy = sy2 - iy2;
        const f2 dz = (D == 3) ? sz2 - iz2 : f2{0.f, 0.f};
        f2 r2 = dx * dx;
        r2 = __builtin_elementwise_fma(dy, dy, r2);
        if (D == 3) r2 = __builtin_elementwise_fma(dz, dz, r2);
        const f2 w = {leaf_weight<D, LAW>(r2.x, sm2.x, dx.x, dy.x, dz.x, eps2), leaf_weight<D, LAW>(r2.y, sm2.y, dx.y, dy.y, dz.y, eps2)};
        ax = __builtin_elementwise_fma(w, dx, ax);
        ay = __builtin_elementwise_fma(w, dy, ay);
        if (D == 3) az = __builtin_elementwise_fma(w, dz, az);
        pending += 2u;
    };
    for (uint32_t base = 0; base < b.far_n; base += kFarTile) {
        const unsigned cur = (b.far_n - base < kFarTile) ? (unsigned)(b.far_n - base) : kFarTile;
        __syncthreads();                                          // the previous tile is consumed
        // every record of the tile and its pad is written: entries past `cur` are pad records
        if (pair_layout) {
            auto put = [&](const unsigned e, const float4 r) {
                float* __restrict__ o = tile_f + (e >> 1) * 8u + (e & 1u);
                o[0] = r.x; o[2] = r.y; o[4] = r.z; o[6] = r.w;
            };
            put(lane, r0); put(lane + 64u, r1); put(lane + 128u, r2_); put(lane + 192u, r3);
            put(kFarTile + lane, pad_rec);
            if constexpr (ORDER == 1) {
                // a pair of q records interleaved like the source pair: {xxa,xxb,yya,yyb},{zza,zzb,xya,xyb},{xza,xzb,yza,yzb},{tra,trb,-,-}
                // in 3D, {xxa,xxb,yya,yyb},{xya,xyb,tra,trb} in 2D
                auto putq = [&](const unsigned e, const float4 (&q)[QV]) {
                    float* __restrict__ o = qtile_f + (e >> 1) * (8u * QV) + (e & 1u);
                    o[0] = q[0].x; o[2] = q[0].y; o[4] = q[0].z; o[6] = q[0].w;
                    if (QV == 2u) { o[8] = q[QV - 1u].x; o[10] = q[QV - 1u].y; o[12] = q[QV - 1u].z; }
                };
                float4 zq[QV];
                for (unsigned v = 0; v < QV; ++v) zq[v] = zero4;
                putq(lane, qr[0]); putq(lane + 64u, qr[1]); putq(lane + 128u, qr[2]); putq(lane + 192u, qr[3]);
                putq(kFarTile + lane, zq);
            }
        } else {
            tile[lane] = r0; tile[lane + 64u] = r1; tile[lane + 128u] = r2_; tile[lane + 192u] = r3;
            tile[kFarTile + lane] = pad_rec;
            if constexpr (ORDER == 1) {
#pragma unroll
                for (unsigned v = 0; v < QV; ++v) {
                    qtile[lane * QV + v] = qr[0][v]; qtile[(lane + 64u) * QV + v] = qr[1][v];
                    qtile[(lane + 128u) * QV + v] = qr[2][v]; qtile[(lane + 192u) * QV + v] = qr[3][v];
                    qtile[(kFarTile + lane) * QV + v] = zero4;
                }
            }
        }
        __syncthreads();
        if (base + kFarTile < b.far_n) gather(base + kFarTile);   // in flight while this tile is consumed
        // record pairs per lane group.  Pair layout: ceil(pairs / P) made odd (the groups' addresses then differ by odd multiples of
        // 32 B); record layout: ceil(ceil(cur / P) / 2) -- with 16 groups of 8 pairs an odd count would be 9, an eighth more terms.
        // Either way P T <= pairs + 2 P - 1, so 2 P T <= kFarTile + kFarTilePad records.
        const unsigned pairs = (cur + 1u) >> 1;
        const unsigned T = pair_layout ? (((pairs + P - 1u) / P) | 1u) : ((((cur + P - 1u) / P) + 1u) >> 1);
        const float4* __restrict__ s = tile + 2u * g * T;
        if constexpr (ORDER == 1) {
            const float4* __restrict__ qs = qtile + 2u * QV * g * T;   // the same records' q: 2 QV float4 per pair in either layout
            if (pair_layout) {
                for (unsigned i = 0; i < T; ++i) {
                    const float4 A = s[2u * i], B = s[2u * i + 1u];
                    if (D == 3) {
                        const float4 Q0 = qs[4u * i], Q1 = qs[4u * i + 1u], Q2 = qs[4u * i + 2u];
                        const f2 Q3 = *reinterpret_cast<const f2*>(qs + 4u * i + 3u);
                        two_terms_quad(f2{A.x, A.y}, f2{A.z, A.w}, f2{B.x, B.y}, f2{B.z, B.w}, f2{Q0.x, Q0.y}, f2{Q0.z, Q0.w}, f2{Q1.x, Q1.y},
                                       f2{Q1.z, Q1.w}, f2{Q2.x, Q2.y}, f2{Q2.z, Q2.w}, Q3);
                    } else {
                        const float4 Q0 = qs[2u * i], Q1 = qs[2u * i + 1u];
                        two_terms_quad(f2{A.x, A.y}, f2{A.z, A.w}, f2{B.x, B.y}, f2{B.z, B.w}, f2{Q0.x, Q0.y}, f2{Q0.z, Q0.w}, f2{0.f, 0.f},
                                       f2{Q1.x, Q1.y}, f2{0.f, 0.f}, f2{0.f, 0.f}, f2{Q1.z, Q1.w});
                    }
                }
            } else {
                for (unsigned i = 0; i < T; ++i) {
                    const float4 A = s[2u * i], B = s[2u * i + 1u];
                    if (D == 3) {
                        const float4 A0 = qs[4u * i], A1 = qs[4u * i + 1u], B0 = qs[4u * i + 2u], B1 = qs[4u * i + 3u];
                        two_terms_quad(f2{A.x, B.x}, f2{A.y, B.y}, f2{A.z, B.z}, f2{A.w, B.w}, f2{A0.x, B0.x}, f2{A0.y, B0.y}, f2{A0.z, B0.z},
                                       f2{A0.w, B0.w}, f2{A1.x, B1.x}, f2{A1.y, B1.y}, f2{A1.z, B1.z});
                    } else {
                        const float4 A0 = qs[2u * i], B0 = qs[2u * i + 1u];
                        two_terms_quad(f2{A.x, B.x}, f2{A.y, B.y}, f2{A.z, B.z}, f2{A.w, B.w}, f2{A0.x, B0.x}, f2{A0.y, B0.y}, f2{0.f, 0.f},
                                       f2{A0.z, B0.z}, f2{0.f, 0.f}, f2{0.f, 0.f}, f2{A0.w, B0.w});
                    }
                }
            }
        } else if (pair_layout) {
            for (unsigned i = 0; i < T; ++i) {
                const float4 A = s[2u * i], B = s[2u * i + 1u];
                two_terms(f2{A.x, A.y}, f2{A.z, A.w}, f2{B.x, B.y}, f2{B.z, B.w});
            }
        } else {
            for (unsigned i = 0; i < T; ++i) {
                const float4 A = s[2u * i], B = s[2u * i + 1u];
                two_terms(f2{A.x, B.x}, f2{A.y, B.y}, f2{A.z, B.z}, f2{A.w, B.w});
            }
        }
    }
    flush();
    osum[0][lane] = sx; osum[1][lane] = sy; osum[2][lane] = sz;
    __syncthreads();
    if (valid && g == 0u) {                                       // the lane groups' sums meet in group order
        double ox = 0.0, oy = 0.0, oz = 0.0;
        for (unsigned q = 0; q < P; ++q) { ox += osum[0][t + q * W]; oy += osum[1][t + q * W]; oz += osum[2][t + q * W]; }
        d.sums[pslot] += ox;
        d.sums[(size_t)d.pslots + pslot] += oy;
        if (D == 3) d.sums[2 * (size_t)d.pslots + pslot] += oz;
    }
}

typedef void (*FarKernel)(FarDevice);
FarKernel pick_far(int dim, int law, int order) {
    static const FarKernel table[2][2][4] = {
        {{far_kernel<2, NBX_LAW_BRUTE, 0>, far_kernel<2, NBX_LAW_TREE_LEAF, 0>, far_kernel<2, NBX_LAW_FMM_P2P, 0>, far_kernel<2, NBX_LAW_NEWTON, 0>},
         {far_kernel<3, NBX_LAW_BRUTE, 0>, far_kernel<3, NBX_LAW_TREE_LEAF, 0>, far_kernel<3, NBX_LAW_FMM_P2P, 0>, far_kernel<3, NBX_LAW_NEWTON, 0>}},
        {{far_kernel<2, NBX_LAW_BRUTE, 1>, far_kernel<2, NBX_LAW_TREE_LEAF, 1>, far_kernel<2, NBX_LAW_FMM_P2P, 1>, far_kernel<2, NBX_LAW_NEWTON, 1>},
         {far_kernel<3, NBX_LAW_BRUTE, 1>, far_kernel<3, NBX_LAW_TREE_LEAF, 1>, far_kernel<3, NBX_LAW_FMM_P2P, 1>, far_kernel<3, NBX_LAW_NEWTON, 1>}}};
    return table[order][dim - 2][law];
}

}  // namespace

hipError_t enqueue_moments(const FarDevice& d, int dim, hipStream_t s) {
    if (!d.n_cells) return hipSuccess;
    (void)hipGetLastError();
    if (d.n_leaves) {
        const size_t lanes = (size_t)d.n_leaves * kLeafLanes;
        hipLaunchKernelGGL(far_leaf_moments_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float*>(d.xp), d.unit_off,
                           d.n_leaves, dim, d.leaf_mom);
    }
    if (d.n_small) hipLaunchKernelGGL(far_small_cells_kernel, dim3((d.n_small + 255u) / 256u), dim3(256), 0, s, d, dim);
    if (d.n_big) hipLaunchKernelGGL(far_big_cells_kernel, dim3(d.n_big), dim3(kCellThreads), 0, s, d, dim);
    if (d.order == 1) {
        if (d.n_leaves) {
            const size_t lanes = (size_t)d.n_leaves * kLeafLanes;
            hipLaunchKernelGGL(far_leaf_quad_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float*>(d.xp),
                               d.unit_off, d.n_leaves, dim, d.leaf_mom, d.leaf_quad);
        }
        if (d.n_small) hipLaunchKernelGGL(far_small_cells_quad_kernel, dim3((d.n_small + 255u) / 256u), dim3(256), 0, s, d, dim);
        if (d.n_big) hipLaunchKernelGGL(far_big_cells_quad_kernel, dim3(d.n_big), dim3(kCellThreads), 0, s, d, dim);
    }
    return hipGetLastError();
}

hipError_t enqueue_far(const FarDevice& d, int dim, int law, hipStream_t s) {
    if (!d.n_blocks) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(pick_far(dim, law, d.order == 1 ? 1 : 0), dim3(d.n_blocks), dim3(64), 0, s, d);
    return hipGetLastError();
}

}  // namespace nbx_far
