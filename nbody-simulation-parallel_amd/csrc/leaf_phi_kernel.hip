// leaf_phi_kernel.hip -- the potential of a leaf plan: per target slot, the law's PAIR POTENTIAL w summed over what the force passes
// sum the gradient of (leaf_pair_kernel.hip, leaf_far_kernel.hip):
//   phi_i = sum over bodies j != i of the leaves on the target leaf's near list of  m_j w(r_ij)
//         + sum over the cells c on its far list of                                 Phi_c(R),   R = com_c - p_i
//   NBX_LAW_NEWTON                 w = 1 / rho, rho^2 = r^2 + eps^2; the body itself is left out by IDENTITY (same slot): two different
//                                  bodies at one position count m_j / eps
//   NBX_LAW_BRUTE / _TREE_LEAF     w = 1 / (2 r^2); pairs below the law's threshold (1e-10 / 1e-9) are skipped, the body itself among them
// The kernels sum m_j / rho and m_j / r^2; the reference laws' factor 1/2, G, m_i and the sign are applied in fp64 behind the sums.
// Both passes walk the tables a plan already holds and change none of them.
//  * near_phi_kernel<D, LAW>: one wave64 per WORK ITEM -- a LeafBlock piece with count > 0, or a PackSub: (first, count) names its
//    targets, (op_lo, op_n) its copy runs, and together the items cover every target slot of a leaf exactly once (leaf_plan.h: a leaf is
//    either packed, one PackSub, or cut into the pieces of its LeafBlocks).  The wave takes the leaf's copy runs kNearOps at a time into
//    LDS (one coalesced load) and the stream they cover in tiles of kNearTilePairs source pairs: every lane finds the run of its pairs
//    by bisection in LDS and loads them, all loads in flight together; the source's slot is `base + position` of its run (CopyOp) and
//    rides with the pair.  A target is shared by P = min(64 / count, 32) lanes; lane group g takes pairs g, g + P, ... of the tile
//    (the lanes of a group read one LDS address).  One v_rsq_f32 (NEWTON) or one v_rcp_f32 behind the threshold select (reference
//    laws) and one multiply per pair; eps^2 is the bias of r^2.  A pad is massless at 1e18: rsq(3e36) = 6e-19 and rcp(3e36) = 3e-37
//    are normal numbers, times 0: exact zeros.  (A first form that streamed every lane group's pairs straight from memory, each lane
//    walking the run table there, was bound by the latency of those dependent loads: 2.4 / 3.9 ms at N = 2^20 where this one takes
//    1.0-1.25 / 2.5-2.85 ms, profiles/r13/tree_energy.txt.)
//  * far_phi_kernel<D, LAW, ORDER>: one wave64 per FarBlock, the cells' records staged in LDS in tiles of kFarTile as far_kernel
//    gathers them; lane group g takes records g, g + P, ... of the tile.  With q = Q / M, t = tr q and u = R / rho^2 (R / r^2: |u| = 1 / r,
//    nothing overflows at a pad's 1e18):
//      NEWTON     (M / rho)  [ 1 - t / (2 rho^2) + (3/2) u^T q u ]
//      reference  (M / r^2)  [ 1 - t / r^2       + 4     u^T q u ]      (x 1/2 behind the sums)
//    ORDER 0 is the bracket left out.  Where the law skips the pair with the pseudo-body the reciprocal is 0 and so is the whole term;
//    a cell of mass 0 is the pad record; an all-zero q record makes the bracket exactly 1: the monopole's bits.
// fp32 terms, at most kFlushTerms of them in a lane's fp32 sum between flushes into its fp64 sum; the lane groups' fp64 sums meet in
// LDS in group order; one lane per target writes (near) or adds to (far) phi[slot].  No atomics, one writer per word.
//  * phi_by_body_kernel, energy_partials_kernel: phi by body through body_slot, and the per-workgroup fp64 partials of sum m_i phi_i and
//    sum m_i |v_i|^2 that the host adds in index order (state_kernels.hip's energy_partials_kernel has the same shape).
#include "leaf_phi.h"
#include "leaf_law.h"

using namespace nbx_leaf;

namespace nbx_phi {
namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

template <int LAW>
__device__ __forceinline__ constexpr float skip_below() { return LAW == NBX_LAW_BRUTE ? nbx::kR2SkipF : kTreeSkipF; }

template <int D, int LAW>
__global__ __launch_bounds__(64) void near_phi_kernel(PhiDevice d) {
    __shared__ __attribute__((aligned(16))) float4 tile[2u * kNearTilePairs];   // source pairs as they lie in xp: {xa,xb,ya,yb},{za,zb,ma,mb}
    __shared__ uint32_t tile_slot[kNearTilePairs];                               // slot of each pair's first body
    __shared__ uint32_t op_end[kNearOps], op_base[kNearOps];
    __shared__ double osum[64];
    const unsigned lane = threadIdx.x;
    const uint32_t item = blockIdx.x;
    uint32_t first, count, op_lo, op_n;
    if (item < 2u * d.n_blocks) {
        const LeafBlock* __restrict__ b = d.blocks + (item >> 1);
        const Piece pc = b->piece[item & 1u];
        first = pc.first; count = pc.count; op_lo = b->op_lo; op_n = b->op_n;
    } else {
        const PackSub sb = d.subs[item - 2u * d.n_blocks];
        first = sb.first; count = sb.count; op_lo = sb.op_lo; op_n = sb.op_n;
    }
    if (count == 0u || count > 64u || first + count > d.pslots) return;   // wave-uniform: a wave that only helped staging owns no target
    const unsigned W = count;
    const unsigned fit = 64u / W;
    const unsigned P = fit < kNearMaxLanes ? fit : kNearMaxLanes;
    const unsigned g = lane / W, t = lane - g * W;
    const bool valid = g < P;                                     // lanes left over sum nothing
    const uint32_t tslot = first + t;
    const float* __restrict__ xf = reinterpret_cast<const float*>(d.xp) + (size_t)(tslot >> 1) * 8u + (tslot & 1u);
    const float ix = xf[0], iy = xf[2], iz = (D == 3) ? xf[4] : 0.0f;
    const f2 ix2 = {ix, ix}, iy2 = {iy, iy}, iz2 = {iz, iz};
    const float eps2 = LAW == NBX_LAW_NEWTON ? d.eps2 : 0.0f;
    const f2 bias = {eps2, eps2};
    f2 acc = {0.f, 0.f};
    double sum = 0.0;
    unsigned pending = 0;
    // The leaf's copy runs kNearOps at a time (one coalesced load into LDS), and the stretch of the stream they cover in tiles of
    // kNearTilePairs source pairs: every lane finds the run of its pairs by bisection in LDS and loads them (independent loads, all in
    // flight together); then lane group g takes pairs g, g + P, ... of the tile.  Everything that steers a loop is wave-uniform.
    for (uint32_t c0 = 0; c0 < op_n; c0 += kNearOps) {
        const uint32_t n_ops = op_n - c0 < kNearOps ? op_n - c0 : kNearOps;
        __syncthreads();                                          // the previous chunk's runs are no longer looked up
        if (lane < n_ops) {
            const CopyOp o = d.ops[op_lo + c0 + lane];
            op_end[lane] = o.end; op_base[lane] = o.base;
        }
        const uint32_t p_begin = (c0 ? d.ops[op_lo + c0 - 1u].end : 0u) >> 1;   // streams are whole pairs (every leaf is padded to an even size)
        __syncthreads();
        const uint32_t p_end = op_end[n_ops - 1u] >> 1;
        for (uint32_t tb = p_begin; tb < p_end; tb += kNearTilePairs) {
            const unsigned cur = p_end - tb < kNearTilePairs ? (unsigned)(p_end - tb) : kNearTilePairs;
            __syncthreads();                                      // the previous tile is consumed
            for (unsigned j = lane; j < cur; j += 64u) {
                const uint32_t pos = 2u * (tb + j);
                unsigned lo = 0, hi = n_ops - 1u;                 // the first run that ends behind pos (there is one: pos < 2 p_end)
                while (lo < hi) {
                    const unsigned mid = (lo + hi) >> 1;
                    if (op_end[mid] > pos) hi = mid; else lo = mid + 1u;
                }
                const uint32_t slot = op_base[lo] + pos;          // base + position: an even slot, the pair's two float4 lie side by side
                const bool ok = slot < d.pslots;                  // never false on a validated plan: nothing outside xp is read
                const uint32_t at = ok ? slot : 0u;
                float4 A = d.xp[at], B = d.xp[at + 1u];
                if (!ok) { A.x = A.y = A.z = A.w = kFar; B.x = B.y = (D == 3) ? kFar : 0.0f; B.z = B.w = 0.0f; }
                tile[2u * j] = A; tile[2u * j + 1u] = B;
                tile_slot[j] = slot;
            }
            __syncthreads();
            if (!valid) continue;
            for (unsigned j = g; j < cur; j += P) {
                const float4 A = tile[2u * j], B = tile[2u * j + 1u];
                const uint32_t slot = tile_slot[j];
                if (pending + 2u > kFlushTerms) { sum += (double)acc.x + (double)acc.y; acc = f2{0.f, 0.f}; pending = 0; }
                const f2 dx = f2{A.x, A.y} - ix2, dy = f2{A.z, A.w} - iy2;
                f2 r2 = __builtin_elementwise_fma(dx, dx, bias);
                r2 = __builtin_elementwise_fma(dy, dy, r2);
                if (D == 3) {
                    const f2 dz = f2{B.x, B.y} - iz2;
                    r2 = __builtin_elementwise_fma(dz, dz, r2);
                }
                const f2 sm = {B.z, B.w};
                f2 w;
                if (LAW == NBX_LAW_NEWTON) {
                    w = f2{__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)} * sm;
                    if (slot == tslot) w.x = 0.f;                  // the body itself, by identity
                    if (slot + 1u == tslot) w.y = 0.f;
                } else {
                    const float ga = r2.x < skip_below<LAW>() ? __builtin_inff() : r2.x, gb = r2.y < skip_below<LAW>() ? __builtin_inff() : r2.y;
                    w = f2{__builtin_amdgcn_rcpf(ga), __builtin_amdgcn_rcpf(gb)} * sm;
                }
                acc += w;
                pending += 2u;
            }
        }
    }
    sum += (double)acc.x + (double)acc.y;
    osum[lane] = sum;
    __syncthreads();
    if (g == 0u) {                                                // the lane groups' sums meet in group order
        double o = 0.0;
        for (unsigned j = 0; j < P; ++j) o += osum[t + j * W];
        d.phi[tslot] = o;
    }
}

template <int D, int LAW, int ORDER>
__global__ __launch_bounds__(64) void far_phi_kernel(nbx_far::FarDevice d, double* __restrict__ phi) {
    using namespace nbx_far;
    constexpr unsigned QV = quad_rec_vecs(D);
    __shared__ __attribute__((aligned(16))) float4 tile[kFarTile];
    __shared__ __attribute__((aligned(16))) float4 qtile[ORDER == 1 ? kFarTile * QV : 1u];
    __shared__ double osum[64];
    const unsigned lane = threadIdx.x;
    const FarBlock b = d.blocks[blockIdx.x];
    const unsigned W = b.count;
    if (W == 0u || W > 64u || b.first + W > d.pslots) return;     // wave-uniform; never by a validated plan
    const unsigned fit = 64u / W;
    const unsigned P = fit < kFarMaxLanes ? fit : kFarMaxLanes;
    const unsigned g = lane / W, t = lane - g * W;
    const bool valid = g < P;
    const uint32_t pslot = b.first + t;
    const float* __restrict__ xf = reinterpret_cast<const float*>(d.xp) + (size_t)(pslot >> 1) * 8u + (pslot & 1u);
    const float ix = xf[0], iy = xf[2], iz = (D == 3) ? xf[4] : 0.0f;
    const float eps2 = LAW == NBX_LAW_NEWTON ? d.eps2 : 0.0f;
    const uint32_t* __restrict__ list = d.far_cells + b.far_lo;
    float acc = 0.f;
    double sum = 0.0;
    unsigned pending = 0;
    for (uint32_t base = 0; base < b.far_n; base += kFarTile) {
        const unsigned cur = (b.far_n - base < kFarTile) ? (unsigned)(b.far_n - base) : kFarTile;
        __syncthreads();                                          // the previous tile is consumed
        for (unsigned e = lane; e < cur; e += 64u) {              // indices coalesced, then the records they name
            const uint32_t c = list[base + e];
            const bool ok = c < d.n_cells;                        // every index was checked when the cells were set
            const uint32_t cc = ok ? c : 0u;                      // (n_cells > 0: the launch has cells)
            float4 r = d.cell_rec[cc];
            if (!ok) { r.x = kFar; r.y = kFar; r.z = (D == 3) ? kFar : 0.0f; r.w = 0.0f; }
            tile[e] = r;
            if constexpr (ORDER == 1) {
#pragma unroll
                for (unsigned v = 0; v < QV; ++v) {
                    float4 q = d.cell_qrec[(size_t)cc * QV + v];
                    if (!ok) { q.x = 0.f; q.y = 0.f; q.z = 0.f; q.w = 0.f; }
                    qtile[e * QV + v] = q;
                }
            }
        }
        __syncthreads();
        if (!valid) continue;
        for (unsigned e = g; e < cur; e += P) {
            // a term is rounded before it is added, at either order: with an all-zero q the bracket is exactly 1 and order 1 adds the
            // monopole's very bits (contracted, order 0 would add rs M unrounded and order 1 the rounded product times 1)
#pragma clang fp contract(off)
            const float4 r = tile[e];
            if (pending + 1u > kFlushTerms) { sum += (double)acc; acc = 0.f; pending = 0; }
            const float dx = r.x - ix, dy = r.y - iy, dz = (D == 3) ? r.z - iz : 0.0f;
            float r2 = __builtin_fmaf(dx, dx, eps2);
            r2 = __builtin_fmaf(dy, dy, r2);
            if (D == 3) r2 = __builtin_fmaf(dz, dz, r2);
            float ri, w;                                          // 1 / rho^2 (1 / r^2), and the monopole's term
            if (LAW == NBX_LAW_NEWTON) {
                const float rs = __builtin_amdgcn_rsqf(r2);
                ri = rs * rs;
                w = rs * r.w;
            } else {
                ri = __builtin_amdgcn_rcpf(r2 < skip_below<LAW>() ? __builtin_inff() : r2);
                w = ri * r.w;
            }
            if constexpr (ORDER == 1) {
                float qxx, qyy, qzz = 0.f, qxy, qxz = 0.f, qyz = 0.f, qtr;
                if (D == 3) {
                    const float4 q0 = qtile[e * QV], q1 = qtile[e * QV + (QV - 1u)];
                    qxx = q0.x; qyy = q0.y; qzz = q0.z; qxy = q0.w; qxz = q1.x; qyz = q1.y; qtr = q1.z;
                } else {
                    const float4 q0 = qtile[e * QV];
                    qxx = q0.x; qyy = q0.y; qxy = q0.z; qtr = q0.w;
                }
                const float ux = dx * ri, uy = dy * ri, uz = dz * ri;
                float gx = qxx * ux, gy = qxy * ux, gz = 0.f;       // q u
                gx = __builtin_fmaf(qxy, uy, gx);
                gy = __builtin_fmaf(qyy, uy, gy);
                if (D == 3) {
                    gx = __builtin_fmaf(qxz, uz, gx);
                    gy = __builtin_fmaf(qyz, uz, gy);
                    gz = qxz * ux;
                    gz = __builtin_fmaf(qyz, uy, gz);
                    gz = __builtin_fmaf(qzz, uz, gz);
                }
                float uqu = ux * gx;
                uqu = __builtin_fmaf(uy, gy, uqu);
                if (D == 3) uqu = __builtin_fmaf(uz, gz, uqu);
                constexpr float kTr = LAW == NBX_LAW_NEWTON ? 0.5f : 1.f, kUqu = LAW == NBX_LAW_NEWTON ? 1.5f : 4.f;
                float sc = __builtin_fmaf(-kTr * qtr, ri, 1.f);
                sc = __builtin_fmaf(kUqu, uqu, sc);
                w *= sc;
            }
            acc += w;
            pending += 1u;
        }
    }
    sum += (double)acc;
    osum[lane] = sum;
    __syncthreads();
    if (g == 0u) {                                                // the lane groups' sums meet in group order
        double o = 0.0;
        for (unsigned j = 0; j < P; ++j) o += osum[t + j * W];
        phi[pslot] += o;
    }
}

__global__ __launch_bounds__(256) void phi_by_body_kernel(const double* __restrict__ phi, const uint32_t* __restrict__ body_slot, size_t n, double factor,
                                                          double* __restrict__ phi_body) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = body_slot[i];
    phi_body[i] = s != 0xffffffffu ? factor * phi[s] : 0.0;
}

__global__ __launch_bounds__(256) void energy_partials_kernel(const double* __restrict__ phi_body, size_t n, int dim, unsigned pad,
                                                              const double* __restrict__ v64, const double* __restrict__ m64, double* __restrict__ out) {
    __shared__ double wave_mv2[4], wave_mphi[4];
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    double mv2 = 0.0, mphi = 0.0;
    if (l < n) {
        double v2 = 0.0;
        for (int k = 0; k < dim; ++k) { const double v = v64[(size_t)k * pad + l]; v2 += v * v; }
        const double m = m64[l];
        mv2 = m * v2;
        mphi = m * phi_body[l];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mv2 += __shfl_down(mv2, off, 64);
        mphi += __shfl_down(mphi, off, 64);
    }
    if ((threadIdx.x & 63u) == 0) { wave_mv2[threadIdx.x >> 6] = mv2; wave_mphi[threadIdx.x >> 6] = mphi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[blockIdx.x] = ((wave_mv2[0] + wave_mv2[1]) + wave_mv2[2]) + wave_mv2[3];
        out[gridDim.x + blockIdx.x] = ((wave_mphi[0] + wave_mphi[1]) + wave_mphi[2]) + wave_mphi[3];
    }
}

typedef void (*NearKernel)(PhiDevice);
NearKernel pick_near(int dim, int law) {
    if (dim == 2) return law == NBX_LAW_NEWTON ? near_phi_kernel<2, NBX_LAW_NEWTON> : law == NBX_LAW_BRUTE ? near_phi_kernel<2, NBX_LAW_BRUTE> : near_phi_kernel<2, NBX_LAW_TREE_LEAF>;
    return law == NBX_LAW_NEWTON ? near_phi_kernel<3, NBX_LAW_NEWTON> : law == NBX_LAW_BRUTE ? near_phi_kernel<3, NBX_LAW_BRUTE> : near_phi_kernel<3, NBX_LAW_TREE_LEAF>;
}

typedef void (*FarKernel)(nbx_far::FarDevice, double*);
template <int D, int ORDER>
FarKernel pick_far_law(int law) {
    return law == NBX_LAW_NEWTON ? far_phi_kernel<D, NBX_LAW_NEWTON, ORDER> : law == NBX_LAW_BRUTE ? far_phi_kernel<D, NBX_LAW_BRUTE, ORDER> : far_phi_kernel<D, NBX_LAW_TREE_LEAF, ORDER>;
}
FarKernel pick_far(int dim, int law, int order) {
    if (dim == 2) return order == 1 ? pick_far_law<2, 1>(law) : pick_far_law<2, 0>(law);
    return order == 1 ? pick_far_law<3, 1>(law) : pick_far_law<3, 0>(law);
}

bool law_has_potential(int law) { return law == NBX_LAW_BRUTE || law == NBX_LAW_TREE_LEAF || law == NBX_LAW_NEWTON; }

}  // namespace

hipError_t enqueue_near_phi(const PhiDevice& d, int dim, int law, hipStream_t s) {
    if ((dim != 2 && dim != 3) || !law_has_potential(law)) return hipErrorInvalidValue;   // a missing kernel is an error, never another law's
    const uint64_t items = 2ull * d.n_blocks + d.n_subs;
    if (!items) return hipSuccess;
    if (items > 0x7fffffffull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(pick_near(dim, law), dim3((unsigned)items), dim3(64), 0, s, d);
    return hipGetLastError();
}

hipError_t enqueue_far_phi(const nbx_far::FarDevice& f, double* phi, int dim, int law, hipStream_t s) {
    if ((dim != 2 && dim != 3) || !law_has_potential(law)) return hipErrorInvalidValue;
    if (!f.n_cells || !f.n_blocks) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(pick_far(dim, law, f.order == 1 ? 1 : 0), dim3(f.n_blocks), dim3(64), 0, s, f, phi);
    return hipGetLastError();
}

hipError_t enqueue_phi_by_body(const double* phi, const uint32_t* body_slot, size_t n, double factor, double* phi_body, hipStream_t s) {
    if (!n) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(phi_by_body_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, phi, body_slot, n, factor, phi_body);
    return hipGetLastError();
}

hipError_t enqueue_energy_partials(const double* phi_body, size_t n, int dim, unsigned pad, const double* v64, const double* m64, double* out,
                                   hipStream_t s) {
    if (!n) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(energy_partials_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, phi_body, n, dim, pad, v64, m64, out);
    return hipGetLastError();
}

}  // namespace nbx_phi
