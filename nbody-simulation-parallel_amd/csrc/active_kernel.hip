// active_kernel.hip -- forces on a device-resident list of targets (nbx_ctx_compute_accel_active; the force evaluation of
// nbx_ctx_step_kdk_block), gfx950, fp32 pair arithmetic, D = 2 or 3, softened laws only.
//
// For the targets list[0 .. n), n read from device memory, against ALL `pad` entries of chunk 0:
//     a_r = sum_j  m_j d / rho^4   (law 0)   or   m_j d / rho^3   (law 1),      d = p_j - p_list[r],  rho^2 = r^2 + eps^2 .
// The pair arithmetic is the default kernel's softened builds (force_kernel.hip interact2_staged: fp32 d, the bias eps^2 folded into
// the first fma of r^2, v_rcp_f32 / v_rsq_f32, the mass applied last); a body and itself (d = 0, weight finite by the context's
// m / eps^p rule) and the pad entries (mass 0 at the origin) give exactly 0, so there is no compare.  Each row is evaluated by
// itself: the list may be in any order and may repeat an index.
//
// The host knows neither n nor which shape fits it, so it queues BOTH builds for the list's capacity and each returns at once
// unless n is on its side of ActiveArgs::long_list (nbx_internal.h's active_layout is all either needs):
//   TPL = 1  the short list -- the two bodies of a binary against a million sources.  One target per lane, 256 per list block, and
//            the sources cut into as many slices as the buffer allows, up to 256 (the mixed mode's fp64 list pass has this layout).
//   TPL = 8  the long list -- a synchronisation point, every body active.  K1's shape: four float2 target pairs per lane, packed
//            fp32 arithmetic, 2,048 targets per workgroup, one ds_read_b128 broadcast feeding 512 pair terms per wave.
// Work is dealt in items, (list block, source slice) pairs with the slice running fastest: workgroup w takes items w, w + G, ... of a
// one-dimensional grid of G workgroups.  Consecutive workgroups -- dealt round-robin to the XCDs -- are then the slices of ONE list
// block, so a list of one block still lands on every XCD and CU, and with 8 | slices an XCD keeps meeting the same eighth of the
// sources.  The grid is sized on the host for the capacity, but never beyond 4,096 workgroups: a two-dimensional grid of every slice
// x every block that a list of the capacity COULD have (131,072 workgroups at N = 2^20, of which a full list uses 4,096) spent four
// times the pair loop's time on workgroups that only read the length and left (profiles/r19/block_steps.txt).
// Summation: fp32 over one 256-source tile, the tile's sum flushed into an fp64 sum per (target, slice); active_fold_kernel adds the
// slices in slice order in fp64.  No atomics: the same list gives the same bits.
#include "nbx_internal.h"

namespace nbx {
namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

template <int D, int TPL, int NEWTON>
__global__ __launch_bounds__(256, TPL > 1 ? 3 : 4) void active_accel_kernel(ActiveArgs a) {
    constexpr int PAIRS = TPL > 1 ? TPL / 2 : 1;
    static_assert(TPL == 1 || TPL % 2 == 0, "one target per lane, or float2 pairs");
    __shared__ float4 tile[2][kTile];
    if (a.stopped && *a.stopped) return;
    const ActiveLayout L = active_layout(a, D);
    if (L.n == 0u || (L.n >= a.long_list) != (TPL > 1)) return;   // the other build's list (workgroup-uniform, before any barrier)
    const unsigned tid = threadIdx.x;
    const unsigned tiles = a.pad / (unsigned)kTile;
    const unsigned nblk = (L.n + 256u * TPL - 1u) / (256u * TPL);
    const unsigned items = nblk * L.slices;                        // (list block, source slice) pairs, the slice running fastest
    const float* __restrict__ px = a.pos_all;
    const float* __restrict__ py = a.pos_all + a.pad;
    const float* __restrict__ pz = a.pos_all + 2 * (size_t)a.pad;
    const f2 bias = f2{a.eps2, a.eps2};

    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        const unsigned tb = item / L.slices, by = item - tb * L.slices;
        unsigned t0 = by * L.tps, t1 = t0 + L.tps;
        if (t1 > tiles) t1 = tiles;
        if (t0 > t1) t0 = t1;                                      // a slice beyond the last tile (the rounding of tps) adds nothing
        const unsigned slot0 = tb * (256u * TPL) + tid;            // this lane's q-th target is list slot slot0 + 256 q
        f2 ix[PAIRS], iy[PAIRS], iz[PAIRS];
        double ox[TPL], oy[TPL], oz[TPL];
#pragma unroll
        for (int q = 0; q < TPL; ++q) {
            const unsigned slot = slot0 + q * 256u;
            const unsigned i = a.list[slot < L.n ? slot : 0u];     // n > 0: slot 0 exists; what a lane past the end computes is not stored
            const float x = px[i], y = py[i], z = (D == 3) ? pz[i] : 0.f;
            if (q & 1) { ix[q >> 1].y = x; iy[q >> 1].y = y; iz[q >> 1].y = z; }
            else       { ix[q >> 1].x = x; iy[q >> 1].x = y; iz[q >> 1].x = z; }
            ox[q] = oy[q] = oz[q] = 0.0;
        }
        if (TPL == 1) { ix[0].y = ix[0].x; iy[0].y = iy[0].x; iz[0].y = iz[0].x; }

        float4 nxt = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t0 < t1) {
            const unsigned j = t0 * kTile + tid;
            nxt = make_float4(px[j], py[j], (D == 3) ? pz[j] : 0.f, a.mass_all[j]);
        }
        int buf = 0;
        for (unsigned t = t0; t < t1; ++t) {
            tile[buf][tid] = nxt;
            __syncthreads();
            if (t + 1 < t1) {
                const unsigned j = (t + 1) * kTile + tid;
                nxt = make_float4(px[j], py[j], (D == 3) ? pz[j] : 0.f, a.mass_all[j]);
            }
            const float4* __restrict__ cur = tile[buf];
            if constexpr (TPL == 1) {
                // scalar forms of the same operations in the same order: the low half of the packed build, bit for bit
                const float tx = ix[0].x, ty = iy[0].x, tz = iz[0].x;
                float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll 8
                for (int j = 0; j < kTile; ++j) {
                    const float4 s = cur[j];                       // the same address in every lane: one ds_read_b128 broadcast
                    const float dx = s.x - tx, dy = s.y - ty, dz = (D == 3) ? s.z - tz : 0.f;
                    float r2 = __builtin_fmaf(dx, dx, a.eps2);
                    r2 = __builtin_fmaf(dy, dy, r2);
                    if (D == 3) r2 = __builtin_fmaf(dz, dz, r2);
                    const float w = NEWTON ? __builtin_amdgcn_rsqf(r2) : __builtin_amdgcn_rcpf(r2);
                    float w2 = w * w;
                    if (NEWTON) w2 = w2 * w;
                    const float wt = s.w * w2;
                    ax = __builtin_fmaf(wt, dx, ax);
                    ay = __builtin_fmaf(wt, dy, ay);
                    if (D == 3) az = __builtin_fmaf(wt, dz, az);
                }
                ox[0] += (double)ax; oy[0] += (double)ay; oz[0] += (double)az;
            } else {
                f2 ax[PAIRS], ay[PAIRS], az[PAIRS];
#pragma unroll
                for (int q = 0; q < PAIRS; ++q) ax[q] = ay[q] = az[q] = f2{0.f, 0.f};
#pragma unroll 4
                for (int j = 0; j < kTile; ++j) {
                    const float4 s = cur[j];
                    f2 dx[PAIRS], dy[PAIRS], dz[PAIRS], r2[PAIRS], w[PAIRS];
                    // stage by stage, so that the PAIRS dependency chains interleave in program order
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) dx[q] = f2{s.x, s.x} - ix[q];
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) dy[q] = f2{s.y, s.y} - iy[q];
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) dz[q] = (D == 3) ? f2{s.z, s.z} - iz[q] : f2{0.f, 0.f};
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) r2[q] = __builtin_elementwise_fma(dx[q], dx[q], bias);
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) r2[q] = __builtin_elementwise_fma(dy[q], dy[q], r2[q]);
                    if (D == 3) {
#pragma unroll
                        for (int q = 0; q < PAIRS; ++q) r2[q] = __builtin_elementwise_fma(dz[q], dz[q], r2[q]);
                    }
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) {
                        w[q].x = NEWTON ? __builtin_amdgcn_rsqf(r2[q].x) : __builtin_amdgcn_rcpf(r2[q].x);
                        w[q].y = NEWTON ? __builtin_amdgcn_rsqf(r2[q].y) : __builtin_amdgcn_rcpf(r2[q].y);
                    }
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) r2[q] = w[q] * w[q];
                    if (NEWTON) {
#pragma unroll
                        for (int q = 0; q < PAIRS; ++q) r2[q] = r2[q] * w[q];
                    }
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) w[q] = f2{s.w, s.w} * r2[q];
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) ax[q] = __builtin_elementwise_fma(w[q], dx[q], ax[q]);
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) ay[q] = __builtin_elementwise_fma(w[q], dy[q], ay[q]);
                    if (D == 3) {
#pragma unroll
                        for (int q = 0; q < PAIRS; ++q) az[q] = __builtin_elementwise_fma(w[q], dz[q], az[q]);
                    }
                }
#pragma unroll
                for (int q = 0; q < PAIRS; ++q) {
                    ox[2 * q] += (double)ax[q].x; oy[2 * q] += (double)ay[q].x; oz[2 * q] += (double)az[q].x;
                    ox[2 * q + 1] += (double)ax[q].y; oy[2 * q + 1] += (double)ay[q].y; oz[2 * q + 1] += (double)az[q].y;
                }
            }
            buf ^= 1;
        }
        double* __restrict__ o = a.part + (size_t)by * D * L.stride;
#pragma unroll
        for (int q = 0; q < TPL; ++q) {
            const unsigned slot = slot0 + q * 256u;
            if (slot < L.n) {
                o[slot] = ox[q];
                o[(size_t)L.stride + slot] = oy[q];
                if (D == 3) o[2 * (size_t)L.stride + slot] = oz[q];
            }
        }
        __syncthreads();   // the next item reuses the tile buffers
    }
}

// sums[k][r] = the slices' sums of row r, component k, added in slice order (fp64).  One lane per (row, component): grid.y = k.
__global__ __launch_bounds__(256) void active_fold_kernel(ActiveArgs a) {
    if (a.stopped && *a.stopped) return;
    const ActiveLayout L = active_layout(a, a.dim);
    const unsigned r = blockIdx.x * 256u + threadIdx.x;
    if (r >= L.n) return;
    const unsigned k = blockIdx.y;
    const double* __restrict__ p = a.part + (size_t)k * L.stride + r;
    const size_t step = (size_t)a.dim * L.stride;
    double s = 0.0;
#pragma unroll 8
    for (unsigned j = 0; j < L.slices; ++j) s += p[(size_t)j * step];
    a.sums[(size_t)k * a.cap + r] = s;
}

// out[r][k] = -(G m[list[r]]) sums[k][r]: export_forces_kernel's arithmetic for the listed rows
__global__ __launch_bounds__(256) void active_export_kernel(ActiveArgs a, double G, const double* __restrict__ m64, double* __restrict__ out) {
    const unsigned listed = *a.count;
    const unsigned n = listed < a.cap ? listed : a.cap;
    const unsigned r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const double gm = G * m64[a.list[r]];
    for (int k = 0; k < a.dim; ++k) out[(size_t)r * a.dim + k] = -(gm * a.sums[(size_t)k * a.cap + r]);
}

template <int TPL>
void launch_build(const ActiveArgs& a, dim3 grid, hipStream_t stream) {
    if (a.dim == 2) {
        if (a.law) hipLaunchKernelGGL((active_accel_kernel<2, TPL, 1>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((active_accel_kernel<2, TPL, 0>), grid, dim3(256), 0, stream, a);
    } else {
        if (a.law) hipLaunchKernelGGL((active_accel_kernel<3, TPL, 1>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((active_accel_kernel<3, TPL, 0>), grid, dim3(256), 0, stream, a);
    }
}

}  // namespace

hipError_t launch_active_accel(const ActiveArgs& a, hipStream_t stream) {
    if (a.cap == 0u) return hipSuccess;
    // Each build's grid covers the items of the lists that can be its own -- the short one fewer than long_list targets, the long one up to
    // cap -- and no more than kActiveMaxGrid workgroups; the item loop walks the rest.
    constexpr unsigned long long kActiveMaxGrid = 4096;
    const unsigned long long short_most = a.long_list - 1u < a.cap ? a.long_list - 1u : a.cap;
    unsigned long long g1 = ((short_most + 255u) / 256u) * (unsigned long long)a.max_slices;
    g1 = g1 < 1u ? 1u : g1 > kActiveMaxGrid ? kActiveMaxGrid : g1;
    unsigned long long g8 = (((unsigned long long)a.cap + kActiveLongBlock - 1u) / kActiveLongBlock) * (unsigned long long)a.max_slices;
    g8 = g8 < 1u ? 1u : g8 > kActiveMaxGrid ? kActiveMaxGrid : g8;
    hipError_t e = hipSuccess;
    if (a.long_list > 1u) {       // a list can be a short one
        launch_build<1>(a, dim3((unsigned)g1), stream);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (a.long_list <= a.cap) {   // a list of this capacity can be a long one
        launch_build<8>(a, dim3((unsigned)g8), stream);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(active_fold_kernel, dim3((a.cap + 255u) / 256u, (unsigned)a.dim, 1), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_active_export(const ActiveArgs& a, double G, const double* m64, double* forces_out, hipStream_t stream) {
    if (a.cap == 0u) return hipSuccess;
    hipLaunchKernelGGL(active_export_kernel, dim3((a.cap + 255u) / 256u), dim3(256), 0, stream, a, G, m64, forces_out);
    return hipGetLastError();
}

}  // namespace nbx
