// active_jerk_kernel.hip -- accelerations AND their time derivatives (jerks) on a device-resident list of targets
// (nbx_ctx_compute_accel_jerk_active; the evaluation of nbx_ctx_step_hermite_block), gfx950, fp32 pair arithmetic, D = 2 or 3,
// softened laws only.
//
// For the targets list[0 .. n), n read from device memory, against ALL `pad` entries of chunk 0:
//     A_r = sum_j m_j w d
//     J_r = sum_j m_j w [ dv - p (d.dv) / rho^2 d ]        d = p_j - p_r,  dv = v_j - v_r,  rho^2 = r^2 + eps^2,  w = rho^-p
// p = 4 for law 0, 3 for law 1: J is the exact time derivative of A along straight paths.  The pair arithmetic of A is
// active_kernel.hip's, operation for operation (fp32 d, eps^2 the bias of r^2, v_rcp_f32 / v_rsq_f32, the mass last); its 1/rho^2 --
// the reciprocal itself for law 0, the square of the reciprocal root for law 1 -- is reused for the jerk's second term.  A body and
// itself (d = dv = 0) and the pads (mass 0, at rest at the origin) give exact zeros: no compare.  A coincident pair with different
// velocities gives the finite term m dv / eps^p.
//
// Sources sit in LDS as two float4 per tile entry, {x, y, z, m} and {vx, vy, vz, 0}, each read back with one ds_read_b128 broadcast.
// Two builds, both queued, the list's length deciding on the device (as in active_kernel.hip):
//   TPL = 1  one target per lane, 256 per list block, up to 256 source slices;
//   TPL = 4  two float2 target pairs per lane, 1,024 per workgroup (kJerkLongBlock).  D = 2 fits four waves per SIMD; D = 3 spills
//            there (4 targets x 2 D fp64 sums are 48 VGPRs alone) and is bounded to three, as active_kernel.hip's long build is.  Eight
//            targets per lane spill in every instantiation: DESIGN.md section 3 has the figures.
// Work distribution, summation (fp32 over a tile, fp64 per (target, slice), the slices folded in order, no floating-point atomics)
// and the layout logic are active_kernel.hip's with 2 D planes per slice: planes 0 .. D-1 hold A, D .. 2D-1 hold J.
#include "nbx_internal.h"

namespace nbx {
namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

template <int D, int TPL, int NEWTON>
__global__ __launch_bounds__(256, TPL > 1 ? 3 : 4) void active_jerk_kernel(ActiveArgs a, const float* __restrict__ vel_all) {
    constexpr int PAIRS = TPL > 1 ? TPL / 2 : 1;
    constexpr float P = NEWTON ? -3.f : -4.f;                      // -p: the factor of (d.dv) / rho^2
    static_assert(TPL == 1 || TPL % 2 == 0, "one target per lane, or float2 pairs");
    __shared__ float4 tile[2][kTile];
    __shared__ float4 tilev[2][kTile];
    if (a.stopped && *a.stopped) return;
    const ActiveLayout L = active_layout(a, 2 * D);
    if (L.n == 0u || (L.n >= a.long_list) != (TPL > 1)) return;   // the other build's list (workgroup-uniform, before any barrier)
    const unsigned tid = threadIdx.x;
    const unsigned tiles = a.pad / (unsigned)kTile;
    const unsigned nblk = (L.n + 256u * TPL - 1u) / (256u * TPL);
    const unsigned items = nblk * L.slices;                        // (list block, source slice) pairs, the slice running fastest
    const float* __restrict__ px = a.pos_all;
    const float* __restrict__ py = a.pos_all + a.pad;
    const float* __restrict__ pz = a.pos_all + 2 * (size_t)a.pad;
    const float* __restrict__ vx = vel_all;
    const float* __restrict__ vy = vel_all + a.pad;
    const float* __restrict__ vz = vel_all + 2 * (size_t)a.pad;
    const f2 bias = f2{a.eps2, a.eps2};

    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        const unsigned tb = item / L.slices, by = item - tb * L.slices;
        unsigned t0 = by * L.tps, t1 = t0 + L.tps;
        if (t1 > tiles) t1 = tiles;
        if (t0 > t1) t0 = t1;                                      // a slice beyond the last tile (the rounding of tps) adds nothing
        const unsigned slot0 = tb * (256u * TPL) + tid;            // this lane's q-th target is list slot slot0 + 256 q
        f2 ix[PAIRS], iy[PAIRS], iz[PAIRS], iu[PAIRS], iv[PAIRS], iw[PAIRS];
        double oa[TPL][D], oj[TPL][D];
#pragma unroll
        for (int q = 0; q < TPL; ++q) {
            const unsigned slot = slot0 + q * 256u;
            const unsigned i = a.list[slot < L.n ? slot : 0u];     // n > 0: slot 0 exists; what a lane past the end computes is not stored
            const float x = px[i], y = py[i], z = (D == 3) ? pz[i] : 0.f;
            const float u = vx[i], v = vy[i], w = (D == 3) ? vz[i] : 0.f;
            if (q & 1) { ix[q >> 1].y = x; iy[q >> 1].y = y; iz[q >> 1].y = z; iu[q >> 1].y = u; iv[q >> 1].y = v; iw[q >> 1].y = w; }
            else       { ix[q >> 1].x = x; iy[q >> 1].x = y; iz[q >> 1].x = z; iu[q >> 1].x = u; iv[q >> 1].x = v; iw[q >> 1].x = w; }
#pragma unroll
            for (int k = 0; k < D; ++k) oa[q][k] = oj[q][k] = 0.0;
        }

        float4 nxt = make_float4(0.f, 0.f, 0.f, 0.f), nxtv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t0 < t1) {
            const unsigned j = t0 * kTile + tid;
            nxt = make_float4(px[j], py[j], (D == 3) ? pz[j] : 0.f, a.mass_all[j]);
            nxtv = make_float4(vx[j], vy[j], (D == 3) ? vz[j] : 0.f, 0.f);
        }
        int buf = 0;
        for (unsigned t = t0; t < t1; ++t) {
            tile[buf][tid] = nxt;
            tilev[buf][tid] = nxtv;
            __syncthreads();
            if (t + 1 < t1) {
                const unsigned j = (t + 1) * kTile + tid;
                nxt = make_float4(px[j], py[j], (D == 3) ? pz[j] : 0.f, a.mass_all[j]);
                nxtv = make_float4(vx[j], vy[j], (D == 3) ? vz[j] : 0.f, 0.f);
            }
            const float4* __restrict__ cur = tile[buf];
            const float4* __restrict__ curv = tilev[buf];
            if constexpr (TPL == 1) {
                // scalar forms of the same operations in the same order: the low half of the packed build, bit for bit
                const float tx = ix[0].x, ty = iy[0].x, tz = iz[0].x, tu = iu[0].x, tv = iv[0].x, tw = iw[0].x;
                float ax = 0.f, ay = 0.f, az = 0.f, jx = 0.f, jy = 0.f, jz = 0.f;
#pragma unroll 8
                for (int j = 0; j < kTile; ++j) {
                    const float4 s = cur[j];                       // the same address in every lane: one ds_read_b128 broadcast each
                    const float4 sv = curv[j];
                    const float dx = s.x - tx, dy = s.y - ty, dz = (D == 3) ? s.z - tz : 0.f;
                    const float du = sv.x - tu, dv = sv.y - tv, dw = (D == 3) ? sv.z - tw : 0.f;
                    float r2 = __builtin_fmaf(dx, dx, a.eps2);
                    r2 = __builtin_fmaf(dy, dy, r2);
                    if (D == 3) r2 = __builtin_fmaf(dz, dz, r2);
                    float rv = dx * du;
                    rv = __builtin_fmaf(dy, dv, rv);
                    if (D == 3) rv = __builtin_fmaf(dz, dw, rv);
                    const float w = NEWTON ? __builtin_amdgcn_rsqf(r2) : __builtin_amdgcn_rcpf(r2);
                    float w2 = w * w;                              // law 1: 1 / rho^2;  law 0: rho^-4
                    const float ir2 = NEWTON ? w2 : w;             // 1 / rho^2
                    if (NEWTON) w2 = w2 * w;
                    const float wt = s.w * w2;
                    const float c = (P * rv) * ir2;
                    ax = __builtin_fmaf(wt, dx, ax);
                    ay = __builtin_fmaf(wt, dy, ay);
                    if (D == 3) az = __builtin_fmaf(wt, dz, az);
                    jx = __builtin_fmaf(wt, __builtin_fmaf(c, dx, du), jx);
                    jy = __builtin_fmaf(wt, __builtin_fmaf(c, dy, dv), jy);
                    if (D == 3) jz = __builtin_fmaf(wt, __builtin_fmaf(c, dz, dw), jz);
                }
                oa[0][0] += (double)ax; oa[0][1] += (double)ay;
                oj[0][0] += (double)jx; oj[0][1] += (double)jy;
                if (D == 3) { oa[0][D - 1] += (double)az; oj[0][D - 1] += (double)jz; }
            } else {
                f2 ax[PAIRS], ay[PAIRS], az[PAIRS], jx[PAIRS], jy[PAIRS], jz[PAIRS];
#pragma unroll
                for (int q = 0; q < PAIRS; ++q) ax[q] = ay[q] = az[q] = jx[q] = jy[q] = jz[q] = f2{0.f, 0.f};
#pragma unroll 4
                for (int j = 0; j < kTile; ++j) {
                    const float4 s = cur[j];
                    const float4 sv = curv[j];
                    f2 dx[PAIRS], dy[PAIRS], dz[PAIRS], du[PAIRS], dv[PAIRS], dw[PAIRS], r2[PAIRS], rv[PAIRS], w[PAIRS], ir2[PAIRS];
                    // stage by stage, so that the PAIRS dependency chains interleave in program order
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) {
                        dx[q] = f2{s.x, s.x} - ix[q];
                        dy[q] = f2{s.y, s.y} - iy[q];
                        dz[q] = (D == 3) ? f2{s.z, s.z} - iz[q] : f2{0.f, 0.f};
                    }
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) {
                        du[q] = f2{sv.x, sv.x} - iu[q];
                        dv[q] = f2{sv.y, sv.y} - iv[q];
                        dw[q] = (D == 3) ? f2{sv.z, sv.z} - iw[q] : f2{0.f, 0.f};
                    }
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) { r2[q] = __builtin_elementwise_fma(dx[q], dx[q], bias); rv[q] = dx[q] * du[q]; }
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) {
                        r2[q] = __builtin_elementwise_fma(dy[q], dy[q], r2[q]);
                        rv[q] = __builtin_elementwise_fma(dy[q], dv[q], rv[q]);
                    }
                    if (D == 3) {
#pragma unroll
                        for (int q = 0; q < PAIRS; ++q) {
                            r2[q] = __builtin_elementwise_fma(dz[q], dz[q], r2[q]);
                            rv[q] = __builtin_elementwise_fma(dz[q], dw[q], rv[q]);
                        }
                    }
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) {
                        w[q].x = NEWTON ? __builtin_amdgcn_rsqf(r2[q].x) : __builtin_amdgcn_rcpf(r2[q].x);
                        w[q].y = NEWTON ? __builtin_amdgcn_rsqf(r2[q].y) : __builtin_amdgcn_rcpf(r2[q].y);
                    }
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) { r2[q] = w[q] * w[q]; ir2[q] = NEWTON ? r2[q] : w[q]; }
                    if (NEWTON) {
#pragma unroll
                        for (int q = 0; q < PAIRS; ++q) r2[q] = r2[q] * w[q];
                    }
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) { w[q] = f2{s.w, s.w} * r2[q]; rv[q] = (f2{P, P} * rv[q]) * ir2[q]; }
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) {
                        ax[q] = __builtin_elementwise_fma(w[q], dx[q], ax[q]);
                        ay[q] = __builtin_elementwise_fma(w[q], dy[q], ay[q]);
                        if (D == 3) az[q] = __builtin_elementwise_fma(w[q], dz[q], az[q]);
                    }
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) {
                        jx[q] = __builtin_elementwise_fma(w[q], __builtin_elementwise_fma(rv[q], dx[q], du[q]), jx[q]);
                        jy[q] = __builtin_elementwise_fma(w[q], __builtin_elementwise_fma(rv[q], dy[q], dv[q]), jy[q]);
                        if (D == 3) jz[q] = __builtin_elementwise_fma(w[q], __builtin_elementwise_fma(rv[q], dz[q], dw[q]), jz[q]);
                    }
                }
#pragma unroll
                for (int q = 0; q < PAIRS; ++q) {
                    oa[2 * q][0] += (double)ax[q].x; oa[2 * q][1] += (double)ay[q].x;
                    oj[2 * q][0] += (double)jx[q].x; oj[2 * q][1] += (double)jy[q].x;
                    oa[2 * q + 1][0] += (double)ax[q].y; oa[2 * q + 1][1] += (double)ay[q].y;
                    oj[2 * q + 1][0] += (double)jx[q].y; oj[2 * q + 1][1] += (double)jy[q].y;
                    if (D == 3) {
                        oa[2 * q][D - 1] += (double)az[q].x; oj[2 * q][D - 1] += (double)jz[q].x;
                        oa[2 * q + 1][D - 1] += (double)az[q].y; oj[2 * q + 1][D - 1] += (double)jz[q].y;
                    }
                }
            }
            buf ^= 1;
        }
        double* __restrict__ o = a.part + (size_t)by * (2 * D) * L.stride;
#pragma unroll
        for (int q = 0; q < TPL; ++q) {
            const unsigned slot = slot0 + q * 256u;
            if (slot < L.n) {
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    o[(size_t)k * L.stride + slot] = oa[q][k];
                    o[(size_t)(D + k) * L.stride + slot] = oj[q][k];
                }
            }
        }
        __syncthreads();   // the next item reuses the tile buffers
    }
}

// sums[k][r] = the slices' sums of row r, plane k (A then J), added in slice order (fp64).  One lane per (row, plane): grid.y = k.
__global__ __launch_bounds__(256) void active_jerk_fold_kernel(ActiveArgs a) {
    if (a.stopped && *a.stopped) return;
    const unsigned planes = 2u * (unsigned)a.dim;
    const ActiveLayout L = active_layout(a, (int)planes);
    const unsigned r = blockIdx.x * 256u + threadIdx.x;
    if (r >= L.n) return;
    const unsigned k = blockIdx.y;
    const double* __restrict__ p = a.part + (size_t)k * L.stride + r;
    const size_t step = (size_t)planes * L.stride;
    double s = 0.0;
#pragma unroll 8
    for (unsigned j = 0; j < L.slices; ++j) s += p[(size_t)j * step];
    a.sums[(size_t)k * a.cap + r] = s;
}

// accel_out[r][k] = -(G sums[k][r]), jerk_out[r][k] = -(G sums[D + k][r]): the scaling of the context's kick without the mass
__global__ __launch_bounds__(256) void active_jerk_export_kernel(ActiveArgs a, double G, double* __restrict__ accel_out,
                                                                 double* __restrict__ jerk_out) {
    const unsigned listed = *a.count;
    const unsigned n = listed < a.cap ? listed : a.cap;
    const unsigned r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    for (int k = 0; k < a.dim; ++k) {
        if (accel_out) accel_out[(size_t)r * a.dim + k] = -(G * a.sums[(size_t)k * a.cap + r]);
        if (jerk_out) jerk_out[(size_t)r * a.dim + k] = -(G * a.sums[(size_t)(a.dim + k) * a.cap + r]);
    }
}

template <int TPL>
void launch_build(const ActiveArgs& a, const float* vel_all, dim3 grid, hipStream_t stream) {
    if (a.dim == 2) {
        if (a.law) hipLaunchKernelGGL((active_jerk_kernel<2, TPL, 1>), grid, dim3(256), 0, stream, a, vel_all);
        else hipLaunchKernelGGL((active_jerk_kernel<2, TPL, 0>), grid, dim3(256), 0, stream, a, vel_all);
    } else {
        if (a.law) hipLaunchKernelGGL((active_jerk_kernel<3, TPL, 1>), grid, dim3(256), 0, stream, a, vel_all);
        else hipLaunchKernelGGL((active_jerk_kernel<3, TPL, 0>), grid, dim3(256), 0, stream, a, vel_all);
    }
}

}  // namespace

hipError_t launch_active_accel_jerk(const ActiveArgs& a, const float* vel_all, hipStream_t stream) {
    if (a.cap == 0u) return hipSuccess;
    // the grids of launch_active_accel, with this kernel's list block
    constexpr unsigned long long kActiveMaxGrid = 4096;
    const unsigned long long short_most = a.long_list - 1u < a.cap ? a.long_list - 1u : a.cap;
    unsigned long long g1 = ((short_most + 255u) / 256u) * (unsigned long long)a.max_slices;
    g1 = g1 < 1u ? 1u : g1 > kActiveMaxGrid ? kActiveMaxGrid : g1;
    unsigned long long g4 = (((unsigned long long)a.cap + kJerkLongBlock - 1u) / kJerkLongBlock) * (unsigned long long)a.max_slices;
    g4 = g4 < 1u ? 1u : g4 > kActiveMaxGrid ? kActiveMaxGrid : g4;
    hipError_t e = hipSuccess;
    if (a.long_list > 1u) {       // a list can be a short one
        launch_build<1>(a, vel_all, dim3((unsigned)g1), stream);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (a.long_list <= a.cap) {   // a list of this capacity can be a long one
        launch_build<kJerkLongBlock / 256>(a, vel_all, dim3((unsigned)g4), stream);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(active_jerk_fold_kernel, dim3((a.cap + 255u) / 256u, 2u * (unsigned)a.dim, 1), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_active_jerk_export(const ActiveArgs& a, double G, double* accel_out, double* jerk_out, hipStream_t stream) {
    if (a.cap == 0u) return hipSuccess;
    hipLaunchKernelGGL(active_jerk_export_kernel, dim3((a.cap + 255u) / 256u), dim3(256), 0, stream, a, G, accel_out, jerk_out);
    return hipGetLastError();
}

}  // namespace nbx
