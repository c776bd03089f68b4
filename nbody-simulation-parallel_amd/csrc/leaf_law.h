// leaf_law.h -- the per-pair laws of the leaf sums (include/nbody_hip.h NBX_LAW_*), shared by the pair kernels
// (leaf_pair_kernel.hip) and the far-field pass (leaf_far_kernel.hip): thresholds and the weight of ONE pair with every special case.
#pragma once
#include "../../include/nbody_hip.h"
#include "nbx_internal.h"

namespace nbx_leaf {

// smallest fp32 thresholds that are >= the reference's fp64 ones, so (r2 < T_f32) == ((double)r2 < T) for fp32 r2
constexpr float kTreeSkipF = 0x1.12e0c0p-30f;   // 1.00000008e-9  (octree.cpp:119, bvh.cpp:167: dist_sq < 1e-9)
constexpr float kSmoothF = 0x1.b7cdfep-34f;     // 1.00000001e-10 (fmm_parlay.cpp:1010: dist_sq < 1e-10)
constexpr float kNormZeroF = 0x1.79ca12p-67f;   // 1.00000005e-20 (vector.h:93-97: |diff| < 1e-10 -> zero vector)
constexpr float kSameF = 1.0e-14f;              // largest fp32 <= 1e-14 (fmm_parlay.cpp:995-1000: |d_k| > 1e-14 -> distinct)
static_assert((double)kTreeSkipF >= 1e-9 && (double)kSmoothF >= 1e-10 && (double)kNormZeroF >= 1e-20 && (double)kSameF <= 1e-14,
              "fp32 thresholds must sit on the right side of the fp64 ones");
constexpr float kFar = 1.0e18f;                 // pad bodies: massless, r^2 ~ 1e36 is finite in fp32 and the weight underflows to 0
static_assert(kTreeSkipF < 9.0e-7f, "a target outside the close set (nbx_internal.h) has no non-zero r^2 below 9.5e-7: no law's special case can apply to it");

#ifdef __HIPCC__
// Weight of d = p_j - p_i in the law's sum for ONE pair, every special case included: m_j / r^4 for an ordinary pair.  `ri` receives
// the reciprocal the weight was made of, 1 / r^2, for the far field's second-order term (leaf_far_kernel.hip) -- or 0 where the law
// skips or softens the pair: the correction of that pair is then dropped (every factor of it carries ri).
// NBX_LAW_NEWTON (the only law that reads eps2 = epsilon^2 > 0): rho^2 = r^2 + eps2, weight m_j / rho^3, ri = 1 / rho^2; no special
// case exists -- d = 0 gives a finite weight times a zero vector.  rs m and rs rs are formed first: neither leaves fp32's range while
// m / eps^3 stays inside it (the plan checks that before it launches), and a massless pad at 1e18 gives 0 x 3e-37 = 0, never a NaN.
template <int D, int LAW>
__device__ __forceinline__ float leaf_weight_ri(float r2, float mj, float dx, float dy, float dz, float& ri, float eps2 = 0.0f) {
    if (LAW == NBX_LAW_NEWTON) {
        const float rs = __builtin_amdgcn_rsqf(r2 + eps2);
        ri = rs * rs;
        return ri * (rs * mj);
    } else if (LAW == NBX_LAW_BRUTE) {
        const float g = (r2 < nbx::kR2SkipF) ? __builtin_inff() : r2;           // methods.cpp:24
        ri = __builtin_amdgcn_rcpf(g);
        return mj * ri * ri;
    } else if (LAW == NBX_LAW_TREE_LEAF) {
        // "same position" (every |d_k| <= 1e-9) implies r2 <= 3e-18 < 1e-9: one test covers both skips
        const float g = (r2 < kTreeSkipF) ? __builtin_inff() : r2;
        ri = __builtin_amdgcn_rcpf(g);
        return mj * ri * ri;
    } else {
        if (r2 < kSmoothF) {   // rare: smoothed magnitude, unsmoothed direction (fmm_parlay.cpp:1010-1020, vector.h:93-97)
            const bool same = __builtin_fabsf(dx) <= kSameF && __builtin_fabsf(dy) <= kSameF && (D == 2 || __builtin_fabsf(dz) <= kSameF);
            const float r2s = r2 + 1.0e-10f;                                                   // epsilon^2, epsilon = 1e-5
            const float mag = mj * __builtin_amdgcn_rcpf(r2s) * __builtin_amdgcn_rsqf(r2s);    // m / (r2s * sqrt(r2s))
            const float inv = (r2 < kNormZeroF) ? 0.0f : __builtin_amdgcn_rsqf(r2);               // normalized(): 0 below 1e-10
            ri = 0.0f;
            return same ? 0.0f : mag * inv;
        }
        ri = __builtin_amdgcn_rcpf(r2);
        return mj * ri * ri;
    }
}

template <int D, int LAW>
__device__ __forceinline__ float leaf_weight(float r2, float mj, float dx, float dy, float dz, float eps2 = 0.0f) {
    float ri;
    return leaf_weight_ri<D, LAW>(r2, mj, dx, dy, dz, ri, eps2);
}
#endif

}  // namespace nbx_leaf
