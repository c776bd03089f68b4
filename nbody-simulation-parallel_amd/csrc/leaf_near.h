// leaf_near.h -- the near field of a leaf plan: what the host (leaf_plan_api.hip) needs of the kernels of leaf_pair_kernel.hip, as
// leaf_far.h is for leaf_far_kernel.hip.  The layout the kernels follow is leaf_plan.h's; the comment at the top of
// leaf_pair_kernel.hip says what each piece is for.
#pragma once
#include <hip/hip_runtime.h>

#include "leaf_plan.h"

namespace nbx_near {

// Device arrays of a laid-out structure and what the pair kernels read and write.
struct NearDevice {
    const float4* xp = nullptr;                 // [pslots + 2] leaf-ordered source pairs, the launch's pad pair behind them
    uint32_t pslots = 0;
    const nbx_leaf::CopyOp* ops = nullptr;
    const nbx_leaf::LeafBlock* blocks = nullptr;   // [n_blocks] one-leaf workgroups of `waves` wave64
    const nbx_leaf::PackBlock* packs = nullptr;    // [n_packs] packed waves ...
    const nbx_leaf::PackSub* subs = nullptr;       // ... and their leaves
    size_t n_blocks = 0, n_packs = 0;
    int waves = 2;
    double* sums = nullptr;                     // [dim][pslots] -- WRITTEN: every slot of a workgroup's targets once
    const uint32_t* max_mass = nullptr;         // the word the gather left
    float eps2 = 0.0f;                          // NBX_LAW_NEWTON only: the softening length squared
};

// The pair kernels, one-leaf workgroups first (they are the long ones).  `fuse`: a structure with both kinds of workgroups and
// one-wave workgroups runs them in ONE launch.
hipError_t enqueue_near(const NearDevice& d, int dim, int law, hipStream_t s, bool fuse);

// staged Body<D> records (fp64, host order, `stride_d` doubles apart) -> source pairs; the call's largest |mass| into *max_mass
hipError_t enqueue_gather_staged(const double* raw, size_t stride_d, int dim, const uint32_t* pslot_body, size_t pslots, float4* xp, uint32_t* max_mass,
                                 hipStream_t s);
// a context's resident fp32 copy (pos[dim][pad], mass[pad]) -> source pairs, one lane per body; pad slots are not touched
hipError_t enqueue_gather_resident(const float* pos, const float* mass, unsigned pad, int dim, const uint32_t* body_slot, size_t n, float4* xp,
                                   uint32_t* max_mass, hipStream_t s);
// the pads of odd leaves and the launch's pad pair: massless and far away
hipError_t enqueue_init_pads(const uint32_t* pslot_body, size_t pslots, int dim, float4* xp, hipStream_t s);
// forces[body] = signedG m_body sums[slot]: by slot (bodies in no leaf are not written), masses from the staged records ...
hipError_t enqueue_scatter(const double* sums, const double* raw, size_t stride_d, int dim, const uint32_t* pslot_body, size_t pslots, double signedG,
                           double* forces, hipStream_t s);
// ... or by body (every entry written: zero for a body in no leaf), masses from mass[body * mass_stride]
hipError_t enqueue_forces_by_body(const double* sums, size_t pslots, const uint32_t* body_slot, size_t n, int dim, double signedG, const double* mass,
                                  size_t mass_stride, double* forces, hipStream_t s);

}  // namespace nbx_near
