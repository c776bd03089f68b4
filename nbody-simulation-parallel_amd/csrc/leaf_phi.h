// leaf_phi.h -- the potential of a leaf plan (include/nbody_hip.h nbx_leaf_plan_energy / _potentials): what the host
// (leaf_plan_api.hip) needs of the kernels of leaf_phi_kernel.hip, as leaf_near.h and leaf_far.h are for the force kernels.  Nothing
// here changes a layout: the passes walk the tables a plan already holds (leaf_plan.h, leaf_far.h).
#pragma once
#include <hip/hip_runtime.h>

#include "leaf_far.h"
#include "leaf_plan.h"

namespace nbx_phi {

constexpr uint32_t kNearMaxLanes = 32;     // lanes that share one target of the near pass (they split its source stream)
constexpr uint32_t kNearTilePairs = 128;   // source pairs a wave of the near pass stages in LDS at a time (4 KB)
constexpr uint32_t kNearOps = 64;          // copy runs it holds in LDS at a time (longer lists go in chunks)
constexpr unsigned kFlushTerms = 248;      // fp32 terms a lane sums between flushes into its fp64 sum

// Device arrays of a laid-out structure as the near pass reads them, and the slot-ordered potential it writes.
struct PhiDevice {
    const float4* xp = nullptr;                    // [pslots + 2] leaf-ordered source pairs
    uint32_t pslots = 0;
    const nbx_leaf::CopyOp* ops = nullptr;
    const nbx_leaf::LeafBlock* blocks = nullptr;   // [n_blocks]: each piece with count > 0 is one work item ...
    const nbx_leaf::PackSub* subs = nullptr;       // [n_subs]:   ... and so is each packed leaf
    uint32_t n_blocks = 0, n_subs = 0;
    double* phi = nullptr;                         // [pslots] -- WRITTEN: every slot of a work item's targets once; zeroed before by the caller
    float eps2 = 0.0f;                             // NBX_LAW_NEWTON only: the softening length squared
};

// sum_j m_j w(r_ij) over the leaf's copy runs for every target slot a work item owns (w without the reference laws' factor 1/2)
hipError_t enqueue_near_phi(const PhiDevice& d, int dim, int law, hipStream_t s);
// the far cells' terms at f.order, ADDED to phi[slot] behind the near pass (f.eps2: the softening length squared)
hipError_t enqueue_far_phi(const nbx_far::FarDevice& f, double* phi, int dim, int law, hipStream_t s);
// phi_body[i] = factor phi[body_slot[i]], 0 for a body in no leaf
hipError_t enqueue_phi_by_body(const double* phi, const uint32_t* body_slot, size_t n, double factor, double* phi_body, hipStream_t s);
// out[2][ceil(n / 256)]: per-workgroup sums of m_i |v_i|^2 and of m_i phi_body[i], wave order within a workgroup; the host adds them
// in index order
hipError_t enqueue_energy_partials(const double* phi_body, size_t n, int dim, unsigned pad, const double* v64, const double* m64, double* out,
                                   hipStream_t s);

}  // namespace nbx_phi
