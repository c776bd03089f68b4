// leaf_plan_api.hip -- the host side of the leaf-pair path behind the C ABI (include/nbody_hip.h): the one-shot call
// nbx_leaf_pair_forces and the device-resident plan nbx_leaf_plan_*.  Validation, the choice of planner (leaf_plan.h on the host,
// leaf_plan_device.h on the device), the octree built on the device (octree_device.h), and every entry point.  Every kick of
// a plan is launch_kick_drift_slots (plan_kick, plan_enqueue_eval) and every fixed-step loop is plan_run_steps; the loop whose steps
// are chosen on the device is plan_run_adaptive, with its kick read from the step clock.  The kernels are
// leaf_pair_kernel.hip's (through leaf_near.h), leaf_far_kernel.hip's (leaf_far.h) and, for the potential, leaf_phi_kernel.hip's
// (leaf_phi.h); device memory is device_block.h's.
#include "../../include/nbody_hip.h"
#include "nbx_ctx.h"
#include "device_block.h"
#include "leaf_plan.h"
#include "leaf_near.h"
#include "leaf_far.h"
#include "leaf_phi.h"
#include "leaf_plan_device.h"
#include "octree_device.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <thread>
#include <utility>
#include <vector>

using namespace nbx;
using namespace nbx_leaf;
using nbx_block::Block;
using nbx_block::carve;
using nbx_block::leaf_pool;

#ifndef NBX_LEAF_PACK
#define NBX_LEAF_PACK 1   /* 0: A/B build without packed small leaves (make LEAF_DEFS=-DNBX_LEAF_PACK=0 ...) */
#endif

namespace {

constexpr size_t kHelperCopyBytes = (size_t)4 << 20;   // staged bodies from this size on are copied by a helper thread while the launch is laid out

// The one-shot call's device arrays are two blocks from the parked pool (device_block.h): a tree code calls once per step with arrays
// of the same size, and so allocates nothing.
struct DeviceBuffers {   // gives back whatever the call took when it leaves, on every path
    Block arena;                    // everything but the staged bodies
    Block body_arena;               // the staged Body<D> array
    hipStream_t stream = nullptr;
    int device = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ~DeviceBuffers() {
        const bool idle = stream && hipStreamSynchronize(stream) == hipSuccess;
        arena.release(idle);
        body_arena.release(idle);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (idle) nbx::park_stream(device, stream);   // back to the pool (nbx_api.hip): a stream costs more than this call's kernels
        else if (stream) (void)hipStreamDestroy(stream);
    }
};

}  // namespace

// ---- device-resident plan (include/nbody_hip.h "device-resident leaf plan") ---------------------------------------------------
// What a tree code keeps between force evaluations while its tree stands: the validated structure laid out for the kernel
// (leaf_plan.h) and every device buffer an evaluation needs.  An evaluation is then: gather (16 B per slot from the resident
// fp32 source copy), pair kernel, and -- only if the caller wants them on the host -- forces by body and one copy out.
struct nbx_leaf_plan {
    int device = 0, dim = 3, waves = 2;
    size_t n = 0, pslots = 0, n_ops = 0, n_blocks = 0, n_subs = 0, n_packs = 0;
    Block arena;                    // xp | sums | pslot_body | body_slot | ops | blocks | max_mass | packed leaves | packed waves
    float4* xp = nullptr;
    double* sums = nullptr;         // [dim][pslots]
    uint32_t* pslot_body = nullptr; // [pslots]
    uint32_t* body_slot = nullptr;  // [n]  inverse map, 0xffffffff for a body in no leaf
    CopyOp* ops = nullptr;
    LeafBlock* blocks = nullptr;
    uint32_t* max_mass = nullptr;
    PackSub* subs = nullptr;
    PackBlock* packs = nullptr;
    double* forces = nullptr;       // [n][dim]: a piece of the arena (the one-shot call's plan), or forces_own ...
    Block forces_own;               // ... allocated when a caller first asks for forces on the host
    Block raw;                      // staged Body<D> array of nbx_leaf_plan_forces (+ 256 bytes): allocated on first use, or (one-shot call) from the pool
    hipStream_t stream = nullptr;   // own stream (host-bodies path)
    hipStream_t last_stream = nullptr;   // stream the last evaluation was ordered on
    hipEvent_t ev0 = nullptr, ev1 = nullptr, done = nullptr;
    bool evaluated = false;
    int last_law = NBX_LAW_TREE_LEAF;
    double last_signedG = 0.0;
    // masses of the last evaluation: a context's m64 (stride 1) or the staged bodies (offset 2 dim, stride the body's)
    const double* last_mass = nullptr;
    size_t last_mass_stride = 1;
    unsigned long long last_ctx_id = 0;   // the context whose m64 last_mass points into (0: the plan's own staged bodies)
    bool device_planned = false;    // laid out on the device (leaf_plan_device.h); false: on the host (leaf_plan.h)
    nbx_leaf_dev::Summary summary_host;   // the device planner's 64 bytes land here
    // ---- the far field (nbx_leaf_plan_set_cells; leaf_far.h): cells, far lists and the moments of the last evaluation ----
    size_t n_leaves = 0;
    uint32_t* unit_off = nullptr;   // [n_leaves + 1] first padded slot of every leaf (in the arena; either planner leaves it there)
    std::vector<uint32_t> unit_host;   // the host planner's copy of it (empty after the device planner: set_cells then reads it back)
    nbx_far::FarDevice far;         // n_cells = 0: no far field, and nothing below is touched by an evaluation
    size_t far_entries = 0;
    Block cell_arena;               // every array `far` names that is the cells' own
    hipEvent_t evm0 = nullptr, evm1 = nullptr, evf0 = nullptr, evf1 = nullptr;   // moment pass, far pass (created with the first cells)
    // an evaluation has run since the cells were set: only then do cell_rec / cell_mass hold moments.  plan_release_cells (every
    // set_cells, destroy) clears it; nbx_leaf_plan_get_cells and the far pass of nbx_leaf_plan_time_kernel rely on that.
    bool cells_evaluated = false;
    bool cells_timed = false;       // ... and it recorded the four events
    // ---- the far field's order (nbx_leaf_plan_set_far_order): the plan's own, it outlives cells and rebuilds ----
    int far_order = NBX_FAR_MONOPOLE;
    // ---- NBX_LAW_NEWTON's softening length (nbx_leaf_plan_set_softening): the plan's own like the order; no other law reads it ----
    double softening = 0.0;
    bool quads_evaluated = false;   // the last evaluation with these cells ran at order 1: cell_quad holds its second moments
    Block quad_arena;               // leaf_quad, cell_quad, cell_qrec of the cells as they stand; never allocated at order 0
    // ---- a structure built on the device (nbx_leaf_plan_create_octree; octree_device.h) ----
    bool octree = false;            // made by nbx_leaf_plan_create_octree
    bool octree_built = false;      // ... and its last build went through (a refused rebuild leaves nothing to evaluate)
    int octree_depth = 0;
    double octree_theta = 0.0;
    size_t octree_capacity = 0;     // > 0: the adaptive tree (nbx_leaf_plan_create_octree_adaptive), octree_depth its max_depth
    Block tree_arena;               // the builder's block: the tree, six of the eight structure arrays, scratch
    nbx_octree::TreeLayout tree_layout{};
    nbx_octree::Tree tree;
    nbx_octree::Counts counts_host{};     // the builder's 64 bytes land here
    const uint32_t* list_sources_dev = nullptr;   // in the arena
    // ---- the potential (nbx_leaf_plan_energy / _potentials; leaf_phi.h): nothing below exists until a caller first asks for one ----
    Block phi_block;                // phi by slot | phi by body | the reduction's partials; fitted by every potential call
    double* phi_slot = nullptr;     // [pslots] per unit G m_i, without the reference laws' factor 1/2
    double* phi_body = nullptr;     // [n] what nbx_leaf_plan_get_potentials hands out
    double* phi_part = nullptr;     // [2][ceil(n / 256)]
    bool phi_valid = false;         // a potential call has gone through
    Block phi_raw;                  // staged Body<D> array of nbx_leaf_plan_potentials -- not `raw`: the masses of the last force evaluation may live there
    // ---- the largest acceleration (nbx_leaf_plan_max_accel): the reduction's 8-byte word, allocated when a caller first asks ----
    Block amax_block;
    // ---- the step clock (nbx_leaf_plan_step_kdk_adaptive; nbx_internal.h: StepClock): allocated by the first adaptive call ----
    Block clock_block;              // the clock and, kStepClockHistoryOffset behind it, the history of the last call
    bool clock_valid = false;       // an adaptive call has gone through: the block holds its clock
    int* stop_look = nullptr;       // pinned host word the loop's looks at the clock's `stopped` land in
    hipEvent_t look_done = nullptr; // ... and the event behind the look in flight
};

namespace {
// The part of the validation that stays on the host whichever planner runs: the two offset arrays (n_leaves + 1 words each; the
// lengths of every copy come from them).
int validate_offsets(size_t n, const uint32_t* leaf_offsets, const uint32_t* leaf_bodies, size_t n_leaves, const uint32_t* list_offsets,
                     const uint32_t* list_sources, size_t* slots_out, size_t* n_list_out) {
    if (n > ((size_t)1 << 31) || n_leaves > ((size_t)1 << 31)) return fail(NBX_ERR_INVALID, "too many bodies / leaves");
    if (n_leaves && (!leaf_offsets || !list_offsets)) return fail(NBX_ERR_INVALID, "null leaf arrays");
    const size_t slots = n_leaves ? leaf_offsets[n_leaves] : 0;
    const size_t n_list = n_leaves ? list_offsets[n_leaves] : 0;
    if (n_leaves && (leaf_offsets[0] != 0 || list_offsets[0] != 0)) return fail(NBX_ERR_INVALID, "CSR offsets must start at 0");
    uint32_t bad = 0;                                    // no exit inside the loop: vectorised
    for (size_t l = 0; l < n_leaves; ++l) bad |= (uint32_t)(leaf_offsets[l + 1] < leaf_offsets[l]) | (uint32_t)(list_offsets[l + 1] < list_offsets[l]);
    if (bad) return fail(NBX_ERR_INVALID, "CSR offsets must be non-decreasing");
    if ((slots && !leaf_bodies) || (n_list && !list_sources)) return fail(NBX_ERR_INVALID, "null leaf arrays");
    *slots_out = slots;
    *n_list_out = n_list;
    return NBX_OK;
}

// Which planner lays a structure out.  NBODY_HIP_LEAF_PLANNER=host|device in the environment decides for every call (tests run
// every case through both); otherwise the device takes structures from kDevicePlanFrom slots + list entries on -- below that the
// host's few microseconds beat the device planner's ~35 launches.
constexpr size_t kDevicePlanFrom = 65536;
bool use_device_planner(size_t n_leaves, size_t slots, size_t n_list) {
    if (n_leaves == 0 || slots == 0) return false;                                  // nothing to lay out: the host path's early exits
    if (slots + n_leaves > 0xfffffff0ull || n_list > 0xfffffff0ull) return false;     // the host planner words the refusal
    if (kPackWindowWaves * (size_t)kPackMaxSubs > 128) return false;                  // A/B builds with larger windows
    if (const char* e = std::getenv("NBODY_HIP_LEAF_PLANNER")) {
        if (!std::strcmp(e, "host")) return false;
        if (!std::strcmp(e, "device")) return true;
    }
    return slots + n_list >= kDevicePlanFrom;
}

// The rest of the host-side validation, behind validate_offsets: every index the kernels will follow, before anything is launched.
int validate_csr(size_t n, const uint32_t* leaf_bodies, size_t n_leaves, const uint32_t* list_sources, size_t slots, size_t n_list) {
    {
        std::vector<unsigned char> seen;
        try { seen.assign(n, 0); } catch (...) { return fail(NBX_ERR_ALLOC, "host allocation failed"); }
        for (size_t s = 0; s < slots; ++s) {
            const uint32_t b = leaf_bodies[s];
            if (b >= n) return fail(NBX_ERR_INVALID, "leaf_bodies entry out of range");
            if (seen[b]) return fail(NBX_ERR_INVALID, "a body may belong to at most one leaf");
            seen[b] = 1;
        }
    }
    {   // the largest entry, without an exit inside the loop (so that it is vectorised: 6.7 million entries for 65,536 BVH leaves)
        uint32_t largest = 0;
        for (size_t e = 0; e < n_list; ++e) largest = list_sources[e] > largest ? list_sources[e] : largest;
        if (n_list && largest >= n_leaves) return fail(NBX_ERR_INVALID, "list_sources entry out of range");
    }
    return NBX_OK;
}

// plan_leaves behind the C ABI: no exception leaves it (its arrays are std::vectors), an allocation failure is NBX_ERR_ALLOC
int lay_out_launch(const uint32_t* leaf_offsets, const uint32_t* leaf_bodies, size_t n_leaves, const uint32_t* list_offsets, const uint32_t* list_sources,
                   LeafPlan& plan) {
    const char* why = nullptr;
    try {
        why = plan_leaves(leaf_offsets, leaf_bodies, n_leaves, list_offsets, list_sources, plan, NBX_LEAF_PACK != 0);
    } catch (...) {
        why = kPlanAllocFailed;
    }
    if (!why) return NBX_OK;
    return fail(why == kPlanAllocFailed ? NBX_ERR_ALLOC : NBX_ERR_INVALID, why);
}

int create_plan(nbx_leaf_plan** out, int device, int dim, size_t n, const uint32_t* leaf_offsets, const uint32_t* leaf_bodies, size_t n_leaves,
                const uint32_t* list_offsets, const uint32_t* list_sources, size_t forces_bytes);

// The caller's current HIP device is put back when an entry point of this file returns
struct DeviceScope {
    int before = -1;
    DeviceScope() { if (hipGetDevice(&before) != hipSuccess) before = -1; (void)hipGetLastError(); }
    ~DeviceScope() { if (before >= 0) (void)hipSetDevice(before); }
};

// a plan in the making, or the one-shot call's: destroyed on every way out that does not hand it over
struct PlanDestroyer { void operator()(nbx_leaf_plan* p) const { nbx_leaf_plan_destroy(p); } };
using PlanHolder = std::unique_ptr<nbx_leaf_plan, PlanDestroyer>;

// brute force: forces[i] -= f (methods.cpp:131); tree codes: += (attractive)
double signed_G(int law, double G) { return law == NBX_LAW_BRUTE ? -G : G; }
}  // namespace

extern "C" int nbx_leaf_pair_forces(const void* bodies, size_t n, int dim, size_t stride_bytes, const uint32_t* leaf_offsets,
                                    const uint32_t* leaf_bodies, size_t n_leaves, const uint32_t* list_offsets,
                                    const uint32_t* list_sources, int law, double G, int device, double* forces_out,
                                    float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    if (dim != 2 && dim != 3) return fail(NBX_ERR_INVALID, "dim must be 2 or 3");
    if (law < NBX_LAW_BRUTE || law > NBX_LAW_FMM_P2P) return fail(NBX_ERR_INVALID, law == NBX_LAW_NEWTON ? "NBX_LAW_NEWTON needs a plan (nbx_leaf_plan_set_softening): the one-shot call has no softening length" : "unknown law");
    if ((!bodies || !forces_out) && n) return fail(NBX_ERR_INVALID, "null argument");
    const size_t min_stride = (size_t)(2 * dim + 1) * sizeof(double);
    if (stride_bytes < min_stride || stride_bytes % sizeof(double) != 0)
        return fail(NBX_ERR_INVALID, "body stride must be a multiple of 8 and >= sizeof(Body<dim>)");
    size_t slots = 0, n_list = 0;
    if (int vrc = validate_offsets(n, leaf_offsets, leaf_bodies, n_leaves, list_offsets, list_sources, &slots, &n_list)) return vrc;
    if (use_device_planner(n_leaves, slots, n_list)) {
        // the structure laid out on the device (leaf_plan_device.h): a plan for this call alone, its block and the staged bodies' from the
        // parked pool, so that a tree code calling once per step allocates nothing
        nbx_leaf_plan* p = nullptr;
        if (int prc = create_plan(&p, device, dim, n, leaf_offsets, leaf_bodies, n_leaves, list_offsets, list_sources, n * (size_t)dim * sizeof(double))) return prc;
        PlanHolder hold(p);
        DeviceScope scope;
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = nbx_block::take(p->raw, leaf_pool(), device, n * stride_bytes + 256);
        if (e != hipSuccess) return nbx::fail_hip(e, "staging the bodies", __FILE__, __LINE__);
        return nbx_leaf_plan_forces(p, bodies, stride_bytes, law, G, forces_out, kernel_ms);
    }
    if (int vrc = validate_csr(n, leaf_bodies, n_leaves, list_sources, slots, n_list)) return vrc;
    int ndev = 0;
    int rc = nbx_device_count(&ndev);
    if (rc != NBX_OK) return rc;
    if (device < 0 || device >= ndev) return fail(NBX_ERR_NO_DEVICE, "device ordinal out of range");
    if (slots == 0) {   // no leaf holds a body: every force is zero (otherwise the device array, zeroed there, is copied out whole)
        for (size_t i = 0; i < n * (size_t)dim; ++i) forces_out[i] = 0.0;
        return NBX_OK;
    }

    DeviceScope scope;   // the caller's current device is restored on every path
    NBX_HIP_TRY(hipSetDevice(device));
    DeviceBuffers d;
    d.device = device;
    NBX_HIP_TRY(nbx::take_stream(device, &d.stream));
    NBX_HIP_TRY(hipEventCreate(&d.ev0));
    NBX_HIP_TRY(hipEventCreate(&d.ev1));
    // The bodies go to the device on a helper thread (58 MB at N = 2^20; the copy from pageable memory blocks its caller for 1 ms)
    // while this thread lays out the launch.
    NBX_HIP_TRY(nbx_block::take(d.body_arena, leaf_pool(), device, n * stride_bytes + 256));
    double* const raw = d.body_arena.as<double>();
    hipError_t copy_rc = hipSuccess;
    std::thread copier;
    struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{copier};   // before d goes, on every path
    if (n * stride_bytes >= kHelperCopyBytes) {
        try {
            copier = std::thread([&]() {
                copy_rc = hipSetDevice(device);
                if (copy_rc == hipSuccess) copy_rc = hipMemcpyAsync(raw, bodies, n * stride_bytes, hipMemcpyHostToDevice, d.stream);
            });
        } catch (...) {   // no thread to be had: copy here
        }
    }
    if (!copier.joinable())   // small input (a thread costs more than the copy takes), or no thread
        NBX_HIP_TRY(hipMemcpyAsync(raw, bodies, n * stride_bytes, hipMemcpyHostToDevice, d.stream));

    // ---- the layout the kernel follows (leaf_plan.h; comment at the top of this file) ----
    static thread_local LeafPlan plan;   // a tree code calls once per step: the arrays keep their capacity (and their pages) between calls
    if (int prc = lay_out_launch(leaf_offsets, leaf_bodies, n_leaves, list_offsets, list_sources, plan)) return prc;
    const size_t pslots = plan.pslots();
    const std::vector<CopyOp>& ops = plan.ops;
    const std::vector<LeafBlock>& blocks = plan.blocks;

    // one allocation for the call's other device arrays (each hipFree of a large buffer costs 0.2 ms on this runtime)
    const size_t sizes[9] = {pslots * sizeof(float4), (size_t)dim * pslots * sizeof(double), n * (size_t)dim * sizeof(double),
                             pslots * sizeof(uint32_t), ops.size() * sizeof(CopyOp), blocks.size() * sizeof(LeafBlock), sizeof(uint32_t),
                             plan.pack_subs.size() * sizeof(PackSub), plan.pack_blocks.size() * sizeof(PackBlock)};
    const auto cut = carve(sizes);
    NBX_HIP_TRY(nbx_block::take(d.arena, leaf_pool(), device, cut.total));
    char* const arena = d.arena.get();
    float4* xp = cut.at<float4>(arena, 0);
    double* acc = cut.at<double>(arena, 1);
    double* dforces = cut.at<double>(arena, 2);
    uint32_t* d_pb = cut.at<uint32_t>(arena, 3);
    CopyOp* d_ops = cut.at<CopyOp>(arena, 4);
    LeafBlock* d_blocks = cut.at<LeafBlock>(arena, 5);
    uint32_t* d_max_mass = cut.at<uint32_t>(arena, 6);
    PackSub* d_subs = cut.at<PackSub>(arena, 7);
    PackBlock* d_packs = cut.at<PackBlock>(arena, 8);
    if (copier.joinable()) copier.join();
    NBX_HIP_TRY(copy_rc);
    NBX_HIP_TRY(hipMemcpyAsync(d_pb, plan.pslot_body.data(), pslots * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    if (!ops.empty()) NBX_HIP_TRY(hipMemcpyAsync(d_ops, ops.data(), ops.size() * sizeof(CopyOp), hipMemcpyHostToDevice, d.stream));
    if (!blocks.empty()) NBX_HIP_TRY(hipMemcpyAsync(d_blocks, blocks.data(), blocks.size() * sizeof(LeafBlock), hipMemcpyHostToDevice, d.stream));
    if (!plan.pack_blocks.empty()) {
        NBX_HIP_TRY(hipMemcpyAsync(d_subs, plan.pack_subs.data(), sizes[7], hipMemcpyHostToDevice, d.stream));
        NBX_HIP_TRY(hipMemcpyAsync(d_packs, plan.pack_blocks.data(), sizes[8], hipMemcpyHostToDevice, d.stream));
    }
    NBX_HIP_TRY(hipMemsetAsync(dforces, 0, n * (size_t)dim * sizeof(double), d.stream));
    NBX_HIP_TRY(hipMemsetAsync(d_max_mass, 0, sizeof(uint32_t), d.stream));
    (void)hipGetLastError();
    NBX_HIP_TRY(nbx_near::enqueue_gather_staged(raw, stride_bytes / sizeof(double), dim, d_pb, pslots, xp, d_max_mass, d.stream));
    nbx_near::NearDevice near;
    near.xp = xp; near.pslots = (uint32_t)pslots; near.ops = d_ops; near.blocks = d_blocks; near.packs = d_packs; near.subs = d_subs;
    near.n_blocks = blocks.size(); near.n_packs = plan.pack_blocks.size(); near.waves = plan.waves;
    near.sums = acc; near.max_mass = d_max_mass;
    NBX_HIP_TRY(hipEventRecord(d.ev0, d.stream));
    NBX_HIP_TRY(nbx_near::enqueue_near(near, dim, law, d.stream, false));   // two launches here, also where a plan fuses them
    NBX_HIP_TRY(hipEventRecord(d.ev1, d.stream));
    NBX_HIP_TRY(nbx_near::enqueue_scatter(acc, raw, stride_bytes / sizeof(double), dim, d_pb, pslots, signed_G(law, G), dforces, d.stream));
    NBX_HIP_TRY(hipMemcpyAsync(forces_out, dforces, n * (size_t)dim * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    NBX_HIP_TRY(hipStreamSynchronize(d.stream));
    if (kernel_ms) NBX_HIP_TRY(hipEventElapsedTime(kernel_ms, d.ev0, d.ev1));
    return NBX_OK;
}

namespace {

int plan_set_device(const nbx_leaf_plan* p) {
    (void)hipGetLastError();
    NBX_HIP_TRY(hipSetDevice(p->device));
    return NBX_OK;
}

// Work about to be queued on `s` must see the plan's buffers as the last evaluation (possibly on another stream) left them.
int plan_order_after_last(nbx_leaf_plan* p, hipStream_t s) {
    if (p->last_stream && p->last_stream != s) NBX_HIP_TRY(hipStreamWaitEvent(s, p->done, 0));
    return NBX_OK;
}

int plan_mark_done(nbx_leaf_plan* p, hipStream_t s) {
    NBX_HIP_TRY(hipEventRecord(p->done, s));
    p->last_stream = s;
    return NBX_OK;
}

// How an entry point that queues work for a plan opens: the plan's device current (the caller's is put back when the scope goes)
// and stream `s` ordered behind the last evaluation.
struct PlanScope {
    DeviceScope device;
    int rc;
    PlanScope(nbx_leaf_plan* p, hipStream_t s) : rc(plan_set_device(p)) { if (!rc) rc = plan_order_after_last(p, s); }
};

float plan_eps2(const nbx_leaf_plan* p) { return (float)(p->softening * p->softening); }

// The last evaluation, for whoever asks for forces or kicks next: its law and sign, and where its masses are -- context c's m64
// (stride 1), or with c == nullptr the plan's staged bodies (offset 2 dim, `staged_stride` doubles apart).
void plan_record_evaluation(nbx_leaf_plan* p, int law, double signedG, const nbx_ctx* c, size_t staged_stride = 1) {
    p->evaluated = true; p->last_law = law;
    p->last_signedG = signedG;
    p->last_mass = c ? c->m64 : p->raw.as<double>() + 2 * p->dim;
    p->last_mass_stride = c ? 1 : staged_stride;
    p->last_ctx_id = c ? c->id : 0;
}

// the plan moved the context's bodies: the context's own accelerations (if any) and close-set lists belong to the old positions
void ctx_bodies_moved(nbx_ctx* c) {
    c->have_accel = false;
    c->tgt_cand_valid = 0; c->bad_list_pass = -1;
}

SlotKickArgs slot_kick_args(const nbx_leaf_plan* p, const nbx_ctx* c, double signedG, double dt_kick, double dt_drift, bool drift) {
    SlotKickArgs k;
    k.sums = p->sums; k.body_slot = p->body_slot; k.pslots = (uint32_t)p->pslots; k.dim = p->dim; k.pad = c->pad; k.drift = drift; k.count = c->count;
    k.signedG = signedG; k.dt_kick = dt_kick; k.dt_drift = dt_drift; k.x64 = c->x64; k.v64 = c->v64; k.m64 = c->m64; k.pos_chunk = c->pos_all;
    return k;
}

// The plan's pointers into its block as the device planner's layout has them (leaf_plan_device.h) ...
void plan_adopt_layout(nbx_leaf_plan* p, const nbx_leaf_dev::Layout& L) {
    const nbx_leaf_dev::DevicePlan d = nbx_leaf_dev::plan_pointers(p->arena.get(), L);
    p->xp = d.xp; p->sums = d.sums; p->pslot_body = d.pslot_body; p->body_slot = d.body_slot; p->ops = d.ops; p->blocks = d.blocks;
    p->subs = d.subs; p->packs = d.packs; p->max_mass = d.max_mass;
    p->unit_off = reinterpret_cast<uint32_t*>(p->arena.get() + L.unit_off);
}
// ... and the counts its 64-byte summary brought back
void plan_adopt_summary(nbx_leaf_plan* p) {
    const nbx_leaf_dev::Summary& S = p->summary_host;
    p->device_planned = true;
    p->waves = (int)S.waves; p->pslots = S.pslots; p->n_ops = S.n_ops; p->n_blocks = S.n_blocks; p->n_subs = S.n_subs; p->n_packs = S.n_packs;
}

// As a new layout is left, queued on s behind it: the sums of slots no workgroup writes (a leaf's pad) are zero, and the pads of odd
// leaves are massless and far away (the body-major gather never touches them).
int plan_fresh_sums_and_pads(nbx_leaf_plan* p, hipStream_t s) {
    const size_t sum_bytes = (size_t)p->dim * p->pslots * sizeof(double);
    NBX_HIP_TRY(hipMemsetAsync(p->sums, 0, sum_bytes ? sum_bytes : 8, s));
    if (p->pslots) NBX_HIP_TRY(nbx_near::enqueue_init_pads(p->pslot_body, p->pslots, p->dim, p->xp, s));
    return NBX_OK;
}

// What an evaluation under `law` needs beyond its arguments, before anything is launched.  Only NBX_LAW_NEWTON needs anything: a
// softening length, and masses for which the heaviest body's weight at zero distance, max|m| / eps^3, is a finite, normal fp32 number
// (the context's rule, nbx_api.hip: neither an overflow nor an all-zero field with status OK).  mass_max < 0: not known, not checked.
int plan_check_law(const nbx_leaf_plan* p, int law, double mass_max) {
    if (law != NBX_LAW_NEWTON) return NBX_OK;
    if (!(p->softening > 0.0)) return fail(NBX_ERR_STATE, "NBX_LAW_NEWTON needs a softening length (nbx_leaf_plan_set_softening)");
    const double eps3 = (double)plan_eps2(p) * p->softening;
    if (mass_max >= 0.0 || mass_max != mass_max) {
        if (!(mass_max / eps3 < 1.0e38)) return fail(NBX_ERR_INVALID, "softening too small for these masses: m / eps^3 must stay finite in fp32");
        if (mass_max > 0.0 && !(mass_max / eps3 > 1.0e-30)) return fail(NBX_ERR_INVALID, "softening too large for these masses: m / eps^3 underflows in fp32");
    }
    return NBX_OK;
}

// plan_check_law for host bodies about to be staged: one host pass over their masses under NBX_LAW_NEWTON (no other law pays for it)
int plan_check_law_staged(const nbx_leaf_plan* p, int law, const void* bodies, size_t stride_bytes) {
    if (law != NBX_LAW_NEWTON) return NBX_OK;
    double mass_max = 0.0;
    const char* const m0 = static_cast<const char*>(bodies) + 2 * (size_t)p->dim * sizeof(double);
    for (size_t i = 0; i < p->n; ++i) {
        double m;
        std::memcpy(&m, m0 + i * stride_bytes, sizeof m);
        m = std::fabs(m);
        if (!(m <= mass_max)) mass_max = m;      // a NaN stays: refused by plan_check_law
    }
    return plan_check_law(p, law, mass_max);
}

// the near field: the pair kernels, which WRITE the slot-ordered sums
int plan_launch_near(nbx_leaf_plan* p, int law, hipStream_t s, bool timed) {
    if (p->n_blocks == 0 && p->n_packs == 0) return NBX_OK;
    if (timed) NBX_HIP_TRY(hipEventRecord(p->ev0, s));
    nbx_near::NearDevice d;
    d.xp = p->xp; d.pslots = (uint32_t)p->pslots; d.ops = p->ops; d.blocks = p->blocks; d.packs = p->packs; d.subs = p->subs;
    d.n_blocks = p->n_blocks; d.n_packs = p->n_packs; d.waves = p->waves;
    d.sums = p->sums; d.max_mass = p->max_mass; d.eps2 = plan_eps2(p);
    NBX_HIP_TRY(nbx_near::enqueue_near(d, p->dim, law, s, true));
    if (timed) NBX_HIP_TRY(hipEventRecord(p->ev1, s));
    return NBX_OK;
}

// The second moments' arrays for the plan's cells at order 1 (one block, kept and reused while it fits; a plan at order 0 never gets
// here with anything to do).  The caller has made sure that nothing on the device still uses the block: every caller has waited for
// the plan's last evaluation.
int plan_fit_quads(nbx_leaf_plan* p) {
    nbx_far::FarDevice& f = p->far;
    f.order = p->far_order;
    f.leaf_quad = nullptr; f.cell_quad = nullptr; f.cell_qrec = nullptr;
    p->quads_evaluated = false;
    if (p->far_order != NBX_FAR_QUADRUPOLE || !f.n_cells) return NBX_OK;
    const size_t sizes[3] = {(size_t)f.n_leaves * 6 * sizeof(double), (size_t)f.n_cells * nbx_far::quad_count(p->dim) * sizeof(double),
                             (size_t)f.n_cells * nbx_far::quad_rec_vecs(p->dim) * sizeof(float4)};
    const auto cut = carve(sizes);
    f.order = NBX_FAR_MONOPOLE;                         // should the allocation fail, the cells stay consistent at order 0
    NBX_HIP_TRY(nbx_block::fit(p->quad_arena, leaf_pool(), p->device, cut.total));
    f.order = p->far_order;
    f.leaf_quad = cut.at<double>(p->quad_arena.get(), 0);
    f.cell_quad = cut.at<double>(p->quad_arena.get(), 1);
    f.cell_qrec = cut.at<float4>(p->quad_arena.get(), 2);
    return NBX_OK;
}

// The far field (leaf_far_kernel.hip): the far terms of the plan's cells ADDED to the sums the pair kernels wrote.  `with_moments`:
// this evaluation's moment pass ran just before (nbx_leaf_plan_time_kernel repeats the far pass on the last evaluation's).
int plan_launch_far(nbx_leaf_plan* p, int law, hipStream_t s, bool timed, bool with_moments = true) {
    if (!p->far.n_cells) return NBX_OK;
    nbx_far::FarDevice f = p->far;
    f.eps2 = plan_eps2(p);
    if (!with_moments && !p->quads_evaluated) f.order = NBX_FAR_MONOPOLE;   // no second moments of these positions: the order the sums were made at
    if (timed) NBX_HIP_TRY(hipEventRecord(p->evf0, s));
    NBX_HIP_TRY(nbx_far::enqueue_far(f, p->dim, law, s));
    if (timed) NBX_HIP_TRY(hipEventRecord(p->evf1, s));
    p->cells_evaluated = true;
    p->cells_timed = timed;
    if (with_moments) p->quads_evaluated = f.order == NBX_FAR_QUADRUPOLE;
    return NBX_OK;
}

// One evaluation's kernels behind the gather: the cells' moments from the positions just gathered, the near field, the far field.
// A plan without cells launches the pair kernels and nothing else.
int plan_launch_pairs(nbx_leaf_plan* p, int law, hipStream_t s, bool timed) {
    if (p->far.n_cells) {
        if (timed) NBX_HIP_TRY(hipEventRecord(p->evm0, s));
        NBX_HIP_TRY(nbx_far::enqueue_moments(p->far, p->dim, s));
        if (timed) NBX_HIP_TRY(hipEventRecord(p->evm1, s));
    }
    if (int rc = plan_launch_near(p, law, s, timed)) return rc;
    return plan_launch_far(p, law, s, timed);
}

int plan_forces_out(nbx_leaf_plan* p, hipStream_t s, double* forces_out) {
    if (p->last_ctx_id && !nbx::ctx_alive(p->last_ctx_id))   // the masses were read where the evaluation found them: in a context that is gone
        return fail(NBX_ERR_STATE, "the context of the last evaluation no longer exists: evaluate again before asking for forces");
    if (!p->forces && p->n) {
        NBX_HIP_TRY(nbx_block::allocate(p->forces_own, p->device, p->n * (size_t)p->dim * sizeof(double)));
        p->forces = p->forces_own.as<double>();
    }
    if (p->n) {
        NBX_HIP_TRY(nbx_near::enqueue_forces_by_body(p->sums, p->pslots, p->body_slot, p->n, p->dim, p->last_signedG, p->last_mass, p->last_mass_stride,
                                                     p->forces, s));
        NBX_HIP_TRY(hipMemcpyAsync(forces_out, p->forces, p->n * (size_t)p->dim * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    NBX_HIP_TRY(hipStreamSynchronize(s));
    return NBX_OK;
}


// The plan's buffers on the device, laid out there (leaf_plan_device.h): the four CSR arrays go over as they are, ~35 kernels build
// what plan_leaves builds on the host, 64 bytes come back.  forces_bytes > 0 reserves the one-shot call's force array in the same block.
int create_plan_on_device(nbx_leaf_plan* p, const uint32_t* leaf_offsets, const uint32_t* leaf_bodies, size_t n_leaves, const uint32_t* list_offsets,
                          const uint32_t* list_sources, size_t slots, size_t n_list, size_t forces_bytes) {
    using namespace nbx_leaf_dev;
    const Bounds b{p->n, n_leaves, slots, n_list};
    const Layout L = make_layout(b, p->dim);
    const size_t forces_off = L.total;
    const size_t total = L.total + (forces_bytes ? nbx_block::carve_span(forces_bytes) : 0);
    NBX_HIP_TRY(nbx_block::take(p->arena, leaf_pool(), p->device, total));
    plan_adopt_layout(p, L);
    if (forces_bytes) p->forces = reinterpret_cast<double*>(p->arena.get() + forces_off);
    NBX_HIP_TRY(enqueue_device_plan(b, p->dim, leaf_offsets, leaf_bodies, list_offsets, list_sources, NBX_LEAF_PACK != 0, p->arena.get(), L, p->stream, &p->summary_host));
    NBX_HIP_TRY(hipStreamSynchronize(p->stream));
    const Summary& S = p->summary_host;
    if (S.err != kErrNone) return fail(NBX_ERR_INVALID, error_text(S.err));
    plan_adopt_summary(p);
    return NBX_OK;
}

int create_plan_on_host(nbx_leaf_plan* p, const uint32_t* leaf_offsets, const uint32_t* leaf_bodies, size_t n_leaves, const uint32_t* list_offsets,
                        const uint32_t* list_sources, size_t forces_bytes) {
    const size_t n = p->n;
    const int dim = p->dim;
    LeafPlan host;
    if (int prc = lay_out_launch(leaf_offsets, leaf_bodies, n_leaves, list_offsets, list_sources, host)) return prc;
    p->waves = host.waves;
    p->pslots = host.pslots(); p->n_ops = host.ops.size(); p->n_blocks = host.blocks.size();
    p->n_subs = host.pack_subs.size(); p->n_packs = host.pack_blocks.size();
    std::vector<uint32_t> body_slot;
    try { body_slot.assign(n, 0xffffffffu); } catch (...) { return fail(NBX_ERR_ALLOC, "host allocation failed"); }
    for (size_t s = 0; s < p->pslots; ++s)
        if (host.pslot_body[s] != 0xffffffffu) body_slot[host.pslot_body[s]] = (uint32_t)s;
    const size_t sizes[11] = {(p->pslots + 2) * sizeof(float4), (size_t)dim * p->pslots * sizeof(double), p->pslots * sizeof(uint32_t),
                              n * sizeof(uint32_t), p->n_ops * sizeof(CopyOp), p->n_blocks * sizeof(LeafBlock), sizeof(uint32_t),
                              p->n_subs * sizeof(PackSub), p->n_packs * sizeof(PackBlock), forces_bytes, host.unit_off.size() * sizeof(uint32_t)};
    const auto cut = carve(sizes);
    NBX_HIP_TRY(nbx_block::take(p->arena, leaf_pool(), p->device, cut.total));   // a tree code makes a plan per step: the last plan's block, parked by its destroy
    char* const arena = p->arena.get();
    p->xp = cut.at<float4>(arena, 0);
    p->sums = cut.at<double>(arena, 1);
    p->pslot_body = cut.at<uint32_t>(arena, 2);
    p->body_slot = cut.at<uint32_t>(arena, 3);
    p->ops = cut.at<CopyOp>(arena, 4);
    p->blocks = cut.at<LeafBlock>(arena, 5);
    p->max_mass = cut.at<uint32_t>(arena, 6);
    p->subs = cut.at<PackSub>(arena, 7);
    p->packs = cut.at<PackBlock>(arena, 8);
    if (forces_bytes) p->forces = cut.at<double>(arena, 9);
    p->unit_off = cut.at<uint32_t>(arena, 10);   // the far field's passes walk the leaves' slots by it (leaf_far.h)
    if (sizes[10]) NBX_HIP_TRY(hipMemcpyAsync(p->unit_off, host.unit_off.data(), sizes[10], hipMemcpyHostToDevice, p->stream));
    if (p->n_packs) {
        NBX_HIP_TRY(hipMemcpyAsync(p->subs, host.pack_subs.data(), sizes[7], hipMemcpyHostToDevice, p->stream));
        NBX_HIP_TRY(hipMemcpyAsync(p->packs, host.pack_blocks.data(), sizes[8], hipMemcpyHostToDevice, p->stream));
    }
    if (p->pslots) NBX_HIP_TRY(hipMemcpyAsync(p->pslot_body, host.pslot_body.data(), sizes[2], hipMemcpyHostToDevice, p->stream));
    if (n) NBX_HIP_TRY(hipMemcpyAsync(p->body_slot, body_slot.data(), sizes[3], hipMemcpyHostToDevice, p->stream));
    if (p->n_ops) NBX_HIP_TRY(hipMemcpyAsync(p->ops, host.ops.data(), sizes[4], hipMemcpyHostToDevice, p->stream));
    if (p->n_blocks) NBX_HIP_TRY(hipMemcpyAsync(p->blocks, host.blocks.data(), sizes[5], hipMemcpyHostToDevice, p->stream));
    NBX_HIP_TRY(hipStreamSynchronize(p->stream));   // the host arrays above go out of scope
    p->unit_host.swap(host.unit_off);
    return NBX_OK;
}

// What a new plan of either kind holds before it has a structure: its device made current (the caller's scope puts the old one
// back), a stream from the parked pool, the pair kernels' two timing events and the event every piece of queued work is followed by.
int plan_open(nbx_leaf_plan* p) {
    NBX_HIP_TRY(hipSetDevice(p->device));
    NBX_HIP_TRY(nbx::take_stream(p->device, &p->stream));
    NBX_HIP_TRY(hipEventCreate(&p->ev0));
    NBX_HIP_TRY(hipEventCreate(&p->ev1));
    NBX_HIP_TRY(hipEventCreateWithFlags(&p->done, hipEventDisableTiming));
    return NBX_OK;
}

// nbx_leaf_plan_create and the one-shot call's plan: validation, the layout (device or host planner), the buffers an evaluation needs.
int create_plan(nbx_leaf_plan** out, int device, int dim, size_t n, const uint32_t* leaf_offsets, const uint32_t* leaf_bodies, size_t n_leaves,
                const uint32_t* list_offsets, const uint32_t* list_sources, size_t forces_bytes) {
    if (!out) return fail(NBX_ERR_INVALID, "out is null");
    *out = nullptr;
    if (dim != 2 && dim != 3) return fail(NBX_ERR_INVALID, "dim must be 2 or 3");
    size_t slots = 0, n_list = 0;
    if (int vrc = validate_offsets(n, leaf_offsets, leaf_bodies, n_leaves, list_offsets, list_sources, &slots, &n_list)) return vrc;
    const bool on_device = use_device_planner(n_leaves, slots, n_list);
    if (!on_device)   // the host planner follows every index: all of them are checked first (the device planner checks as it goes)
        if (int vrc = validate_csr(n, leaf_bodies, n_leaves, list_sources, slots, n_list)) return vrc;
    int ndev = 0;
    int rc = nbx_device_count(&ndev);
    if (rc != NBX_OK) return rc;
    if (device < 0 || device >= ndev) return fail(NBX_ERR_NO_DEVICE, "device ordinal out of range");
    nbx_leaf_plan* p = new (std::nothrow) nbx_leaf_plan();
    if (!p) return fail(NBX_ERR_ALLOC, "host allocation failed");
    PlanHolder hold(p);
    p->device = device; p->dim = dim; p->n = n; p->n_leaves = n_leaves;
    DeviceScope scope;
    if ((rc = plan_open(p))) return rc;
    rc = on_device ? create_plan_on_device(p, leaf_offsets, leaf_bodies, n_leaves, list_offsets, list_sources, slots, n_list, forces_bytes)
                   : create_plan_on_host(p, leaf_offsets, leaf_bodies, n_leaves, list_offsets, list_sources, forces_bytes);
    // the fresh sums: queued behind the layout, waited for by whoever evaluates first (plan_order_after_last)
    if (!rc) rc = plan_fresh_sums_and_pads(p, p->stream);
    if (!rc) rc = plan_mark_done(p, p->stream);
    if (!rc) *out = hold.release();
    return rc;
}

}  // namespace

namespace {
// Gives the cells' device arrays back (parked when nothing on the device can still touch them) and forgets the cells; with
// `events` the four timing events go too (destroy).
void plan_release_cells(nbx_leaf_plan* p, bool device_idle, bool events) {
    p->cell_arena.release(device_idle);
    p->far = nbx_far::FarDevice();
    p->far_entries = 0;
    p->cells_evaluated = p->cells_timed = p->quads_evaluated = false;
    if (events) {
        p->quad_arena.release(device_idle);            // destroy: the block of the second moments goes too (set_cells keeps it for the next cells)
        hipEvent_t* const evs[4] = {&p->evm0, &p->evm1, &p->evf0, &p->evf1};
        for (hipEvent_t* e : evs) {
            if (*e) (void)hipEventDestroy(*e);
            *e = nullptr;
        }
    }
}

// Build (or build again) the octree of a plan made by nbx_leaf_plan_create_octree from the context's current positions, and lay the
// plan and its far field out, all on the context's stream.  Two read-backs of 64 bytes: the builder's counts, the planner's summary.
// A refusal leaves the plan without a structure (octree_built = false) but with its blocks, for the next build.
int plan_build_octree(nbx_leaf_plan* p, nbx_ctx* c) {
    using namespace nbx_leaf_dev;
    hipStream_t s = c->stream;
    if (int rc = plan_order_after_last(p, s)) return rc;
    p->octree_built = false;
    p->evaluated = false;
    p->cells_evaluated = p->cells_timed = p->quads_evaluated = false;
    p->far = nbx_far::FarDevice();
    p->far_entries = 0;
    const int dim = p->dim, depth = p->octree_depth;
    const nbx_octree::TreeLayout& T = p->tree_layout;
    NBX_HIP_TRY(nbx_block::fit(p->tree_arena, leaf_pool(), p->device, T.total));
    if (p->octree_capacity)
        NBX_HIP_TRY(nbx_octree::enqueue_build_adaptive(c->x64, c->pad, p->n, dim, depth, p->octree_capacity, p->octree_theta, p->tree_arena.get(), T, s, &p->counts_host,
                                                       &p->tree));
    else
        NBX_HIP_TRY(nbx_octree::enqueue_build(c->x64, c->pad, p->n, dim, depth, p->octree_theta, p->tree_arena.get(), T, s, &p->counts_host, &p->tree));
    NBX_HIP_TRY(hipStreamSynchronize(s));   // the counts are here; whatever used the plan's blocks before is over
    if (int rc = plan_mark_done(p, s)) return rc;
    const nbx_octree::Counts C = p->counts_host;
    if (C.bad) return fail(NBX_ERR_INVALID, "a coordinate is not finite");
    if (C.near_entries > 0xfffffff0ull) return fail(NBX_ERR_INVALID, "near lists too long");
    if (C.far_entries > 0xfffffff0ull) return fail(NBX_ERR_INVALID, "far lists too long");
    // the plan's block, sized by the counts (leaf_plan_device.h)
    const Bounds b{p->n, C.n_leaves, p->n, (size_t)C.near_entries};
    const Layout L = make_layout(b, dim);
    NBX_HIP_TRY(nbx_block::fit(p->arena, leaf_pool(), p->device, L.total));
    plan_adopt_layout(p, L);
    p->unit_host.clear();
    p->n_leaves = C.n_leaves;
    uint32_t* const list_sources = reinterpret_cast<uint32_t*>(p->arena.get() + L.list_sources);
    p->list_sources_dev = list_sources;
    // the cells' block: far lists, the far pass's waves, the moments, the far layout's scratch
    const size_t nc = C.n_cells, nl = C.n_leaves;
    const size_t sizes[7] = {(size_t)C.far_entries * 4, (size_t)C.far_blocks * sizeof(nbx_far::FarBlock), nl * 4 * sizeof(double), nc * sizeof(double),
                             nc * (size_t)dim * sizeof(double), nc * sizeof(float4), nbx_octree::far_scratch_bytes(C.far_blocks)};
    const auto cut = carve(sizes);
    NBX_HIP_TRY(nbx_block::fit(p->cell_arena, leaf_pool(), p->device, cut.total));
    for (hipEvent_t* ev : {&p->evm0, &p->evm1, &p->evf0, &p->evf1})
        if (!*ev) NBX_HIP_TRY(hipEventCreate(ev));
    char* const cells = p->cell_arena.get();
    uint32_t* const far_cells = cut.at<uint32_t>(cells, 0);
    nbx_far::FarBlock* const far_blocks = cut.at<nbx_far::FarBlock>(cells, 1);
    if (p->octree_capacity)
        NBX_HIP_TRY(nbx_octree::enqueue_fill_adaptive(p->n, dim, depth, p->octree_capacity, p->octree_theta, p->tree_arena.get(), T, list_sources, far_cells, s));
    else
        NBX_HIP_TRY(nbx_octree::enqueue_fill(p->n, dim, depth, p->octree_theta, p->tree_arena.get(), T, list_sources, far_cells, s));
    NBX_HIP_TRY(enqueue_device_plan(b, dim, p->tree.leaf_offsets, p->tree.leaf_bodies, p->tree.list_offsets, list_sources, NBX_LEAF_PACK != 0, p->arena.get(), L, s,
                                    &p->summary_host, true));
    if (nc) NBX_HIP_TRY(nbx_octree::enqueue_far_layout(p->unit_off, C, p->tree_arena.get(), T, far_blocks, cut.at<char>(cells, 6), s));
    NBX_HIP_TRY(hipStreamSynchronize(s));
    if (p->summary_host.err != kErrNone) return fail(NBX_ERR_INVALID, error_text(p->summary_host.err));
    plan_adopt_summary(p);
    if (nc) {
        nbx_far::FarDevice& f = p->far;
        f.xp = p->xp; f.unit_off = p->unit_off; f.sums = p->sums;
        f.pslots = (uint32_t)p->pslots; f.n_leaves = C.n_leaves; f.n_cells = C.n_cells;
        f.n_small = C.n_small; f.n_big = C.n_cells - C.n_small; f.n_blocks = C.far_blocks;
        f.cell_first = p->tree.cell_first; f.cell_count = p->tree.cell_count;
        f.small_cells = p->tree.small_cells; f.big_cells = p->tree.small_cells + C.n_small;
        f.far_cells = far_cells; f.blocks = far_blocks;
        f.leaf_mom = cut.at<double>(cells, 2);
        f.cell_mass = cut.at<double>(cells, 3);
        f.cell_com = cut.at<double>(cells, 4);
        f.cell_rec = cut.at<float4>(cells, 5);
        p->far_entries = (size_t)C.far_entries;
        if (int rc = plan_fit_quads(p)) { p->far = nbx_far::FarDevice(); p->far_entries = 0; return rc; }   // the stream is idle (synchronised above)
    }
    if (int rc = plan_fresh_sums_and_pads(p, s)) return rc;   // as create_plan leaves a new plan
    p->octree_built = true;
    return plan_mark_done(p, s);
}

int plan_needs_structure(const nbx_leaf_plan* p) {
    if (p->octree && !p->octree_built) return fail(NBX_ERR_STATE, "the plan's last octree build was refused: rebuild it first");
    return NBX_OK;
}

// `uploaded`: bodies must be there to be read (a kick of what the last evaluation read asks for that evaluation instead)
int plan_check_ctx(const nbx_leaf_plan* p, const nbx_ctx* c, bool uploaded = true) {
    if (c->device != p->device || c->dim != p->dim || c->n_total != p->n || c->n_shards != 1)
        return fail(NBX_ERR_INVALID, "the context must be a single-shard context of the plan's device, dimension and body count");
    if (uploaded && !c->uploaded) return fail(NBX_ERR_STATE, "upload bodies to the context first");
    return NBX_OK;
}

// both octree entry points: leaf_capacity = 0 is the fixed-depth tree
int create_octree_plan(nbx_leaf_plan** out, nbx_ctx* c, int depth, size_t leaf_capacity, double theta) {
    if (!out) return fail(NBX_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!c) return fail(NBX_ERR_INVALID, "ctx is null");
    if (depth < 0 || depth > nbx_octree::kMaxDepth) return fail(NBX_ERR_INVALID, "depth must be in [0, 10]");
    if (!(theta >= 0.0) || !std::isfinite(theta)) return fail(NBX_ERR_INVALID, "theta must be finite and >= 0");
    if (c->n_shards != 1) return fail(NBX_ERR_INVALID, "the context must be a single-shard context");
    if (c->n_total == 0 || c->n_total > ((size_t)1 << 31)) return fail(NBX_ERR_INVALID, "the context must hold between 1 and 2^31 bodies");
    if (!c->uploaded) return fail(NBX_ERR_STATE, "upload bodies to the context first");
    nbx_leaf_plan* p = new (std::nothrow) nbx_leaf_plan();
    if (!p) return fail(NBX_ERR_ALLOC, "host allocation failed");
    PlanHolder hold(p);
    p->device = c->device; p->dim = c->dim; p->n = c->n_total;
    p->octree = true; p->octree_depth = depth; p->octree_theta = theta; p->octree_capacity = leaf_capacity;
    p->tree_layout = nbx_octree::make_tree_layout(p->n, p->dim, depth, leaf_capacity > 0);
    DeviceScope scope;
    int rc = plan_open(p);
    if (!rc) rc = plan_build_octree(p, c);
    if (!rc) *out = hold.release();
    return rc;
}
}  // namespace

extern "C" {

int nbx_leaf_plan_create_octree(nbx_leaf_plan** out, nbx_ctx* c, int depth, double theta) { return create_octree_plan(out, c, depth, 0, theta); }

int nbx_leaf_plan_create_octree_adaptive(nbx_leaf_plan** out, nbx_ctx* c, int max_depth, int leaf_capacity, double theta) {
    if (leaf_capacity < 0) {
        if (out) *out = nullptr;
        return fail(NBX_ERR_INVALID, out ? "leaf_capacity must be >= 0" : "out is null");
    }
    return create_octree_plan(out, c, max_depth, (size_t)leaf_capacity, theta);
}

int nbx_leaf_plan_rebuild_octree(nbx_leaf_plan* p, nbx_ctx* c) {
    if (!p || !c) return fail(NBX_ERR_INVALID, "null argument");
    if (!p->octree) return fail(NBX_ERR_STATE, "the plan was not made by nbx_leaf_plan_create_octree");
    if (int rc = plan_check_ctx(p, c)) return rc;
    DeviceScope scope;
    if (int rc = plan_set_device(p)) return rc;
    return plan_build_octree(p, c);
}

int nbx_leaf_plan_structure_sizes(const nbx_leaf_plan* p, size_t* n_leaves, size_t* near_entries, size_t* n_cells, size_t* far_entries) {
    if (!p) return fail(NBX_ERR_INVALID, "plan is null");
    if (!p->octree || !p->octree_built) return fail(NBX_ERR_STATE, "the plan holds no structure built on the device");
    if (n_leaves) *n_leaves = p->counts_host.n_leaves;
    if (near_entries) *near_entries = (size_t)p->counts_host.near_entries;
    if (n_cells) *n_cells = p->counts_host.n_cells;
    if (far_entries) *far_entries = (size_t)p->counts_host.far_entries;
    return NBX_OK;
}

int nbx_leaf_plan_get_structure(nbx_leaf_plan* p, uint32_t* leaf_offsets, uint32_t* leaf_bodies, uint32_t* list_offsets, uint32_t* list_sources,
                                uint32_t* cell_first_leaf, uint32_t* cell_leaf_count, uint32_t* far_offsets, uint32_t* far_cells) {
    if (!p) return fail(NBX_ERR_INVALID, "plan is null");
    if (!p->octree || !p->octree_built) return fail(NBX_ERR_STATE, "the plan holds no structure built on the device");
    hipStream_t s = p->stream;
    PlanScope in(p, s);
    if (in.rc) return in.rc;
    const nbx_octree::Counts& C = p->counts_host;
    const size_t nl = C.n_leaves, nc = C.n_cells;
    // the far lists live with the cells; nbx_leaf_plan_set_cells on this plan would have replaced them
    const uint32_t* const far_dev = p->far.n_cells == nc ? p->far.far_cells : nullptr;
    if (far_cells && C.far_entries && !far_dev) return fail(NBX_ERR_STATE, "the plan's cells were replaced by nbx_leaf_plan_set_cells");
    struct Piece { uint32_t* to; const uint32_t* from; size_t words; };
    const Piece pieces[8] = {{leaf_offsets, p->tree.leaf_offsets, nl + 1}, {leaf_bodies, p->tree.leaf_bodies, p->n}, {list_offsets, p->tree.list_offsets, nl + 1},
                             {list_sources, p->list_sources_dev, (size_t)C.near_entries}, {cell_first_leaf, p->tree.cell_first, nc},
                             {cell_leaf_count, p->tree.cell_count, nc}, {far_offsets, p->tree.far_offsets, nl + 1}, {far_cells, far_dev, (size_t)C.far_entries}};
    for (const Piece& piece : pieces)
        if (piece.to && piece.words) NBX_HIP_TRY(hipMemcpyAsync(piece.to, piece.from, piece.words * 4, hipMemcpyDeviceToHost, s));
    NBX_HIP_TRY(hipStreamSynchronize(s));
    return plan_mark_done(p, s);
}

int nbx_leaf_plan_create(nbx_leaf_plan** out, int device, int dim, size_t n, const uint32_t* leaf_offsets, const uint32_t* leaf_bodies,
                         size_t n_leaves, const uint32_t* list_offsets, const uint32_t* list_sources) {
    return create_plan(out, device, dim, n, leaf_offsets, leaf_bodies, n_leaves, list_offsets, list_sources, 0);
}

int nbx_leaf_plan_destroy(nbx_leaf_plan* p) {
    if (!p) return NBX_OK;
    DeviceScope scope;
    (void)hipSetDevice(p->device);
    // the last evaluation may have been queued on a context's stream, and that context may be gone by now (its stream with it):
    // wait on the plan's own event, which every piece of work queued on a foreign stream is followed by
    const bool last_wait_ok = !(p->last_stream && p->done) || hipEventSynchronize(p->done) == hipSuccess;
    const bool idle = p->stream && hipStreamSynchronize(p->stream) == hipSuccess;
    const bool all_idle = idle && last_wait_ok;   // else the blocks are freed, not parked
    plan_release_cells(p, all_idle, true);
    p->arena.release(all_idle);
    p->tree_arena.release(all_idle);
    p->forces_own.release(all_idle);
    p->raw.release(all_idle);
    p->phi_block.release(all_idle);
    p->phi_raw.release(all_idle);
    p->amax_block.release(all_idle);
    p->clock_block.release(all_idle);
    if (p->stop_look) (void)hipHostFree(p->stop_look);
    if (p->look_done) (void)hipEventDestroy(p->look_done);
    if (p->ev0) (void)hipEventDestroy(p->ev0);
    if (p->ev1) (void)hipEventDestroy(p->ev1);
    if (p->done) (void)hipEventDestroy(p->done);
    if (p->stream) { if (idle) nbx::park_stream(p->device, p->stream); else (void)hipStreamDestroy(p->stream); }
    (void)hipGetLastError();
    delete p;
    return NBX_OK;
}

int nbx_leaf_plan_info(const nbx_leaf_plan* p, size_t* slots, size_t* runs, size_t* workgroups, int* waves) {
    if (!p) return fail(NBX_ERR_INVALID, "plan is null");
    if (slots) *slots = p->pslots;
    if (runs) *runs = p->n_ops;
    if (workgroups) *workgroups = p->n_blocks + p->n_packs;
    if (waves) *waves = p->waves;
    return NBX_OK;
}

int nbx_leaf_plan_forces(nbx_leaf_plan* p, const void* bodies, size_t stride_bytes, int law, double G, double* forces_out, float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    if (!p) return fail(NBX_ERR_INVALID, "plan is null");
    if (law < NBX_LAW_BRUTE || law > NBX_LAW_NEWTON) return fail(NBX_ERR_INVALID, "unknown law");
    if ((!bodies || !forces_out) && p->n) return fail(NBX_ERR_INVALID, "null argument");
    const size_t min_stride = (size_t)(2 * p->dim + 1) * sizeof(double);
    if (stride_bytes < min_stride || stride_bytes % sizeof(double) != 0)
        return fail(NBX_ERR_INVALID, "body stride must be a multiple of 8 and >= sizeof(Body<dim>)");
    if (int src = plan_needs_structure(p)) return src;
    if (int lrc = plan_check_law_staged(p, law, bodies, stride_bytes)) return lrc;
    hipStream_t s = p->stream;
    PlanScope in(p, s);
    if (in.rc) return in.rc;
    const size_t bytes = p->n * stride_bytes;
    if (bytes && bytes + 256 > p->raw.bytes()) {   // the first call, or wider bodies than the block has room for (a freed block is forgotten: Block)
        if (p->raw) NBX_HIP_TRY(hipStreamSynchronize(s));
        NBX_HIP_TRY(nbx_block::allocate(p->raw, p->device, bytes + 256));
    }
    if (bytes) NBX_HIP_TRY(hipMemcpyAsync(p->raw.get(), bodies, bytes, hipMemcpyHostToDevice, s));
    NBX_HIP_TRY(hipMemsetAsync(p->max_mass, 0, sizeof(uint32_t), s));
    if (p->pslots)
        NBX_HIP_TRY(nbx_near::enqueue_gather_staged(p->raw.as<double>(), stride_bytes / sizeof(double), p->dim, p->pslot_body, p->pslots, p->xp, p->max_mass, s));
    if (int rc = plan_launch_pairs(p, law, s, true)) return rc;
    plan_record_evaluation(p, law, signed_G(law, G), nullptr, stride_bytes / sizeof(double));
    if (int rc = plan_mark_done(p, s)) return rc;
    if (int rc = plan_forces_out(p, s, forces_out)) return rc;
    if (kernel_ms && (p->n_blocks || p->n_packs)) NBX_HIP_TRY(hipEventElapsedTime(kernel_ms, p->ev0, p->ev1));
    return NBX_OK;
}

// positions and masses of a context's resident bodies -> the plan's leaf-ordered source pairs, on stream s.  One lane per body
// (coalesced reads, four 4-byte stores into its slot's pair record): 0.048 ms at N = 2^20.  A two-kernel form (SoA -> one float4 per
// body, then one lane per slot reading its body's 16 bytes and writing whole records) was measured at 0.006 + 0.044 ms: no better.
// What had made this gather 0.14-0.17 ms was not its memory traffic but publish_max_mass's predecessor (tools/ubench_gather.hip:
// the traffic alone is 0.02 ms back to back).
static int plan_gather_resident(nbx_leaf_plan* p, nbx_ctx* c, hipStream_t s) {
    if (!p->pslots || !p->n) return NBX_OK;
    NBX_HIP_TRY(nbx_near::enqueue_gather_resident(c->pos_all, c->mass_all, c->pad, p->dim, p->body_slot, p->n, p->xp, p->max_mass, s));
    return NBX_OK;
}

int nbx_leaf_plan_forces_ctx(nbx_leaf_plan* p, nbx_ctx* c, int law, double G, double* forces_out, float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    if (!p || !c) return fail(NBX_ERR_INVALID, "null argument");
    if (law < NBX_LAW_BRUTE || law > NBX_LAW_NEWTON) return fail(NBX_ERR_INVALID, "unknown law");
    if (int crc = plan_check_ctx(p, c)) return crc;
    if (int src = plan_needs_structure(p)) return src;
    if (int lrc = plan_check_law(p, law, c->mass_max)) return lrc;
    hipStream_t s = c->stream;
    PlanScope in(p, s);
    if (in.rc) return in.rc;
    NBX_HIP_TRY(hipMemsetAsync(p->max_mass, 0, sizeof(uint32_t), s));
    if (int rc = plan_gather_resident(p, c, s)) return rc;
    if (int rc = plan_launch_pairs(p, law, s, kernel_ms != nullptr)) return rc;
    plan_record_evaluation(p, law, signed_G(law, G), c);
    if (int rc = plan_mark_done(p, s)) return rc;
    if (forces_out) { if (int rc = plan_forces_out(p, s, forces_out)) return rc; }
    else if (kernel_ms) NBX_HIP_TRY(hipStreamSynchronize(s));
    if (kernel_ms && (p->n_blocks || p->n_packs)) NBX_HIP_TRY(hipEventElapsedTime(kernel_ms, p->ev0, p->ev1));
    return NBX_OK;
}

int nbx_leaf_plan_get_forces(nbx_leaf_plan* p, double* forces_out) {
    if (!p || (!forces_out && p->n)) return fail(NBX_ERR_INVALID, "null argument");
    if (!p->evaluated) return fail(NBX_ERR_STATE, "no evaluation on the device");
    // on the plan's own stream, behind the last evaluation's event (the stream that evaluation ran on may belong to a context that no longer exists)
    PlanScope in(p, p->stream);
    if (in.rc) return in.rc;
    if (int rc = plan_forces_out(p, p->stream, forces_out)) return rc;
    return plan_mark_done(p, p->stream);
}

// ---- kicks and stepping loops (include/nbody_hip.h; "kick-drift-kick through a plan" for the _kdk and kick_drift2 entry points) ----
// The kick of what the last evaluation left in the sums.  `drift` false is the pure kick, which leaves the positions -- and with
// them the context's accelerations and lists -- valid; nbx_leaf_plan_kick_drift drifts for every dt, 0 included.
static int plan_kick(nbx_leaf_plan* p, nbx_ctx* c, double dt_kick, double dt_drift, bool drift, const char* not_evaluated) {
    if (!p || !c) return fail(NBX_ERR_INVALID, "null argument");
    if (!p->evaluated) return fail(NBX_ERR_STATE, not_evaluated);
    if (int crc = plan_check_ctx(p, c, false)) return crc;
    if (p->last_ctx_id != c->id) return fail(NBX_ERR_STATE, "the last evaluation was not made from this context");
    hipStream_t s = c->stream;
    PlanScope in(p, s);
    if (in.rc) return in.rc;
    NBX_HIP_TRY(launch_kick_drift_slots(slot_kick_args(p, c, p->last_signedG, dt_kick, dt_drift, drift), s));
    if (drift) ctx_bodies_moved(c);
    return plan_mark_done(p, s);
}

int nbx_leaf_plan_kick_drift(nbx_leaf_plan* p, nbx_ctx* c, double dt) {
    return plan_kick(p, c, dt, dt, true, "evaluate the leaf sums before kick_drift");
}

int nbx_leaf_plan_kick_drift2(nbx_leaf_plan* p, nbx_ctx* c, double dt_kick, double dt_drift) {
    return plan_kick(p, c, dt_kick, dt_drift, dt_drift != 0.0, "evaluate the leaf sums before kick_drift2");
}

// one evaluation's device work on stream s and the kick (and drift) behind it, nothing else (no events, no waits)
static int plan_enqueue_eval(nbx_leaf_plan* p, nbx_ctx* c, int law, double signedG, double dt_kick, double dt_drift, bool drift, hipStream_t s) {
    NBX_HIP_TRY(hipMemsetAsync(p->max_mass, 0, sizeof(uint32_t), s));
    if (int rc = plan_gather_resident(p, c, s)) return rc;
    if (int rc = plan_launch_pairs(p, law, s, false)) return rc;
    NBX_HIP_TRY(launch_kick_drift_slots(slot_kick_args(p, c, signedG, dt_kick, dt_drift, drift), s));
    return NBX_OK;
}

enum class Scheme { KickDrift, KickDriftKick };

// Every stepping loop, behind its entry point's argument checks.  Kick-drift is nsteps evaluations, each followed by a kick and a
// drift by dt.  Kick-drift-kick is F K(dt/2) D(dt) [F K(dt) D(dt)]^(n-1) F K(dt/2), evaluations 0 .. nsteps with the adjacent
// half-kicks merged into one multiply by dt (nbx_ctx_step_kdk's form); its kicks are nbx_leaf_plan_kick_drift2's, for which a
// drift by 0 is the pure kick.  rebuild_every > 0 rebuilds the plan's octree before every rebuild_every-th evaluation.
static int plan_run_steps(nbx_leaf_plan* p, nbx_ctx* c, int law, double G, double dt, int nsteps, int rebuild_every, Scheme scheme) {
    if (nsteps == 0) return NBX_OK;
    const bool rebuilds = rebuild_every > 0;   // evaluation 0 rebuilds: what the last build left does not matter
    if (!rebuilds)
        if (int src = plan_needs_structure(p)) return src;
    if (int lrc = plan_check_law(p, law, c->mass_max)) return lrc;
    hipStream_t s = c->stream;
    PlanScope in(p, s);
    if (in.rc) return in.rc;
    const double signedG = signed_G(law, G);
    const bool kdk = scheme == Scheme::KickDriftKick;
    // Plain launches, queued ahead of the device: a step is GPU-bound (0.36 ms of kernels at N = 2^20; 5 launches cost the host
    // ~25 us).  A captured HIP graph was measured: 8-15 ms to capture and instantiate, then the same 72.4 ms per 200 steps at
    // N = 2^20 and 7.97 against 8.39 ms at N = 20,000 -- it would need thousands of steps to pay for itself (tools/time_leaf_steps.py).
    // The bookkeeping is done once behind the loop, unless the loop rebuilds: then a later evaluation can leave early (a refused
    // build) and plan_build_octree orders itself behind `done`, so every evaluation is recorded as it is queued.
    auto queued = [&](bool drifted) {   // the bookkeeping behind evaluations queued on s
        plan_record_evaluation(p, law, signedG, c);
        if (drifted) ctx_bodies_moved(c);
        return plan_mark_done(p, s);
    };
    for (int e = 0; e < nsteps + (kdk ? 1 : 0); ++e) {
        if (rebuilds) {
            int rc = e % rebuild_every == 0 ? plan_build_octree(p, c) : NBX_OK;
            if (!rc) rc = plan_needs_structure(p);
            if (rc) return rc;
        }
        const bool closing = kdk && e == nsteps;            // the closing half-kick: no drift behind it
        const double dt_kick = kdk && (e == 0 || closing) ? 0.5 * dt : dt, dt_drift = closing ? 0.0 : dt;
        if (int rc = plan_enqueue_eval(p, c, law, signedG, dt_kick, dt_drift, !kdk || dt_drift != 0.0, s)) return rc;
        if (rebuilds)
            if (int rc = queued(!closing)) return rc;
    }
    return rebuilds ? NBX_OK : queued(true);
}

int nbx_leaf_plan_step(nbx_leaf_plan* p, nbx_ctx* c, int law, double G, double dt, int nsteps) {
    if (!p || !c) return fail(NBX_ERR_INVALID, "null argument");
    if (law < NBX_LAW_BRUTE || law > NBX_LAW_NEWTON) return fail(NBX_ERR_INVALID, "unknown law");
    if (nsteps < 0) return fail(NBX_ERR_INVALID, "nsteps must be >= 0");
    if (int crc = plan_check_ctx(p, c)) return crc;
    return plan_run_steps(p, c, law, G, dt, nsteps, 0, Scheme::KickDrift);
}

int nbx_leaf_plan_step_kdk(nbx_leaf_plan* p, nbx_ctx* c, int law, double G, double dt, int nsteps) {
    if (!p || !c) return fail(NBX_ERR_INVALID, "null argument");
    if (law < NBX_LAW_BRUTE || law > NBX_LAW_NEWTON) return fail(NBX_ERR_INVALID, "unknown law");
    if (nsteps < 0) return fail(NBX_ERR_INVALID, "nsteps must be >= 0");
    if (int crc = plan_check_ctx(p, c)) return crc;
    return plan_run_steps(p, c, law, G, dt, nsteps, 0, Scheme::KickDriftKick);
}

// what the two octree loops check before plan_run_steps
static int check_octree_steps(const nbx_leaf_plan* p, const nbx_ctx* c, int law, int nsteps, int rebuild_every) {
    if (!p || !c) return fail(NBX_ERR_INVALID, "null argument");
    if (law < NBX_LAW_BRUTE || law > NBX_LAW_NEWTON) return fail(NBX_ERR_INVALID, "unknown law");
    if (nsteps < 0 || rebuild_every < 0) return fail(NBX_ERR_INVALID, "nsteps and rebuild_every must be >= 0");
    if (int rc = plan_check_ctx(p, c)) return rc;
    if (rebuild_every > 0 && !p->octree) return fail(NBX_ERR_STATE, "the plan was not made by nbx_leaf_plan_create_octree");
    return NBX_OK;
}

int nbx_leaf_plan_step_octree(nbx_leaf_plan* p, nbx_ctx* c, int law, double G, double dt, int nsteps, int rebuild_every) {
    if (int rc = check_octree_steps(p, c, law, nsteps, rebuild_every)) return rc;
    return plan_run_steps(p, c, law, G, dt, nsteps, rebuild_every, Scheme::KickDrift);
}

int nbx_leaf_plan_step_octree_kdk(nbx_leaf_plan* p, nbx_ctx* c, int law, double G, double dt, int nsteps, int rebuild_every) {
    if (int rc = check_octree_steps(p, c, law, nsteps, rebuild_every)) return rc;
    return plan_run_steps(p, c, law, G, dt, nsteps, rebuild_every, Scheme::KickDriftKick);
}

// ---- kick-drift-kick with the step chosen on the device (include/nbody_hip.h has the rule; state_kernels.hip the controller) ----
constexpr int kStopLookEvery = 16;   // evaluations between two looks at the clock's `stopped` (the context's close-set look's spacing)

// The step clock's block with room for a call of max_steps steps, and what the loop's looks need.  Growing the block waits for
// the plan's queued work first: an earlier call's kernels may still read the one held.
static int plan_fit_clock(nbx_leaf_plan* p, hipStream_t s, int max_steps) {
    const size_t need = kStepClockHistoryOffset + ((size_t)max_steps + 1) * 2 * sizeof(double);
    if (p->clock_block.bytes() < need) {
        if (p->clock_block) NBX_HIP_TRY(hipStreamSynchronize(s));
        p->clock_valid = false;
        NBX_HIP_TRY(nbx_block::allocate(p->clock_block, p->device, need));
    }
    if (!p->stop_look) NBX_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&p->stop_look), 64, hipHostMallocDefault));
    if (!p->look_done) NBX_HIP_TRY(hipEventCreateWithFlags(&p->look_done, hipEventDisableTiming));
    return NBX_OK;
}

// plan_run_steps' sibling: evaluations 0 .. max_steps, each followed by the reduction, the controller and the clock kick.  The host
// knows neither the steps' sizes nor when the loop stops; what it queues behind the stop changes nothing (the positions stand, so
// the sums come out the same; the controller records nothing and the kick is not applied).  It stops queueing once a look has
// shown it the stop: before every rebuild after the first (the build reads back right behind it, so that wait costs nothing, and a
// structure built behind the stop would not be the one the last kick was made on), and, without rebuilds, by a copy every
// kStopLookEvery evaluations that is polled, never waited for.
static int plan_run_adaptive(nbx_leaf_plan* p, nbx_ctx* c, int law, double G, const nbx_step_control& k, int max_steps, int rebuild_every) {
    if (max_steps == 0) return NBX_OK;
    const bool rebuilds = rebuild_every > 0;
    if (!rebuilds)
        if (int src = plan_needs_structure(p)) return src;
    if (int lrc = plan_check_law(p, law, c->mass_max)) return lrc;
    hipStream_t s = c->stream;
    PlanScope in(p, s);
    if (in.rc) return in.rc;
    if (int rc = plan_fit_clock(p, s, max_steps)) return rc;
    StepClock* const clock = p->clock_block.as<StepClock>();
    const double signedG = signed_G(law, G);
    NBX_HIP_TRY(launch_step_clock_init(clock, k.accel_length, k.dt_min, k.dt_max, k.t_start, k.t_end, k.pow2, (uint32_t)max_steps + 1u, s));
    p->clock_valid = true;
    auto queued = [&]() {
        plan_record_evaluation(p, law, signedG, c);
        ctx_bodies_moved(c);
        return plan_mark_done(p, s);
    };
    bool look_in_flight = false;
    for (int e = 0; e <= max_steps; ++e) {
        if (rebuilds) {
            int rc = NBX_OK;
            if (e % rebuild_every == 0) {
                if (e > 0) {
                    NBX_HIP_TRY(hipMemcpyAsync(p->stop_look, &clock->stopped, sizeof(int), hipMemcpyDeviceToHost, s));
                    NBX_HIP_TRY(hipStreamSynchronize(s));
                    if (*p->stop_look) break;
                }
                rc = plan_build_octree(p, c);
            }
            if (!rc) rc = plan_needs_structure(p);
            if (rc) return rc;
        } else if (e > 0 && e % kStopLookEvery == 0) {
            if (look_in_flight && hipEventQuery(p->look_done) == hipSuccess) {
                look_in_flight = false;
                if (*p->stop_look) break;
            }
            (void)hipGetLastError();                        // hipErrorNotReady of the query is no failure
            if (!look_in_flight) {
                NBX_HIP_TRY(hipMemcpyAsync(p->stop_look, &clock->stopped, sizeof(int), hipMemcpyDeviceToHost, s));
                NBX_HIP_TRY(hipEventRecord(p->look_done, s));
                look_in_flight = true;
            }
        }
        NBX_HIP_TRY(hipMemsetAsync(p->max_mass, 0, sizeof(uint32_t), s));
        if (int rc = plan_gather_resident(p, c, s)) return rc;
        if (int rc = plan_launch_pairs(p, law, s, false)) return rc;
        NBX_HIP_TRY(launch_step_controller(p->sums, p->pslot_body, (uint32_t)p->pslots, p->dim, std::fabs(signedG), clock, e == max_steps, s));
        NBX_HIP_TRY(launch_kick_drift_slots_clock(slot_kick_args(p, c, signedG, 0.0, 0.0, true), clock, s));
        if (rebuilds)
            if (int rc = queued()) return rc;
    }
    return queued();
}

int nbx_leaf_plan_step_kdk_adaptive(nbx_leaf_plan* p, nbx_ctx* c, int law, double G, const nbx_step_control* control, int max_steps,
                                    int rebuild_every) {
    // what needs no device first: the control, the law, the counts, then the two handles
    if (!control) return fail(NBX_ERR_INVALID, "null argument");
    if (const char* why = step_control_fault(control)) return fail(NBX_ERR_INVALID, why);
    if (law < NBX_LAW_BRUTE || law > NBX_LAW_NEWTON) return fail(NBX_ERR_INVALID, "unknown law");
    if (max_steps < 0 || max_steps > (1 << 20)) return fail(NBX_ERR_INVALID, "max_steps must be in [0, 1 << 20]");
    if (rebuild_every < 0) return fail(NBX_ERR_INVALID, "rebuild_every must be >= 0");
    if (!p || !c) return fail(NBX_ERR_INVALID, "null argument");
    if (int rc = plan_check_ctx(p, c)) return rc;
    if (rebuild_every > 0 && !p->octree) return fail(NBX_ERR_STATE, "the plan was not made by nbx_leaf_plan_create_octree");
    return plan_run_adaptive(p, c, law, G, *control, max_steps, rebuild_every);
}

// the clock's record, read back on the plan's own stream behind the last queued work
static int plan_read_clock(nbx_leaf_plan* p, StepClock* host) {
    NBX_HIP_TRY(hipMemcpyAsync(host, p->clock_block.get(), sizeof(StepClock), hipMemcpyDeviceToHost, p->stream));
    NBX_HIP_TRY(hipStreamSynchronize(p->stream));
    return NBX_OK;
}

int nbx_leaf_plan_get_step_clock(nbx_leaf_plan* p, nbx_step_clock* out) {
    if (!p || !out) return fail(NBX_ERR_INVALID, "null argument");
    if (!p->clock_valid) return fail(NBX_ERR_STATE, "no adaptive call on this plan yet (nbx_leaf_plan_step_kdk_adaptive)");
    PlanScope in(p, p->stream);
    if (in.rc) return in.rc;
    StepClock k;
    if (int rc = plan_read_clock(p, &k)) return rc;
    out->t = k.t; out->dt_last = k.prev; out->a_max_last = k.a_max_last;
    out->steps = k.steps; out->evaluations = k.evaluations;
    out->finished = k.finished; out->status = k.status;
    return plan_mark_done(p, p->stream);
}

int nbx_leaf_plan_get_step_history(nbx_leaf_plan* p, double* a_max_out, double* dt_out, size_t capacity, size_t* count) {
    if (!p || !count) return fail(NBX_ERR_INVALID, "null argument");
    if (!p->clock_valid) return fail(NBX_ERR_STATE, "no adaptive call on this plan yet (nbx_leaf_plan_step_kdk_adaptive)");
    PlanScope in(p, p->stream);
    if (in.rc) return in.rc;
    StepClock k;
    if (int rc = plan_read_clock(p, &k)) return rc;
    *count = k.recorded;
    const size_t take = capacity < (size_t)k.recorded ? capacity : (size_t)k.recorded;
    if (take && (a_max_out || dt_out)) {
        std::vector<double> pairs;
        try { pairs.resize(2 * take); } catch (...) { return fail(NBX_ERR_ALLOC, "host allocation failed"); }
        NBX_HIP_TRY(hipMemcpyAsync(pairs.data(), p->clock_block.get() + kStepClockHistoryOffset, 2 * take * sizeof(double), hipMemcpyDeviceToHost, p->stream));
        NBX_HIP_TRY(hipStreamSynchronize(p->stream));
        for (size_t i = 0; i < take; ++i) {
            if (a_max_out) a_max_out[i] = pairs[2 * i];
            if (dt_out) dt_out[i] = pairs[2 * i + 1];
        }
    }
    return plan_mark_done(p, p->stream);
}

// An observer like the potential calls: it reads the slot sums and the inverse map and writes its own 8-byte word.
int nbx_leaf_plan_max_accel(nbx_leaf_plan* p, double* a_max) {
    if (!p || !a_max) return fail(NBX_ERR_INVALID, "null argument");
    if (!p->evaluated) return fail(NBX_ERR_STATE, "no evaluation on the device");
    if (p->last_ctx_id && !nbx::ctx_alive(p->last_ctx_id))
        return fail(NBX_ERR_STATE, "the context of the last evaluation no longer exists: evaluate again before asking for the largest acceleration");
    PlanScope in(p, p->stream);   // the plan's own stream, behind the last evaluation's event (nbx_leaf_plan_get_forces)
    if (in.rc) return in.rc;
    if (!p->amax_block) NBX_HIP_TRY(nbx_block::allocate(p->amax_block, p->device, 256));
    unsigned long long bits = 0ull;
    NBX_HIP_TRY(launch_slot_accel_max(p->sums, p->body_slot, (uint32_t)p->pslots, p->dim, p->n, std::fabs(p->last_signedG),
                                      p->amax_block.as<unsigned long long>(), p->stream));
    NBX_HIP_TRY(hipMemcpyAsync(&bits, p->amax_block.get(), sizeof bits, hipMemcpyDeviceToHost, p->stream));
    NBX_HIP_TRY(hipStreamSynchronize(p->stream));
    std::memcpy(a_max, &bits, sizeof bits);
    return plan_mark_done(p, p->stream);
}

int nbx_leaf_plan_set_cells(nbx_leaf_plan* p, const uint32_t* cell_first_leaf, const uint32_t* cell_leaf_count, size_t n_cells,
                            const uint32_t* far_offsets, const uint32_t* far_cells) {
    if (!p) return fail(NBX_ERR_INVALID, "plan is null");
    if (int src = plan_needs_structure(p)) return src;
    // every index the two passes will follow, before anything is launched; a refused call leaves the plan and its cells as they were
    if (const char* why = nbx_far::validate_cells(p->n_leaves, cell_first_leaf, cell_leaf_count, n_cells, far_offsets, far_cells))
        return fail(NBX_ERR_INVALID, why);
    hipStream_t s = p->stream;   // the plan's own stream, behind the last evaluation wherever that was queued
    PlanScope in(p, s);
    if (in.rc) return in.rc;
    if (!n_cells) {
        NBX_HIP_TRY(hipStreamSynchronize(s));
        plan_release_cells(p, true, false);
        return plan_mark_done(p, s);
    }
    nbx_far::FarPlan fp;
    std::vector<uint32_t> read_back;
    const uint32_t* unit = p->unit_host.data();
    if (p->unit_host.size() != p->n_leaves + 1) {      // laid out on the device: the array comes back once per set_cells (4 B per leaf)
        try { read_back.assign(p->n_leaves + 1, 0u); } catch (...) { return fail(NBX_ERR_ALLOC, "host allocation failed"); }
        if (p->n_leaves) {
            NBX_HIP_TRY(hipMemcpyAsync(read_back.data(), p->unit_off, (p->n_leaves + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            NBX_HIP_TRY(hipStreamSynchronize(s));
        }
        unit = read_back.data();
    }
    try { nbx_far::plan_far(unit, p->n_leaves, cell_leaf_count, n_cells, far_offsets, fp); } catch (...) { return fail(NBX_ERR_ALLOC, "host allocation failed"); }
    const size_t dim = (size_t)p->dim;
    const size_t sizes[10] = {n_cells * 4, n_cells * 4, fp.small_cells.size() * 4, fp.big_cells.size() * 4, fp.far_entries * 4,
                              fp.blocks.size() * sizeof(nbx_far::FarBlock), p->n_leaves * 4 * sizeof(double), n_cells * sizeof(double),
                              n_cells * dim * sizeof(double), n_cells * sizeof(float4)};
    const auto cut = carve(sizes);
    Block cells;                                        // freed if the upload fails: the copies may be under way
    NBX_HIP_TRY(nbx_block::take(cells, leaf_pool(), p->device, cut.total));
    char* const arena = cells.get();
    hipError_t e = hipSuccess;
    for (hipEvent_t* ev : {&p->evm0, &p->evm1, &p->evf0, &p->evf1})
        if (!*ev && e == hipSuccess) e = hipEventCreate(ev);
    const void* const src[6] = {cell_first_leaf, cell_leaf_count, fp.small_cells.data(), fp.big_cells.data(), far_cells, fp.blocks.data()};
    for (int i = 0; i < 6 && e == hipSuccess; ++i)
        if (sizes[i]) e = hipMemcpyAsync(arena + cut.off[i], src[i], sizes[i], hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // the caller's arrays and the layout's are copied; the last evaluation is over too
    if (e != hipSuccess) return nbx::fail_hip(e, "uploading the cells", __FILE__, __LINE__);
    plan_release_cells(p, true, false);                 // the previous cells, if any: nothing on the device uses them any more
    p->cell_arena = std::move(cells);
    nbx_far::FarDevice& d = p->far;
    d.xp = p->xp; d.unit_off = p->unit_off; d.sums = p->sums;
    d.pslots = (uint32_t)p->pslots; d.n_leaves = (uint32_t)p->n_leaves; d.n_cells = (uint32_t)n_cells;
    d.n_small = (uint32_t)fp.small_cells.size(); d.n_big = (uint32_t)fp.big_cells.size(); d.n_blocks = (uint32_t)fp.blocks.size();
    d.cell_first = cut.at<uint32_t>(arena, 0);
    d.cell_count = cut.at<uint32_t>(arena, 1);
    d.small_cells = cut.at<uint32_t>(arena, 2);
    d.big_cells = cut.at<uint32_t>(arena, 3);
    d.far_cells = cut.at<uint32_t>(arena, 4);
    d.blocks = cut.at<nbx_far::FarBlock>(arena, 5);
    d.leaf_mom = cut.at<double>(arena, 6);
    d.cell_mass = cut.at<double>(arena, 7);
    d.cell_com = cut.at<double>(arena, 8);
    d.cell_rec = cut.at<float4>(arena, 9);
    p->far_entries = fp.far_entries;
    if (int rc = plan_fit_quads(p)) { plan_release_cells(p, true, false); return rc; }   // the plan's order holds for the new cells
    return plan_mark_done(p, s);
}

int nbx_leaf_plan_set_far_order(nbx_leaf_plan* p, int order) {
    if (!p) return fail(NBX_ERR_INVALID, "plan is null");
    if (order != NBX_FAR_MONOPOLE && order != NBX_FAR_QUADRUPOLE) return fail(NBX_ERR_INVALID, "order must be NBX_FAR_MONOPOLE or NBX_FAR_QUADRUPOLE");
    hipStream_t s = p->stream;
    PlanScope in(p, s);
    if (in.rc) return in.rc;
    NBX_HIP_TRY(hipStreamSynchronize(s));               // the last evaluation is over: nothing reads the cells' records any more
    if (order == p->far_order) return plan_mark_done(p, s);
    const int before = p->far_order;
    p->far_order = order;
    if (int rc = plan_fit_quads(p)) { p->far_order = before; (void)plan_fit_quads(p); return rc; }
    return plan_mark_done(p, s);
}

int nbx_leaf_plan_get_far_order(const nbx_leaf_plan* p, int* order) {
    if (!p) return fail(NBX_ERR_INVALID, "plan is null");
    if (!order) return fail(NBX_ERR_INVALID, "order is null");
    *order = p->far_order;
    return NBX_OK;
}

int nbx_leaf_plan_set_softening(nbx_leaf_plan* p, double epsilon) {
    if (!p) return fail(NBX_ERR_INVALID, "plan is null");
    if (!(epsilon == 0.0 || (epsilon >= 1.0e-6 && epsilon <= 1.0e15))) return fail(NBX_ERR_INVALID, "softening must be 0 or in [1e-6, 1e15]");
    hipStream_t s = p->stream;
    PlanScope in(p, s);
    if (in.rc) return in.rc;
    NBX_HIP_TRY(hipStreamSynchronize(s));               // the last evaluation is over (its launches carry their own copy of eps^2 anyway)
    p->softening = epsilon;
    return plan_mark_done(p, s);
}

int nbx_leaf_plan_get_softening(const nbx_leaf_plan* p, double* epsilon) {
    if (!p) return fail(NBX_ERR_INVALID, "plan is null");
    if (!epsilon) return fail(NBX_ERR_INVALID, "epsilon is null");
    *epsilon = p->softening;
    return NBX_OK;
}

int nbx_leaf_plan_get_cell_quadrupoles(nbx_leaf_plan* p, double* q_out) {
    if (!p) return fail(NBX_ERR_INVALID, "plan is null");
    if (p->far_order != NBX_FAR_QUADRUPOLE) return fail(NBX_ERR_STATE, "the plan's far order is NBX_FAR_MONOPOLE: no second moments are computed");
    if (!p->far.n_cells) return NBX_OK;
    if (!p->cells_evaluated || !p->quads_evaluated) return fail(NBX_ERR_STATE, "no evaluation at NBX_FAR_QUADRUPOLE since the cells were set");
    if (!q_out) return fail(NBX_ERR_INVALID, "q_out is null");
    hipStream_t s = p->stream;
    PlanScope in(p, s);
    if (in.rc) return in.rc;
    NBX_HIP_TRY(hipMemcpyAsync(q_out, p->far.cell_quad, (size_t)p->far.n_cells * nbx_far::quad_count(p->dim) * sizeof(double), hipMemcpyDeviceToHost, s));
    NBX_HIP_TRY(hipStreamSynchronize(s));
    return plan_mark_done(p, s);
}

int nbx_leaf_plan_get_cells(nbx_leaf_plan* p, double* mass_out, double* com_out) {
    if (!p) return fail(NBX_ERR_INVALID, "plan is null");
    if (!p->far.n_cells) return NBX_OK;
    if (!p->cells_evaluated) return fail(NBX_ERR_STATE, "no evaluation since the cells were set");
    hipStream_t s = p->stream;
    PlanScope in(p, s);
    if (in.rc) return in.rc;
    const size_t nc = p->far.n_cells;
    if (mass_out) NBX_HIP_TRY(hipMemcpyAsync(mass_out, p->far.cell_mass, nc * sizeof(double), hipMemcpyDeviceToHost, s));
    if (com_out) NBX_HIP_TRY(hipMemcpyAsync(com_out, p->far.cell_com, nc * (size_t)p->dim * sizeof(double), hipMemcpyDeviceToHost, s));
    NBX_HIP_TRY(hipStreamSynchronize(s));
    return plan_mark_done(p, s);
}

int nbx_leaf_plan_cell_info(nbx_leaf_plan* p, size_t* n_cells, size_t* far_entries, float* moments_ms, float* far_ms) {
    if (moments_ms) *moments_ms = 0.0f;
    if (far_ms) *far_ms = 0.0f;
    if (!p) return fail(NBX_ERR_INVALID, "plan is null");
    if (n_cells) *n_cells = p->far.n_cells;
    if (far_entries) *far_entries = p->far_entries;
    if ((moments_ms || far_ms) && p->far.n_cells && p->cells_evaluated && p->cells_timed) {
        DeviceScope scope;
        int rc = plan_set_device(p);
        if (rc) return rc;
        NBX_HIP_TRY(hipEventSynchronize(p->evf1));
        if (moments_ms) NBX_HIP_TRY(hipEventElapsedTime(moments_ms, p->evm0, p->evm1));
        if (far_ms) NBX_HIP_TRY(hipEventElapsedTime(far_ms, p->evf0, p->evf1));
    }
    return NBX_OK;
}

int nbx_leaf_plan_time_kernel(nbx_leaf_plan* p, int law, int reps, float* mean_ms) {
    if (!p || !mean_ms) return fail(NBX_ERR_INVALID, "null argument");
    *mean_ms = 0.0f;
    if (law < NBX_LAW_BRUTE || law > NBX_LAW_NEWTON) return fail(NBX_ERR_INVALID, "unknown law");
    if (reps < 1 || reps > 1000) return fail(NBX_ERR_INVALID, "reps must be in [1, 1000]");
    if (!p->evaluated) return fail(NBX_ERR_STATE, "evaluate once before timing (the bodies of the last evaluation are used)");
    if (int lrc = plan_check_law(p, law, -1.0)) return lrc;      // the softening length; the masses below
    hipStream_t s = p->stream;   // the plan's own stream, behind the last evaluation (see nbx_leaf_plan_get_forces)
    PlanScope in(p, s);
    if (in.rc) return in.rc;
    if (law == NBX_LAW_NEWTON) {   // the largest |mass| of the bodies the launches will read: the word the last gather left (fp32 bits)
        float mass_max = 0.0f;
        NBX_HIP_TRY(hipMemcpyAsync(&mass_max, p->max_mass, sizeof(float), hipMemcpyDeviceToHost, s));
        NBX_HIP_TRY(hipStreamSynchronize(s));
        if (int lrc = plan_check_law(p, law, (double)mass_max)) return lrc;
    }
    const int timed_from = reps / 2;
    for (int r = 0; r < reps; ++r) {
        if (r == timed_from) NBX_HIP_TRY(hipEventRecord(p->ev0, s));
        if (int rc = plan_launch_near(p, law, s, false)) return rc;
    }
    NBX_HIP_TRY(hipEventRecord(p->ev1, s));
    if (p->cells_evaluated)   // the sums keep their far terms (the last evaluation's moments)
        if (int rc = plan_launch_far(p, law, s, false, false)) return rc;
    NBX_HIP_TRY(hipStreamSynchronize(s));
    if (p->n_blocks || p->n_packs) NBX_HIP_TRY(hipEventElapsedTime(mean_ms, p->ev0, p->ev1));
    *mean_ms /= (float)(reps - timed_from);
    // the sums now belong to `law`: keep the bookkeeping of the last evaluation consistent with them
    p->last_signedG = signed_G(law, std::fabs(p->last_signedG));
    p->last_law = law;
    return plan_mark_done(p, s);
}

// ---- the potential (leaf_phi.h) -------------------------------------------------------------------------------------------------
// A potential call is an OBSERVER: it writes the plan's source pairs, the largest-mass word and the cells' moments (which every
// evaluation writes afresh), the plan's phi block, and nothing else -- not the slot sums, not the record of the last evaluation.
static int phi_check_law(int law) {
    if (law == NBX_LAW_FMM_P2P) return fail(NBX_ERR_INVALID, "NBX_LAW_FMM_P2P has no potential: its smoothed magnitude with unsmoothed direction is no gradient");
    if (law != NBX_LAW_BRUTE && law != NBX_LAW_TREE_LEAF && law != NBX_LAW_NEWTON) return fail(NBX_ERR_INVALID, "unknown law");
    return NBX_OK;
}

// The phi block for the structure as it stands.  Nothing on the device uses the block: every potential call ends synchronised.
static int plan_fit_phi(nbx_leaf_plan* p) {
    p->phi_valid = false;
    const size_t nblk = (p->n + 255) / 256;
    const size_t sizes[3] = {p->pslots * sizeof(double), p->n * sizeof(double), 2 * nblk * sizeof(double)};
    const auto cut = carve(sizes);
    NBX_HIP_TRY(nbx_block::fit(p->phi_block, leaf_pool(), p->device, cut.total));
    char* const base = p->phi_block.get();
    p->phi_slot = cut.at<double>(base, 0);
    p->phi_body = cut.at<double>(base, 1);
    p->phi_part = cut.at<double>(base, 2);
    return NBX_OK;
}

// behind the gather on s: moments (if the plan has cells), near + far potential, phi by body
static int plan_launch_phi(nbx_leaf_plan* p, int law, hipStream_t s) {
    if (p->far.n_cells) {
        NBX_HIP_TRY(nbx_far::enqueue_moments(p->far, p->dim, s));
        p->cells_evaluated = true;                          // the cells' records now belong to the positions just gathered
        p->quads_evaluated = p->far.order == NBX_FAR_QUADRUPOLE;
    }
    NBX_HIP_TRY(hipMemsetAsync(p->phi_slot, 0, p->pslots ? p->pslots * sizeof(double) : 8, s));
    nbx_phi::PhiDevice d;
    d.xp = p->xp; d.pslots = (uint32_t)p->pslots; d.ops = p->ops; d.blocks = p->blocks; d.subs = p->subs;
    d.n_blocks = (uint32_t)p->n_blocks; d.n_subs = (uint32_t)p->n_subs; d.phi = p->phi_slot; d.eps2 = plan_eps2(p);
    NBX_HIP_TRY(nbx_phi::enqueue_near_phi(d, p->dim, law, s));
    nbx_far::FarDevice f = p->far;
    f.eps2 = plan_eps2(p);
    NBX_HIP_TRY(nbx_phi::enqueue_far_phi(f, p->phi_slot, p->dim, law, s));
    NBX_HIP_TRY(nbx_phi::enqueue_phi_by_body(p->phi_slot, p->body_slot, p->n, law == NBX_LAW_NEWTON ? 1.0 : 0.5, p->phi_body, s));
    return NBX_OK;
}

int nbx_leaf_plan_potentials(nbx_leaf_plan* p, const void* bodies, size_t stride_bytes, int law, double* phi_out) {
    if (!p) return fail(NBX_ERR_INVALID, "plan is null");
    if (int lrc = phi_check_law(law)) return lrc;
    if ((!bodies || !phi_out) && p->n) return fail(NBX_ERR_INVALID, "null argument");
    const size_t min_stride = (size_t)(2 * p->dim + 1) * sizeof(double);
    if (stride_bytes < min_stride || stride_bytes % sizeof(double) != 0)
        return fail(NBX_ERR_INVALID, "body stride must be a multiple of 8 and >= sizeof(Body<dim>)");
    if (int src = plan_needs_structure(p)) return src;
    if (int lrc = plan_check_law_staged(p, law, bodies, stride_bytes)) return lrc;
    hipStream_t s = p->stream;
    PlanScope in(p, s);
    if (in.rc) return in.rc;
    if (int rc = plan_fit_phi(p)) return rc;
    const size_t bytes = p->n * stride_bytes;
    if (bytes && bytes + 256 > p->phi_raw.bytes()) NBX_HIP_TRY(nbx_block::allocate(p->phi_raw, p->device, bytes + 256));
    if (bytes) NBX_HIP_TRY(hipMemcpyAsync(p->phi_raw.get(), bodies, bytes, hipMemcpyHostToDevice, s));
    NBX_HIP_TRY(hipMemsetAsync(p->max_mass, 0, sizeof(uint32_t), s));
    if (p->pslots)
        NBX_HIP_TRY(nbx_near::enqueue_gather_staged(p->phi_raw.as<double>(), stride_bytes / sizeof(double), p->dim, p->pslot_body, p->pslots, p->xp, p->max_mass, s));
    if (int rc = plan_launch_phi(p, law, s)) return rc;
    if (p->n) NBX_HIP_TRY(hipMemcpyAsync(phi_out, p->phi_body, p->n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (int rc = plan_mark_done(p, s)) return rc;
    NBX_HIP_TRY(hipStreamSynchronize(s));
    p->phi_valid = true;
    return NBX_OK;
}

int nbx_leaf_plan_energy(nbx_leaf_plan* p, nbx_ctx* c, int law, double G, double* kinetic, double* potential) {
    if (!p || !c) return fail(NBX_ERR_INVALID, "null argument");
    if (int lrc = phi_check_law(law)) return lrc;
    if (int crc = plan_check_ctx(p, c)) return crc;
    if (int src = plan_needs_structure(p)) return src;
    if (int lrc = plan_check_law(p, law, c->mass_max)) return lrc;
    const size_t nblk = (p->n + 255) / 256;
    std::vector<double> host;
    try { host.resize(2 * nblk); } catch (...) { return fail(NBX_ERR_ALLOC, "host allocation failed"); }
    hipStream_t s = c->stream;
    PlanScope in(p, s);
    if (in.rc) return in.rc;
    if (int rc = plan_fit_phi(p)) return rc;
    NBX_HIP_TRY(hipMemsetAsync(p->max_mass, 0, sizeof(uint32_t), s));
    if (int rc = plan_gather_resident(p, c, s)) return rc;
    if (int rc = plan_launch_phi(p, law, s)) return rc;
    NBX_HIP_TRY(nbx_phi::enqueue_energy_partials(p->phi_body, p->n, p->dim, c->pad, c->v64, c->m64, p->phi_part, s));
    if (nblk) NBX_HIP_TRY(hipMemcpyAsync(host.data(), p->phi_part, 2 * nblk * sizeof(double), hipMemcpyDeviceToHost, s));
    if (int rc = plan_mark_done(p, s)) return rc;
    NBX_HIP_TRY(hipStreamSynchronize(s));
    p->phi_valid = true;
    long double mv2 = 0.0L, mphi = 0.0L;                    // workgroup order over the device's per-workgroup sums: a fixed tree
    for (size_t l = 0; l < nblk; ++l) { mv2 += host[l]; mphi += host[nblk + l]; }
    if (kinetic) *kinetic = 0.5 * (double)mv2;
    if (potential) *potential = (law == NBX_LAW_BRUTE ? 0.5 : -0.5) * G * (double)mphi;   // U = s (G / 2) sum_i m_i phi_i
    return NBX_OK;
}

int nbx_leaf_plan_get_potentials(nbx_leaf_plan* p, double* phi_out) {
    if (!p || (!phi_out && p->n)) return fail(NBX_ERR_INVALID, "null argument");
    if (!p->phi_valid) return fail(NBX_ERR_STATE, "no potential call on this plan yet (nbx_leaf_plan_energy / nbx_leaf_plan_potentials)");
    PlanScope in(p, p->stream);
    if (in.rc) return in.rc;
    if (p->n) NBX_HIP_TRY(hipMemcpyAsync(phi_out, p->phi_body, p->n * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    NBX_HIP_TRY(hipStreamSynchronize(p->stream));
    return plan_mark_done(p, p->stream);
}

}  // extern "C"
