// nbx_internal.h -- shared between the HIP translation units of libnbody_hip.so (not installed).
#ifndef NBX_INTERNAL_H
#define NBX_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace nbx {

// Source tile = bodies staged per LDS fill (BASELINE config 2: "LDS tile=256") = workgroup size.
constexpr int kTile = 256;
// Shard arrays are padded to a multiple of this many bodies so that every force-kernel variant
// (up to 16 targets per lane x 256 lanes) sees whole target blocks and whole source tiles.
constexpr int kPadQuantum = 4096;

// Smallest fp32 that is >= the reference's fp64 skip threshold 1e-10 (methods.cpp:24): for any fp32
// r2, (r2 < kR2SkipF) == ((double)r2 < 1e-10).   0x2edbe6ff = 1.00000001335e-10f.
constexpr float kR2SkipF = 1.0e-10f;
static_assert((double)kR2SkipF >= 1e-10, "fp32 threshold must not round below the fp64 one");
constexpr double kR2Skip64 = 1.0e-10;   // the same threshold for the strict fp64 kernel, compared as the reference compares it

// ---- close-pair bookkeeping of the fast force path (force_kernel.hip) --------------------------------
// The fast kernel carries no per-pair guard: it biases r^2 by kTiny = 2^-47 so that coincident bodies
// (d = 0) contribute exactly 0 and 1/r^2 stays finite.  That reproduces the reference for a target unless
// it has a source with 0 < r^2 < X, where X = max(1e-10 [the reference's skip threshold, methods.cpp:24],
// 2^25 * kTiny = 2.4e-7 [below this the bias moves r^2 by more than half a unit roundoff]) = 2.4e-7.
// Targets that might own such a pair are found exactly, once per position update, in two cheap steps:
//  1. candidates.  Two DISTINCT fp32 coordinates a, b of equal sign differ by at least the fp32 spacing at
//     min(|a|,|b|) (opposite signs: by |a|+|b|).  A pair with 0 < r^2 < 2.4e-7 has some |d_k| in (0, 4.9e-4),
//     hence min(|a_k|,|b_k|) < 2^13 and max < 2^13 + 4.9e-4: BOTH members have a coordinate of magnitude below
//     kCloseCoord = 2^14 (twice what the argument needs).  classify_close_kernel lists the shard's targets with
//     any |coordinate| < kCloseCoord (0.5 % of the reference's uniform bodies).  Conversely a non-candidate
//     differs from every other body, in each coordinate where they differ, by >= 2^-10, so its non-zero r^2
//     are >= 9.5e-7: never skipped by the reference and biased by < 1e-8 relative.
//  2. The same argument holds for the SOURCE member of such a pair, whichever chunk (shard) it lives in, so
//     classify_sources_kernel lists the candidate sources of the pass being launched -- every real body of
//     the pass's chunk list (ALL / LOCAL / REMOTE) with a coordinate below kCloseCoord, read from the exchange
//     buffer as it stands when the pass runs (for REMOTE: after the all-gather) -- and refine_close_kernel
//     checks the shard's candidate targets against that list (all-pairs over two small lists, the same fp32
//     r^2) and keeps the targets with a partner at 0 < r^2 < kBadR2 = 1e-6 (4x the X above) -- almost
//     always none.  Above kRefineLimit candidate targets (or kRefinePairLimit checks) it keeps them all.
//     A pair that straddles a shard boundary is therefore found by the pass that evaluates it.
// Bad targets of a pass are flagged (the fast kernel does not store them) and evaluated against that pass's
// sources with the exact compare-and-select guard by extra workgroups of the same launch (close_set_path),
// then scattered into acc.  The result therefore has the reference's skip semantics for every pair.
constexpr float kTiny = 0x1p-47f;          // 7.1e-15
constexpr float kCloseCoord = 16384.0f;
constexpr float kBadR2 = 1.0e-6f;
constexpr unsigned kRefineLimit = 131072;  // candidate targets beyond this are all treated as bad (O(n^2) check avoided)
constexpr unsigned long long kRefinePairLimit = 1ull << 36;  // same for (candidate targets) x (candidate sources)
// m / (kTiny^2) must stay finite in fp32 for a coincident source: masses above this force the exact path.
constexpr double kFastMaxMass = 1.0e10;
// One-reciprocal fast variant: W = 1/(r2a*r2b) must stay finite.  With every |coordinate| <= X, r^2 <= 12 X^2 and
// the product <= 144 X^4; X = 1e9 would still fit (1.4e38), 1e8 leaves a 10x margin for bodies that drift after
// the upload-time check.  Violations fall back to the two-reciprocal fast kernel (same results to ~2 ulp).
constexpr double kOneRcpMaxCoord = 1.0e8;
constexpr int kCloseBlocksX = 32;          // extra workgroups per source slice that a fast launch adds for bad targets

// Workspace of the sorted-cell form of the close-set refinement (close_hash.hip); all null when not in use.
struct HashWork {
    unsigned* keys = nullptr;          // [capacity] 32-bit cell keys of the pass's candidate sources; sorted in place (four passes, two buffers)
    unsigned* keys_alt = nullptr;      // [capacity] the radix sort's second buffer
    unsigned* vals = nullptr;          // [capacity] slot in src_cand_pos, carried along
    unsigned* vals_alt = nullptr;
    void* temp = nullptr;              // per-tile digit histograms of the radix sort
    size_t temp_bytes = 0;
    unsigned capacity = 0;             // = n_chunks * pad (every body may be a candidate)
};

// How one force evaluation walks the exchange buffer  pos_all[n_shards][dim][pad] / mass_all[n_shards][pad].
struct AccelLaunch {
    const float* pos_all;
    const float* mass_all;
    float* acc;          // [splits][dim][pad] partial accelerations of the target shard
    unsigned pad;        // bodies per chunk (multiple of kPadQuantum)
    unsigned count;      // real targets in the shard (<= pad)
    int tgt_chunk;       // chunk whose bodies are the targets
    int chunk_first;     // first real chunk of the virtual source list
    int vchunks;         // number of chunks in the virtual source list
    int chunk_skip;      // real chunk left out of the list (INT_MAX: none)
    int splits;          // gridDim.y: slices of the virtual tile list
    int accumulate;      // 0: acc = result, 1: acc += result
    int variant;         // force-kernel variant id
    // workspace of the fast path (may be null for exact variants)
    unsigned* cand_list;      // [pad] candidate target indices
    float* cand_pos;          // [dim][pad] their positions, compacted
    unsigned* bad_list;       // [pad] targets that own a pair with 0 < r^2 < kBadR2
    unsigned* bad_flag;  // [pad] 1 for listed targets
    unsigned* counters;       // [0] = candidate targets, [1] = bad targets, [2] = candidate sources
    float* close_acc;         // [splits][dim][pad]
    float* src_cand_pos;      // [dim][n_shards*pad] positions of the pass's candidate sources, compacted
    size_t n_total;           // real bodies over all chunks
    size_t shard_len;         // real bodies per chunk (the last non-empty chunk may hold fewer)
    int n_chunks;             // chunks in the exchange buffer (= n_shards)
    int pass;                 // NBX_SRC_* selector of this launch (cache key of the bad-target list)
    int cacheable;            // the pass's sources change only through this context (single shard, or LOCAL)
    int* tgt_cand_valid;      // host flag owned by the context: cand_list matches the own chunk's positions
    int* bad_list_pass;       // host flag owned by the context: pass whose bad list is current (-1: none)
    float eps2;               // > 0: softened law (fast variants only; no close-set pipeline)
    int law;                  // 0: the reference's r^-4 d law, 1: Newtonian r^-3 d (needs eps2 > 0)
    HashWork hash;            // non-null: refine through sorted cells instead of candidates x candidates
    int lists_only;           // 1: build the close-set lists and return (upload-time probe of the bad-target count)
    // mixed mode (nbx_ctx_set_refine; see RefineLaunch): non-null = the fast kernel also writes, per slice and target, the sum
    // over the slice's tiles of |tile partial sum|^2  -- [grid slices][pad]
    float* qsum = nullptr;
    // optional: recorded on the stream immediately before / after the main force kernel
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    // measurement (nbx_ctx_enable_clock_stamps): non-null = every workgroup of the three-level force kernel stamps the shader
    // clock and the 100 MHz reference clock around its work -- [2 x workgroups of the launch] {d s_memtime, d s_memrealtime}
    unsigned long long* clk = nullptr;
    unsigned* clk_slots = nullptr;   // host: receives the number of workgroups of the stamped launch
};

// Kernel-side view of one force launch (built by launch_accel from an AccelLaunch).
struct KArgs {
    const float* __restrict__ pos_all;
    const float* __restrict__ mass_all;
    float* __restrict__ acc;
    unsigned pad;
    unsigned count;
    unsigned tiles_per_chunk;
    unsigned total_tiles;      // vchunks * tiles_per_chunk
    unsigned tiles_per_split;
    int tgt_chunk, chunk_first, chunk_skip;
    int accumulate;
    int splits;                // fp32 planes of acc (= grid slices x planes per slice)
    int grid_slices;           // source slices of the launch = planes of close_acc and of qsum
    unsigned close_blocks;     // fast kernels: workgroups with blockIdx.x < close_blocks run close_set_path
    unsigned* __restrict__ cand_list;
    float* __restrict__ cand_pos;
    unsigned* __restrict__ bad_list;
    unsigned* __restrict__ bad_flag;
    unsigned* __restrict__ counters;
    float* __restrict__ close_acc;
    float* __restrict__ src_cand_pos;
    unsigned src_stride;       // floats between the coordinate planes of src_cand_pos (= n_chunks * pad)
    unsigned n_total, shard_len;
    float eps2;                // softened law: epsilon^2 (0: the reference law)
    // mixed mode / strict kernel with listed targets
    float* __restrict__ qsum;          // [grid slices][pad] or null
    unsigned* __restrict__ strict_list;   // [strict_cap] targets to re-evaluate in fp64; their number is counters[3]
    double* __restrict__ strict_acc;   // [slices][dim][stride] with slices and stride chosen ON THE DEVICE from the list's length (strict_layout)
    unsigned strict_cap;               // = the shard's pad: every target can be listed, nothing overflows
    int strict_slices;                 // most source slices the fp64 pass may use (<= 256, <= total_tiles) = its gridDim.y
    unsigned long long strict_budget;  // doubles in strict_acc: slices x dim x stride never exceeds it
    double refine_c2;                  // a target is listed when |a|^2 < refine_c2 * Q  (Q = sum over slices of qsum)
    unsigned long long* __restrict__ clk;   // null, or [2 x gridDim.x x gridDim.y] clock stamps (AccelLaunch::clk)
};

struct KernelVariant {
    const char* name;
    int tpl;              // targets per lane
    void (*k2)(KArgs);    // D = 2
    void (*k3)(KArgs);    // D = 3
    int fast;             // 1: unguarded fast kernel + close-set pipeline (exact overall)
    int max_tiles_per_slice;  // > 0: the kernel's fp32 second-level sums want at most this many tiles per slice
    int needs_extent;     // 1: only valid while every |coordinate| <= kOneRcpMaxCoord (one-reciprocal kernel)
    void (*soft2)(KArgs); // softened-law build of the same kernel (null: none), D = 2 / 3
    void (*soft3)(KArgs);
    void (*newton2)(KArgs);  // softened Newtonian law (two-reciprocal form of the same kernel)
    void (*newton3)(KArgs);
    void (*qs2)(KArgs);      // the same fast kernel also writing KArgs::qsum (mixed mode; null: none)
    void (*qs3)(KArgs);
    int planes;              // fp32 planes of acc written per source slice: 1, or 2 = {hi, lo} of an fp64 sum (strict kernel)
    int aux;                 // 1: the kernel itself writes KArgs::qsum (the strict kernel's magnitude-sum build)
    int stamps;              // 1: the kernel writes KArgs::clk when it is non-null (measurement)
    int sym;                 // 1: the symmetric own-shard pass (force_sym_kernel.hip): own launch shape, S + K slots of `planes` planes (sym_plan.h)
};
// force_kernel.hip
const KernelVariant* kernel_variants(int* count);
// force_sym_kernel.hip
KernelVariant sym_kernel_variant();
KernelVariant sym_dpp_kernel_variant();   // the same pass with every rotation on DPP moves (comparator, last in the table)
struct CloseKernels { void (*classify[2])(KArgs); void (*classify_src[2])(KArgs); void (*refine[2])(KArgs); void (*scatter[2])(KArgs); void (*potential[2])(KArgs); void (*potential_soft[2])(KArgs); void (*potential_newton[2])(KArgs);
                      void (*refine_select[2])(KArgs); void (*strict_list[2])(KArgs); void (*refine_fold[2])(KArgs);
                      void (*close_only[2])(KArgs); };  // [0]: D=2, [1]: D=3
CloseKernels close_kernels();

// close_hash.hip
size_t hash_temp_bytes(unsigned capacity);
hipError_t hash_refine(int dim, const KArgs& a, const HashWork& h, hipStream_t stream);

// force_launch.hip
hipError_t launch_accel(int dim, const AccelLaunch& a, hipStream_t stream);
// Mixed mode, after the fast kernel has produced acc (all planes) and qsum (all slices) for the FULL source set:
//   select: a target is a suspect when its acceleration is small against the spread of its tile partial sums,
//           |a|^2 < c2 * sum_tiles |a_tile|^2 (or it is a close-set target) -> strict_list, count in counters[3];
//   strict: accel_f64_kernel<LIST> over ALL chunks, the listed targets x strict_slices source slices, fp64 throughout;
//   fold:   the slices added in fp64, the target's planes rewritten (plane 0 = hi, plane 1 = lo, the rest 0).
struct RefineLaunch {
    AccelLaunch base;          // pos/mass/acc/pad/count/tgt_chunk/n_chunks/counters/bad_flag/qsum of the evaluation to refine
    unsigned* strict_list;
    double* strict_acc;
    unsigned strict_cap;
    int strict_slices;
    unsigned long long strict_budget;
    double c2;
    int grid_slices;           // slices of the fast launch (planes of qsum)
};
hipError_t launch_refine(int dim, const RefineLaunch& R, hipStream_t stream);
// phi[splits][pad] = sum_j m_j / r^2 over ALL chunks (L.acc points at the phi buffer; L.splits slices)
hipError_t launch_potential(int dim, const AccelLaunch& a, hipStream_t stream);
int num_variants();
const char* variant_name(int variant);
int variant_tpl(int variant);
int variant_is_fast(int variant);
int variant_max_tiles_per_slice(int variant);
int variant_needs_extent(int variant);
int variant_has_law_builds(int variant);  // softened / Newtonian builds of the kernel exist (the A/B table entries have none)
int variant_planes(int variant);          // fp32 planes of acc per source slice (2: strict fp64 kernel)
int variant_has_qsum(int variant);        // the variant has a build that writes qsum (mixed mode possible)
int variant_writes_aux(int variant);      // the variant's own kernel writes qsum (strict magnitude-sum build)
int variant_is_sym(int variant);           // the symmetric own-shard pass: launched for single-shard contexts only (sym_plan.h)
int variant_sym_slots(int variant, unsigned pad);   // its S + K slots for a shard of `pad` bodies; 0: no symmetric decomposition
int variant_sym_workgroups(int variant, unsigned pad);   // workgroups of its launch (B x S); 0: no symmetric decomposition
int variant_has_clock_stamps(int variant);   // the variant's kernel honours AccelLaunch::clk (the three-level kernel)
// demangled symbol of the kernel launch_accel launches for (variant, dim, law, softened, mixed mode) -- the name rocprofv3 prints
int variant_kernel_symbol(int variant, int dim, int law, int soft, int qsum, char* buf, size_t len);
int default_fast_two_rcp_variant();   // fast variant without the extent precondition
int variant_by_name(const char* name);
int default_variant();        // the fast default
int default_exact_variant();  // used when the fast path's preconditions do not hold

// state_kernels.hip
struct PackArgs {
    const double* raw;     // staged Body<D> array, n_total bodies
    size_t stride_d;       // doubles between consecutive bodies
    size_t n_total;
    size_t shard_len;      // bodies per shard (last shard may hold fewer)
    unsigned pad;
    int n_shards, shard, dim;
    float* pos_all;        // [n_shards][dim][pad]
    float* mass_all;       // [n_shards][pad]
    double* x64;           // [dim][pad]   own shard
    double* v64;           // [dim][pad]
    double* m64;           // [pad]
    int only_own;          // 1: `raw` holds the own shard's bodies only (n_own of them) and only the own chunk is packed
    size_t n_own;
    unsigned long long* facts;  // [3], zeroed by the caller: bit patterns of max |mass| and max |coordinate| over all bodies
                                // (NaN sorts above everything), and the own shard's count of close-set candidates
};
hipError_t launch_pack(const PackArgs& p, hipStream_t stream);

struct KickDriftArgs {
    const float* acc;      // [splits][dim][pad]
    int splits, dim;
    unsigned pad;
    size_t count;          // real bodies in this shard
    double G, dt_kick, dt_drift;   // v += (F/m) * dt_kick;  x += v * dt_drift  (both = dt: the reference's kick then drift)
    double* x64; double* v64; const double* m64;
    float* pos_chunk;      // this shard's chunk of pos_all: [dim][pad]
};
hipError_t launch_kick_drift(const KickDriftArgs& k, hipStream_t stream);
// The same update from fp64 leaf sums indexed by padded slot (leaf plan, leaf_plan_api.hip): body l's sum is
// sums[k][body_slot[l]] (0 when body_slot[l] == 0xffffffff: the body belongs to no leaf); F = (signedG m) sum.  The caller says
// whether the drift runs: `drift` false launches the pure kick, which touches no position, while a drift by dt_drift = 0 still
// reads and writes them.
struct SlotKickArgs {
    const double* sums;        // [dim][pslots]
    const uint32_t* body_slot; // [count]
    uint32_t pslots;
    int dim;
    unsigned pad;
    bool drift;                // host side only (it picks the kernel); it lies in the padding in front of `count`
    size_t count;
    double signedG, dt_kick, dt_drift;   // as KickDriftArgs': both = dt is the reference's kick then drift
    double* x64; double* v64; const double* m64;
    float* pos_chunk;
};
static_assert(offsetof(SlotKickArgs, drift) == 28 && offsetof(SlotKickArgs, count) == 32 && sizeof(SlotKickArgs) == 96,
              "SlotKickArgs::drift must stay inside the padding: the kernels' argument block is the one they were compiled for");
hipError_t launch_kick_drift_slots(const SlotKickArgs& k, hipStream_t stream);
// *out (device, 8 bytes; zeroed here first) = bit pattern of max over the n bodies with a slot of absG * |sums[.][slot]|, fp64
hipError_t launch_slot_accel_max(const double* sums, const uint32_t* body_slot, uint32_t pslots, int dim, size_t n, double absG,
                                 unsigned long long* out, hipStream_t stream);

// The device's step clock of nbx_leaf_plan_step_kdk_adaptive (include/nbody_hip.h has the rule): one block in device memory, this
// record at its start and the history -- (a_max, dt) pairs, 16 bytes each -- kStepClockHistoryOffset bytes behind it.  The controller
// (one thread behind every evaluation's reduction) writes it; the clock kick reads this evaluation's {dt_kick, dt_drift, drift,
// apply}; the host reads `stopped` (a look it never waits for) and, when asked, the rest.
struct StepClock {
    unsigned long long amax_bits;      // the reduction's word (launch_step_controller zeroes it first)
    double accel_length, dt_min, dt_max, t_end;
    double t, prev, a_max_last;
    double dt_kick, dt_drift;          // this evaluation's kick
    int pow2, drift, apply;            // drift, apply: this evaluation's kick drifts / is made at all
    int stopped, finished, status;
    uint32_t steps, evaluations, recorded;
    uint32_t capacity;                 // history entries the block has room for
};
constexpr size_t kStepClockHistoryOffset = 256;
static_assert(sizeof(StepClock) <= kStepClockHistoryOffset, "the history starts behind the clock");
// the clock as a call finds it: the control's values, t = t_start, nothing recorded
hipError_t launch_step_clock_init(StepClock* clock, double accel_length, double dt_min, double dt_max, double t_start, double t_end, int pow2,
                                  uint32_t capacity, hipStream_t stream);
// launch_slot_accel_max's value into clock->amax_bits, reduced slot by slot (pslot_body[pslots]: the body of every slot, 0xffffffff for
// a pad), and the controller behind it; `last`: this is evaluation number max_steps
hipError_t launch_step_controller(const double* sums, const uint32_t* pslot_body, uint32_t pslots, int dim, double absG, StepClock* clock, bool last,
                                  hipStream_t stream);
// launch_kick_drift_slots with dt_kick, dt_drift and the two flags read from the clock (k's own are not read)
hipError_t launch_kick_drift_slots_clock(const SlotKickArgs& k, const StepClock* clock, hipStream_t stream);
// The same loop for the all-pairs context (nbx_ctx_step_kdk_adaptive), whose sums are the fp32 planes of KickDriftArgs:
// *out (device, 8 bytes; zeroed here first) = bit pattern of max over the count real bodies of absG * |A[l]|, A_k[l] the fp64 sum of
// the planes in plane order (kick_drift_kernel's sum_partials, bit for bit); a sum that is not finite makes it not finite
hipError_t launch_ctx_accel_max(const float* acc, int splits, int dim, unsigned pad, size_t count, double absG, unsigned long long* out,
                                hipStream_t stream);
// the controller alone, behind whichever reduction has filled clock->amax_bits (launch_step_controller = the plan's reduction + this)
hipError_t launch_step_control(StepClock* clock, bool last, hipStream_t stream);
// launch_kick_drift with dt_kick and dt_drift read from the clock (k's own are not read); nothing is touched when clock->apply == 0
hipError_t launch_kick_drift_clock(const KickDriftArgs& k, const StepClock* clock, hipStream_t stream);

// ---- forces on a list of targets (active_kernel.hip; nbx_ctx_compute_accel_active) and block time steps (nbx_ctx_step_kdk_block) ----
// One evaluation of the softened laws for the targets list[0 .. *count) against the `pad` entries of chunk 0.  The list and its length
// live on the device; the launch is sized for `cap` targets and everything that depends on the length -- slices, stride, which of
// the two instantiations works -- is decided there (active_kernel.hip: active_layout).  part holds [slices][dim][stride] fp64 slice
// sums, sums the folded [dim][cap] result: row r belongs to list[r].
struct ActiveArgs {
    const float* pos_all;        // chunk 0: [dim][pad]
    const float* mass_all;       // [pad]
    const unsigned* list;        // [cap]
    const unsigned* count;       // device word: the list's length (read as min(*count, cap))
    double* part;                // [slices][dim][stride], at most `budget` doubles
    double* sums;                // [dim][cap]
    const int* stopped;          // null, or a device word: non-zero makes every kernel return at once (the block loop's stop)
    unsigned long long budget;   // doubles in part: >= dim * cap rounded up to 256 (one slice of every target always fits)
    unsigned pad, cap;
    unsigned long_list;          // lists of at least this many targets go to the long-list build (8 targets per lane), shorter ones to 1 per lane
    int max_slices;              // most source slices (<= 256, <= pad / kTile)
    int dim, law;                // law 0: m d / rho^4, 1: m d / rho^3; rho^2 = r^2 + eps2
    float eps2;
};
// What a launch looks like for the list as it stands: n targets, `stride` doubles between the planes of a slice (n in whole blocks
// of 256), as many source slices as the buffer holds (at most the grid's), `tps` source tiles per slice.  `planes` sums are kept per
// (target, slice): dim for the forces, 2 dim for the accelerations and jerks of active_jerk_kernel.hip.
struct ActiveLayout { unsigned n, stride, slices, tps; };
__device__ __forceinline__ ActiveLayout active_layout(const ActiveArgs& a, int planes) {
    ActiveLayout s;
    const unsigned listed = *a.count;
    s.n = listed < a.cap ? listed : a.cap;
    s.stride = s.n ? (s.n + 255u) / 256u * 256u : 256u;
    unsigned long long fit = a.budget / ((unsigned long long)planes * s.stride);
    if (fit > (unsigned long long)a.max_slices) fit = (unsigned long long)a.max_slices;
    s.slices = fit ? (unsigned)fit : 1u;
    const unsigned tiles = a.pad / (unsigned)kTile;
    s.tps = (tiles + s.slices - 1u) / s.slices;
    return s;
}
constexpr unsigned kActiveLongBlock = 2048;   // targets per workgroup of the long-list build: 256 lanes x 4 float2 pairs
hipError_t launch_active_accel(const ActiveArgs& a, hipStream_t stream);
// active_jerk_kernel.hip: the same evaluation with the time derivative.  a.part holds [slices][2 dim][stride] slice sums (a.budget >=
// 2 dim * cap rounded up to 256), a.sums the folded [2 dim][cap] result, planes 0 .. dim-1 the acceleration sums, dim .. 2 dim-1 the
// jerk sums; vel_all: chunk 0's fp32 velocities [dim][pad], pads zero.
constexpr unsigned kJerkLongBlock = 1024;     // targets per workgroup of its long-list build: 256 lanes x 2 float2 pairs
hipError_t launch_active_accel_jerk(const ActiveArgs& a, const float* vel_all, hipStream_t stream);
// accel_out, jerk_out (either may be null): AoS double[*count][dim] on the device, row r = -(G sums[.][r])
hipError_t launch_active_jerk_export(const ActiveArgs& a, double G, double* accel_out, double* jerk_out, hipStream_t stream);
// forces_out: AoS double[*count][dim] on the device, row r = -(G m[list[r]]) sums[.][r]
hipError_t launch_active_export(const ActiveArgs& a, double G, const double* m64, double* forces_out, hipStream_t stream);

// The device's clock of nbx_ctx_step_kdk_block (include/nbody_hip.h has the rule): this record at the start of one block of device
// memory, the history -- (n_active, dn) pairs of 32-bit words -- kBlockClockHistoryOffset bytes behind it.
struct BlockClock {
    double accel_length, dt_max, tick, t_start, t;
    double dt_drift;                    // this substep's drift, dn * tick
    unsigned long long T, T_end, pair_terms, n_total;
    unsigned n_active;                  // the active list's length: what the force kernels read
    unsigned n_bodies;                  // = n_total, the select scan's count word
    unsigned bad;                       // an active body's acceleration was not finite (this evaluation)
    unsigned pop[21];                   // bodies per level
    int levels;                         // L
    int first, closing, apply, drift;   // this evaluation: the call's first / at T_end / kicks are made / a drift follows
    int stopped, finished, status, deepest;
    uint32_t substeps, evaluations, recorded, capacity, max_substeps;
};
constexpr size_t kBlockClockHistoryOffset = 512;
static_assert(sizeof(BlockClock) <= kBlockClockHistoryOffset, "the history starts behind the clock");
struct BlockStepArgs {
    BlockClock* clock;
    int* level;                 // [count] the bodies' levels
    unsigned* list;             // [count] the active list (ascending), its length in clock->n_active
    unsigned* flags;            // [count + 1] select: 1 for an active body; scanned in place
    unsigned* tile_sums;        // device_sort.h exclusive_scan's workspace
    const double* sums;         // [dim][cap] ActiveArgs::sums of this evaluation
    unsigned cap;
    int dim;
    unsigned pad;
    size_t count;
    double G;                   // as KickDriftArgs::G (negated for the attractive law)
    double absG;
    double* x64; double* v64; const double* m64;
    float* pos_chunk;
};
hipError_t launch_block_clock_init(const BlockStepArgs& b, double accel_length, double dt_max, double t_start, int levels, unsigned long long T_end,
                                   uint32_t max_substeps, uint32_t capacity, hipStream_t stream);
// behind an evaluation's fold: the finiteness check, the controller's first half, the kick of the active bodies
hipError_t launch_block_kick(const BlockStepArgs& b, hipStream_t stream);
// the controller's second half (history, stop, dn, T), the drift of all bodies, the next active list
hipError_t launch_block_advance(const BlockStepArgs& b, hipStream_t stream);
// the active list for the clock's T as it stands (launch_block_advance ends with it; a call starts with it)
hipError_t launch_block_select(const BlockStepArgs& b, hipStream_t stream);

// ---- fourth-order Hermite with block time steps (nbx_ctx_step_hermite_block; include/nbody_hip.h has the rule) ----
// The loop shares the block clock, both controllers, the levels and the select with the kick-drift-kick loop (b; b.sums is not
// read).  Its own state: a, j at each body's own time t_i (in ticks), and the fp32 velocity chunk next to b.pos_chunk.
struct HermiteArgs {
    BlockStepArgs b;
    const double* sums;             // [2 dim][b.cap]: launch_active_accel_jerk's folded sums of this evaluation
    double* a64; double* j64;       // [dim][pad]
    unsigned long long* t_i;        // [count]
    float* vel_chunk;               // [dim][pad]
    double eta, eta_start;
};
// vel_chunk = (float) v64 for the real bodies (the pads stay zero)
hipError_t launch_hermite_refresh_velocities(const HermiteArgs& h, hipStream_t stream);
// behind an evaluation's fold: the finiteness check of both sum sets, the controller's first half, then the first evaluation's
// start (a, j, level, t_i = 0) or the corrector and the level choice of the active bodies
hipError_t launch_hermite_correct(const HermiteArgs& h, hipStream_t stream);
// the controller's second half, the predictor of ALL bodies into the fp32 chunks, the next active list
hipError_t launch_hermite_advance(const HermiteArgs& h, hipStream_t stream);

// forces_out: AoS double[count][dim] on the device
hipError_t launch_export_forces(const float* acc, int splits, int dim, unsigned pad, size_t count,
                                double G, const double* m64, double* forces_out, hipStream_t stream);
// accel_out: SoA float[dim][count] on the device (splits summed in fp64, rounded once)
hipError_t launch_export_accel(const float* acc, int splits, int dim, unsigned pad, size_t count,
                               float* accel_out, hipStream_t stream);
// energy_out: double[2][ceil(count/256)]: per-workgroup sums (wave-level reduction on the device) of the bodies' kinetic
// m v^2 / 2 and potential (G m / 4) * sum_slices phi
hipError_t launch_export_energy(const float* phi, int splits, int dim, unsigned pad, size_t count, double G,
                                const double* v64, const double* m64, double* energy_out, hipStream_t stream);
// *accurate = number of bodies whose force is within the reference's 1 % rule of ref_forces (device AoS double[count][dim])
// out[count] (device, double) = sum over the aux planes of aux[plane][i], in plane order
hipError_t launch_export_aux(const float* aux, int planes, unsigned pad, size_t count, double* out, hipStream_t stream);
hipError_t launch_accuracy(const float* acc, int splits, int dim, unsigned pad, size_t count, double G,
                           const double* m64, const double* ref_forces, unsigned* accurate, hipStream_t stream);
// state_out: AoS double[count][2*dim] = position then velocity
hipError_t launch_export_state(const double* x64, const double* v64, int dim, unsigned pad, size_t count,
                               double* state_out, hipStream_t stream);

}  // namespace nbx
#endif
