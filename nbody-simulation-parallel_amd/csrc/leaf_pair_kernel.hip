// leaf_pair_kernel.hip -- SURVEY 8(f-4): batched (target leaf, source leaf) direct sums for the reference's tree
// codes -- the near-field step either side of the brute-force path:
//   FMM_Parlay<D>::p2p_phase   nbody-sim-new/fmm_parlay.cpp:916-1022   (law NBX_LAW_FMM_P2P)
//   BVH leaf loop              nbody-sim-new/bvh.cpp:150-176           (law NBX_LAW_TREE_LEAF)
//   octree leaf term           nbody-sim-new/octree.cpp:105-125        (law NBX_LAW_TREE_LEAF)
// and, for completeness, the brute-force law itself over leaf lists (NBX_LAW_BRUTE, methods.cpp:21-37).
// All three are m_j d / r^4 sums; they differ in sign and in what happens below ~1e-5 separation.
//
// Mapping to CDNA4.  The reference walks pointer lists per (body, neighbour leaf) work item and adds into
// forces[body] from several work items at once (fmm_parlay.cpp:986-1020).  Here the work is target-leaf-major and
// everything the kernel follows is laid out for it once per call:
//  * bodies are gathered into leaf order as fp32 SOURCE PAIRS {xa,xb,ya,yb},{za,zb,ma,mb} (32 B; a leaf of odd size
//    ends in a massless body far away), so a source leaf is a run of whole pairs that is copied into LDS as it lies
//    and read back with ds_read_b128 straight into the aligned register pairs of v_pk_*_f32;
//  * a leaf's source list becomes a few COPY OPS on the host: consecutive list entries whose leaves are neighbours
//    in leaf order are merged (the 27 cells of a grid neighbourhood are 9 to 11 runs), with the running length of the
//    stream they form -- no list walk, no leaf-offset lookup and no prefix sum on the device;
//  * one workgroup = two wave64 = ONE leaf: the waves share the staged tiles (512 bodies) and each owns one PIECE of
//    the leaf's targets.  A piece of c targets runs floor(64 / c) lanes per target (at most 8), which split the
//    tile's pairs between them; the host cuts the leaf where the two pieces together waste the fewest lanes
//    (43 targets: 11 x 5 lanes + 32 x 2 lanes = 96 % of the lanes busy; one wave64 with one lane each: 67 %).  Small leaves
//    (a mean of <= 20 bodies) get one wave per workgroup and no cut;
//  * structures of SMALL leaves (a mean of <= 8 bodies) are PACKED instead: 4, 8, 10 or 16 leaves share a wave64, every lane holds two
//    targets and streams its share of its leaf's source pairs straight from memory (leaf_pack_kernel below; leaf_plan.h);
//  * the workgroups are launched longest first, so that the launch drains in a fraction of a mean workgroup's time, and the
//    blocks of a duration class are dealt to the eight XCDs in consecutive runs (leaf_plan.h order_launch);
//  * the law's special cases sit below r^2 = 1e-9.  A target whose fp32 coordinates are all >= 2^14 in magnitude
//    cannot own such a pair other than with an identical position (the brute-force kernel's argument,
//    nbx_internal.h: distinct fp32 numbers that large differ by >= 2^-10), so a wave of such targets runs the pair
//    loop with no compare at all: r^2 biased by 2^-47, an identical position contributes m 2^94 x 0 = 0 as every law
//    asks.  Each wave decides for itself from its lanes' own coordinates (and the call's largest mass); the other waves
//    take the guarded loop (the smallest r^2 of a trip's four pairs, one compare, a wave vote, and the law's exact
//    weights for the wave that saw a pair below the threshold);
//  * NBX_LAW_NEWTON (extension: m_j d / (r^2 + eps^2)^(3/2), eps the plan's softening length) is the simplest law here: with eps^2 in
//    place of the 2^-47 bias no special case exists, so EVERY wave runs the unguarded loop -- no close-set test, no mass bound, no
//    vote -- with v_rsq_f32 where the other laws have v_rcp_f32 (PairTerm::plain).
// fp32 sums over at most 256 terms per lane, flushed into fp64 accumulators.  No atomics, a fixed summation order,
// every output written once.  Leaves are small (the reference caps them at 100 bodies, methods.h:26), so the launch
// is tens of thousands of short workgroups; HBM traffic is 16 B per (workgroup, source body), served mostly from L2.
#include "../../include/nbody_hip.h"
#include "nbx_internal.h"
#include "leaf_near.h"
#include "leaf_law.h"

#include <type_traits>

using namespace nbx;
using namespace nbx_leaf;

namespace {

constexpr int kUnitsPerLane = 4;               // 16-byte units (= bodies) a lane stages per tile (the kernel names that many registers)
// a tile is 64 x WAVES x kUnitsPerLane bodies: 512 (256 source pairs, 8 KB of LDS) with two waves per workgroup
constexpr int kPadPairs = 16;                  // massless pairs behind the tile's last one: the lane groups' last trips reach up to 2 P - 1 past it
constexpr int kMaxOps = 64;                    // copy ops held in LDS at a time (longer lists go in chunks)
constexpr unsigned kFlushTerms = 248;          // fp32 terms per lane between flushes into the fp64 sums (+ 2 for a closing single pair)

// the laws' thresholds, kFar and leaf_weight: leaf_law.h (shared with the far-field pass, leaf_far_kernel.hip)

struct LeafArgs {
    const float4* __restrict__ xp;     // [pslots] units: pair p = units 2p {xa,xb,ya,yb} and 2p+1 {za,zb,ma,mb}
    uint32_t pslots;                   // padded slots = 2 x pairs
    const CopyOp* __restrict__ ops;
    const LeafBlock* __restrict__ blocks;
    double* __restrict__ acc;          // [dim][pslots]
    const uint32_t* __restrict__ max_mass_bits;   // bit pattern of the largest |mass| as fp32 (leaf_gather_kernel); a NaN compares above every number
    float eps2;                        // NBX_LAW_NEWTON: the plan's softening length squared (> 0); no other law reads it
};

typedef float f2 __attribute__((ext_vector_type(2)));

// Below this r^2 a pair leaves the plain m_j d / r^4 form under the law (skip or smoothing); leaf_weight decides how.
template <int LAW>
__device__ __forceinline__ constexpr float law_special_below() {
    return LAW == NBX_LAW_BRUTE ? kR2SkipF : LAW == NBX_LAW_TREE_LEAF ? kTreeSkipF : kSmoothF;
}

// One source pair {A, B} (two float4 of the tile) against this lane's target.
template <int D>
struct PairTerm {
    f2 dx, dy, dz, r2, sm;
    __device__ __forceinline__ PairTerm(const float4 A, const float4 B, const f2 ix2, const f2 iy2, const f2 iz2, const f2 bias) {
        sm = f2{B.z, B.w};
        dx = f2{A.x, A.y} - ix2;
        dy = f2{A.z, A.w} - iy2;
        dz = (D == 3) ? f2{B.x, B.y} - iz2 : f2{0.f, 0.f};
        r2 = __builtin_elementwise_fma(dx, dx, bias);
        r2 = __builtin_elementwise_fma(dy, dy, r2);
        if (D == 3) r2 = __builtin_elementwise_fma(dz, dz, r2);
    }
    template <int LAW, bool PACKED = false>
    __device__ __forceinline__ f2 plain() const {
        if (LAW == NBX_LAW_NEWTON) {
            // r2 carries eps^2 as its bias: m / (r^2 + eps^2)^(3/2) = rs^3 m, 2 v_rsq_f32 + 3 v_pk_mul per two pairs.  Nothing overflows
            // while m / eps^3 is finite (plan_check_law), and a massless pad at 1e18 gives 2e-55 -> 0, times 0: exact zeros, never a NaN.
            // The order of the three products is chosen per kernel by the registers the allocator then needs (every instantiation at
            // or below its TREE_LEAF twin, profiles/r12/newton_tree.txt): ((m rs) rs) rs in the one-leaf workgroups, ((rs rs) rs) m in
            // the packed waves -- the other way round, and either mixed order, costs 2 and 8 VGPRs.  The packed order forms rho^-3
            // BEFORE the mass: it is a normal fp32 number only for rho = sqrt(r^2 + eps^2) < 4.4e12 and loses bits beyond (the one-leaf
            // order and leaf_weight_ri do not).  That is the law's documented range (include/nbody_hip.h); the other laws' 1 / r^4
            // leaves fp32's normal range at r = 3e9 already.
            const f2 rs = {__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)};
            if (PACKED) return ((rs * rs) * rs) * sm;
            f2 t = rs * sm;
            t = t * rs;
            return t * rs;
        }
        f2 w = {__builtin_amdgcn_rcpf(r2.x), __builtin_amdgcn_rcpf(r2.y)};
        w = w * w;
        return w * sm;
    }
    template <int LAW>
    __device__ __forceinline__ unsigned long long special() const {
        return __builtin_amdgcn_ballot_w64(r2.x < law_special_below<LAW>()) | __builtin_amdgcn_ballot_w64(r2.y < law_special_below<LAW>());
    }
    template <int LAW>
    __device__ __forceinline__ f2 guarded() const {
        float ra = r2.x, rb = r2.y;
        asm volatile("" : "+v"(ra), "+v"(rb));   // keeps the guarded form's compares in this (rare) branch: hipcc hoists them otherwise
        return f2{leaf_weight<D, LAW>(ra, sm.x, dx.x, dy.x, dz.x), leaf_weight<D, LAW>(rb, sm.y, dx.y, dy.y, dz.y)};
    }
};

// Does any lane of the wave hold a pair (of the four of a trip) below the law's threshold?  The smallest of the four r^2 by two
// v_min3_f32, one compare, one vote.
template <int LAW, int D>
__device__ __forceinline__ bool any_special(const PairTerm<D>& q0, const PairTerm<D>& q1) {
    const float m = __builtin_fminf(__builtin_fminf(q0.r2.x, q0.r2.y), __builtin_fminf(q1.r2.x, q1.r2.y));
    return __builtin_amdgcn_ballot_w64(m < law_special_below<LAW>()) != 0ull;
}

// The sums of one lane: fp32 per-tile level, fp64 second level.
template <int D>
struct Sums {
    f2 ax = {0.f, 0.f}, ay = {0.f, 0.f}, az = {0.f, 0.f};
    double* o;              // this lane's fp64 sums, kept in LDS (they are touched once per ~250 terms; 6 VGPRs less): o[0], o[stride], o[2 stride]
    unsigned stride;        // lanes of the workgroup
    unsigned pending = 0;   // terms in the fp32 sums since the last flush (wave-uniform)
    __device__ __forceinline__ void add(const PairTerm<D>& q, const f2 w) {
        ax = __builtin_elementwise_fma(w, q.dx, ax);
        ay = __builtin_elementwise_fma(w, q.dy, ay);
        if (D == 3) az = __builtin_elementwise_fma(w, q.dz, az);
    }
    __device__ __forceinline__ void store() {   // flush() into sums that hold nothing yet: no read, no zeroing beforehand
        o[0] = (double)ax.x + (double)ax.y;
        o[stride] = (double)ay.x + (double)ay.y;
        if (D == 3) o[2u * stride] = (double)az.x + (double)az.y;
        ax = ay = az = f2{0.f, 0.f};
        pending = 0;
    }
    __device__ __forceinline__ void flush() {
        o[0] += (double)ax.x + (double)ax.y;
        o[stride] += (double)ay.x + (double)ay.y;
        if (D == 3) o[2u * stride] += (double)az.x + (double)az.y;
        ax = ay = az = f2{0.f, 0.f};
        pending = 0;
    }
};

// T source pairs (T odd) at s, for this lane's target: (T - 1) / 2 trips of two pairs -- two independent dependency chains --
// and a closing single pair.  GUARD: the law's special cases are possible for this wave's targets (one wave vote per trip);
// without it a trip is 26 VALU (6 v_pk_add, 6 + 6 v_pk_fma, 4 v_pk_mul, 4 v_rcp_f32) and half an address increment, and the
// LDS reads of the trip after next are in flight while a trip is computed.
template <int D, int LAW, bool GUARD>
__device__ __forceinline__ void consume(const float4* __restrict__ s, const unsigned T, const f2 ix2, const f2 iy2, const f2 iz2, Sums<D>& S, const float eps2) {
    static_assert(!(GUARD && LAW == NBX_LAW_NEWTON), "the softened law has no special case: every wave runs the unguarded form");
    const f2 bias = LAW == NBX_LAW_NEWTON ? f2{eps2, eps2} : GUARD ? f2{0.f, 0.f} : f2{kTiny, kTiny};
    const unsigned ndt = T >> 1;
    unsigned done = 0;
    while (done < ndt) {                                    // wave-uniform bookkeeping
        if (S.pending + 4u > kFlushTerms) S.flush();
        const unsigned room = (kFlushTerms - S.pending) >> 2;
        const unsigned n = __builtin_amdgcn_readfirstlane((ndt - done < room) ? ndt - done : room);
        if (!GUARD) {
            // the trip after next is read while this one is computed: two register sets, taking turns (no copies)
            auto trip = [&](const float4 A0, const float4 B0, const float4 A1, const float4 B1) {
                const PairTerm<D> q0(A0, B0, ix2, iy2, iz2, bias), q1(A1, B1, ix2, iy2, iz2, bias);
                const f2 w0 = q0.template plain<LAW>(), w1 = q1.template plain<LAW>();
                S.add(q0, w0);
                S.add(q1, w1);
            };
            float4 a0 = s[0], a1 = s[1], a2 = s[2], a3 = s[3];
            unsigned i = n;
            for (; i >= 2u; i -= 2u, s += 8) {
                const float4 b0 = s[4], b1 = s[5], b2 = s[6], b3 = s[7];
                __builtin_amdgcn_sched_barrier(0);
                trip(a0, a1, a2, a3);
                __builtin_amdgcn_sched_barrier(0);
                a0 = s[8]; a1 = s[9]; a2 = s[10]; a3 = s[11];     // may lie past the segment: read, not used (the tile has room)
                __builtin_amdgcn_sched_barrier(0);
                trip(b0, b1, b2, b3);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (i) { trip(a0, a1, a2, a3); s += 4; }
        } else {
            // the guarded form keeps one register set (with two, the rare branch's live values push the kernel past 96 VGPRs)
            for (unsigned i = n; i != 0u; --i, s += 4) {
                const PairTerm<D> q0(s[0], s[1], ix2, iy2, iz2, bias), q1(s[2], s[3], ix2, iy2, iz2, bias);
                f2 w0, w1;
                if (__builtin_expect(any_special<LAW>(q0, q1), 0)) {   // wave-uniform, rare
                    w0 = q0.template guarded<LAW>();
                    w1 = q1.template guarded<LAW>();
                } else {
                    w0 = q0.template plain<LAW>();
                    w1 = q1.template plain<LAW>();
                }
                S.add(q0, w0);
                S.add(q1, w1);
            }
        }
        S.pending += 4u * n;
        done += n;
    }
    const PairTerm<D> q0(s[0], s[1], ix2, iy2, iz2, bias);
    const f2 w0 = (GUARD && __builtin_expect(q0.template special<LAW>() != 0ull, 0)) ? q0.template guarded<LAW>() : q0.template plain<LAW>();
    S.add(q0, w0);
    S.pending += 2u;
}

// One workgroup = one target leaf (or 128 targets of a larger one) against the stream of source pairs its copy ops describe.
//  * Staging: a tile is kTileUnits consecutive stream positions; lane l copies positions l, l + 128, ... (one 16-byte
//    load and one ds_write_b128 each, conflict-free); the run a position falls in is found by stepping a cursor through the
//    ops' running lengths in LDS -- it only ever moves forward and a run holds ~100 bodies.  The next tile's loads
//    are issued before the current tile is consumed.
//  * The pair loop: lane group g of a piece takes the T consecutive pairs from g T on, T = ceil(pairs / P) made odd:
//    consecutive pairs sit at immediate offsets of one address register, and the groups' addresses differ by odd
//    multiples of 32 B, which no two of <= 8 groups share a bank on.  Pairs past the tile's end are the pad pairs.
//  * A body meets itself in its own leaf: r^2 = 0 falls under every law's skip rule (methods.cpp:113 skips i == j by
//    index, which only differs from the r^2 rule for r^2 >= 1e-10 -- impossible for a body and itself).
// LDS of one one-leaf workgroup: the tile (+ what the pipelined pair loop reads ahead of its last trip), the run tables, the closing sums
template <int WAVES>
constexpr unsigned pair_smem_bytes() {
    return (unsigned)((64 * WAVES * kUnitsPerLane + 2 * kPadPairs + 16) * sizeof(float4) + 2 * kMaxOps * sizeof(uint32_t) + 3 * 64 * WAVES * sizeof(double));
}
template <int D, int LAW, int WAVES>
__device__ __forceinline__ void leaf_pair_body(const LeafArgs& a, const unsigned block, char* __restrict__ smem) {
    constexpr int kThreads = 64 * WAVES;
    constexpr int kTileUnits = kThreads * kUnitsPerLane;
    constexpr int kTileSlots = kTileUnits + 2 * kPadPairs + 16;
    float4* const tile = reinterpret_cast<float4*>(smem);
    uint32_t* const op_end = reinterpret_cast<uint32_t*>(smem + kTileSlots * sizeof(float4));
    uint32_t* const op_base = op_end + kMaxOps;
    double (*const osum)[kThreads] = reinterpret_cast<double (*)[kThreads]>(smem + kTileSlots * sizeof(float4) + 2 * kMaxOps * sizeof(uint32_t));
    static_assert(kUnitsPerLane == 2 || kUnitsPerLane == 4, "the kernel names two or four staging registers");
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const LeafBlock* __restrict__ bp = a.blocks + block;
    const uint32_t op_lo = bp->op_lo, op_n = bp->op_n;
    const uint32_t max_mass_bits = *a.max_mass_bits;
    const uint32_t p_first = bp->piece[wave].first, p_count = bp->piece[wave].count;
    // lanes per target: as many whole groups of `count` lanes as the wave holds (21 targets: 3 lanes each)
    const unsigned W = p_count ? p_count : 1u;
    const unsigned fit = 64u / W;
    const unsigned P = fit < (unsigned)kMaxLanesPerTarget ? fit : (unsigned)kMaxLanesPerTarget;
    const unsigned inv_P = (65536u + P - 1u) / P;                 // q / P = (q * inv_P) >> 16 for q < 2^13
    // lane / W through fp32: (lane + 0.5) / W is at least 1/128 away from an integer, the arithmetic is good to 2e-5
    const unsigned g_raw = (unsigned)(((float)lane + 0.5f) * __builtin_amdgcn_rcpf((float)W));
    const unsigned t = lane - g_raw * W;
    const bool valid = p_count != 0u && g_raw < P;             // lanes left over compute along with group 0, unused
    const unsigned g = valid ? g_raw : 0u;
    const uint32_t pslot = p_first + (valid ? t : 0u);
    const float* __restrict__ xf = reinterpret_cast<const float*>(a.xp) + (size_t)(pslot >> 1) * 8u + (pslot & 1u);
    float ix = 0.f, iy = 0.f, iz = 0.f;
    if (p_count) { ix = xf[0]; iy = xf[2]; if (D == 3) iz = xf[4]; }
    const f2 ix2 = {ix, ix}, iy2 = {iy, iy}, iz2 = {iz, iz};
    // No special case of any law can apply to a pair of this wave (comment at the top of the file): every target of the piece lies
    // outside the close set, and m 2^94 stays finite for every mass.  The lanes left over hold the piece's first target.
    const bool in_close_set = !(__builtin_fabsf(ix) >= kCloseCoord && __builtin_fabsf(iy) >= kCloseCoord && (D == 2 || __builtin_fabsf(iz) >= kCloseCoord));
    const bool safe = __builtin_amdgcn_ballot_w64(in_close_set) == 0ull && max_mass_bits <= __builtin_bit_cast(uint32_t, (float)kFastMaxMass);
    Sums<D> S;
    osum[0][tid] = 0.0; osum[1][tid] = 0.0; osum[2][tid] = 0.0;   // only this lane touches them until the closing barrier
    S.o = &osum[0][tid];
    S.stride = (unsigned)kThreads;
    // a pad pair: unit {x,x,y,y} = far, unit {z,z,m,m} = {far (0 in 2D), 0}; selected by component (an indexed pair of constants ends up in scratch)
    const bool odd_unit = (tid & 1u) != 0u;
    const float pad_xy = odd_unit ? ((D == 3) ? kFar : 0.0f) : kFar, pad_zm = odd_unit ? 0.0f : kFar;
    const float4 pad_unit = make_float4(pad_xy, pad_xy, pad_zm, pad_zm);
    // the ops in chunks of kMaxOps (one chunk for every list the reference's trees produce); all workgroup-uniform
    for (uint32_t c0 = 0; c0 < op_n; c0 += (uint32_t)kMaxOps) {
        const unsigned n_ops = (op_n - c0 < (uint32_t)kMaxOps) ? (unsigned)(op_n - c0) : (unsigned)kMaxOps;
        __syncthreads();                                       // the previous chunk's last tile and tables are done with
        if (tid < n_ops) {
            const CopyOp o = a.ops[op_lo + c0 + tid];
            op_end[tid] = o.end;
            op_base[tid] = o.base;
        }
        const uint32_t u_begin = c0 ? a.ops[op_lo + c0 - 1u].end : 0u;
        const uint32_t u_end = a.ops[op_lo + c0 + n_ops - 1u].end;
        __syncthreads();
        unsigned k = 0;                                        // this lane's cursor in the chunk's ops; only ever moves forward
        uint32_t run_end = 0u, run_base = 0u;                  // the run it is in, in registers (every unit read them from LDS before: two reads and their waits)
        // kUnitsPerLane named registers (an indexed array ends up in scratch)
        float4 nxt0 = pad_unit, nxt1 = pad_unit, nxt2 = pad_unit, nxt3 = pad_unit;
        auto load1 = [&](const uint32_t u, float4& v) {
            if (u < u_end) {
                while (u >= run_end) { run_end = op_end[k]; run_base = op_base[k]; ++k; }   // u < u_end = the last run's end: k stays inside the chunk
                v = a.xp[run_base + u];
            }
        };
        auto load = [&](const uint32_t u0) {
            load1(u0 + tid, nxt0);
            load1(u0 + (uint32_t)kThreads + tid, nxt1);
            if (kUnitsPerLane > 2) {
                load1(u0 + 2u * (uint32_t)kThreads + tid, nxt2);
                load1(u0 + 3u * (uint32_t)kThreads + tid, nxt3);
            }
        };
        load(u_begin);
        for (uint32_t u0 = u_begin; u0 < u_end; u0 += (uint32_t)kTileUnits) {
            const unsigned cur = (u_end - u0 < (uint32_t)kTileUnits) ? (unsigned)(u_end - u0) : (unsigned)kTileUnits;   // even
            __syncthreads();                                   // previous tile fully consumed by both waves
            if (tid < cur) tile[tid] = nxt0;
            if ((unsigned)kThreads + tid < cur) tile[(unsigned)kThreads + tid] = nxt1;
            if (kUnitsPerLane > 2) {
                if (2u * (unsigned)kThreads + tid < cur) tile[2u * (unsigned)kThreads + tid] = nxt2;
                if (3u * (unsigned)kThreads + tid < cur) tile[3u * (unsigned)kThreads + tid] = nxt3;
            }
            if (tid < 2u * (unsigned)kPadPairs) tile[cur + tid] = pad_unit;
            __syncthreads();
            if (u0 + (uint32_t)kTileUnits < u_end) load(u0 + (uint32_t)kTileUnits);   // in flight while this tile is consumed
            if (p_count) {                                     // wave-uniform
                const unsigned pairs = cur >> 1;
                const unsigned T = (((pairs + P - 1u) * inv_P) >> 16) | 1u;
                const float4* s = tile + 2u * g * T;
                if constexpr (LAW == NBX_LAW_NEWTON) consume<D, LAW, false>(s, T, ix2, iy2, iz2, S, a.eps2);   // no close set, no mass bound, no vote
                else if (safe) consume<D, LAW, false>(s, T, ix2, iy2, iz2, S, 0.0f);
                else consume<D, LAW, true>(s, T, ix2, iy2, iz2, S, 0.0f);
            }
        }
    }
    S.flush();
    // the lane groups' fp64 sums meet in LDS, in group order (deterministic)
    __syncthreads();
    if (valid && g == 0u) {
        double ox = 0.0, oy = 0.0, oz = 0.0;
        const unsigned l0 = (tid & ~63u) + t;
        for (unsigned q = 0; q < P; ++q) { ox += osum[0][l0 + q * W]; oy += osum[1][l0 + q * W]; oz += osum[2][l0 + q * W]; }
        a.acc[pslot] = ox;
        a.acc[(size_t)a.pslots + pslot] = oy;
        if (D == 3) a.acc[2 * (size_t)a.pslots + pslot] = oz;
    }
}

template <int D, int LAW, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void leaf_pair_kernel(LeafArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[pair_smem_bytes<WAVES>()];
    leaf_pair_body<D, LAW, WAVES>(a, blockIdx.x, smem);
}

// Packed small leaves (leaf_plan.h PackBlock): one wave64 = K = 64 / w leaves side by side, P lanes per target.  Nothing is staged:
// lane group g of a target walks pairs [g T, (g + 1) T) of its leaf's source stream straight from memory (two 16-byte loads per
// pair; the lanes of a leaf's targets share addresses, so a wave's load touches K x P distinct 32-byte records -- L2 hits, the
// neighbouring leaves' lists name the same bodies).  The leaf's copy runs sit in LDS, the run a lane is in in registers.  Every
// lane holds TWO targets (t and t + W of its leaf, W = ceil(count / 2) lanes per group): a loaded pair feeds four terms, which
// halves the loads (the texture-address path limits a loop of 13 packed VALU per 32 bytes loaded by every lane) and the
// bookkeeping per term.  The loop computes two pairs while the next two are in flight, two register sets taking turns (no
// copies): four loads outstanding per lane, so that a wave waits for memory once per ~90 instructions rather than once per pair.  T is the block's (every lane of the
// wave runs the same trips); a lane past its leaf's stream, or without a target, reads the launch's pad pair (massless, far
// away: exact zeros) at unit `pslots`.  No barrier in the loop, one start-up per K leaves.
// Replaces this round's first packed kernel (same blocks, each leaf's stream staged through its own region of an LDS tile):
// 0.213 -> 0.140 ms at 4-body leaves, profiles/r4/leaf_direct_ab.txt.
struct LeafPackArgs {
    const float4* __restrict__ xp;     // [pslots + 2] units: the launch's pad pair behind the last leaf's
    uint32_t pslots;
    const CopyOp* __restrict__ ops;
    const PackBlock* __restrict__ blocks;
    const PackSub* __restrict__ subs;
    double* __restrict__ acc;
    const uint32_t* __restrict__ max_mass_bits;
    float eps2;                        // as LeafArgs::eps2
};

#ifndef NBX_PACK_WAVES
#define NBX_PACK_WAVES 4   /* waves per SIMD the register allocation aims at: 3D 110 VGPRs (5 spills 14 registers, 6 spills 34) */
#endif
// Round 5: the pair OFFSETS of the wave's leaves are expanded into LDS once, before the loop -- entry q of a leaf's row is the byte
// offset of pair q of its stream (the pad pair's behind the stream's end) -- so that the loop reads two offsets with one ds_read_b64
// (one stage ahead of the loads they address) where it used to step a cursor through the copy runs for every pair: ~16 VALU per
// loop body of 52 (profiles/r4/pmc_pack_kernel.txt: 39 % of the wave's instructions were bookkeeping).  Waves whose rows do not
// fit kPackExpand entries (K x P x T; long streams) keep the cursor loop.
#ifndef NBX_PACK_EXPAND
#define NBX_PACK_EXPAND 1280
#endif
constexpr unsigned kPackExpand = NBX_PACK_EXPAND;           // offsets per wave (5 KB; they share their LDS with the cursor loop's run tables: 8.2 KB per wave with the closing sums)
constexpr unsigned kPackExpandSlack = 8;         // the pipelined loop reads offsets up to 6 entries past its share
constexpr unsigned kPackTableWords = 2u * kPackMaxSubs * (kPackMaxOps + 1);
// LDS of a packed wave: ONE region for the cursor loop's run tables or the expanded loop's offsets (a wave runs one of the two loops),
// and the closing sums behind it
constexpr unsigned kPackLoopWords = kPackTableWords > kPackExpand + kPackExpandSlack ? kPackTableWords : kPackExpand + kPackExpandSlack;
constexpr unsigned kPackSmemBytes = kPackLoopWords * 4u + 3u * 128u * (unsigned)sizeof(double);
template <int D, int LAW>
__device__ __forceinline__ void leaf_pack_body(const LeafPackArgs& a, const unsigned block, char* __restrict__ smem) {
    static_assert(kPackLoopWords % 4u == 0u, "the closing sums behind the loop's region are doubles");
    uint32_t* const tables = reinterpret_cast<uint32_t*>(smem);                 // the cursor loop: the leaves' copy runs
    uint32_t* const poff = tables;                                              // the expanded loop: the pair offsets (same region)
    uint32_t (*op_end)[kPackMaxOps + 1] = reinterpret_cast<uint32_t (*)[kPackMaxOps + 1]>(tables);
    uint32_t (*op_base)[kPackMaxOps + 1] = reinterpret_cast<uint32_t (*)[kPackMaxOps + 1]>(tables + kPackMaxSubs * (kPackMaxOps + 1));
    const unsigned lane = threadIdx.x;
    const PackBlock* __restrict__ bp = a.blocks + block;
    const uint32_t w = bp->w, inv_w = bp->inv_w, P = bp->P, n_sub = bp->n_sub, sub_lo = bp->sub_lo, T = bp->trips;   // wave-uniform
    const unsigned sub = (lane * inv_w) >> 16, lw = lane - sub * w;   // w is 4, 6, 8 or 16: 64 / w leaves; the lanes left over (w = 6: four) hold no leaf
    PackSub my = PackSub{0u, 0u, 0u, 0u};
    if (sub < n_sub) my = a.subs[sub_lo + sub];
    // TWO targets per lane (t and t + W): a loaded source pair is used twice, and the loop's bookkeeping is shared by four terms
    const uint32_t W = my.count ? (my.count + 1u) >> 1 : 1u;       // lanes per group
    // lw / W through fp32, as above ((lw + 0.5) / W is at least 1/32 away from an integer)
    const unsigned g_raw = (unsigned)(((float)lw + 0.5f) * __builtin_amdgcn_rcpf((float)W));
    const unsigned t = lw - g_raw * W;
    const bool valid = my.count != 0u && g_raw < P;
    const bool valid1 = valid && t + W < my.count;                 // a leaf of odd size: its last lane holds one target
    const unsigned g = valid ? g_raw : 0u;
    const uint32_t pslot0 = my.first + (valid ? t : 0u), pslot1 = valid1 ? pslot0 + W : pslot0;
    const char* __restrict__ const xp_bytes = reinterpret_cast<const char*>(a.xp);   // 32-bit byte offsets from a scalar base: the plan packs nothing beyond 2^28 units
    const float* __restrict__ xf0 = reinterpret_cast<const float*>(xp_bytes + ((pslot0 >> 1) * 32u + (pslot0 & 1u) * 4u));
    const float* __restrict__ xf1 = reinterpret_cast<const float*>(xp_bytes + ((pslot1 >> 1) * 32u + (pslot1 & 1u) * 4u));
    float ix = 0.f, iy = 0.f, iz = 0.f, jx = 0.f, jy = 0.f, jz = 0.f;
    if (my.count) { ix = xf0[0]; iy = xf0[2]; jx = xf1[0]; jy = xf1[2]; if (D == 3) { iz = xf0[4]; jz = xf1[4]; } }
    const f2 ix2 = {ix, ix}, iy2 = {iy, iy}, iz2 = {iz, iz}, jx2 = {jx, jx}, jy2 = {jy, jy}, jz2 = {jz, jz};
    // lanes of an unused leaf slot hold no target: they must not drag the wave into the guarded loop
    auto close = [](const float x, const float y, const float z) { return !(__builtin_fabsf(x) >= kCloseCoord && __builtin_fabsf(y) >= kCloseCoord && (D == 2 || __builtin_fabsf(z) >= kCloseCoord)); };
    const bool in_close_set = my.count != 0u && (close(ix, iy, iz) || close(jx, jy, jz));
    // the softened law has no special case: every wave runs the unguarded form, whatever its targets and the masses
    const bool safe = LAW == NBX_LAW_NEWTON || (__builtin_amdgcn_ballot_w64(in_close_set) == 0ull && *a.max_mass_bits <= __builtin_bit_cast(uint32_t, (float)kFastMaxMass));
    // this leaf's copy runs, as {end of the run in the stream, byte offset of the run's first unit minus 16 x its stream position}
    // (32-bit byte offsets from a scalar base: the plan packs nothing beyond 2^28 units), and behind the last one the PAD RUN:
    // it never ends, and every position of it is the launch's pad pair (its positions are masked to zero)
    const uint32_t PT = P * T;                                     // entries of a leaf's row = pairs its lane groups walk between them
    const bool expanded = T != 0u && n_sub * PT <= kPackExpand;    // wave-uniform
    if (!expanded) {                                               // the cursor loop's run tables
        for (unsigned k = lw; k < my.op_n; k += w) {
            const CopyOp o = a.ops[my.op_lo + k];
            op_end[sub][k] = o.end;
            op_base[sub][k] = o.base << 4;
        }
        if (lw == 0u) { op_end[sub][my.op_n] = 0xffffffffu; op_base[sub][my.op_n] = a.pslots << 4; }
    }
    Sums<D> S0, S1;
    bool flushed = false;                                          // wave-uniform: the fp64 sums hold something (they are not zeroed: the first flush stores)
    double* const osum = reinterpret_cast<double*>(smem + kPackLoopWords * 4u);   // [component][second target? 64 : 0][lane]
    S0.o = osum + lane;
    S1.o = osum + 64u + lane;
    S0.stride = S1.stride = 128u;
    if (!expanded) __syncthreads();                                // the run tables (one wave: cheap)
    // The cursor k only ever moves forward; the run it is in sits in registers.  A lane without a leaf starts (and stays) in a pad
    // run of its own.
    unsigned k = 0;
    uint32_t run_end = my.count ? 0u : 0xffffffffu, run_off = a.pslots << 4, run_mask = 0u;
    auto offset_of = [&](const uint32_t v) -> uint32_t {           // byte offset of the pair at stream position v (even)
        while (v >= run_end) {                                     // rare (a run is ~3 leaves); the pad run ends the search
            run_end = op_end[sub][k];
            run_off = op_base[sub][k];
            run_mask = k == my.op_n ? 0u : 0xffffffffu;
            ++k;
        }
        return ((v & run_mask) << 4) + run_off;                    // a run is whole leaves, a leaf whole pairs: both units of the pair
    };
    static_assert(kPackPairsPerTrip == 2, "the loops below");
    // one form of the pair term per wave (GUARD: a special case of the law is possible for one of this wave's targets)
    auto compute_with = [&](auto guard, const float4 (&A)[2], const float4 (&B)[2]) {
        constexpr bool GUARD = decltype(guard)::value && LAW != NBX_LAW_NEWTON;
        const f2 bias = LAW == NBX_LAW_NEWTON ? f2{a.eps2, a.eps2} : GUARD ? f2{0.f, 0.f} : f2{kTiny, kTiny};
        auto term = [&](const float4 A1, const float4 B1, const f2 x2, const f2 y2, const f2 z2, Sums<D>& S) {
            const PairTerm<D> q(A1, B1, x2, y2, z2, bias);
            f2 wgt;
            if (GUARD && __builtin_expect(q.template special<LAW>() != 0ull, 0)) wgt = q.template guarded<LAW>();
            else wgt = q.template plain<LAW, true>();
            S.add(q, wgt);
        };
        if (S0.pending + 4u > kFlushTerms) {
            if (flushed) { S0.flush(); S1.flush(); } else { S0.store(); S1.store(); flushed = true; }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            term(A[j], B[j], ix2, iy2, iz2, S0);
            term(A[j], B[j], jx2, jy2, jz2, S1);
        }
        S0.pending += 4u;
    };
    if (expanded) {
        // every lane of a leaf fills the entries q = lw, lw + w, ... of its leaf's row; lanes without a leaf fill the slack behind the
        // last row (the loop's read-ahead must find loadable offsets there) and walk row 0 (their sums are never stored)
        // RUN by run, straight from the plan's copy runs (no tables, no search): lane lw of a leaf takes its runs lw, lw + w, ... and
        // writes their pairs' offsets (consecutive records, 32 bytes apart), then its share of the pad entries behind the stream's end
        const uint32_t row = sub < n_sub ? sub * PT : 0u;
        const uint32_t pad_off = a.pslots << 4;
        if (sub < n_sub) {
            for (uint32_t r = lw; r < my.op_n; r += w) {
                const CopyOp o = a.ops[my.op_lo + r];
                const uint32_t begin = r ? a.ops[my.op_lo + r - 1u].end : 0u;
                uint32_t off = (o.base + begin) << 4;              // the run's first unit
                for (uint32_t q = begin >> 1; q < (o.end >> 1); ++q, off += 32u) poff[row + q] = off;
            }
            const uint32_t stream_pairs = my.op_n ? a.ops[my.op_lo + my.op_n - 1u].end >> 1 : 0u;   // <= PT: T covers the wave's longest stream
            for (uint32_t q = stream_pairs + lw; q < PT; q += w) poff[row + q] = pad_off;
        }
        if (lane < kPackExpandSlack) poff[n_sub * PT + lane] = pad_off;
        __syncthreads();
        const uint2* __restrict__ const mine = reinterpret_cast<const uint2*>(poff + row + g * T);   // T and PT are even: 8-byte aligned
        auto issue = [&](const uint2 o, float4 (&A)[2], float4 (&B)[2]) {
            const float4* __restrict__ s0 = reinterpret_cast<const float4*>(xp_bytes + o.x);
            const float4* __restrict__ s1 = reinterpret_cast<const float4*>(xp_bytes + o.y);
            A[0] = s0[0]; B[0] = s0[1];
            A[1] = s1[0]; B[1] = s1[1];
        };
        auto run = [&](auto guard) {
            float4 A0[2], B0[2], A1[2], B1[2];
            uint2 o_now = mine[0], o_next = mine[1];               // the offsets run one stage ahead of the loads they address
            issue(o_now, A0, B0);
            uint32_t i = 0;
            for (; i + 4u <= T; i += 4u) {                         // loads past the share's end fetch the next share's pairs or the pad pair: not used
                issue(o_next, A1, B1);
                o_now = mine[(i >> 1) + 2u];
                compute_with(guard, A0, B0);
                issue(o_now, A0, B0);
                o_next = mine[(i >> 1) + 3u];
                compute_with(guard, A1, B1);
            }
            if (i < T) compute_with(guard, A0, B0);                // T is even: the last two pairs
        };
        // Leaves of 3-4 bodies (two lanes to a lane group, which read the same records): the loads are what limits their waves (texture
        // address unit 71 % busy, VALU 46 %: profiles/r5/pmc_pack_kernel.txt), so the two lanes of a group load ONE half of each
        // 32-byte record each -- the even lane {xa,xb,ya,yb}, the odd lane {za,zb,ma,mb} -- and hand it to each other with DPP moves
        // (quad_perm: a leaf's four lanes are one quad): half the load instructions for 16 more moves per loop body of 52.
        // Measured and lost (profiles/r5/leaf_small_leaves.txt): the same exchange for EVERY class through ds_bpermute_b32 (no VALU
        // instruction added, but its latency sits between the loads and the arithmetic): 8-body leaves 0.315 -> 0.265, 4-body cells 0.161 -> 0.152.
        auto run_shared = [&](auto guard) {
            const uint32_t half = (lane & 1u) << 4;                // this lane's half of a record
            auto issue_half = [&](const uint2 o, float4 (&H)[2]) {
                H[0] = *reinterpret_cast<const float4*>(xp_bytes + (o.x + half));
                H[1] = *reinterpret_cast<const float4*>(xp_bytes + (o.y + half));
            };
            auto from_even = [](const float v) { return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xA0, 0xF, 0xF, true)); };   // quad_perm:[0,0,2,2]
            auto from_odd = [](const float v) { return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xF5, 0xF, 0xF, true)); };    // quad_perm:[1,1,3,3]
            auto compute_halves = [&](const float4 (&H)[2]) {
                float4 A[2], B[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    A[j] = make_float4(from_even(H[j].x), from_even(H[j].y), from_even(H[j].z), from_even(H[j].w));
                    B[j] = make_float4(from_odd(H[j].x), from_odd(H[j].y), from_odd(H[j].z), from_odd(H[j].w));
                }
                compute_with(guard, A, B);
            };
            float4 H0[2], H1[2];
            uint2 o_now = mine[0], o_next = mine[1];
            issue_half(o_now, H0);
            uint32_t i = 0;
            for (; i + 4u <= T; i += 4u) {
                issue_half(o_next, H1);
                o_now = mine[(i >> 1) + 2u];
                compute_halves(H0);
                issue_half(o_now, H0);
                o_next = mine[(i >> 1) + 3u];
                compute_halves(H1);
            }
            if (i < T) compute_halves(H0);
        };
        if (bp->shape == 1u && w == 4u && P == 2u) {               // wave-uniform: every leaf of the wave has W = 2 lanes per group
            if (safe) run_shared(std::false_type{});
            else run_shared(std::true_type{});
        } else if (safe) run(std::false_type{});
        else run(std::true_type{});
    } else if (T) {
        // the cursor loop (rounds 3-4): lane group g walks stream positions [2 g T, 2 (g + 1) T) of its leaf straight from the run tables
        if (!valid) { run_end = 0xffffffffu; run_off = a.pslots << 4; run_mask = 0u; }   // no target: a pad run of its own
        const uint32_t v_begin = 2u * g * T;
        auto issue = [&](const uint32_t i, float4 (&A)[2], float4 (&B)[2]) {   // pairs i and i + 1 of this lane's share
            const uint32_t v = v_begin + 2u * i;
            const uint32_t o0 = offset_of(v), o1 = offset_of(v + 2u);
            const float4* __restrict__ s0 = reinterpret_cast<const float4*>(xp_bytes + o0);
            const float4* __restrict__ s1 = reinterpret_cast<const float4*>(xp_bytes + o1);
            A[0] = s0[0]; B[0] = s0[1];
            A[1] = s1[0]; B[1] = s1[1];
        };
        auto run = [&](auto guard) {
            float4 A0[2], B0[2], A1[2], B1[2];
            issue(0u, A0, B0);
            // One back edge, no exit in the middle: with a `break` between the halves the compiler waits for EVERY outstanding load at
            // the loop head (s_waitcnt vmcnt(0)); this way it waits for the four older ones only, the reload stays in flight.
            uint32_t i = 0;
            for (; i + 4u <= T; i += 4u) {                         // loads past the share's end fetch the next share's pairs or the pad pair: not used
                issue(i + 2u, A1, B1);
                compute_with(guard, A0, B0);
                issue(i + 4u, A0, B0);
                compute_with(guard, A1, B1);
            }
            if (i < T) compute_with(guard, A0, B0);                // T is even: the last two pairs
        };
        if (safe) run(std::false_type{});
        else run(std::true_type{});
    }
    if (flushed) { S0.flush(); S1.flush(); } else { S0.store(); S1.store(); }   // T = 0: zeros are stored
    __syncthreads();
    if (valid && g == 0u) {
        const unsigned l0 = sub * w + t;
        for (unsigned h = 0; h < (valid1 ? 2u : 1u); ++h) {
            double ox = 0.0, oy = 0.0, oz = 0.0;
            for (unsigned q = 0; q < P; ++q) { ox += osum[64u * h + l0 + q * W]; oy += osum[128u + 64u * h + l0 + q * W]; oz += osum[256u + 64u * h + l0 + q * W]; }
            const uint32_t pslot = h ? pslot1 : pslot0;
            a.acc[pslot] = ox;
            a.acc[(size_t)a.pslots + pslot] = oy;
            if (D == 3) a.acc[2 * (size_t)a.pslots + pslot] = oz;
        }
    }
}

template <int D, int LAW>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NBX_PACK_WAVES, 8))) void leaf_pack_kernel(LeafPackArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[kPackSmemBytes];
    leaf_pack_body<D, LAW>(a, blockIdx.x, smem);
}

// A structure with BOTH kinds of workgroups -- packed waves and a few one-leaf workgroups (leaves whose lists have too many runs to
// pack) -- in ONE launch: the first n_one workgroups are the one-leaf ones (the long ones: dispatched first), the others the packed
// waves.  Two launches ran the 25 one-leaf workgroups of an 8-body structure alone for 8.7 us ahead of 85 us of packed waves
// (profiles/r4/leaf_kernel_stats_final_8body.csv).  Both bodies use the same 64 lanes and the same LDS (the larger of the two).
template <int D, int LAW>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NBX_PACK_WAVES, 8))) void leaf_fused_kernel(LeafArgs one, LeafPackArgs pack, uint32_t n_one) {
    constexpr unsigned kBytes = pair_smem_bytes<1>() > kPackSmemBytes ? pair_smem_bytes<1>() : kPackSmemBytes;
    __shared__ __attribute__((aligned(16))) char smem[kBytes];
    if (blockIdx.x < n_one) leaf_pair_body<D, LAW, 1>(one, blockIdx.x, smem);
    else leaf_pack_body<D, LAW>(pack, blockIdx.x - n_one, smem);
}

// The call's largest |mass| (as fp32 bits) into one word: the block's maximum through LDS, then ONE lane per block, and only when an
// ordinary (cached) read of the word says the block's maximum is above it.  16,384 atomics on the word cost 0.15 ms; so did 16,384
// atomic LOADS of it (one L2 channel serves them one after the other) -- the resident gather spent 0.12 of its 0.14 ms there.  A stale
// read only costs a superfluous atomicMax; the atomic decides.
__device__ __forceinline__ void publish_max_mass(uint32_t wave_max, uint32_t* __restrict__ max_mass_bits) {
    __shared__ uint32_t block_max[4];
    if ((threadIdx.x & 63u) == 0u) block_max[threadIdx.x >> 6] = wave_max;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t m = block_max[0];
        for (unsigned w = 1; w < (blockDim.x + 63u) / 64u; ++w) m = block_max[w] > m ? block_max[w] : m;
        if (m > *static_cast<volatile const uint32_t*>(max_mass_bits)) atomicMax(max_mass_bits, m);
    }
}

// the launch's pad pair, behind the last leaf's slots (pslots is even: every leaf is padded to whole pairs); the arrays' arena keeps
// 256 bytes of slack behind each of them
__device__ __forceinline__ void write_pad_pair(float* __restrict__ xp, uint32_t pslots, int dim) {
    float* __restrict__ o = xp + (size_t)pslots * 4u;
    const float zc = dim == 3 ? kFar : 0.0f;
    o[0] = kFar; o[1] = kFar; o[2] = kFar; o[3] = kFar; o[4] = zc; o[5] = zc; o[6] = 0.0f; o[7] = 0.0f;
}

// staged Body<D> AoS fp64 (host order) -> leaf-ordered source pairs, fp32; a padded slot without a body is massless and far away
__global__ __launch_bounds__(256) void leaf_gather_kernel(const double* __restrict__ raw, size_t stride_d, int dim,
                                                          const uint32_t* __restrict__ pslot_body, uint32_t pslots, float* __restrict__ xp,
                                                          uint32_t* __restrict__ max_mass_bits) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const uint32_t body = p < pslots ? pslot_body[p] : 0xffffffffu;
    float x = kFar, y = kFar, z = dim == 3 ? kFar : 0.0f, m = 0.0f;
    if (body != 0xffffffffu) {
        const double* __restrict__ b = raw + (size_t)body * stride_d;
        x = (float)b[0]; y = (float)b[1]; z = dim == 3 ? (float)b[2] : 0.0f; m = (float)b[2 * dim];
    }
    // largest |mass| of the call: non-negative fp32 order like their bit patterns, a NaN above them all
    uint32_t mb = __builtin_bit_cast(uint32_t, __builtin_fabsf(m));
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)mb, d);
        mb = other > mb ? other : mb;
    }
    // one lane per wave, and only while the wave's maximum is above what is already there (16,384 atomics on one word cost 0.15 ms)
    publish_max_mass(mb, max_mass_bits);
    if (p == 0u) write_pad_pair(xp, pslots, dim);
    if (p >= pslots) return;
    float* __restrict__ o = xp + (size_t)(p >> 1) * 8u + (p & 1u);
    o[0] = x; o[2] = y; o[4] = z; o[6] = m;
}

// forces_out[body] = sign * (G m_body) * acc[slot]   (fp64; every body belongs to at most one leaf)
__global__ __launch_bounds__(256) void leaf_scatter_kernel(const double* __restrict__ acc, const double* __restrict__ raw, size_t stride_d,
                                                           int dim, const uint32_t* __restrict__ pslot_body, uint32_t pslots, double signedG,
                                                           double* __restrict__ forces) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= pslots) return;
    const uint32_t body = pslot_body[p];
    if (body == 0xffffffffu) return;
    const double gm = signedG * raw[(size_t)body * stride_d + 2 * dim];
    for (int k = 0; k < dim; ++k) forces[(size_t)body * dim + k] = gm * acc[(size_t)k * pslots + p];
}

// ---- kernels of the device-resident plan (nbx_leaf_plan_*) ----
// resident fp32 SoA (a single-shard context's source copy: pos[dim][pad], mass[pad]) -> leaf-ordered source pairs, BODY-major: one
// lane per body reads its coordinates and mass coalesced and writes its slot's 16 bytes (four words of one 32-byte pair record).  Slot-major, every slot's four words came from four different cache lines of the SoA arrays (0.106 ms at
// N = 2^20, a quarter of an evaluation); this way the scattered side is one 32-byte sector per body.  Pad slots are written once, at plan
// creation (leaf_init_pads_kernel): nothing here touches them.
__global__ __launch_bounds__(256) void leaf_gather_by_body_kernel(const float* __restrict__ pos, const float* __restrict__ mass, unsigned pad, int dim,
                                                                  const uint32_t* __restrict__ body_slot, size_t n, float* __restrict__ xp,
                                                                  uint32_t* __restrict__ max_mass_bits) {
    const size_t b = (size_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t slot = 0xffffffffu;
    float x = 0.f, y = 0.f, z = 0.f, m = 0.f;
    if (b < n) {
        slot = body_slot[b];
        if (slot != 0xffffffffu) { x = pos[b]; y = pos[(size_t)pad + b]; z = dim == 3 ? pos[2 * (size_t)pad + b] : 0.0f; m = mass[b]; }
    }
    uint32_t mb = __builtin_bit_cast(uint32_t, __builtin_fabsf(m));   // bodies in no leaf are no sources: they do not count (m = 0)
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)mb, d);
        mb = other > mb ? other : mb;
    }
    publish_max_mass(mb, max_mass_bits);
    if (slot == 0xffffffffu) return;
    float* __restrict__ o = xp + (size_t)(slot >> 1) * 8u + (slot & 1u);
    o[0] = x; o[2] = y; o[4] = z; o[6] = m;
}

__global__ __launch_bounds__(256) void leaf_init_pads_kernel(const uint32_t* __restrict__ pslot_body, uint32_t pslots, int dim, float* __restrict__ xp) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p == 0u) write_pad_pair(xp, pslots, dim);
    if (p >= pslots || pslot_body[p] != 0xffffffffu) return;
    float* __restrict__ o = xp + (size_t)(p >> 1) * 8u + (p & 1u);
    o[0] = kFar; o[2] = kFar; o[4] = dim == 3 ? kFar : 0.0f; o[6] = 0.0f;   // a leaf's pad: massless and far away
}

// forces[body] = (signedG m_body) * sums[slot of body], one lane per body (every entry written: zero for a body in no leaf);
// the mass comes from mass[body * mass_stride] -- a context's m64 (stride 1) or the staged Body<D> array (offset 2 dim, stride the body's)
__global__ __launch_bounds__(256) void leaf_forces_by_body_kernel(const double* __restrict__ sums, uint32_t pslots, const uint32_t* __restrict__ body_slot,
                                                                  size_t n, int dim, double signedG, const double* __restrict__ mass, size_t mass_stride,
                                                                  double* __restrict__ forces) {
    const size_t b = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= n) return;
    const uint32_t slot = body_slot[b];
    const double gm = signedG * mass[b * mass_stride];
    for (int k = 0; k < dim; ++k) forces[b * dim + k] = slot == 0xffffffffu ? 0.0 : gm * sums[(size_t)k * pslots + slot];
}

typedef void (*LeafKernel)(LeafArgs);
LeafKernel pick(int dim, int law, int waves) {
    static const LeafKernel table[2][2][4] = {
        {{leaf_pair_kernel<2, NBX_LAW_BRUTE, 1>, leaf_pair_kernel<2, NBX_LAW_TREE_LEAF, 1>, leaf_pair_kernel<2, NBX_LAW_FMM_P2P, 1>, leaf_pair_kernel<2, NBX_LAW_NEWTON, 1>},
         {leaf_pair_kernel<3, NBX_LAW_BRUTE, 1>, leaf_pair_kernel<3, NBX_LAW_TREE_LEAF, 1>, leaf_pair_kernel<3, NBX_LAW_FMM_P2P, 1>, leaf_pair_kernel<3, NBX_LAW_NEWTON, 1>}},
        {{leaf_pair_kernel<2, NBX_LAW_BRUTE, 2>, leaf_pair_kernel<2, NBX_LAW_TREE_LEAF, 2>, leaf_pair_kernel<2, NBX_LAW_FMM_P2P, 2>, leaf_pair_kernel<2, NBX_LAW_NEWTON, 2>},
         {leaf_pair_kernel<3, NBX_LAW_BRUTE, 2>, leaf_pair_kernel<3, NBX_LAW_TREE_LEAF, 2>, leaf_pair_kernel<3, NBX_LAW_FMM_P2P, 2>, leaf_pair_kernel<3, NBX_LAW_NEWTON, 2>}}};
    return table[waves - 1][dim - 2][law];
}

typedef void (*PackKernel)(LeafPackArgs);
PackKernel pick_pack(int dim, int law) {
    static const PackKernel table[2][4] = {
        {leaf_pack_kernel<2, NBX_LAW_BRUTE>, leaf_pack_kernel<2, NBX_LAW_TREE_LEAF>, leaf_pack_kernel<2, NBX_LAW_FMM_P2P>, leaf_pack_kernel<2, NBX_LAW_NEWTON>},
        {leaf_pack_kernel<3, NBX_LAW_BRUTE>, leaf_pack_kernel<3, NBX_LAW_TREE_LEAF>, leaf_pack_kernel<3, NBX_LAW_FMM_P2P>, leaf_pack_kernel<3, NBX_LAW_NEWTON>}};
    return table[dim - 2][law];
}

typedef void (*FusedKernel)(LeafArgs, LeafPackArgs, uint32_t);
FusedKernel pick_fused(int dim, int law) {
    static const FusedKernel table[2][4] = {
        {leaf_fused_kernel<2, NBX_LAW_BRUTE>, leaf_fused_kernel<2, NBX_LAW_TREE_LEAF>, leaf_fused_kernel<2, NBX_LAW_FMM_P2P>, leaf_fused_kernel<2, NBX_LAW_NEWTON>},
        {leaf_fused_kernel<3, NBX_LAW_BRUTE>, leaf_fused_kernel<3, NBX_LAW_TREE_LEAF>, leaf_fused_kernel<3, NBX_LAW_FMM_P2P>, leaf_fused_kernel<3, NBX_LAW_NEWTON>}};
    return table[dim - 2][law];
}

}  // namespace

// ---- the launch interface (leaf_near.h) ----
namespace nbx_near {

hipError_t enqueue_near(const NearDevice& d, int dim, int law, hipStream_t s, bool fuse) {
    LeafArgs a;
    a.xp = d.xp; a.pslots = d.pslots; a.ops = d.ops; a.blocks = d.blocks; a.acc = d.sums; a.max_mass_bits = d.max_mass; a.eps2 = d.eps2;
    LeafPackArgs pa;
    pa.xp = d.xp; pa.pslots = d.pslots; pa.ops = d.ops; pa.blocks = d.packs; pa.subs = d.subs; pa.acc = d.sums; pa.max_mass_bits = d.max_mass; pa.eps2 = d.eps2;
    if (fuse && d.n_blocks && d.n_packs && d.waves == 1) {   // both kinds (packing implies one-wave workgroups): one launch, the one-leaf workgroups first
        hipLaunchKernelGGL(pick_fused(dim, law), dim3((unsigned)(d.n_blocks + d.n_packs)), dim3(64), 0, s, a, pa, (uint32_t)d.n_blocks);
        return hipGetLastError();
    }
    if (d.n_blocks) {
        hipLaunchKernelGGL(pick(dim, law, d.waves), dim3((unsigned)d.n_blocks), dim3(64u * (unsigned)d.waves), 0, s, a);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    if (d.n_packs) hipLaunchKernelGGL(pick_pack(dim, law), dim3((unsigned)d.n_packs), dim3(64), 0, s, pa);
    return hipGetLastError();
}

static dim3 grid256(size_t items) { return dim3((unsigned)((items + 255) / 256)); }

hipError_t enqueue_gather_staged(const double* raw, size_t stride_d, int dim, const uint32_t* pslot_body, size_t pslots, float4* xp, uint32_t* max_mass,
                                 hipStream_t s) {
    hipLaunchKernelGGL(leaf_gather_kernel, grid256(pslots), dim3(256), 0, s, raw, stride_d, dim, pslot_body, (uint32_t)pslots, reinterpret_cast<float*>(xp), max_mass);
    return hipGetLastError();
}
hipError_t enqueue_gather_resident(const float* pos, const float* mass, unsigned pad, int dim, const uint32_t* body_slot, size_t n, float4* xp,
                                   uint32_t* max_mass, hipStream_t s) {
    hipLaunchKernelGGL(leaf_gather_by_body_kernel, grid256(n), dim3(256), 0, s, pos, mass, pad, dim, body_slot, n, reinterpret_cast<float*>(xp), max_mass);
    return hipGetLastError();
}
hipError_t enqueue_init_pads(const uint32_t* pslot_body, size_t pslots, int dim, float4* xp, hipStream_t s) {
    hipLaunchKernelGGL(leaf_init_pads_kernel, grid256(pslots), dim3(256), 0, s, pslot_body, (uint32_t)pslots, dim, reinterpret_cast<float*>(xp));
    return hipGetLastError();
}
hipError_t enqueue_scatter(const double* sums, const double* raw, size_t stride_d, int dim, const uint32_t* pslot_body, size_t pslots, double signedG,
                           double* forces, hipStream_t s) {
    hipLaunchKernelGGL(leaf_scatter_kernel, grid256(pslots), dim3(256), 0, s, sums, raw, stride_d, dim, pslot_body, (uint32_t)pslots, signedG, forces);
    return hipGetLastError();
}
hipError_t enqueue_forces_by_body(const double* sums, size_t pslots, const uint32_t* body_slot, size_t n, int dim, double signedG, const double* mass,
                                  size_t mass_stride, double* forces, hipStream_t s) {
    hipLaunchKernelGGL(leaf_forces_by_body_kernel, grid256(n), dim3(256), 0, s, sums, (uint32_t)pslots, body_slot, n, dim, signedG, mass, mass_stride, forces);
    return hipGetLastError();
}

}  // namespace nbx_near
