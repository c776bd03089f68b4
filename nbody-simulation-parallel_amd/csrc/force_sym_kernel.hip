// force_sym_kernel.hip -- K1-S: the symmetric own-shard force pass for gfx950 (MI355X), fp32, D = 2 or 3.
//
// The one-sided kernels (force_kernel.hip) evaluate every ORDERED pair: d, r^2, the reciprocal and its square are computed
// twice per pair of bodies.  This pass computes them once per UNORDERED pair and uses them for both bodies (Newton's third
// law; per two unordered pairs 16 v_pk + 2 v_rcp for FOUR pair terms against 2 x (11 v_pk + 2 v_rcp)).  It applies where
// the sources of a pass are exactly the context's own bodies and nothing is accumulated onto an earlier pass (a
// single-shard context); the decomposition is in sym_plan.h.
//
//   * A wave holds 512 HOME bodies, 8 per lane as 4 float2 pairs with their masses, like the one-sided fast kernels.
//   * D = 2: it takes 64 VISITORS, one per lane: {x, y}, {z, m} and a float2 x 3 reaction accumulator.  One step = the fast
//     kernel's loop body with the source operands read from the lane's visitor registers instead of an LDS broadcast, plus
//     the multiply by the home masses and 3 v_pk_fma_f32 into the visitor's accumulator.  Then the visitor and its
//     accumulator move one lane on.  After 64 steps every home body has met every visitor and every visitor is back in
//     its lane.  No LDS broadcast, no barrier and no cross-lane reduction in the pair loop.
//   * D = 3: it takes 128 visitors, TWO per lane (SymLanes): a float2 holds the same position of two consecutive groups of a
//     chunk against one home body, which op_sel broadcasts from its pair.  The arithmetic per pair term is the same; a
//     step is 8 home bodies x 2 visitors, and the float2 x 3 accumulator carries two visitors' sums.
//   * The rotation (template parameter ROT).  The accumulator changes every step and moves by v_mov_b32_dpp wave_ror:1
//     (6 moves per step: per 8 pair terms at D = 2, per 16 at D = 3).  The visitors' {x, y, z, m} never change during a rotation:
//       kRotLds: the wave writes its visitors once per rotation into a wave-private LDS buffer and every lane reads the
//                next step's visitor (D = 3: visitor pair) with one (two) ds_read_b128, issued one step ahead -- the VALU is
//                the saturated pipe, the LDS pipe is idle.  A wave's LDS operations complete in order and nobody else
//                touches the buffer: no barrier.
//       kRotDpp: four (eight) more DPP moves per step (the comparator sympk3l_t8_w3_dpp: same values, same sums, bit for bit).
//   * Summation, three levels on both sides:
//       home:    fp32 over the 64 steps of one visitor group -> fp32 over the <= 4 groups of a chunk -> fp64 (LDS).  At D = 3
//                the two halves of a home body's float2 are the chains over groups 2j and 2j + 1, folded in that order.
//       visitor: fp32 over 8 steps (D = 2: 32 terms per float2 half, the halves added at the flush; D = 3: one chain of 64
//                terms, the lane's home bodies in register order) -> fp32 over the 8 such blocks of a rotation, kept in the
//                wave's LDS slot of that visitor -> fp64: the four waves of the workgroup, which meet the same visitors,
//                are added in wave order, and the workgroup keeps the running fp64 sum over its home passes in the planes
//                that only it writes.
//     Q (mixed mode) adds |level-1 sum|^2 on both sides.
//   * Deterministic: no atomics, every plane entry has one writer, every order is fixed by the indices.
//   * kTiny bias and close set as in the fast kernels: a flagged body's home sums are not stored, and scatter_close_kernel
//     replaces ALL its planes (the reaction slots too) by the guarded evaluation.  A pair with a flagged and an unflagged
//     body is at r^2 >= kBadR2, so the unflagged body's term is good.
#include "nbx_internal.h"
#include "sym_plan.h"

namespace nbx {
namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

// lane i receives lane i-1's value (lane 0: lane 63's)
__device__ __forceinline__ float ror1(float v) {
    const int i = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, 0x13C, 0xF, 0xF, false));
}
__device__ __forceinline__ void ror1(f2& v) { v.x = ror1(v.x); v.y = ror1(v.y); }

enum { kRotDpp = 0, kRotLds = 1 };   // how the visitor's {x, y, z, m} reach the next lane
// Visitors a lane carries.  D = 2: one, broadcast by op_sel against float2 pairs of home bodies.  D = 3: two -- a float2 holds
// the same position p of two consecutive 64-visitor groups of a chunk (.x: group 2j, .y: group 2j + 1) against ONE home body,
// which op_sel broadcasts from the {h0, h1} pairs ix / iy / iz / hm.  The reaction accumulator float2 x 3 then carries two
// visitors' sums, and its six DPP moves per step serve 16 unordered pairs instead of 8.
template <int D> struct SymLanes { static constexpr int kVisitors = (D == 3) ? 2 : 1; };
// steps between two flushes of the visitors' level-1 sums (D = 3: one fp32 chain of 8 terms per step, 64 terms per block;
// tests/sym_sum_model_pairs.cpp compares 8 with 4)
constexpr int kSymBlockSteps = 8;
// kRotLds, the wave's buffer.  With delta = +-1 the lanes' move per step, entry k holds the visitor of the lane -k * delta
// (mod 64), and the lane that starts at entry r = -lane * delta finds the visitor of step t at entry r - t: the direction
// is in the placement, the loop reads downwards whichever it is.  Entries 64 .. 71 repeat entries 0 .. 7 so that a block of
// eight steps reads base + 7 .. base + 0 without a wrap inside it; the block's base wraps.  D = 2: one plane of {x, y, z, m}.
// D = 3: two planes, {xa, xb, ya, yb} and {za, zb, ma, mb} of the lane's visitor pair, on one base register.
template <int D> struct RotBuf {
    static constexpr unsigned kEntries = 72u;
    static constexpr unsigned kPlanes = (unsigned)SymLanes<D>::kVisitors;
    static constexpr unsigned kWaveBytes = kPlanes * kEntries * (unsigned)sizeof(float4);
};

// One step with one visitor per lane (what D = 2 runs; D = 3 runs sym_step_pairs below, and this form only if SymLanes says
// so): the lane's PAIRS home pairs against the lane's visitor.  Per home pair, D = 3: v_pk_add x3, v_pk_fma x3
// (r^2 + bias), v_rcp x2, v_pk_mul (w^2), v_pk_mul x2 (the two masses), v_pk_fma x3 (home), v_pk_fma x3 (visitor) = 16 + 2.
// d = visitor - home: the home sums add m_v w^2 d; the visitor's accumulator adds m_h w^2 d and is NEGATED when it is flushed.
template <int D, int PAIRS>
__device__ __forceinline__ void sym_step(const f2 vxy, const f2 vzm, const f2 (&ix)[PAIRS], const f2 (&iy)[PAIRS],
                                         const f2 (&iz)[PAIRS], const f2 (&hm)[PAIRS], f2 (&ax)[PAIRS], f2 (&ay)[PAIRS],
                                         f2 (&az)[PAIRS], f2& vax, f2& vay, f2& vaz, const f2 bias) {
    f2 dx[PAIRS], dy[PAIRS], dz[PAIRS], r2[PAIRS], w[PAIRS], wh[PAIRS];
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) dx[q] = __builtin_shufflevector(vxy, vxy, 0, 0) - ix[q];
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) dy[q] = __builtin_shufflevector(vxy, vxy, 1, 1) - iy[q];
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) dz[q] = (D == 3) ? __builtin_shufflevector(vzm, vzm, 0, 0) - iz[q] : f2{0.f, 0.f};
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) r2[q] = __builtin_elementwise_fma(dx[q], dx[q], bias);
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) r2[q] = __builtin_elementwise_fma(dy[q], dy[q], r2[q]);
    if (D == 3) {
#pragma unroll
        for (int q = 0; q < PAIRS; ++q) r2[q] = __builtin_elementwise_fma(dz[q], dz[q], r2[q]);
    }
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) { w[q].x = __builtin_amdgcn_rcpf(r2[q].x); w[q].y = __builtin_amdgcn_rcpf(r2[q].y); }
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) r2[q] = w[q] * w[q];
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) w[q] = __builtin_shufflevector(vzm, vzm, 1, 1) * r2[q];
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) wh[q] = hm[q] * r2[q];
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) ax[q] = __builtin_elementwise_fma(w[q], dx[q], ax[q]);
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) ay[q] = __builtin_elementwise_fma(w[q], dy[q], ay[q]);
    if (D == 3) {
#pragma unroll
        for (int q = 0; q < PAIRS; ++q) az[q] = __builtin_elementwise_fma(w[q], dz[q], az[q]);
    }
    // the three components interleaved: each accumulator is touched every third instruction
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) {
        vax = __builtin_elementwise_fma(wh[q], dx[q], vax);
        vay = __builtin_elementwise_fma(wh[q], dy[q], vay);
        if (D == 3) vaz = __builtin_elementwise_fma(wh[q], dz[q], vaz);
    }
}

template <int D>
__device__ __forceinline__ void load_visitor(const float* __restrict__ tp, const float* __restrict__ mp, unsigned pad,
                                             unsigned v, f2& vxy, f2& vzm) {
    vxy = f2{tp[v], tp[(size_t)pad + v]};
    vzm = f2{(D == 3) ? tp[2 * (size_t)pad + v] : 0.0f, mp[v]};
}

template <int H> __device__ __forceinline__ f2 bcast(const f2 v) { return __builtin_shufflevector(v, v, H, H); }

// One step, D = 3, two visitors per lane: the lane's 8 home bodies, each broadcast, against the visitor pair {a, b}.  Per home
// body: v_pk_add x3, v_pk_fma x3 (r^2 + bias), v_rcp x2, v_pk_mul (w^2), v_pk_mul x2 (the visitors' masses, the home mass),
// v_pk_fma x3 (home: .x from a, .y from b), v_pk_fma x3 (the visitors) = 15 + 2, in two batches of four home bodies.  The terms are
// sym_step's; a home body's .x and .y sums are the chains sym_step builds over group 2j and group 2j + 1.  The visitors'
// accumulator takes its 8 terms per step in register order (k = 2 q + h).
__device__ __forceinline__ void sym_step_pairs(const f2 vx, const f2 vy, const f2 vz, const f2 vm, const f2 (&ix)[4],
                                               const f2 (&iy)[4], const f2 (&iz)[4], const f2 (&hm)[4], f2 (&ax)[8], f2 (&ay)[8],
                                               f2 (&az)[8], f2& vax, f2& vay, f2& vaz, const f2 bias) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        f2 dx[4], dy[4], dz[4], r2[4], w[4], wh[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) dx[k] = vx - ((k & 1) ? bcast<1>(ix[2 * b + k / 2]) : bcast<0>(ix[2 * b + k / 2]));
#pragma unroll
        for (int k = 0; k < 4; ++k) dy[k] = vy - ((k & 1) ? bcast<1>(iy[2 * b + k / 2]) : bcast<0>(iy[2 * b + k / 2]));
#pragma unroll
        for (int k = 0; k < 4; ++k) dz[k] = vz - ((k & 1) ? bcast<1>(iz[2 * b + k / 2]) : bcast<0>(iz[2 * b + k / 2]));
#pragma unroll
        for (int k = 0; k < 4; ++k) r2[k] = __builtin_elementwise_fma(dx[k], dx[k], bias);
#pragma unroll
        for (int k = 0; k < 4; ++k) r2[k] = __builtin_elementwise_fma(dy[k], dy[k], r2[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) r2[k] = __builtin_elementwise_fma(dz[k], dz[k], r2[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) { w[k].x = __builtin_amdgcn_rcpf(r2[k].x); w[k].y = __builtin_amdgcn_rcpf(r2[k].y); }
#pragma unroll
        for (int k = 0; k < 4; ++k) r2[k] = w[k] * w[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = vm * r2[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) wh[k] = ((k & 1) ? bcast<1>(hm[2 * b + k / 2]) : bcast<0>(hm[2 * b + k / 2])) * r2[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) ax[4 * b + k] = __builtin_elementwise_fma(w[k], dx[k], ax[4 * b + k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) ay[4 * b + k] = __builtin_elementwise_fma(w[k], dy[k], ay[4 * b + k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) az[4 * b + k] = __builtin_elementwise_fma(w[k], dz[k], az[4 * b + k]);
        // the three components interleaved: each accumulator is touched every third instruction
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            vax = __builtin_elementwise_fma(wh[k], dx[k], vax);
            vay = __builtin_elementwise_fma(wh[k], dy[k], vay);
            vaz = __builtin_elementwise_fma(wh[k], dz[k], vaz);
        }
        if (b == 0) __builtin_amdgcn_sched_barrier(0);   // one batch at a time: interleaving the two only costs registers
    }
}

// The home bodies stay the {h0, h1} pairs they are, broadcast by op_sel where they are used: left to itself the compiler
// hoists the broadcasts out of the loops as 32 more registers ({h0, h0} and {h1, h1} of every pair) and spills.  The pairs
// pass through an empty asm in front of every step; no instruction.
__device__ __forceinline__ void keep_packed(f2 (&ix)[4], f2 (&iy)[4], f2 (&iz)[4], f2 (&hm)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(ix[q]), "+v"(iy[q]), "+v"(iz[q]), "+v"(hm[q]));
}

// D = 3: position v of one group in .x, of the next group in .y
__device__ __forceinline__ void load_visitor_pair(const float* __restrict__ tp, const float* __restrict__ mp, unsigned pad,
                                                  unsigned v, f2& vx, f2& vy, f2& vz, f2& vm) {
    vx = f2{tp[v], tp[v + kSymGroup]};
    vy = f2{tp[(size_t)pad + v], tp[(size_t)pad + v + kSymGroup]};
    vz = f2{tp[2 * (size_t)pad + v], tp[2 * (size_t)pad + v + kSymGroup]};
    vm = f2{mp[v], mp[v + kSymGroup]};
}

__device__ __forceinline__ void store_hi_lo(float* __restrict__ hi_plane, float* __restrict__ lo_plane, size_t idx, double v) {
    const float hi = (float)v;
    hi_plane[idx] = hi;
    lo_plane[idx] = (float)(v - (double)hi);
}

// grid = (B super-blocks, S slices), 256 lanes.  acc = [S + K slots][{hi, lo}][D][pad], qsum = [S + K slots][pad].
template <int D, int QS, int ROT>
__global__ __launch_bounds__(256, 2) void accel_sym3l_kernel(KArgs a) {
    constexpr int PAIRS = 4;
    constexpr unsigned kSumBytes = (unsigned)PAIRS * D * 256u * sizeof(double2);          // home level 3: [PAIRS*D][256] double2
    constexpr unsigned kVisBytes = 4u * kSymChunkGroups * kSymGroup * sizeof(float4);     // visitor level 2: [wave][group][visitor] {x, y, z, Q}
    constexpr int VPL = SymLanes<D>::kVisitors;
    constexpr unsigned kRotEntries = RotBuf<D>::kEntries;
    constexpr unsigned kRotBytes = (ROT == kRotLds) ? 4u * RotBuf<D>::kWaveBytes : 0u;   // rotation: [wave][plane][entry]
    __shared__ __attribute__((aligned(16))) char smem[kSumBytes + kVisBytes + kRotBytes];
    double2* __restrict__ sums = reinterpret_cast<double2*>(smem);
    float4* __restrict__ vbuf = reinterpret_cast<float4*>(smem + kSumBytes);

    SymPlan P;
    if (!sym_make_plan(a.pad, &P) || P.B != gridDim.x || P.S != gridDim.y) return;   // the launcher checked; a guard, not a path
    if (VPL == 2 && P.G < 2u) return;   // every plan has S <= 64 (K >= 1): a chunk is 2 or 4 groups.  A guard likewise
    const unsigned A = blockIdx.x, s = blockIdx.y;
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // measurement only, as in accel_fast3l_kernel (a.clk is null in every other launch): the shader clock this workgroup held
    unsigned long long clk_r0 = 0, clk_t0 = 0;
    if (a.clk) {
        clk_r0 = __builtin_amdgcn_s_memrealtime();
        clk_t0 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_s_waitcnt(0xC07F);
    }
    const size_t pad = a.pad;
    const float* __restrict__ tp = a.pos_all + (size_t)a.tgt_chunk * D * pad;
    const float* __restrict__ mp = a.mass_all + (size_t)a.tgt_chunk * pad;
    const f2 bias = f2{kTiny, kTiny};
    const size_t slot_stride = 2 * (size_t)D * pad;   // floats between the hi planes of consecutive slots

    // after t moves a lane holds the visitor that started (t * delta) lanes further on (mod 64); delta is read off the move itself
    const unsigned delta = ((unsigned)__builtin_amdgcn_update_dpp((int)lane, (int)lane, 0x13C, 0xF, 0xF, false) - lane) & 63u;
    // kRotLds: the lane's starting entry in its wave's rotation buffer (RotBuf)
    const unsigned rpos = ((0u - delta) * lane) & 63u;
    const unsigned vrot = kSumBytes + kVisBytes + ((ROT == kRotLds) ? wave * RotBuf<D>::kWaveBytes : 0u);   // bytes into smem

    if (sym_clears_last_slot(P, A)) {   // rows nobody else writes (sym_plan.h)
        float* __restrict__ hi = a.acc + (size_t)(P.S + P.K - 1u) * slot_stride;
        const unsigned len = kSymSuper / P.S;
        for (unsigned t = tid; t < len; t += 256u) {
            const size_t v = (size_t)A * kSymSuper + (size_t)s * len + t;
            if (v < pad) {
#pragma unroll
                for (int k = 0; k < 2 * D; ++k) hi[(size_t)k * pad + v] = 0.0f;
                if (QS) a.qsum[(size_t)(P.S + P.K - 1u) * pad + v] = 0.0f;
            }
        }
    }

    for (unsigned hp = 0; hp < kSymSuper / kSymHomePass; ++hp) {
        const unsigned h0 = A * kSymSuper + hp * kSymHomePass;
        if (h0 >= a.pad) break;   // ragged last super-block
        const unsigned tgt0 = h0 + tid;
        f2 ix[PAIRS], iy[PAIRS], iz[PAIRS], hm[PAIRS], qq[QS ? PAIRS : 1];
#pragma unroll
        for (int q = 0; q < PAIRS; ++q) {
            const unsigned i0 = tgt0 + (2 * q) * 256u, i1 = i0 + 256u;
            ix[q] = f2{tp[i0], tp[i1]};
            iy[q] = f2{tp[pad + i0], tp[pad + i1]};
            iz[q] = (D == 3) ? f2{tp[2 * pad + i0], tp[2 * pad + i1]} : f2{0.f, 0.f};
            hm[q] = f2{mp[i0], mp[i1]};
            if (QS) qq[q] = f2{0.f, 0.f};
        }
#pragma unroll
        for (int c = 0; c < PAIRS * D; ++c) sums[c * 256 + tid] = double2{0.0, 0.0};   // own slots only: no barrier needed

        SymWalk nw;
        nw.k = 0u; nw.c = ~0u;
        bool more = sym_next_chunk(P, A, s, &nw);
        f2 nxy = f2{0.f, 0.f}, nzm = f2{0.f, 0.f};                                   // one visitor per lane: the next group's
        f2 nvx = f2{0.f, 0.f}, nvy = f2{0.f, 0.f}, nvz = f2{0.f, 0.f}, nvm = f2{0.f, 0.f};   // two: the next pair of groups'
        if (more) {
            if constexpr (VPL == 2) load_visitor_pair(tp, mp, a.pad, nw.first + lane, nvx, nvy, nvz, nvm);
            else load_visitor<D>(tp, mp, a.pad, nw.first + lane, nxy, nzm);
        }
        while (more) {
            const SymWalk cw = nw;
            f2 ox[PAIRS], oy[PAIRS], oz[PAIRS];
#pragma unroll
            for (int q = 0; q < PAIRS; ++q) ox[q] = oy[q] = oz[q] = f2{0.f, 0.f};
            if constexpr (VPL == 2) {
#pragma unroll 1
                for (unsigned g = 0; g < cw.groups; g += 2u) {   // groups g (.x) and g + 1 (.y)
                    f2 vx = nvx, vy = nvy, vz = nvz, vm = nvm;
                    // the next pair of groups flies while this one rotates
                    if (g + 2u < cw.groups) {
                        load_visitor_pair(tp, mp, a.pad, cw.first + (g + 2u) * kSymGroup + lane, nvx, nvy, nvz, nvm);
                    } else {
                        more = sym_next_chunk(P, A, s, &nw);
                        if (more) load_visitor_pair(tp, mp, a.pad, nw.first + lane, nvx, nvy, nvz, nvm);
                    }
                    float4* __restrict__ vslot = vbuf + (wave * kSymChunkGroups + g) * kSymGroup;   // group g; group g + 1 follows
                    // cleared here rather than by a branch on the first block: the block loop's body stays one basic block
                    vslot[lane] = make_float4(0.f, 0.f, 0.f, 0.f);
                    vslot[kSymGroup + lane] = make_float4(0.f, 0.f, 0.f, 0.f);
                    // the two groups' visitors into the wave's rotation buffer: the last read of the previous pair precedes this
                    // write in the wave's LDS queue, and the first read below follows it
                    constexpr unsigned kPlane = kRotEntries * (unsigned)sizeof(float4);
                    constexpr unsigned kBlockBytes = (unsigned)kSymBlockSteps * (unsigned)sizeof(float4);
                    unsigned roff = 0u;   // bytes into the wave's first plane of the entry the block's last read takes
                    if (ROT == kRotLds) {
                        const float4 lo4 = make_float4(vx.x, vx.y, vy.x, vy.y), hi4 = make_float4(vz.x, vz.y, vm.x, vm.y);
                        *reinterpret_cast<float4*>(smem + vrot + rpos * 16u) = lo4;
                        *reinterpret_cast<float4*>(smem + vrot + kPlane + rpos * 16u) = hi4;
                        if (rpos < kRotEntries - 64u) {
                            *reinterpret_cast<float4*>(smem + vrot + (rpos + 64u) * 16u) = lo4;
                            *reinterpret_cast<float4*>(smem + vrot + kPlane + (rpos + 64u) * 16u) = hi4;
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        // block 0 reads steps 1 .. 8 = entries r + 63 .. r + 56 (mod 64)
                        roff = ((rpos + 64u - (unsigned)kSymBlockSteps) & 63u) * 16u;
                        asm volatile("" : "+v"(roff));
                    }
                    f2 ax[2 * PAIRS], ay[2 * PAIRS], az[2 * PAIRS];   // per home body: .x over group g, .y over group g + 1
#pragma unroll
                    for (int k = 0; k < 2 * PAIRS; ++k) ax[k] = ay[k] = az[k] = f2{0.f, 0.f};
#pragma unroll 1
                    for (unsigned blk = 0; blk < kSymGroup / (unsigned)kSymBlockSteps; ++blk) {
                        f2 vax = f2{0.f, 0.f}, vay = f2{0.f, 0.f}, vaz = f2{0.f, 0.f};   // .x: the visitor of group g, .y: of g + 1
                        // the block's base address stays one register (see the one-visitor loop below)
                        const char* rot = smem;
                        if (ROT == kRotLds) rot = smem + (vrot + roff);
#pragma unroll
                        for (int j = 0; j < kSymBlockSteps; ++j) {
                            if (ROT == kRotLds) {
                                // where the wait for the previous step's two reads lands: behind that step's arithmetic
                                asm volatile("" : "+v"(vx), "+v"(vy), "+v"(vz), "+v"(vm));
                                // the next step's visitor pair flies while this step computes: two reads on one base register,
                                // immediates only.  (The 64th pair of reads fetches step 0's visitors again, unused.)
                                const float4 n0 = *reinterpret_cast<const float4*>(rot + (kSymBlockSteps - 1 - j) * 16);
                                const float4 n1 = *reinterpret_cast<const float4*>(rot + kPlane + (kSymBlockSteps - 1 - j) * 16);
                                __builtin_amdgcn_sched_barrier(0);   // issued first: the scheduler would sink them towards their use
                                keep_packed(ix, iy, iz, hm);
                                sym_step_pairs(vx, vy, vz, vm, ix, iy, iz, hm, ax, ay, az, vax, vay, vaz, bias);
                                vx = f2{n0.x, n0.y}; vy = f2{n0.z, n0.w}; vz = f2{n1.x, n1.y}; vm = f2{n1.z, n1.w};
                            } else {
                                keep_packed(ix, iy, iz, hm);
                                sym_step_pairs(vx, vy, vz, vm, ix, iy, iz, hm, ax, ay, az, vax, vay, vaz, bias);
                                ror1(vx); ror1(vy); ror1(vz); ror1(vm);
                            }
                            ror1(vax); ror1(vay); ror1(vaz);
                            __builtin_amdgcn_sched_barrier(0);   // one step at a time: interleaving the unrolled steps only costs registers
                        }
                        if (ROT == kRotLds) {   // the next block's entries lie below; the base wraps
                            roff = (roff - kBlockBytes) & 1023u;
                            asm volatile("" : "+v"(roff));
                        }
                        // visitor level 1 -> level 2: the block's one chain per visitor, in the wave's slots of the two visitors
                        // that now sit in this lane (the same position of groups g and g + 1)
                        const unsigned vid = (lane + (blk + 1u) * (unsigned)kSymBlockSteps * delta) & 63u;
                        float4 c0 = vslot[vid], c1 = vslot[kSymGroup + vid];
                        c0.x += vax.x; c0.y += vay.x; c0.z += vaz.x;
                        c1.x += vax.y; c1.y += vay.y; c1.z += vaz.y;
                        if (QS) {
                            c0.w = __builtin_fmaf(vaz.x, vaz.x, __builtin_fmaf(vay.x, vay.x, __builtin_fmaf(vax.x, vax.x, c0.w)));
                            c1.w = __builtin_fmaf(vaz.y, vaz.y, __builtin_fmaf(vay.y, vay.y, __builtin_fmaf(vax.y, vax.y, c1.w)));
                        }
                        vslot[vid] = c0;
                        vslot[kSymGroup + vid] = c1;
                    }
                    // home level 1 -> level 2 in group order, scalar: group g's 64-term chain, then group g + 1's
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) {
                        ox[q].x += ax[2 * q].x; oy[q].x += ay[2 * q].x; oz[q].x += az[2 * q].x;
                        ox[q].y += ax[2 * q + 1].x; oy[q].y += ay[2 * q + 1].x; oz[q].y += az[2 * q + 1].x;
                        ox[q].x += ax[2 * q].y; oy[q].x += ay[2 * q].y; oz[q].x += az[2 * q].y;
                        ox[q].y += ax[2 * q + 1].y; oy[q].y += ay[2 * q + 1].y; oz[q].y += az[2 * q + 1].y;
                    }
                    if (QS) {
#pragma unroll
                        for (int q = 0; q < PAIRS; ++q) {
                            const f2 x0 = f2{ax[2 * q].x, ax[2 * q + 1].x}, y0 = f2{ay[2 * q].x, ay[2 * q + 1].x}, z0 = f2{az[2 * q].x, az[2 * q + 1].x};
                            const f2 x1 = f2{ax[2 * q].y, ax[2 * q + 1].y}, y1 = f2{ay[2 * q].y, ay[2 * q + 1].y}, z1 = f2{az[2 * q].y, az[2 * q + 1].y};
                            qq[q] = __builtin_elementwise_fma(x0, x0, qq[q]);
                            qq[q] = __builtin_elementwise_fma(y0, y0, qq[q]);
                            qq[q] = __builtin_elementwise_fma(z0, z0, qq[q]);
                            qq[q] = __builtin_elementwise_fma(x1, x1, qq[q]);
                            qq[q] = __builtin_elementwise_fma(y1, y1, qq[q]);
                            qq[q] = __builtin_elementwise_fma(z1, z1, qq[q]);
                        }
                    }
                }
            } else {
#pragma unroll 1
                for (unsigned g = 0; g < cw.groups; ++g) {
                    f2 vxy = nxy, vzm = nzm;
                    // the next group's bodies fly while this one rotates
                    if (g + 1u < cw.groups) {
                        load_visitor<D>(tp, mp, a.pad, cw.first + (g + 1u) * kSymGroup + lane, nxy, nzm);
                    } else {
                        more = sym_next_chunk(P, A, s, &nw);
                        if (more) load_visitor<D>(tp, mp, a.pad, nw.first + lane, nxy, nzm);
                    }
                    float4* __restrict__ vslot = vbuf + (wave * kSymChunkGroups + g) * kSymGroup;
                    // cleared here rather than by a branch on the first block: the block loop's body stays one basic block (a branch
                    // made the compiler sink the home sums' arithmetic of all eight steps below it, at 256 VGPRs and spills)
                    vslot[lane] = make_float4(0.f, 0.f, 0.f, 0.f);
                    // the group's visitors into the wave's rotation buffer: the last read of the previous group precedes this write
                    // in the wave's LDS queue, and the first read below follows it
                    unsigned roff = 0u;   // bytes into the wave's buffer of the entry the block's last read takes
                    if (ROT == kRotLds) {
                        const float4 me = make_float4(vxy.x, vxy.y, vzm.x, vzm.y);
                        *reinterpret_cast<float4*>(smem + vrot + rpos * 16u) = me;
                        if (rpos < kRotEntries - 64u) *reinterpret_cast<float4*>(smem + vrot + (rpos + 64u) * 16u) = me;
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        // block 0 reads steps 1 .. 8 = entries r + 63 .. r + 56
                        roff = ((rpos + 56u) & 63u) * 16u;
                        asm volatile("" : "+v"(roff));
                    }
                    f2 ax[PAIRS], ay[PAIRS], az[PAIRS];
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) ax[q] = ay[q] = az[q] = f2{0.f, 0.f};
#pragma unroll 1
                    for (unsigned blk = 0; blk < 8u; ++blk) {
                        f2 vax = f2{0.f, 0.f}, vay = f2{0.f, 0.f}, vaz = f2{0.f, 0.f};
                        // the block's base address stays one register: left to itself the compiler splits it into a per-lane and a
                        // per-block part and adds them up again in front of every read
                        const char* rot = smem;
                        if (ROT == kRotLds) rot = smem + (vrot + roff);
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            if (ROT == kRotLds) {
                                // {z, m} stays one register pair (taken apart, m's broadcast costs a v_mov_b32 per step); this is
                                // also where the wait for the previous step's read lands: behind that step's arithmetic
                                asm volatile("" : "+v"(vzm));
                                // the next step's visitor flies while this step computes; the eight reads of a block differ in the
                                // instruction's immediate offset only.  (The 64th read fetches step 0's visitor again, unused.)
                                const float4 nv = *reinterpret_cast<const float4*>(rot + (7 - j) * 16);
                                __builtin_amdgcn_sched_barrier(0);   // issued first: the scheduler would sink it to within 40 cycles of its use
                                sym_step<D, PAIRS>(vxy, vzm, ix, iy, iz, hm, ax, ay, az, vax, vay, vaz, bias);
                                vxy = f2{nv.x, nv.y}; vzm = f2{nv.z, nv.w};
                            } else {
                                sym_step<D, PAIRS>(vxy, vzm, ix, iy, iz, hm, ax, ay, az, vax, vay, vaz, bias);
                                ror1(vxy); ror1(vzm);
                            }
                            ror1(vax); ror1(vay);
                            if (D == 3) ror1(vaz);
                            __builtin_amdgcn_sched_barrier(0);   // one step at a time: interleaving the unrolled steps only costs registers
                        }
                        if (ROT == kRotLds) {   // the next block's eight entries lie below; the base wraps
                            roff = (roff - 128u) & 1023u;
                            asm volatile("" : "+v"(roff));
                        }
                        // visitor level 1 -> level 2, in the wave's slot of the visitor that now sits in this lane
                        const unsigned vid = (lane + (blk + 1u) * 8u * delta) & 63u;
                        const float bx = vax.x + vax.y, by = vay.x + vay.y, bz = (D == 3) ? vaz.x + vaz.y : 0.0f;
                        float4 cur = vslot[vid];
                        cur.x += bx; cur.y += by; cur.z += bz;
                        if (QS) cur.w = __builtin_fmaf(bz, bz, __builtin_fmaf(by, by, __builtin_fmaf(bx, bx, cur.w)));
                        vslot[vid] = cur;
                    }
                    // home level 1 -> level 2
#pragma unroll
                    for (int q = 0; q < PAIRS; ++q) { ox[q] += ax[q]; oy[q] += ay[q]; if (D == 3) oz[q] += az[q]; }
                    if (QS) {
#pragma unroll
                        for (int q = 0; q < PAIRS; ++q) {
                            qq[q] = __builtin_elementwise_fma(ax[q], ax[q], qq[q]);
                            qq[q] = __builtin_elementwise_fma(ay[q], ay[q], qq[q]);
                            if (D == 3) qq[q] = __builtin_elementwise_fma(az[q], az[q], qq[q]);
                        }
                    }
                }
            }
            // home level 2 -> level 3: the lane's own fp64 slots
#pragma unroll
            for (int q = 0; q < PAIRS; ++q) {
                double2 v = sums[(q * D + 0) * 256 + tid];
                v.x += (double)ox[q].x; v.y += (double)ox[q].y;
                sums[(q * D + 0) * 256 + tid] = v;
                v = sums[(q * D + 1) * 256 + tid];
                v.x += (double)oy[q].x; v.y += (double)oy[q].y;
                sums[(q * D + 1) * 256 + tid] = v;
                if (D == 3) {
                    v = sums[(q * D + 2) * 256 + tid];
                    v.x += (double)oz[q].x; v.y += (double)oz[q].y;
                    sums[(q * D + 2) * 256 + tid] = v;
                }
            }
            if (!cw.two_sided) continue;   // own block: the visitors' sums are dropped (workgroup-uniform)
            // visitor level 2 -> level 3: the four waves' sums of one visitor in wave order, onto what the earlier home passes left
            __syncthreads();
            if (tid < cw.groups * kSymGroup) {
                const unsigned g = tid >> 6;
                const size_t v = (size_t)cw.first + tid;
                const float4 b0 = vbuf[(0u * kSymChunkGroups + g) * kSymGroup + lane], b1 = vbuf[(1u * kSymChunkGroups + g) * kSymGroup + lane];
                const float4 b2 = vbuf[(2u * kSymChunkGroups + g) * kSymGroup + lane], b3 = vbuf[(3u * kSymChunkGroups + g) * kSymGroup + lane];
                float* __restrict__ hi = a.acc + (size_t)(P.S + cw.k - 1u) * slot_stride;
                float* __restrict__ lo = hi + (size_t)D * pad;
                double rx = -((((double)b0.x + (double)b1.x) + (double)b2.x) + (double)b3.x);
                double ry = -((((double)b0.y + (double)b1.y) + (double)b2.y) + (double)b3.y);
                double rz = -((((double)b0.z + (double)b1.z) + (double)b2.z) + (double)b3.z);
                if (hp != 0u) {
                    rx += (double)hi[v] + (double)lo[v];
                    ry += (double)hi[pad + v] + (double)lo[pad + v];
                    if (D == 3) rz += (double)hi[2 * pad + v] + (double)lo[2 * pad + v];
                }
                store_hi_lo(hi, lo, v, rx);
                store_hi_lo(hi, lo, pad + v, ry);
                if (D == 3) store_hi_lo(hi, lo, 2 * pad + v, rz);
                if (QS) {
                    float* __restrict__ qo = a.qsum + (size_t)(P.S + cw.k - 1u) * pad + v;
                    const float qv = ((b0.w + b1.w) + b2.w) + b3.w;
                    *qo = (hp != 0u) ? *qo + qv : qv;
                }
            }
            __syncthreads();   // everybody has read the visitors' slots before the next chunk overwrites them
        }

        // the home pass's sums: slot s, rows of A
        float* __restrict__ hi = a.acc + (size_t)s * slot_stride;
        float* __restrict__ lo = hi + (size_t)D * pad;
        float* __restrict__ qout = QS ? a.qsum + (size_t)s * pad : nullptr;
#pragma unroll
        for (int q = 0; q < PAIRS; ++q) {
            const double2 vx = sums[(q * D + 0) * 256 + tid], vy = sums[(q * D + 1) * 256 + tid];
            const double2 vz = (D == 3) ? sums[(q * D + (D == 3 ? 2 : 0)) * 256 + tid] : double2{0.0, 0.0};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned i = tgt0 + (2 * q + h) * 256u;
                if (!a.bad_flag[i]) {   // flagged targets belong to the guarded side path + scatter_close_kernel
                    store_hi_lo(hi, lo, i, h ? vx.y : vx.x);
                    store_hi_lo(hi, lo, pad + i, h ? vy.y : vy.x);
                    if (D == 3) store_hi_lo(hi, lo, 2 * pad + i, h ? vz.y : vz.x);
                    if (QS) qout[i] = h ? qq[q].y : qq[q].x;
                } else if (QS) {
                    qout[i] = __builtin_inff();   // a close-set target keeps no spread sum: it is always a suspect
                }
            }
        }
    }
    if (a.clk) {
        const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        if (tid == 0) {
            const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
            a.clk[2 * wg] = t1 - clk_t0;
            a.clk[2 * wg + 1] = r1 - clk_r0;
        }
    }
}

}  // namespace

// the table entry of this unit (force_launch.hip appends it to force_kernel.hip's)
namespace {
template <int ROT>
KernelVariant sym_variant(const char* name) {
    KernelVariant v = {};
    v.name = name;
    v.tpl = 8;
    v.k2 = accel_sym3l_kernel<2, 0, ROT>; v.k3 = accel_sym3l_kernel<3, 0, ROT>;
    v.qs2 = accel_sym3l_kernel<2, 1, ROT>; v.qs3 = accel_sym3l_kernel<3, 1, ROT>;
    v.fast = 1;
    v.planes = 2;
    v.sym = 1;
    v.stamps = 1;
    return v;
}
}  // namespace
KernelVariant sym_kernel_variant() { return sym_variant<kRotLds>("sympk3l_t8_w3"); }
// the parent form of the rotation, for the A/B and the identity test: never a default, last in the table
KernelVariant sym_dpp_kernel_variant() { return sym_variant<kRotDpp>("sympk3l_t8_w3_dpp"); }

}  // namespace nbx
