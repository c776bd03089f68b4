// state_kernels.hip -- K3/K4: layout pack/unpack at the boundary and the fused kick+drift step.
//
// All O(N), HBM-streaming kernels; one lane per body, SoA arrays so every access is coalesced.
// The integrator state (position, velocity, mass of the own shard) is kept in fp64 and advanced
// with exactly the reference's arithmetic (nbody-sim-new/methods.cpp:425-450); only the pair sum
// feeding it is fp32.  Each drift also refreshes the shard's fp32 chunk of the exchange buffer.
#include "nbx_internal.h"
#include "device_sort.h"

namespace nbx {
namespace {

// Sum the per-slice partial accelerations of body l, component k, in slice order (deterministic).
__device__ __forceinline__ double sum_partials(const float* __restrict__ acc, int splits, int dim,
                                               unsigned pad, int k, size_t l) {
    double a = 0.0;
#pragma unroll 8   // eight plane loads in flight (the additions stay in plane order): 64 planes at N = 65,536 are a latency chain otherwise
    for (int s = 0; s < splits; ++s) a += (double)acc[((size_t)s * dim + k) * pad + l];
    return a;
}

// K4: AoS fp64 Body<D> (body.h:8-11) -> SoA fp32 exchange buffers for every shard + fp64 state of
// the own shard.  Pad entries become massless bodies at the origin.  The same pass collects what the host needs to
// know about the bodies before it picks a force kernel (p.facts): a million-body scan on one host thread cost 4 ms.
__global__ __launch_bounds__(256) void pack_kernel(PackArgs p) {
    __shared__ unsigned long long s_mass, s_coord;
    __shared__ unsigned s_close;
    if (threadIdx.x == 0) { s_mass = 0ull; s_coord = 0ull; s_close = 0u; }
    __syncthreads();
    const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;  // index into [n_shards][pad], or into the own chunk's [pad]
    if (b < (p.only_own ? (size_t)p.pad : (size_t)p.n_shards * p.pad)) {
        const int g = p.only_own ? p.shard : (int)(b / p.pad);
        const size_t l = p.only_own ? b : b - (size_t)g * p.pad;
        const size_t id = p.only_own ? l : (size_t)g * p.shard_len + l;          // index into raw
        const bool real = p.only_own ? (l < p.n_own) : ((l < p.shard_len) && (id < p.n_total));
        const double* __restrict__ src = p.raw + id * p.stride_d;
        double cmin = 0.0, cmax = 0.0;
        for (int k = 0; k < p.dim; ++k) {
            const double x = real ? src[k] : 0.0;
            p.pos_all[((size_t)g * p.dim + k) * p.pad + l] = (float)x;
            if (g == p.shard) {
                p.x64[(size_t)k * p.pad + l] = x;
                p.v64[(size_t)k * p.pad + l] = real ? src[p.dim + k] : 0.0;
            }
            const double ax = fabs(x);
            cmin = (k == 0 || ax < cmin) ? ax : cmin;
            cmax = (cmax != cmax) ? cmax : (!(ax <= cmax) ? ax : cmax);   // sticky NaN: once seen, a later finite coordinate does not replace it
        }
        const double m = real ? src[2 * p.dim] : 0.0;
        p.mass_all[(size_t)g * p.pad + l] = (float)m;
        if (g == p.shard) p.m64[l] = m;
        // non-negative doubles order like their bit patterns, and a NaN's pattern lies above infinity's: maxima over the
        // wave by butterfly shuffles, then one LDS atomic per wave (one per lane made this pass 4x longer)
        unsigned long long mb = real ? (unsigned long long)__double_as_longlong(fabs(m)) : 0ull;
        unsigned long long cb = real ? (unsigned long long)__double_as_longlong(cmax) : 0ull;
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long om = __shfl_xor(mb, off), oc = __shfl_xor(cb, off);
            mb = om > mb ? om : mb;
            cb = oc > cb ? oc : cb;
        }
        const unsigned long long votes = __ballot(real && g == p.shard && cmin < (double)kCloseCoord);
        if ((threadIdx.x & 63u) == 0u) {
            if (mb) atomicMax(&s_mass, mb);
            if (cb) atomicMax(&s_coord, cb);
            if (votes) atomicAdd(&s_close, (unsigned)__popcll(votes));
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_mass > *(volatile unsigned long long*)&p.facts[0]) atomicMax(&p.facts[0], s_mass);     // same economy at L2
        if (s_coord > *(volatile unsigned long long*)&p.facts[1]) atomicMax(&p.facts[1], s_coord);
        if (s_close) atomicAdd(&p.facts[2], (unsigned long long)s_close);
    }
}

// K3: fused kick + drift (methods.cpp:436 then :448), fp64:
//   F = -(G m) a ;  v += (F / m) * dt ;  x += v * dt ;  pos32 = (float)x
// One lane per (body, component): grid.y = component.  The components are independent (v_k += (F_k/m) dt; x_k += v_k dt),
// so this is the same arithmetic in the same order as a loop over k in one lane -- with dim times the lanes in flight,
// which is what a latency-bound kernel wants at small N (one lane per body was 25 us at N = 65,536: S = 32 dependent-address
// loads per component and one workgroup per CU).
__global__ __launch_bounds__(256) void kick_drift_kernel(KickDriftArgs a) {
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= a.count) return;
    const int k = (int)blockIdx.y;
    const double m = a.m64[l];
    const double gm = a.G * m;
    const double acc = sum_partials(a.acc, a.splits, a.dim, a.pad, k, l);
    const double F = -(gm * acc);
    double v = a.v64[(size_t)k * a.pad + l];
    double x = a.x64[(size_t)k * a.pad + l];
    v += (F / m) * a.dt_kick;
    x += v * a.dt_drift;
    a.v64[(size_t)k * a.pad + l] = v;
    a.x64[(size_t)k * a.pad + l] = x;
    a.pos_chunk[(size_t)k * a.pad + l] = (float)x;
}

// The leaf plan's kick and drift, every stepping loop's and kick-drift-kick's building block: kick_drift_kernel's two helpers fed the
// near-field sums of the tree codes (fp64, per padded slot), the kick's and the drift's step apart as there.  dt_kick == dt_drift is
// the reference's kick then drift (this file is built without contraction: each multiply and each add rounds by itself).  DRIFT =
// false is a pure kick: x64 and the fp32 position chunk are neither read nor written, so a velocity that is not finite cannot reach
// a position through inf * 0.
template <bool DRIFT>
__global__ __launch_bounds__(256) void kick_drift_slots_kernel(SlotKickArgs a) {
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= a.count) return;
    const int k = (int)blockIdx.y;
    const double m = a.m64[l];
    const uint32_t slot = a.body_slot[l];
    const double sum = slot == 0xffffffffu ? 0.0 : a.sums[(size_t)k * a.pslots + slot];
    const double F = (a.signedG * m) * sum;
    double v = a.v64[(size_t)k * a.pad + l];
    v += (F / m) * a.dt_kick;
    a.v64[(size_t)k * a.pad + l] = v;
    if (DRIFT) {
        double x = a.x64[(size_t)k * a.pad + l];
        x += v * a.dt_drift;
        a.x64[(size_t)k * a.pad + l] = x;
        a.pos_chunk[(size_t)k * a.pad + l] = (float)x;
    }
}

// The largest acceleration magnitude of the last evaluation, |signedG| * |sums[.][slot_i]|, over the bodies that have a slot (fp64).
// pack_kernel's idiom: non-negative doubles order like their bit patterns and a NaN's pattern lies above infinity's, so a sum that
// is not finite makes the result not finite; butterfly maxima over the wave, one LDS atomic per wave, one L2 atomic per workgroup.
// Every lane stays for the shuffles (no early exit); lanes past n and bodies in no leaf carry 0.
__global__ __launch_bounds__(256) void slot_accel_max_kernel(const double* __restrict__ sums, const uint32_t* __restrict__ body_slot,
                                                             uint32_t pslots, int dim, size_t n, double absG,
                                                             unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_max;
    if (threadIdx.x == 0) s_max = 0ull;
    __syncthreads();
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long ab = 0ull;
    if (l < n) {
        const uint32_t slot = body_slot[l];
        if (slot != 0xffffffffu) {
            double s2 = 0.0;
            for (int k = 0; k < dim; ++k) { const double s = sums[(size_t)k * pslots + slot]; s2 += s * s; }
            ab = (unsigned long long)__double_as_longlong(fabs(absG * sqrt(s2)));   // fabs: a NaN's sign bit goes too
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(ab, off);
        ab = o > ab ? o : ab;
    }
    if ((threadIdx.x & 63u) == 0u && ab) atomicMax(&s_max, ab);
    __syncthreads();
    if (threadIdx.x == 0 && s_max > *(volatile unsigned long long*)out) atomicMax(out, s_max);
}

// ---- the step chosen on the device (nbx_leaf_plan_step_kdk_adaptive; include/nbody_hip.h has the rule) ----
// slot_accel_max_kernel's maximum taken slot by slot: a slot that holds a body (pslot_body is body_slot's inverse; a leaf's pad holds
// 0xffffffff) contributes what that body contributes there, and a maximum does not depend on the order, so the word is the same bits.
// One lane per slot reads its dim sums and its 4-byte body index coalesced (28 B per slot) where one lane per body gathers dim
// scattered doubles -- the form for a reduction behind EVERY evaluation.
__global__ __launch_bounds__(256) void slot_accel_max_by_slot_kernel(const double* __restrict__ sums, const uint32_t* __restrict__ pslot_body,
                                                                     uint32_t pslots, int dim, double absG, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_max;
    if (threadIdx.x == 0) s_max = 0ull;
    __syncthreads();
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long ab = 0ull;
    if (l < pslots && pslot_body[l] != 0xffffffffu) {
        double s2 = 0.0;
        for (int k = 0; k < dim; ++k) { const double s = sums[(size_t)k * pslots + l]; s2 += s * s; }
        ab = (unsigned long long)__double_as_longlong(fabs(absG * sqrt(s2)));
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(ab, off);
        ab = o > ab ? o : ab;
    }
    if ((threadIdx.x & 63u) == 0u && ab) atomicMax(&s_max, ab);
    __syncthreads();
    if (threadIdx.x == 0 && s_max > *(volatile unsigned long long*)out) atomicMax(out, s_max);
}

__global__ void step_clock_init_kernel(StepClock* __restrict__ c, double accel_length, double dt_min, double dt_max, double t_start, double t_end,
                                       int pow2, uint32_t capacity) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    c->amax_bits = 0ull;
    c->accel_length = accel_length; c->dt_min = dt_min; c->dt_max = dt_max; c->t_end = t_end;
    c->t = t_start; c->prev = 0.0; c->a_max_last = 0.0;
    c->dt_kick = 0.0; c->dt_drift = 0.0;
    c->pow2 = pow2; c->drift = 0; c->apply = 0;
    c->stopped = 0; c->finished = 0; c->status = 0;
    c->steps = 0u; c->evaluations = 0u; c->recorded = 0u;
    c->capacity = capacity;
}

// The controller: one thread, behind slot_accel_max_kernel on the same stream (the stream orders them: no fence, no ticket), runs
// the loop rule for the evaluation just reduced, in fp64 without contraction, and leaves this evaluation's kick in the clock.  Once
// the loop has stopped every later evaluation finds apply = 0 and records nothing.
__global__ void step_controller_kernel(StepClock* __restrict__ c, int last) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (c->stopped) { c->apply = 0; c->drift = 0; return; }
    const double a_max = __longlong_as_double((long long)c->amax_bits);
    double* const history = reinterpret_cast<double*>(reinterpret_cast<char*>(c) + kStepClockHistoryOffset);
    c->evaluations += 1u;
    c->a_max_last = a_max;
    if (!(fabs(a_max) <= 1.7976931348623157e308)) {      // NaN or infinity: no kick with these sums
        c->status = 1; c->stopped = 1; c->apply = 0; c->drift = 0;
        return;
    }
    const double t = c->t, t_end = c->t_end, prev = c->prev;
    const uint32_t slot = c->recorded;
    if (t >= t_end || last) {                             // the closing half-kick
        c->dt_kick = 0.5 * prev; c->dt_drift = 0.0;
        c->drift = 0; c->apply = prev != 0.0 ? 1 : 0;
        if (slot < c->capacity) { history[2 * (size_t)slot] = a_max; history[2 * (size_t)slot + 1] = 0.0; c->recorded = slot + 1u; }
        c->finished = t >= t_end ? 1 : 0;
        c->stopped = 1;
        return;
    }
    const double raw = a_max == 0.0 ? __longlong_as_double(0x7ff0000000000000ll) : sqrt(c->accel_length / a_max);
    const double dt_min = c->dt_min, dt_max = c->dt_max;
    double dt;
    if (c->pow2) {
        dt = dt_max;
        while (dt > raw && 0.5 * dt >= dt_min) dt = 0.5 * dt;
    } else {
        dt = raw < dt_min ? dt_min : raw;                 // min(max(raw, dt_min), dt_max)
        dt = dt > dt_max ? dt_max : dt;
    }
    const double left = t_end - t;
    if (dt >= left) { dt = left; c->t = t_end; }
    else c->t = t + dt;
    c->dt_kick = 0.5 * prev + 0.5 * dt; c->dt_drift = dt;
    c->drift = dt != 0.0 ? 1 : 0; c->apply = 1;
    c->prev = dt;
    c->steps += 1u;
    if (slot < c->capacity) { history[2 * (size_t)slot] = a_max; history[2 * (size_t)slot + 1] = dt; c->recorded = slot + 1u; }
}

// kick_drift_slots_kernel's body with the kick's and the drift's step and the two flags read from the clock (uniform addresses, the
// same for every lane).  apply == 0: nothing is read or written.  drift == 0 is the pure kick: x64 and the fp32 chunk are neither
// read nor written.
__global__ __launch_bounds__(256) void kick_drift_slots_clock_kernel(SlotKickArgs a, const StepClock* __restrict__ clock) {
    if (clock->apply == 0) return;
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= a.count) return;
    const double dt_kick = clock->dt_kick, dt_drift = clock->dt_drift;
    const bool drift = clock->drift != 0;
    const int k = (int)blockIdx.y;
    const double m = a.m64[l];
    const uint32_t slot = a.body_slot[l];
    const double sum = slot == 0xffffffffu ? 0.0 : a.sums[(size_t)k * a.pslots + slot];
    const double F = (a.signedG * m) * sum;
    double v = a.v64[(size_t)k * a.pad + l];
    v += (F / m) * dt_kick;
    a.v64[(size_t)k * a.pad + l] = v;
    if (drift) {
        double x = a.x64[(size_t)k * a.pad + l];
        x += v * dt_drift;
        a.x64[(size_t)k * a.pad + l] = x;
        a.pos_chunk[(size_t)k * a.pad + l] = (float)x;
    }
}

// ---- the same loop for the all-pairs context (nbx_ctx_step_kdk_adaptive) ----
// The largest acceleration of the context's last evaluation: max over the real bodies l < count of absG * sqrt(sum_k A_k[l]^2), A_k[l]
// = sum_partials, the very number kick_drift_kernel is about to use (same loop, same load batching, plane order: same bits).  It
// streams 4 * DIM * splits bytes per body and writes nothing but the word.  One lane per (body, component), as kick_drift_kernel and
// for its reason -- one lane per body is a chain of DIM * splits dependent-address loads, 25 us at N = 65,536 -- with threadIdx.y the
// component: a wave is 64 consecutive bodies of ONE component (a 256-byte row per plane), the DIM squares of a body meet in LDS and
// are added in component order by the lanes of component 0.  The maximum is pack_kernel's idiom: bit patterns of non-negative
// doubles (a NaN's lies above infinity's: a sum that is not finite makes the result not finite), butterfly over the wave, one LDS
// atomic per wave that holds bodies, one L2 atomic per workgroup.  Every lane stays for the shuffles; pads never count.
template <int DIM>
__global__ __launch_bounds__(256 * DIM) void ctx_accel_max_kernel(const float* __restrict__ acc, int splits, unsigned pad, size_t count,
                                                                  double absG, unsigned long long* __restrict__ out) {
    __shared__ double s_sq[DIM][256];
    __shared__ unsigned long long s_max;
    if (threadIdx.x == 0 && threadIdx.y == 0) s_max = 0ull;
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int k = (int)threadIdx.y;
    double sq = 0.0;
    if (l < count) {
        const double s = sum_partials(acc, splits, DIM, pad, k, l);
        sq = s * s;
    }
    s_sq[k][threadIdx.x] = sq;
    __syncthreads();
    unsigned long long ab = 0ull;
    if (k == 0 && l < count) {
        double s2 = 0.0;
#pragma unroll
        for (int j = 0; j < DIM; ++j) s2 += s_sq[j][threadIdx.x];
        ab = (unsigned long long)__double_as_longlong(fabs(absG * sqrt(s2)));   // fabs: a NaN's sign bit goes too
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(ab, off);
        ab = o > ab ? o : ab;
    }
    if (k == 0 && (threadIdx.x & 63u) == 0u && ab) atomicMax(&s_max, ab);
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0 && s_max > *(volatile unsigned long long*)out) atomicMax(out, s_max);
}

// kick_drift_kernel's body with dt_kick and dt_drift read from the clock (uniform addresses, the same for every lane): given the
// same two numbers, the same bits.  apply == 0 (the loop has stopped, or a closing kick of nothing): nothing is read or written.
__global__ __launch_bounds__(256) void kick_drift_clock_kernel(KickDriftArgs a, const StepClock* __restrict__ clock) {
    if (clock->apply == 0) return;
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= a.count) return;
    const double dt_kick = clock->dt_kick, dt_drift = clock->dt_drift;
    const int k = (int)blockIdx.y;
    const double m = a.m64[l];
    const double gm = a.G * m;
    const double acc = sum_partials(a.acc, a.splits, a.dim, a.pad, k, l);
    const double F = -(gm * acc);
    double v = a.v64[(size_t)k * a.pad + l];
    double x = a.x64[(size_t)k * a.pad + l];
    v += (F / m) * dt_kick;
    x += v * dt_drift;
    a.v64[(size_t)k * a.pad + l] = v;
    a.x64[(size_t)k * a.pad + l] = x;
    a.pos_chunk[(size_t)k * a.pad + l] = (float)x;
}

// ---- kick-drift-kick with block time steps (nbx_ctx_step_kdk_block; include/nbody_hip.h has the rule) ----
// Per evaluation the stream carries: the force kernels and their fold (active_kernel.hip), then block_check, block_control_pre,
// block_kick (launch_block_kick), then block_control_post, block_drift and the select pipeline (launch_block_advance).  The
// stream orders them: no fence, no ticket.  Once clock->stopped is set every one of them returns at once.
__global__ void block_clock_init_kernel(BlockClock* __restrict__ c, double accel_length, double dt_max, double t_start, int levels,
                                        unsigned long long T_end, unsigned long long n_total, uint32_t max_substeps, uint32_t capacity) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    c->accel_length = accel_length; c->dt_max = dt_max; c->t_start = t_start; c->t = t_start;
    double tick = dt_max;
    for (int l = 0; l < levels; ++l) tick = 0.5 * tick;     // exact halvings
    c->tick = tick; c->dt_drift = 0.0;
    c->T = 0ull; c->T_end = T_end; c->pair_terms = 0ull; c->n_total = n_total;
    c->n_active = 0u; c->n_bodies = (unsigned)n_total; c->bad = 0u;
    for (int l = 0; l < 21; ++l) c->pop[l] = 0u;
    c->levels = levels;
    c->first = 1; c->closing = 0; c->apply = 0; c->drift = 0;
    c->stopped = 0; c->finished = 0; c->status = 0; c->deepest = 0;
    c->substeps = 0u; c->evaluations = 0u; c->recorded = 0u; c->capacity = capacity; c->max_substeps = max_substeps;
}

__global__ __launch_bounds__(256) void block_levels_init_kernel(int* __restrict__ level, size_t count) {
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l < count) level[l] = 0;
}

// a_r = absG |A_r| of active row r: what the rule calls a_i (the squares added in component order)
__device__ __forceinline__ double block_row_accel(const BlockStepArgs& b, unsigned r) {
    double s2 = 0.0;
    for (int k = 0; k < b.dim; ++k) { const double s = b.sums[(size_t)k * b.cap + r]; s2 += s * s; }
    return fabs(b.absG * sqrt(s2));
}

// "any a_i not finite: status 1, stop; nobody is kicked": the look at every active row comes before the first kick
__global__ __launch_bounds__(256) void block_check_kernel(BlockStepArgs b) {
    BlockClock* const c = b.clock;
    if (c->stopped) return;
    const unsigned r = blockIdx.x * 256u + threadIdx.x;
    const bool bad = r < c->n_active && !(block_row_accel(b, r) <= 1.7976931348623157e308);
    const unsigned long long votes = __ballot(bad);
    if ((threadIdx.x & 63u) == 0u && votes) atomicOr(&c->bad, 1u);
}

__global__ void block_control_pre_kernel(BlockClock* __restrict__ c) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    c->apply = 0; c->drift = 0;
    if (c->stopped) return;
    c->evaluations += 1u;
    if (c->bad) { c->status = 1; c->stopped = 1; return; }
    c->closing = c->T == c->T_end ? 1 : 0;
    c->apply = 1;
}

// The active bodies' level rule and kick, one lane per active row (a body's level needs all its components).  The population of
// the levels is kept with integer atomics: one add per wave and level that gained or lost bodies would be finer, but a substep
// moves few bodies between levels.
__global__ __launch_bounds__(256) void block_kick_kernel(BlockStepArgs b) {
    BlockClock* const c = b.clock;
    if (c->apply == 0) return;
    const unsigned r = blockIdx.x * 256u + threadIdx.x;
    if (r >= c->n_active) return;
    const unsigned i = b.list[r];
    const int L = c->levels;
    const double dt_max = c->dt_max;
    const unsigned long long T = c->T;
    const bool first = c->first != 0, closing = c->closing != 0;
    const double a = block_row_accel(b, r);
    const double raw = a == 0.0 ? __longlong_as_double(0x7ff0000000000000ll) : sqrt(c->accel_length / a);
    int w = 0;
    for (double d = dt_max; d > raw && w < L; ++w) d = 0.5 * d;
    const int old = first ? -1 : b.level[i];
    int now;
    if (first) now = w;
    else if (closing) now = old;
    else if (w > old) now = w;
    else if (w < old && old > 0 && (T & ((2ull << (L - old)) - 1ull)) == 0ull) now = old - 1;
    else now = old;
    double dt_old = dt_max, dt_new = dt_max;
    for (int l = 0; l < old; ++l) dt_old = 0.5 * dt_old;
    for (int l = 0; l < now; ++l) dt_new = 0.5 * dt_new;
    const double kick = first ? 0.5 * dt_new : closing ? 0.5 * dt_old : 0.5 * dt_old + 0.5 * dt_new;
    const double m = b.m64[i];
    const double gm = b.G * m;
    for (int k = 0; k < b.dim; ++k) {
        const double F = -(gm * b.sums[(size_t)k * b.cap + r]);
        double v = b.v64[(size_t)k * b.pad + i];
        v += (F / m) * kick;
        b.v64[(size_t)k * b.pad + i] = v;
    }
    if (now != old) {
        b.level[i] = now;
        atomicAdd(&c->pop[now], 1u);
        if (old >= 0) atomicSub(&c->pop[old], 1u);
    }
}

// The controller behind the kick: history, the stops, dn from the deepest level present, T and t.
__global__ void block_control_post_kernel(BlockClock* __restrict__ c) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (c->stopped) return;
    uint32_t* const history = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(c) + kBlockClockHistoryOffset);
    const int L = c->levels;
    int deepest = 0;
    for (int l = 0; l <= L; ++l) if (c->pop[l]) deepest = l;
    if (deepest > c->deepest) c->deepest = deepest;
    c->first = 0;
    c->pair_terms += (unsigned long long)c->n_active * c->n_total;
    const bool closing = c->closing != 0, capped = !closing && c->substeps == c->max_substeps;
    const uint32_t dn = (closing || capped) ? 0u : 1u << (L - deepest);
    const uint32_t slot = c->recorded;
    if (slot < c->capacity) { history[2 * (size_t)slot] = c->n_active; history[2 * (size_t)slot + 1] = dn; c->recorded = slot + 1u; }
    if (closing) { c->finished = 1; c->stopped = 1; return; }
    if (capped) { c->status = 2; c->stopped = 1; return; }
    c->dt_drift = (double)dn * c->tick;
    c->drift = 1;
    c->T += dn;
    c->t = c->t_start + (double)c->T * c->tick;
    c->substeps += 1u;
}

// x += v * (dn tick) for ALL bodies, the fp32 chunk refreshed: kick_drift_kernel's drift, one lane per (body, component)
__global__ __launch_bounds__(256) void block_drift_kernel(BlockStepArgs b) {
    if (b.clock->drift == 0) return;
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= b.count) return;
    const size_t at = (size_t)blockIdx.y * b.pad + l;
    double x = b.x64[at];
    x += b.v64[at] * b.clock->dt_drift;
    b.x64[at] = x;
    b.pos_chunk[at] = (float)x;
}

// select, first half: flags[i] = body i's own step ends at the clock's T
__global__ __launch_bounds__(256) void block_flag_kernel(BlockStepArgs b) {
    const BlockClock* const c = b.clock;
    if (c->stopped) return;
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= b.count) return;
    b.flags[l] = (c->T & ((1ull << (c->levels - b.level[l])) - 1ull)) == 0ull ? 1u : 0u;
}

// select, second half, behind the exclusive scan of the flags (in place; the total behind the last one): ascending order
__global__ __launch_bounds__(256) void block_scatter_kernel(BlockStepArgs b) {
    BlockClock* const c = b.clock;
    if (c->stopped) return;
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l == 0) c->n_active = b.flags[b.count];
    if (l >= b.count) return;
    const unsigned at = b.flags[l];
    if (b.flags[l + 1] != at) b.list[at] = (unsigned)l;
}

// ---- fourth-order Hermite with block time steps (nbx_ctx_step_hermite_block; include/nbody_hip.h has the rule) ----
// Per evaluation the stream carries: the list kernels with the jerk and their fold (active_jerk_kernel.hip), then hermite_check,
// block_control_pre, hermite_correct (launch_hermite_correct), then block_control_post, hermite_predict and the select pipeline
// (launch_hermite_advance).  The clock, both controllers and the select are the kick-drift-kick loop's, unchanged.
__global__ __launch_bounds__(256) void hermite_velocity_kernel(HermiteArgs h) {
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= h.b.count) return;
    const size_t at = (size_t)blockIdx.y * h.b.pad + l;
    h.vel_chunk[at] = (float)h.b.v64[at];
}

// "any component of a or j not finite: status 1, stop; nobody is corrected": the look at every active row comes before the corrector
__global__ __launch_bounds__(256) void hermite_check_kernel(HermiteArgs h) {
    BlockClock* const c = h.b.clock;
    if (c->stopped) return;
    const unsigned r = blockIdx.x * 256u + threadIdx.x;
    bool bad = false;
    if (r < c->n_active)
        for (int k = 0; k < 2 * h.b.dim; ++k) bad = bad || !(fabs(h.b.G * h.sums[(size_t)k * h.b.cap + r]) <= 1.7976931348623157e308);
    const unsigned long long votes = __ballot(bad);
    if ((threadIdx.x & 63u) == 0u && votes) atomicOr(&c->bad, 1u);
}

// One lane per active row.  The call's first evaluation starts every body: a, j, the level from eta_start |a| / |j|, t_i = 0.  Later
// ones correct the body over its own step h = dt_level, choose its next level by Aarseth's criterion under the kick-drift-kick
// loop's level rule, and leave (x, v, a, j) at t_i = T; the fp32 chunks take the corrected state (at T_end that is every body).
__global__ __launch_bounds__(256) void hermite_correct_kernel(HermiteArgs h) {
    const BlockStepArgs& b = h.b;
    BlockClock* const c = b.clock;
    if (c->apply == 0) return;
    const unsigned r = blockIdx.x * 256u + threadIdx.x;
    if (r >= c->n_active) return;
    const unsigned i = b.list[r];
    const int L = c->levels;
    const double dt_max = c->dt_max;
    const unsigned long long T = c->T;
    const bool first = c->first != 0, closing = c->closing != 0;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const int old = first ? -1 : b.level[i];
    double a1[3], j1[3], sa = 0.0, sj = 0.0;
    for (int k = 0; k < b.dim; ++k) {
        a1[k] = -(b.G * h.sums[(size_t)k * b.cap + r]);
        j1[k] = -(b.G * h.sums[(size_t)(b.dim + k) * b.cap + r]);
        sa += a1[k] * a1[k];
        sj += j1[k] * j1[k];
    }
    const double na = sqrt(sa), nj = sqrt(sj);
    double raw;
    if (first) {
        raw = nj == 0.0 ? inf : (h.eta_start * na) / nj;
    } else {
        double dt = dt_max;
        for (int l = 0; l < old; ++l) dt = 0.5 * dt;
        const double h2 = dt * dt, h3 = h2 * dt;
        double s2 = 0.0, s3 = 0.0;
        for (int k = 0; k < b.dim; ++k) {
            const size_t at = (size_t)k * b.pad + i;
            const double a0 = h.a64[at], j0 = h.j64[at], v0 = b.v64[at], x0 = b.x64[at];
            const double da = a0 - a1[k];
            const double v1 = (v0 + (0.5 * dt) * (a0 + a1[k])) + (h2 / 12.0) * (j0 - j1[k]);
            const double x1 = (x0 + (0.5 * dt) * (v0 + v1)) + (h2 / 12.0) * da;
            const double a2 = (-6.0 * da - dt * (4.0 * j0 + 2.0 * j1[k])) / h2;
            const double a3 = (12.0 * da + (6.0 * dt) * (j0 + j1[k])) / h3;
            const double a2e = a2 + dt * a3;
            s2 += a2e * a2e;
            s3 += a3 * a3;
            b.v64[at] = v1;
            b.x64[at] = x1;
            b.pos_chunk[at] = (float)x1;
            h.vel_chunk[at] = (float)v1;
        }
        const double n2 = sqrt(s2), n3 = sqrt(s3);
        const double den = nj * n3 + n2 * n2;
        raw = den == 0.0 ? inf : sqrt((h.eta * (na * n2 + nj * nj)) / den);
    }
    for (int k = 0; k < b.dim; ++k) {
        const size_t at = (size_t)k * b.pad + i;
        h.a64[at] = a1[k];
        h.j64[at] = j1[k];
    }
    h.t_i[i] = T;
    int w = 0;
    for (double d = dt_max; d > raw && w < L; ++w) d = 0.5 * d;
    int now;
    if (first) now = w;
    else if (closing) now = old;
    else if (w > old) now = w;
    else if (w < old && old > 0 && (T & ((2ull << (L - old)) - 1ull)) == 0ull) now = old - 1;
    else now = old;
    if (now != old) {
        b.level[i] = now;
        atomicAdd(&c->pop[now], 1u);
        if (old >= 0) atomicSub(&c->pop[old], 1u);
    }
}

// The predictor of ALL bodies to the clock's T, into the fp32 chunks only: x, v themselves stay.  One lane per (body, component).
__global__ __launch_bounds__(256) void hermite_predict_kernel(HermiteArgs h) {
    const BlockClock* const c = h.b.clock;
    if (c->drift == 0 && c->status != 2) return;
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= h.b.count) return;
    const size_t at = (size_t)blockIdx.y * h.b.pad + l;
    if (c->drift == 0) {   // stopped at the cap: the bodies stay at their own times, and the fp32 chunks go back to being their roundings
        h.b.pos_chunk[at] = (float)h.b.x64[at];
        h.vel_chunk[at] = (float)h.b.v64[at];
        return;
    }
    const double dt = (double)(c->T - h.t_i[l]) * c->tick;
    const double h2 = dt * dt;
    const double x = h.b.x64[at], v = h.b.v64[at], a = h.a64[at], j = h.j64[at];
    const double xp = ((x + v * dt) + a * (0.5 * h2)) + j * ((h2 * dt) / 6.0);
    const double vp = (v + a * dt) + j * (0.5 * h2);
    h.b.pos_chunk[at] = (float)xp;
    h.vel_chunk[at] = (float)vp;
}

__global__ __launch_bounds__(256) void export_forces_kernel(const float* __restrict__ acc, int splits, int dim,
                                                            unsigned pad, size_t count, double G,
                                                            const double* __restrict__ m64,
                                                            double* __restrict__ out) {
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= count) return;
    const double gm = G * m64[l];
    for (int k = 0; k < dim; ++k) out[l * dim + k] = -(gm * sum_partials(acc, splits, dim, pad, k, l));
}

__global__ __launch_bounds__(256) void export_accel_kernel(const float* __restrict__ acc, int splits, int dim,
                                                           unsigned pad, size_t count, float* __restrict__ out) {
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= count) return;
    for (int k = 0; k < dim; ++k) out[(size_t)k * count + l] = (float)sum_partials(acc, splits, dim, pad, k, l);
}

__global__ __launch_bounds__(256) void export_state_kernel(const double* __restrict__ x64,
                                                           const double* __restrict__ v64, int dim,
                                                           unsigned pad, size_t count, double* __restrict__ out) {
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= count) return;
    for (int k = 0; k < dim; ++k) {
        out[l * 2 * dim + k] = x64[(size_t)k * pad + l];
        out[l * 2 * dim + dim + k] = v64[(size_t)k * pad + l];
    }
}

// Per-body energies for the reference law: kinetic m v^2 / 2 and potential (G m / 4) * phi,
// phi = sum over slices of potential_kernel's output (fp64, slice order).
// Energy reduction: per-body kinetic m v^2 / 2 and potential (G m / 4) * sum_slices phi, summed on the device --
// wave64 butterfly over the lanes (__shfl_down on fp64 = two DPP/permute moves per step, 6 steps), the four wave sums of
// a workgroup through LDS in wave order, one {kinetic, potential} pair per workgroup in energy_out[2][blocks].  The host
// adds the per-workgroup pairs in block order: a fixed summation tree, bit-reproducible, and 16 B per 256 bodies cross
// PCIe instead of 16 B per body.
__global__ __launch_bounds__(256) void energy_partials_kernel(const float* __restrict__ phi, int splits, int dim,
                                                              unsigned pad, size_t count, double G,
                                                              const double* __restrict__ v64,
                                                              const double* __restrict__ m64, double* __restrict__ out) {
    __shared__ double wave_ke[4], wave_pe[4];
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    double ke = 0.0, pe = 0.0;
    if (l < count) {
        double p = 0.0;
        for (int s = 0; s < splits; ++s) p += (double)phi[(size_t)s * pad + l];
        double v2 = 0.0;
        for (int k = 0; k < dim; ++k) { const double v = v64[(size_t)k * pad + l]; v2 += v * v; }
        const double m = m64[l];
        ke = 0.5 * m * v2;
        pe = 0.25 * G * m * p;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ke += __shfl_down(ke, off, 64);
        pe += __shfl_down(pe, off, 64);
    }
    if ((threadIdx.x & 63u) == 0) { wave_ke[threadIdx.x >> 6] = ke; wave_pe[threadIdx.x >> 6] = pe; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[blockIdx.x] = ((wave_ke[0] + wave_ke[1]) + wave_ke[2]) + wave_ke[3];
        out[gridDim.x + blockIdx.x] = ((wave_pe[0] + wave_pe[1]) + wave_pe[2]) + wave_pe[3];
    }
}

// The reference's accuracy metric (nbody-sim-new/utils.h:170-219) on the device: a body counts as accurate
// when every force component is within 1 % of the reference's; components with |ref| < 1e-20 are held to
// |f| <= 1e-9 instead.  F = -(G m) a is formed exactly as export_forces_kernel does.
__global__ __launch_bounds__(256) void accuracy_kernel(const float* __restrict__ acc, int splits, int dim, unsigned pad,
                                                       size_t count, double G, const double* __restrict__ m64,
                                                       const double* __restrict__ ref, unsigned* __restrict__ accurate) {
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool ok = l < count;
    if (ok) {
        const double gm = G * m64[l];
        for (int k = 0; k < dim && ok; ++k) {
            const double f = -(gm * sum_partials(acc, splits, dim, pad, k, l));
            const double r = ref[l * dim + k];
            if (fabs(r) < 1e-20) ok = !(fabs(f) > 1e-9);
            else ok = !(fabs((f - r) / r) > 0.01);
        }
    }
    const unsigned long long votes = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && votes) atomicAdd(accurate, (unsigned)__popcll(votes));
}

__global__ __launch_bounds__(256) void export_aux_kernel(const float* __restrict__ aux, int planes, unsigned pad, size_t count,
                                                         double* __restrict__ out) {
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= count) return;
    double v = 0.0;
    for (int s = 0; s < planes; ++s) v += (double)aux[(size_t)s * pad + l];
    out[l] = v;
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

hipError_t launch_pack(const PackArgs& p, hipStream_t stream) {
    const size_t total = p.only_own ? (size_t)p.pad : (size_t)p.n_shards * p.pad;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(pack_kernel, dim3(blocks_for(total)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_kick_drift(const KickDriftArgs& k, hipStream_t stream) {
    if (k.count == 0) return hipSuccess;
    hipLaunchKernelGGL(kick_drift_kernel, dim3(blocks_for(k.count), (unsigned)k.dim, 1), dim3(256), 0, stream, k);
    return hipGetLastError();
}

hipError_t launch_kick_drift_slots(const SlotKickArgs& k, hipStream_t stream) {
    if (k.count == 0) return hipSuccess;
    const dim3 grid(blocks_for(k.count), (unsigned)k.dim, 1);
    if (k.drift) hipLaunchKernelGGL(kick_drift_slots_kernel<true>, grid, dim3(256), 0, stream, k);
    else hipLaunchKernelGGL(kick_drift_slots_kernel<false>, grid, dim3(256), 0, stream, k);
    return hipGetLastError();
}

hipError_t launch_slot_accel_max(const double* sums, const uint32_t* body_slot, uint32_t pslots, int dim, size_t n, double absG,
                                 unsigned long long* out, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(out, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(slot_accel_max_kernel, dim3(blocks_for(n)), dim3(256), 0, stream, sums, body_slot, pslots, dim, n, absG, out);
    return hipGetLastError();
}

hipError_t launch_step_clock_init(StepClock* clock, double accel_length, double dt_min, double dt_max, double t_start, double t_end, int pow2,
                                  uint32_t capacity, hipStream_t stream) {
    hipLaunchKernelGGL(step_clock_init_kernel, dim3(1), dim3(64), 0, stream, clock, accel_length, dt_min, dt_max, t_start, t_end, pow2, capacity);
    return hipGetLastError();
}

hipError_t launch_step_controller(const double* sums, const uint32_t* pslot_body, uint32_t pslots, int dim, double absG, StepClock* clock, bool last,
                                  hipStream_t stream) {
    hipError_t e = hipMemsetAsync(&clock->amax_bits, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    if (pslots) {
        hipLaunchKernelGGL(slot_accel_max_by_slot_kernel, dim3(blocks_for(pslots)), dim3(256), 0, stream, sums, pslot_body, pslots, dim, absG, &clock->amax_bits);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return launch_step_control(clock, last, stream);
}

hipError_t launch_step_control(StepClock* clock, bool last, hipStream_t stream) {
    hipLaunchKernelGGL(step_controller_kernel, dim3(1), dim3(64), 0, stream, clock, last ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_ctx_accel_max(const float* acc, int splits, int dim, unsigned pad, size_t count, double absG, unsigned long long* out,
                                hipStream_t stream) {
    hipError_t e = hipMemsetAsync(out, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess || count == 0) return e;
    if (dim == 2) hipLaunchKernelGGL(ctx_accel_max_kernel<2>, dim3(blocks_for(count)), dim3(256, 2, 1), 0, stream, acc, splits, pad, count, absG, out);
    else hipLaunchKernelGGL(ctx_accel_max_kernel<3>, dim3(blocks_for(count)), dim3(256, 3, 1), 0, stream, acc, splits, pad, count, absG, out);
    return hipGetLastError();
}

hipError_t launch_kick_drift_clock(const KickDriftArgs& k, const StepClock* clock, hipStream_t stream) {
    if (k.count == 0) return hipSuccess;
    hipLaunchKernelGGL(kick_drift_clock_kernel, dim3(blocks_for(k.count), (unsigned)k.dim, 1), dim3(256), 0, stream, k, clock);
    return hipGetLastError();
}

hipError_t launch_kick_drift_slots_clock(const SlotKickArgs& k, const StepClock* clock, hipStream_t stream) {
    if (k.count == 0) return hipSuccess;
    hipLaunchKernelGGL(kick_drift_slots_clock_kernel, dim3(blocks_for(k.count), (unsigned)k.dim, 1), dim3(256), 0, stream, k, clock);
    return hipGetLastError();
}

hipError_t launch_block_clock_init(const BlockStepArgs& b, double accel_length, double dt_max, double t_start, int levels, unsigned long long T_end,
                                   uint32_t max_substeps, uint32_t capacity, hipStream_t stream) {
    hipLaunchKernelGGL(block_clock_init_kernel, dim3(1), dim3(64), 0, stream, b.clock, accel_length, dt_max, t_start, levels, T_end,
                       (unsigned long long)b.count, max_substeps, capacity);
    if (b.count) hipLaunchKernelGGL(block_levels_init_kernel, dim3(blocks_for(b.count)), dim3(256), 0, stream, b.level, b.count);
    return hipGetLastError();
}

hipError_t launch_block_kick(const BlockStepArgs& b, hipStream_t stream) {
    if (b.count) hipLaunchKernelGGL(block_check_kernel, dim3(blocks_for(b.count)), dim3(256), 0, stream, b);
    hipLaunchKernelGGL(block_control_pre_kernel, dim3(1), dim3(64), 0, stream, b.clock);
    if (b.count) hipLaunchKernelGGL(block_kick_kernel, dim3(blocks_for(b.count)), dim3(256), 0, stream, b);
    return hipGetLastError();
}

hipError_t launch_block_select(const BlockStepArgs& b, hipStream_t stream) {
    if (b.count == 0) return hipSuccess;
    hipLaunchKernelGGL(block_flag_kernel, dim3(blocks_for(b.count)), dim3(256), 0, stream, b);
    hipError_t e = nbx_sort::exclusive_scan(b.flags, b.flags, &b.clock->n_bodies, (unsigned)b.count, b.tile_sums, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(block_scatter_kernel, dim3(blocks_for(b.count)), dim3(256), 0, stream, b);
    return hipGetLastError();
}

hipError_t launch_block_advance(const BlockStepArgs& b, hipStream_t stream) {
    hipLaunchKernelGGL(block_control_post_kernel, dim3(1), dim3(64), 0, stream, b.clock);
    if (b.count) hipLaunchKernelGGL(block_drift_kernel, dim3(blocks_for(b.count), (unsigned)b.dim, 1), dim3(256), 0, stream, b);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_block_select(b, stream);
}

hipError_t launch_hermite_refresh_velocities(const HermiteArgs& h, hipStream_t stream) {
    if (h.b.count) hipLaunchKernelGGL(hermite_velocity_kernel, dim3(blocks_for(h.b.count), (unsigned)h.b.dim, 1), dim3(256), 0, stream, h);
    return hipGetLastError();
}

hipError_t launch_hermite_correct(const HermiteArgs& h, hipStream_t stream) {
    if (h.b.count) hipLaunchKernelGGL(hermite_check_kernel, dim3(blocks_for(h.b.count)), dim3(256), 0, stream, h);
    hipLaunchKernelGGL(block_control_pre_kernel, dim3(1), dim3(64), 0, stream, h.b.clock);
    if (h.b.count) hipLaunchKernelGGL(hermite_correct_kernel, dim3(blocks_for(h.b.count)), dim3(256), 0, stream, h);
    return hipGetLastError();
}

hipError_t launch_hermite_advance(const HermiteArgs& h, hipStream_t stream) {
    hipLaunchKernelGGL(block_control_post_kernel, dim3(1), dim3(64), 0, stream, h.b.clock);
    if (h.b.count) hipLaunchKernelGGL(hermite_predict_kernel, dim3(blocks_for(h.b.count), (unsigned)h.b.dim, 1), dim3(256), 0, stream, h);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_block_select(h.b, stream);
}

hipError_t launch_export_forces(const float* acc, int splits, int dim, unsigned pad, size_t count, double G,
                                const double* m64, double* forces_out, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(export_forces_kernel, dim3(blocks_for(count)), dim3(256), 0, stream, acc, splits, dim, pad,
                       count, G, m64, forces_out);
    return hipGetLastError();
}

hipError_t launch_export_accel(const float* acc, int splits, int dim, unsigned pad, size_t count,
                               float* accel_out, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(export_accel_kernel, dim3(blocks_for(count)), dim3(256), 0, stream, acc, splits, dim, pad,
                       count, accel_out);
    return hipGetLastError();
}

hipError_t launch_export_energy(const float* phi, int splits, int dim, unsigned pad, size_t count, double G,
                                const double* v64, const double* m64, double* energy_out, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(energy_partials_kernel, dim3(blocks_for(count)), dim3(256), 0, stream, phi, splits, dim, pad, count,
                       G, v64, m64, energy_out);
    return hipGetLastError();
}

hipError_t launch_export_aux(const float* aux, int planes, unsigned pad, size_t count, double* out, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(export_aux_kernel, dim3(blocks_for(count)), dim3(256), 0, stream, aux, planes, pad, count, out);
    return hipGetLastError();
}

hipError_t launch_accuracy(const float* acc, int splits, int dim, unsigned pad, size_t count, double G,
                           const double* m64, const double* ref_forces, unsigned* accurate, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(accurate, 0, sizeof(unsigned), stream);
    if (e != hipSuccess || count == 0) return e;
    hipLaunchKernelGGL(accuracy_kernel, dim3(blocks_for(count)), dim3(256), 0, stream, acc, splits, dim, pad, count, G,
                       m64, ref_forces, accurate);
    return hipGetLastError();
}

hipError_t launch_export_state(const double* x64, const double* v64, int dim, unsigned pad, size_t count,
                               double* state_out, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(export_state_kernel, dim3(blocks_for(count)), dim3(256), 0, stream, x64, v64, dim, pad,
                       count, state_out);
    return hipGetLastError();
}

}  // namespace nbx
