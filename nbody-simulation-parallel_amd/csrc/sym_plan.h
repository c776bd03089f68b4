// sym_plan.h -- decomposition of the symmetric own-shard force pass (force_sym_kernel.hip): which workgroup meets which
// bodies, so that every unordered pair of the shard is evaluated exactly once.  Plain C++ shared by the kernel, the
// launcher and the host-side checker (tests/sym_plan_check.cpp); no HIP types.
//
// The padded shard is cut into B super-blocks of kSymSuper bodies (the last one may hold half of that: pad is a multiple
// of 4096).  Workgroup (A, s) owns home super-block A -- held in registers kSymHomePass bodies at a time, 8 per lane --
// and meets slice s (kSymSuper / S consecutive bodies) of
//   * super-block A itself, one-sided: the home bodies collect, the visitors' reaction sums are dropped (the pair's
//     other half is collected when the roles are swapped, in the workgroup whose slice holds the home body);
//   * super-blocks A+1 .. A+K (mod B), K = floor(B/2), two-sided: both bodies of a pair collect.
// For even B the block A+K is also block A-K: the pair of blocks {lo, lo+K} belongs to lo when lo is even and to lo+K
// when it is odd, so that the extra block falls on every second workgroup of both halves.
// Results: home sums of (A, s) -> slot s, rows of A.  Reaction sums on the visitors of block A+k -> slot S + k - 1, rows of
// the visitor.  One writer per entry; S + K slots of {hi, lo} fp32 planes.
#ifndef NBX_SYM_PLAN_H
#define NBX_SYM_PLAN_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NBX_SYM_HD __host__ __device__
#else
#define NBX_SYM_HD
#endif

namespace nbx {

constexpr unsigned kSymSuper = 8192;      // bodies per super-block = 4 home passes
constexpr unsigned kSymHomePass = 2048;   // home bodies a workgroup holds at a time: 4 waves x 64 lanes x 8
constexpr unsigned kSymGroup = 64;        // visitors that rotate through one wave
constexpr unsigned kSymChunkGroups = 4;   // visitor groups between two reductions across the workgroup's waves
constexpr unsigned kSymMaxSlots = 128;    // S + K: two fp32 planes each, within the 256 planes the consumers take
constexpr unsigned kSymWantGroups = 4096; // workgroups of a launch: as many as the one-sided kernel's at N = 2^20

struct SymPlan {
    unsigned pad;   // bodies of the padded shard
    unsigned B;     // super-blocks (the last may be ragged)
    unsigned S;     // slices of a super-block's bodies = gridDim.y
    unsigned K;     // two-sided blocks per workgroup = reaction slots
    unsigned G;     // visitor groups per slice of one super-block = kSymSuper / (S * kSymGroup)
};

// false: the shard has no symmetric decomposition (fewer than two super-blocks, or more slots than the planes allow)
NBX_SYM_HD inline bool sym_make_plan(unsigned pad, SymPlan* p) {
    p->pad = pad;
    p->B = (pad + kSymSuper - 1u) / kSymSuper;
    p->K = p->B / 2u;
    p->S = 0; p->G = 0;
    if (pad == 0u || pad % (kSymSuper / 2u) != 0u || p->B < 2u || p->K + 1u > kSymMaxSlots) return false;
    unsigned S = kSymSuper / kSymGroup;   // 128: one visitor group per slice and block
    while (S > 1u && (S + p->K > kSymMaxSlots || p->B * S > kSymWantGroups)) S /= 2u;
    p->S = S;
    p->G = kSymSuper / (S * kSymGroup);
    return true;
}

// The k-th block workgroup A meets (k = 0: its own, one-sided; 1..K: two-sided).  false: the block pair belongs to the
// other side (even B, k = K only).
NBX_SYM_HD inline bool sym_visit(const SymPlan& p, unsigned A, unsigned k, unsigned* block, bool* two_sided) {
    *two_sided = k != 0u;
    *block = (A + k) % p.B;
    if (k != 0u && 2u * k == p.B) {
        const bool low = A < k;
        const unsigned lo = low ? A : A - k;
        return ((lo & 1u) == 0u) == low;
    }
    return true;
}

// Even B only: nobody writes the rows of block A in the last reaction slot when A owns its pair with the antipodal block
// (the reaction then lands on the antipode's rows).  The workgroups of A clear their slice of those rows.
NBX_SYM_HD inline bool sym_clears_last_slot(const SymPlan& p, unsigned A) {
    if (p.B % 2u != 0u) return false;
    unsigned block; bool two;
    return sym_visit(p, A, p.K, &block, &two);
}

// Visitor chunks (up to kSymChunkGroups groups, reduced together) of one home pass of workgroup (A, s), in the order the
// kernel walks them.  Start with k = 0, c = ~0u; returns false after the last chunk.
struct SymWalk { unsigned k, c, first, groups; bool two_sided; };
NBX_SYM_HD inline bool sym_next_chunk(const SymPlan& p, unsigned A, unsigned s, SymWalk* w) {
    const unsigned gc = p.G < kSymChunkGroups ? p.G : kSymChunkGroups;
    const unsigned chunks = p.G / gc;
    unsigned k = w->k, c = w->c + 1u;   // ~0u + 1 = 0: the first call
    for (; k <= p.K; ++k, c = 0u) {
        unsigned block; bool two;
        if (!sym_visit(p, A, k, &block, &two)) continue;
        const unsigned first = block * kSymSuper + s * (kSymSuper / p.S) + c * gc * kSymGroup;
        if (c >= chunks || first >= p.pad) continue;   // a ragged last block ends early (whole chunks: pad is a multiple of 4096)
        w->k = k; w->c = c; w->first = first; w->groups = gc; w->two_sided = two;
        return true;
    }
    w->k = k; w->c = 0u;
    return false;
}

}  // namespace nbx
#endif
