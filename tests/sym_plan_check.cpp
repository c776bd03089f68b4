// Host-side checker of the symmetric pass's decomposition (csrc/sym_plan.h), compiled and run by tests/test_sym_plan_cpu.py.
// For every shard size given on the command line it walks every workgroup (A, s), every home pass and every visitor chunk
// exactly as the kernel does (sym_next_chunk) and checks that
//   * every ORDERED pair of bodies (target, source) is collected exactly once -- a two-sided chunk collects both orders,
//     the own block's one-sided chunks one -- which is "every unordered pair met exactly once" plus the diagonal rule;
//   * every entry of a reaction slot has exactly one writer, or none and is then cleared by the rows' own workgroups;
//   * every entry of a home slot has exactly one writer; no slot index reaches S + K; chunks lie inside the padded shard.
// Bodies are counted in units of `unit` consecutive bodies (a divisor of every chunk and home pass).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../nbody-simulation-parallel_amd/csrc/sym_plan.h"

using namespace nbx;

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAIL pad=%u: ", pad); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

static int check(unsigned pad) {
    SymPlan P;
    const bool ok = sym_make_plan(pad, &P);
    const unsigned blocks = (pad + kSymSuper - 1) / kSymSuper;
    if (blocks < 2 || pad % 4096 != 0 || blocks / 2 + 1 > kSymMaxSlots) {
        CHECK(!ok, "a plan for a shard that has none");
        std::printf("pad=%u: no plan (as expected)\n", pad);
        return 0;
    }
    CHECK(ok, "no plan");
    CHECK(P.B == blocks && P.K == P.B / 2 && P.S >= 1 && P.S + P.K <= kSymMaxSlots, "B=%u K=%u S=%u", P.B, P.K, P.S);
    CHECK(P.S * P.G * kSymGroup == kSymSuper, "slices x groups do not tile a super-block: S=%u G=%u", P.S, P.G);
    const unsigned gc = P.G < kSymChunkGroups ? P.G : kSymChunkGroups;
    const unsigned unit = gc * kSymGroup;   // chunk length; divides the home pass
    CHECK(kSymHomePass % unit == 0 && pad % unit == 0, "unit %u", unit);
    const size_t U = pad / unit;
    std::vector<unsigned char> met(U * U, 0);                              // [target unit][source unit]
    std::vector<unsigned char> rw((size_t)P.K * U, 0), rc((size_t)P.K * U, 0);   // reaction slots: writers, clears
    std::vector<unsigned char> hw((size_t)P.S * U, 0);                     // home slots: writers
    for (unsigned A = 0; A < P.B; ++A)
        for (unsigned s = 0; s < P.S; ++s) {
            if (sym_clears_last_slot(P, A)) {
                CHECK(P.K >= 1, "clear without a slot");
                const unsigned len = kSymSuper / P.S;
                for (unsigned t = 0; t < len; t += unit) {
                    const size_t v = (size_t)A * kSymSuper + (size_t)s * len + t;
                    if (v < pad) ++rc[(size_t)(P.K - 1) * U + v / unit];
                }
            }
            for (unsigned hp = 0; hp < kSymSuper / kSymHomePass; ++hp) {
                const unsigned h0 = A * kSymSuper + hp * kSymHomePass;
                if (h0 >= pad) break;
                CHECK(h0 + kSymHomePass <= pad, "home pass beyond the shard");
                for (unsigned h = h0; h < h0 + kSymHomePass; h += unit) ++hw[(size_t)s * U + h / unit];
                SymWalk w; w.k = 0; w.c = ~0u;
                unsigned last_k = 0;
                while (sym_next_chunk(P, A, s, &w)) {
                    CHECK(w.k <= P.K && w.k >= last_k, "walk order");
                    last_k = w.k;
                    CHECK(w.groups == gc && w.first % unit == 0 && (size_t)w.first + unit <= pad, "chunk at %u", w.first);
                    CHECK(w.two_sided == (w.k != 0), "sidedness");
                    const size_t vu = w.first / unit;
                    for (unsigned h = h0; h < h0 + kSymHomePass; h += unit) {
                        const size_t hu = h / unit;
                        CHECK(met[hu * U + vu] < 200 && met[vu * U + hu] < 200, "overflow");
                        ++met[hu * U + vu];
                        if (w.two_sided) ++met[vu * U + hu];
                    }
                    if (w.two_sided && hp == 0) {   // later home passes add onto the same entries: same writer
                        CHECK(w.k >= 1 && P.S + w.k - 1 < P.S + P.K, "slot");
                        ++rw[(size_t)(w.k - 1) * U + vu];
                    }
                }
            }
        }
    for (size_t i = 0; i < U * U; ++i) CHECK(met[i] == 1, "units (%zu <- %zu) met %d times", i / U, i % U, (int)met[i]);
    for (size_t i = 0; i < (size_t)P.K * U; ++i)
        CHECK(rw[i] + rc[i] == 1, "reaction slot %zu unit %zu: %d writers, %d clears", i / U, i % U, (int)rw[i], (int)rc[i]);
    for (size_t i = 0; i < (size_t)P.S * U; ++i) CHECK(hw[i] == 1, "home slot %zu unit %zu: %d writers", i / U, i % U, (int)hw[i]);
    std::printf("pad=%u: B=%u S=%u K=%u G=%u workgroups=%u slots=%u ok\n", pad, P.B, P.S, P.K, P.G, P.B * P.S, P.S + P.K);
    return 0;
}

int main(int argc, char** argv) {
    int bad = 0, n = 0;
    for (int i = 1; i < argc; ++i, ++n) bad += check((unsigned)std::strtoul(argv[i], nullptr, 10));
    std::printf("%s %d shard sizes\n", bad ? "FAILED" : "OK", n);
    return bad ? 1 : 0;
}
