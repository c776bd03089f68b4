// CPU model of the summation ORDER of the symmetric pass with TWO VISITORS PER LANE (force_sym_kernel.hip, D = 3), compiled
// and run by tests/test_sym_pairs_cpu.py.  Same fp32 pair terms as tests/sym_sum_model.cpp -- d = source - target exact, r^2
// by fma with the kTiny bias, w = m (1/r^2)^2, fma into the sum, 1/r^2 a correctly rounded division -- walked through
// csrc/sym_plan.h like the kernel, and added in three orders inside one walk:
//   parent:  sym_sum_model.cpp's symmetric order, restated: one group at a time; the visitor's level 1 is two chains (the
//            float2 halves, 4 home pairs per step each) added every 8 steps;
//   pairs:   a lane carries the same position of groups g (.x) and g + 1 (.y) of a chunk.  Home: per home body one chain per
//            half over the 64 steps, folded into level 2 as .x then .y.  Visitor: ONE chain, the lane's 8 home bodies in register
//            order (k = 2 q + h) per step, flushed into the visitor's level-2 slot every BLOCK steps, for BLOCK = 8 and 4.
// Levels 2 -> 3 (fp64) are the same in all of them.  The home side's level-1 and level-2 sums of "pairs" are compared with
// "parent"'s bit for bit where they arise; the counts of differing values are printed.
// usage: sym_sum_model_pairs IN.f32 OUT.f64 N      IN: [N][4] float {x, y, z, m}
//        OUT: [N][16] double {ref xyz, S, parent xyz, Q, pairs/8 xyz, Q, pairs/4 xyz, Q}
//        stdout: "home_level1_differ=<n> home_level2_differ=<n>"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../nbody-simulation-parallel_amd/csrc/sym_plan.h"

using namespace nbx;
static const float kTiny = 0x1p-47f;

static inline float pair_w2(const float* t, const float* s, float d[3]) {
    d[0] = s[0] - t[0]; d[1] = s[1] - t[1]; d[2] = s[2] - t[2];
    float r2 = std::fmaf(d[0], d[0], kTiny);
    r2 = std::fmaf(d[1], d[1], r2);
    r2 = std::fmaf(d[2], d[2], r2);
    const float w = 1.0f / r2;
    return w * w;
}

// a block's level-1 sum into the visitor's level-2 slot {x, y, z, Q}
static inline void flush(float* cur, const float* blk) {
    for (int c = 0; c < 3; ++c) cur[c] += blk[c];
    cur[3] = std::fmaf(blk[2], blk[2], std::fmaf(blk[1], blk[1], std::fmaf(blk[0], blk[0], cur[3])));
}

// visitor level 2 -> level 3: the four waves in wave order, onto the running fp64 sum of the earlier home passes
static void reduce_waves(const std::vector<float>& vb, const SymWalk& w, unsigned hp, double* slot_row0) {
    for (unsigned t = 0; t < w.groups * 64u; ++t) {
        double* dst = slot_row0 + (size_t)t * 4;
        const unsigned g = t >> 6, v = t & 63u;
        const float* b0 = &vb[(((size_t)0 * w.groups + g) * 64 + v) * 4];
        const float* b1 = &vb[(((size_t)1 * w.groups + g) * 64 + v) * 4];
        const float* b2 = &vb[(((size_t)2 * w.groups + g) * 64 + v) * 4];
        const float* b3 = &vb[(((size_t)3 * w.groups + g) * 64 + v) * 4];
        for (int c = 0; c < 3; ++c) {
            double r = -((((double)b0[c] + (double)b1[c]) + (double)b2[c]) + (double)b3[c]);
            if (hp != 0) r += dst[c];
            dst[c] = r;
        }
        const float qv = ((b0[3] + b1[3]) + b2[3]) + b3[3];
        dst[3] = (hp != 0) ? (double)((float)dst[3] + qv) : (double)qv;
    }
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const unsigned N = (unsigned)std::atoi(argv[3]);
    std::vector<float> b((size_t)N * 4);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(b.data(), sizeof(float), b.size(), f) != b.size()) return 3;
    std::fclose(f);
    SymPlan P;
    if (!sym_make_plan(N, &P) || N % 4096u != 0 || P.G < 2u) return 4;
    std::vector<double> out((size_t)N * 16, 0.0);

    // fp64 reference + magnitude sums
#pragma omp parallel for schedule(dynamic, 64)
    for (long long ii = 0; ii < (long long)N; ++ii) {
        const float* t = &b[(size_t)ii * 4];
        double r[3] = {0, 0, 0}, mag = 0;
        for (unsigned j = 0; j < N; ++j) {
            const float* s = &b[(size_t)j * 4];
            const double dx = (double)s[0] - t[0], dy = (double)s[1] - t[1], dz = (double)s[2] - t[2];
            const double r2 = dx * dx + dy * dy + dz * dz;
            if (r2 < 1e-10) continue;
            const double w = (double)s[3] / (r2 * r2);
            r[0] += w * dx; r[1] += w * dy; r[2] += w * dz; mag += w * std::sqrt(r2);
        }
        double* w = &out[(size_t)ii * 16];
        w[0] = r[0]; w[1] = r[1]; w[2] = r[2]; w[3] = mag;
    }

    // slot sums [S + K][N] {x, y, z, Q}: parent order, pairs with blocks of 8 steps, pairs with blocks of 4
    const unsigned slots = P.S + P.K;
    enum { kParent = 0, kPairs8 = 1, kPairs4 = 2, kOrders = 3 };
    std::vector<double> slot[kOrders];
    for (auto& sl : slot) sl.assign((size_t)slots * N * 4, 0.0);
    unsigned long long differ1 = 0, differ2 = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : differ1, differ2)
    for (long long wg = 0; wg < (long long)(P.B * P.S); ++wg) {
        const unsigned A = (unsigned)wg / P.S, s = (unsigned)wg % P.S;
        for (unsigned hp = 0; hp < kSymSuper / kSymHomePass; ++hp) {
            const unsigned h0 = A * kSymSuper + hp * kSymHomePass;
            if (h0 >= N) break;
            std::vector<double> sums[2] = {std::vector<double>((size_t)kSymHomePass * 3, 0.0), std::vector<double>((size_t)kSymHomePass * 3, 0.0)};
            std::vector<float> qq[2] = {std::vector<float>(kSymHomePass, 0.f), std::vector<float>(kSymHomePass, 0.f)};   // [parent, pairs]
            SymWalk w; w.k = 0; w.c = ~0u;
            while (sym_next_chunk(P, A, s, &w)) {
                if (w.groups % 2u != 0) std::abort();
                std::vector<float> l2h[2] = {std::vector<float>((size_t)kSymHomePass * 3, 0.f), std::vector<float>((size_t)kSymHomePass * 3, 0.f)};
                std::vector<float> vb[kOrders];   // visitor level 2 + Q: [wave][group][visitor]
                for (auto& v : vb) v.assign((size_t)4 * w.groups * 64 * 4, 0.f);
                for (unsigned g = 0; g < w.groups; g += 2)
                    for (unsigned wave = 0; wave < 4; ++wave) {
                        // ---- parent: group g, then group g + 1 (sym_sum_model.cpp's loops)
                        float l1p[2][64][8][3] = {};   // home level 1: [group - g][lane][2q+h]
                        for (unsigned half = 0; half < 2; ++half) {
                            float va[64][2][3] = {};   // visitor level 1 by visitor: [v][float2 half]
                            for (unsigned t = 0; t < 64; ++t) {
                                for (unsigned l = 0; l < 64; ++l) {
                                    const unsigned v = (l - t) & 63u;   // lane l receives lane l-1's visitor each step
                                    const float* sv = &b[((size_t)w.first + (g + half) * 64u + v) * 4];
                                    for (unsigned q = 0; q < 4; ++q)
                                        for (unsigned h = 0; h < 2; ++h) {
                                            const float* th = &b[(size_t)(h0 + wave * 64u + l + (2 * q + h) * 256u) * 4];
                                            float d[3];
                                            const float w2 = pair_w2(th, sv, d);
                                            const float wv = sv[3] * w2, wh = th[3] * w2;
                                            for (int c = 0; c < 3; ++c) {
                                                l1p[half][l][2 * q + h][c] = std::fmaf(wv, d[c], l1p[half][l][2 * q + h][c]);
                                                va[v][h][c] = std::fmaf(wh, d[c], va[v][h][c]);
                                            }
                                        }
                                }
                                if (t % 8u == 7u)
                                    for (unsigned v = 0; v < 64; ++v) {
                                        float blk[3];
                                        for (int c = 0; c < 3; ++c) { blk[c] = va[v][0][c] + va[v][1][c]; va[v][0][c] = va[v][1][c] = 0.f; }
                                        flush(&vb[kParent][(((size_t)wave * w.groups + g + half) * 64 + v) * 4], blk);
                                    }
                            }
                            for (unsigned l = 0; l < 64; ++l)
                                for (unsigned k = 0; k < 8; ++k) {
                                    const unsigned rel = wave * 64u + l + k * 256u;
                                    for (int c = 0; c < 3; ++c) {
                                        l2h[0][(size_t)rel * 3 + c] += l1p[half][l][k][c];
                                        qq[0][rel] = std::fmaf(l1p[half][l][k][c], l1p[half][l][k][c], qq[0][rel]);
                                    }
                                }
                        }
                        // ---- pairs: both groups in one rotation, the lane's visitors are position v of g (.x) and of g + 1 (.y)
                        float l1n[2][64][8][3] = {};        // home level 1: [half][lane][k]
                        float va8[64][2][3] = {}, va4[64][2][3] = {};   // visitor level 1: [v][half], one chain each
                        for (unsigned t = 0; t < 64; ++t) {
                            for (unsigned l = 0; l < 64; ++l) {
                                const unsigned v = (l - t) & 63u;
                                for (unsigned k = 0; k < 8; ++k) {       // register order: k = 2 q + h
                                    const float* th = &b[(size_t)(h0 + wave * 64u + l + k * 256u) * 4];
                                    for (unsigned half = 0; half < 2; ++half) {
                                        const float* sv = &b[((size_t)w.first + (g + half) * 64u + v) * 4];
                                        float d[3];
                                        const float w2 = pair_w2(th, sv, d);
                                        const float wv = sv[3] * w2, wh = th[3] * w2;
                                        for (int c = 0; c < 3; ++c) {
                                            l1n[half][l][k][c] = std::fmaf(wv, d[c], l1n[half][l][k][c]);
                                            va8[v][half][c] = std::fmaf(wh, d[c], va8[v][half][c]);
                                            va4[v][half][c] = std::fmaf(wh, d[c], va4[v][half][c]);
                                        }
                                    }
                                }
                            }
                            for (unsigned v = 0; v < 64 && t % 4u == 3u; ++v)
                                for (unsigned half = 0; half < 2; ++half) {
                                    const size_t at = (((size_t)wave * w.groups + g + half) * 64 + v) * 4;
                                    flush(&vb[kPairs4][at], va4[v][half]);
                                    va4[v][half][0] = va4[v][half][1] = va4[v][half][2] = 0.f;
                                    if (t % 8u != 7u) continue;
                                    flush(&vb[kPairs8][at], va8[v][half]);
                                    va8[v][half][0] = va8[v][half][1] = va8[v][half][2] = 0.f;
                                }
                        }
                        for (unsigned l = 0; l < 64; ++l)
                            for (unsigned k = 0; k < 8; ++k) {
                                const unsigned rel = wave * 64u + l + k * 256u;
                                for (unsigned half = 0; half < 2; ++half) {   // .x (group g), then .y (group g + 1)
                                    for (int c = 0; c < 3; ++c) l2h[1][(size_t)rel * 3 + c] += l1n[half][l][k][c];
                                    for (int c = 0; c < 3; ++c) qq[1][rel] = std::fmaf(l1n[half][l][k][c], l1n[half][l][k][c], qq[1][rel]);
                                }
                            }
                        const float* pa = &l1p[0][0][0][0];
                        const float* pn = &l1n[0][0][0][0];
                        for (size_t k = 0; k < sizeof(l1p) / sizeof(float); ++k) differ1 += std::memcmp(pa + k, pn + k, sizeof(float)) != 0;
                    }
                for (size_t k = 0; k < (size_t)kSymHomePass * 3; ++k) {
                    differ2 += std::memcmp(&l2h[0][k], &l2h[1][k], sizeof(float)) != 0;
                    sums[0][k] += (double)l2h[0][k];
                    sums[1][k] += (double)l2h[1][k];
                }
                if (!w.two_sided) continue;
                for (int o = 0; o < kOrders; ++o) reduce_waves(vb[o], w, hp, &slot[o][((size_t)(P.S + w.k - 1) * N + w.first) * 4]);
            }
            for (unsigned rel = 0; rel < kSymHomePass; ++rel) {
                differ2 += std::memcmp(&qq[0][rel], &qq[1][rel], sizeof(float)) != 0;
                for (int o = 0; o < kOrders; ++o) {
                    double* dst = &slot[o][((size_t)s * N + h0 + rel) * 4];
                    const int side = o == kParent ? 0 : 1;
                    for (int c = 0; c < 3; ++c) dst[c] = sums[side][(size_t)rel * 3 + c];
                    dst[3] = (double)qq[side][rel];
                }
            }
        }
    }
    for (unsigned i = 0; i < N; ++i)
        for (int o = 0; o < kOrders; ++o) {
            double a[4] = {0, 0, 0, 0};
            for (unsigned k = 0; k < slots; ++k)
                for (int c = 0; c < 4; ++c) a[c] += slot[o][((size_t)k * N + i) * 4 + c];
            for (int c = 0; c < 4; ++c) out[(size_t)i * 16 + 4 + 4 * o + c] = a[c];
        }
    std::printf("home_level1_differ=%llu home_level2_differ=%llu\n", differ1, differ2);
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 5;
    std::fclose(f);
    return 0;
}
