// CPU model of the summation ORDER of the force kernels (compiled and run by tests/test_sym_plan_cpu.py): the same fp32
// pair terms -- d = source - target exact, r^2 by fma with the kTiny bias, w = m (1/r^2)^2, fma into the sum -- added in
//   (1) the one-sided three-level order of accel_fast3l_kernel: 64-source blocks -> 256-source tile -> fp64 slice sums;
//   (2) the symmetric pass's order on both sides (force_sym_kernel.hip, walked through csrc/sym_plan.h like the kernel):
//       home:    64 steps of one visitor group -> the groups of a chunk -> fp64;
//       visitor: 8 steps x 4 home pairs per float2 half -> 8 blocks of a rotation -> fp64 over waves, home passes, slots;
// next to the fp64 sum of the fp64 terms and the magnitude sum S_i.  1/r^2 is a correctly rounded division here (the
// device's v_rcp_f32 is good to 1 ulp): the model is about the order of the additions, not the reciprocal.
// usage: sym_sum_model IN.f32 OUT.f64 N S1     IN: [N][4] float {x, y, z, m};  S1: source slices of the one-sided launch
//        OUT: [N][12] double {ref xyz, S, one-sided xyz, Q, symmetric xyz, Q}
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../nbody-simulation-parallel_amd/csrc/sym_plan.h"

using namespace nbx;
static const float kTiny = 0x1p-47f;

struct Term { float wx, d[3]; };
// the pair arithmetic shared by both kernels: returns w^2 (without a mass) and d = p_s - p_t
static inline float pair_w2(const float* t, const float* s, float d[3]) {
    d[0] = s[0] - t[0]; d[1] = s[1] - t[1]; d[2] = s[2] - t[2];
    float r2 = std::fmaf(d[0], d[0], kTiny);
    r2 = std::fmaf(d[1], d[1], r2);
    r2 = std::fmaf(d[2], d[2], r2);
    const float w = 1.0f / r2;
    return w * w;
}

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const unsigned N = (unsigned)std::atoi(argv[3]), S1 = (unsigned)std::atoi(argv[4]);
    std::vector<float> b((size_t)N * 4);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(b.data(), sizeof(float), b.size(), f) != b.size()) return 3;
    std::fclose(f);
    SymPlan P;
    if (!sym_make_plan(N, &P) || N % 4096u != 0 || (N / 256u) % S1 != 0) return 4;
    std::vector<double> out((size_t)N * 12, 0.0);

    // fp64 reference + magnitude sums, and the one-sided three-level order
#pragma omp parallel for schedule(dynamic, 64)
    for (long long ii = 0; ii < (long long)N; ++ii) {
        const unsigned i = (unsigned)ii;
        const float* t = &b[(size_t)i * 4];
        double r[3] = {0, 0, 0}, mag = 0;
        for (unsigned j = 0; j < N; ++j) {
            const float* s = &b[(size_t)j * 4];
            const double dx = (double)s[0] - t[0], dy = (double)s[1] - t[1], dz = (double)s[2] - t[2];
            const double r2 = dx * dx + dy * dy + dz * dz;
            if (r2 < 1e-10) continue;
            const double w = (double)s[3] / (r2 * r2);
            r[0] += w * dx; r[1] += w * dy; r[2] += w * dz; mag += w * std::sqrt(r2);
        }
        double o[3] = {0, 0, 0}, Q = 0;
        const unsigned tiles_per_slice = N / 256u / S1;
        for (unsigned sl = 0; sl < S1; ++sl) {
            double s3[3] = {0, 0, 0}; float q = 0.f;
            for (unsigned tl = 0; tl < tiles_per_slice; ++tl) {
                float l2[3] = {0, 0, 0};
                for (unsigned blk = 0; blk < 4; ++blk) {
                    float l1[3] = {0, 0, 0};
                    for (unsigned k = 0; k < 64; ++k) {
                        const float* s = &b[((size_t)(sl * tiles_per_slice + tl) * 256u + blk * 64u + k) * 4];
                        float d[3];
                        const float w = s[3] * pair_w2(t, s, d);
                        for (int c = 0; c < 3; ++c) l1[c] = std::fmaf(w, d[c], l1[c]);
                    }
                    for (int c = 0; c < 3; ++c) { l2[c] += l1[c]; q = std::fmaf(l1[c], l1[c], q); }
                }
                for (int c = 0; c < 3; ++c) s3[c] += (double)l2[c];
            }
            for (int c = 0; c < 3; ++c) o[c] += s3[c];
            Q += (double)q;
        }
        double* w = &out[(size_t)i * 12];
        w[0] = r[0]; w[1] = r[1]; w[2] = r[2]; w[3] = mag; w[4] = o[0]; w[5] = o[1]; w[6] = o[2]; w[7] = Q;
    }

    // the symmetric pass: slot sums [S + K][N] {x, y, z, Q}
    const unsigned slots = P.S + P.K;
    std::vector<double> slot((size_t)slots * N * 4, 0.0);
#pragma omp parallel for schedule(dynamic, 1)
    for (long long wg = 0; wg < (long long)(P.B * P.S); ++wg) {
        const unsigned A = (unsigned)wg / P.S, s = (unsigned)wg % P.S;
        for (unsigned hp = 0; hp < kSymSuper / kSymHomePass; ++hp) {
            const unsigned h0 = A * kSymSuper + hp * kSymHomePass;
            if (h0 >= N) break;
            std::vector<double> sums((size_t)kSymHomePass * 3, 0.0);   // home level 3, by (body - h0)
            std::vector<float> qq(kSymHomePass, 0.f);
            SymWalk w; w.k = 0; w.c = ~0u;
            while (sym_next_chunk(P, A, s, &w)) {
                std::vector<float> l2h((size_t)kSymHomePass * 3, 0.f);         // home level 2
                std::vector<float> vb((size_t)4 * w.groups * 64 * 4, 0.f);    // visitor level 2 + Q: [wave][group][visitor]
                for (unsigned g = 0; g < w.groups; ++g)
                    for (unsigned wave = 0; wave < 4; ++wave) {
                        float l1h[64][8][3] = {};       // home level 1: [lane][2q+h]
                        float va[64][2][3] = {};        // visitor level 1 by visitor: [v][half]
                        for (unsigned t = 0; t < 64; ++t) {
                            for (unsigned l = 0; l < 64; ++l) {
                                const unsigned v = (l - t) & 63u;   // lane l receives lane l-1's visitor each step
                                const float* sv = &b[((size_t)w.first + g * 64u + v) * 4];
                                for (unsigned q = 0; q < 4; ++q)
                                    for (unsigned h = 0; h < 2; ++h) {
                                        const unsigned home = h0 + wave * 64u + l + (2 * q + h) * 256u;
                                        const float* th = &b[(size_t)home * 4];
                                        float d[3];
                                        const float w2 = pair_w2(th, sv, d);
                                        const float wv = sv[3] * w2, wh = th[3] * w2;
                                        for (int c = 0; c < 3; ++c) {
                                            l1h[l][2 * q + h][c] = std::fmaf(wv, d[c], l1h[l][2 * q + h][c]);
                                            va[v][h][c] = std::fmaf(wh, d[c], va[v][h][c]);
                                        }
                                    }
                            }
                            if (t % 8u == 7u)
                                for (unsigned v = 0; v < 64; ++v) {
                                    float* cur = &vb[(((size_t)wave * w.groups + g) * 64 + v) * 4];
                                    float blk[3];
                                    for (int c = 0; c < 3; ++c) { blk[c] = va[v][0][c] + va[v][1][c]; cur[c] += blk[c]; va[v][0][c] = va[v][1][c] = 0.f; }
                                    cur[3] = std::fmaf(blk[2], blk[2], std::fmaf(blk[1], blk[1], std::fmaf(blk[0], blk[0], cur[3])));
                                }
                        }
                        for (unsigned l = 0; l < 64; ++l)
                            for (unsigned k = 0; k < 8; ++k) {
                                const unsigned rel = wave * 64u + l + k * 256u;
                                for (int c = 0; c < 3; ++c) {
                                    l2h[(size_t)rel * 3 + c] += l1h[l][k][c];
                                    qq[rel] = std::fmaf(l1h[l][k][c], l1h[l][k][c], qq[rel]);
                                }
                            }
                    }
                for (size_t k = 0; k < (size_t)kSymHomePass * 3; ++k) sums[k] += (double)l2h[k];
                if (!w.two_sided) continue;
                for (unsigned t = 0; t < w.groups * 64u; ++t) {
                    double* dst = &slot[((size_t)(P.S + w.k - 1) * N + w.first + t) * 4];
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
            for (unsigned rel = 0; rel < kSymHomePass; ++rel) {
                double* dst = &slot[((size_t)s * N + h0 + rel) * 4];
                for (int c = 0; c < 3; ++c) dst[c] = sums[(size_t)rel * 3 + c];
                dst[3] = (double)qq[rel];
            }
        }
    }
    for (unsigned i = 0; i < N; ++i) {
        double a[4] = {0, 0, 0, 0};
        for (unsigned k = 0; k < slots; ++k)
            for (int c = 0; c < 4; ++c) a[c] += slot[((size_t)k * N + i) * 4 + c];
        for (int c = 0; c < 4; ++c) out[(size_t)i * 12 + 8 + c] = a[c];
    }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 5;
    std::fclose(f);
    return 0;
}
