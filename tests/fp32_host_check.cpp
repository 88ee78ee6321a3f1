// Stand-alone host check of the fp32-ieee conv's index arithmetic (csrc/nn/fp32_forward.h): the conv
// kernel's tiling walked serially on the CPU -- the same staging loop, neighbour rows, weight-fragment
// offsets and MFMA lane maps -- against a naive 'same' convolution, with every generated index
// asserted in bounds.  Built with -fsanitize=address,undefined and run directly by
// tests/test_fp32_mode.py; exits 0 when everything holds.
#include "../galvanise_zero_amd/csrc/nn/fp32_forward.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

using namespace gzfp32;

#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

namespace {

struct Shape {
    int H, W, rows, cin, taps, F;
};

// v_mfma_f32_16x16x4_f32 on one wave: lane l holds A[l % 16][l / 16] and B[l / 16][l % 16]; D[i][j]
// accumulates the 4 k in order
void mfma16x16x4(const float (&a)[64], const float (&b)[64], float (&d)[16][16]) {
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j)
            for (int k = 0; k < 4; ++k) d[i][j] = std::fmaf(a[i + 16 * k], b[j + 16 * k], d[i][j]);
}

// the conv kernel (fp32_forward.hip conv_f32_kernel), workgroups / waves / lanes one after another
void conv_tiled(const std::vector<float>& x, const std::vector<float>& wimg, const std::vector<float>& bias,
                const Shape& s, int cinp, int FP, std::vector<float>& out) {
    const int npos = s.H * s.W, ncols = s.rows * npos, W = s.W;
    const int CT = wave_co_tiles(FP), TT = kWaveTiles, stride = lds_row_stride(), cotiles = FP >> 4;
    CHECK(FP % (32 * CT) == 0 && cinp % 16 == 0);
    const int gx = (ncols + kTileCols - 1) / kTileCols, gy = FP / (32 * CT);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int bx = 0; bx < gx; ++bx)
        for (int by = 0; by < gy; ++by) {
            std::vector<float> lds(lds_bytes(W) / sizeof(float), nan);
            const long c0 = (long)bx * kTileCols;
            for (int i = 0; i < stride; ++i) {
                const size_t o = (size_t)lds_zero_row(W) * stride + i;
                CHECK(o < lds.size());
                lds[o] = 0.f;
            }
            std::vector<float> acc((size_t)4 * CT * TT * 256, 0.f);   // [wave][ct][t][16][16]
            for (int kc = 0; kc < cinp; kc += kChunk) {
                const int kcl = cinp - kc < kChunk ? cinp - kc : kChunk, q4 = kcl >> 2, nrows = lds_zero_row(W);
                for (int i = 0; i < nrows * q4; ++i) {
                    const int r = i / q4, q = i - r * q4;
                    const long f = lds_row_column(c0, W, r);
                    const size_t lo = (size_t)r * stride + 4 * q;
                    CHECK(lo + 3 < (size_t)lds_zero_row(W) * stride);   // never the zero row
                    for (int e = 0; e < 4; ++e) {
                        float v = 0.f;
                        if (f >= 0 && f < ncols) {
                            const size_t xo = (size_t)f * cinp + kc + 4 * q + e;
                            CHECK(xo < x.size());
                            v = x[xo];
                        }
                        lds[lo + e] = v;
                    }
                }
                for (int wave = 0; wave < 4; ++wave) {
                    const int co_wave = (by * 2 + (wave & 1)) * CT * 16, tc0 = (wave >> 1) * (TT * 16);
                    for (int tp = 0; tp < s.taps; ++tp) {
                        const int tap = s.taps == 1 ? 4 : tp;
                        for (int kb = 0; kb < (kcl >> 4); ++kb)
                            for (int step = 0; step < 4; ++step)
                                for (int ct = 0; ct < CT; ++ct)
                                    for (int t = 0; t < TT; ++t) {
                                        float a[64], b[64];
                                        for (int lane = 0; lane < 64; ++lane) {
                                            const int li = lane & 15, g = lane >> 4;
                                            const long c = c0 + tc0 + 16 * t + li;
                                            const bool live = c < ncols;
                                            const int p = live ? (int)(c % npos) : 0;
                                            const int y = p / W, xx = p - y * W;
                                            const int row = nbr_row(s.H, W, y, xx, tap, tc0 + 16 * t + li, live);
                                            CHECK(row >= 0 && row < lds_rows(W));
                                            const size_t lo = (size_t)row * stride + 4 * g + 16 * kb + step;
                                            CHECK(lo < lds.size());
                                            CHECK(row == lds_zero_row(W) || 4 * g + 16 * kb + step < kcl);
                                            b[lane] = lds[lo];
                                            CHECK(!std::isnan(b[lane]));   // only staged data is read
                                            const size_t wo = (((size_t)tp * (cinp >> 4) + (kc >> 4) + kb) * cotiles +
                                                               (co_wave >> 4) + ct) * 256 + 4 * lane + step;
                                            CHECK(wo < wimg.size());
                                            a[lane] = wimg[wo];
                                        }
                                        float(&d)[16][16] = *reinterpret_cast<float(*)[16][16]>(
                                            acc.data() + ((size_t)(wave * CT + ct) * TT + t) * 256);
                                        mfma16x16x4(a, b, d);
                                    }
                    }
                }
            }
            // epilogue: lane (li, g) register r = D[4 g + r][li]
            for (int wave = 0; wave < 4; ++wave) {
                const int co_wave = (by * 2 + (wave & 1)) * CT * 16, tc0 = (wave >> 1) * (TT * 16);
                for (int ct = 0; ct < CT; ++ct)
                    for (int t = 0; t < TT; ++t)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int li = lane & 15, g = lane >> 4;
                            const long c = c0 + tc0 + 16 * t + li;
                            if (c >= ncols) continue;
                            for (int r = 0; r < 4; ++r) {
                                const int co = co_wave + 16 * ct + 4 * g + r;
                                CHECK(co < FP);
                                const size_t o = (size_t)c * FP + co;
                                CHECK(o < out.size());
                                CHECK(std::isnan(out[o]));   // every output written exactly once
                                out[o] = acc[((size_t)(wave * CT + ct) * TT + t) * 256 + (4 * g + r) * 16 + li] + bias[co];
                            }
                        }
            }
        }
}

int run(const Shape& s, unsigned seed) {
    const int npos = s.H * s.W, ncols = s.rows * npos;
    const int FP = padded_filters(s.F), cinp = s.cin == s.F ? FP : pad16(s.cin);   // trunk convs read FP channels
    CHECK(FP >= s.F && cinp >= s.cin);
    CHECK(s.H <= kMaxBoardSide && s.W <= kMaxBoardSide && lds_bytes(s.W) <= 64 * 1024);
    std::mt19937 rng(seed);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<float> w((size_t)s.taps * s.cin * s.F), scale(s.F), bias(FP, 0.f), x((size_t)ncols * cinp, 0.f);
    for (float& v : w) v = nd(rng);
    for (float& v : scale) v = 0.5f + std::fabs(nd(rng));
    for (int co = 0; co < s.F; ++co) bias[co] = nd(rng);
    for (int c = 0; c < ncols; ++c)
        for (int ci = 0; ci < s.cin; ++ci) x[(size_t)c * cinp + ci] = nd(rng);
    std::vector<float> wimg(conv_image_floats(s.taps, cinp, FP), 0.f);
    // every model weight lands on its own in-bounds slot
    std::vector<char> used(wimg.size(), 0);
    for (int tap = 0; tap < s.taps; ++tap)
        for (int ci = 0; ci < cinp; ++ci)
            for (int co = 0; co < FP; ++co) {
                const size_t o = wfrag_index(tap, co, ci, cinp, FP);
                CHECK(o < wimg.size() && !used[o]);
                used[o] = 1;
            }
    pack_conv_host(wimg.data(), w.data(), scale.data(), s.taps, s.cin, cinp, s.F, FP);

    std::vector<float> out((size_t)ncols * FP, std::numeric_limits<float>::quiet_NaN());
    conv_tiled(x, wimg, bias, s, cinp, FP, out);

    double worst = 0.0;
    for (int c = 0; c < ncols; ++c) {
        const int p = c % npos, y = p / s.W, xx = p % s.W;
        for (int co = 0; co < FP; ++co) {
            double ref = bias[co], mag = std::fabs(bias[co]);
            if (co < s.F)
                for (int tp = 0; tp < s.taps; ++tp) {
                    const int tap = s.taps == 1 ? 4 : tp, yy = y + tap / 3 - 1, xn = xx + tap % 3 - 1;
                    if (yy < 0 || yy >= s.H || xn < 0 || xn >= s.W) continue;
                    const float* xr = &x[(size_t)(c + (tap / 3 - 1) * s.W + (tap % 3 - 1)) * cinp];
                    for (int ci = 0; ci < s.cin; ++ci) {
                        const double t = (double)(w[((size_t)tp * s.cin + ci) * s.F + co] * scale[co]) * xr[ci];
                        ref += t;
                        mag += std::fabs(t);
                    }
                }
            const double got = out[(size_t)c * FP + co];
            CHECK(!std::isnan(got));
            const double e = std::fabs(got - ref) / (mag + 1.0);
            if (e > worst) worst = e;
        }
    }
    std::printf("H=%d W=%d rows=%d cin=%d taps=%d F=%d (FP %d): max rel err %.3g\n", s.H, s.W, s.rows, s.cin, s.taps, s.F, FP,
                worst);
    // an fp32 fmaf chain against double: far below 2e-5 of the sum of magnitudes; an index slip is O(1)
    return worst <= 2e-5 ? 0 : 1;
}

}  // namespace

int main() {
    int bad = 0;
    unsigned seed = 1;
    // boards: partial position tiles (6 x 6 x 5 rows = 180 columns, 13 x 13, 19 x 19) and a whole
    // number of full tiles (8 x 8 x 4 rows = 256 columns)
    const int boards[4][3] = {{6, 6, 5}, {8, 8, 4}, {13, 13, 2}, {19, 19, 1}};
    for (const auto& b : boards) {
        for (int cin : {3, 15, 24})        // initial convs, 3 x 3
            for (int F : {64, 80, 256}) bad += run(Shape{b[0], b[1], b[2], cin, 9, F}, seed++);
        bad += run(Shape{b[0], b[1], b[2], 15, 1, 80}, seed++);   // a v2 net's 1 x 1 initial conv
        for (int F : {64, 80})             // trunk convs (input channels = the padded filters)
            bad += run(Shape{b[0], b[1], b[2], F, 9, F}, seed++);
    }
    bad += run(Shape{6, 6, 5, 256, 9, 256}, seed++);   // F = 256 trunk conv: four input-channel chunks
    bad += run(Shape{7, 19, 1, 24, 9, 64}, seed++);    // a non-square board, W > H
    bad += run(Shape{19, 5, 2, 3, 9, 64}, seed++);     // and H > W

    // row chunks cover a launch exactly once, in order
    for (int n : {1, 7, 64, 65, 2731})
        for (int chunk : {1, 5, 64, 948, 1 << 20}) {
            int next = 0;
            for (int i = 0; i < chunk_count(n, chunk); ++i) {
                int first, count;
                chunk_bounds(n, chunk, i, &first, &count);
                CHECK(first == next && count >= 1 && count <= chunk);
                next += count;
            }
            CHECK(next == n);
        }
    // the scratch of a chunk stays within its limit for every supported geometry
    for (int side : {6, 8, 13, 19})
        for (int FP : {64, 128, 256})
            for (int CP : {16, 32, 64}) {
                const int rows = chunk_rows_for(side * side, CP, FP);
                const ScratchLayout L = scratch_layout(rows, side * side, CP, FP);
                CHECK(rows >= 1 && L.total <= kScratchMax);
                CHECK(L.in < L.s && L.s < L.t && L.t < L.x && L.x < L.gate && L.gate < L.total);
            }
    if (bad) std::fprintf(stderr, "%d shapes failed\n", bad);
    return bad ? 1 : 0;
}
