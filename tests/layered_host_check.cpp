// Stand-alone host check of the layered bf16 conv's index arithmetic (csrc/nn/layered_forward.h): the
// conv kernel's tiling walked serially on the CPU using only the shared header's index functions --
// the LDS row of a column and tap (gzfp32::nbr_row / lds_row_column), the staged channel's offset,
// the B-fragment address, the A-fragment offsets into the trunk (wres_index order) and initial-conv
// ([K0 / 32][FP][32]) images -- with the weights pack_image_host made, against a direct convolution
// of the same bf16-rounded operands (hi hi [+ hi lo + lo hi]), both summed in double: any index slip
// is O(1), agreement is to rounding.  Every generated index is asserted in bounds.  Also: the
// layered modes' image of a net equals the fused modes' byte for byte.  Built with
// -fsanitize=address,undefined and run directly by tests/test_layered_mode.py; exits 0 when
// everything holds.
#include "../galvanise_zero_amd/csrc/nn/layered_forward.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

using namespace gzlayered;
using namespace gzw;
using gzfp32::lds_row_column;
using gzfp32::lds_rows;
using gzfp32::lds_zero_row;
using gzfp32::nbr_row;

#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

namespace {

float bf(uint16_t h) { return __builtin_bit_cast(float, (uint32_t)h << 16); }

struct Net {
    const char* name;
    gz_net_desc d;
    int rows;
};

gz_net_desc desc(int C, int H, int W, int F, int B, int k0, bool v2) {
    gz_net_desc d{};
    d.input_channels = C; d.input_columns = H; d.input_rows = W;
    d.cnn_filter_size = F; d.cnn_kernel_size = 3; d.residual_layers = B;
    d.role_count = 2; d.policy_dist_count[0] = 7; d.policy_dist_count[1] = 9;
    d.value_hidden_size = 6;
    d.num_values = 2;
    d.resnet_v2 = v2 ? 1 : 0;
    d.initial_kernel = k0;
    d.initial_bn = 1;
    return d;
}

// One conv as the kernel runs it (layered_forward.hip conv_bf16_kernel), workgroups / waves / lanes
// one after another.  x [ncols][cinp] fp32; img the bf16 image (whi / wlo: element offsets of the hi
// and lo images of this conv); w0: the initial conv's layout (taps == 1).
void conv_tiled(const std::vector<float>& x, int ncols, int cinp, int taps, int H, int W, int FP, int P,
                const std::vector<uint16_t>& img, size_t whi, size_t wlo, bool w0, std::vector<double>& out) {
    const int npos = H * W, NP = operand_parts(P);
    const int CT = gzfp32::wave_co_tiles(FP), TT = kWaveTiles, stride = lds_row_bytes(P);
    CHECK(FP % (32 * CT) == 0 && cinp % kStep == 0 && (taps == 1 || taps == 9));
    CHECK(lds_bytes(W, P) <= 64 * 1024 && stride % 16 == 0);
    const int gx = (ncols + kTileCols - 1) / kTileCols, gy = FP / (32 * CT);
    const uint16_t poison = 0x7fc0;   // a bf16 NaN: only staged data may be read
    for (int bx = 0; bx < gx; ++bx)
        for (int by = 0; by < gy; ++by) {
            std::vector<uint16_t> lds(lds_bytes(W, P) / 2, poison);
            const long c0 = (long)bx * kTileCols;
            for (int i = 0; i < stride / 2; ++i) {
                const size_t o = (size_t)lds_zero_row(W) * (stride / 2) + i;
                CHECK(o < lds.size());
                lds[o] = 0;
            }
            std::vector<double> acc((size_t)4 * CT * TT * 256, 0.0);   // [wave][ct][t][16][16]
            for (int kc = 0; kc < cinp; kc += kChunk) {
                const int kcl = cinp - kc < kChunk ? cinp - kc : kChunk, nrows = lds_zero_row(W);
                CHECK(kcl % kStep == 0);
                for (int r = 0; r < nrows; ++r)
                    for (int cc = 0; cc < kcl; ++cc) {
                        const long f = lds_row_column(c0, W, r);
                        float v = 0.f;
                        if (f >= 0 && f < ncols) {
                            const size_t xo = (size_t)f * cinp + kc + cc;
                            CHECK(xo < x.size());
                            v = x[xo];
                        }
                        for (int part = 0; part < NP; ++part) {
                            const size_t o = (size_t)r * stride + lds_channel_offset(cc, part);
                            CHECK(o % 2 == 0 && o + 1 < (size_t)lds_zero_row(W) * stride);   // never the zero row
                            CHECK(lds_channel_offset(cc, part) + 1 < stride);
                            lds[o / 2] = part ? lo_of(v) : f2bf(v);
                        }
                    }
                for (int wave = 0; wave < 4; ++wave) {
                    const int cot0 = (by * 2 + (wave & 1)) * CT, tc0 = (wave >> 1) * (TT * 16);
                    for (int tp = 0; tp < taps; ++tp) {
                        const int tap = taps == 1 ? 4 : tp;
                        for (int ks = 0; ks < (kcl >> 5); ++ks) {
                            const int kstep = (kc >> 5) + ks;
                            // fragments: [part][tile][lane][8]
                            std::vector<float> A((size_t)2 * CT * 64 * 8, 0.f), B((size_t)2 * TT * 64 * 8, 0.f);
                            for (int part = 0; part < NP; ++part)
                                for (int lane = 0; lane < 64; ++lane) {
                                    const int li = lane & 15, g = lane >> 4;
                                    for (int ct = 0; ct < CT; ++ct) {
                                        const size_t wo = w0 ? (part ? wlo : whi) + w0_frag_index(kstep, cot0 + ct, li, g, FP)
                                                             : whi + wres_frag_index(tp, kstep, cot0 + ct, li, g, part, FP, NP);
                                        CHECK(wo + 7 < img.size());
                                        for (int e = 0; e < 8; ++e) A[(((size_t)part * CT + ct) * 64 + lane) * 8 + e] = bf(img[wo + e]);
                                    }
                                    for (int t = 0; t < TT; ++t) {
                                        const long c = c0 + tc0 + 16 * t + li;
                                        const bool live = c < ncols;
                                        const int p = live ? (int)(c % npos) : 0;
                                        const int y = p / W, xx = p - y * W;
                                        const int row = nbr_row(H, W, y, xx, tap, tc0 + 16 * t + li, live);
                                        CHECK(row >= 0 && row < lds_rows(W));
                                        const int o = bfrag_addr(row, ks, g, part, P);
                                        CHECK(o % 16 == 0 && (size_t)o / 2 + 7 < lds.size());
                                        CHECK(o - row * stride + 16 <= stride);
                                        for (int e = 0; e < 8; ++e) {
                                            const uint16_t h = lds[o / 2 + e];
                                            CHECK(h != poison);
                                            B[(((size_t)part * TT + t) * 64 + lane) * 8 + e] = bf(h);
                                        }
                                    }
                                }
                            // v_mfma_f32_16x16x32_bf16: lane l holds A[l % 16][8 (l / 16) ..] and B[8 (l / 16) ..][l % 16];
                            // the products of a k-step in the kernel's order hi hi, hi lo, lo hi
                            const int prod[3][2] = {{0, 0}, {0, 1}, {1, 0}};
                            for (int pr = 0; pr < (P == 3 ? 3 : 1); ++pr)
                                for (int ct = 0; ct < CT; ++ct)
                                    for (int t = 0; t < TT; ++t) {
                                        const float* a = &A[((size_t)prod[pr][0] * CT + ct) * 512];
                                        const float* b = &B[((size_t)prod[pr][1] * TT + t) * 512];
                                        double* d = &acc[((size_t)(wave * CT + ct) * TT + t) * 256];
                                        for (int i = 0; i < 16; ++i)
                                            for (int j = 0; j < 16; ++j) {
                                                double s = 0.0;
                                                for (int k = 0; k < 32; ++k)
                                                    s += (double)a[(i + 16 * (k >> 3)) * 8 + (k & 7)] * b[(j + 16 * (k >> 3)) * 8 + (k & 7)];
                                                d[i * 16 + j] += s;
                                            }
                                    }
                        }
                    }
                }
            }
            // epilogue: lane (li, g) register r = D[4 g + r][li]
            for (int wave = 0; wave < 4; ++wave) {
                const int cot0 = (by * 2 + (wave & 1)) * CT, tc0 = (wave >> 1) * (TT * 16);
                for (int ct = 0; ct < CT; ++ct)
                    for (int t = 0; t < TT; ++t)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int li = lane & 15, g = lane >> 4;
                            const long c = c0 + tc0 + 16 * t + li;
                            if (c >= ncols) continue;
                            for (int r = 0; r < 4; ++r) {
                                const int co = 16 * (cot0 + ct) + 4 * g + r;
                                CHECK(co < FP);
                                const size_t o = (size_t)c * FP + co;
                                CHECK(o < out.size());
                                CHECK(std::isnan(out[o]));   // every output written exactly once
                                out[o] = acc[((size_t)(wave * CT + ct) * TT + t) * 256 + (4 * g + r) * 16 + li];
                            }
                        }
            }
        }
}

// an operand as the kernel sees it: bf16 hi and (P = 3) lo
struct Split {
    double hi, lo;
};
Split split(float v, int P) { return Split{bf(f2bf(v)), P == 3 ? bf(lo_of(v)) : 0.0}; }
// the sum of the parts' products of one weight and one activation: hi hi [+ hi lo + lo hi]
double product(const Split& w, const Split& x) { return w.hi * x.hi + w.hi * x.lo + w.lo * x.hi; }

double compare(const std::vector<double>& got, const std::vector<double>& ref, const std::vector<double>& mag) {
    double worst = 0.0;
    CHECK(got.size() == ref.size());
    for (size_t i = 0; i < got.size(); ++i) {
        CHECK(!std::isnan(got[i]));
        worst = std::max(worst, std::fabs(got[i] - ref[i]) / (mag[i] + 1.0));
    }
    return worst;
}

// the image of the net in `precision`, its spec and layout
struct Packed {
    PackSpec s;
    ImageLayout I;
    std::vector<char> img;
};
Packed pack(const gz_net_desc& d, int precision, int fpad, const std::vector<float>& blob) {
    Packed k;
    k.s = pack_spec(d, precision, fpad, false);
    k.I = image_layout(k.s);
    k.img.assign(k.I.total, 0);
    pack_image_host(job_list(k.s, blob_plan(d), k.I), blob.data(), RawImage{k.img.data()});
    return k;
}

int run(const Net& n, int P, unsigned seed) {
    const gz_net_desc& d = n.d;
    const int H = d.input_columns, W = d.input_rows, npos = H * W, ncols = n.rows * npos;
    const int F = d.cnn_filter_size, C = d.input_channels, FP = gzfp32::padded_filters(F);
    const int T0 = initial_kernel(d) * initial_kernel(d);
    CHECK(FP >= F && H <= gzfp32::kMaxBoardSide && W <= gzfp32::kMaxBoardSide);
    const BlobPlan plan = blob_plan(d);
    std::mt19937 rng(seed);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<float> blob(plan.consumed);
    for (float& v : blob) v = nd(rng);
    for (const BNRef& b : plan.folds)
        if (b.g != kNone)
            for (int i = 0; i < b.n; ++i) blob[b.var + i] = 0.5f + std::fabs(blob[b.var + i]);
    std::vector<float> fold((size_t)plan.fold_floats);
    for (const BNRef& b : plan.folds)
        for (int i = 0; i < b.n; ++i) fold_element(b, i, blob.data(), fold.data());
    const Packed k = pack(d, P == 3 ? GZ_PRECISION_SPLIT_LAYERED : GZ_PRECISION_BF16_LAYERED, FP, blob);
    CHECK(k.s.p2 == operand_parts(P) && !k.s.fp32 && k.I.total % 2 == 0);
    std::vector<uint16_t> img(k.I.total / 2);
    std::memcpy(img.data(), k.img.data(), k.I.total);
    const double nan = std::numeric_limits<double>::quiet_NaN();

    // ---- the initial conv: planes -> im2col image -> 1-tap conv over the w0 image
    const int K0 = k.s.K0;
    std::vector<float> planes((size_t)n.rows * C * npos);
    for (float& v : planes) v = nd(rng);
    std::vector<float> col((size_t)ncols * K0, -1.f);
    for (int c = 0; c < ncols; ++c)
        for (int kk = 0; kk < K0; ++kk) {
            const int row = c / npos, p = c % npos;
            float v = 0.f;
            int ch, dy, dx;
            if (im2col_source(kk, C, T0, &ch, &dy, &dx)) {
                CHECK(ch >= 0 && ch < C);
                const int y = p / W + dy, x = p % W + dx;
                if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) v = planes[((size_t)row * C + ch) * npos + y * W + x];
            }
            col[(size_t)c * K0 + kk] = v;
        }
    std::vector<double> out0((size_t)ncols * FP, nan), ref0((size_t)ncols * FP, 0.0), mag0((size_t)ncols * FP, 0.0);
    CHECK(k.I.w0 % 2 == 0 && k.I.w0lo % 2 == 0);
    conv_tiled(col, ncols, K0, 1, H, W, FP, P, img, k.I.w0 / 2, k.I.w0lo / 2, true, out0);
    for (int c = 0; c < ncols; ++c) {
        const int row = c / npos, p = c % npos, y = p / W, x = p % W;
        for (int tp = 0; tp < T0; ++tp) {
            const int tap = T0 == 1 ? 4 : tp, yy = y + tap / 3 - 1, xn = x + tap % 3 - 1;
            if (yy < 0 || yy >= H || xn < 0 || xn >= W) continue;
            for (int ci = 0; ci < C; ++ci) {
                const Split xv = split(planes[((size_t)row * C + ci) * npos + yy * W + xn], P);
                for (int co = 0; co < F; ++co) {
                    const float w = f_mul(blob[plan.w0 + ((size_t)tp * C + ci) * F + co], fold[plan.bn0.scale() + co]);
                    const double t = product(split(w, P), xv);
                    ref0[(size_t)c * FP + co] += t;
                    mag0[(size_t)c * FP + co] += std::fabs(t);
                }
            }
        }
    }
    const double e0 = compare(out0, ref0, mag0);

    // ---- the first trunk conv over random activations (padded channels too: their weights are zero)
    std::vector<float> x((size_t)ncols * FP);
    for (float& v : x) v = nd(rng);
    std::vector<double> out1((size_t)ncols * FP, nan), ref1((size_t)ncols * FP, 0.0), mag1((size_t)ncols * FP, 0.0);
    CHECK(d.residual_layers >= 1 && k.I.wres % 2 == 0);
    conv_tiled(x, ncols, FP, 9, H, W, FP, P, img, k.I.wres / 2, 0, false, out1);
    std::vector<Split> ws((size_t)9 * F * F), xs(x.size());
    for (size_t i = 0; i < ws.size(); ++i) ws[i] = split(f_mul(blob[plan.wconv[0] + i], fold[plan.bnconv[0].scale() + i % F]), P);
    for (size_t i = 0; i < xs.size(); ++i) xs[i] = split(x[i], P);
    for (int c = 0; c < ncols; ++c) {
        const int p = c % npos, y = p / W, xx = p % W;
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
            if (y + dy < 0 || y + dy >= H || xx + dx < 0 || xx + dx >= W) continue;
            const Split* xr = &xs[(size_t)(c + dy * W + dx) * FP];
            for (int ci = 0; ci < F; ++ci)
                for (int co = 0; co < F; ++co) {
                    const double t = product(ws[((size_t)tap * F + ci) * F + co], xr[ci]);
                    ref1[(size_t)c * FP + co] += t;
                    mag1[(size_t)c * FP + co] += std::fabs(t);
                }
        }
    }
    const double e1 = compare(out1, ref1, mag1);
    std::printf("%s P=%d: H=%d W=%d rows=%d C=%d K0=%d F=%d (FP %d): max rel err initial %.3g trunk %.3g\n", n.name, P, H, W,
                n.rows, C, K0, F, FP, e0, e1);
    return e0 <= 1e-12 && e1 <= 1e-12 ? 0 : 1;
}

// the layered modes pack the fused modes' image
void same_image(const gz_net_desc& d, int fpad, unsigned seed) {
    const BlobPlan plan = blob_plan(d);
    std::mt19937 rng(seed);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<float> blob(plan.consumed);
    for (float& v : blob) v = 0.5f + std::fabs(nd(rng));
    const int pairs[2][2] = {{GZ_PRECISION_BF16, GZ_PRECISION_BF16_LAYERED}, {GZ_PRECISION_SPLIT, GZ_PRECISION_SPLIT_LAYERED}};
    for (const auto& pr : pairs) {
        const Packed a = pack(d, pr[0], fpad, blob), b = pack(d, pr[1], fpad, blob);
        CHECK(a.I.total == b.I.total && a.img == b.img);
        CHECK(a.s.p2 == b.s.p2 && !b.s.fp32 && b.s.p2 == (pr[0] == GZ_PRECISION_SPLIT ? 2 : 1));
        std::printf("image p2=%d: %zu bytes, layered == fused\n", a.s.p2, a.I.total);
    }
}

}  // namespace

int main() {
    int bad = 0;
    // (a) a legacy v1 net on a 5 x 4 board, 3 planes, F 40 -> 64, conv biases, 7 rows: 140 columns,
    //     a partial second tile
    Net a{"5x4_legacy", desc(3, 5, 4, 40, 1, 0, false), 7};
    a.d.conv_bias = a.d.value_bn = a.d.value_sigmoid = 1;
    // (b) 19 x 19, F = 256 at 2 rows: 722 columns, tile 2 straddles the two boards; v2's 1 x 1 initial conv
    Net b{"19x19_f256", desc(5, 19, 19, 256, 1, 0, true), 2};
    // (c) a 3 x 3 initial conv with 15 planes (K0 = 160: chunks of 64, 64, 32) on a non-square board
    Net c{"6x9_c15", desc(15, 6, 9, 64, 1, 0, false), 3};
    CHECK(pack_spec(c.d, GZ_PRECISION_BF16_LAYERED, 64, false).K0 == 160);
    CHECK(pack_spec(b.d, GZ_PRECISION_BF16_LAYERED, 256, false).K0 == 32);
    bad += run(a, 1, 1);
    bad += run(a, 3, 2);
    bad += run(b, 3, 3);
    bad += run(c, 1, 4);
    bad += run(c, 3, 5);
    same_image(a.d, 64, 6);
    // the LDS row strides: 16-byte slots, 2 (mod 8) of them, so that each ds_read_b128 lane group's 8
    // rows of k group g take the even and its 8 rows of g + 1 the odd slots of the 16
    for (int P : {1, 3}) {
        const int slots = lds_row_bytes(P) / 16;
        CHECK(lds_row_bytes(P) % 16 == 0 && slots % 8 == 2);
        for (int grp = 0; grp < 2; ++grp)       // lanes {0-3, 12-15 | 20-27} and {4-11 | 16-19, 28-31}
            for (int r0 = 0; r0 < 16; ++r0) {   // the tile's first LDS row
                bool used[16] = {false};
                for (int lane = 0; lane < 32; ++lane) {
                    const bool first = lane < 4 || (lane >= 12 && lane < 16) || (lane >= 20 && lane < 28);
                    if (first != (grp == 0)) continue;
                    const int slot = (bfrag_addr(r0 + (lane & 15), 1, lane >> 4, P == 3 ? 1 : 0, P) / 16) % 16;
                    CHECK(!used[slot]);
                    used[slot] = true;
                }
            }
    }
    if (bad) std::fprintf(stderr, "%d cases failed\n", bad);
    return bad ? 1 : 0;
}
