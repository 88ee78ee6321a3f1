// Stand-alone host check of the "fp16x3-layered" arithmetic (csrc/nn/layered_forward.h, weight_image.h):
// the conv of gzlayered::conv_f16_kernel restated on the CPU from the shared pieces alone -- the LDS row
// of a column and tap, the staged channel's offset, the B-fragment address, the A-fragment offsets into
// the trunk and initial-conv images, board_exponent, and the fp16 hi | scaled-lo image pack_image_host
// made -- in the kernel's arithmetic: rows scaled by 2^-e of their board, split by f2h / h_lo_of, a
// k-step's 32 products exact and summed into the fp32 accumulators main (hi hi) and corr (hi lo, then
// lo hi), out = (main + corr 2^-11) 2^e.  Checked against a float64 convolution of the unrounded fp32
// operands:
//   * error <= 4e-6 of the sum of |w x| per output (fp32-class), and, over the tensor, more than 10 x
//     closer than the same operands as bf16 hi + lo (bf16x3's arithmetic, summed in double);
//   * a board whose inputs reach 1e6 stays finite at the same bound; with every exponent forced to 0
//     the same conv is not finite;
//   * board_exponent at 0, the smallest subnormal, 65,504, 2^15 -+ 1 ulp and infinity;
//   * a row computed alone equals the row inside a two-board tile, bit for bit;
//   * f2h rounds to nearest even at every midpoint of fp16, and the image differs from bf16x3's only
//     in the conv parts' values (same layout).
// Every generated index is asserted in bounds.  Built with -fsanitize=address,undefined and run
// directly by tests/test_fp16x3_mode.py; exits 0 when everything holds.
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

constexpr int P = kF16Parts;
constexpr double kBound = 4e-6;

float bf(uint16_t h) { return __builtin_bit_cast(float, (uint32_t)h << 16); }
unsigned bits(float f) { return __builtin_bit_cast(unsigned, f); }

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

// bexp as board_exp_kernel writes it: one exponent per board of npos x cinp inputs
std::vector<int> board_exponents(const std::vector<float>& x, int ncols, int cinp, int npos, bool force0) {
    CHECK(ncols % npos == 0);
    std::vector<int> e(ncols / npos, 0);
    for (int b = 0; b < ncols / npos; ++b) {
        unsigned m = 0;
        for (size_t i = (size_t)b * npos * cinp; i < (size_t)(b + 1) * npos * cinp; ++i) m = std::max(m, bits(x[i]) & 0x7fffffffu);
        e[b] = force0 ? 0 : board_exponent(m);
    }
    return e;
}

// One conv as conv_f16_kernel runs it, workgroups / waves / lanes one after another.  x [ncols][cinp]
// fp32; img the fp16 image (whi / wlo: element offsets of this conv's hi and lo images); w0: the
// initial conv's layout (taps == 1).  out: before bias / skip / activation.
void conv_tiled(const std::vector<float>& x, int ncols, int cinp, int taps, int H, int W, int FP, const std::vector<uint16_t>& img,
                size_t whi, size_t wlo, bool w0, const std::vector<int>& bexp, std::vector<float>& out) {
    const int npos = H * W, NP = operand_parts(P);
    const int CT = gzfp32::wave_co_tiles(FP), TT = kWaveTiles, stride = lds_row_bytes(P);
    CHECK(NP == 2 && stride == 288 && FP % (32 * CT) == 0 && cinp % kStep == 0 && (taps == 1 || taps == 9));
    CHECK(lds_bytes(W, P) <= 64 * 1024 && (int)bexp.size() == ncols / npos);
    const int gx = (ncols + kTileCols - 1) / kTileCols, gy = FP / (32 * CT);
    const uint16_t poison = 0x7e01;   // an fp16 NaN: only staged data may be read
    for (int bx = 0; bx < gx; ++bx)
        for (int by = 0; by < gy; ++by) {
            std::vector<uint16_t> lds(lds_bytes(W, P) / 2, poison);
            const long c0 = (long)bx * kTileCols;
            for (int i = 0; i < stride / 2; ++i) lds[(size_t)lds_zero_row(W) * (stride / 2) + i] = 0;
            std::vector<float> acc((size_t)4 * CT * TT * 256, 0.f), cor(acc.size(), 0.f);   // [wave][ct][t][16][16]
            for (int kc = 0; kc < cinp; kc += kChunk) {
                const int kcl = cinp - kc < kChunk ? cinp - kc : kChunk, nrows = lds_zero_row(W);
                CHECK(kcl % kStep == 0);
                for (int r = 0; r < nrows; ++r) {
                    const long f = lds_row_column(c0, W, r);
                    const bool in = f >= 0 && f < ncols;
                    int eb = 0;
                    if (in) {
                        CHECK((size_t)(f / npos) < bexp.size());
                        eb = bexp[f / npos];
                    }
                    for (int cc = 0; cc < kcl; ++cc) {
                        float v = 0.f;
                        if (in) {
                            const size_t xo = (size_t)f * cinp + kc + cc;
                            CHECK(xo < x.size());
                            v = std::ldexp(x[xo], -eb);
                        }
                        for (int part = 0; part < NP; ++part) {
                            const size_t o = (size_t)r * stride + lds_channel_offset(cc, part);
                            CHECK(o % 2 == 0 && o + 1 < (size_t)lds_zero_row(W) * stride);   // never the zero row
                            CHECK(lds_channel_offset(cc, part) + 1 < stride);
                            lds[o / 2] = part ? h_lo_of(v) : f2h(v);
                        }
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
                                        for (int e = 0; e < 8; ++e) A[(((size_t)part * CT + ct) * 64 + lane) * 8 + e] = h2f(img[wo + e]);
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
                                            B[(((size_t)part * TT + t) * 64 + lane) * 8 + e] = h2f(h);
                                        }
                                    }
                                }
                            // v_mfma_f32_16x16x32_f16: lane l holds A[l % 16][8 (l / 16) ..] and B[8 (l / 16) ..][l % 16];
                            // the k-step's products in the kernel's order: main hi hi, corr hi lo, corr lo hi
                            const int prod[3][2] = {{0, 0}, {0, 1}, {1, 0}};
                            for (int pr = 0; pr < 3; ++pr)
                                for (int ct = 0; ct < CT; ++ct)
                                    for (int t = 0; t < TT; ++t) {
                                        const float* a = &A[((size_t)prod[pr][0] * CT + ct) * 512];
                                        const float* b = &B[((size_t)prod[pr][1] * TT + t) * 512];
                                        float* d = &(pr ? cor : acc)[((size_t)(wave * CT + ct) * TT + t) * 256];
                                        for (int i = 0; i < 16; ++i)
                                            for (int j = 0; j < 16; ++j) {
                                                double s = 0.0;
                                                for (int k = 0; k < 32; ++k)
                                                    s += (double)a[(i + 16 * (k >> 3)) * 8 + (k & 7)] * b[(j + 16 * (k >> 3)) * 8 + (k & 7)];
                                                d[i * 16 + j] = (float)((double)d[i * 16 + j] + s);
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
                                const size_t o = (size_t)c * FP + co, ai = ((size_t)(wave * CT + ct) * TT + t) * 256 + (4 * g + r) * 16 + li;
                                CHECK(o < out.size());
                                CHECK(bits(out[o]) == 0x7fc00001u);   // every output written exactly once
                                out[o] = std::ldexp((float)((double)acc[ai] + (double)cor[ai] * kF16LoInv), bexp[c / npos]);
                            }
                        }
            }
        }
}

// bf16x3's operand: bf16 hi + lo; the three products summed in double
struct Split {
    double hi, lo;
};
Split split(float v) { return Split{bf(f2bf(v)), bf(lo_of(v))}; }
double product(const Split& w, const Split& x) { return w.hi * x.hi + w.hi * x.lo + w.lo * x.hi; }

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

struct Errors {
    double pointwise = 0.0;   // max |got - ref| / sum |w x|
    double f16 = 0.0, bf16 = 0.0;   // max |. - ref| / max |ref| over the tensor
    bool finite = true;
};
std::vector<float> fresh(size_t n) { return std::vector<float>(n, __builtin_bit_cast(float, 0x7fc00001u)); }

struct Case {
    const char* name;
    gz_net_desc d;
    int rows;
};

struct Model {
    gz_net_desc d;
    int H, W, npos, F, FP, C, T0, K0;
    BlobPlan plan;
    std::vector<float> blob, fold;
    Packed k;
    std::vector<uint16_t> img;
};
Model make_model(const gz_net_desc& d, unsigned seed) {
    Model m;
    m.d = d;
    m.H = d.input_columns; m.W = d.input_rows; m.npos = m.H * m.W;
    m.F = d.cnn_filter_size; m.C = d.input_channels; m.FP = gzfp32::padded_filters(m.F);
    m.T0 = initial_kernel(d) * initial_kernel(d);
    m.plan = blob_plan(d);
    std::mt19937 rng(seed);
    std::normal_distribution<float> nd(0.f, 1.f);
    m.blob.resize(m.plan.consumed);
    for (float& v : m.blob) v = nd(rng);
    for (const BNRef& b : m.plan.folds)
        if (b.g != kNone)
            for (int i = 0; i < b.n; ++i) m.blob[b.var + i] = 0.5f + std::fabs(m.blob[b.var + i]);
    m.fold.resize((size_t)m.plan.fold_floats);
    for (const BNRef& b : m.plan.folds)
        for (int i = 0; i < b.n; ++i) fold_element(b, i, m.blob.data(), m.fold.data());
    m.k = pack(d, GZ_PRECISION_F16X3_LAYERED, m.FP, m.blob);
    CHECK(m.k.s.p2 == 2 && m.k.s.f16 && !m.k.s.fp32 && m.k.I.total % 2 == 0);
    m.K0 = m.k.s.K0;
    m.img.resize(m.k.I.total / 2);
    std::memcpy(m.img.data(), m.k.img.data(), m.k.I.total);
    CHECK(f16_range_check(job_list(m.k.s, m.plan, m.k.I), m.blob.data()) == -1);
    return m;
}

// the first trunk conv over x [ncols][FP] (padded channels too: their weights are zero)
std::vector<float> trunk_conv(const Model& m, const std::vector<float>& x, int ncols, bool force0) {
    std::vector<float> out = fresh((size_t)ncols * m.FP);
    CHECK(m.d.residual_layers >= 1 && m.k.I.wres % 2 == 0);
    conv_tiled(x, ncols, m.FP, 9, m.H, m.W, m.FP, m.img, m.k.I.wres / 2, 0, false, board_exponents(x, ncols, m.FP, m.npos, force0), out);
    return out;
}
Errors trunk_errors(const Model& m, const std::vector<float>& x, int ncols, const std::vector<float>& got) {
    const int F = m.F, FP = m.FP, W = m.W, H = m.H;
    std::vector<float> w((size_t)9 * F * F);
    for (size_t i = 0; i < w.size(); ++i) w[i] = f_mul(m.blob[m.plan.wconv[0] + i], m.fold[m.plan.bnconv[0].scale() + i % F]);
    std::vector<Split> ws(w.size()), xs(x.size());
    for (size_t i = 0; i < w.size(); ++i) ws[i] = split(w[i]);
    for (size_t i = 0; i < x.size(); ++i) xs[i] = split(x[i]);
    Errors e;
    double maxref = 0.0, ef = 0.0, eb = 0.0;
    std::vector<double> ref(F), mag(F), b16(F);
    for (int c = 0; c < ncols; ++c) {
        const int p = c % m.npos, y = p / W, xx = p % W;
        std::fill(ref.begin(), ref.end(), 0.0);
        std::fill(mag.begin(), mag.end(), 0.0);
        std::fill(b16.begin(), b16.end(), 0.0);
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
            if (y + dy < 0 || y + dy >= H || xx + dx < 0 || xx + dx >= W) continue;
            const size_t xo = (size_t)(c + dy * W + dx) * FP;
            for (int ci = 0; ci < F; ++ci)
                for (int co = 0; co < F; ++co) {
                    const size_t wi = ((size_t)tap * F + ci) * F + co;
                    const double t = (double)w[wi] * x[xo + ci];
                    ref[co] += t;
                    mag[co] += std::fabs(t);
                    b16[co] += product(ws[wi], xs[xo + ci]);
                }
        }
        for (int co = 0; co < FP; ++co) {
            const float g = got[(size_t)c * FP + co];
            if (!std::isfinite(g)) { e.finite = false; continue; }
            if (co >= F) { CHECK(g == 0.f); continue; }
            e.pointwise = std::max(e.pointwise, std::fabs(g - ref[co]) / (mag[co] + 1e-300));
            maxref = std::max(maxref, std::fabs(ref[co]));
            ef = std::max(ef, std::fabs(g - ref[co]));
            eb = std::max(eb, std::fabs(b16[co] - ref[co]));
        }
    }
    e.f16 = ef / maxref;
    e.bf16 = eb / maxref;
    return e;
}

// the initial conv: planes -> im2col image -> 1-tap conv over the w0 images
Errors initial_conv(const Model& m, int rows, std::mt19937& rng) {
    const int H = m.H, W = m.W, npos = m.npos, C = m.C, K0 = m.K0, F = m.F, FP = m.FP, T0 = m.T0, ncols = rows * npos;
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<float> planes((size_t)rows * C * npos);
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
    std::vector<float> out = fresh((size_t)ncols * FP);
    CHECK(m.k.I.w0 % 2 == 0 && m.k.I.w0lo % 2 == 0);
    conv_tiled(col, ncols, K0, 1, H, W, FP, m.img, m.k.I.w0 / 2, m.k.I.w0lo / 2, true, board_exponents(col, ncols, K0, npos, false), out);
    Errors e;
    double maxref = 0.0, ef = 0.0, eb = 0.0;
    for (int c = 0; c < ncols; ++c) {
        const int row = c / npos, p = c % npos, y = p / W, x = p % W;
        std::vector<double> ref(F, 0.0), mag(F, 0.0), b16(F, 0.0);
        for (int tp = 0; tp < T0; ++tp) {
            const int tap = T0 == 1 ? 4 : tp, yy = y + tap / 3 - 1, xn = x + tap % 3 - 1;
            if (yy < 0 || yy >= H || xn < 0 || xn >= W) continue;
            for (int ci = 0; ci < C; ++ci) {
                const float xv = planes[((size_t)row * C + ci) * npos + yy * W + xn];
                for (int co = 0; co < F; ++co) {
                    const float w = f_mul(m.blob[m.plan.w0 + ((size_t)tp * C + ci) * F + co], m.fold[m.plan.bn0.scale() + co]);
                    const double t = (double)w * xv;
                    ref[co] += t;
                    mag[co] += std::fabs(t);
                    b16[co] += product(split(w), split(xv));
                }
            }
        }
        for (int co = 0; co < F; ++co) {
            const float g = out[(size_t)c * FP + co];
            CHECK(std::isfinite(g));
            e.pointwise = std::max(e.pointwise, std::fabs(g - ref[co]) / (mag[co] + 1e-300));
            maxref = std::max(maxref, std::fabs(ref[co]));
            ef = std::max(ef, std::fabs(g - ref[co]));
            eb = std::max(eb, std::fabs(b16[co] - ref[co]));
        }
    }
    e.f16 = ef / maxref;
    e.bf16 = eb / maxref;
    return e;
}

int report(const char* name, const char* what, const Errors& e) {
    const bool ok = e.finite && e.pointwise <= kBound && e.f16 <= kBound && e.bf16 > 10 * e.f16;
    std::printf("%s %s: pointwise %.3g tensor fp16x3 %.3g bf16x3 %.3g (ratio %.1f)%s\n", name, what, e.pointwise, e.f16, e.bf16,
                e.bf16 / e.f16, ok ? "" : "  FAILED");
    return ok ? 0 : 1;
}

int run(const Case& n, unsigned seed, bool with_trunk) {
    const Model m = make_model(n.d, seed);
    std::mt19937 rng(seed + 100);
    std::normal_distribution<float> nd(0.f, 1.f);
    int bad = 0;
    std::printf("%s: H=%d W=%d rows=%d C=%d K0=%d F=%d (FP %d)\n", n.name, m.H, m.W, n.rows, m.C, m.K0, m.F, m.FP);
    bad += report(n.name, "initial", initial_conv(m, n.rows, rng));
    if (with_trunk) {
        const int ncols = n.rows * m.npos;
        std::vector<float> x((size_t)ncols * m.FP);
        for (float& v : x) v = nd(rng);
        bad += report(n.name, "trunk", trunk_errors(m, x, ncols, trunk_conv(m, x, ncols, false)));
    }
    return bad;
}

// fp16's range: a board whose inputs reach 1e6; the same conv without the exponents
int range_case(const gz_net_desc& d, unsigned seed) {
    const Model m = make_model(d, seed);
    std::mt19937 rng(seed + 7);
    std::normal_distribution<float> nd(0.f, 1.f);
    const int rows = 2, ncols = rows * m.npos;
    std::vector<float> x((size_t)ncols * m.FP);
    float big = 0.f;
    for (float& v : x) v = nd(rng);
    for (size_t i = 0; i < (size_t)m.npos * m.FP; ++i) big = std::max(big, std::fabs(x[i]));
    for (size_t i = 0; i < (size_t)m.npos * m.FP; ++i) x[i] *= 1e6f / big;   // board 0 reaches 1e6, board 1 stays O(1)
    const std::vector<int> be = board_exponents(x, ncols, m.FP, m.npos, false);
    CHECK(be[0] == 19 - 14 && be[1] <= 2 - 14 + 1);
    const Errors e = trunk_errors(m, x, ncols, trunk_conv(m, x, ncols, false));
    const Errors e0 = trunk_errors(m, x, ncols, trunk_conv(m, x, ncols, true));
    const bool ok = e.finite && e.pointwise <= kBound && !e0.finite;
    std::printf("range: inputs to 1e6 (exponents %d, %d): pointwise %.3g finite %d; exponents forced to 0: finite %d%s\n", be[0], be[1],
                e.pointwise, (int)e.finite, (int)e0.finite, ok ? "" : "  FAILED");
    return ok ? 0 : 1;
}

// a row alone equals the row inside a two-board tile
int invariance_case(const gz_net_desc& d, unsigned seed) {
    const Model m = make_model(d, seed);
    std::mt19937 rng(seed + 9);
    std::normal_distribution<float> nd(0.f, 1.f);
    const int ncols = 2 * m.npos;
    CHECK(ncols <= kTileCols);
    std::vector<float> x((size_t)ncols * m.FP);
    for (float& v : x) v = nd(rng);
    for (size_t i = 0; i < (size_t)m.npos * m.FP; ++i) x[i] *= 3000.f;   // the neighbour's exponent differs
    const std::vector<float> both = trunk_conv(m, x, ncols, false);
    const std::vector<float> second(x.begin() + (size_t)m.npos * m.FP, x.end());
    const std::vector<float> alone = trunk_conv(m, second, m.npos, false);
    const bool ok = std::memcmp(alone.data(), both.data() + (size_t)m.npos * m.FP, alone.size() * 4) == 0;
    std::printf("row invariance: a row alone == the row in a two-board tile: %s\n", ok ? "identical" : "FAILED");
    return ok ? 0 : 1;
}

void exponent_checks() {
    const float inf = std::numeric_limits<float>::infinity();
    CHECK(board_exponent(0u) == 0);
    CHECK(board_exponent(1u) == -149 - 14);                       // the smallest subnormal, 2^-149
    CHECK(board_exponent(0x007fffffu) == -127 - 14);              // the largest subnormal
    CHECK(board_exponent(0x00800000u) == -126 - 14);
    CHECK(board_exponent(bits(1.f)) == -14);
    CHECK(board_exponent(bits(65504.f)) == 1);
    CHECK(board_exponent(bits(32768.f)) == 1);
    CHECK(board_exponent(bits(std::nextafter(32768.f, 0.f))) == 0);
    CHECK(board_exponent(bits(std::nextafter(32768.f, inf))) == 1);
    CHECK(board_exponent(bits(std::numeric_limits<float>::max())) == 127 - 14);
    CHECK(board_exponent(bits(inf)) == 0);
    CHECK(board_exponent(bits(std::numeric_limits<float>::quiet_NaN()) & 0x7fffffffu) == 0);
    // the board's largest scaled value lies in [2^14, 2^15): finite in fp16 with its lo part
    for (float v : {1e-45f, 1e-40f, 1e-38f, 3e-5f, 1.f, 65504.f, 65520.f, 1e6f, 3e38f}) {
        const float s = std::ldexp(v, -board_exponent(bits(v)));
        CHECK(s >= 16384.f && s < 32768.f);
        CHECK((f2h(s) & 0x7fffu) < 0x7c00u && (h_lo_of(s) & 0x7fffu) < 0x7c00u);
    }
    std::printf("board_exponent: 0, subnormals, 65504, 2^15 -+ 1 ulp, inf\n");
}

// f2h against fp16's own grid: every value maps to itself, every midpoint to the even neighbour
void f2h_checks() {
    const float inf = std::numeric_limits<float>::infinity();
    for (unsigned h = 0; h < 0x7c00u; ++h) {
        const float a = h2f((uint16_t)h);
        CHECK(f2h(a) == h && f2h(-a) == (h | 0x8000u));
        const float b = h + 1 < 0x7c00u ? h2f((uint16_t)(h + 1)) : 65536.f;   // (past the largest: 2^16 rounds to infinity)
        const float mid = 0.5f * a + 0.5f * b;                                 // exact in fp32
        const unsigned even = (h & 1u) ? h + 1 : h;
        CHECK(f2h(mid) == even);
        CHECK(f2h(std::nextafter(mid, 0.f)) == h && f2h(std::nextafter(mid, inf)) == h + 1);
    }
    CHECK(f2h(inf) == 0x7c00u && f2h(-inf) == 0xfc00u && (f2h(std::nanf("")) & 0x7fffu) > 0x7c00u);
    CHECK(f2h(65504.f) == 0x7bffu && f2h(65519.996f) == 0x7bffu && f2h(65520.f) == 0x7c00u && f2h(1e9f) == 0x7c00u);
    CHECK(h2f(0x7c00u) == inf && std::isnan(h2f(0x7e00u)) && h2f(0x0001u) == std::ldexp(1.f, -24));
    // hi + lo 2^-11 carries 22 bits: the split of a float loses at most 2^-23 relative
    std::mt19937 rng(11);
    std::normal_distribution<float> nd(0.f, 1.f);
    for (int i = 0; i < 100000; ++i) {
        const float v = nd(rng) * std::ldexp(1.f, (int)(rng() % 20) - 10);
        if (std::fabs(v) < std::ldexp(1.f, -12)) continue;   // (hi within fp16's normals)
        const double back = (double)h2f(f2h(v)) + (double)h2f(h_lo_of(v)) / 2048.0;
        CHECK(std::fabs(back - v) <= std::ldexp(std::fabs((double)v), -22));
    }
    std::printf("f2h: nearest even on all of fp16's midpoints; hi + lo keeps 22 bits\n");
}

// the image: the split image's layout, other values in the conv parts only; an out-of-range weight is found
void image_checks(const gz_net_desc& d, unsigned seed) {
    Model m = make_model(d, seed);
    const Packed s = pack(d, GZ_PRECISION_SPLIT_LAYERED, m.FP, m.blob);
    CHECK(s.I.total == m.k.I.total && s.I.w0 == m.k.I.w0 && s.I.w0lo == m.k.I.w0lo && s.I.wres == m.k.I.wres && s.I.b0 == m.k.I.b0);
    CHECK(s.img != m.k.img);
    CHECK(std::memcmp(s.img.data() + s.I.bres, m.k.img.data() + s.I.bres, s.I.total - s.I.bres) == 0);
    std::printf("image: bf16x3's layout, %zu bytes, conv parts differ\n", s.I.total);
    const JobList J = job_list(m.k.s, m.plan, m.k.I);
    std::vector<float> blob = m.blob;
    blob[m.plan.wconv[1] + 5] = 3e38f;
    CHECK(f16_range_check(J, blob.data()) == 2);
    blob = m.blob;
    blob[m.plan.w0 + 1] = -3e38f;
    CHECK(f16_range_check(J, blob.data()) == 0);
    std::printf("range check: names the conv of a weight fp16 cannot hold\n");
}

}  // namespace

int main() {
    int bad = 0;
    exponent_checks();
    f2h_checks();
    // (a) a legacy v1 net on a 5 x 4 board, 3 planes, F 40 -> 64, conv biases, 7 rows: 140 columns, a
    //     partial second tile
    Case a{"5x4_legacy", desc(3, 5, 4, 40, 1, 0, false), 7};
    a.d.conv_bias = a.d.value_bn = a.d.value_sigmoid = 1;
    // (b) 19 x 19, F = 256 at 2 rows: 722 columns, tile 2 straddles the two boards
    Case b{"19x19_f256", desc(5, 19, 19, 256, 1, 0, true), 2};
    // (c) a 3 x 3 initial conv with 15 planes (K0 = 160: chunks of 64, 64, 32) on a non-square board
    Case c{"6x9_c15", desc(15, 6, 9, 64, 1, 0, false), 3};
    CHECK(pack_spec(c.d, GZ_PRECISION_F16X3_LAYERED, 64, false).K0 == 160);
    bad += run(a, 1, true);
    bad += run(b, 3, true);
    bad += run(c, 5, false);
    bad += range_case(a.d, 21);
    bad += invariance_case(a.d, 22);
    image_checks(desc(3, 5, 4, 40, 1, 0, false), 6);
    if (bad) std::fprintf(stderr, "%d cases failed\n", bad);
    return bad ? 1 : 0;
}
