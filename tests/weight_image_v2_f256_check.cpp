// Stand-alone host check that the weight image (csrc/nn/weight_image.h) needs no layout change for
// v2 nets with up to 256 filters: (a) v2 on 8 x 8, F 192 -> 256, two blocks, 64 squeeze-excite
// units, the pooling value head with its BatchNorm; (b) v2 on 13 x 13, F = 256, two blocks, 85
// squeeze-excite units (filters / 3), concat_all_layers.  Each packed on the CPU as bf16, bf16x3
// and fp32 into heap buffers of exactly the image's size.  Asserts that the blob plan consumes the
// float count desc.py gives (argv: one count per case), that every write lands inside the image
// and no byte is written twice, that two runs agree, that every real conv weight is there and that
// the padded channels (192 .. 255) are zero in the convs, the bias / pre-activation / head-conv
// rows and both squeeze-excite matrices -- the zeros that keep them out of the SE means, the
// pooled features and the head convs.  Built with -fsanitize=address,undefined and run directly by
// tests/test_v2_f256.py; prints one line per (case, precision) and exits 0 when everything holds.
#include "../galvanise_zero_amd/csrc/nn/weight_image.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

using namespace gzw;

#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

namespace {

// an image that takes each byte once, inside its size
struct MarkImage {
    char* p;
    char* written;
    size_t total;
    void put(size_t off, const void* v, size_t n) const {
        CHECK(off + n <= total);
        for (size_t i = 0; i < n; ++i) CHECK(!written[off + i]);
        std::memset(written + off, 1, n);
        std::memcpy(p + off, v, n);
    }
    void put16(size_t off, uint16_t v) const { put(off, &v, 2); }
    void put32(size_t off, float v) const { put(off, &v, 4); }
};

struct Case {
    const char* name;
    gz_net_desc d;
};

gz_net_desc v2_desc(int C, int side, int F, int B, int P0, int P1, int S) {
    gz_net_desc d{};
    d.input_channels = C; d.input_columns = side; d.input_rows = side;
    d.cnn_filter_size = F; d.cnn_kernel_size = 3; d.residual_layers = B;
    d.role_count = 2; d.policy_dist_count[0] = P0; d.policy_dist_count[1] = P1;
    d.value_hidden_size = 6;   // not a multiple of 4
    d.num_values = 2;
    d.resnet_v2 = d.initial_bn = 1;
    d.se_units = S;
    return d;
}

void run(const Case& c, int p2, bool fp32, size_t count) {
    PackSpec s;
    s.d = c.d;
    s.fpad = 256;
    s.p2 = p2;
    s.K0 = (initial_kernel(c.d) * initial_kernel(c.d) * c.d.input_channels + 31) / 32 * 32;
    s.cp = gzfp32::pad16(c.d.input_channels);
    s.fp32 = fp32;
    s.gemm_heads = false;
    CHECK(gzfp32::padded_filters(c.d.cnn_filter_size) == s.fpad);
    const gz_net_desc& d = s.d;
    const int F = d.cnn_filter_size, FP = s.fpad, B = d.residual_layers, C = d.input_channels;
    const int T0 = initial_kernel(d) * initial_kernel(d);

    const BlobPlan P = blob_plan(d);
    CHECK(P.consumed == count);   // desc.py blob_size's
    // exact in fp32 and strictly positive (no variance below zero, no real weight folding to zero)
    std::unique_ptr<float[]> blob(new float[count]);
    for (size_t i = 0; i < count; ++i) blob[i] = 0.25f + (float)(i % 251) / 256.f;

    const ImageLayout I = image_layout(s);
    const JobList J = job_list(s, P, I);
    std::unique_ptr<char[]> a(new char[I.total]()), b(new char[I.total]()), written(new char[I.total]());
    pack_image_host(J, blob.get(), RawImage{a.get()});
    pack_image_host(J, blob.get(), MarkImage{b.get(), written.get(), I.total});
    CHECK(std::memcmp(a.get(), b.get(), I.total) == 0);

    const size_t wb = fp32 ? 4 : 2;
    auto zero = [&](size_t off, size_t n) {
        CHECK(off + n <= I.total);
        for (size_t i = 0; i < n; ++i)
            if (a[off + i]) return false;
        return true;
    };
    auto conv = [&](size_t base, int taps, int cin, int cinp, bool initial) {
        for (int tap = 0; tap < taps; ++tap)
            for (int ci = 0; ci < cinp; ++ci)
                for (int co = 0; co < FP; ++co) {
                    const int k = tap * cin + ci;   // the bf16 initial conv's k (cinp = cin there)
                    const size_t o = fp32 ? gzfp32::wfrag_index(tap, co, ci, cinp, FP)
                                          : initial ? ((size_t)(k / 32) * FP + co) * 32 + k % 32 : wres_index(tap, co, ci, FP, p2);
                    const bool real = ci < cin && co < F;
                    CHECK(zero(base + o * wb, wb) == !real);
                    if (!fp32 && p2 == 2 && !real) CHECK(zero((initial ? I.w0lo + o * 2 : base + (o + 512) * 2), 2));
                }
    };
    conv(I.w0, T0, C, fp32 ? s.cp : C, true);
    for (int c2 = 0; c2 < 2 * B; ++c2) conv(I.wres + c2 * I.conv_bytes, 9, F, FP, false);
    // rows of FP floats: channels from F on are zero
    auto rows = [&](size_t base, int n) {
        for (int r = 0; r < n; ++r) CHECK(zero(base + ((size_t)r * FP + F) * 4, (size_t)(FP - F) * 4));
    };
    rows(I.b0, 1);
    rows(I.bres, 2 * B);
    rows(I.wh, 2 * d.role_count + (d.concat_all_layers ? 0 : 1));
    rows(I.wcl, cal_layers(d));
    rows(I.pre, 2 * B);
    CHECK(d.se_units > 0);
    rows(I.sew2, B * d.se_units);
    for (int blk = 0; blk < B; ++blk)   // [FP][S]: input channels from F on
        CHECK(zero(I.sew1 + ((size_t)blk * FP + F) * d.se_units * 4, (size_t)(FP - F) * d.se_units * 4));
    // the pooled features stop at the model's F: the value hidden Dense has gapF + HW inputs
    CHECK(gap_features(d) == (d.global_pooling_value ? F : 0));
    size_t bytes = 0;
    for (size_t i = 0; i < I.total; ++i) bytes += written[i];
    std::printf("case %s %s: %zu floats, %zu folds + %zu jobs wrote %zu of %zu bytes\n", c.name,
                fp32 ? "fp32" : p2 == 2 ? "p2=2" : "p2=1", count, J.folds.size(), J.packs.size(), bytes, I.total);
}

}  // namespace

int main(int argc, char** argv) {
    Case cases[2];
    cases[0] = Case{"a", v2_desc(5, 8, 192, 2, 155, 155, 64)};
    cases[0].d.global_pooling_value = cases[0].d.value_bn = 1;
    cases[1] = Case{"b", v2_desc(5, 13, 256, 2, 170, 171, 85)};
    cases[1].d.concat_all_layers = 1;
    CHECK(argc == 3);
    for (int i = 0; i < 2; ++i)
        for (int mode = 0; mode < 3; ++mode) run(cases[i], mode == 1 ? 2 : 1, mode == 2, (size_t)std::atoll(argv[1 + i]));
    return 0;
}
