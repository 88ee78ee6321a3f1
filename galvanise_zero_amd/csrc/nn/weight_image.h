// The device weight image: what the canonical Keras-order float32 blob (galvanise_zero_amd/nn/desc.py
// weight_spec) turns into -- inference BatchNorm (eps 1e-3, model.py:21-22) folded into the
// preceding conv, conv kernels in MFMA fragment order (bf16 hi / lo, or fp32 for fp32-ieee), padded
// dense layers -- described once, for whoever executes it:
//   blob_plan     the one walk of the blob's tensor order, as float offsets from its start;
//   image_layout  byte offsets of every packed tensor in the image (one allocation);
//   job_list      every BN fold and every pack / copy as offsets into blob, fold buffer and image:
//                 the only place that knows which tensor lands where;
//   fold_element / pack_element   one output of a job, __host__ __device__;
//   pack_image_host               the job list run on the CPU (gz_net_set_weights);
// gz_nn.hip's kernels run the same jobs over the same element functions on a device blob
// (gz_net_set_weights_device), so the two images are byte-identical (tests/test_weight_roll_gpu.py).
// Plain C++: usable without a HIP compiler (tests/weight_image_host_check.cpp).
#pragma once

#include "fp32_forward.h"
#include "../../../include/gzero_nn.h"

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GZW_HD __host__ __device__
#else
#define GZW_HD
#endif

namespace gzw {

// everything the packing depends on (gz_net_create fills it in)
struct PackSpec {
    gz_net_desc d{};
    int fpad = 0;              // filters rounded up to the compiled 64 / 128 / 256 (zero channels)
    int p2 = 1;                // bf16 parts per operand: 1 (bf16) or 2 (split precision)
    int K0 = 0;                // initial conv's k = taps x planes, padded to 32
    int cp = 0;                // input planes padded to 16 (fp32-ieee)
    bool fp32 = false;         // GZ_PRECISION_FP32: fp32 conv images (fp32_forward.h) instead of the bf16 ones
    bool gemm_heads = false;   // policy heads by policy_gemm_kernel: its A fragments follow the image
    bool f16 = false;          // GZ_PRECISION_F16X3_LAYERED: the conv images' parts are fp16 hi | fp16 lo scaled by 2^11
};

inline int initial_kernel(const gz_net_desc& d) {
    return d.initial_kernel ? d.initial_kernel : (d.resnet_v2 ? 1 : d.cnn_kernel_size);
}
// The spec of desc d in arithmetic mode `precision` (gz_net_desc.precision, not 0) with fpad padded
// filters.  The layered modes pack the image of the fused mode with the same operand parts: the two
// specs are equal, so are the images.  "fp16x3-layered" packs the split image's layout (p2 = 2) with
// fp16 parts (f2h / h_lo_of in place of f2bf / lo_of).
inline PackSpec pack_spec(const gz_net_desc& d, int precision, int fpad, bool gemm_heads) {
    PackSpec s;
    s.d = d;
    s.fpad = fpad;
    s.f16 = precision == GZ_PRECISION_F16X3_LAYERED;
    s.p2 = (precision == GZ_PRECISION_SPLIT || precision == GZ_PRECISION_SPLIT_LAYERED || s.f16) ? 2 : 1;
    s.K0 = ((initial_kernel(d) * initial_kernel(d) * d.input_channels + 31) / 32) * 32;
    s.cp = (d.input_channels + 15) & ~15;
    s.fp32 = precision == GZ_PRECISION_FP32;
    s.gemm_heads = gemm_heads;
    return s;
}
inline bool has_initial_bn(const gz_net_desc& d) { return !d.resnet_v2 || d.initial_bn; }
inline int gap_features(const gz_net_desc& d) { return d.global_pooling_value ? d.cnn_filter_size : 0; }
// trunk layers the concat_all_layers value head reads (model.py:251-260), 0 for the other heads
inline int cal_layers(const gz_net_desc& d) { return d.concat_all_layers ? d.residual_layers + 1 : 0; }
// value hidden Dense inputs
inline int value_features(const gz_net_desc& d) {
    const int HW = d.input_columns * d.input_rows;
    return d.concat_all_layers ? cal_layers(d) * HW : gap_features(d) + HW;
}

// ---- the blob ----------------------------------------------------------------------------------
constexpr size_t kNone = ~(size_t)0;   // no such tensor

// A BatchNorm over n channels after a conv with optional bias cb (float offsets in the blob), and
// where its fold goes: scale[n] | bias[n] at `out` in the fold buffer.  g == kNone: no BN (scale 1,
// bias cb or 0).
struct BNRef {
    size_t g = kNone, be = kNone, mu = kNone, var = kNone, cb = kNone;
    int n = 0, out = 0;
    size_t scale() const { return (size_t)out; }
    size_t bias() const { return (size_t)out + n; }
};

// float offsets of the blob's tensors
struct BlobPlan {
    size_t w0 = 0;
    BNRef bn0;
    std::vector<size_t> wconv;      // [2B] 3x3 conv kernels
    std::vector<BNRef> bnconv;      // [2B] the BN folded into each
    std::vector<BNRef> pre;         // v2: [B] the block's first BN (scale / shift of the stream)
    std::vector<size_t> se_c, se_g;
    size_t hw[GZ_MAX_ROLES] = {};
    BNRef hbn[GZ_MAX_ROLES];
    size_t pd[GZ_MAX_ROLES] = {}, pb[GZ_MAX_ROLES] = {};
    std::vector<size_t> clw;
    std::vector<BNRef> clbn;
    size_t vw = 0;
    BNRef vbn;
    size_t vhw = 0, vhb = 0, vdw = 0, vdb = 0;
    std::vector<BNRef> folds;       // every BNRef above
    size_t consumed = 0;            // the blob's float count
    int fold_floats = 0;
};

// The tensors of the canonical blob, in desc.py weight_spec's order.
inline BlobPlan blob_plan(const gz_net_desc& d) {
    BlobPlan P;
    struct Cursor {
        size_t p = 0;
        size_t take(size_t n) { const size_t r = p; p += n; return r; }
    } cur;
    const int F = d.cnn_filter_size, C = d.input_channels, B = d.residual_layers, R = d.role_count, S = d.se_units;
    const int HW = d.input_columns * d.input_rows, k0 = initial_kernel(d), NL = cal_layers(d);
    // a conv's optional bias (legacy model files), then its BN (with_bn) or none
    auto bias_bn = [&](int n, bool with_conv_bias, bool with_bn) {
        BNRef b;
        if (with_conv_bias && d.conv_bias) b.cb = cur.take(n);
        if (with_bn) { b.g = cur.take(n); b.be = cur.take(n); b.mu = cur.take(n); b.var = cur.take(n); }
        b.n = n;
        b.out = P.fold_floats;
        P.fold_floats += 2 * n;
        P.folds.push_back(b);
        return b;
    };
    P.w0 = cur.take((size_t)k0 * k0 * C * F);
    P.bn0 = bias_bn(F, true, has_initial_bn(d));   // v2 files with a bare initial conv: no BN, no activation
    for (int blk = 0; blk < B; ++blk) {
        if (!d.resnet_v2) {      // conv-BN-act-conv-BN-add-act: both BNs fold into their convs
            for (int j = 0; j < 2; ++j) {
                P.wconv.push_back(cur.take((size_t)9 * F * F));
                P.bnconv.push_back(bias_bn(F, true, true));
            }
            continue;
        }
        // v2: BN_1 (scale / shift applied to the stream when the block's input image is written),
        // conv1 with BN_2 folded, conv2 (no BN), squeeze-excite dense layers
        P.pre.push_back(bias_bn(F, false, true));
        P.wconv.push_back(cur.take((size_t)9 * F * F));
        P.bnconv.push_back(bias_bn(F, true, true));
        P.wconv.push_back(cur.take((size_t)9 * F * F));
        P.bnconv.push_back(bias_bn(F, true, false));
        if (S) {
            P.se_c.push_back(cur.take((size_t)F * S));   // Dense [F][S]
            P.se_g.push_back(cur.take((size_t)S * F));   // Dense [S][F]
        }
    }
    for (int r = 0; r < R; ++r) {
        P.hw[r] = cur.take((size_t)F * 2);               // [1][1][F][2]
        P.hbn[r] = bias_bn(2, true, true);
        P.pd[r] = cur.take((size_t)2 * HW * d.policy_dist_count[r]);
        P.pb[r] = cur.take(d.policy_dist_count[r]);
    }
    for (int j = 0; j < NL; ++j) {   // concat_all_layers: conv2d_block(1, 1) per trunk layer
        P.clw.push_back(cur.take(F));
        P.clbn.push_back(bias_bn(1, true, true));
    }
    if (NL == 0) {
        P.vw = cur.take(F);          // [1][1][F][1], no BN, no bias (model.py:275-279)
        P.vbn = bias_bn(1, true, d.value_bn != 0);   // legacy files: bias, then BN (value_bn)
    }
    P.vhw = cur.take((size_t)value_features(d) * d.value_hidden_size);   // [GAP F] + HW, or (B + 1) HW inputs
    P.vhb = cur.take(d.value_hidden_size);
    P.vdw = cur.take((size_t)d.value_hidden_size * d.num_values);
    P.vdb = cur.take(d.num_values);
    P.consumed = cur.p;
    return P;
}

// ---- the image ---------------------------------------------------------------------------------
// byte offsets of every packed tensor (each 256-byte aligned)
struct ImageLayout {
    size_t w0, w0lo, b0, wres, bres, wh, bh, wcl, bcl, pd[GZ_MAX_ROLES], pb[GZ_MAX_ROLES], vhw, vhb, pre, sew1, sew2, vdw,
        vdb, pdp[GZ_MAX_ROLES] = {}, total;
    size_t conv_bytes;   // one trunk conv's image within wres
};

inline ImageLayout image_layout(const PackSpec& s) {
    const gz_net_desc& d = s.d;
    const size_t FP = s.fpad, B = d.residual_layers, P2 = s.p2, S = d.se_units, HW = (size_t)d.input_columns * d.input_rows;
    const size_t HC = 2 * d.role_count + 1, NL = std::max(cal_layers(d), 1), VH = d.value_hidden_size;
    const int k0 = initial_kernel(d);
    // (fp32-ieee: fp32 conv images in fp32_forward.h's wfrag_index order in place of the bf16 ones)
    const size_t wb = s.fp32 ? 4 : 2;
    const size_t n_w0 = s.fp32 ? gzfp32::conv_image_floats(k0 * k0, s.cp, s.fpad) : s.K0 * FP;
    ImageLayout I;
    size_t off = 0;
    auto alloc = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    I.conv_bytes = P2 * 9 * FP * FP * wb;
    I.w0 = alloc(n_w0 * wb);
    I.w0lo = alloc((P2 == 2 ? n_w0 : 1) * 2);
    I.b0 = alloc(FP * 4);
    I.wres = alloc(2 * B * I.conv_bytes);
    I.bres = alloc(2 * B * FP * 4);
    I.wh = alloc(HC * FP * 4);
    I.bh = alloc(HC * 4);
    I.wcl = alloc(NL * FP * 4);
    I.bcl = alloc(NL * 4);
    for (int r = 0; r < d.role_count; ++r) {
        I.pd[r] = alloc(2 * HW * ((d.policy_dist_count[r] + 3) & ~3) * 4);
        I.pb[r] = alloc((size_t)d.policy_dist_count[r] * 4);
    }
    I.vhw = alloc((size_t)value_features(d) * ((VH + 3) & ~(size_t)3) * 4);
    I.vhb = alloc(VH * 4);
    I.pre = alloc((d.resnet_v2 ? 2 * B * FP : 1) * 4);
    I.sew1 = alloc((S ? B * FP * S : 1) * 4);
    I.sew2 = alloc((S ? B * S * FP : 1) * 4);
    I.vdw = alloc(VH * d.num_values * 4);
    I.vdb = alloc((size_t)d.num_values * 4);
    if (s.gemm_heads)   // [P / 16][2 HW / 32][hi | lo][64][8] bf16
        for (int r = 0; r < d.role_count; ++r)
            I.pdp[r] = alloc((size_t)((d.policy_dist_count[r] + 15) / 16) * ((2 * HW + 31) / 32) * 2 * 64 * 8 * 2);
    I.total = off;
    return I;
}

// ---- the jobs ----------------------------------------------------------------------------------
// A job makes rows x cols elements (r, c).  src / sc / bi: float offsets in the blob (kFoldVec's src:
// in the fold buffer) and of a fold's scale / bias in the fold buffer; dst*: byte offsets in the image.
enum JobKind {
    kPackW0,      // bf16 initial conv [r = tap C + ci][c = co] * scale[co] -> [K0 / 32][FP][32] hi (dst), lo (dst_lo)
    kPackTrunk,   // bf16 trunk conv [r = tap F + ci][c = co] * scale[co] -> wres_index order, hi (+ lo: P2 == 2)
    kPackF32,     // fp32-ieee conv [r = tap cin + ci][c = co] * scale[co] -> fp32_forward.h wfrag_index order
                  // (the three convs: row 0 also writes the folded bias[co] to dst_bias)
    kScaleVec,    // dst[c ds] = blob[src + c ss] * fold[sc]      (heads' 1x1 convs, per-layer value convs)
    kFoldVec,     // dst[c] = fold[src + c]                       (their biases, v2 pre-BN rows)
    kRowCopy,     // dst[r ds + c] = blob[src + r ss + c]         (dense / squeeze-excite layers, rows padded to ds)
    kGemmFrag,    // policy_gemm_kernel's A fragments of the Dense [cin = K][F = P] at src: W^T tiles
                  // [jt][kt][hi | lo][64 lanes][8 k] bf16, r = jt nkt + kt, c = 8 lane + e, lane l holding
                  // row j = 16 jt + l % 16 and k = 32 kt + 8 (l / 16) + e (zero padded)
};
struct Job {
    int kind = 0, rows = 1, cols = 0;
    int F = 0, FP = 0, cin = 0, cinp = 0, P2 = 1;   // convs: model / padded output and input channels
    int f16 = 0;                                    // convs: fp16 hi | scaled lo parts instead of bf16 ones
    int ss = 1, ds = 1;
    size_t src = 0, sc = kNone, bi = kNone;
    size_t dst = 0, dst_lo = kNone, dst_bias = kNone;
    GZW_HD size_t count() const { return (size_t)rows * cols; }
};
struct JobList {
    std::vector<BNRef> folds;   // first, into a buffer of fold_floats floats
    std::vector<Job> packs;     // then, in any order, into the zeroed image
    int fold_floats = 0;
};

inline JobList job_list(const PackSpec& s, const BlobPlan& P, const ImageLayout& I) {
    const gz_net_desc& d = s.d;
    // F = the model's filters; FP = the kernel's (padded with zero channels: zero weights and zero
    // folded bias keep them at 0 through every ReLU and residual add)
    const int F = d.cnn_filter_size, FP = s.fpad, B = d.residual_layers, R = d.role_count, S = d.se_units;
    const int HW = d.input_columns * d.input_rows, NL = cal_layers(d), VH = d.value_hidden_size;
    const int T0 = initial_kernel(d) * initial_kernel(d);
    JobList J;
    J.folds = P.folds;
    J.fold_floats = P.fold_floats;
    auto conv = [&](int kind, size_t w, const BNRef& bn, int taps, int cin, int cinp, size_t dst, size_t dst_lo, size_t dst_bias) {
        Job j;
        j.kind = kind; j.rows = taps * cin; j.cols = F;
        j.F = F; j.FP = FP; j.cin = cin; j.cinp = cinp; j.P2 = s.p2; j.f16 = s.f16 ? 1 : 0;
        j.src = w; j.sc = bn.scale(); j.bi = bn.bias();
        j.dst = dst; j.dst_lo = dst_lo; j.dst_bias = dst_bias;
        J.packs.push_back(j);
    };
    // a 1x1 conv [F][stride] column times its BN's scale -> a row of FP floats, its folded bias -> one float
    auto conv1x1 = [&](size_t w, int stride, const BNRef& bn, int ch, size_t dst_row, size_t dst_bias) {
        Job j;
        j.kind = kScaleVec; j.cols = F; j.ss = stride;
        j.src = w + ch; j.sc = bn.scale() + ch; j.dst = dst_row;
        J.packs.push_back(j);
        Job b;
        b.kind = kFoldVec; b.cols = 1;
        b.src = bn.bias() + ch; b.dst = dst_bias;
        J.packs.push_back(b);
    };
    auto fold_row = [&](size_t src, size_t dst) {
        Job j;
        j.kind = kFoldVec; j.cols = F; j.src = src; j.dst = dst;
        J.packs.push_back(j);
    };
    auto rows = [&](size_t src, int nrows, int width, int dst_pitch, size_t dst) {
        Job j;
        j.kind = kRowCopy; j.rows = nrows; j.cols = width; j.ss = width; j.ds = dst_pitch;
        j.src = src; j.dst = dst;
        J.packs.push_back(j);
    };
    if (s.fp32) conv(kPackF32, P.w0, P.bn0, T0, d.input_channels, s.cp, I.w0, kNone, I.b0);
    else conv(kPackW0, P.w0, P.bn0, T0, d.input_channels, s.K0, I.w0, s.p2 == 2 ? I.w0lo : kNone, I.b0);
    for (int c = 0; c < 2 * B; ++c)
        conv(s.fp32 ? kPackF32 : kPackTrunk, P.wconv[c], P.bnconv[c], 9, F, FP, I.wres + c * I.conv_bytes, kNone,
             I.bres + (size_t)c * FP * 4);
    for (int blk = 0; blk < (int)P.pre.size(); ++blk) {
        fold_row(P.pre[blk].scale(), I.pre + (size_t)(2 * blk) * FP * 4);
        fold_row(P.pre[blk].bias(), I.pre + (size_t)(2 * blk + 1) * FP * 4);
    }
    for (int blk = 0; blk < (int)P.se_c.size(); ++blk) {   // [F][S] -> [FP][S] and [S][F] -> [S][FP]
        rows(P.se_c[blk], 1, F * S, F * S, I.sew1 + (size_t)blk * FP * S * 4);
        rows(P.se_g[blk], S, F, FP, I.sew2 + (size_t)blk * S * FP * 4);
    }
    // head 1x1 convs: 2 per role, then the value conv (unused with concat_all_layers)
    for (int r = 0; r < R; ++r)
        for (int c = 0; c < 2; ++c) conv1x1(P.hw[r], 2, P.hbn[r], c, I.wh + (size_t)(2 * r + c) * FP * 4, I.bh + (2 * r + c) * 4);
    for (int j = 0; j < NL; ++j) conv1x1(P.clw[j], 1, P.clbn[j], 0, I.wcl + (size_t)j * FP * 4, I.bcl + j * 4);
    if (NL == 0) conv1x1(P.vw, 1, P.vbn, 0, I.wh + (size_t)(2 * R) * FP * 4, I.bh + 2 * R * 4);
    // the dense heads, Keras [K][N] (k-major), with their output dimension padded to a multiple of 4
    // (zero columns: forward_kernel.h dense_heads loads 4 consecutive outputs per float4)
    for (int r = 0; r < R; ++r) {
        const int Pr = d.policy_dist_count[r];
        rows(P.pd[r], 2 * HW, Pr, (Pr + 3) & ~3, I.pd[r]);
        rows(P.pb[r], 1, Pr, Pr, I.pb[r]);
        if (s.gemm_heads) {
            Job j;
            j.kind = kGemmFrag; j.rows = ((Pr + 15) / 16) * ((2 * HW + 31) / 32); j.cols = 64 * 8;
            j.F = Pr; j.cin = 2 * HW;
            j.src = P.pd[r]; j.dst = I.pdp[r];
            J.packs.push_back(j);
        }
    }
    rows(P.vhw, value_features(d), VH, (VH + 3) & ~3, I.vhw);
    rows(P.vhb, 1, VH, VH, I.vhb);
    rows(P.vdw, 1, VH * d.num_values, VH * d.num_values, I.vdw);
    rows(P.vdb, 1, d.num_values, d.num_values, I.vdb);
    return J;
}

// ---- the elements ------------------------------------------------------------------------------
// Float operations with the host's rounding whatever the device compiler contracts or approximates:
// each computed in double and rounded to float at once -- correctly rounded, since 53 >= 2 x 24 + 2
// bits makes the double rounding innocuous for + - * / sqrt.  The opaque register barriers keep the
// compiler from narrowing the double operation back to a float one and from fusing a multiply with
// the next add into one v_fma_f32 (which -ffp-contract=fast would otherwise do: observed as 1-5 ulp
// differences of the folded biases from the host's).  The host's are the plain float operations.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ double f_keep(double x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ float f_keep(float x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ float f_mul(float a, float b) { return f_keep((float)f_keep((double)a * (double)b)); }
__device__ __forceinline__ float f_add(float a, float b) { return f_keep((float)f_keep((double)a + (double)b)); }
__device__ __forceinline__ float f_sub(float a, float b) { return f_keep((float)f_keep((double)a - (double)b)); }
__device__ __forceinline__ float f_div(float a, float b) { return f_keep((float)f_keep(__ddiv_rn((double)a, (double)b))); }
__device__ __forceinline__ float f_sqrt(float a) { return f_keep((float)f_keep(__dsqrt_rn((double)a))); }
#else
inline float f_mul(float a, float b) { return a * b; }
inline float f_add(float a, float b) { return a + b; }
inline float f_sub(float a, float b) { return a - b; }
inline float f_div(float a, float b) { return a / b; }
inline float f_sqrt(float a) { return std::sqrt(a); }
#endif

// bf16, round to nearest even
GZW_HD inline uint16_t f2bf(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // quiet NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
// split precision: x = hi + lo, hi = bf16(x), lo = bf16(x - hi)
GZW_HD inline uint16_t lo_of(float v) {
    return f2bf(f_sub(v, __builtin_bit_cast(float, (uint32_t)f2bf(v) << 16)));
}

// fp16 (IEEE binary16), round to nearest even: subnormals kept, 65,520 and above to infinity
GZW_HD inline uint16_t f2h(float f) {
    const uint32_t u = __builtin_bit_cast(uint32_t, f), a = u & 0x7fffffffu;
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);   // quiet NaN
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // rounds to 2^16 or more: infinity
    if (a < 0x33000001u) return sign;                         // at most 2^-25: zero (the tie goes to even)
    const int e = (int)(a >> 23) - 127;                       // -25 .. 15
    const uint32_t m = (a & 0x007fffffu) | 0x00800000u;       // 24 bits
    // the result's unit in the last place is 2^(e - 10), or 2^-24 below the normals: drop `sh` bits
    const int sh = e >= -14 ? 13 : 13 + (-14 - e);            // 13 .. 24
    const uint32_t keep = m >> sh, rest = m & ((1u << sh) - 1u), half = 1u << (sh - 1);
    const uint32_t r = keep + ((rest > half || (rest == half && (keep & 1u))) ? 1u : 0u);
    // normals: r carries the hidden bit at 2^10, a carry out of the significand raises the exponent
    // (subnormals: the exponent field is 0 and r, up to 2^10, is the field or the smallest normal)
    return (uint16_t)(sign | (e >= -14 ? (uint32_t)(e + 14) * 1024u + r : r));
}
GZW_HD inline float h2f(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
    if (e == 31u) return __builtin_bit_cast(float, sign | 0x7f800000u | (m << 13));
    if (e) return __builtin_bit_cast(float, sign | ((e + 112u) << 23) | (m << 13));
    // subnormal: m 2^-24, exact in fp32 (the product of an integer below 2^10 and a power of two)
    const float v = (float)m * 5.9604644775390625e-8f;
    return sign ? -v : v;
}
// fp16x3: x = hi + lo 2^-11, hi = f16(x), lo = f16((x - hi) 2^11) -- the subtraction and the scaling are
// exact in fp32; the scaled lo part stays clear of fp16's subnormals (Ootomo and Yokota's scheme)
constexpr float kF16LoScale = 2048.f;
GZW_HD inline uint16_t h_lo_of(float v) { return f2h(f_mul(f_sub(v, h2f(f2h(v))), kF16LoScale)); }

// Element offset (within one trunk conv's image) of weight [co][ci] of tap `tap`, hi part; the lo
// part (split precision) sits 512 elements (1 KB) further.  A k-step (tap, 32 input channels) is
// FP/16 blocks of 16 output channels; block = P2 fragments of 1 KB, each in MFMA A-fragment lane
// order (lane = co % 16 + 16 * (k / 8), 8 consecutive k per lane), so one wave-wide 16-byte load
// reads 1 KB contiguous (forward_kernel.h FragOff).
GZW_HD inline size_t wres_index(int tap, int co, int ci, int FP, int P2) {
    const int kc = ci >> 5, k = ci & 31;
    const size_t blk = ((size_t)(tap * (FP >> 5) + kc) * (FP >> 4) + (co >> 4)) * P2;
    return (blk * 64 + (co & 15) + 16 * (k >> 3)) * 8 + (k & 7);
}

// where elements go: the image itself (the CPU check substitutes one that records every write)
struct RawImage {
    char* p;
    GZW_HD void put16(size_t off, uint16_t v) const { *(uint16_t*)(p + off) = v; }
    GZW_HD void put32(size_t off, float v) const { *(float*)(p + off) = v; }
};

// scale = g / sqrt(var + eps), bias = be - mu scale; after a conv with bias cb (legacy model files):
// gamma (conv + cb - mean) / sqrt(var + eps) + beta = scale conv + (be + (cb - mu) scale)
GZW_HD inline void fold_element(const BNRef& b, int i, const float* blob, float* fold) {
    float sc = 1.f, bi = b.cb != kNone ? blob[b.cb + i] : 0.f;
    if (b.g != kNone) {
        sc = f_div(blob[b.g + i], f_sqrt(f_add(blob[b.var + i], 1e-3f)));
        bi = b.cb != kNone ? f_add(blob[b.be + i], f_mul(f_sub(blob[b.cb + i], blob[b.mu + i]), sc))
                           : f_sub(blob[b.be + i], f_mul(blob[b.mu + i], sc));
    }
    fold[b.out + i] = sc;
    fold[b.out + b.n + i] = bi;
}

template <class Img>
GZW_HD inline void w0_element(const Img& img, const Job& j, int k, int co, float v) {
    const size_t o = (((size_t)(k / 32) * j.FP + co) * 32 + (k % 32)) * 2;
    img.put16(j.dst + o, j.f16 ? f2h(v) : f2bf(v));
    if (j.dst_lo != kNone) img.put16(j.dst_lo + o, j.f16 ? h_lo_of(v) : lo_of(v));
}
template <class Img>
GZW_HD inline void trunk_conv_element(const Img& img, const Job& j, int tap, int co, int ci, float v) {
    const size_t o = j.dst + wres_index(tap, co, ci, j.FP, j.P2) * 2;
    img.put16(o, j.f16 ? f2h(v) : f2bf(v));
    if (j.P2 == 2) img.put16(o + 512 * 2, j.f16 ? h_lo_of(v) : lo_of(v));
}
// (the product is one fp32 multiply, rounded once)
template <class Img>
GZW_HD inline void f32_conv_element(const Img& img, size_t dst, int tap, int co, int ci, int cinp, int FP, float w, float scale) {
    img.put32(dst + gzfp32::wfrag_index(tap, co, ci, cinp, FP) * 4, f_mul(w, scale));
}
template <class Img>
GZW_HD inline void gemm_frag_element(const Img& img, const Job& j, int t, int c, const float* blob) {
    const int P = j.F, K = j.cin, nkt = (K + 31) / 32, l = c >> 3, e = c & 7;
    const int row = 16 * (t / nkt) + (l & 15), k = 32 * (t % nkt) + 8 * (l >> 4) + e;
    if (row >= P || k >= K) return;
    const float v = blob[j.src + (size_t)k * P + row];
    const size_t o = j.dst + ((((size_t)t * 2) * 64 + l) * 8 + e) * 2;
    img.put16(o, f2bf(v));
    img.put16(o + 64 * 8 * 2, lo_of(v));
}

// element (r, c) of a job of kind `kind` (= j.kind; apart so that a caller can make it a constant)
template <class Img>
GZW_HD inline void pack_element(int kind, const Job& j, int r, int c, const float* blob, const float* fold, const Img& img) {
    switch (kind) {
    case kPackW0:
    case kPackTrunk:
    case kPackF32: {
        const float w = blob[j.src + (size_t)r * j.F + c], scale = fold[j.sc + c];
        if (r == 0) img.put32(j.dst_bias + (size_t)c * 4, fold[j.bi + c]);
        if (kind == kPackW0) w0_element(img, j, r, c, f_mul(w, scale));
        else if (kind == kPackTrunk) trunk_conv_element(img, j, r / j.cin, c, r % j.cin, f_mul(w, scale));
        else f32_conv_element(img, j.dst, r / j.cin, c, r % j.cin, j.cinp, j.FP, w, scale);
        break;
    }
    case kScaleVec: img.put32(j.dst + (size_t)c * j.ds * 4, f_mul(blob[j.src + (size_t)c * j.ss], fold[j.sc])); break;
    case kFoldVec: img.put32(j.dst + (size_t)c * 4, fold[j.src + c]); break;
    case kRowCopy: img.put32(j.dst + ((size_t)r * j.ds + c) * 4, blob[j.src + (size_t)r * j.ss + c]); break;
    case kGemmFrag: gemm_frag_element(img, j, r, c, blob); break;
    }
}

// ---- the host executor -------------------------------------------------------------------------
// The jobs over a host blob into img, which the caller zeroed (I.total bytes behind a RawImage).
template <class Img>
inline void pack_image_host(const JobList& J, const float* blob, const Img& img) {
    std::vector<float> fold((size_t)J.fold_floats);
    for (const BNRef& b : J.folds)
        for (int i = 0; i < b.n; ++i) fold_element(b, i, blob, fold.data());
    // (the job a copy, so its fields stay in registers across the image's stores; the trunk convs,
    // nearly all of the elements, with the kind a constant, so pack_element's switch folds: together
    // a third of the time)
    auto run = [&](auto kind, const Job j) {
        for (int r = 0; r < j.rows; ++r)
            for (int c = 0; c < j.cols; ++c) pack_element(kind, j, r, c, blob, fold.data(), img);
    };
    for (const Job& j : J.packs)
        switch (j.kind) {
        case kPackTrunk: run(std::integral_constant<int, kPackTrunk>(), j); break;
        case kPackF32: run(std::integral_constant<int, kPackF32>(), j); break;
        default: run(j.kind, j);
        }
}

// fp16x3-layered: the first conv with a folded weight that fp16 cannot hold (its hi part would be
// infinite) -- 0 the initial conv, c + 1 trunk conv c -- or -1 when every weight fits
GZW_HD inline bool f16_holds(const Job& j, int r, int c, const float* blob, const float* fold) {
    return (f2h(f_mul(blob[j.src + (size_t)r * j.F + c], fold[j.sc + c])) & 0x7fffu) < 0x7c00u;
}
inline int f16_range_check(const JobList& J, const float* blob) {
    std::vector<float> fold((size_t)J.fold_floats);
    for (const BNRef& b : J.folds)
        for (int i = 0; i < b.n; ++i) fold_element(b, i, blob, fold.data());
    int conv = 0;
    for (const Job& j : J.packs) {
        if (j.kind != kPackW0 && j.kind != kPackTrunk) continue;
        for (int r = 0; r < j.rows; ++r)
            for (int c = 0; c < j.cols; ++c)
                if (!f16_holds(j, r, c, blob, fold.data())) return conv;
        ++conv;
    }
    return -1;
}

}  // namespace gzw

namespace gzfp32 {
// One conv's kernel (Keras HWIO [taps][cin][F]) times scale[co] into the zeroed image dst
// (conv_image_floats(taps, cinp, FP) floats; cinp >= cin input channels of the activations it
// multiplies): the kPackF32 job's elements on their own (tests/fp32_host_check.cpp).
inline void pack_conv_host(float* dst, const float* w, const float* scale, int taps, int cin, int cinp, int F, int FP) {
    const gzw::RawImage img{(char*)dst};
    for (int tap = 0; tap < taps; ++tap)
        for (int ci = 0; ci < cin; ++ci)
            for (int co = 0; co < F; ++co)
                gzw::f32_conv_element(img, 0, tap, co, ci, cinp, FP, w[((size_t)tap * cin + ci) * F + co], scale[co]);
}
}  // namespace gzfp32
