// libgz_nn.so -- C-ABI (include/gzero_nn.h) around the fused gfx950 forward kernel.
//
// Weights: weight_image.h describes the device image of the canonical Keras-order float32 blob
// (BatchNorm folded, conv kernels in MFMA fragment order) as one job list; here it runs on the CPU
// for a host blob and as kernels for a device blob, into one device allocation.
#define GZNN_DEFINE_HEADS_KERNEL
#include "forward_kernel.h"
#include "trunk_variants.h"
#include "fp32_forward.h"
#include "layered_forward.h"
#include "eval_cache.h"
#include "shadow_compare.h"
#include "symmetry.h"
#include "weight_image.h"
#include "../../../include/gzero_nn.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace gznn;
using namespace gzw;

static thread_local std::string g_err;

static int fail(const std::string& msg) {
    g_err = msg;
    return -1;
}

#define HIPCHK(x)                                                                        \
    do {                                                                                 \
        hipError_t e_ = (x);                                                             \
        if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)


struct gz_net : PackSpec {         // d, fpad, p2, K0, cp, fp32, gemm_heads: what the weight image depends on
    int device = 0;
    size_t nweights = 0;
    struct Trunk {
        const void* fn = nullptr;
        int nb = 1;                // boards per workgroup
        int smem = 0;              // dynamic LDS bytes
        int btab_off = 0;          // LDS offset of the bias table
        int se_off = 0;            // LDS offset of the squeeze-excite scratch
        int cal_off = 0;           // LDS offset of the concat_all_layers partial sums
        bool fused_heads = false;  // the dense heads run inside the trunk kernel (no heads_kernel launch)
        int resid_bytes = 0;       // global residual scratch per workgroup
        int threads = 256;         // workgroup size (512: two wave groups)
        int wgs_per_cu = 1;        // workgroups resident per CU (2: the in-place kernel, variant 25)
        std::string name;          // kernel name (rocprofv3's)
    } small, large;                // launches below / from large_min_rows rows
    int large_min_rows = 1 << 30;
    bool has_weights = false;
    size_t image_bytes = 0;        // bytes of the device weight image
    float last_roll_ms = 0.f;      // device time of the last gz_net_set_weights_device

    char* dmem = nullptr;          // all weights, one allocation
    KParams kp{};                  // weight pointers filled in, outputs per launch
    std::mutex wmu;                // guards dmem / kp's weight pointers / has_weights (weight rolls)
    unsigned long long wepoch = 1; // weight generation (under wmu): every installed image and every change of
                                   // kp.logits bumps it; an evaluation cache flushes when it moves (eval_cache.h)

    hipStream_t stream = nullptr;  // for the synchronous host-buffer forward
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float* d_io = nullptr;         // staging: planes + outputs
    int io_cap = 0;
    float last_ms = 0.f;
    int heads_smem = 0;
    std::map<hipStream_t, std::pair<float*, int>> glog;   // policy_gemm_kernel's logits scratch per stream (gemm_heads)
    std::mutex feat_mu;            // head-feature scratch, one per stream (launches on one stream are ordered)
    std::map<hipStream_t, std::pair<float*, int>> feat;
    std::map<hipStream_t, std::pair<char*, size_t>> resid;   // global-residual scratch per stream
    unsigned long long* d_stamps = nullptr;   // GZ_KERNEL_STAMPS diagnostics
    int stamp_cap = 0;
    bool stamps_on = false;
    double stamp_avg[8] = {0};
    // GZ_PRECISION_FP32 (fp32_forward.h): fp32 conv images, the layer-wise trunk's scratch per stream
    int chunk_rows = 1;           // rows per sequential chunk of a launch (GZ_FP32_CHUNK_ROWS overrides)
    const float* w0f = nullptr;
    const float* wresf = nullptr;
    std::map<hipStream_t, std::pair<char*, int>> fscr;   // scratch and the rows it holds
    // GZ_PRECISION_BF16_LAYERED / _SPLIT_LAYERED (layered_forward.h): the same layer-wise trunk and scratch
    // with the bf16 conv over the fused modes' weight image; 1 (bf16) or 3 (split) parts, 0: another mode.
    // GZ_PRECISION_F16X3_LAYERED: gzlayered::kF16Parts (PackSpec::f16 set), the fp16 hi | lo image and the
    // per-board exponents of each conv's input, one buffer of as many ints as scratch rows per stream
    int layered = 0;
    std::map<hipStream_t, int*> bexp;
    int in_width() const { return layered ? K0 : cp; }   // input channels of the initial conv's launch
    // the shadow check (gzero_nn.h gz_net_shadow_enable): `shadow` is read by launches under wmu and by
    // gz_net_shadow_stats under shadow_mu, and changed under both (lock order wmu, shadow_mu)
    struct Shadow;
    Shadow* shadow = nullptr;
    std::mutex shadow_mu;
    bool is_shadow = false;        // a shadow has none of its own and is reached through its net alone
};

// A net's shadow: the second net, the device block of running totals, and a ring of pinned snapshots
// of that block, one per check in flight, each with the events around its check.
struct gz_net::Shadow {
    static constexpr int kSlots = 8;
    gz_net* net = nullptr;         // same desc, another precision; its images are installed under the owner's wmu
    int every = 64, max_rows = 256;
    bool from_env = false;         // GZ_NN_SHADOW: gz_net_destroy prints the totals
    long forwards = 0;             // the owner's forwards of n > 0 since the enable
    gz_shadow_stats* d_acc = nullptr;        // the cumulative block (device)
    struct Out { float* out = nullptr; gzshadow::RowRecord* rec = nullptr; };
    std::map<hipStream_t, Out> out;          // the shadow's outputs [max_rows][sum P_r + V] and row records, per stream
    struct Slot {
        gz_shadow_stats* host = nullptr;     // pinned
        hipEvent_t e0 = nullptr, e1 = nullptr;
        bool pending = false;
        long epoch = 0;
    } slot[kSlots];
    int next = 0;                  // the slot of the next check (the ring is harvested oldest first from here)
    hipStream_t last_stream = nullptr;
    int last_slot = -1;
    long epoch = 0;                // bumped by a reset: snapshots of earlier epochs are dropped
    bool fresh = true;             // the next check's fold starts the block from zero
    gz_shadow_stats done{};        // the newest completed snapshot of this epoch, device_ms summed
};

extern "C" const char* gz_nn_last_error(void) { return g_err.c_str(); }

// ---- kernel instantiations: trunk_variants.h (per padded filter count and position tiles) ----------
// Variants: NB = boards per workgroup (weight-fragment reuse factor), WPE = minimum resident waves
// per SIMD the register budget must allow (= workgroups per CU).  GZ_KERNEL_VARIANT=<NB><WPE>
// (e.g. "12") overrides the per-launch choice for experiments.

// Measured on MI355X (profiles/r01c_kernel_variants.txt): one board per workgroup with the whole
// register file (11) is fastest while the launch has fewer boards than ~1.5x the CU count; from
// there two boards per workgroup (21) win, each weight fragment feeding twice the MFMAs.  Every
// variant computes each row identically (tests/test_nn_gpu.py::test_kernel_variants_identical), so
// choosing per launch keeps results batch-invariant.
// Launches of 257-383 rows also take the two-board kernel: at one board per workgroup they would
// need a second wave of workgroups on the 256 CUs (one trunk workgroup per CU by LDS).
// large launches: the two-board 4-wave kernel (21).  The 8-wave kernel (24) is 5 % faster back to
// back (profiles/r04t_w8_kexp.txt) but equal inside the bench, whose launches arrive with gaps
// (0.4954 vs 0.4942 ms per 1,024-row launch, same box; profiles/r04x_variants_in_bench.txt):
// selectable (GZ_KERNEL_VARIANT=24), bit-identical.  Round 5: the split F = 128 kernels of boards up
// to 64 positions take variant 23 (trunk_kernel_h2: two groups of two waves, a board each -- half the
// B-fragment reads per MFMA), 1-1.5 % faster than 21 at 1,024 rows (profiles/r05t_ab_v23.txt) and
// bit-identical (the kernels build with -ffp-contract=on).  kLargeFallback: where kLargeVariant is
// not compiled for a geometry.
// Variant 25 (trunk_kernel_h2i: 23's decomposition with one image per board in place, 256 registers
// per wave) is built for two workgroups per CU.  It takes the large launches only where two of its
// workgroups fit the LDS side by side (2 x smem <= 160 KB: with the bias table in LDS, F = 128 nets of
// up to 8 residual blocks) and the runtime reports two resident workgroups; otherwise 23 stays.
constexpr int kSmallVariant = 11, kLargeVariant = 23, kLargeFallback = 21, kLargeMinRows = 257;
constexpr int kLargeInPlace = 25;
// At four position tiles variant 25 is the row-pair kernel (rowpair.h), for 8 x 8 boards without a
// pooling value head; the other such boards get the same in-place kernel with a board per group.
constexpr int kInPlaceGeneric = 26;
constexpr int kCUs = 256;

static KernelChoice select_kernel(const gz_net_desc& d, int fpad, int pt, int v, int precision, bool v2) {
    if (pt < 1 || pt > kMaxPT) return KernelChoice{};
    KernelChoice k = trunk_variant(fpad, pt, v, precision, v2);
    if (k.fn && k.square8 && (d.input_columns != 8 || d.input_rows != 8 || gap_features(d)))
        k = trunk_variant(fpad, pt, kInPlaceGeneric, precision, v2);
    return k;
}

// gz_net_create's first half: every refusal that needs no device, and the net's host-side state.
static gz_net* create_host(const gz_net_desc& d, int device, gz_net::Trunk* in_place) {
    if (d.cnn_kernel_size != 3) { fail("only cnn_kernel_size 3 is supported"); return nullptr; }
    if (d.role_count < 1 || d.role_count > GZ_MAX_ROLES) { fail("role_count out of range"); return nullptr; }
    if (d.num_values < 1 || d.num_values > 4) { fail("num_values out of range"); return nullptr; }
    if (initial_kernel(d) != 1 && initial_kernel(d) != 3) { fail("initial conv kernel must be 1 or 3"); return nullptr; }
    if (d.se_units < 0 || d.se_units > kMaxSE || (d.se_units && !d.resnet_v2)) {
        fail("squeeze-excite units must be 0.." + std::to_string(kMaxSE) + " on a v2 net");
        return nullptr;
    }
    if (d.concat_all_layers && (!d.resnet_v2 || d.global_pooling_value || d.value_bn)) {
        fail("concat_all_layers needs a v2 net without the pooling value head (model.py:251-252)");
        return nullptr;
    }
    const int precision = d.precision == 0 ? GZ_PRECISION_BF16 : d.precision;
    const bool fp32 = precision == GZ_PRECISION_FP32;
    const int layered = precision == GZ_PRECISION_BF16_LAYERED ? 1 : precision == GZ_PRECISION_SPLIT_LAYERED ? 3 :
                        precision == GZ_PRECISION_F16X3_LAYERED ? gzlayered::kF16Parts : 0;
    const bool layerwise = fp32 || layered;   // the trunk layer by layer through HBM: no LDS-image limit
    if (precision != GZ_PRECISION_BF16 && precision != GZ_PRECISION_SPLIT && !layerwise) { fail("unknown precision"); return nullptr; }
    int vs = kSmallVariant, vl = kLargeVariant, min_large = kLargeMinRows;
    if (const char* e = getenv("GZ_KERNEL_VARIANT")) {   // experiments: one fixed variant
        vs = vl = atoi(e);
        min_large = 1 << 30;
    }
    // kernels are compiled per padded filter count and position-tile count; the board's H and W
    // are kernel arguments (H = input_columns, W = input_rows: bases.py:104-121)
    const int npos_ = d.input_columns * d.input_rows;
    const int pt = kernel_tiles((npos_ + 15) / 16);
    const int fpad = fp32 ? gzfp32::padded_filters(d.cnn_filter_size) : kernel_filters(d.cnn_filter_size, (npos_ + 15) / 16);
    if (d.input_rows > 32 || npos_ >= 1024) { fail("board too large"); return nullptr; }
    const bool v2 = d.resnet_v2 != 0;
    if (layerwise) {
        // the layer-wise paths have no LDS-image limit: any board up to 19 x 19, F <= 256, v1 or v2
        if (d.input_columns < 1 || d.input_rows < 1 || d.input_columns > gzfp32::kMaxBoardSide ||
            d.input_rows > gzfp32::kMaxBoardSide || fpad == 0 || d.input_channels < 1) {
            fail("unsupported network geometry F=" + std::to_string(d.cnn_filter_size) + " H=" +
                 std::to_string(d.input_columns) + " W=" + std::to_string(d.input_rows) +
                 (fp32 ? " (fp32-ieee: boards up to 19 x 19, F <= 256)" : " (layered modes: boards up to 19 x 19, F <= 256)"));
            return nullptr;
        }
        min_large = 1 << 30;   // one conv kernel for every launch size
    }
    KernelChoice kc = layerwise ? KernelChoice{} : select_kernel(d, fpad, pt, vs, precision, v2);
    KernelChoice kl = layerwise ? KernelChoice{} : select_kernel(d, fpad, pt, vl, precision, v2);
    if (!kl.fn && vl == kLargeVariant) kl = select_kernel(d, fpad, pt, kLargeFallback, precision, v2);
    // wave-group kernels: each group's staging / heads scratch must fit its own image
    auto wg_fits = [&](const KernelChoice& c) {
        if (c.groups == 1) return true;
        const int np = d.input_columns * d.input_rows;
        const int kk0 = initial_kernel(d);
        const int k0p = ((kk0 * kk0 * d.input_channels + 31) / 32) * 32;
        const int p2 = precision == GZ_PRECISION_SPLIT ? 2 : 1;
        return trunk_scratch_bytes(np, d.input_channels, k0p, d.role_count, p2, fpad) <= c.act_bytes &&
               fused_heads_bytes(np, d.role_count, heads_row(d.role_count, d.policy_dist_count, d.value_hidden_size),
                                 gap_features(d), c.nb, 1, fpad) <= c.act_bytes;
    };
    if (kl.fn && !wg_fits(kl)) {
        // the wave-group default (23) does not fit this geometry's scratch: the two-board 4-wave
        // kernel (21, one image per workgroup) before the one-board one
        kl = vl == kLargeVariant ? select_kernel(d, fpad, pt, kLargeFallback, precision, v2) : KernelChoice{};
        if (kl.fn && !wg_fits(kl)) kl = KernelChoice{};
    }
    if (kc.fn && !wg_fits(kc)) kc = KernelChoice{};
    // the two-workgroups-per-CU candidate for the large launches (decided below, with the device)
    KernelChoice ki = !layerwise && getenv("GZ_KERNEL_VARIANT") == nullptr && kl.fn
                          ? select_kernel(d, fpad, pt, kLargeInPlace, precision, v2) : KernelChoice{};
    if (ki.fn && !wg_fits(ki)) ki = KernelChoice{};
    if (kc.fn && !kl.fn && vl != vs) {   // geometries with a single (one board per workgroup) variant
        kl = kc;
        min_large = 1 << 30;
    }
    if (!layerwise && (!kc.fn || !kl.fn)) {
        fail("unsupported network geometry F=" + std::to_string(d.cnn_filter_size) + " H=" +
             std::to_string(d.input_columns) + " W=" + std::to_string(d.input_rows) +
             (precision == GZ_PRECISION_SPLIT ? " (split precision)" : "") + (v2 ? " (v2)" : "") +
             (fpad == 256 ? " (F > 128: boards of up to 176 positions; larger boards run in fp32-ieee)" : ""));
        return nullptr;
    }
    gz_net* net = new gz_net;
    net->d = d;
    net->device = device;
    net->large_min_rows = min_large;
    static_cast<PackSpec&>(*net) = pack_spec(d, precision, fpad, false);   // (gemm_heads: below)
    net->layered = layered;
    const int k0 = initial_kernel(d);
    if (layerwise) {
        net->chunk_rows = gzfp32::chunk_rows_for(npos_, net->in_width(), fpad);
        if (const char* e = getenv("GZ_FP32_CHUNK_ROWS"))   // tests: chunking without a large launch
            net->chunk_rows = std::max(1, std::min(atoi(e), net->chunk_rows));
    }
    net->nweights = blob_plan(d).consumed;
    int maxP = 0;
    for (int r = 0; r < d.role_count; ++r) maxP = std::max(maxP, d.policy_dist_count[r]);
    const int npos = d.input_columns * d.input_rows;
    // the dense heads' LDS row: the two-phase layout where every kernel's LDS still fits, else the
    // sequential one (forward_kernel.h dense_heads / dense_heads_seq)
    int lgrow = heads_row(d.role_count, d.policy_dist_count, d.value_hidden_size, true);
    bool heads_seq = false;
    // LDS: two ping-pong activation images per board; the scratch (input staging, heads) aliases
    // the second image set, which holds nothing live at those times.
    const int scr_in = trunk_scratch_bytes(npos, d.input_channels, net->K0, d.role_count, net->p2, fpad);
    auto trunk = [&](const KernelChoice& c) {
        gz_net::Trunk t;
        t.fn = c.fn;
        t.nb = c.nb;
        t.threads = c.threads;
        t.wgs_per_cu = c.wgs_per_cu;
        t.name = c.name;
        t.fused_heads = !c.single_image && !d.concat_all_layers;
        const int scr = t.fused_heads ? std::max(scr_in, fused_heads_bytes(npos, d.role_count, lgrow, gap_features(d), c.nb,
                                                                           c.groups == 2 ? 1 : c.nb, fpad))
                                      : scr_in;
        // (in place: the scratch lies inside the images, wg_fits)
        t.btab_off = c.single_image ? align16(std::max(c.act_bytes, scr))
                     : c.in_place   ? c.nb * c.act_bytes + c.img_pad
                                    : c.nb * c.act_bytes + std::max(c.nb * c.act_bytes, scr);
        t.resid_bytes = c.resid_bytes;
        t.smem = t.btab_off + bias_table_bytes(fpad, d.residual_layers);
        t.se_off = t.smem;
        if (d.se_units) t.smem += se_scratch_bytes(fpad, c.nb, d.se_units);
        t.cal_off = t.smem;
        if (d.concat_all_layers) t.smem += align16(4 * c.nb * npos * 4);
        return t;
    };
    const int FS = 2 * d.role_count * npos + value_features(d);   // head features per board
    for (int pass = 0; pass < 2; ++pass) {
        net->small = trunk(kc);
        net->large = trunk(kl);
        if (layerwise) {   // no trunk kernel: fp32_forward.hip's launches, then heads_kernel
            gz_net::Trunk t;
            t.name = layered ? gzlayered::conv_kernel_name(fpad, layered) : gzfp32::conv_kernel_name(fpad);
            net->small = net->large = t;
        }
        net->heads_smem = heads_lds_bytes(FS, lgrow);
        if (pass == 1 || (net->small.smem <= 160 * 1024 && net->large.smem <= 160 * 1024 && net->heads_smem <= 160 * 1024))
            break;
        heads_seq = true;
        lgrow = heads_row(d.role_count, d.policy_dist_count, d.value_hidden_size, false);
    }
    // Large policies on nets whose every launch runs the separate heads kernel: the policy Dense
    // layers run as one MFMA GEMM per launch (policy_gemm_kernel) instead of heads_kernel's
    // per-4-board fp32 loop (amazons P = 3041: 12 % of the forward).  Every launch of such a net
    // takes this path, so results stay batch-invariant.
    // (fp32-ieee, fp16x3-layered: the policy Dense stays fp32 on the VALU)
    net->gemm_heads = !fp32 && !net->f16 && !net->small.fused_heads && !net->large.fused_heads && maxP >= 512 &&
                      getenv("GZ_NO_GEMM_HEADS") == nullptr;
    KParams& kp = net->kp;
    kp.C = d.input_channels;
    kp.K0 = net->K0;
    kp.B = d.residual_layers;
    kp.R = d.role_count;
    kp.VH = d.value_hidden_size;
    kp.V = d.num_values;
    kp.leaky = d.leaky_relu;
    kp.flatten_nchw = d.flatten_nchw;
    kp.value_sigmoid = d.value_sigmoid;
    kp.v2 = d.resnet_v2 ? 1 : 0;
    kp.k0taps = k0 * k0;
    kp.init_act = has_initial_bn(d) ? 1 : 0;
    kp.S = d.se_units;
    kp.gapF = gap_features(d);
    kp.FS = FS;
    kp.VK = value_features(d);
    kp.cal = cal_layers(d);
    kp.nofuse = d.concat_all_layers ? 1 : 0;
    kp.maxP = maxP;
    kp.lgrow = lgrow;
    kp.heads_seq = heads_seq ? 1 : 0;
    kp.npos = npos;
    kp.gemm_heads = net->gemm_heads ? 1 : 0;
    kp.pkt = (2 * npos + 31) / 32;
    kp.plog = 0;
    for (int r = 0; r < d.role_count; ++r) kp.plog += d.policy_dist_count[r];
    kp.H = d.input_columns;
    kp.W = d.input_rows;
    kp.wmagic = (65536 + kp.W - 1) / kp.W;
    for (int r = 0; r < d.role_count; ++r) kp.P[r] = d.policy_dist_count[r];

    // the last refusal that needs no device: the image, the bias table (8 F bytes per residual block)
    // and the scratch beside them must fit the 160 KB of LDS
    for (const gz_net::Trunk* t : {&net->small, &net->large}) {
        if (t->smem > 160 * 1024) {
            fail("network needs " + std::to_string(t->smem) + " B of LDS per workgroup (160 KB max): too many residual blocks "
                 "for this board in this mode");
            delete net;
            return nullptr;
        }
    }
    // the two-workgroups-per-CU candidate for the large launches (create_device decides, with the device)
    *in_place = ki.fn && net->large_min_rows < (1 << 30) ? trunk(ki) : gz_net::Trunk{};
    return net;
}

// gz_net_create's second half: the net's stream and events, the kernels' LDS limits and residency.
// Deletes the net on failure.
static gz_net* create_device(gz_net* net, const gz_net::Trunk& in_place) {
    const int device = net->device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&net->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&net->ev0) != hipSuccess || hipEventCreate(&net->ev1) != hipSuccess) {
        fail(std::string("HIP init failed: ") + hipGetErrorString(hipGetLastError()));
        delete net;
        return nullptr;
    }
    // workgroups of a trunk kernel the runtime keeps resident per CU at its dynamic LDS size
    auto resident = [&](const gz_net::Trunk& t) {
        int nblk = 0;
        if (t.smem > 64 * 1024 && hipFuncSetAttribute(t.fn, hipFuncAttributeMaxDynamicSharedMemorySize, t.smem) != hipSuccess)
            return 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nblk, t.fn, t.threads, t.smem) != hipSuccess) return 0;
        return nblk;
    };
    if (in_place.fn) {
        const gz_net::Trunk& t = in_place;
        if (2 * t.smem <= 160 * 1024 && resident(t) >= t.wgs_per_cu) net->large = t;
    }
    for (gz_net::Trunk* t : {&net->small, &net->large}) {
        if (t->smem > 64 * 1024 &&
            hipFuncSetAttribute(t->fn, hipFuncAttributeMaxDynamicSharedMemorySize, t->smem) != hipSuccess) {
            fail("cannot raise dynamic LDS limit");
            delete net;
            return nullptr;
        }
        // a fixed variant (GZ_KERNEL_VARIANT) reports what the device gives it
        if (t->wgs_per_cu > 1) t->wgs_per_cu = std::max(1, std::min(t->wgs_per_cu, resident(*t)));
    }
    if (net->heads_smem > 64 * 1024 &&
        hipFuncSetAttribute(net->fp32 || net->f16 ? (const void*)&heads_kernel_blocked : (const void*)&heads_kernel,
                            hipFuncAttributeMaxDynamicSharedMemorySize, net->heads_smem) != hipSuccess) {
        fail("cannot raise dynamic LDS limit (heads)");
        delete net;
        return nullptr;
    }
    return net;
}

// ---- the shadow check (gzero_nn.h) -----------------------------------------------------------------
namespace {
int net_precision(const gz_net_desc& d) { return d.precision == 0 ? GZ_PRECISION_BF16 : d.precision; }

// The refusals of gz_net_shadow_enable that need no device, then the shadow's host half: NULL with
// "shadow: ..." in g_err, or the shadow net (create_device still to run).
gz_net* shadow_host(const gz_net_desc& d, int device, int precision, int every, int max_rows, gz_net::Trunk* in_place) {
    if (precision == 0) precision = GZ_PRECISION_BF16;
    if (precision == net_precision(d)) {
        fail("shadow: precision " + std::to_string(precision) + " is the net's own mode");
        return nullptr;
    }
    if (every < 1 || max_rows < 1) {
        fail("shadow: every and max_rows must be at least 1");
        return nullptr;
    }
    gz_net_desc sd = d;
    sd.precision = precision;
    gz_net* s = create_host(sd, device, in_place);
    if (!s) {
        fail("shadow: " + g_err);
        return nullptr;
    }
    s->is_shadow = true;
    return s;
}

// GZ_NN_SHADOW=<precision>[:<every>[:<max_rows>]]: 1 parsed, 0 unset, -1 malformed (g_err)
int shadow_env(int* precision, int* every, int* max_rows) {
    const char* e = getenv("GZ_NN_SHADOW");
    if (!e || !*e) return 0;
    long v[3] = {0, 64, 256};
    int got = 0;
    const char* p = e;
    bool ok = true;
    while (ok && got < 3) {
        char* end = nullptr;
        const long x = strtol(p, &end, 10);
        ok = end != p && x >= 0 && x <= (1 << 20);
        v[got++] = x;
        p = end;
        if (!ok || *p == 0) break;
        ok = *p == ':' && got < 3;
        ++p;
    }
    if (!ok || *p != 0 || v[1] < 1 || v[2] < 1) {
        fail(std::string("GZ_NN_SHADOW: expected <precision>[:<every>[:<max_rows>]] with every and max_rows >= 1, got \"") + e + "\"");
        return -1;
    }
    *precision = (int)v[0];
    *every = (int)v[1];
    *max_rows = (int)v[2];
    return 1;
}

void shadow_free(gz_net::Shadow* sh) {   // (after a device sync, or before any launch)
    if (!sh) return;
    if (sh->net) gz_net_destroy(sh->net);
    if (sh->d_acc) (void)hipFree(sh->d_acc);
    for (auto& o : sh->out) (void)hipFree(o.second.out);   // (one allocation: the records follow the outputs)
    for (auto& s : sh->slot) {
        if (s.host) (void)hipHostFree(s.host);
        if (s.e0) (void)hipEventDestroy(s.e0);
        if (s.e1) (void)hipEventDestroy(s.e1);
    }
    delete sh;
}

// The device half of an enable: the shadow net's, the totals block and the snapshot ring.  Takes
// over (and on failure frees) the shadow net s.
int shadow_attach(gz_net* net, gz_net* s, const gz_net::Trunk& in_place, int every, int max_rows, bool from_env) {
    if (!create_device(s, in_place)) return fail("shadow: " + g_err);
    gz_net::Shadow* sh = new gz_net::Shadow;
    sh->net = s;
    sh->every = every;
    sh->max_rows = max_rows;
    sh->from_env = from_env;
    s->kp.logits = net->kp.logits;
    hipError_t e = hipMalloc((void**)&sh->d_acc, sizeof(gz_shadow_stats));
    for (auto& sl : sh->slot) {
        if (e == hipSuccess) e = hipHostMalloc((void**)&sl.host, sizeof(gz_shadow_stats), hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreate(&sl.e0);
        if (e == hipSuccess) e = hipEventCreate(&sl.e1);
    }
    if (e != hipSuccess) {
        shadow_free(sh);
        return fail(std::string("shadow: ") + hipGetErrorString(e));
    }
    std::lock_guard<std::mutex> wl(net->wmu);
    std::lock_guard<std::mutex> sl(net->shadow_mu);
    net->shadow = sh;
    return 0;
}

// Takes what has completed off the ring, oldest first (shadow_mu held): device_ms grows by each
// completed check's, `done` becomes the newest completed snapshot.  wait_slot >= 0: first wait for
// that slot's check (the ring is full, or the shadow is going away).
void shadow_harvest(gz_net::Shadow* sh, int wait_slot = -1) {
    if (wait_slot >= 0 && sh->slot[wait_slot].pending) (void)hipEventSynchronize(sh->slot[wait_slot].e1);
    for (int k = 0; k < gz_net::Shadow::kSlots; ++k) {
        gz_net::Shadow::Slot& s = sh->slot[(sh->next + k) % gz_net::Shadow::kSlots];
        if (!s.pending) continue;
        if (hipEventQuery(s.e1) != hipSuccess) break;   // (in issue order: a later one is not taken before it)
        s.pending = false;
        if (s.epoch != sh->epoch) continue;             // issued before the last reset
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, s.e0, s.e1);
        const double total = sh->done.device_ms + (double)ms;
        sh->done = *s.host;
        sh->done.device_ms = total;
    }
}
}  // namespace

extern "C" gz_net* gz_net_create(const gz_net_desc* desc, int device) {
    if (!desc) { fail("null desc"); return nullptr; }
    gz_net::Trunk in_place, s_in_place;
    gz_net* net = create_host(*desc, device, &in_place);
    if (!net) return nullptr;
    // GZ_NN_SHADOW (diagnostics): the spec and the shadow's geometry, still in front of the device
    gz_net* s = nullptr;
    int sp = 0, every = 0, max_rows = 0;
    const int env = shadow_env(&sp, &every, &max_rows);
    if (env > 0) s = shadow_host(*desc, device, sp, every, max_rows, &s_in_place);
    if (env < 0 || (env > 0 && !s)) {
        delete net;
        return nullptr;
    }
    net = create_device(net, in_place);
    if (!net) {
        delete s;
        return nullptr;
    }
    if (s && shadow_attach(net, s, s_in_place, every, max_rows, true)) {
        const std::string msg = g_err;
        gz_net_destroy(net);
        g_err = msg;
        return nullptr;
    }
    return net;
}

extern "C" size_t gz_shadow_stats_sizeof(void) { return sizeof(gz_shadow_stats); }

extern "C" int gz_net_shadow_enable(gz_net* net, int precision, int every, int max_rows) {
    if (!net) return fail("null net");
    if (net->is_shadow) return fail("shadow: a shadow cannot have a shadow of its own");
    {
        std::lock_guard<std::mutex> sl(net->shadow_mu);
        if (net->shadow) return fail("shadow: the net already has a shadow");
    }
    gz_net::Trunk in_place;
    gz_net* s = shadow_host(net->d, net->device, precision, every, max_rows, &in_place);
    if (!s) return -1;
    return shadow_attach(net, s, in_place, every, max_rows, false);
}

extern "C" int gz_net_shadow_disable(gz_net* net) {
    if (!net) return fail("null net");
    gz_net::Shadow* sh = nullptr;
    {
        std::lock_guard<std::mutex> wl(net->wmu);
        std::lock_guard<std::mutex> sl(net->shadow_mu);
        sh = net->shadow;
        net->shadow = nullptr;
    }
    if (!sh) return fail("shadow: the net has no shadow");
    HIPCHK(hipSetDevice(net->device));
    HIPCHK(hipDeviceSynchronize());   // checks still queued read the shadow's buffers
    shadow_free(sh);
    return 0;
}

extern "C" int gz_net_shadow_stats(gz_net* net, gz_shadow_stats* out, int reset) {
    if (!net || !out) return fail("null argument");
    std::lock_guard<std::mutex> sl(net->shadow_mu);
    gz_net::Shadow* sh = net->shadow;
    if (!sh) return fail("shadow: the net has no shadow");
    shadow_harvest(sh);
    *out = sh->done;
    if (reset) {
        ++sh->epoch;
        sh->fresh = true;
        sh->done = gz_shadow_stats{};
    }
    return 0;
}

extern "C" void gz_net_destroy(gz_net* net) {
    if (!net) return;
    (void)hipSetDevice(net->device);
    if (gz_net::Shadow* sh = net->shadow) {
        (void)hipDeviceSynchronize();
        if (sh->from_env) {
            shadow_harvest(sh);
            const gz_shadow_stats& t = sh->done;
            const long ok = t.rows - t.nonfinite_rows;
            fprintf(stderr,
                    "gz_nn shadow (precision %d vs %d, every %d, max_rows %d): checks %ld rows %ld nonfinite_rows %ld "
                    "max_abs_dp %.6g mean_abs_dp %.6g max_row_kl %.6g mean_row_kl %.6g argmax_mismatch %ld of %ld "
                    "max_abs_dv %.6g mean_abs_dv %.6g worst check %ld row %ld device_ms %.3f\n",
                    net_precision(net->d), net_precision(sh->net->d), sh->every, sh->max_rows, t.checks, t.rows, t.nonfinite_rows,
                    t.max_abs_dp, t.policy_elems ? t.sum_abs_dp / t.policy_elems : 0.0, t.max_row_kl,
                    t.policy_rows ? t.sum_row_kl / t.policy_rows : 0.0, t.argmax_mismatch, ok * net->d.role_count, t.max_abs_dv,
                    t.value_elems ? t.sum_abs_dv / t.value_elems : 0.0, t.worst_check, t.worst_row, t.device_ms);
        }
        net->shadow = nullptr;
        shadow_free(sh);
    }
    if (net->dmem) (void)hipFree(net->dmem);
    if (net->d_io) (void)hipFree(net->d_io);
    if (net->d_stamps) (void)hipFree(net->d_stamps);
    for (auto& f : net->feat) (void)hipFree(f.second.first);
    for (auto& f : net->resid) (void)hipFree(f.second.first);
    for (auto& f : net->glog) (void)hipFree(f.second.first);
    for (auto& f : net->fscr) (void)hipFree(f.second.first);
    for (auto& f : net->bexp) (void)hipFree(f.second);
    if (net->ev0) (void)hipEventDestroy(net->ev0);
    if (net->ev1) (void)hipEventDestroy(net->ev1);
    if (net->stream) (void)hipStreamDestroy(net->stream);
    delete net;
}

extern "C" size_t gz_net_weight_count(const gz_net* net) { return net ? net->nweights : 0; }

extern "C" int gz_net_heads_fused(const gz_net* net) { return net->large.fused_heads ? 1 : 0; }
extern "C" int gz_net_heads_path(const gz_net* net) {
    return (net->small.fused_heads ? GZ_HEADS_FUSED_SMALL : 0) | (net->large.fused_heads ? GZ_HEADS_FUSED_LARGE : 0) |
           (net->kp.heads_seq ? GZ_HEADS_SEQ : 0) | (net->gemm_heads ? GZ_HEADS_GEMM : 0) |
           (net->kp.maxP > kGemmSoftmaxMax ? GZ_HEADS_LONG_ROW : 0);
}

extern "C" double gz_net_flops_per_eval(const gz_net* net) {
    const gz_net_desc& d = net->d;   // = NetDesc.flops_per_eval (desc.py)
    const double F = d.cnn_filter_size, C = d.input_channels, HW = (double)d.input_columns * d.input_rows;
    const double k0 = initial_kernel(d);
    double f = 2 * HW * C * F * k0 * k0 + d.residual_layers * 2 * (2 * HW * F * F * 9);
    f += d.residual_layers * 2.0 * (2 * F * d.se_units);
    for (int r = 0; r < d.role_count; ++r) f += 2 * HW * F * 2 + 2 * (2 * HW) * d.policy_dist_count[r];
    f += 2 * HW * F * std::max(1, cal_layers(d)) + 2.0 * value_features(d) * d.value_hidden_size +
         2.0 * d.value_hidden_size * d.num_values;
    return f;
}

// ---- the weight image: weight_image.h's job list, run here or on the device ---------------------
namespace {
// Swaps in the device image m (laid out by I) under the lock launch_segments takes, so a launcher
// thread running a generation roll sees either the old or the new image, never a mix; the replaced
// image is freed after a device sync (launches already queued may still read it).
// (swap_image: one net's pointers, its owner's wmu held; returns the replaced image.)  A net with a
// shadow installs both nets' images in that one critical section: a launch compares two nets of one
// generation.
char* swap_image(gz_net* net, char* m, const ImageLayout& I) {
    const int R = net->d.role_count;
    char* old = net->dmem;
    net->dmem = m;
    KParams& kp = net->kp;
    kp.w0 = (const __bf16*)(m + I.w0);
    kp.w0lo = (const __bf16*)(m + I.w0lo);
    kp.b0 = (const float*)(m + I.b0);
    kp.wres = (const __bf16*)(m + I.wres);
    net->w0f = (const float*)(m + I.w0);
    net->wresf = (const float*)(m + I.wres);
    kp.bres = (const float*)(m + I.bres);
    kp.wh = (const float*)(m + I.wh);
    kp.bh = (const float*)(m + I.bh);
    kp.wcl = (const float*)(m + I.wcl);
    kp.bcl = (const float*)(m + I.bcl);
    for (int r = 0; r < R; ++r) {
        kp.pd[r] = (const float*)(m + I.pd[r]);
        kp.pb[r] = (const float*)(m + I.pb[r]);
    }
    kp.vhw = (const float*)(m + I.vhw);
    kp.vhb = (const float*)(m + I.vhb);
    kp.vdw = (const float*)(m + I.vdw);
    kp.vdb = (const float*)(m + I.vdb);
    kp.pre = (const float*)(m + I.pre);
    kp.sew1 = (const float*)(m + I.sew1);
    kp.sew2 = (const float*)(m + I.sew2);
    for (int r = 0; r < R; ++r) kp.pdp[r] = net->gemm_heads ? (const __bf16*)(m + I.pdp[r]) : nullptr;
    net->has_weights = true;
    net->image_bytes = I.total;
    return old;
}

int install_image(gz_net* net, char* m, const ImageLayout& I, char* sm = nullptr, const ImageLayout* sI = nullptr) {
    std::unique_lock<std::mutex> wl(net->wmu);
    char* old = swap_image(net, m, I);
    ++net->wepoch;
    char* sold = nullptr;
    if (sm && net->shadow) {
        sold = swap_image(net->shadow->net, sm, *sI);
    } else if (sm) {   // the shadow went away (gz_net_shadow_disable) while its image was built
        sold = sm;
    }
    wl.unlock();
    if (old || sold) {
        HIPCHK(hipDeviceSynchronize());
        if (old) HIPCHK(hipFree(old));
        if (sold) HIPCHK(hipFree(sold));
    }
    return 0;
}

// the shadow net of `net` at this moment (NULL: none)
gz_net* shadow_of(gz_net* net) {
    if (!net || net->is_shadow) return nullptr;
    std::lock_guard<std::mutex> sl(net->shadow_mu);
    return net->shadow ? net->shadow->net : nullptr;
}

int check_count(const gz_net* net, const float* blob, size_t count) {
    if (!net || !blob) return fail("null argument");
    if (count != net->nweights)
        return fail("weight count mismatch: got " + std::to_string(count) + " expected " + std::to_string(net->nweights));
    return 0;
}

// the BN folds, one workgroup each
__global__ void fold_kernel(const BNRef* folds, const float* blob, float* fold) {
    const BNRef b = folds[blockIdx.x];
    for (int i = threadIdx.x; i < b.n; i += blockDim.x) fold_element(b, i, blob, fold);
}
// the packs: job blockIdx.y, its elements grid-strided over x
__global__ void pack_kernel(const Job* jobs, const float* blob, const float* fold, char* image) {
    const Job j = jobs[blockIdx.y];
    const size_t n = j.count();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        pack_element(j.kind, j, (int)(i / j.cols), (int)(i % j.cols), blob, fold, RawImage{image});
}
}  // namespace

// One net's device image of a host blob: *m (to be installed, or freed by the caller) laid out by *I.
static int build_image_host(gz_net* net, const float* blob, size_t count, char** mp, ImageLayout* Ip) {
    if (check_count(net, blob, count)) return -1;
    const ImageLayout I = image_layout(*net);
    std::vector<char> img(I.total, 0);
    const JobList J = job_list(*net, blob_plan(net->d), I);
    if (net->f16) {   // a weight fp16 cannot hold would turn the conv's outputs non-finite
        const int conv = f16_range_check(J, blob);
        if (conv >= 0)
            return fail((conv == 0 ? std::string("initial conv") : "trunk conv " + std::to_string(conv - 1) + " (residual block " +
                                                                     std::to_string((conv - 1) / 2) + ")") +
                        ": a BN-folded weight is outside fp16's finite range (|w| >= 65,520): fp16x3-layered cannot hold it");
    }
    pack_image_host(J, blob, RawImage{img.data()});
    HIPCHK(hipSetDevice(net->device));
    char* m = nullptr;
    HIPCHK(hipMalloc((void**)&m, I.total));
    if (hipMemcpy(m, img.data(), I.total, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(m);
        return fail("weight upload failed");
    }
    *mp = m;
    *Ip = I;
    return 0;
}

extern "C" int gz_net_set_weights(gz_net* net, const float* blob, size_t count) {
    char *m = nullptr, *sm = nullptr;
    ImageLayout I, sI;
    if (build_image_host(net, blob, count, &m, &I)) return -1;
    if (gz_net* s = shadow_of(net)) {   // both nets take the blob, or neither
        if (build_image_host(s, blob, count, &sm, &sI)) {
            (void)hipFree(m);
            return fail("shadow: " + g_err);
        }
    }
    return install_image(net, m, I, sm, &sI);
}

// The same jobs on the device (generation roll: the blob arrives in HBM by an RCCL broadcast), the
// element functions computing every value with the host's operations and rounding.
// fp16x3-layered: the blob's BN-folded conv weights must lie within fp16's finite range (a
// precondition here, checked by gz_net_set_weights only): a larger one becomes an infinite hi part
// and non-finite outputs; nothing is clamped.
static int build_image_device(gz_net* net, const float* d_blob, size_t count, char** mp, ImageLayout* Ip) {
    const ImageLayout I = image_layout(*net);
    const JobList J = job_list(*net, blob_plan(net->d), I);
    HIPCHK(hipSetDevice(net->device));
    // The blob's producer (an RCCL broadcast, a copy on torch's stream, ...) ran on some other
    // stream: net->stream is non-blocking, so nothing orders the fold / pack kernels after it.  Wait
    // for all work issued to the device so far (a roll is rare; the runner applies it between
    // launches, whose in-flight ones gz_net_set_weights waits for anyway).
    HIPCHK(hipDeviceSynchronize());
    hipStream_t st = net->stream;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, st));
    char* m = nullptr;
    char* scratch = nullptr;   // the fold buffer, then the two job arrays
    auto cleanup = [&]() {
        if (scratch) (void)hipFree(scratch);
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    };
    auto bail = [&](const std::string& what, hipError_t e) {
        cleanup();
        if (m) (void)hipFree(m);
        return fail(what + ": " + hipGetErrorString(e));
    };
    const size_t fold_bytes = ((size_t)J.fold_floats * 4 + 15) & ~(size_t)15;
    const size_t folds_bytes = (J.folds.size() * sizeof(BNRef) + 15) & ~(size_t)15, packs_bytes = J.packs.size() * sizeof(Job);
    hipError_t e;
    if ((e = hipMalloc((void**)&m, I.total)) != hipSuccess) return bail("hipMalloc image", e);
    if ((e = hipMalloc((void**)&scratch, fold_bytes + folds_bytes + packs_bytes)) != hipSuccess) return bail("hipMalloc jobs", e);
    float* fold = (float*)scratch;
    BNRef* folds_d = (BNRef*)(scratch + fold_bytes);
    Job* packs_d = (Job*)(scratch + fold_bytes + folds_bytes);
    if ((e = hipMemsetAsync(m, 0, I.total, st)) != hipSuccess) return bail("hipMemsetAsync", e);
    if ((e = hipMemcpyAsync(folds_d, J.folds.data(), J.folds.size() * sizeof(BNRef), hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = hipMemcpyAsync(packs_d, J.packs.data(), packs_bytes, hipMemcpyHostToDevice, st)) != hipSuccess)
        return bail("jobs", e);
    size_t most = 1;
    for (const Job& j : J.packs) most = std::max(most, j.count());
    hipLaunchKernelGGL(fold_kernel, dim3((unsigned)J.folds.size()), dim3(256), 0, st, folds_d, d_blob, fold);
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)std::min<size_t>((most + 255) / 256, 4096), (unsigned)J.packs.size()), dim3(256),
                       0, st, packs_d, d_blob, fold, m);
    if ((e = hipGetLastError()) != hipSuccess) return bail("pack kernels", e);
    if ((e = hipEventRecord(e1, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess) return bail("roll sync", e);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    net->last_roll_ms = ms;
    cleanup();
    *mp = m;
    *Ip = I;
    return 0;
}

extern "C" int gz_net_set_weights_device(gz_net* net, const float* d_blob, size_t count) {
    if (check_count(net, d_blob, count)) return -1;
    if (getenv("GZ_HOST_WEIGHT_ROLL")) {   // diagnostics: the round-trip path (D2H, host fold / pack, H2D)
        std::vector<float> h(count);
        HIPCHK(hipSetDevice(net->device));
        HIPCHK(hipMemcpy(h.data(), d_blob, count * 4, hipMemcpyDeviceToHost));
        return gz_net_set_weights(net, h.data(), count);
    }
    char *m = nullptr, *sm = nullptr;
    ImageLayout I, sI;
    if (build_image_device(net, d_blob, count, &m, &I)) return -1;
    if (gz_net* s = shadow_of(net)) {   // both nets take the blob, or neither
        if (build_image_device(s, d_blob, count, &sm, &sI)) {
            (void)hipFree(m);
            return fail("shadow: " + g_err);
        }
    }
    return install_image(net, m, I, sm, &sI);
}


extern "C" double gz_net_last_roll_ms(const gz_net* net) { return net ? (double)net->last_roll_ms : -1.0; }

// diagnostics: the device weight image (out == NULL: its size)
extern "C" size_t gz_net_copy_weight_image(gz_net* net, void* out, size_t cap) {
    if (!net || !net->dmem) return 0;
    std::lock_guard<std::mutex> wl(net->wmu);
    if (!out) return net->image_bytes;
    const size_t n = std::min(cap, net->image_bytes);
    if (hipSetDevice(net->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(out, net->dmem, n, hipMemcpyDeviceToHost) != hipSuccess)
        return 0;
    return n;
}

// One net's forward, queued on `stream`; *rows = the launch's rows.  The caller holds the wmu that
// guards the net's weight pointers (its own, or its owner's for a shadow).
static int launch_net(gz_net* net, hipStream_t stream, const gz_segment* segs, int nseg, hipEvent_t mid, int* rows) {
    *rows = 0;
    if (nseg < 1 || nseg > kMaxSegments) return fail("segment count out of range (1.." + std::to_string(kMaxSegments) + ")");
    if (!net->has_weights) return fail("weights not set");
    KParams kp = net->kp;
    int n = 0;
    for (int i = 0; i < nseg; ++i) {
        if (segs[i].rows < 0) return fail("negative segment rows");
        Segment& g = kp.seg[i];
        g.row0 = n;
        g.planes = segs[i].planes;
        for (int r = 0; r < kp.R; ++r) g.pol[r] = segs[i].policies[r];
        g.val = segs[i].values;
        n += segs[i].rows;
    }
    if (n <= 0) return 0;
    *rows = n;
    kp.n = n;
    kp.nseg = nseg;
    kp.stamps = net->stamps_on ? net->d_stamps : nullptr;
    {   // head-feature scratch of this stream (grown with a device sync: rare, sizes only increase)
        std::lock_guard<std::mutex> lk(net->feat_mu);
        auto& f = net->feat[stream];
        if (f.second < n) {
            if (f.first) {
                HIPCHK(hipDeviceSynchronize());
                HIPCHK(hipFree(f.first));
                f.first = nullptr;
            }
            const int cap = std::max(n, 8192);
            HIPCHK(hipMalloc((void**)&f.first, (size_t)cap * kp.FS * sizeof(float)));
            f.second = cap;
        }
        kp.feat = f.first;
        kp.glog = nullptr;
        if (net->gemm_heads) {
            auto& g = net->glog[stream];
            if (g.second < n) {
                if (g.first) {
                    HIPCHK(hipDeviceSynchronize());
                    HIPCHK(hipFree(g.first));
                    g.first = nullptr;
                }
                const int cap = std::max(n, 8192);
                HIPCHK(hipMalloc((void**)&g.first, (size_t)cap * kp.plog * sizeof(float)));
                g.second = cap;
            }
            kp.glog = g.first;
        }
    }
    if (net->fp32 || net->layered) {
        // the layer-wise trunk (fp32_forward.hip), then the heads: fp32-ieee's kernel with blocked Dense
        // sums (fp16x3-layered's too), the bf16 layered modes' as after a single-image bf16 / bf16x3 trunk
        gzfp32::Forward f;
        f.parts = net->layered;
        if (net->fp32) {
            f.w0 = net->w0f;
            f.wres = net->wresf;
        }
        f.CP = net->in_width();
        f.FP = net->fpad;
        f.chunk_rows = net->chunk_rows;
        {   // this stream's activation scratch (grown with a device sync: rare, sizes only increase)
            std::lock_guard<std::mutex> lk(net->feat_mu);
            auto& s = net->fscr[stream];
            const int need = std::min(n, net->chunk_rows);
            if (s.second < need) {
                if (s.first) {
                    HIPCHK(hipDeviceSynchronize());
                    HIPCHK(hipFree(s.first));
                    s.first = nullptr;
                    s.second = 0;
                }
                const int cap = std::max(need, std::min(net->chunk_rows, 64));
                HIPCHK(hipMalloc((void**)&s.first, gzfp32::scratch_layout(cap, kp.npos, f.CP, f.FP).total));
                s.second = cap;
                if (net->f16) {   // (the sync above, if any, covers the launches that read the old one)
                    int*& be = net->bexp[stream];
                    if (be) HIPCHK(hipFree(be));
                    be = nullptr;
                    HIPCHK(hipMalloc((void**)&be, (size_t)cap * sizeof(int)));
                }
            }
            if (net->f16) f.bexp = net->bexp[stream];
            f.scratch = s.first;
            f.scratch_rows = s.second;
            f.scratch_bytes = gzfp32::scratch_layout(s.second, kp.npos, f.CP, f.FP).total;
        }
        if (f.scratch_bytes > gzfp32::kScratchMax) return fail("internal: fp32 scratch over its limit");
        if (const char* e = gzfp32::forward(kp, f, stream)) return fail(e);
        if (mid) HIPCHK(hipEventRecord(mid, stream));
        void* hargs[] = {&kp};
        if (net->gemm_heads) {
            int maxjt = 0;
            for (int r = 0; r < kp.R; ++r) maxjt = std::max(maxjt, (kp.P[r] + 15) / 16);
            HIPCHK(hipLaunchKernel((const void*)&policy_gemm_kernel, dim3((n + 63) / 64, (maxjt + 7) / 8, kp.R), dim3(256),
                                   hargs, 0, stream));
        }
        HIPCHK(hipLaunchKernel(net->fp32 || net->f16 ? (const void*)&heads_kernel_blocked : (const void*)&heads_kernel,
                               dim3((n + kHeadBoards - 1) / kHeadBoards), dim3(256), hargs, net->heads_smem, stream));
        return 0;
    }
    const gz_net::Trunk& t = n >= net->large_min_rows ? net->large : net->small;
    kp.resid = nullptr;
    if (t.resid_bytes) {
        std::lock_guard<std::mutex> lk(net->feat_mu);
        auto& f = net->resid[stream];
        const size_t need = (size_t)((n + t.nb - 1) / t.nb) * t.resid_bytes;
        if (f.second < need) {
            if (f.first) {
                HIPCHK(hipDeviceSynchronize());
                HIPCHK(hipFree(f.first));
                f.first = nullptr;
            }
            const size_t cap = std::max(need, (size_t)1024 * t.resid_bytes);
            HIPCHK(hipMalloc((void**)&f.first, cap));
            f.second = cap;
        }
        kp.resid = (f32x4*)f.first;
    }
    kp.btab_off = t.btab_off;
    kp.se_off = t.se_off;
    kp.cal_off = t.cal_off;
    void* args[] = {&kp};
    HIPCHK(hipLaunchKernel(t.fn, dim3((n + t.nb - 1) / t.nb), dim3(t.threads), args, t.smem, stream));
    if (mid) HIPCHK(hipEventRecord(mid, stream));
    if (net->gemm_heads) {
        int maxjt = 0;
        for (int r = 0; r < kp.R; ++r) maxjt = std::max(maxjt, (kp.P[r] + 15) / 16);
        HIPCHK(hipLaunchKernel((const void*)&policy_gemm_kernel, dim3((n + 63) / 64, (maxjt + 7) / 8, kp.R), dim3(256),
                               args, 0, stream));
    }
    if (!t.fused_heads)
        HIPCHK(hipLaunchKernel((const void*)&heads_kernel, dim3((n + kHeadBoards - 1) / kHeadBoards), dim3(256), args,
                               net->heads_smem, stream));
    return 0;
}

// The shadow check of a launch of n rows just queued on `stream` (net->wmu held): the first
// min(n, max_rows) rows through the shadow net into its own buffer, the comparison against the
// outputs `segs` point to, and an asynchronous snapshot of the totals into the ring.
static int shadow_check(gz_net* net, hipStream_t stream, const gz_segment* segs, int nseg, int n) {
    std::lock_guard<std::mutex> sl(net->shadow_mu);
    gz_net::Shadow* sh = net->shadow;
    const long index = sh->forwards++;
    gz_net* s = sh->net;
    if (index % sh->every != 0 || !s->has_weights) return 0;
    const gz_net_desc& d = net->d;
    const int R = d.role_count, V = d.num_values, k = std::min(n, sh->max_rows);
    size_t out_f = V;
    for (int r = 0; r < R; ++r) out_f += d.policy_dist_count[r];
    gz_net::Shadow::Out& o = sh->out[stream];
    if (!o.out) {   // this stream's outputs [max_rows][sum P_r + V], then its row records
        const size_t out_bytes = ((size_t)sh->max_rows * out_f * sizeof(float) + 15) & ~(size_t)15;
        HIPCHK(hipMalloc((void**)&o.out, out_bytes + (size_t)sh->max_rows * sizeof(gzshadow::RowRecord)));
        o.rec = (gzshadow::RowRecord*)((char*)o.out + out_bytes);
    }
    shadow_harvest(sh);
    gz_net::Shadow::Slot& slot = sh->slot[sh->next];
    if (slot.pending) shadow_harvest(sh, sh->next);   // the ring is full: wait for its oldest check
    // the totals block has one writer at a time: a check on another stream follows the last one
    if (sh->last_slot >= 0 && sh->last_stream != stream && sh->slot[sh->last_slot].pending)
        HIPCHK(hipStreamWaitEvent(stream, sh->slot[sh->last_slot].e1, 0));
    HIPCHK(hipEventRecord(slot.e0, stream));
    // the truncated segment list: the net's planes, the shadow's buffer; the same rows of the net's outputs
    gz_segment ss[GZ_MAX_SEGMENTS];
    gzshadow::CompareArgs ca{};
    float* pol_b[GZ_MAX_ROLES];
    float* p = o.out;
    for (int r = 0; r < R; ++r) {
        pol_b[r] = p;
        p += (size_t)sh->max_rows * d.policy_dist_count[r];
        ca.pol_b[r] = pol_b[r];
        ca.P[r] = d.policy_dist_count[r];
    }
    ca.val_b = p;
    int m = 0, row0 = 0;
    for (int i = 0; i < nseg && row0 < k; ++i) {
        if (segs[i].rows <= 0) continue;
        gz_segment& g = ss[m];
        g = segs[i];
        g.rows = std::min(segs[i].rows, k - row0);
        ca.seg[m].row0 = row0;
        for (int r = 0; r < R; ++r) {
            ca.seg[m].pol[r] = segs[i].policies[r];
            g.policies[r] = pol_b[r] + (size_t)row0 * d.policy_dist_count[r];
        }
        ca.seg[m].val = segs[i].values;
        g.values = p + (size_t)row0 * V;
        row0 += g.rows;
        ++m;
    }
    int srows = 0;
    if (launch_net(s, stream, ss, m, nullptr, &srows)) return fail("shadow: " + g_err);
    ca.nseg = m;
    ca.n = k;
    ca.R = R;
    ca.V = V;
    ca.logits = net->kp.logits;
    ca.rec = o.rec;
    if (const char* e = gzshadow::launch_compare(ca, index, sh->fresh ? 1 : 0, sh->d_acc, stream)) return fail(std::string("shadow: ") + e);
    sh->fresh = false;
    HIPCHK(hipMemcpyAsync(slot.host, sh->d_acc, sizeof(gz_shadow_stats), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipEventRecord(slot.e1, stream));
    slot.pending = true;
    slot.epoch = sh->epoch;
    sh->last_slot = sh->next;
    sh->last_stream = stream;
    sh->next = (sh->next + 1) % gz_net::Shadow::kSlots;
    return 0;
}

// `end` (may be NULL) is recorded after the net's own launches, before a shadow check's.
static int launch_segments(gz_net* net, hipStream_t stream, const gz_segment* segs, int nseg,
                           hipEvent_t mid = nullptr, hipEvent_t end = nullptr, unsigned long long* epoch = nullptr) {
    // the weight image stays valid until this launch is queued (gz_net_set_weights frees a replaced
    // image only after a device sync)
    std::lock_guard<std::mutex> wl(net->wmu);
    if (epoch) *epoch = net->wepoch;
    int n = 0;
    if (launch_net(net, stream, segs, nseg, mid, &n)) return -1;
    if (end) HIPCHK(hipEventRecord(end, stream));
    if (n > 0 && net->shadow) return shadow_check(net, stream, segs, nseg, n);
    return 0;
}

static int launch(gz_net* net, hipStream_t stream, const float* d_planes, int n,
                  float* const* d_pol, float* d_val, hipEvent_t end = nullptr) {
    gz_segment sg{};
    sg.rows = n;
    sg.planes = d_planes;
    for (int r = 0; r < net->kp.R; ++r) sg.policies[r] = d_pol[r];
    sg.values = d_val;
    return launch_segments(net, stream, &sg, 1, nullptr, end);
}

extern "C" int gz_net_forward_device(gz_net* net, void* stream, const float* d_planes, int n,
                                     float* const* d_policies, float* d_values) {
    if (!net) return fail("null net");
    return launch(net, (hipStream_t)stream, d_planes, n, d_policies, d_values);
}

extern "C" int gz_net_forward_segments(gz_net* net, void* stream, const gz_segment* segs, int nseg) {
    if (!net || !segs) return fail("null argument");
    return launch_segments(net, (hipStream_t)stream, segs, nseg);
}

extern "C" int gz_net_forward_segments_ev(gz_net* net, void* stream, const gz_segment* segs, int nseg,
                                          void* trunk_done_event) {
    if (!net || !segs) return fail("null argument");
    return launch_segments(net, (hipStream_t)stream, segs, nseg, (hipEvent_t)trunk_done_event);
}

extern "C" int gz_net_forward(gz_net* net, const float* planes, int n, float* const* policies, float* values) {
    if (!net || !planes || !policies || !values) return fail("null argument");
    if (n <= 0) return 0;
    const gz_net_desc& d = net->d;
    const size_t in_f = (size_t)d.input_channels * d.input_columns * d.input_rows;
    size_t out_f = d.num_values;
    for (int r = 0; r < d.role_count; ++r) out_f += d.policy_dist_count[r];
    HIPCHK(hipSetDevice(net->device));
    if (n > net->io_cap) {
        if (net->d_io) HIPCHK(hipFree(net->d_io));
        net->d_io = nullptr;
        HIPCHK(hipMalloc((void**)&net->d_io, (size_t)n * (in_f + out_f) * 4 + 1024));
        net->io_cap = n;
    }
    float* d_in = net->d_io;
    float* d_pol[GZ_MAX_ROLES];
    float* p = d_in + (size_t)n * in_f;
    for (int r = 0; r < d.role_count; ++r) { d_pol[r] = p; p += (size_t)n * d.policy_dist_count[r]; }
    float* d_val = p;
    HIPCHK(hipMemcpyAsync(d_in, planes, (size_t)n * in_f * 4, hipMemcpyHostToDevice, net->stream));
    const bool stamps = getenv("GZ_KERNEL_STAMPS") != nullptr;
    const int grid = n;   // >= workgroups of either trunk variant
    if (stamps && grid > net->stamp_cap) {
        if (net->d_stamps) HIPCHK(hipFree(net->d_stamps));
        HIPCHK(hipMalloc((void**)&net->d_stamps, (size_t)grid * 8 * sizeof(unsigned long long)));
        net->stamp_cap = grid;
    }
    if (stamps) HIPCHK(hipMemsetAsync(net->d_stamps, 0, (size_t)grid * 8 * sizeof(unsigned long long), net->stream));
    HIPCHK(hipEventRecord(net->ev0, net->stream));
    net->stamps_on = stamps;
    // (ev1 follows the net's own launches: a shadow check's work comes after it and is not timed here)
    const int lrc = launch(net, net->stream, d_in, n, d_pol, d_val, net->ev1);
    net->stamps_on = false;
    if (lrc) return -1;
    for (int r = 0; r < d.role_count; ++r)
        HIPCHK(hipMemcpyAsync(policies[r], d_pol[r], (size_t)n * d.policy_dist_count[r] * 4, hipMemcpyDeviceToHost, net->stream));
    HIPCHK(hipMemcpyAsync(values, d_val, (size_t)n * d.num_values * 4, hipMemcpyDeviceToHost, net->stream));
    HIPCHK(hipStreamSynchronize(net->stream));
    HIPCHK(hipEventElapsedTime(&net->last_ms, net->ev0, net->ev1));
    if (stamps) {
        std::vector<unsigned long long> h((size_t)grid * 8);
        HIPCHK(hipMemcpy(h.data(), net->d_stamps, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        // the launch ran ceil(n / NB) workgroups: average over the ones that stamped
        for (int i = 0; i < 8; ++i) net->stamp_avg[i] = 0;
        int wgs = 0;
        for (int b = 0; b < grid; ++b) {
            if (h[(size_t)b * 8] == 0 || h[(size_t)b * 8 + 4] == 0) continue;
            ++wgs;
            for (int i = 1; i < 5; ++i) net->stamp_avg[i] += (double)(h[(size_t)b * 8 + i] - h[(size_t)b * 8 + i - 1]);
        }
        for (int i = 1; i < 5; ++i) net->stamp_avg[i] = wgs ? net->stamp_avg[i] / wgs : 0.0;
        net->stamp_avg[0] = wgs;
    }
    return 0;
}

extern "C" int gz_net_stamp_avg(const gz_net* net, double* out8) {
    if (net && (net->fp32 || net->layered))
        return fail("no kernel stamps in the fp32-ieee and layered modes (the trunk is many launches)");
    for (int i = 0; i < 8; ++i) out8[i] = net->stamp_avg[i];
    return 0;
}

extern "C" float gz_net_last_kernel_ms(const gz_net* net) { return net ? net->last_ms : 0.f; }

extern "C" int gz_net_set_output_logits(gz_net* net, int on) {
    if (!net) return fail("null net");
    std::lock_guard<std::mutex> wl(net->wmu);
    if (net->kp.logits != (on ? 1 : 0)) ++net->wepoch;   // stored outputs are what the forward wrote
    net->kp.logits = on ? 1 : 0;
    if (net->shadow) net->shadow->net->kp.logits = net->kp.logits;
    return 0;
}

// what symmetry.hip (the symmetry ensemble's entry points) may know of a net
void gzsym::net_view(gz_net* net, gzsym::NetView* out) {
    std::lock_guard<std::mutex> wl(net->wmu);
    const gz_net_desc& d = net->d;
    out->device = net->device;
    out->plane_elems = d.input_channels * d.input_columns * d.input_rows;
    out->roles = d.role_count;
    out->num_values = d.num_values;
    for (int r = 0; r < GZ_MAX_ROLES; ++r) out->policy[r] = r < d.role_count ? d.policy_dist_count[r] : 0;
    out->logits = net->kp.logits;
    out->host_stream = net->stream;
}

int gzsym::set_error(const std::string& msg) { return fail(msg); }

// what eval_cache.hip (the evaluation cache) needs beyond that
unsigned long long gzcache::net_epoch(gz_net* net) {
    std::lock_guard<std::mutex> wl(net->wmu);
    return net->wepoch;
}

int gzcache::forward_segments_epoch(gz_net* net, void* stream, const gz_segment* segs, int nseg, unsigned long long* epoch) {
    return launch_segments(net, (hipStream_t)stream, segs, nseg, nullptr, nullptr, epoch);
}

extern "C" int gz_nn_compare_outputs(int device, int n, int roles, const int* policy_sizes, int num_values,
                                     const float* const* pol_a, const float* val_a, const float* const* pol_b,
                                     const float* val_b, gz_shadow_stats* out) {
    if (!policy_sizes || !pol_a || !val_a || !pol_b || !val_b || !out) return fail("null argument");
    if (n < 1 || roles < 1 || roles > GZ_MAX_ROLES || num_values < 1 || num_values > 4) return fail("compare: sizes out of range");
    size_t row_f = num_values;
    for (int r = 0; r < roles; ++r) {
        if (policy_sizes[r] < 1 || !pol_a[r] || !pol_b[r]) return fail("compare: bad policy array");
        row_f += policy_sizes[r];
    }
    HIPCHK(hipSetDevice(device));
    // one allocation: a's arrays, b's arrays, the records, the block
    const size_t side = ((size_t)n * row_f * sizeof(float) + 15) & ~(size_t)15;
    const size_t recs = (size_t)n * sizeof(gzshadow::RowRecord);
    char* mem = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipMalloc((void**)&mem, 2 * side + recs + sizeof(gz_shadow_stats));
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    gzshadow::CompareArgs ca{};
    ca.nseg = 1;
    ca.n = n;
    ca.R = roles;
    ca.V = num_values;
    ca.rec = (gzshadow::RowRecord*)(mem + 2 * side);
    gz_shadow_stats* d_acc = (gz_shadow_stats*)(mem + 2 * side + recs);
    const char* cmp_err = nullptr;
    if (e == hipSuccess) {
        for (int sd = 0; sd < 2 && e == hipSuccess; ++sd) {
            float* p = (float*)(mem + sd * side);
            for (int r = 0; r < roles && e == hipSuccess; ++r) {
                const size_t cnt = (size_t)n * policy_sizes[r];
                e = hipMemcpyAsync(p, (sd ? pol_b : pol_a)[r], cnt * sizeof(float), hipMemcpyHostToDevice, st);
                if (sd) ca.pol_b[r] = p; else ca.seg[0].pol[r] = p;
                ca.P[r] = policy_sizes[r];
                p += cnt;
            }
            if (e == hipSuccess) e = hipMemcpyAsync(p, sd ? val_b : val_a, (size_t)n * num_values * sizeof(float), hipMemcpyHostToDevice, st);
            if (sd) ca.val_b = p; else ca.seg[0].val = p;
        }
        if (e == hipSuccess) e = hipEventRecord(e0, st);
        if (e == hipSuccess) cmp_err = gzshadow::launch_compare(ca, 0, 1, d_acc, st);
        if (e == hipSuccess && !cmp_err) e = hipEventRecord(e1, st);
        if (e == hipSuccess && !cmp_err) e = hipMemcpyAsync(out, d_acc, sizeof(gz_shadow_stats), hipMemcpyDeviceToHost, st);
        const hipError_t es = hipStreamSynchronize(st);   // (also after a failure: the uploads read the caller's arrays)
        if (e == hipSuccess) e = es;
        float ms = 0.f;
        if (e == hipSuccess && !cmp_err) e = hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess && !cmp_err) out->device_ms = ms;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (st) (void)hipStreamDestroy(st);
    if (mem) (void)hipFree(mem);
    if (cmp_err) return fail(cmp_err);
    if (e != hipSuccess) return fail(std::string("gz_nn_compare_outputs: ") + hipGetErrorString(e));
    return 0;
}

extern "C" int gz_net_large_min_rows(const gz_net* net) { return net ? net->large_min_rows : 0; }

extern "C" const char* gz_net_kernel_name(const gz_net* net, int large) {
    if (!net) return "";
    return (large ? net->large : net->small).name.c_str();
}

extern "C" int gz_net_wave_rows(const gz_net* net) {
    if (!net) return 0;
    if (net->fp32 || net->layered) {   // rows whose conv grid is one workgroup per CU
        const int gy = net->fpad / (32 * gzfp32::wave_co_tiles(net->fpad));
        return std::max(1, (kCUs / gy) * gzfp32::kTileCols / net->kp.npos);
    }
    const gz_net::Trunk& t = net->large_min_rows < (1 << 30) ? net->large : net->small;
    return t.nb * t.wgs_per_cu * kCUs;
}

extern "C" int gz_net_workgroups_per_cu(const gz_net* net) {
    if (!net || net->fp32 || net->layered) return 1;
    return (net->large_min_rows < (1 << 30) ? net->large : net->small).wgs_per_cu;
}
