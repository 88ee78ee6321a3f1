/* gzero_nn.h -- C-ABI of the MI355X policy/value network forward (libgz_nn.so).
 *
 * Replaces, for the self-play hot path, the Keras model the reference runs through
 *   NeuralNetwork.get_model().predict_on_batch(X)      src/ggpzero/util/cppinterface.py:119
 * built by get_network_model()                          src/ggpzero/nn/model.py:154-296 (v1 path)
 * and loaded by Manager.load_network / create_new_network   src/ggpzero/nn/manager.py:96-139.
 *
 * All entry points take plain pointers and sizes.  Every function returning int returns 0 on
 * success and a negative code on failure; gz_nn_last_error() then holds a message (thread-local).
 */
#ifndef GZERO_NN_H
#define GZERO_NN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GZ_MAX_ROLES 4

/* Mirror of the forward-relevant fields of confs.NNModelConfig (src/ggpzero/defs/confs.py:127-151)
 * plus GenerationDescription.draw_head (num_values 3) and the Flatten data_format of the model
 * file. */
typedef struct gz_net_desc {
    int input_channels;                       /* C                                  */
    int input_columns;                        /* H = len(y_cords)  (bases.py:115)   */
    int input_rows;                           /* W = len(x_cords)  (bases.py:111)   */
    int cnn_filter_size;                      /* F                                  */
    int cnn_kernel_size;                      /* must be 3                          */
    int residual_layers;                      /* B                                  */
    int role_count;                           /* R = number of policy heads         */
    int policy_dist_count[GZ_MAX_ROLES];      /* P_r                                */
    int value_hidden_size;
    int num_values;                           /* 2, or 3 with a draw head           */
    int leaky_relu;                           /* 0: relu, 1: LeakyReLU(alpha=0.03)  */
    int flatten_nchw;                         /* 0: Keras>=2.1.6 (H,W,C) flatten; 1: legacy (C,H,W) */
    /* legacy v1 model files (data/breakthrough/models/x6_102.json, keras 2.1.3): */
    int conv_bias;                            /* every Conv2D has use_bias: a bias after each kernel */
    int value_bn;                             /* BatchNormalization after the value head's 1x1 conv  */
    int value_sigmoid;                        /* value Dense activation sigmoid (else softmax)      */
    /* Arithmetic of the residual trunk (build extension; the reference runs fp32 TF kernels):
     *   GZ_PRECISION_BF16 (0 or 1): bf16 operands, fp32 accumulation and residual stream;
     *   GZ_PRECISION_SPLIT (3): each fp32 operand as bf16 hi + bf16 lo and each product as
     *   hi*hi + hi*lo + lo*hi on the MFMA (~16 significant bits per operand against fp32's 24, fp32
     *   accumulation: pre-softmax logits within ~1e-4 relative of an fp32 forward, the per-config
     *   bounds of nn/tolerance.py); F <= 128 on boards <= 64 positions two per workgroup, larger
     *   boards (up to 19 x 19) one per workgroup, by two passes per conv where the hi + lo image
     *   exceeds the LDS (F = 256 on 13 x 13, F = 128 on 19 x 19; v2 nets with F = 256 also on
     *   8 x 8).  F = 256 (any filter count from 129 up, padded), v1 and v2, runs on boards of up
     *   to 176 positions (13 x 13) in both modes, as deep as the image, the bias table (2,048
     *   bytes per residual block) and the squeeze-excite / concat_all_layers scratch fit the
     *   160 KB of LDS -- 13 blocks on 13 x 13 (12 with squeeze-excite), 20 on 10 x 10 in the split
     *   mode, 37 in bf16; gz_net_create refuses a deeper net before any device call
     *   ("network needs ... B of LDS").  The heads' 1x1 convs, softmaxes and value MLP are
     *   fp32 in both modes; the policy Dense is fp32 except for single-image nets with a policy of
     *   >= 512 moves (amazons), whose policy Dense of the whole launch runs as one bf16x3 split MFMA
     *   GEMM in both modes (policy_gemm_kernel; GZ_NO_GEMM_HEADS=1 keeps it fp32 on the VALU).
     *   GZ_PRECISION_FP32 (4): IEEE fp32, the reference's arithmetic -- every conv on the f32-input
     *   MFMA (v_mfma_f32_16x16x4_f32: f32 operands, f32 accumulation, a k-ordered fmaf chain), BN
     *   folded in fp32, fp32 activations.  The trunk runs layer by layer through a device scratch
     *   (no LDS-image limit: every board up to 19 x 19 with F <= 256, v1 and v2 with up to 128
     *   squeeze-excite units, any depth), large launches in
     *   sequential row chunks; the heads kernel follows and the policy Dense is always fp32.  About
     *   16/3 of the split mode's MFMA time: for match play, gating and numerics checks, not for
     *   self-play throughput.  Every row's outputs are bit-identical whatever the launch.
     *   Stated error per config: galvanise_zero_amd/nn/tolerance.py.
     *   GZ_PRECISION_BF16_LAYERED (5) / GZ_PRECISION_SPLIT_LAYERED (6): the arithmetic of
     *   GZ_PRECISION_BF16 / GZ_PRECISION_SPLIT for the nets those modes refuse.  The trunk runs layer
     *   by layer through GZ_PRECISION_FP32's device scratch (fp32 activations, the same
     *   squeeze-excite, pooling and head-feature kernels), its convs on v_mfma_f32_16x16x32_bf16
     *   with the activations converted to bf16 (split: to bf16 hi + lo, three MFMAs per product) as
     *   they are staged into the LDS; the weight image is the fused mode's, byte for byte.  No
     *   LDS-image limit: every board up to 19 x 19 with F <= 256 at any depth, v1 and v2 with up to
     *   128 squeeze-excite units, every value head.  The heads run as after a single-image fused
     *   trunk (policy_gemm_kernel for policies of >= 512 moves, then the fp32 heads kernel).  Slower
     *   than the fused modes where those run (the activations cross HBM between layers), so
     *   opt-in; every row's outputs are bit-identical whatever the launch.
     *   GZ_PRECISION_F16X3_LAYERED (7): fp32-class arithmetic at the bf16 MFMA's rate, on the same
     *   layer-by-layer trunk.  Each operand is an fp16 hi part plus an fp16 lo part scaled by 2^11
     *   (22 significand bits against fp32's 24), three v_mfma_f32_16x16x32_f16 per product (hi hi
     *   into one fp32 accumulator, hi lo + lo hi into a second, joined as main + corr 2^-11).  fp16's
     *   range is kept by one power-of-two exponent per board and conv input (board_exp_kernel: the
     *   board's largest |x| scaled into [2^14, 2^15)), a function of the board's own data, so every
     *   row's outputs stay bit-identical whatever the launch.  Geometry limits as modes 5 / 6; the
     *   heads run as in GZ_PRECISION_FP32 (policy Dense fp32 on the VALU).  A BN-folded conv weight
     *   of 65,520 or more in magnitude does not fit fp16: gz_net_set_weights refuses such a blob
     *   naming the conv; gz_net_set_weights_device requires the caller to rule it out (the weight
     *   becomes infinite and the outputs non-finite, nothing is clamped).  For match play, gating
     *   and numerics checks; GZ_PRECISION_FP32 stays the IEEE reference. */
    int precision;
    /* v2 (pre-activation) trunk, model.py:78-151 (the reference's features=True templates and its
     * non-legacy model files); all zero = v1. */
    int resnet_v2;                            /* blocks BN-act-conv-BN-act-conv [SE], add, no act    */
    int initial_kernel;                       /* 1 or 3; 0 = model.py's (1 for v2, 3 for v1)        */
    int initial_bn;                           /* v2: BN + act after the initial conv (0: bare conv)  */
    int se_units;                             /* squeeze-excite compress units, 0 = none (<= 128)    */
    int global_pooling_value;                 /* value features = [trunk channel means (F), conv (HW)] */
    /* v2 only, model.py:251-260: the value head reads every trunk layer (the initial conv block's
     * output and each residual block's add), each through its own 1x1 conv + BN + act: (B + 1) HW
     * features in layer order.  Such nets run the dense heads in a separate heads launch. */
    int concat_all_layers;
} gz_net_desc;

#define GZ_PRECISION_BF16 1
#define GZ_PRECISION_SPLIT 3
#define GZ_PRECISION_FP32 4
#define GZ_PRECISION_BF16_LAYERED 5
#define GZ_PRECISION_SPLIT_LAYERED 6
#define GZ_PRECISION_F16X3_LAYERED 7

typedef struct gz_net gz_net;

/* Create a network on HIP device `device`.  Returns NULL on error (see gz_nn_last_error). */
gz_net* gz_net_create(const gz_net_desc* desc, int device);
void gz_net_destroy(gz_net* net);

/* Number of float32 values of the canonical weight blob (layout: galvanise_zero_amd/nn/desc.py
 * weight_spec(): Keras storage order, conv HWIO, BN as gamma,beta,mean,var, dense [in][out]). */
size_t gz_net_weight_count(const gz_net* net);

/* Upload weights from a host float32 blob (BN folded + packed to bf16 on the host).  Safe while a
 * runner is launching on this net (generation roll): launches issued after the call use the new
 * weights, launches already in flight finish on the old ones, which are freed after a device sync. */
int gz_net_set_weights(gz_net* net, const float* blob, size_t count);

/* Upload weights from a *device* float32 blob (e.g. after an RCCL broadcast into device memory): the
 * BN fold and the bf16 (hi / lo) packing run as HIP kernels reading the blob in place -- no PCIe
 * round trip -- and produce the byte-identical image gz_net_set_weights builds on the host.  The
 * generation roll of a live runner (gz_runner_update_network with device_blob = 1) takes this path.
 * The blob may still be in flight on any stream (a broadcast, an async copy): the call first waits
 * for all work issued to the device (hipDeviceSynchronize), so no caller-side synchronisation is
 * needed. */
int gz_net_set_weights_device(gz_net* net, const float* d_blob, size_t count);
/* device milliseconds of the last gz_net_set_weights_device (fold + pack kernels and copies) */
double gz_net_last_roll_ms(const gz_net* net);
/* diagnostics: copies the packed device weight image to host memory (out == NULL: returns its size) */
size_t gz_net_copy_weight_image(gz_net* net, void* out, size_t cap);

/* One contiguous run of boards of a segmented launch.  Pointers may be device memory or pinned host
 * memory (hipHostMalloc): the kernel gathers planes from, and scatters outputs to, each segment
 * directly.  (The native runner DMAs each launch's planes to an HBM staging buffer on a copy stream
 * first and passes that as the planes; outputs go straight to the pools' pinned buffers.) */
#define GZ_MAX_SEGMENTS 32
typedef struct gz_segment {
    int rows;
    const float* planes;                      /* [rows][C][H][W] */
    float* policies[GZ_MAX_ROLES];            /* [rows][P_r] */
    float* values;                            /* [rows][num_values] */
} gz_segment;

/* Asynchronous forward of up to GZ_MAX_SEGMENTS segments on `stream`.  Nets whose trunk kernel
 * holds two activation images (F <= 128, and F = 256 up to 8 x 8) run the whole forward -- trunk and
 * dense heads -- in one launch (gz_net_heads_fused); single-image nets (F = 256 on 10 x 10 / 13 x 13)
 * launch the trunk (planes -> head features), then the policy GEMM for large policies, then the
 * heads kernel. */
int gz_net_forward_segments(gz_net* net, void* stream, const gz_segment* segs, int nseg);
/* Same, recording `trunk_done_event` (a hipEvent_t, may be NULL) after the trunk launch so the
 * caller can time the trunk kernel alone. */
int gz_net_forward_segments_ev(gz_net* net, void* stream, const gz_segment* segs, int nseg,
                               void* trunk_done_event);

/* Synchronous forward, host buffers: planes float32 [n][C][H][W] (the poll() buffer layout,
 * cppinterface.py:114); policies[r] float32 [n][P_r]; values float32 [n][num_values].
 * Equivalent of predict_on_batch on one batch. */
int gz_net_forward(gz_net* net, const float* planes, int n,
                   float* const* policies, float* values);

/* Asynchronous forward on a caller stream (hipStream_t passed as void*), device buffers. */
int gz_net_forward_device(gz_net* net, void* stream, const float* d_planes, int n,
                          float* const* d_policies, float* d_values);

/* Diagnostics: on != 0 makes later forwards write the heads' pre-activation outputs (policy logits
 * before the softmax, value logits before the softmax / sigmoid) instead of probabilities, so parity
 * tests can compare nets whose softmaxes saturate. */
int gz_net_set_output_logits(gz_net* net, int on);

/* Device time (ms) of the last gz_net_forward (both launches), measured with HIP events on its stream. */
float gz_net_last_kernel_ms(const gz_net* net);

/* Launches of at least this many rows run the two-boards-per-workgroup trunk variant, smaller ones
 * the one-board variant (both compute every row identically).  GZ_PRECISION_FP32 and the layered
 * modes have one conv kernel for every launch size: 1 << 30, as for geometries with a single variant. */
int gz_net_large_min_rows(const gz_net* net);

/* The trunk kernel of launches below (large = 0) / from (large = 1) gz_net_large_min_rows rows, as
 * rocprofv3 names it (diagnostics: the bench reports its roofline per kernel).  GZ_PRECISION_FP32
 * and the layered modes: the conv kernel, for both. */
const char* gz_net_kernel_name(const gz_net* net, int large);

/* Rows one full wave of workgroups of the large variant covers (boards per workgroup x 256 CUs,
 * one trunk workgroup per CU): the native runner launches multiples of it beyond one wave.
 * GZ_PRECISION_FP32 and the layered modes: the rows whose conv grid (128 board positions x 64 / 128 filters per
 * workgroup) is one workgroup per CU. */
int gz_net_wave_rows(const gz_net* net);

/* Workgroups of the large variant resident per CU: 2 for the in-place split kernel (trunk_kernel_h2i,
 * where two of its workgroups fit the LDS and the runtime reports two), else 1.  gz_net_wave_rows
 * counts them: boards per workgroup x workgroups per CU x 256 CUs. */
int gz_net_workgroups_per_cu(const gz_net* net);

/* Algorithmic FLOPs of one leaf evaluation (2 FLOP/MAC). */
double gz_net_flops_per_eval(const gz_net* net);

/* 1 when the large (two-board) trunk variant runs the dense policy / value heads itself (two-image
 * kernels: no separate heads launch), 0 when a separate heads kernel follows it. */
int gz_net_heads_fused(const gz_net* net);

/* Which of their code paths the dense heads of this net take (read-only; decided at gz_net_create
 * from the geometry, the mode and the LDS budget): an OR of
 *   GZ_HEADS_FUSED_SMALL  the small trunk variant (launches below gz_net_large_min_rows) runs the heads itself
 *   GZ_HEADS_FUSED_LARGE  the large trunk variant does (what gz_net_heads_fused returns)
 *   GZ_HEADS_SEQ          one Dense after another with a max(P, VH) LDS row: the two-phase row
 *                         [P4_0 | .. | VH4] would push a kernel past the 160 KB of LDS
 *   GZ_HEADS_GEMM         the policy Denses run as one MFMA GEMM per launch (no fused heads, largest
 *                         policy >= 512, not fp32-ieee / fp16x3-layered)
 *   GZ_HEADS_LONG_ROW     the largest policy exceeds the register softmax of the GEMM logits (3,072):
 *                         with GZ_HEADS_GEMM, such roles' softmax goes through LDS, one role at a time
 * For tests and diagnostics: a test names the path it is about and asserts it here, so that it
 * cannot stop covering that path unnoticed when a budget constant moves. */
#define GZ_HEADS_FUSED_SMALL 1
#define GZ_HEADS_FUSED_LARGE 2
#define GZ_HEADS_SEQ 4
#define GZ_HEADS_GEMM 8
#define GZ_HEADS_LONG_ROW 16
int gz_net_heads_path(const gz_net* net);

const char* gz_nn_last_error(void);

/* ---- shadow check: live forwards against a second arithmetic mode --------------------------------
 * A net can carry a shadow: a second net of the same description and weights in another arithmetic
 * mode (e.g. GZ_PRECISION_FP32 beside a GZ_PRECISION_SPLIT net).  Counting the net's forwards of at
 * least one row from the enable, forward i is checked when i % every == 0 and both nets have
 * weights: its first min(rows, max_rows) rows, in segment order, also run through the shadow on the
 * caller's stream (same planes; outputs into a buffer of the shadow's), and two kernels
 * (csrc/nn/shadow_compare.hip) compare the two sets of outputs and add to running totals on the
 * device.  The net's own launches, outputs and trunk event are unchanged; gz_net_last_kernel_ms
 * times the net's forward alone.  A caller timing the whole call on its stream (the runner's
 * kernel_ms) sees a checked launch's shadow work: device_ms says how much.
 * With GZ_NN_SHADOW=<precision>[:<every>[:<max_rows>]] in the environment (defaults 64 and 256)
 * gz_net_create gives every net a shadow from birth and gz_net_destroy prints its totals to stderr;
 * a malformed value fails gz_net_create with "GZ_NN_SHADOW: ...". */
typedef struct gz_shadow_stats {
    long checks;           /* launches compared */
    long rows;             /* rows compared, the non-finite ones included */
    long nonfinite_rows;   /* rows with a non-finite value in either net's policies or values:
                              counted here and left out of every field below */
    long policy_elems;     /* policy elements compared (denominator of the mean |dp|) */
    long policy_rows;      /* (row, role) pairs compared (denominator of the mean KL) */
    long value_elems;
    double max_abs_dp, sum_abs_dp;     /* |p_net - p_shadow| over policy elements */
    double max_row_kl, sum_row_kl;     /* KL(p_shadow || p_net) per (row, role), both clipped at 1e-30
                                          (sum_i r_i log(r_i / g_i): slightly negative where the two rows'
                                          sums differ; the maxima start from 0) */
    long argmax_mismatch;              /* (row, role) pairs whose first-maximum index differs */
    double max_abs_dv, sum_abs_dv;     /* values */
    long worst_check, worst_row;       /* where max_abs_dp was seen: forward index of this net, row in it
                                          (0, 0 while max_abs_dp is 0) */
    double device_ms;                  /* shadow forward + comparison of all checks (HIP events) */
} gz_shadow_stats;
size_t gz_shadow_stats_sizeof(void);

/* Gives `net` a shadow in arithmetic mode `precision` on the net's device.  Fails ("shadow: ...") when
 * precision is the net's own mode, every < 1, max_rows < 1, the net already has a shadow, or
 * gz_net_create refuses the geometry in that mode.  The shadow starts without weights (the net keeps
 * no blob): checks begin with the first gz_net_set_weights / gz_net_set_weights_device after this
 * call.  From then on both calls give both nets the blob -- if either refuses it ("shadow: ..." when
 * it is the shadow), neither net's weights change -- and install both images in the critical
 * section a launch takes, so a launch compares two nets of one generation (a live runner's roll
 * included).  gz_net_set_output_logits reaches the shadow (KL fields then stay untouched);
 * gz_net_destroy destroys it. */
int gz_net_shadow_enable(gz_net* net, int precision, int every, int max_rows);
int gz_net_shadow_disable(gz_net* net);
/* Totals over the checks that have completed on the device, never a half-updated set; synchronises
 * neither the device nor a stream (at most 8 checks are in flight: a launch that would queue a 9th
 * first waits for the oldest).  reset != 0: later totals start from zero (checks still in flight
 * are dropped).  The same sequence of checks gives the same bits (device_ms apart). */
int gz_net_shadow_stats(gz_net* net, gz_shadow_stats* out, int reset);

/* The comparison alone on `device`, host arrays in: a = the net ("got"), b = the shadow ("ref"),
 * pol_x[r] float32 [n][policy_sizes[r]], val_x float32 [n][num_values].  *out = the totals of one
 * check (checks 1, worst_check 0, device_ms the two kernels' time).  Outputs that are logits have no
 * KL: compare them through a net in gz_net_set_output_logits mode. */
int gz_nn_compare_outputs(int device, int n, int roles, const int* policy_sizes, int num_values,
                          const float* const* pol_a, const float* val_a,
                          const float* const* pol_b, const float* val_b, gz_shadow_stats* out);

/* ---- symmetry ensemble: a forward averaged over a board's symmetries ------------------------------
 * A gz_symmetry holds the tables of a group of S = count <= 8 board symmetries, element 0 being the
 * identity by convention (galvanise_zero_amd/util/symmetry.py builds them from a game's descriptor):
 *   plane_src[s][i]     the planes of row X transformed by element s are X_s[i] = X[plane_src[s][i]],
 *                       i over plane_elems = C * H * W;
 *   move_src[r][s][m]   move m of role r is move move_src[r][s][m] in the transformed position.
 * gz_net_forward_sym computes, for every row, the net's ordinary forward (its own arithmetic mode) of
 * the S transformed rows -> p_s, v_s, and then in fp32, in this order,
 *   acc = p_0[move_src[0][m]];  acc += p_s[move_src[s][m]] for s = 1 .. S - 1;
 *   out[m] = acc * (1 / S) when S is a power of two (exact), else acc / S;
 * values alike without a permutation.  A row's result depends on its planes and the tables alone --
 * not on n, on how the call chunks its rows, or on the entry point -- and count = 1 with identity
 * tables is gz_net_forward bit for bit.  Non-finite values propagate.  Two kernels
 * (csrc/nn/symmetry.hip) expand the planes and reduce the outputs around one gz_net_forward_device
 * of S * rows rows, in chunks of 2,048 / S rows through scratch the gz_symmetry owns (the bound:
 * csrc/nn/symmetry.h; GZ_SYM_CHUNK_ROWS in the environment lowers the rows per chunk).  A net's shadow
 * check sees the inner forward as one more forward.
 * Refusals ("symmetry: ..."): gz_symmetry_create -- count outside 1..8, a plane or move table that is
 * not a permutation (the message names the element and the role); tables are copied and everything
 * is validated before any device call (the device is first touched by a forward).  A forward -- tables
 * whose plane_elems, roles or policy sizes are not the net's, and a net in gz_net_set_output_logits
 * mode (an average of logits is not what this computes). */
typedef struct gz_symmetry gz_symmetry;
gz_symmetry* gz_symmetry_create(int device, int count, int plane_elems, const int* plane_src /*[count][plane_elems]*/,
                                int roles, const int* policy_sizes, const int* const* move_src /*[roles] -> [count][P_r]*/);
void gz_symmetry_destroy(gz_symmetry* s);
int gz_symmetry_count(const gz_symmetry* s);
/* Synchronous, host buffers as gz_net_forward; takes the net's weight lock as gz_net_forward does and
 * runs on the net's own stream. */
int gz_net_forward_sym(gz_net* net, gz_symmetry* s, const float* planes, int n, float* const* policies, float* values);
/* Asynchronous on the caller's stream, device (or pinned host) buffers as gz_net_forward_device.  The
 * scratch belongs to the gz_symmetry: one gz_symmetry serves one stream at a time. */
int gz_net_forward_sym_device(gz_net* net, gz_symmetry* s, void* stream, const float* d_planes, int n,
                              float* const* d_policies, float* d_values);

/* ---- one symmetry per row, picked from the row's own planes ---------------------------------------
 * The one-evaluation form (AlphaGo Zero's self-play, KataGo's nnRandomize): each row is evaluated
 * under ONE element g of the tables and its policy mapped back -- one forward, not S.  g is not drawn
 * from a host RNG but hashed on the GPU from the row's own planes, so a row's result stays a function
 * of that row alone (any batch, slot, pool, entry point or replay gives the same bits).  With b_i the
 * 32-bit pattern of plane element i as stored (-0.0 differs from 0.0), E = plane_elems, S = count and
 * a 32-bit salt, in wrapping uint32 arithmetic:
 *   fmix(x): x ^= x>>16; x *= 0x85ebca6b; x ^= x>>13; x *= 0xc2b2ae35; x ^= x>>16
 *   h = sum over i in [0, E) of fmix(b_i + 0x9E3779B9 * (i + 1))
 *   g = (uint64(fmix(h ^ salt)) * S) >> 32                                  in [0, S)
 *   X'[i] = X[plane_src[g][i]];  p', v' = the net's ordinary forward of X';
 *   out_r[m] = p'_r[move_src[r][g][m]];  values = v'
 * No floating-point operation is added: a picked row is bit for bit the plain forward of the permuted
 * planes read through the move table, and count = 1 is gz_net_forward.  Two kernels
 * (csrc/nn/symmetry.hip: sym_pick_expand_kernel hashes and permutes, sym_pick_gather_kernel maps back)
 * around one gz_net_forward_device per chunk of 2,048 rows (GZ_SYM_CHUNK_ROWS lowers it), through the
 * gz_symmetry's scratch.  Refusals ("symmetry: ...", before any device call): tables that are not the
 * net's or were made for another device.  A net in gz_net_set_output_logits mode IS served: a
 * permutation of logits is the logits of the permuted position (nothing is averaged).
 * Whether this plays or trains stronger is the literature's claim; it is not measured here. */
int gz_net_forward_sym_pick(gz_net* net, gz_symmetry* s, unsigned salt, const float* planes, int n,
                            float* const* policies, float* values);
int gz_net_forward_sym_pick_device(gz_net* net, gz_symmetry* s, unsigned salt, void* stream, const float* d_planes, int n,
                                   float* const* d_policies, float* d_values);
/* The g of each row of planes [n][plane_elems] (host memory, or device memory when device_ptr), as
 * the GPU kernel computes it: for tests and diagnostics.  Synchronous. */
int gz_symmetry_picks(gz_symmetry* s, unsigned salt, int device_ptr, const float* planes, int n, int* out);

/* ---- evaluation cache: stored outputs for rows evaluated before ------------------------------------
 * Every forward mode computes a row's outputs from that row alone, so a table that returns the stored
 * outputs of a row returns the very bits the forward would write: the cache is exact.  A gz_eval_cache
 * is a direct-mapped table of `entries` entries in HBM, keyed by the row's plane words as stored (32-bit
 * patterns: -0.0 is not 0.0): a 64-bit tag from two modular row hashes picks the slot and filters, and
 * a hit needs all plane words equal (csrc/nn/eval_cache.h states the definition, csrc/nn/eval_cache.hip
 * holds the three kernels).  A call goes through in chunks of 2,048 rows: probe (hits are copied out,
 * misses claim their slot: the newest chunk, and in it the lowest row, wins), compact (the missed rows
 * gathered), the net's ordinary forward of the missed rows alone -- none when every row hit -- and fill
 * (outputs delivered, the claim's holder writes the entry).  Which rows hit is a function of the
 * sequence of calls, `entries` and the chunk size alone (galvanise_zero_amd/util/evalcache.py is the
 * model).  Rows of one chunk with equal planes all miss: nothing is deduplicated inside a call.
 * Entries belong to one weight generation of the net: gz_net_set_weights, gz_net_set_weights_device (a
 * live runner's roll included) and a change of gz_net_set_output_logits flush the cache at its next
 * call, and a call that a roll from another thread lands in is redone uncached, so every row of a call
 * comes from the one generation its forward was issued under.  A net's shadow sees the rows the inner
 * forward computes.
 * Environment, read at creation (tests): GZ_EVAL_CACHE_TAG_BITS (0..64) lowers the tag bits a probe
 * compares -- at 0 the plane compare alone separates keys; GZ_EVAL_CACHE_CHUNK_ROWS lowers the rows
 * per chunk.
 * Refusals ("eval cache: ..."), before any device call: a null argument; entries < 1; a table over
 * 16 GiB (the message names the bytes); a call with a cache made for another net or device -- the net
 * stays usable. */
typedef struct gz_eval_cache gz_eval_cache;
struct gz_eval_cache_stats {
    long calls;            /* gz_net_forward_cached / _device calls of at least one row */
    long rows;             /* rows of those calls = hits + forward_rows */
    long hits;             /* rows answered from the table */
    long forward_rows;     /* rows that went through the net's forward */
    long inserts;          /* entries written (device counter) */
    long replaced;         /* of those, over a valid entry of another key (device counter) */
    long flushes;          /* gz_eval_cache_clear, weight generations, output-logits changes */
    long entries;
    long entry_bytes;      /* bytes of one entry: header, planes, outputs */
};
gz_eval_cache* gz_eval_cache_create(gz_net* net, long entries);
void gz_eval_cache_destroy(gz_eval_cache* cache);
/* a flush: O(1), every entry becomes invalid */
int gz_eval_cache_clear(gz_eval_cache* cache);
/* waits for the cache's last call to finish on the device; reset != 0: the counts start from zero */
int gz_eval_cache_stats(gz_eval_cache* cache, struct gz_eval_cache_stats* out, int reset);
/* Synchronous, host buffers as gz_net_forward, on the net's own stream. */
int gz_net_forward_cached(gz_net* net, gz_eval_cache* cache, const float* planes, int n, float* const* policies, float* values);
/* On the caller's stream, device buffers as gz_net_forward_device; the outputs are complete in stream
 * order.  Blocks the calling thread once per chunk, until the chunk's count of misses has arrived (the
 * forward's grid is sized on the host).  Calls on one cache are serialised by a mutex and ordered on
 * the device by an event the cache owns. */
int gz_net_forward_cached_device(gz_net* net, gz_eval_cache* cache, void* stream, const float* d_planes, int n,
                                 float* const* d_policies, float* d_values);
/* hit[i] = 1 where row i of planes [n][plane_elems] (host memory, or device memory when device_ptr)
 * would hit now; no claim, no copy, no flush.  For tests and diagnostics.  Synchronous. */
int gz_eval_cache_probe(gz_eval_cache* cache, int device_ptr, const float* planes, int n, int* hit);

/* ---- canonical orientation: symmetric positions share one forward and one cache entry -------------
 * A third symmetry form beside the average and the pick.  Each row is evaluated under the ONE element
 * g that maps it to its symmetry class's canonical image, and the policy is mapped back; a cache may
 * stand in front of that forward.  With the pick's reading of a row (32-bit patterns), E, S, a 32-bit
 * salt, and the cache's hashes (above; csrc/nn/symmetry.h states all of it as functions a CPU runs):
 *   X_s[i] = X[plane_src[s][i]]                          image s, s in [0, S)
 *   t_s = h2(X_s) << 32 | h1(X_s)                        the cache's 64-bit row tag of image s
 *   k_s = mix64(t_s ^ uint64(salt))                      a bijection of the tag
 *   g   = the s with the smallest (k_s, s)               ties, equal images included: the lowest s
 *   X'  = X_g;  p', v' = the net's ordinary forward of X' (cache == NULL) or the cached forward of X';
 *   out_r[m] = p'_r[move_src[r][g][m]];  values = v'
 * 1. No floating-point operation is added: g depends on the row, the tables and the salt alone, and a
 *    row is bit for bit the plain forward of X_g read through move_src[g] in any batch, chunk, entry
 *    point or replay.  count = 1 with the identity is gz_net_forward.  Tables that are no group are
 *    served; they get this and nothing more.
 * 2. Where the tables are closed under composition (every game's are), a row and each of its images
 *    get the same X': through a cache the second one hits, and if the row's S images are all distinct
 *    out_X[r][m] == out_Y[r][move_src[r][t][m]] exactly for Y = X_t (the average gives that to 1e-6).
 * 3. A row that is its own image under some element is evaluated correctly, under the lowest such s;
 *    2's equality is not promised for it.  A tag collision between different images (2^-64 a pair)
 *    can cost sharing, never correctness: the cache compares all plane words.
 * sym_canon_expand_kernel (csrc/nn/symmetry.hip: one workgroup per row, the row in LDS, 2 S modular
 * sums) and the pick's gather stand around one gz_net_forward_device, or one cached call, per chunk
 * of 2,048 rows (GZ_SYM_CHUNK_ROWS lowers it) of canonical planes: at the defaults a call of n rows is
 * util/evalcache.py's CacheModel.call(canonical planes) exactly, and the cache's flush rules hold
 * unchanged.  Refusals, before any device call: the pick's ("symmetry: ..."), and with a cache the
 * cache's ("eval cache: ...": made for another net or device).  A net in gz_net_set_output_logits
 * mode is served.  Whether this plays or trains stronger is not measured here. */
int gz_net_forward_sym_canon(gz_net* net, gz_symmetry* s, unsigned salt, gz_eval_cache* cache /* may be NULL */,
                             const float* planes, int n, float* const* policies, float* values);
/* On the caller's stream; with a cache it blocks once per chunk, as gz_net_forward_cached_device. */
int gz_net_forward_sym_canon_device(gz_net* net, gz_symmetry* s, unsigned salt, gz_eval_cache* cache, void* stream,
                                    const float* d_planes, int n, float* const* d_policies, float* d_values);
/* g and (tag_out != NULL) t_g of each row of planes [n][plane_elems] (host memory, or device memory
 * when device_ptr), as the GPU kernel computes them: for tests and diagnostics.  Synchronous. */
int gz_symmetry_canon(gz_symmetry* s, unsigned salt, int device_ptr, const float* planes, int n, int* g_out,
                      unsigned long long* tag_out /* may be NULL */);

/* Diagnostics: with GZ_KERNEL_STAMPS set in the environment, gz_net_forward records per-workgroup
 * s_memtime stamps at phase boundaries; out8[0] = workgroups averaged, out8[1..4] = their mean
 * cycles of (input + initial conv, residual trunk, head 1x1 convs + features, fused dense heads)
 * in the last call.  GZ_PRECISION_FP32 and the layered modes (many launches per forward) have no
 * stamps: an error. */
int gz_net_stamp_avg(const gz_net* net, double* out8);

/* ---- native self-play driver (runner.hip) ----------------------------------------------------
 * Replaces the Python poll loop of the reference (cppinterface.py:131-144 driven by
 * distributed/worker.py:191) and its worker threads (supervisor.cpp:79-99,196-245) for the
 * steady state: num_threads engine threads x pools_per_thread game pools x batch_size games; one
 * launcher thread merges the pools waiting for predictions into segmented launches
 * (gz_net_forward_segments) that read planes from / write predictions to the pools' pinned host
 * buffers directly.
 * Uses the engine C-ABI (include/gzero_engine.h) for the pools. */
struct gz_sm;
struct gz_transformer;
struct gz_selfplay_config;
typedef struct gz_runner gz_runner;

typedef struct gz_runner_config {
    int device;
    int num_threads;
    int pools_per_thread;
    int batch_size;              /* games per pool = rows per NN batch */
    unsigned long long seed;
    long game_index_base;        /* global index of the first game (multi-GPU sharding) */
    int per_pool_unique_states;  /* 1: each pool owns its duplicate filter (deterministic per pool);
                                    0: one filter shared by every pool (reference, supervisor.cpp:31) */
    int keep_samples;            /* 1: queue samples for gz_runner_fetch_samples; 0: count and drop */
    int max_launch_rows;         /* cap on rows merged into one launch (0: no cap beyond 32 pools) */
    int min_launch_rows;         /* hold a launch until this many rows are queued ... (0: launch at once) */
    int max_launch_wait_us;      /* ... or its oldest pool has waited this long */
} gz_runner_config;

typedef struct gz_runner_stats {
    long batches;                /* NN forwards completed */
    long rows;                   /* leaf evaluations completed */
    double kernel_ms;            /* summed forward device time (HIP events around trunk + heads launches) */
    double trunk_ms;             /* summed trunk-kernel device time (events around the trunk launch) */
    long kernel_launches;
    long games_completed;
    long games_with_samples;
    long samples;
    long no_samples;
    long resigns;
    long aborts;
    long dupes;
    long segments;               /* pools merged into launches, summed over launches */
    long completed_game_evals;   /* NN evaluations consumed by the completed games */
    long large_launches;         /* launches that ran the two-boards-per-workgroup trunk variant */
    long large_rows;
    double large_trunk_ms;
    double engine_idle_ms;       /* summed over engine threads: time with none of the thread's pools ready */
    long tree_playouts;          /* tree playouts of all games (NN-free ones = tree_playouts - rows) */
    long large_rounds;           /* workgroup rounds of the large launches: sum of ceil(rows / gz_net_wave_rows) */
    long split_launches;         /* launches holding part of a pool's batch (exact-round composition) */
} gz_runner_stats;

gz_runner* gz_runner_create(gz_net* net, const struct gz_sm* sm, const struct gz_transformer* t,
                            const gz_runner_config* cfg, const struct gz_selfplay_config* conf,
                            const int* policy_sizes, int num_policies, int num_values);
/* Self-play under one board symmetry per position (gz_net_forward_sym_pick's definition, above): every
 * row of every launch is hashed, permuted, evaluated and mapped back on the GPU.  The launcher stages
 * the planes in HBM as always, sym_pick_expand_kernel writes the permuted rows to a second per-slot
 * buffer the forward reads, the forward writes raw outputs to a per-slot buffer and
 * sym_pick_gather_kernel writes the slot's output staging, which the third stream copies to the
 * pools' pinned buffers (output staging is forced on) -- one launch of each kernel per net launch.
 * Before gz_runner_start only.  Refused ("runner: ..." / "symmetry: ..."), before any device call: a
 * started runner; a zero-copy runner (GZ_RUNNER_ZERO_COPY=1: the pick needs the HBM plane staging);
 * tables that are not the net's or were made for another device.  The gz_symmetry must outlive the
 * runner.  Without this call the launcher issues exactly the calls it always did. */
int gz_runner_set_symmetry(gz_runner* r, gz_symmetry* s, unsigned salt);
/* rows that went through the pick path (equal to gz_runner_stats.rows with a symmetry set, else 0) */
long gz_runner_sym_pick_rows(gz_runner* r);
/* Self-play through an evaluation cache (gz_eval_cache, above): a launch becomes plane copy -> probe +
 * compact on the launch stream -> the launcher waits for the count of misses (the older launch retires
 * meanwhile) -> the forward of the missed rows alone -> fill.  The rows' destinations are the segments
 * the launch would have written (the pools' pinned buffers, or the output staging's blocks, which are
 * then copied as always); an all-hit launch records its events without a forward, and a launch's
 * trunk time is its whole cached time.  A generation roll is applied on the launcher thread, so the
 * next launch flushes the cache.  Before gz_runner_start only.  Refused ("runner: ..." / "eval cache:
 * ..."), before any device call: a started runner; a zero-copy runner (GZ_RUNNER_ZERO_COPY=1); a runner
 * with a symmetry set (and gz_runner_set_symmetry on a runner with a cache); a cache made for another
 * net.  The cache must outlive the runner.  Without this call the launcher issues exactly the calls it
 * always did. */
int gz_runner_set_cache(gz_runner* r, gz_eval_cache* cache);
/* Self-play in the canonical orientation (gz_net_forward_sym_canon, above), with or without a cache:
 * gz_runner_set_symmetry's launch with sym_canon_expand_kernel in the pick expand's place, and with a
 * cache gz_runner_set_cache's probe / forward of the misses / fill reading the canonical planes and
 * writing the raw outputs the gather reads.  Output staging is forced on, and
 * gz_runner_sym_pick_rows counts these rows.  Before gz_runner_start only.  Refused, before any
 * device call: a started runner; a zero-copy runner; a runner that already has a symmetry, a cache or
 * a canonical setting (and gz_runner_set_symmetry / gz_runner_set_cache on a runner in canonical
 * mode); the pick's and the cache's refusals.  Both objects must outlive the runner. */
int gz_runner_set_canonical(gz_runner* r, gz_symmetry* s, unsigned salt, gz_eval_cache* cache /* may be NULL */);
int gz_runner_start(gz_runner* r);   /* once per runner: a stopped runner cannot be restarted */
int gz_runner_wait_batches(gz_runner* r, long total_batches, double timeout_s);
int gz_runner_wait_rows(gz_runner* r, long total_rows, double timeout_s);
int gz_runner_stats_get(gz_runner* r, gz_runner_stats* out);
int gz_runner_stop(gz_runner* r);
void gz_runner_destroy(gz_runner* r);
/* Samples queued since the last call, as one JSON array of datadesc.Sample records
 * (supervisor_impl.cpp:75-118 field names), or NULL when none; free with gz_free. */
char* gz_runner_fetch_samples(gz_runner* r);
/* clear_unique_states (supervisor_impl.cpp:138-144) at a generation roll (worker.py:160); safe while
 * the runner is running. */
int gz_runner_clear_unique_states(gz_runner* r);
/* Generation roll on a live runner (worker.py:138-160: Supervisor.update_nn + clear_unique_states):
 * the launcher swaps in the new weights (blob: host float32, or device memory when device_blob,
 * e.g. after an RCCL broadcast) between two launches, so every pool batch runs on exactly one
 * network, then clears the duplicate filters if clear_unique_states.  Blocks until applied. */
int gz_runner_update_network(gz_runner* r, const float* blob, size_t count, int device_blob,
                             int clear_unique_states, double timeout_s);
/* After a roll: pool_batches[i] = batches of pool i launched on the previous network;
 * *launches_before = launches issued before the swap. */
int gz_runner_roll_info(gz_runner* r, long* pool_batches, int npools, long* launches_before);
/* wall milliseconds the launcher spent applying the last roll (the weight fold / pack and swap) */
double gz_runner_roll_apply_ms(gz_runner* r);
/* Per-game costs by the game's ordinal within its slot, summed over the runner's pools (struct
 * gz_ordinal_stats, include/gzero_engine.h); a snapshot, safe while the runner runs. */
struct gz_ordinal_stats;
int gz_runner_ordinal_stats(gz_runner* r, struct gz_ordinal_stats* out);
const char* gz_runner_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* GZERO_NN_H */
