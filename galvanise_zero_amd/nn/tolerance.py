"""The stated accuracy of the MI355X forward in the bench's arithmetic (bf16x3 split), per BASELINE
config: the north-star tolerance "policy/value outputs match the reference net on identical board
batches within a stated fp tolerance" (BASELINE.json), against the float64 restatement of the
reference forward (oracle/nn_ref.py; reference src/ggpzero/nn/model.py:154-296).

Measured on MI355X (profiles/r04a_split_error_dist.json, tools/split_error_dist.py): the bench's own
weights (random_weights(desc, 7921), undamped), 10 input seeds, one launch each of >= 1,024 rows in
pool-sized pinned-host segments with HBM staging -- the runner's launch shape.  Each bound is 3x the
maximum over the seeds, rounded up:

  max    max |p - p_ref| over every policy / value output element
  mean   mean |p - p_ref| (per output, the largest)
  kl     max over rows of KL(p_ref || p) (per output, the largest)
  logits max |z - z_ref| / max(1, max |z_ref|) of the heads' pre-softmax outputs

The deep configs' random nets have logits of magnitude 10^2 - 10^4 (no trained .h5 exists), so their
softmaxes saturate and a 5e-5 relative logit error moves individual probabilities by up to ~0.05: the
logits bound is the fp32-class criterion, the probability bounds state what that does to the outputs.
tests/test_bench_shape_gpu.py, tests/test_nn_gpu.py::test_split_precision_against_fp32 and
__graft_entry__.smoke() assert these constants (test_deep_config_bench_weights asserts each config's
logits bound on its own, cfg2 included).  These are offline figures on random nets; the error on the
positions self-play visits with the weights actually loaded is what a net's shadow check reports
live (HipNet.enable_shadow / shadow_stats, include/gzero_nn.h gz_net_shadow_enable).

These constants come from the kernels they check (3x what was measured), so they bound what the
kernels did on that day, not what a correct kernel may do.  What does not depend on any measurement
is the exact suite (tests/exact_lattice.py, tests/test_nn_exact.py, tests/test_nn_exact_gpu.py;
DESIGN 5): on nets whose every operand, product, sum and activation is representable in a mode's
arithmetic, every mode, trunk family and kernel variant returns the float64 oracle's logits bit for
bit -- it pins indices, taps, padding, channel order, the lo parts and their scales, the per-board
exponents, with no tolerance at all.  It says nothing about rounding: the tolerance tests and the
constants below remain the statement of accuracy on dense weights.

What the arithmetic is: bf16x3 ("split"; HipNet / bench.py --precision "bf16x3", the old name "fp32"
is a deprecated alias) keeps ~16 significant bits per operand against IEEE fp32's 24, with fp32
accumulation and an fp32 residual stream.  It is fp32-CLASS, not fp32: on the headline cfg2 batch
(1,024 rows, tests/test_nn_gpu.py::test_split_precision_against_fp32) its max error against the
float64 oracle is 1.5-2.0e-4, about 35x the 5.7e-6 of an IEEE fp32 forward of the same net (torch
fp32 on the CPU), and 300x below bf16's 5.9e-2.

The three modes: "bf16" (bf16 operands; 1e-2-class errors on deep nets; fastest), "bf16x3" (above; the
bench's and self-play's mode) and "fp32-ieee" (GZ_PRECISION_FP32: every conv on the f32-input MFMA,
fp32 activations, blocked fp32 sums -- the reference's arithmetic).  fp32-ieee's error against the
float64 oracle is a true fp32 forward's: 0.2-1.6x torch-CPU fp32's on every v1 case of
tests/test_nn_fp32_gpu.py, whose bound is 4 x max(torch fp32's error, 1e-6) (cfg2 on the bench's
weights: 2.1e-6 at 37 rows, 4.7e-6 at 256 rows against bf16x3's 9.7e-5); v2 nets' relative logit
error is 1.9-3.7e-7 against bf16x3's 2.7-5.1e-6.  It costs 4.2x a bf16x3 forward: use
it for match play, gating games and for separating a wrong net from a saturated softmax moved by
the split arithmetic; the constants below are bf16x3's.

v2 nets with 256 filters (tests/test_nn_v2_f256_gpu.py: two-block nets on 8 x 8, 10 x 10 and 13 x 13,
85 squeeze-excite units, damped weights, 1 and 7 rows; profiles/v2_f256_gpu_tests.log) are asserted
against the 256-filter constants below: bf16x3's relative logit error is at most 7.2e-6 against the
cfg4 bound of 1.2e-4, its probabilities within max 8.9e-7 / mean 4.0e-7 / row KL 1.1e-7 against
DAMPED_TOLERANCE; bf16 errs at most 1.0e-3 / 4.6e-4 (its 128-filter twins: 8.2e-4 / 4.2e-4);
fp32-ieee 1.2e-7 / 3.2e-8 with a relative logit error of 2.9e-7.

The layered modes ("bf16-layered" / "bf16x3-layered": bf16's / bf16x3's operands and products on
fp32-ieee's layer-by-layer trunk, for the nets the fused kernels refuse) are asserted against the
same constants (tests/test_nn_layered_gpu.py; damped weights, 1-7 rows): bf16x3-layered's relative
logit error against LOGITS_TOL = 1.2e-4 and, where the fused bf16x3 runs the net, 3 x the fused
mode's; its probabilities against DAMPED_TOLERANCE; bf16-layered per output against max(TOL_V2_BF16,
3 x the fused bf16 error of the net or of its fused-size twin).  Measured on MI355X (profiles/layered_gpu_tests.txt):
bf16x3-layered probabilities within max 1.62e-6 / mean 1.13e-6 / row KL 1.16e-7, relative logit error
at most 2.91e-5 (both on the 13 x 13 v1 net of 14 x 256, 2 rows; 2.8-7.2e-6 on the two-block nets,
0.76-1.01 x the fused bf16x3's on the same rows); bf16-layered max 1.04e-3 (6 x 9 legacy net, 7 rows), equal to
the fused bf16's on the same rows to the printed digits on every net both run.

"fp16x3-layered" (GZ_PRECISION_F16X3_LAYERED: the layered trunk with each operand as fp16 hi + fp16
lo scaled by 2^11 -- 22 significand bits against bf16x3's 16 and fp32's 24 --, three f16 MFMAs per
product into two fp32 accumulators, one power-of-two exponent per board and conv input against
fp16's range, the heads fp32-ieee's) has no constants here: tests/test_nn_fp16x3_gpu.py bounds its
relative logit error by the two neighbouring modes' on the same weights and rows -- at most 4 x
fp32-ieee's (two significand bits fewer per operand) and at most a quarter of bf16x3-layered's (six
bits more) -- and its probabilities by DAMPED_TOLERANCE.  The errors measured on MI355X are in
profiles/fp16x3_gpu_tests.txt and DESIGN 3.1.

The north-star tolerance per config, then:
  cfg2, cfg3   the probability bounds below (max / mean / KL), on the bench's weights
  cfg4, cfg5   the relative logits bound below on the bench's (saturating) weights, and in probability
               space DAMPED_TOLERANCE on damped weights (res_gamma 0.15, interior softmaxes) at the
               runner's launch shape (>= 1,024 rows in pinned-host segments;
               tests/test_bench_shape_gpu.py::test_deep_config_damped_at_launch_shape)
"""

# Bounds in probability space for the deep configs on damped weights at the launch shape: 3x the
# worst measured on MI355X over cfg4 / cfg5 (profiles/r05g_deep_parity.log: max |dp| 4.65e-6, mean
# 8.1e-7, row KL 1.65e-7) -- fp32-class (tests/test_nn_gpu.py's TOL_FP32 is 2e-4 / 5e-5 / 5e-7)
DAMPED_TOLERANCE = {"max": 1.4e-5, "mean": 2.5e-6, "kl": 5e-7}

# 3x the max over 10 seeds (measured max in the comment)
SPLIT_TOLERANCE = {
    # breakthrough 8x8, 6 x 128 (the headline kernel trunk_kernel<128, 4, 2, 1, 3>)
    "cfg2": {"max": 5.4e-4, "mean": 4.4e-6, "kl": 7.7e-7, "logits": 2.1e-4},     # 1.80e-4 1.45e-6 2.56e-7 6.76e-5
    # reversi 8x8, 10 x 128, draw head
    "cfg3": {"max": 2.2e-3, "mean": 3.6e-6, "kl": 3.3e-6, "logits": 1.4e-4},     # 7.17e-4 1.18e-6 1.07e-6 4.35e-5
    # hexLG13, 12 x 256 (two-pass split kernel)
    "cfg4": {"max": 1.3e-2, "mean": 2.2e-6, "kl": 1.2e-4, "logits": 1.2e-4},     # 4.30e-3 7.18e-7 3.86e-5 3.74e-5
    # amazons 10x10, 20 x 256 (single-image split kernel + split policy GEMM)
    "cfg5": {"max": 0.17, "mean": 1.7e-4, "kl": 2.0e-2, "logits": 1.5e-4},       # 5.43e-2 5.66e-5 6.48e-3 4.99e-5
}
MEASURED = "profiles/r04a_split_error_dist.json"
