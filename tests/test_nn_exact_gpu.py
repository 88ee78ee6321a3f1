"""Every forward mode, bit for bit, on exactly representable nets (tests/exact_lattice.py).

On these nets every operand, product, partial sum and activation is representable in the arithmetic
of the mode under test (tests/test_nn_exact.py asserts exact_lattice.check_representable for every
(net, mode) pair below, on the CPU), so a correct kernel returns the float64 oracle's logits exactly:
each policy role's logits and the value logits, in set_output_logits(True), are np.array_equal to
exact_lattice.expected_logits cast to float32.  Nothing here is compared under a bound that was
measured on the kernels; the one bounded comparison, test_probabilities, isolates the heads' softmax
on exact logits and asserts the project's DAMPED_TOLERANCE.

A net is listed with the modes whose conditions it meets and whose kernels take it; nets that need
more bits than a mode has are not run in that mode.  Squeeze-excite nets are in (SE_CASES), on
weights and planes that saturate every gate at exactly 0, 1/2 or 1 (exact_lattice's docstring): the
two-image and the single-image / two-pass gate paths of the fused kernels and the layered modes'
gate and apply kernels, under each kernel variant and across row chunks.  The dense heads are in
(HEAD_CASES): one to four roles of unequal size, one to four values, hidden widths of 6, 299 and 301,
and every path the heads can take -- fused two-phase and sequential, heads_kernel and its blocked
form, the policy GEMM with the register and with the LDS softmax -- each asserted through
HipNet.heads_path(), at launches whose last heads workgroup and last GEMM board tile are partial;
test_saturated_outputs puts one logit (or two tied) 2^12 above the rest and asserts probabilities of
exactly 1, 0.5 and 0.  Left to the tolerance tests: leaky nets, the pooling value head on boards
whose position count is no power of two (exact_lattice's docstring: the channel mean multiplies by
fl32(1 / npos), forward_kernel.h "sm[r] * inv"), and small errors in the scale of the squeeze-excite
mean on such boards, which a saturated gate cannot see by construction.
"""
import dataclasses

import numpy as np
import pytest

import exact_lattice as xl
from galvanise_zero_amd._native import HEADS_FUSED_LARGE, HEADS_FUSED_SMALL, HEADS_GEMM, HEADS_LONG_ROW, HEADS_SEQ
from galvanise_zero_amd.nn.desc import NetDesc
from galvanise_zero_amd.nn.tolerance import DAMPED_TOLERANCE
from galvanise_zero_amd.nn.weights import to_blob

pytestmark = pytest.mark.gpu

FUSED = ("bf16", "bf16x3")
LAYERED = ("fp32-ieee", "bf16-layered", "bf16x3-layered", "fp16x3-layered")
ALL = FUSED + LAYERED
WIDE16 = ("bf16x3", "bf16x3-layered", "fp16x3-layered", "fp32-ieee")
ROWS = (1, 3)
SCALES = (2.0 ** -4, 1.0, 2.0 ** 7, 2.0 ** 12)
LEGACY = dict(flatten_nchw=True, conv_bias=True, value_bn=True, value_sigmoid=True)
F128 = NetDesc(5, 8, 8, 128, 2, [155, 155])
WIDE_NET = NetDesc(5, 8, 8, 128, 1, [155, 155], value_bn=True)
GEMM_NET = NetDesc(12, 10, 10, 256, 1, [3041, 3041], value_bn=True)
V2_POOL = dict(resnet_v2=True, global_pooling_value=True, value_bn=True)


@dataclasses.dataclass
class Case:
    desc: NetDesc
    modes: tuple
    seed: int = 1
    nnz: int = 2
    wmax: int = 1
    wide: dict = None
    scales: tuple = None          # one power of two per board (then rows = len(scales))
    order: tuple = None           # the scaled boards in this order
    homogeneous: bool = False     # trunk shifts zeroed (exact_lattice.zero_trunk_shifts)
    exhaustive: bool = False      # modes = every mode whose conditions hold (test_nn_exact.py asserts it)
    family: str = None            # kernel family this net represents in test_nn_exact.py's fault checks
    se: bool = False              # squeeze-excite with saturated gates (exact_lattice.lattice_se_weights)
    plane_seed: int = None        # SE nets: the planes' seed (default 100 + rows), chosen for the liveness conditions
    head: bool = False            # a dense-heads case (HEAD_CASES): exact_lattice.head_last_rows applied, head liveness asserted
    rows: tuple = None            # the launches of test_exact (default ROWS); the planes are built for the largest
    path: dict = None             # head cases: {mode: HipNet.heads_path() bits} the case is there for
    large_kernel: dict = None     # head cases: {mode: kernel_name(True)} where the case is about the large variant's choice


CASES = {
    # ---- the fused bf16 / bf16x3 trunk kernels; the first net in the four layered modes too ----
    "8x8_f128_b2": Case(F128, ALL, family="fused_f128", seed=4),
    "6x7_c12_f128_b2": Case(NetDesc(12, 6, 7, 128, 2, [85, 86]), FUSED),           # partial last position tile
    "5x5_c12_f128_b2": Case(NetDesc(12, 5, 5, 128, 2, [51, 50]), FUSED),
    "8x8_f64_b1_v3": Case(NetDesc(5, 8, 8, 64, 1, [65, 65], num_values=3), FUSED, family="fused_f64", seed=2),
    "8x8_f96_b1": Case(NetDesc(5, 8, 8, 96, 1, [155, 155]), FUSED, family="fused_f96_padded", seed=2),
    "8x8_legacy_f128_b1": Case(NetDesc(5, 8, 8, 128, 1, [155, 155], **LEGACY), FUSED, seed=3),
    "13x13_f256_b2": Case(NetDesc(5, 13, 13, 256, 2, [170, 171]), FUSED, family="split_two_pass_f256"),
    "10x10_c12_f256_b1_gemm": Case(NetDesc(12, 10, 10, 256, 1, [3041, 3041]), FUSED, family="single_image_gemm_heads"),
    "19x19_f128_b1": Case(NetDesc(5, 19, 19, 128, 1, [362, 362]), FUSED, family="fused_19x19"),
    "v2_8x8_f128_b2_pool": Case(NetDesc(5, 8, 8, 128, 2, [155, 155], resnet_v2=True, global_pooling_value=True, value_bn=True),
                                FUSED, family="v2_pool"),
    "v2_13x13_f256_b2_concat": Case(NetDesc(5, 13, 13, 256, 2, [170, 171], value_hidden_size=128, resnet_v2=True,
                                            concat_all_layers=True), ALL, family="v2_concat"),
    "v2_10x10_f256_b1_bare": Case(NetDesc(5, 10, 10, 256, 1, [101, 101], resnet_v2=True, initial_kernel_size=3,
                                          initial_bn=False), FUSED),
    # ---- the layer-by-layer trunk: fp32-ieee, bf16-layered, bf16x3-layered, fp16x3-layered ----
    "19x19_f256_b2": Case(NetDesc(5, 19, 19, 256, 2, [362, 362]), LAYERED, family="layered_19x19", seed=2),
    "6x9_legacy_f40_b2": Case(NetDesc(4, 6, 9, 40, 2, [55, 54], value_hidden_size=48, **LEGACY), ALL, family="legacy_f40"),
    # ---- wide operands: the lo parts (every net above is hi-exact everywhere) ----
    "wide_w0_16": Case(WIDE_NET, WIDE16, wide={"kind": "initial_weights", "bits": 16}, exhaustive=True),
    "wide_w0_22": Case(WIDE_NET, ("fp16x3-layered", "fp32-ieee"), wide={"kind": "initial_weights", "bits": 22}, exhaustive=True),
    "wide_w0_24": Case(WIDE_NET, ("fp32-ieee",), wide={"kind": "initial_weights", "bits": 24}, exhaustive=True),
    "wide_stream_16": Case(WIDE_NET, WIDE16, wide={"kind": "stream", "bits": 16}, exhaustive=True),
    "wide_stream_22": Case(WIDE_NET, ("fp16x3-layered", "fp32-ieee"), wide={"kind": "stream", "bits": 22}, exhaustive=True),
    "wide_stream_24": Case(WIDE_NET, ("fp32-ieee",), wide={"kind": "stream", "bits": 24}, exhaustive=True),
    # the policy GEMM's split of its features (11 bits under +-1 weights) and of its weights (16 bits)
    "gemm_wide_features": Case(GEMM_NET, WIDE16, wide={"kind": "stream", "bits": 16}, exhaustive=True),
    "gemm_wide_weights": Case(GEMM_NET, ALL, wide={"kind": "policy_dense", "bits": 16}),
    # ---- boards of different scale in one launch, and the same boards permuted ----
    "8x8_scaled": Case(F128, ALL, scales=SCALES, homogeneous=True, exhaustive=True, seed=4),
    "8x8_scaled_permuted": Case(F128, ALL, scales=SCALES, order=(2, 0, 3, 1), homogeneous=True, exhaustive=True, seed=4),
}
SE = dict(se=True, homogeneous=True)
SE_CASES = {
    # ---- squeeze-excite with saturated gates (0, 1/2, 1 exactly): se_gates / squeeze_excite in the fused
    # kernels, se_gate_kernel / se_apply_kernel in the four layered modes.  Trunk shifts zeroed and planes of
    # mixed fill, so that the channel means' proportions, and with them the gates, differ from board to board;
    # the seeds are those at which test_nn_exact.py's conditions, liveness and fault checks all hold ----
    # the two-image squeeze_excite, and the layered kernels
    "se_8x8_f128_b2_s42_pool": Case(NetDesc(5, 8, 8, 128, 2, [155, 155], se_units=42, **V2_POOL), ALL, family="se_two_image_f128",
                                    seed=2, plane_seed=200, **SE),
    "se_8x8_f64_b3_s21": Case(NetDesc(5, 8, 8, 64, 3, [155, 155], se_units=21, **V2_POOL), FUSED, family="se_f64",
                              seed=8, plane_seed=200, **SE),
    # se_gate_kernel's j += FP loop runs twice
    "se_8x8_f64_b1_s128": Case(NetDesc(5, 8, 8, 64, 1, [155, 155], se_units=128, **V2_POOL), LAYERED,
                               family="se_layered_s128", seed=1, plane_seed=100, **SE),
    # F padded to 128: the padded channels' means and compress rows must contribute nothing
    "se_8x8_f80_b2_s26_concat": Case(NetDesc(5, 8, 8, 80, 2, [155, 155], value_hidden_size=128, resnet_v2=True, se_units=26,
                                             concat_all_layers=True), FUSED + ("fp32-ieee",), family="se_f80_padded",
                                     seed=1, plane_seed=200, **SE),
    # the single-image / ADDB path, S no multiple of 4
    "se_8x8_f256_b2_s85": Case(NetDesc(5, 8, 8, 256, 2, [155, 155], se_units=85, **V2_POOL), FUSED,
                               family="se_single_image_f256", seed=1, plane_seed=100, **SE),
    # the two-pass split, a partial last position tile under the 16 * pt + li < npos guard
    "se_13x13_f256_b2_s85": Case(NetDesc(5, 13, 13, 256, 2, [170, 171], resnet_v2=True, se_units=85), FUSED,
                                 family="se_two_pass_f256", seed=1, plane_seed=100, **SE),
    "se_10x10_f192_b2_s64_v3": Case(NetDesc(12, 10, 10, 192, 2, [101, 101], num_values=3, resnet_v2=True, se_units=64), FUSED,
                                    family="se_f192_padded", seed=2, plane_seed=100, **SE),
    "se_19x19_f128_b1_s42": Case(NetDesc(5, 19, 19, 128, 1, [362, 362], resnet_v2=True, se_units=42), ALL,
                                 family="se_19x19", seed=4, plane_seed=200, **SE),
}
CASES.update(SE_CASES)


def _path(fused, gemm_layered, valu_layered):
    """{mode: heads_path bits}: the fused modes, the layered modes that have the policy GEMM, and the
    two whose policy Dense stays on the VALU."""
    return {"bf16": fused, "bf16x3": fused, "bf16-layered": gemm_layered, "bf16x3-layered": gemm_layered,
            "fp32-ieee": valu_layered, "fp16x3-layered": valu_layered}


BOTH = HEADS_FUSED_SMALL | HEADS_FUSED_LARGE
GEMM_MODES = ("bf16", "bf16x3", "bf16-layered", "bf16x3-layered")
HEAD_ROWS = (1, 3, 5)       # 5: heads_kernel's second workgroup of kHeadBoards = 4 holds one board
GEMM_ROWS = (1, 3, 65)      # 65: policy_gemm_kernel's second tile of 64 boards holds one board
HEAD = dict(head=True)
HEAD_CASES = {
    # ---- the dense heads (forward_kernel.h dense_heads / dense_heads_seq / policy_gemm_kernel) away from two
    # roles of nearly equal size: one-block trunks, every case named for the path it pins (path: the bits of
    # HipNet.heads_path() per mode, asserted by test_exact).  The seeds are those at which test_nn_exact.py's
    # conditions, head liveness and head faults all hold ----
    # role counts on fused heads (FS = (2R + 1) npos, the unit-to-role walk, fused_heads_bytes)
    "head_r1_f64": Case(NetDesc(5, 8, 8, 64, 1, [155]), ALL, path=_path(BOTH, 0, 0), seed=6, **HEAD),
    "head_r3_f128": Case(NetDesc(5, 8, 8, 128, 1, [65, 64, 63]), ALL, rows=HEAD_ROWS, path=_path(BOTH, 0, 0), seed=24, **HEAD),
    "head_r4_f64_v4": Case(NetDesc(5, 8, 8, 64, 1, [1, 255, 256, 257], num_values=4), ALL, rows=HEAD_ROWS, path=_path(BOTH, 0, 0), seed=68, **HEAD),
    # the value head: one value from 6 hidden units behind the pooled means; 299 hidden units (j += NT runs
    # twice, VH4 = 300) into two sigmoids on a legacy net
    "head_v1_vh6_pool": Case(NetDesc(5, 8, 8, 128, 1, [155, 154], num_values=1, value_hidden_size=6, **V2_POOL), ALL,
                             path=_path(BOTH, 0, 0), seed=3, **HEAD),
    "head_vh299_sigmoid": Case(NetDesc(5, 8, 8, 128, 1, [155, 154], value_hidden_size=299, **LEGACY), ALL,
                               path=_path(BOTH, 0, 0), seed=14, **HEAD),
    "head_vh301_f64": Case(NetDesc(5, 8, 8, 64, 1, [66, 65], value_hidden_size=301, num_values=3), ALL,
                           path=_path(BOTH, 0, 0), seed=15, **HEAD),
    # the separate heads_kernel (heads_kernel_blocked in fp32-ieee / fp16x3-layered), two-phase: three unequal
    # roles below the GEMM's threshold behind a single-image trunk and behind the layered trunks
    "head_sep_r3": Case(NetDesc(5, 10, 10, 256, 1, [101, 37, 250]), ALL, rows=HEAD_ROWS, path=_path(0, 0, 0), seed=5, **HEAD),
    # the policy GEMM with the register softmax: the threshold beside a role of one j-tile; a role at
    # kGemmSoftmaxMax exactly between two whose sizes are no multiples of 16.  fp32-ieee and fp16x3-layered
    # run the same policies on the VALU (heads_kernel_blocked)
    "head_gemm_512_7": Case(NetDesc(5, 10, 10, 256, 1, [512, 7]), ALL, rows=GEMM_ROWS, path=_path(HEADS_GEMM, HEADS_GEMM, 0),
                            seed=3, **HEAD),
    "head_gemm_r3_3072": Case(NetDesc(5, 10, 10, 256, 1, [1001, 3072, 17]), ALL, rows=GEMM_ROWS,
                              path=_path(HEADS_GEMM, HEADS_GEMM, 0), seed=15, **HEAD),
    # the GEMM logits' LDS softmax (dense_heads_seq with gemm_heads): both roles through LDS or one; and a
    # register role, an LDS role, a register role in one net.  On the VALU the LDS row is the long one
    "head_gemm_lds_3073": Case(NetDesc(5, 10, 10, 256, 1, [3073, 3072]), ALL, rows=GEMM_ROWS,
                               path=_path(HEADS_GEMM | HEADS_LONG_ROW, HEADS_GEMM | HEADS_LONG_ROW, HEADS_LONG_ROW), seed=2, **HEAD),
    "head_gemm_mixed": Case(NetDesc(5, 10, 10, 256, 1, [530, 3100, 17]), ALL, rows=GEMM_ROWS,
                            path=_path(HEADS_GEMM | HEADS_LONG_ROW, HEADS_GEMM | HEADS_LONG_ROW, HEADS_LONG_ROW), seed=15, **HEAD),
    # large policies on a fused trunk (no GEMM): the two-phase row still fits; the two-board kernel's LDS
    # forces heads_seq; the wave-group kernel's image is too small for the heads' scratch (wg_fits), so the
    # large launches fall back to the two-board kernel (DESIGN.md has the arithmetic)
    "head_fused_p3100_f64": Case(NetDesc(5, 8, 8, 64, 1, [3100, 600]), FUSED, rows=HEAD_ROWS, path=_path(BOTH | HEADS_LONG_ROW, 0, 0),
                                 large_kernel={"bf16": "gznn::trunk_kernel<64, 4, 2, 1, 1>", "bf16x3": "gznn::trunk_kernel<64, 4, 1, 1, 3>"},
                                 seed=16, **HEAD),
    "head_fused_seq_f128": Case(NetDesc(5, 8, 8, 128, 1, [4500, 4700]), FUSED, rows=HEAD_ROWS, path=_path(BOTH | HEADS_SEQ | HEADS_LONG_ROW, 0, 0),
                                large_kernel={"bf16": "gznn::trunk_kernel<128, 4, 2, 1, 1>", "bf16x3": "gznn::trunk_kernel<128, 4, 2, 1, 3>"},
                                seed=9, **HEAD),
    "head_fused_wgfits_f128": Case(NetDesc(5, 8, 8, 128, 1, [1500, 1501]), FUSED, rows=HEAD_ROWS, path=_path(BOTH, 0, 0),
                                   large_kernel={"bf16": "gznn::trunk_kernel<128, 4, 2, 1, 1>", "bf16x3": "gznn::trunk_kernel<128, 4, 2, 1, 3>"},
                                   seed=2, **HEAD),
}
CASES.update(HEAD_CASES)
# one net at 5 rows in 2-row chunks (GZ_FP32_CHUNK_ROWS, read at net creation): the last chunk partial
CHUNKED = "6x9_legacy_f40_b2"
# kernel variants (GZ_KERNEL_VARIANT) on the first net at 5 rows: two boards per workgroup, a dead
# board in the last
VARIANTS = [("bf16", v) for v in ("11", "12", "21")] + [("bf16x3", v) for v in ("11", "21", "22", "23", "24", "25")]
# the first SE net at 5 rows under every variant that the v2 kernels of its geometry accept, and in 2-row chunks
SE_VARIED = "se_8x8_f128_b2_s42_pool"
SE_VARIANTS = [("bf16", v, 1) for v in ("11", "12", "21")] + [("bf16x3", v, 3) for v in ("11", "21")]
# the three-role head case at 5 rows and at 2 under every variant, as the first net; the fused large-policy
# cases under the two-board kernel, whose LDS is what decides heads_seq, at 5 rows and at 2
HEAD_VARIED = "head_r3_f128"
HEAD_LARGE_VARIANTS = [(name, mode, "21") for name in ("head_fused_seq_f128", "head_fused_wgfits_f128") for mode in FUSED] + \
                      [("head_fused_p3100_f64", "bf16", "21")]
# one GEMM case at 5 rows in 2-row chunks, in the two layered modes that have the GEMM; and one long-row case
# with the GEMM switched off (GZ_NO_GEMM_HEADS): the plain heads_kernel's Dense on a row longer than 3,072
HEAD_CHUNKED = "head_gemm_r3_3072"
HEAD_NO_GEMM = "head_gemm_lds_3073"
# saturated outputs (test_saturated_outputs): fused (four roles with a P = 1 role and four values; one value
# behind the pooling head; two sigmoids), heads_kernel two-phase, GEMM with the register softmax, GEMM with
# the LDS softmax between two register roles
SATURATED = [("head_r4_f64_v4", "bf16x3"), ("head_v1_vh6_pool", "bf16"), ("head_vh299_sigmoid", "bf16x3"),
             ("head_sep_r3", "bf16x3"), ("head_sep_r3", "fp32-ieee"), ("head_gemm_512_7", "bf16x3"),
             ("head_gemm_mixed", "bf16x3-layered")]
SAT = 2.0 ** 12
LARGE_ROWS = 300       # above large_min_rows() = 257: the large-launch default runs
PROBABILITY = [("8x8_f128_b2", "bf16"), ("8x8_f128_b2", "bf16x3"), ("13x13_f256_b2", "bf16x3"),
               ("10x10_c12_f256_b1_gemm", "bf16x3"), ("v2_8x8_f128_b2_pool", "bf16x3"), ("v2_13x13_f256_b2_concat", "bf16x3"),
               ("19x19_f256_b2", "fp32-ieee"), ("19x19_f256_b2", "bf16-layered"), ("19x19_f256_b2", "bf16x3-layered"),
               ("19x19_f256_b2", "fp16x3-layered"), ("6x9_legacy_f40_b2", "fp32-ieee"),
               # the heads' paths, one each: fused two-phase, fused sequential, heads_kernel two-phase, the GEMM's
               # register softmax, its LDS softmax, heads_kernel_blocked on a long row
               ("head_r4_f64_v4", "bf16x3"), ("head_fused_seq_f128", "bf16"), ("head_sep_r3", "bf16x3"),
               ("head_gemm_r3_3072", "bf16x3"), ("head_gemm_mixed", "bf16x3-layered"), ("head_gemm_lds_3073", "fp32-ieee")]

_cache = {}


def build(name, rows=None):
    """(desc, weights, planes, expected logits) of a case, computed once; rows: another row count on the
    same weights (its planes from their own seed; an SE net's gating scale K is derived from them)."""
    key = (name, rows)
    if key not in _cache:
        c = CASES[name]
        n = rows or (len(c.scales) if c.scales else max(c.rows or ROWS))
        if c.se:
            # every (board, plane) keeps its set bits with a probability of its own: boards filled
            # differently have different gates (test_nn_exact.py::test_liveness)
            x = xl.lattice_planes(c.desc, n, (c.plane_seed or 100) + n, mixed_fill=True)
            w = xl.lattice_se_weights(c.desc, c.seed, x, nnz=c.nnz, wmax=c.wmax, homogeneous=c.homogeneous)
        else:
            w = xl.lattice_weights(c.desc, c.seed, nnz=c.nnz, wmax=c.wmax, wide=c.wide)
            x = xl.lattice_planes(c.desc, n, 100 + n, board_scale=c.scales if not rows else None)
        if c.homogeneous and not c.se:
            w = xl.zero_trunk_shifts(c.desc, w)
        if c.head:
            w = xl.head_last_rows(c.desc, w)
        if c.order:
            x = np.ascontiguousarray(x[list(c.order)])
        _cache[key] = (c.desc, w, x, xl.expected_logits(c.desc, w, x))
    return _cache[key]


def _net(desc, w, device, mode):
    from galvanise_zero_amd._native import HipNet
    net = HipNet(desc, device, mode)
    net.set_weights(to_blob(w))
    net.set_output_logits(True)
    return net


def _assert_exact(tag, net, x, expected, n):
    got = net.forward(x[:n])
    assert len(got) == len(expected)
    for i, (g, e) in enumerate(zip(got, expected)):
        e32 = e[:n].astype(np.float32)
        assert np.array_equal(e32.astype(np.float64), e[:n])
        assert np.array_equal(g, e32), (tag, n, i, int((g != e32).sum()), float(np.abs(g.astype(np.float64) - e[:n]).max()))


@pytest.mark.parametrize("name,mode", [(name, mode) for name, c in CASES.items() for mode in c.modes])
def test_exact(name, mode, hip_device):
    """The logits equal the oracle's, at 1 and 3 rows or at the case's own row counts (scaled boards:
    the four boards in one launch, and each board alone).  Head cases: the dense heads took the path
    the case is there for (HipNet.heads_path), and the large launches the kernel it names."""
    desc, w, x, expected = build(name)
    net = _net(desc, w, hip_device, mode)
    if CASES[name].path:
        assert net.heads_path() == CASES[name].path[mode], (name, mode, net.heads_path())
        assert net.heads_fused() == bool(net.heads_path() & HEADS_FUSED_LARGE)
    if CASES[name].large_kernel:
        assert net.kernel_name(True) == CASES[name].large_kernel[mode], (name, mode, net.kernel_name(True))
    for n in ((x.shape[0], 1) if CASES[name].scales else (CASES[name].rows or ROWS)):
        _assert_exact((name, mode), net, x, expected, n)
    if CASES[name].scales:
        for b in range(1, x.shape[0]):
            _assert_exact((name, mode, "board", b), net, x[b:], [e[b:] for e in expected], 1)
    net.close()


@pytest.mark.parametrize("mode,variant", VARIANTS)
def test_variants(mode, variant, hip_device, monkeypatch):
    desc, w, x, expected = build("8x8_f128_b2", 5)
    monkeypatch.setenv("GZ_KERNEL_VARIANT", variant)
    net = _net(desc, w, hip_device, mode)
    for n in (5, 2):
        _assert_exact((mode, variant), net, x, expected, n)
    net.close()


@pytest.mark.parametrize("mode,variant,parts", SE_VARIANTS)
def test_se_variants(mode, variant, parts, hip_device, monkeypatch):
    """The squeeze-excite net at 5 rows and at 2 under each kernel variant (two boards per workgroup:
    each board its own gates; a dead board in the last workgroup), and the intended kernel ran."""
    desc, w, x, expected = build(SE_VARIED, 5)
    monkeypatch.setenv("GZ_KERNEL_VARIANT", variant)
    net = _net(desc, w, hip_device, mode)
    kernel = "gznn::trunk_kernel_v2<128, 4, %s, %s, %d>" % (variant[0], variant[1], parts)
    assert net.kernel_name(False) == net.kernel_name(True) == kernel
    for n in (5, 2):
        _assert_exact((mode, variant), net, x, expected, n)
    net.close()


@pytest.mark.parametrize("mode,variant", VARIANTS)
def test_head_variants(mode, variant, hip_device, monkeypatch):
    """Three unequal roles at 5 rows and at 2 under each kernel variant: the fused heads of every trunk
    kernel, two boards per workgroup (BPW = 2, a wave group's own board), a dead board in the last."""
    desc, w, x, expected = build(HEAD_VARIED)
    monkeypatch.setenv("GZ_KERNEL_VARIANT", variant)
    net = _net(desc, w, hip_device, mode)
    assert net.heads_path() == BOTH
    for n in (5, 2):
        _assert_exact((HEAD_VARIED, mode, variant), net, x, expected, n)
    net.close()


@pytest.mark.parametrize("name,mode,variant", HEAD_LARGE_VARIANTS)
def test_head_large_variant(name, mode, variant, hip_device, monkeypatch):
    """The fused large-policy cases on the two-board kernel that their large launches take (the kernel
    whose LDS decides between the two-phase and the sequential row), at 5 rows and at 2."""
    desc, w, x, expected = build(name)
    monkeypatch.setenv("GZ_KERNEL_VARIANT", variant)
    net = _net(desc, w, hip_device, mode)
    assert net.heads_path() == CASES[name].path[mode]
    assert net.kernel_name(False) == net.kernel_name(True) == CASES[name].large_kernel[mode]
    for n in (5, 2):
        _assert_exact((name, mode, variant), net, x, expected, n)
    net.close()


@pytest.mark.parametrize("mode", ("bf16-layered", "bf16x3-layered"))
def test_head_gemm_partial_chunk(mode, hip_device, monkeypatch):
    """The policy GEMM's logits scratch and the heads' board indices across chunks: 5 rows in chunks of 2."""
    desc, w, x, expected = build(HEAD_CHUNKED)
    monkeypatch.setenv("GZ_FP32_CHUNK_ROWS", "2")
    net = _net(desc, w, hip_device, mode)
    assert net.heads_path() == HEADS_GEMM
    _assert_exact((HEAD_CHUNKED, mode, "chunks of 2"), net, x, expected, 5)
    net.close()


def test_head_long_row_without_gemm(hip_device, monkeypatch):
    """GZ_NO_GEMM_HEADS: the plain heads_kernel runs the Dense of two policies above 3,072 on the VALU,
    its two-phase LDS row [3076 | 3072 | 256] the longest of the suite."""
    desc, w, x, expected = build(HEAD_NO_GEMM)
    monkeypatch.setenv("GZ_NO_GEMM_HEADS", "1")
    net = _net(desc, w, hip_device, "bf16x3")
    assert net.heads_path() == HEADS_LONG_ROW
    for n in (5, 1):
        _assert_exact((HEAD_NO_GEMM, "no gemm"), net, x, expected, n)
    net.close()


def saturated(name, tie):
    """(desc, weights, planes, expected logits, expected probabilities) of a head case, on the first 5
    boards of its launch at most, with saturated outputs: every role's last policy bias raised by 2^12 (tie: the last column made a copy of the
    first, and both raised), the last value bias raised by 2^12 (a sigmoid net: value 0 raised, the
    last value lowered).  The lattice's logits lie within a few hundred of 0, so in float32 the
    raised column's exp(v - m) is exp(0) = 1, every other's is exp of less than -3,000 = 0, the sum is 1
    (tie: 2, and 1 * 0.5), 1 / (1 + exp(-4096)) = 1 / (1 + 0) = 1 and 1 / (1 + exp(4096)) = 1 / inf = 0."""
    key = (name, "saturated", tie)
    if key not in _cache:
        desc, w, x, _ = build(name)
        x = x[:5]
        w = [(n, a.copy()) for n, a in w]
        wd = dict(w)
        probs = []
        for r, P in enumerate(desc.policy_dist_count):
            k, b = wd["policy%d_dense" % r], wd["policy%d_bias" % r]
            p = np.zeros((x.shape[0], P))
            if tie and P >= 2:
                k[:, -1], b[-1] = k[:, 0], b[0]
                b[0] += SAT
                p[:, 0] = p[:, -1] = 0.5
            else:
                p[:, -1] = 1.0
            b[-1] += SAT
            probs.append(p)
        vb = wd["value_bias"]
        v = np.zeros((x.shape[0], desc.num_values))
        if desc.value_sigmoid:
            vb[0] += SAT
            v[:, 0] = 1.0
            if desc.num_values >= 2:
                vb[-1] -= SAT
        else:
            vb[-1] += SAT
            v[:, -1] = 1.0
        _cache[key] = (desc, w, x, xl.expected_logits(desc, w, x), probs + [v])
    return _cache[key]


@pytest.mark.parametrize("tie", (False, True), ids=("one", "tie"))
@pytest.mark.parametrize("name,mode", SATURATED)
def test_saturated_outputs(name, mode, tie, hip_device):
    """One logit per output 2^12 above the rest, or two tied there: the logits still equal the
    oracle's, and the probabilities are exactly 1 (0.5 and 0.5), 0 everywhere else, the sigmoids
    exactly 1 and 0; a P = 1 role and a V = 1 value are 1.  Nothing is NaN."""
    desc, w, x, expected, probs = saturated(name, tie)
    net = _net(desc, w, hip_device, mode)
    assert net.heads_path() == CASES[name].path[mode]
    for n in (x.shape[0], 1):
        _assert_exact((name, mode, "saturated", tie), net, x, expected, n)
    net.set_output_logits(False)
    for n in (x.shape[0], 1):
        got = net.forward(x[:n])
        for i, (g, p) in enumerate(zip(got, probs)):
            assert not np.isnan(g).any(), (name, mode, i)
            assert np.array_equal(g, p[:n].astype(np.float32)), (name, mode, tie, n, i, int((g != p[:n]).sum()),
                                                                  float(np.abs(g - p[:n]).max()))
    net.close()


def test_large_launch_default(hip_device, monkeypatch):
    """300 rows with no override: the large-launch default (the in-place split kernel) is what runs."""
    desc, w, x, expected = build("8x8_f128_b2", LARGE_ROWS)
    monkeypatch.delenv("GZ_KERNEL_VARIANT", raising=False)
    net = _net(desc, w, hip_device, "bf16x3")
    assert LARGE_ROWS >= net.large_min_rows() == 257
    assert net.kernel_name(True) == "gznn::trunk_kernel_h2i<128, 4, 3>"
    assert net.kernel_name(False) != net.kernel_name(True)
    _assert_exact("large", net, x, expected, LARGE_ROWS)
    net.close()


@pytest.mark.parametrize("mode", LAYERED)
def test_partial_chunk(mode, hip_device, monkeypatch):
    desc, w, x, expected = build(CHUNKED, 5)
    monkeypatch.setenv("GZ_FP32_CHUNK_ROWS", "2")
    net = _net(desc, w, hip_device, mode)
    _assert_exact((mode, "chunks of 2"), net, x, expected, 5)
    net.close()


@pytest.mark.parametrize("mode", LAYERED)
def test_se_partial_chunk(mode, hip_device, monkeypatch):
    """The gate buffer's row indexing across chunks: 5 rows in chunks of 2."""
    desc, w, x, expected = build(SE_VARIED, 5)
    monkeypatch.setenv("GZ_FP32_CHUNK_ROWS", "2")
    net = _net(desc, w, hip_device, mode)
    _assert_exact((mode, "SE, chunks of 2"), net, x, expected, 5)
    net.close()


def _softmax64(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("name,mode", PROBABILITY)
def test_probabilities(name, mode, hip_device):
    """Probability mode on an exact net: the logits are exact there, so what is left is the heads'
    softmax (sigmoid) alone, against the float64 softmax of the expected logits."""
    desc, w, x, expected = build(name)
    net = _net(desc, w, hip_device, mode)
    net.set_output_logits(False)
    got = net.forward(x)
    net.close()
    for i, (g, z) in enumerate(zip(got, expected)):
        value = i == len(expected) - 1
        ref = 1.0 / (1.0 + np.exp(-z)) if (value and desc.value_sigmoid) else _softmax64(z)
        d = np.abs(g.astype(np.float64) - ref)
        r, q = np.clip(ref, 1e-30, None), np.clip(g.astype(np.float64), 1e-30, None)
        kl = 0.0 if (value and desc.value_sigmoid) else float((r * np.log(r / q)).sum(axis=1).max())
        print("exact %s %s out%d softmax alone: max %.3g mean %.3g kl %.3g" % (name, mode, i, d.max(), d.mean(), kl))
        assert d.max() <= DAMPED_TOLERANCE["max"] and d.mean() <= DAMPED_TOLERANCE["mean"] and kl <= DAMPED_TOLERANCE["kl"], \
            (name, mode, i, d.max(), d.mean(), kl)
