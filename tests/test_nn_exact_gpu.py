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
gate and apply kernels, under each kernel variant and across row chunks.  Left to the tolerance
tests: leaky nets, the pooling value head on boards whose position count is no power of two
(exact_lattice's docstring: the channel mean multiplies by fl32(1 / npos), forward_kernel.h
"sm[r] * inv"), and small errors in the scale of the squeeze-excite mean on such boards, which a
saturated gate cannot see by construction.
"""
import dataclasses

import numpy as np
import pytest

import exact_lattice as xl
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
# one net at 5 rows in 2-row chunks (GZ_FP32_CHUNK_ROWS, read at net creation): the last chunk partial
CHUNKED = "6x9_legacy_f40_b2"
# kernel variants (GZ_KERNEL_VARIANT) on the first net at 5 rows: two boards per workgroup, a dead
# board in the last
VARIANTS = [("bf16", v) for v in ("11", "12", "21")] + [("bf16x3", v) for v in ("11", "21", "22", "23", "24", "25")]
# the first SE net at 5 rows under every variant that the v2 kernels of its geometry accept, and in 2-row chunks
SE_VARIED = "se_8x8_f128_b2_s42_pool"
SE_VARIANTS = [("bf16", v, 1) for v in ("11", "12", "21")] + [("bf16x3", v, 3) for v in ("11", "21")]
LARGE_ROWS = 300       # above large_min_rows() = 257: the large-launch default runs
PROBABILITY = [("8x8_f128_b2", "bf16"), ("8x8_f128_b2", "bf16x3"), ("13x13_f256_b2", "bf16x3"),
               ("10x10_c12_f256_b1_gemm", "bf16x3"), ("v2_8x8_f128_b2_pool", "bf16x3"), ("v2_13x13_f256_b2_concat", "bf16x3"),
               ("19x19_f256_b2", "fp32-ieee"), ("19x19_f256_b2", "bf16-layered"), ("19x19_f256_b2", "bf16x3-layered"),
               ("19x19_f256_b2", "fp16x3-layered"), ("6x9_legacy_f40_b2", "fp32-ieee")]

_cache = {}


def build(name, rows=None):
    """(desc, weights, planes, expected logits) of a case, computed once; rows: another row count on the
    same weights (its planes from their own seed; an SE net's gating scale K is derived from them)."""
    key = (name, rows)
    if key not in _cache:
        c = CASES[name]
        n = rows or (len(c.scales) if c.scales else max(ROWS))
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
    """The logits equal the oracle's, at 1 and 3 rows (scaled boards: the four boards in one launch,
    and each board alone)."""
    desc, w, x, expected = build(name)
    net = _net(desc, w, hip_device, mode)
    for n in ((x.shape[0], 1) if CASES[name].scales else ROWS):
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
