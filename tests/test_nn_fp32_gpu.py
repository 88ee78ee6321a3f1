"""GPU tests of the exact-fp32 arithmetic mode ("fp32-ieee", GZ_PRECISION_FP32: every conv on the
f32-input MFMA, layer by layer through device memory; csrc/nn/fp32_forward.hip).

Yardsticks: the float64 oracle oracle/nn_ref.forward, and for accuracy a true IEEE fp32 forward of
the same weights and inputs, oracle/nn_torch.TorchCPUNet (v1 nets), evaluated here.  Bound for the
v1 cases:

    err_hip <= 4 x max(err_torch32, 1e-6)        (max |delta| over all outputs of the case)

4x: a serial k-ordered fmaf chain's rounding error grows like sqrt(K) against a 16-lane blocked
sum's sqrt(K / 16).  The floor is about eight float32 ulps of a probability: near the output quantum
the ratio is noise.  (A serial float32 emulation with two roundings per product gave 0.06-0.57 of
this bound on cfg1 / cfg2 / b2_13x13_f256; torch fp32's own error there is 2.1e-7 .. 1.06e-5.)
v2 nets (TorchCPUNet is v1-only) are compared with the bf16x3 split mode on the same input.
Rows must be bit-identical whatever the batch, segment split or internal row chunking.
"""
import json
import os

import numpy as np
import pytest

from galvanise_zero_amd.nn.desc import BASELINE_CONFIGS, NetDesc
from galvanise_zero_amd.nn.weights import random_planes, random_weights, to_blob
from gpu_helpers import Pinned
from oracle import nn_ref

pytestmark = pytest.mark.gpu

MODE = "fp32-ieee"
TOL_FP32 = (2e-4, 5e-5)   # tests/test_nn_gpu.py's split-mode bound (max |err|, mean |err|)

# tests/test_nn_gpu.py's VARIANTS, the v1 ones this mode is checked on
V1 = {
    "cfg1": BASELINE_CONFIGS[1]["desc"],
    "cfg2": BASELINE_CONFIGS[2]["desc"],
    "leaky_v3_8x8": NetDesc(5, 8, 8, 64, 1, [65, 65], num_values=3, leaky_relu=True),
    "nchw_6x6": NetDesc(5, 6, 6, 128, 1, [81, 81], flatten_nchw=True),
    "legacy_v1_8x8": NetDesc(5, 8, 8, 128, 2, [155, 155], flatten_nchw=True, conv_bias=True, value_bn=True,
                             value_sigmoid=True),
    "b2_13x13_f256": NetDesc(5, 13, 13, 256, 2, [170, 171], flatten_nchw=True),
    "b0_10x10_f256_v3": NetDesc(12, 10, 10, 256, 0, [3041, 3041], num_values=3, leaky_relu=True),
}
with open(os.path.join(os.path.dirname(__file__), "golden", "keras_descs.json")) as _f:
    _FILES = {k: NetDesc(**v["desc"]) for k, v in json.load(_f).items() if "desc" in v}
# tests/test_nn_v2_gpu.py's nets: squeeze-excite + pooling value head, concat-all-layers with padded
# filters / without squeeze-excite, a model file with the pooling value head, and hex19 (19 x 19,
# F = 80 padded, squeeze-excite, concat-all-layers)
V2 = {
    "se21_8x8": (NetDesc(5, 8, 8, 64, 3, [155, 155], resnet_v2=True, se_units=21, global_pooling_value=True,
                         value_bn=True), 7),
    "concat_8x8_f80": (NetDesc(5, 8, 8, 80, 3, [155, 155], value_hidden_size=128, resnet_v2=True, se_units=26,
                               concat_all_layers=True, flatten_nchw=True), 7),
    "concat_13x13_nose": (NetDesc(5, 13, 13, 64, 3, [170, 171], resnet_v2=True, concat_all_layers=True), 7),
    "b1_58_gap": (_FILES["breakthroughSmall/models/b1_58.json"], 7),
    "h2_477_19x19": (_FILES["hex19/models/h2_477.json"], 3),
}
V2_GAMMA = 0.3   # (tests/test_nn_v2_gpu.py: damps the v2 stream's growth)


def _hip(desc, w, device, precision=MODE):
    from galvanise_zero_amd._native import HipNet
    net = HipNet(desc, device, precision)
    net.set_weights(to_blob(w))
    return net


def _maxerr(got, ref):
    return max(float(np.abs(np.asarray(g, np.float64) - np.asarray(r, np.float64)).max()) for g, r in zip(got, ref))


def _check_v1(tag, desc, w, x, net):
    """The bound of the module docstring on one case, plus shapes / finiteness / softmax sums."""
    from oracle.nn_torch import TorchCPUNet
    got = net.forward(x)
    ref = nn_ref.forward(desc, w, x)
    t32 = TorchCPUNet(desc, w).predict_on_batch(x)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and g.dtype == np.float32
        assert np.all(np.isfinite(g))
        if not (desc.value_sigmoid and i == len(got) - 1):
            np.testing.assert_allclose(g.sum(axis=1), 1.0, atol=1e-4)
    e_hip, e_t32 = _maxerr(got, ref), _maxerr(t32, ref)
    bound = 4 * max(e_t32, 1e-6)
    print("%s n=%d: fp32-ieee max err %.3g, torch fp32 %.3g, bound %.3g (%.2f of it)"
          % (tag, x.shape[0], e_hip, e_t32, bound, e_hip / bound))
    assert e_hip <= bound, (tag, x.shape[0], e_hip, e_t32)


@pytest.mark.parametrize("name", list(V1))
def test_v1_parity(name, hip_device):
    desc = V1[name]
    w = random_weights(desc, 7919, bias_std=0.2)
    net = _hip(desc, w, hip_device)
    for n in (1, 7, 19):
        _check_v1(name, desc, w, random_planes(desc, n, 100 + n), net)
    net.close()


def test_v1_parity_bench_weights(hip_device):
    """cfg2 on the bench's weights (seed 7921), a batch past one 128-column tile per 2 boards."""
    desc = V1["cfg2"]
    w = random_weights(desc, 7921)
    net = _hip(desc, w, hip_device)
    _check_v1("cfg2/7921", desc, w, random_planes(desc, 37, 137), net)
    net.close()


@pytest.mark.parametrize("hw", [8, 13])
@pytest.mark.parametrize("C", [3, 15, 24])
def test_initial_conv_widths(C, hw, hip_device):
    """Input planes below, just below and above one 16-channel k-block of the initial conv."""
    desc = NetDesc(C, hw, hw, 64, 1, [hw * hw + 1, hw * hw + 1])
    w = random_weights(desc, 7919, bias_std=0.2)
    net = _hip(desc, w, hip_device)
    _check_v1("C%d_%dx%d" % (C, hw, hw), desc, w, random_planes(desc, 7, 107), net)
    net.close()


def test_mode_is_fp32(hip_device):
    """On the headline net and the bench's weights the mode's error against the float64 oracle is at
    least 4x smaller than bf16x3's on the same batch (a true fp32 forward's is about 35x smaller)."""
    desc = V1["cfg2"]
    w = random_weights(desc, 7921)
    x = random_planes(desc, 256, 5)
    ref = nn_ref.forward(desc, w, x)
    errs = {}
    for precision in (MODE, "bf16x3"):
        net = _hip(desc, w, hip_device, precision)
        errs[precision] = _maxerr(net.forward(x), ref)
        net.close()
    print("cfg2/7921 n=256 max err vs float64: %s" % errs)
    assert 4 * errs[MODE] <= errs["bf16x3"], errs


@pytest.mark.parametrize("name", list(V2))
def test_v2_family(name, hip_device):
    """v2 nets against the split mode: relative logit error at most a quarter of bf16x3's on the
    same input, probabilities within the split mode's stated tolerance."""
    desc, n = V2[name]
    w = random_weights(desc, 7919, bias_std=0.2, res_gamma=V2_GAMMA)
    x = random_planes(desc, n, 100 + n)
    ref_p = nn_ref.forward(desc, w, x)
    ref_z = nn_ref.forward(desc, w, x, logits=True)
    rel = {}
    for precision in (MODE, "bf16x3"):
        net = _hip(desc, w, hip_device, precision)
        if precision == MODE:
            got = net.forward(x)
            for i, (g, r) in enumerate(zip(got, ref_p)):
                assert g.shape == r.shape and np.all(np.isfinite(g))
                d = np.abs(g.astype(np.float64) - r.astype(np.float64))
                print("v2 %s out%d probs: max %.3g mean %.3g" % (name, i, d.max(), d.mean()))
                assert d.max() <= TOL_FP32[0] and d.mean() <= TOL_FP32[1], (name, i, d.max(), d.mean())
        net.set_output_logits(True)
        z = net.forward(x)
        rel[precision] = max(float(np.abs(g.astype(np.float64) - r).max() / max(1.0, np.abs(r).max()))
                             for g, r in zip(z, ref_z))
        net.close()
    print("v2 %s relative logit error: %s" % (name, rel))
    assert rel[MODE] <= 0.25 * rel["bf16x3"], (name, rel)


@pytest.mark.parametrize("name", ["cfg2", "b2_13x13_f256"])
def test_batch_invariance(name, hip_device):
    desc = V1[name]
    net = _hip(desc, random_weights(desc, 3, bias_std=0.2), hip_device)
    x = random_planes(desc, 64, 9)
    full = net.forward(x)
    perm = np.random.default_rng(0).permutation(64)[:37]
    for a, b in zip(full, net.forward(x[perm])):
        assert np.array_equal(a[perm], b)
    for a, b in zip(full, net.forward(x[5:6])):
        assert np.array_equal(a[5:6], b)
    net.close()


@pytest.mark.parametrize("placement", ["device", "pinned"])
@pytest.mark.parametrize("name", ["cfg2", "b2_13x13_f256"])
def test_segments_match_forward(name, placement, hip_device):
    """forward_segments over odd-sized segments (an empty one among them) in device or pinned host
    memory equals a forward of each segment alone, bit for bit."""
    import torch
    desc = V1[name]
    net = _hip(desc, random_weights(desc, 7921), hip_device)
    C, H, W = desc.input_channels, desc.input_columns, desc.input_rows
    P, V = list(desc.policy_dist_count), desc.num_values
    sizes = (37, 0, 129, 1)
    xs = [random_planes(desc, n, 50 + i) if n else np.zeros((0, C, H, W), np.float32) for i, n in enumerate(sizes)]
    keep, segs, outs = [], [], []
    for x in xs:
        n = x.shape[0]
        if placement == "device":
            tp = torch.from_numpy(x.reshape(-1).copy()).cuda() if n else torch.zeros(1, device="cuda")
            tpol = [torch.full((max(1, n * p),), -1.0, device="cuda") for p in P]
            tval = torch.full((max(1, n * V),), -1.0, device="cuda")
            keep += [tp, tval] + tpol
            segs.append((n, tp.data_ptr(), [t.data_ptr() for t in tpol], tval.data_ptr()))
            outs.append((tpol, tval))
        else:
            bp = Pinned(x.size)
            bp.a[:] = x.reshape(-1)
            bpol = [Pinned(n * p) for p in P]
            bval = Pinned(n * V)
            for b in bpol + [bval]:
                b.a[:] = -1.0
            keep += [bp, bval] + bpol
            segs.append((n, bp.ptr.value, [b.ptr.value for b in bpol], bval.ptr.value))
            outs.append((bpol, bval))
    net.forward_segments(torch.cuda.current_stream().cuda_stream, segs)
    torch.cuda.synchronize()
    for x, (pol, val) in zip(xs, outs):
        n = x.shape[0]
        if n == 0:
            continue
        ref = net.forward(x)
        if placement == "device":
            got = [t[:n * p].cpu().numpy().reshape(n, p) for t, p in zip(pol, P)] + [val[:n * V].cpu().numpy().reshape(n, V)]
        else:
            got = [b.a.reshape(n, p).copy() for b, p in zip(pol, P)] + [val.a.reshape(n, V).copy()]
        for g, r in zip(got, ref):
            assert np.array_equal(g, r)
    net.close()
    if placement == "pinned":
        for b in keep:
            b.free()


@pytest.mark.parametrize("name", ["cfg2", "b2_13x13_f256"])
def test_row_chunks_invariant(name, hip_device, monkeypatch):
    """A launch that crosses the internal row-chunk boundary (GZ_FP32_CHUNK_ROWS, read at net
    creation: 5-row chunks here, the last one partial) equals its two halves and an unchunked net."""
    desc = V1[name]
    w = random_weights(desc, 3, bias_std=0.2)
    x = random_planes(desc, 13, 21)
    whole = _hip(desc, w, hip_device)
    base = whole.forward(x)
    whole.close()
    monkeypatch.setenv("GZ_FP32_CHUNK_ROWS", "5")
    net = _hip(desc, w, hip_device)
    monkeypatch.delenv("GZ_FP32_CHUNK_ROWS")
    full = net.forward(x)
    halves = [net.forward(x[:6]), net.forward(x[6:])]
    net.close()
    for i, (a, b) in enumerate(zip(full, base)):
        assert np.array_equal(a, b)
        assert np.array_equal(a, np.concatenate([halves[0][i], halves[1][i]]))


WEIGHT_NETS = {
    "cfg1_v1": BASELINE_CONFIGS[1]["desc"],
    "x6_102_legacy": _FILES["breakthrough/models/x6_102.json"],
    "concat_8x8_f80_se": V2["concat_8x8_f80"][0],
}


@pytest.mark.parametrize("name", sorted(WEIGHT_NETS))
def test_device_roll_image_identical(name, hip_device):
    """gz_net_set_weights_device builds the byte-identical fp32 image from a device blob."""
    import torch
    desc = WEIGHT_NETS[name]
    blob = to_blob(random_weights(desc, 7922, bias_std=0.2))
    from galvanise_zero_amd._native import HipNet
    host = HipNet(desc, hip_device, MODE)
    host.set_weights(blob)
    dev = HipNet(desc, hip_device, MODE)
    t = torch.from_numpy(blob).to("cuda")
    torch.cuda.synchronize()
    dev.set_weights_device(t.data_ptr(), t.numel())
    a, b = host.weight_image(), dev.weight_image()
    assert a.size == b.size and a.size > 0
    diff = np.flatnonzero(a != b)
    assert diff.size == 0, "%d bytes differ of %d; first: %s" % (
        diff.size, a.size, [(int(i), int(a[i]), int(b[i])) for i in diff[:12]])
    x = random_planes(desc, 5, 3)
    for u, v in zip(host.forward(x), dev.forward(x)):
        assert np.array_equal(u, v)
    host.close()
    dev.close()


def test_second_set_weights_takes_effect(hip_device):
    desc = V1["cfg1"]
    w1, w2 = random_weights(desc, 1, bias_std=0.2), random_weights(desc, 2, bias_std=0.2)
    x = random_planes(desc, 7, 4)
    net = _hip(desc, w1, hip_device)
    first = net.forward(x)
    net.set_weights(to_blob(w2))
    second = net.forward(x)
    assert any(not np.array_equal(a, b) for a, b in zip(first, second))
    _check_v1("cfg1/second weights", desc, w2, x, net)
    net.close()


def test_queries(hip_device):
    """The diagnostics / runner queries of the mode (include/gzero_nn.h)."""
    desc = V1["cfg2"]
    net = _hip(desc, random_weights(desc, 1), hip_device)
    assert not net.heads_fused()
    assert net.kernel_name(False) == net.kernel_name(True) == "gzfp32::conv_f32_kernel<4>"
    assert net.large_min_rows() > 0 and net.wave_rows() > 0
    assert net.flops_per_eval() == pytest.approx(desc.flops_per_eval())
    with pytest.raises(RuntimeError):
        net.stamp_avg()
    net.close()
