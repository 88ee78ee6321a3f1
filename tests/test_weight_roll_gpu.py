"""The generation roll's weight load on the device (the reference swaps networks between poll loops:
worker.py:138-160, cppinterface.py:146-147; here the new blob arrives in HBM by an RCCL broadcast,
SURVEY 8e): gz_net_set_weights_device folds BatchNorm and packs the bf16 hi / lo MFMA fragments with
HIP kernels reading the blob in place.  Both paths run one job list (csrc/nn/weight_image.h: the blob
plan, the image layout, the element functions), the host path (gz_net_set_weights) on the CPU, the
device path as kernels over the same element functions.  The device path must build exactly the
image the host path builds -- byte for byte, so every forward is bit-identical whichever way the
weights arrived -- for every head and trunk kind: v1 / legacy (conv biases, value BN, sigmoid), v2
(squeeze-excite, pooling and concat-all-layers value heads), large policies (the split GEMM heads'
fragments), every arithmetic mode, padded filter counts; and the host path's image must be the one
recorded before the two packers became one (tests/golden/weight_image_sha256.json)."""
import hashlib
import json
import os
import time

import numpy as np
import pytest

from galvanise_zero_amd.nn.desc import BASELINE_CONFIGS, NetDesc
from galvanise_zero_amd.nn.weights import random_planes, random_weights, to_blob

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(__file__), "golden", "keras_descs.json")) as _f:
    _FILES = {k: NetDesc(**v["desc"]) for k, v in json.load(_f).items() if "desc" in v}

NETS = {
    "cfg2": BASELINE_CONFIGS[2]["desc"],
    "cfg4": BASELINE_CONFIGS[4]["desc"],
    "cfg5": BASELINE_CONFIGS[5]["desc"],
    "x6_102_legacy": _FILES["breakthrough/models/x6_102.json"],
    "b1_58_v2_gap": _FILES["breakthroughSmall/models/b1_58.json"],
    "f1_581_v2_k0_160": _FILES["draughts_killer/models/f1_581.json"],
    "h2_477_v2_concat_19x19": _FILES["hex19/models/h2_477.json"],
    "v3_leaky_f96": NetDesc(5, 8, 8, 96, 2, [65, 65], num_values=3, leaky_relu=True, flatten_nchw=True),
}
PRECISIONS = ("bf16", "bf16x3", "fp32-ieee")
DIGESTS = os.path.join(os.path.dirname(__file__), "golden", "weight_image_sha256.json")
_MIB = 1 << 20


def image_digest(image):
    """SHA-256 of a weight image and, to place a difference, 12 hex digits of it per MiB block."""
    b = memoryview(np.ascontiguousarray(image, dtype=np.uint8)).cast("B")
    return {"bytes": len(b), "sha256": hashlib.sha256(b).hexdigest(),
            "blocks": [hashlib.sha256(b[o:o + _MIB]).hexdigest()[:12] for o in range(0, len(b), _MIB)]}


def image_layout(desc, precision, FP, gemm_heads):
    """[(tensor, byte offset)] of the device weight image in order, and its size: csrc/nn/weight_image.h
    image_layout for FP padded filters (diagnostics: names the tensor a differing byte lies in)."""
    d, fp32, P2 = desc, precision == "fp32-ieee", 2 if precision == "bf16x3" else 1
    B, R, S, HW, T0 = d.residual_layers, d.role_count, d.se_units, d.hw, d.initial_kernel ** 2
    NL = B + 1 if d.concat_all_layers else 0
    n_w0 = T0 * ((d.input_channels + 15) // 16 * 16) * FP if fp32 else (T0 * d.input_channels + 31) // 32 * 32 * FP
    wb = 4 if fp32 else 2
    sizes = [("w0", n_w0 * wb), ("w0lo", (n_w0 if P2 == 2 else 1) * 2), ("b0", FP * 4),
             ("wres", P2 * 2 * B * 9 * FP * FP * wb), ("bres", 2 * B * FP * 4), ("wh", (2 * R + 1) * FP * 4),
             ("bh", (2 * R + 1) * 4), ("wcl", max(NL, 1) * FP * 4), ("bcl", max(NL, 1) * 4)]
    for r, p in enumerate(d.policy_dist_count):
        sizes += [("pd%d" % r, 2 * HW * ((p + 3) & ~3) * 4), ("pb%d" % r, p * 4)]
    VH = d.value_hidden_size
    sizes += [("vhw", d.value_features * ((VH + 3) & ~3) * 4), ("vhb", VH * 4),
              ("pre", (2 * B * FP if d.resnet_v2 else 1) * 4), ("sew1", (B * FP * S if S else 1) * 4),
              ("sew2", (B * S * FP if S else 1) * 4), ("vdw", VH * d.num_values * 4), ("vdb", d.num_values * 4)]
    if gemm_heads:
        sizes += [("pdp%d" % r, (p + 15) // 16 * ((2 * HW + 31) // 32) * 2 * 64 * 8 * 2)
                  for r, p in enumerate(d.policy_dist_count)]
    out, off = [], 0
    for name, n in sizes:
        out.append((name, off))
        off = (off + n + 255) & ~255
    return out, off


def tensor_at(desc, precision, size, offset):
    """The tensor of a `size`-byte image that byte `offset` lies in (the padded filter count and the
    GEMM heads' fragments, which the library chooses, are found by the size)."""
    for FP in (64, 128, 256):
        for gemm in (False, True):
            lay, total = image_layout(desc, precision, FP, gemm)
            if FP >= desc.cnn_filter_size and total == size:
                return [n for n, o in lay if o <= offset][-1]
    return "? (no layout of %d bytes)" % size


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_device_roll_image_identical(name, precision, hip_device):
    import torch
    from galvanise_zero_amd._native import HipNet
    desc = NETS[name]
    blob = to_blob(random_weights(desc, 7922, bias_std=0.2))
    host = HipNet(desc, hip_device, precision)
    host.set_weights(blob)
    dev = HipNet(desc, hip_device, precision)
    t = torch.from_numpy(blob).to("cuda")
    torch.cuda.synchronize()
    dev.set_weights_device(t.data_ptr(), t.numel())
    a, b = host.weight_image(), dev.weight_image()
    assert a.size == b.size and a.size > 0
    diff = np.flatnonzero(a != b)
    assert diff.size == 0, "%d bytes differ of %d; first: %s" % (
        diff.size, a.size, [(int(i), int(a[i]), int(b[i])) for i in diff[:12]])
    x = random_planes(desc, 9, 3)
    for u, v in zip(host.forward(x), dev.forward(x)):
        assert np.array_equal(u, v)
    print("%s %s: %d-byte image identical; device fold + pack %.3f ms" % (name, precision, a.size, dev.last_roll_ms()))
    host.close()
    dev.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", sorted(NETS))
def test_host_image_is_the_recorded_one(name, precision, hip_device):
    """The host path's image against tests/golden/weight_image_sha256.json, recorded by
    tools/record_weight_image_digests.py on the build before the two packers became one job list:
    with test_device_roll_image_identical (here and in tests/test_nn_fp32_gpu.py) this pins both
    paths' images to that build's, byte for byte."""
    from galvanise_zero_amd._native import HipNet
    with open(DIGESTS) as f:
        want = json.load(f)["%s/%s" % (name, precision)]
    desc = NETS[name]
    net = HipNet(desc, hip_device, precision)
    net.set_weights(to_blob(random_weights(desc, 7922, bias_std=0.2)))
    got = image_digest(net.weight_image())
    net.close()
    if got != want:
        print("%s %s: image of %d bytes, recorded %d" % (name, precision, got["bytes"], want["bytes"]))
        for i, (a, b) in enumerate(zip(got["blocks"], want["blocks"])):
            if a != b:
                print("first differing MiB block %d: in tensor %s" % (i, tensor_at(desc, precision, got["bytes"], i * _MIB)))
                break
    assert got["bytes"] == want["bytes"]
    assert got["sha256"] == want["sha256"]


def test_device_roll_orders_after_async_copy(hip_device):
    """gz_net_set_weights_device needs no caller-side synchronisation: the blob is
    written by an asynchronous pinned-host copy on torch's current stream, with no
    torch.cuda.synchronize() before the call (and a large unrelated copy queued ahead of it, so the
    blob is still in flight when the call starts); the packed image must equal the host path's."""
    import torch
    from galvanise_zero_amd._native import HipNet
    desc = NETS["cfg5"]
    blob = to_blob(random_weights(desc, 7923))
    host = HipNet(desc, hip_device, "bf16x3")
    host.set_weights(blob)
    dev = HipNet(desc, hip_device, "bf16x3")
    for _ in range(3):
        pinned = torch.from_numpy(blob).pin_memory()
        ballast = torch.empty(1 << 28, dtype=torch.uint8).pin_memory()
        d_ballast = torch.empty_like(ballast, device="cuda")
        t = torch.zeros(blob.size, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        d_ballast.copy_(ballast, non_blocking=True)   # 256 MB ahead of the blob on the same stream
        t.copy_(pinned, non_blocking=True)
        dev.set_weights_device(t.data_ptr(), t.numel())
        a, b = host.weight_image(), dev.weight_image()
        assert np.array_equal(a, b), "%d bytes differ" % np.count_nonzero(a != b)
    host.close()
    dev.close()


def test_device_roll_faster_than_round_trip(hip_device, monkeypatch):
    """The device fold / pack against the round trip it replaces (D2H copy of the blob, host fold and
    pack, H2D upload; GZ_HOST_WEIGHT_ROLL=1), on amazons' 20 x 256 net (cfg5: 24.9 M parameters)."""
    import torch
    from galvanise_zero_amd._native import HipNet
    desc = NETS["cfg5"]
    blob = to_blob(random_weights(desc, 7922))
    t = torch.from_numpy(blob).to("cuda")
    net = HipNet(desc, hip_device, "bf16x3")
    times = {}
    for mode in ("device", "round_trip"):
        if mode == "round_trip":
            monkeypatch.setenv("GZ_HOST_WEIGHT_ROLL", "1")
        best = 1e9
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            net.set_weights_device(t.data_ptr(), t.numel())
            best = min(best, time.perf_counter() - t0)
        times[mode] = best * 1e3
    print("cfg5 weight roll: device %.1f ms (kernels %.2f ms), round trip %.1f ms" %
          (times["device"], net.last_roll_ms(), times["round_trip"]))
    assert times["device"] < times["round_trip"]
    net.close()
