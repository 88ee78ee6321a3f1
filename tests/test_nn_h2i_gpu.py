"""The in-place split trunk kernel (variant 25, trunk_kernel_h2i: variant 23's two groups of two
waves with one LDS image per board, overwritten in place, in 256 registers per wave, so two
workgroups are resident per CU) computes every row exactly as variants 21 and 23 do, alone and with
co-resident workgroups; it is the large-launch default where two of its workgroups fit the LDS
(split F = 128 nets of up to 8 residual blocks) and nowhere else."""
import dataclasses

import numpy as np
import pytest

from galvanise_zero_amd.nn.desc import BASELINE_CONFIGS, NetDesc
from galvanise_zero_amd.nn.tolerance import SPLIT_TOLERANCE
from galvanise_zero_amd.nn.weights import random_planes, random_weights, to_blob
from gpu_helpers import err, kl
from oracle import nn_ref
from test_bench_shape_gpu import _segmented_forward

pytestmark = pytest.mark.gpu

H2I = "gznn::trunk_kernel_h2i<128, %d, 3>"
# 8 x 8: four full position tiles; 6 x 7: three, the last partial (its off-board lanes store to the
# scratch row); 5 x 5: two, the last partial.  12 input channels: the 8 x 8 staging scratch (36,352 B)
# then covers the image's zero rows, which must be zeroed after it.
BOARDS = {"8x8": (8, 8, [155, 155]), "6x7": (6, 7, [85, 86]), "5x5": (5, 5, [51, 50])}
ROWS = (1, 2, 3, 5)   # a dead second board; one full workgroup; a half-full second / third workgroup


def _variant_net(monkeypatch, desc, w, variant, device):
    from galvanise_zero_amd._native import HipNet
    if variant is None:
        monkeypatch.delenv("GZ_KERNEL_VARIANT", raising=False)
    else:
        monkeypatch.setenv("GZ_KERNEL_VARIANT", variant)
    net = HipNet(desc, device, "bf16x3")
    net.set_weights(w)
    return net


@pytest.mark.parametrize("blocks", [0, 1, 2, 6])
@pytest.mark.parametrize("board", list(BOARDS))
def test_rows_identical_to_variants_21_and_23(board, blocks, hip_device, monkeypatch):
    h, w_, pol = BOARDS[board]
    desc = NetDesc(12, h, w_, 128, blocks, pol)
    w = to_blob(random_weights(desc, 5, bias_std=0.2))
    x = random_planes(desc, max(ROWS), 4)
    nets = {v: _variant_net(monkeypatch, desc, w, v, hip_device) for v in ("21", "23", "25")}
    assert nets["25"].kernel_name(True) == H2I % ((h * w_ + 15) // 16)
    for n in ROWS:
        outs = {v: net.forward(x[:n]) for v, net in nets.items()}
        for ref in ("21", "23"):
            for a, b in zip(outs[ref], outs["25"]):
                assert np.array_equal(a, b), (board, blocks, n, ref)
    for net in nets.values():
        net.close()


def test_coresident_workgroups_and_repeated_launches(hip_device, monkeypatch):
    """1,030 rows of the 2-block net = 515 workgroups on 256 CUs, so two run side by side on some CUs,
    each overwriting its images in place at its own pace; three uneven segments; 20 launches back to
    back, every one identical to the first and to variant 23's (a missing barrier between a conv's
    last read of the image and its epilogue's stores would show here)."""
    desc = NetDesc(12, 8, 8, 128, 2, [155, 155])
    w = to_blob(random_weights(desc, 5, bias_std=0.2))
    sizes = [401, 7, 622]
    x = random_planes(desc, sum(sizes), 6)
    ref_net = _variant_net(monkeypatch, desc, w, "23", hip_device)
    ref = _segmented_forward(ref_net, desc, x, sizes)
    ref_net.close()
    net = _variant_net(monkeypatch, desc, w, "25", hip_device)
    assert net.workgroups_per_cu() == 2
    for it in range(20):
        got = _segmented_forward(net, desc, x, sizes)
        for i, (g, r) in enumerate(zip(got, ref)):
            assert np.array_equal(g, r), (it, i)
    net.close()


def test_cfg2_tolerance_and_queries(hip_device, monkeypatch):
    """cfg2 on the bench's weights at one full round of the variant (1,024 rows) against the float64
    oracle, within the stated split tolerance; and what the variant reports about itself."""
    desc = BASELINE_CONFIGS[2]["desc"]
    w = random_weights(desc, 7921)
    net = _variant_net(monkeypatch, desc, to_blob(w), "25", hip_device)
    assert net.kernel_name(True) == H2I % 4
    assert net.heads_fused()
    assert net.workgroups_per_cu() == 2
    assert net.wave_rows() == 1024
    x = random_planes(desc, 1024, 11)
    got = net.forward(x)
    ref = nn_ref.forward(desc, w, x)
    tol = SPLIT_TOLERANCE["cfg2"]
    for i, (g, r) in enumerate(zip(got, ref)):
        assert np.all(np.isfinite(g)), i
        e, k = err(g, r), kl(r, g)
        print("h2i cfg2 out%d: max %.3g mean %.3g kl %.3g" % (i, e[0], e[1], k))
        assert e[0] <= tol["max"] and e[1] <= tol["mean"], (i, e)
        assert k <= tol["kl"], (i, k)
    net.close()


def test_default_selection(hip_device, monkeypatch):
    """Large launches of cfg2 (6 blocks: two workgroups' LDS fit a CU) run the in-place kernel; a
    10-block 8 x 8 net (bias table too large for two workgroups) stays on trunk_kernel_h2; small
    launches keep the one-board kernel in both."""
    cfg2 = BASELINE_CONFIGS[2]["desc"]
    deep = dataclasses.replace(cfg2, residual_layers=10)
    small = "gznn::trunk_kernel<128, 4, 1, 1, 3>"
    for desc, large, wgs in ((cfg2, H2I % 4, 2), (deep, "gznn::trunk_kernel_h2<128, 4, 3>", 1)):
        w = to_blob(random_weights(desc, 3, bias_std=0.1, res_gamma=0.15 if desc.residual_layers > 6 else 1.0))
        net = _variant_net(monkeypatch, desc, w, None, hip_device)
        assert net.kernel_name(True) == large
        assert net.kernel_name(False) == small
        assert net.workgroups_per_cu() == wgs
        assert net.wave_rows() == 512 * wgs
        assert net.large_min_rows() == 257
        assert net.heads_fused()
        net.close()
