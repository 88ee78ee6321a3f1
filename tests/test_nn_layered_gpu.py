"""GPU parity of the layered arithmetic modes ("bf16-layered" / "bf16x3-layered": fp32-ieee's
layer-by-layer trunk with gzlayered::conv_bf16_kernel on the bf16 MFMA, layered_forward.hip) against
the float64 oracle (oracle/nn_ref.forward), on nets the fused modes refuse and on nets both run.

Nets (weights random_weights(desc, 7919, bias_std=0.2, res_gamma=0.3) as in test_nn_v2_f256_gpu.py):
19 x 19 with 256 filters (v2 with squeeze-excite and the pooling value head; v1 with 15 planes, a
3 x 3 initial conv and 192 -> 256 filters): partial last tiles, tiles that straddle boards; 13 x 13
v1 with 14 blocks, one past the fused modes' limit; and four nets the fused modes run too: 13 x 13
concat_all_layers, 10 x 10 amazons (the policy GEMM beside the layered trunk, 3 values), a
non-square 6 x 9 legacy net (40 -> 64 filters) and BASELINE cfg2's net with 2 blocks.

Bounds:
  bf16x3-layered  relative logit error <= test_nn_v2_f256_gpu.LOGITS_TOL (1.2e-4), probabilities
                  within tolerance.DAMPED_TOLERANCE; on the nets the fused bf16x3 runs, at 7 rows,
                  also <= 3 x the fused mode's relative logit error on the same weights and rows
  bf16-layered    per output max / mean <= max(test_nn_v2_gpu.TOL_V2_BF16, 3 x the fused bf16
                  error on the same rows); on the new geometries the fused twin is the same desc at
                  128 filters (19 x 19) or at 13 blocks (13x13_v1_b14)
Every row's outputs are bit-identical whatever the launch, the segment split or the row chunk.
"""
import dataclasses

import numpy as np
import pytest

from galvanise_zero_amd.nn.desc import BASELINE_CONFIGS, NetDesc
from galvanise_zero_amd.nn.tolerance import DAMPED_TOLERANCE
from galvanise_zero_amd.nn.weights import random_planes, random_weights, to_blob
from gpu_helpers import Pinned
from test_nn_v2_f256_gpu import (LOGITS_TOL, NETS as F256_NETS, POOLED, RES_GAMMA, TOL_V2_BF16, _case, _hip, _logit_error,
                                 _prob_errors, _twin)

pytestmark = pytest.mark.gpu

SPLIT, BF16 = "bf16x3-layered", "bf16-layered"
# name -> (desc, rows); the first three are refused by both fused modes, the BOTH four are not
NETS = {
    "19x19_f256_se85": (NetDesc(5, 19, 19, 256, 2, [362, 362], se_units=85, **POOLED), (1, 3)),
    "19x19_v1_f192_c15": (NetDesc(15, 19, 19, 192, 2, [362, 362]), (1, 3)),
    "13x13_v1_b14": (NetDesc(5, 13, 13, 256, 14, [170, 171]), (2,)),
    "13x13_f256_concat": (F256_NETS["13x13_f256_concat"], (1, 7)),
    "10x10_f192_amazons": (F256_NETS["10x10_f192_amazons"], (1, 7)),
    "6x9_legacy_f40": (NetDesc(4, 6, 9, 40, 2, [55, 54], value_hidden_size=48, flatten_nchw=True, conv_bias=True,
                               value_bn=True, value_sigmoid=True), (1, 7)),
    "8x8_cfg2_b2": (dataclasses.replace(BASELINE_CONFIGS[2]["desc"], residual_layers=2), (1, 7)),
}
BOTH = ("13x13_f256_concat", "10x10_f192_amazons", "6x9_legacy_f40", "8x8_cfg2_b2")


def _bf16_twin(name):
    """The net whose fused bf16 error sets the bf16-layered bound: the net itself where the fused
    mode runs it, else its 128-filter twin, or 13 of the 14 blocks."""
    desc = NETS[name][0]
    if name in BOTH:
        return desc
    return dataclasses.replace(desc, residual_layers=13) if name == "13x13_v1_b14" else _twin(desc)


@pytest.mark.parametrize("name", sorted(NETS))
def test_split_layered(name, hip_device):
    """bf16x3-layered: relative logit error within the 256-filter configs' bound, probabilities within
    the damped-weights bound; where the fused bf16x3 runs the net, within 3 x its logit error at 7 rows."""
    desc, rows = NETS[name]
    for n in rows:
        w, x, ref_p, ref_z = _case(desc, n)
        net = _hip(desc, w, hip_device, SPLIT)
        errs = _prob_errors(name, SPLIT, n, net.forward(x), ref_p)
        rel = _logit_error(name, SPLIT, n, net, x, ref_z)
        net.close()
        assert rel <= LOGITS_TOL, (name, n, rel)
        for i, (mx, mean, kl) in enumerate(errs):
            assert mx <= DAMPED_TOLERANCE["max"] and mean <= DAMPED_TOLERANCE["mean"] and kl <= DAMPED_TOLERANCE["kl"], \
                (name, n, i, mx, mean, kl)
        if name in BOTH and n == 7:
            fused = _hip(desc, w, hip_device, "bf16x3")
            frel = _logit_error(name, "bf16x3", n, fused, x, ref_z)
            fused.close()
            assert rel <= 3 * frel, (name, n, rel, frel)


@pytest.mark.parametrize("name", sorted(NETS))
def test_bf16_layered(name, hip_device):
    """bf16-layered: per output within max(TOL_V2_BF16, 3 x the fused bf16 error of the net or its
    twin on the same rows)."""
    desc, rows = NETS[name]
    twin = _bf16_twin(name)
    for n in rows:
        w, x, ref_p, _ = _case(desc, n)
        tw, tx, tref_p, _ = _case(twin, n)
        tnet = _hip(twin, tw, hip_device, "bf16")
        terrs = _prob_errors(name + ("/fused" if twin is desc else "/twin"), "bf16", n, tnet.forward(tx), tref_p)
        tnet.close()
        net = _hip(desc, w, hip_device, BF16)
        errs = _prob_errors(name, BF16, n, net.forward(x), ref_p)
        net.close()
        for i, ((mx, mean, _), (tmx, tmean, _)) in enumerate(zip(errs, terrs)):
            assert mx <= max(TOL_V2_BF16[0], 3 * tmx) and mean <= max(TOL_V2_BF16[1], 3 * tmean), \
                (name, n, i, (mx, mean), (tmx, tmean))


@pytest.mark.parametrize("precision", [BF16, SPLIT])
def test_batch_and_chunk_invariance(precision, hip_device, monkeypatch):
    """A row does not depend on the launch it runs in (300 rows, a permuted 37-row subset, a single
    row), nor on the internal row chunks (GZ_FP32_CHUNK_ROWS, read at net creation: 5-row chunks,
    the last one partial)."""
    desc = F256_NETS["13x13_f256_se85"]
    w = random_weights(desc, 3, bias_std=0.2, res_gamma=RES_GAMMA)
    net = _hip(desc, w, hip_device, precision)
    x = random_planes(desc, 300, 9)
    full = net.forward(x)
    perm = np.random.default_rng(0).permutation(300)[:37]
    for a, b in zip(full, net.forward(x[perm])):
        assert np.array_equal(a[perm], b)
    for a, b in zip(full, net.forward(x[5:6])):
        assert np.array_equal(a[5:6], b)
    net.close()
    monkeypatch.setenv("GZ_FP32_CHUNK_ROWS", "5")
    chunked = _hip(desc, w, hip_device, precision)
    for a, b in zip(full, chunked.forward(x[perm])):
        assert np.array_equal(a[perm], b)
    chunked.close()


def test_segments_match_forward(hip_device):
    """forward_segments (the runner's call path) over three pinned-host segments of 5, 1 and 9 rows
    equals one flat forward of the same 15 rows, bit for bit."""
    import torch
    desc = NETS["19x19_f256_se85"][0]
    net = _hip(desc, random_weights(desc, 7921, bias_std=0.2, res_gamma=RES_GAMMA), hip_device, SPLIT)
    P, V = list(desc.policy_dist_count), desc.num_values
    x = random_planes(desc, 15, 57)
    keep, segs, outs, row = [], [], [], 0
    for n in (5, 1, 9):
        bp = Pinned(x[row:row + n].size)
        bp.a[:] = x[row:row + n].reshape(-1)
        bpol = [Pinned(n * p) for p in P]
        bval = Pinned(n * V)
        for b in bpol + [bval]:
            b.a[:] = -1.0
        keep += [bp, bval] + bpol
        segs.append((n, bp.ptr.value, [b.ptr.value for b in bpol], bval.ptr.value))
        outs.append((n, bpol, bval))
        row += n
    net.forward_segments(torch.cuda.current_stream().cuda_stream, segs)
    torch.cuda.synchronize()
    flat = net.forward(x)
    row = 0
    for n, pol, val in outs:
        got = [b.a.reshape(n, p).copy() for b, p in zip(pol, P)] + [val.a.reshape(n, V).copy()]
        for g, r in zip(got, flat):
            assert np.array_equal(g, r[row:row + n])
        row += n
    net.close()
    for b in keep:
        b.free()


@pytest.mark.parametrize("fused,layered", [("bf16x3", SPLIT), ("bf16", BF16)])
def test_weight_image(fused, layered, hip_device):
    """The layered mode's weight image is the fused mode's, byte for byte, whether packed on the host
    (set_weights) or by the device roll (set_weights_device): a padded 192 -> 256 filter v2 net with
    the GEMM heads."""
    import torch
    from galvanise_zero_amd._native import HipNet
    desc = F256_NETS["10x10_f192_amazons"]
    blob = to_blob(random_weights(desc, 7919, bias_std=0.2, res_gamma=RES_GAMMA))
    ref = HipNet(desc, hip_device, fused)
    ref.set_weights(blob)
    host = HipNet(desc, hip_device, layered)
    host.set_weights(blob)
    dev = HipNet(desc, hip_device, layered)
    t = torch.from_numpy(blob).to("cuda")
    torch.cuda.synchronize()
    dev.set_weights_device(t.data_ptr(), t.numel())
    a, b, c = ref.weight_image(), host.weight_image(), dev.weight_image()
    assert a.size > 0 and a.size == b.size == c.size
    assert np.array_equal(a, b) and np.array_equal(b, c)
    for net in (ref, host, dev):
        net.close()


@pytest.mark.parametrize("precision,parts", [(BF16, 1), (SPLIT, 3)])
def test_queries(precision, parts, hip_device):
    """The diagnostics / runner queries (include/gzero_nn.h) answer as in fp32-ieee mode: one conv
    kernel for every launch size, heads not fused, the same wave of rows, no stamps."""
    wide, narrow = F256_NETS["13x13_f256_se85"], NETS["6x9_legacy_f40"][0]
    for desc, ct in ((wide, 4), (narrow, 2)):
        net = _hip(desc, random_weights(desc, 1), hip_device, precision)
        ieee = _hip(desc, random_weights(desc, 1), hip_device, "fp32-ieee")
        assert not net.heads_fused()
        assert net.kernel_name(False) == net.kernel_name(True) == "gzlayered::conv_bf16_kernel<%d, %d>" % (ct, parts)
        assert net.large_min_rows() == ieee.large_min_rows() == 1 << 30
        assert net.wave_rows() == ieee.wave_rows() > 0
        assert net.flops_per_eval() == pytest.approx(desc.flops_per_eval())
        with pytest.raises(RuntimeError):
            net.stamp_avg()
        net.close()
        ieee.close()


def test_public_interface(hip_device):
    """hexLG13's features=True template with 256 filters and 14 residual layers -- one block past
    what bf16x3 takes at 13 x 13 with squeeze-excite -- through Manager.create_new_network with
    precision="bf16x3-layered": predict_on_batch within the bf16x3-layered bounds on this file's
    weights; the same call with "bf16x3" is refused with the LDS message."""
    from galvanise_zero_amd.defs import templates
    from galvanise_zero_amd.nn.manager import Manager
    man = Manager(device=hip_device)
    game = "hexLG13"
    conf = templates.nn_model_config_template(game, "small", man.get_transformer(game), features=True)
    conf.cnn_filter_size = 256
    conf.residual_layers = 14
    with pytest.raises(RuntimeError, match="of LDS"):
        man.create_new_network(game, conf, precision="bf16x3")
    nn = man.create_new_network(game, conf, precision=SPLIT)
    model = nn.get_model()
    desc = model.desc
    assert model.net.precision == SPLIT
    assert desc.resnet_v2 and desc.global_pooling_value and desc.se_units == 85
    assert desc.cnn_filter_size == 256 and desc.residual_layers == 14
    n = 3
    w, x, ref_p, ref_z = _case(desc, n)
    model.set_weights(w)
    errs = _prob_errors("template256_b14", SPLIT, n, model.predict_on_batch(x), ref_p)
    rel = _logit_error("template256_b14", SPLIT, n, model.net, x, ref_z)
    model.net.close()
    assert rel <= LOGITS_TOL, rel
    for i, (mx, mean, kl) in enumerate(errs):
        assert mx <= DAMPED_TOLERANCE["max"] and mean <= DAMPED_TOLERANCE["mean"] and kl <= DAMPED_TOLERANCE["kl"], \
            (i, mx, mean, kl)
