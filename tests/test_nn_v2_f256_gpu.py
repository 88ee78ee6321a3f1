"""GPU parity of v2 (pre-activation, squeeze-excite, pooling value head) nets with up to 256 filters
-- the trunk_kernel_v2<256, ...> instantiations (trunk_f256_v2.hip) and the fp32-ieee path with up
to 128 squeeze-excite units -- against the float64 oracle (oracle/nn_ref.forward), in all three
arithmetic modes.

Nets (weights random_weights(desc, 7919, bias_std=0.2, res_gamma=0.3) as in test_nn_v2_gpu.py):
8 x 8 with 85 SE units (the two-pass split at 4 position tiles), 10 x 10 with 192 filters padded to
256 and amazons' 3,041-move policies (partial last tile, single-image split, the policy GEMM beside
a pooling value head), 13 x 13 with the global residual (two-pass split), with and without
concat_all_layers, and a one-block net with a bare 3 x 3 initial conv.

Bounds:
  bf16x3 logits   max|z - z_ref| / max(1, max|z_ref|) <= the tighter of tolerance.SPLIT_TOLERANCE's
                  cfg4 / cfg5 "logits" (1.2e-4), the project's bound for its 256-filter nets
  bf16x3 probs    tolerance.DAMPED_TOLERANCE (max / mean / row KL)
  bf16 probs      per output max(test_nn_v2_gpu.TOL_V2_BF16, 3 x the error measured here on the
                  net's 128-filter twin: the same desc with 128 filters and 42 SE units, same seeds,
                  on kernels whose results this file's kernels leave untouched)
  fp32-ieee       test_nn_fp32_gpu's v2 criteria: probabilities within (2e-4, 5e-5), relative logit
                  error at most a quarter of bf16x3's on the same input

Worst measured on MI355X (profiles/v2_f256_gpu_tests.log):
  bf16x3     relative logit error 7.19e-6 (13x13_f256_concat, n = 7; bound 1.2e-4); probabilities
             max 8.94e-7 / mean 4.01e-7 (13x13_f256_concat out2) / row KL 1.06e-7 (13x13_f256_se85)
             against DAMPED_TOLERANCE's 1.4e-5 / 2.5e-6 / 5e-7
  bf16       max 1.0e-3 (10x10_f256_b1_bare out1, n = 1) / mean 4.63e-4 (13x13_f256_concat out2) /
             row KL 2.82e-6; the 128-filter twins: max 8.2e-4 / mean 4.22e-4 (8x8_f256_se85 out2)
  fp32-ieee  max 1.19e-7 / mean 3.19e-8 / row KL 1.13e-7; relative logit error 2.81e-7 and 2.92e-7
             against bf16x3's 3.15e-6 and 5.84e-6 (8 x 8, 13 x 13)
  template   hexLG13 features=True at 256 filters, bf16, on its own undamped weights: max 2.7e-3 /
             mean 2.99e-4 (twin at 128 filters: 8.54e-4 / 4.01e-4)
"""
import dataclasses

import numpy as np
import pytest

from galvanise_zero_amd.nn.desc import NetDesc
from galvanise_zero_amd.nn.tolerance import DAMPED_TOLERANCE, SPLIT_TOLERANCE
from galvanise_zero_amd.nn.weights import random_planes, random_weights, to_blob
from oracle import nn_ref
from test_nn_fp32_gpu import TOL_FP32 as TOL_IEEE
from test_nn_v2_gpu import RES_GAMMA, TOL_V2_BF16

pytestmark = pytest.mark.gpu

LOGITS_TOL = min(SPLIT_TOLERANCE["cfg4"]["logits"], SPLIT_TOLERANCE["cfg5"]["logits"])
POOLED = dict(resnet_v2=True, global_pooling_value=True, value_bn=True)
NETS = {
    "8x8_f256_se85": NetDesc(5, 8, 8, 256, 2, [155, 155], se_units=85, **POOLED),
    "10x10_f192_amazons": NetDesc(12, 10, 10, 192, 2, [3041, 3041], num_values=3, se_units=64, **POOLED),
    "13x13_f256_se85": NetDesc(5, 13, 13, 256, 2, [170, 171], se_units=85, **POOLED),
    "13x13_f256_concat": NetDesc(5, 13, 13, 256, 2, [170, 171], value_hidden_size=128, resnet_v2=True,
                                 concat_all_layers=True),
    "10x10_f256_b1_bare": NetDesc(5, 10, 10, 256, 1, [101, 101], resnet_v2=True, initial_kernel_size=3,
                                  initial_bn=False),
}
BATCHES = (1, 7)


def _twin(desc):
    """The 128-filter twin: same shape, seeds and heads, 42 squeeze-excite units where SE is on."""
    return dataclasses.replace(desc, cnn_filter_size=128, se_units=42 if desc.se_units else 0)


_cache = {}


def _case(desc, n, seed=7919, damped=True):
    """(weights, planes, oracle probabilities, oracle logits) of a net at n rows, computed once."""
    key = (repr(desc), n, seed, damped)
    if key not in _cache:
        w = random_weights(desc, seed, bias_std=0.2, res_gamma=RES_GAMMA) if damped else random_weights(desc, seed)
        x = random_planes(desc, n, 100 + n)
        _cache[key] = (w, x, nn_ref.forward(desc, w, x), nn_ref.forward(desc, w, x, logits=True))
    return _cache[key]


def _hip(desc, w, device, precision):
    from galvanise_zero_amd._native import HipNet
    net = HipNet(desc, device, precision)
    net.set_weights(to_blob(w))
    return net


def _kl(ref, got):
    r = np.clip(ref.astype(np.float64), 1e-30, None)
    g = np.clip(got.astype(np.float64), 1e-30, None)
    return float((r * np.log(r / g)).sum(axis=1).max())


def _prob_errors(tag, precision, n, got, ref):
    """[(max, mean, kl)] per output, printed the way the other GPU files print them."""
    out = []
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and np.all(np.isfinite(g)), (tag, precision, i)
        d = np.abs(g.astype(np.float64) - r.astype(np.float64))
        e = (float(d.max()), float(d.mean()), _kl(r, g))
        print("v2f256 %s %s n=%d out%d vs_ref max %.3g mean %.3g kl %.3g" % ((tag, precision, n, i) + e))
        out.append(e)
    return out


def _logit_error(tag, precision, n, net, x, ref_z):
    net.set_output_logits(True)
    z = net.forward(x)
    net.set_output_logits(False)
    rel = max(float(np.abs(g.astype(np.float64) - r).max() / max(1.0, np.abs(r).max())) for g, r in zip(z, ref_z))
    print("v2f256 %s %s n=%d relative logit error %.3g" % (tag, precision, n, rel))
    return rel


@pytest.mark.parametrize("name", sorted(NETS))
def test_split(name, hip_device):
    """bf16x3: relative logit error within the 256-filter configs' stated bound, probabilities within
    the damped-weights bound."""
    desc = NETS[name]
    for n in BATCHES:
        w, x, ref_p, ref_z = _case(desc, n)
        net = _hip(desc, w, hip_device, "bf16x3")
        errs = _prob_errors(name, "bf16x3", n, net.forward(x), ref_p)
        rel = _logit_error(name, "bf16x3", n, net, x, ref_z)
        net.close()
        assert rel <= LOGITS_TOL, (name, n, rel)
        for i, (mx, mean, kl) in enumerate(errs):
            assert mx <= DAMPED_TOLERANCE["max"] and mean <= DAMPED_TOLERANCE["mean"] and kl <= DAMPED_TOLERANCE["kl"], \
                (name, n, i, mx, mean, kl)


@pytest.mark.parametrize("name", sorted(NETS))
def test_bf16(name, hip_device):
    """bf16: per output within max(TOL_V2_BF16, 3 x the 128-filter twin's error on the same rows)."""
    desc, twin = NETS[name], _twin(NETS[name])
    for n in BATCHES:
        w, x, ref_p, _ = _case(desc, n)
        tw, tx, tref_p, _ = _case(twin, n)
        tnet = _hip(twin, tw, hip_device, "bf16")
        terrs = _prob_errors(name + "/twin128", "bf16", n, tnet.forward(tx), tref_p)
        tnet.close()
        net = _hip(desc, w, hip_device, "bf16")
        errs = _prob_errors(name, "bf16", n, net.forward(x), ref_p)
        net.close()
        for i, ((mx, mean, _), (tmx, tmean, _)) in enumerate(zip(errs, terrs)):
            assert mx <= max(TOL_V2_BF16[0], 3 * tmx) and mean <= max(TOL_V2_BF16[1], 3 * tmean), \
                (name, n, i, (mx, mean), (tmx, tmean))


@pytest.mark.parametrize("name", ["8x8_f256_se85", "13x13_f256_se85"])
def test_fp32_ieee(name, hip_device):
    """fp32-ieee with 85 squeeze-excite units: probabilities within (2e-4, 5e-5), relative logit error
    at most a quarter of bf16x3's on the same input."""
    desc, n = NETS[name], 7
    w, x, ref_p, ref_z = _case(desc, n)
    rel = {}
    for precision in ("fp32-ieee", "bf16x3"):
        net = _hip(desc, w, hip_device, precision)
        if precision == "fp32-ieee":
            for i, (mx, mean, _) in enumerate(_prob_errors(name, precision, n, net.forward(x), ref_p)):
                assert mx <= TOL_IEEE[0] and mean <= TOL_IEEE[1], (name, i, mx, mean)
        rel[precision] = _logit_error(name, precision, n, net, x, ref_z)
        net.close()
    assert rel["fp32-ieee"] <= 0.25 * rel["bf16x3"], (name, rel)


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("name", ["10x10_f192_amazons", "13x13_f256_se85"])
def test_batch_invariance(name, precision, hip_device):
    """The squeeze-excite means, the pooled features and the global residual are per board: a row
    does not depend on the launch it runs in (300 rows, a permuted 37-row subset, a single row)."""
    desc = NETS[name]
    net = _hip(desc, random_weights(desc, 3, bias_std=0.2, res_gamma=RES_GAMMA), hip_device, precision)
    x = random_planes(desc, 300, 9)
    full = net.forward(x)
    perm = np.random.default_rng(0).permutation(300)[:37]
    for a, b in zip(full, net.forward(x[perm])):
        assert np.array_equal(a[perm], b)
    for a, b in zip(full, net.forward(x[5:6])):
        assert np.array_equal(a[5:6], b)
    net.close()


@pytest.mark.parametrize("precision", ["bf16", "bf16x3", "fp32-ieee"])
def test_device_roll_identical(precision, hip_device):
    """set_weights (host job list) and set_weights_device (the same jobs as kernels) give the same
    weight image, byte for byte, for a padded 192 -> 256 filter v2 net with the GEMM heads."""
    import torch
    from galvanise_zero_amd._native import HipNet
    desc = NETS["10x10_f192_amazons"]
    blob = to_blob(random_weights(desc, 7919, bias_std=0.2, res_gamma=RES_GAMMA))
    host = HipNet(desc, hip_device, precision)
    host.set_weights(blob)
    dev = HipNet(desc, hip_device, precision)
    t = torch.from_numpy(blob).to("cuda")
    torch.cuda.synchronize()
    dev.set_weights_device(t.data_ptr(), t.numel())
    a, b = host.weight_image(), dev.weight_image()
    assert a.size == b.size and a.size > 0 and np.array_equal(a, b)
    host.close()
    dev.close()


def test_public_interface(hip_device):
    """The reference's features=True template at 256 filters through Manager.create_new_network:
    squeeze-excite with 256 // 3 = 85 units, predict_on_batch (HipModel's default bf16) against the
    oracle on the network's own weights, at the bf16 bound above (twin: the same template at 128
    filters, same seed)."""
    from galvanise_zero_amd.defs import templates
    from galvanise_zero_amd.nn.manager import Manager
    man = Manager(device=hip_device)
    game = "hexLG13"
    t = man.get_transformer(game)
    errs = {}
    for filters in (256, 128):
        conf = templates.nn_model_config_template(game, "small", t, features=True)
        conf.cnn_filter_size = filters
        conf.residual_layers = 2
        nn = man.create_new_network(game, conf)
        model = nn.get_model()
        desc = model.desc
        assert desc.resnet_v2 and desc.global_pooling_value and desc.cnn_filter_size == filters
        assert desc.se_units == filters // 3
        x = random_planes(desc, 7, 107)
        errs[filters] = _prob_errors("template%d" % filters, "bf16", 7, model.predict_on_batch(x),
                                     nn_ref.forward(desc, model.weights, x))
        model.net.close()
    assert errs[256] and len(errs[256]) == len(errs[128])
    for i, ((mx, mean, _), (tmx, tmean, _)) in enumerate(zip(errs[256], errs[128])):
        assert mx <= max(TOL_V2_BF16[0], 3 * tmx) and mean <= max(TOL_V2_BF16[1], 3 * tmean), \
            (i, (mx, mean), (tmx, tmean))
