"""GPU parity of the "fp16x3-layered" arithmetic mode (GZ_PRECISION_F16X3_LAYERED: the layered trunk
with gzlayered::conv_f16_kernel on v_mfma_f32_16x16x32_f16 behind board_exp_kernel, operands as fp16
hi + fp16 lo scaled by 2^11, one exponent per board and conv input) against the float64 oracle
(oracle/nn_ref.forward), on test_nn_layered_gpu.py's nets and rows.

Bounds, against the two neighbouring modes on the same weights and rows (nothing here is measured
from the mode itself):
  relative logit error <= 4 x fp32-ieee's        (22 against 24 significand bits per operand)
  relative logit error <= bf16x3-layered's / 4   (22 against 16 bits: 64 x in theory; a kernel that
                                                  loses or mis-scales a correction term cannot pass)
  probabilities within tolerance.DAMPED_TOLERANCE
Range: a 24-block v1 net on undamped weights whose float64 activations pass fp16's 65,504 stays
finite at the first bound.  Every row's outputs are bit-identical whatever the launch, the segment
split or the row chunk.  The host and the device packers give the same fp16 weight image.
"""
import numpy as np
import pytest

from galvanise_zero_amd.nn.desc import NetDesc
from galvanise_zero_amd.nn.tolerance import DAMPED_TOLERANCE
from galvanise_zero_amd.nn.weights import random_planes, random_weights, to_blob
from gpu_helpers import Pinned
from oracle import nn_ref
from test_nn_layered_gpu import NETS as LAYERED_NETS
from test_nn_v2_f256_gpu import NETS as F256_NETS, RES_GAMMA, _case, _hip, _logit_error, _prob_errors

pytestmark = pytest.mark.gpu

MODE, IEEE, SPLIT = "fp16x3-layered", "fp32-ieee", "bf16x3-layered"
NETS = {name: LAYERED_NETS[name] for name in ("19x19_f256_se85", "19x19_v1_f192_c15", "13x13_f256_concat", "10x10_f192_amazons",
                                              "6x9_legacy_f40", "8x8_cfg2_b2")}
F16_MAX = 65504.0


def _three_errors(tag, desc, w, x, ref_z, device, net=None):
    """Relative logit errors of fp32-ieee, bf16x3-layered and fp16x3-layered on the same weights and rows."""
    rel = {}
    for precision in (IEEE, SPLIT, MODE):
        n = net if (net is not None and precision == MODE) else _hip(desc, w, device, precision)
        rel[precision] = _logit_error(tag, precision, x.shape[0], n, x, ref_z)
        if n is not net:
            n.close()
    print("fp16x3 %s n=%d relative logit error: fp32-ieee %.3g bf16x3-layered %.3g fp16x3-layered %.3g (%.2f x ieee, 1/%.1f of bf16x3)" %
          (tag, x.shape[0], rel[IEEE], rel[SPLIT], rel[MODE], rel[MODE] / rel[IEEE], rel[SPLIT] / rel[MODE]))
    return rel


def _assert_errors(tag, rel):
    assert rel[MODE] <= 4 * rel[IEEE], (tag, rel)
    assert rel[MODE] <= 0.25 * rel[SPLIT], (tag, rel)


@pytest.mark.parametrize("name", sorted(NETS))
def test_accuracy(name, hip_device):
    """Relative logit error at most 4 x fp32-ieee's and at most a quarter of bf16x3-layered's, on the
    same weights and rows; probabilities within the damped-weights bound."""
    desc, rows = NETS[name]
    for n in rows:
        w, x, ref_p, ref_z = _case(desc, n)
        net = _hip(desc, w, hip_device, MODE)
        errs = _prob_errors(name, MODE, n, net.forward(x), ref_p)
        rel = _three_errors(name, desc, w, x, ref_z, hip_device, net)
        net.close()
        _assert_errors((name, n), rel)
        for i, (mx, mean, kl) in enumerate(errs):
            assert mx <= DAMPED_TOLERANCE["max"] and mean <= DAMPED_TOLERANCE["mean"] and kl <= DAMPED_TOLERANCE["kl"], \
                (name, n, i, mx, mean, kl)


def _trunk_max(desc, weights, planes):
    """The largest |activation| of the v1 trunk in float64 (oracle/nn_ref.py's own pieces)."""
    w = dict(weights)
    x = np.transpose(planes.astype(np.float64), (0, 2, 3, 1))
    x = nn_ref._act(nn_ref._bn(nn_ref._conv_same(x, w["initial_conv"]), w, "initial_bn"), desc.leaky_relu)
    top = np.abs(x).max()
    for i in range(desc.residual_layers):
        y = nn_ref._act(nn_ref._bn(nn_ref._conv_same(x, w["res%d_conv0" % i]), w, "res%d_bn0" % i), desc.leaky_relu)
        top = max(top, np.abs(y).max())
        y = nn_ref._bn(nn_ref._conv_same(y, w["res%d_conv1" % i]), w, "res%d_bn1" % i)
        x = nn_ref._act(x + y, desc.leaky_relu)
        top = max(top, np.abs(x).max())
    return float(top)


def test_range(hip_device):
    """Activations beyond fp16's range: the 20-block 10 x 10 recipe (v1, undamped res_gamma) at 64
    filters and 24 blocks, where the float64 residual stream reaches 1.9e5 (it passes 65,504 at block
    22).  Without the per-board exponent the fp16 operands would be infinite; the outputs are finite
    and the logit error is at most 4 x fp32-ieee's."""
    desc = NetDesc(5, 10, 10, 64, 24, [101, 101])
    w = random_weights(desc, 7921)
    x = random_planes(desc, 2, 11)
    top = _trunk_max(desc, w, x)
    print("fp16x3 range: largest float64 trunk activation %.4g" % top)
    assert top > F16_MAX
    ref_z = nn_ref.forward(desc, w, x, logits=True)
    net = _hip(desc, w, hip_device, MODE)
    for out in net.forward(x):
        assert np.all(np.isfinite(out))
    rel = _three_errors("10x10_v1_f64_b24_undamped", desc, w, x, ref_z, hip_device, net)
    net.close()
    assert rel[MODE] <= 4 * rel[IEEE], rel


def test_batch_and_chunk_invariance(hip_device, monkeypatch):
    """A row does not depend on the launch it runs in (300 rows, a permuted 37-row subset, a single
    row), nor on the internal row chunks (GZ_FP32_CHUNK_ROWS, read at net creation: 5-row chunks,
    the last one partial): its exponents are its own."""
    desc = F256_NETS["13x13_f256_se85"]
    w = random_weights(desc, 3, bias_std=0.2, res_gamma=RES_GAMMA)
    net = _hip(desc, w, hip_device, MODE)
    x = random_planes(desc, 300, 9)
    full = net.forward(x)
    perm = np.random.default_rng(0).permutation(300)[:37]
    for a, b in zip(full, net.forward(x[perm])):
        assert np.array_equal(a[perm], b)
    for a, b in zip(full, net.forward(x[5:6])):
        assert np.array_equal(a[5:6], b)
    net.close()
    monkeypatch.setenv("GZ_FP32_CHUNK_ROWS", "5")
    chunked = _hip(desc, w, hip_device, MODE)
    for a, b in zip(full, chunked.forward(x[perm])):
        assert np.array_equal(a[perm], b)
    chunked.close()


def test_segments_match_forward(hip_device):
    """forward_segments (the runner's call path) over three pinned-host segments of 5, 1 and 9 rows
    equals one flat forward of the same 15 rows, bit for bit."""
    import torch
    desc = NETS["19x19_f256_se85"][0]
    net = _hip(desc, random_weights(desc, 7921, bias_std=0.2, res_gamma=RES_GAMMA), hip_device, MODE)
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


def test_weight_image(hip_device):
    """The host packer (set_weights) and the device roll (set_weights_device) give the same fp16 hi |
    scaled-lo image, byte for byte, on a padded 192 -> 256 filter v2 net; it has the bf16x3 image's size
    and differs from it."""
    import torch
    from galvanise_zero_amd._native import HipNet
    desc = F256_NETS["10x10_f192_amazons"]
    blob = to_blob(random_weights(desc, 7919, bias_std=0.2, res_gamma=RES_GAMMA))
    host = HipNet(desc, hip_device, MODE)
    host.set_weights(blob)
    dev = HipNet(desc, hip_device, MODE)
    t = torch.from_numpy(blob).to("cuda")
    torch.cuda.synchronize()
    dev.set_weights_device(t.data_ptr(), t.numel())
    a, b = host.weight_image(), dev.weight_image()
    assert a.size > 0 and a.size == b.size and np.array_equal(a, b)
    split = HipNet(desc, hip_device, SPLIT)
    split.set_weights_device(t.data_ptr(), t.numel())
    c = split.weight_image()
    # (bf16x3-layered carries the policy GEMM's fragments behind the common part)
    assert c.size >= a.size and not np.array_equal(a, c[:a.size])
    for net in (host, dev, split):
        net.close()


def test_weight_out_of_range_refused(hip_device):
    """set_weights refuses a blob with a BN-folded conv weight fp16 cannot hold, naming the conv; the
    net keeps working with a blob that fits."""
    from galvanise_zero_amd._native import HipNet
    from galvanise_zero_amd.nn.desc import weight_spec
    desc = NETS["6x9_legacy_f40"][0]
    w = random_weights(desc, 5)
    blob = to_blob(w)
    off = 0
    for name, shape in weight_spec(desc):
        if name == "res1_conv0":
            break
        off += int(np.prod(shape))
    bad = blob.copy()
    bad[off + 3] = 1e9
    net = HipNet(desc, hip_device, MODE)
    with pytest.raises(RuntimeError, match=r"trunk conv 2 \(residual block 1\).*fp16's finite range"):
        net.set_weights(bad)
    net.set_weights(blob)
    for out in net.forward(random_planes(desc, 2, 1)):
        assert np.all(np.isfinite(out))
    net.close()


def test_queries(hip_device):
    """The diagnostics / runner queries (include/gzero_nn.h) answer as the layered modes' do: one conv
    kernel for every launch size, heads not fused, fp32-ieee's wave of rows, no stamps."""
    wide, narrow = F256_NETS["13x13_f256_se85"], NETS["6x9_legacy_f40"][0]
    for desc, ct in ((wide, 4), (narrow, 2)):
        net = _hip(desc, random_weights(desc, 1), hip_device, MODE)
        ieee = _hip(desc, random_weights(desc, 1), hip_device, IEEE)
        assert not net.heads_fused()
        assert net.kernel_name(False) == net.kernel_name(True) == "gzlayered::conv_f16_kernel<%d>" % ct
        assert net.large_min_rows() == ieee.large_min_rows() == 1 << 30
        assert net.wave_rows() == ieee.wave_rows() > 0
        assert net.flops_per_eval() == pytest.approx(desc.flops_per_eval())
        with pytest.raises(RuntimeError):
            net.stamp_avg()
        net.close()
        ieee.close()


def test_public_interface(hip_device):
    """hexLG13's features=True template with 256 filters and 14 residual layers through
    Manager.create_new_network with precision="fp16x3-layered": predict_on_batch within the
    damped-weights bound, the logits within this file's two bounds."""
    from galvanise_zero_amd.defs import templates
    from galvanise_zero_amd.nn.manager import Manager
    man = Manager(device=hip_device)
    game = "hexLG13"
    conf = templates.nn_model_config_template(game, "small", man.get_transformer(game), features=True)
    conf.cnn_filter_size = 256
    conf.residual_layers = 14
    nn = man.create_new_network(game, conf, precision=MODE)
    model = nn.get_model()
    desc = model.desc
    assert model.net.precision == MODE
    assert desc.resnet_v2 and desc.global_pooling_value and desc.se_units == 85
    assert desc.cnn_filter_size == 256 and desc.residual_layers == 14
    n = 3
    w, x, ref_p, ref_z = _case(desc, n)
    model.set_weights(w)
    errs = _prob_errors("template256_b14", MODE, n, model.predict_on_batch(x), ref_p)
    rel = _three_errors("template256_b14", desc, w, x, ref_z, hip_device, model.net)
    model.net.close()
    _assert_errors("template256_b14", rel)
    for i, (mx, mean, kl) in enumerate(errs):
        assert mx <= DAMPED_TOLERANCE["max"] and mean <= DAMPED_TOLERANCE["mean"] and kl <= DAMPED_TOLERANCE["kl"], \
            (i, mx, mean, kl)
    # Manager(precision=...) passes the name on too
    assert Manager(device=hip_device, precision=MODE).precision == MODE
