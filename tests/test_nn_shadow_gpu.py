"""The shadow check on the GPU (include/gzero_nn.h gz_net_shadow_*, csrc/nn/shadow_compare.hip): the
comparison kernels against a float64 numpy restatement, a net with a shadow against two separate
nets, the schedule (every / max_rows / reset), the ordering against weight rolls, a refusing shadow,
the GEMM-heads path, logits mode, reproducibility and gz_net_last_kernel_ms.

The restatement (Restated below) does the kernels' arithmetic in the kernels' order -- every double
operation is IEEE and unfused on both sides, so it gives the same bits: a role's elements are added
per lane (elements lane, lane + 64, ... ascending), the 64 lane sums meet in an xor butterfly, a row
adds its roles in order and the fold adds the rows in order.  The logarithm is the kernel's own
(_log_pos; pinned to numpy's within 1 ulp by test_restated_log_is_a_log, which needs no GPU).  Counts,
maxima and positions are asserted exactly, the sums to 1e-12 relative: double math in both places."""
import numpy as np
import pytest

from galvanise_zero_amd import _native
from galvanise_zero_amd.nn.desc import NetDesc, weight_spec
from galvanise_zero_amd.nn.weights import random_planes, random_weights, to_blob

gpu = pytest.mark.gpu

SUM_RTOL = 1e-12
EXACT = ("checks", "rows", "nonfinite_rows", "policy_elems", "policy_rows", "value_elems", "argmax_mismatch",
         "max_abs_dp", "max_row_kl", "max_abs_dv", "worst_check", "worst_row")
SUMS = ("sum_abs_dp", "sum_row_kl", "sum_abs_dv")

DESC = NetDesc(5, 8, 8, 128, 2, [155, 155])              # 8 x 8, 5 planes, 2 x 128: fused heads
AMAZONS = NetDesc(12, 10, 10, 256, 1, [3041, 3041])      # single-image net: policy_gemm_kernel heads


def _log_pos(x):
    """shadow_compare.hip's log_pos, operation for operation."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = x.view(np.uint64)
    hx = (b >> np.uint64(32)).astype(np.uint32) + np.uint32(0x3ff00000 - 0x3fe6a09e)
    dk = ((hx >> np.uint32(20)).astype(np.int64) - 0x3ff).astype(np.float64)
    hx = (hx & np.uint32(0x000fffff)) + np.uint32(0x3fe6a09e)
    m = ((hx.astype(np.uint64) << np.uint64(32)) | (b & np.uint64(0xffffffff))).view(np.float64)
    f = m - 1.0
    hfsq = (0.5 * f) * f
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01))
    t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 +
                                                                             w * 1.479819860511658591e-01)))
    r = s * (hfsq + (t2 + t1))
    r = r + dk * 1.90821492927058770002e-10
    r = r - hfsq
    r = r + f
    return r + dk * 6.93147180369123816490e-01


def _lane_sum(t):
    """Sum of a role's terms in the wave's order."""
    k = -(-t.size // 64)
    pad = np.zeros(k * 64)
    pad[:t.size] = t
    lanes = np.zeros(64)
    for chunk in pad.reshape(k, 64):
        lanes = lanes + chunk
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[idx ^ off]
    assert np.all(lanes == lanes[0])
    return float(lanes[0])


class Restated(object):
    """gz_shadow_stats by the definitions of include/gzero_nn.h, in float64 numpy."""

    def __init__(self):
        self.t = dict.fromkeys(EXACT + SUMS, 0)
        for k in SUMS + ("max_abs_dp", "max_row_kl", "max_abs_dv"):
            self.t[k] = 0.0

    def check(self, outs_a, outs_b, index=0, logits=False):
        """One check: outs_a the net's ("got"), outs_b the shadow's ("ref")."""
        t = self.t
        pa, pb = outs_a[:-1], outs_b[:-1]
        va, vb = outs_a[-1].astype(np.float64), outs_b[-1].astype(np.float64)
        for row in range(va.shape[0]):
            t["rows"] += 1
            if not all(np.all(np.isfinite(x[row])) for x in list(outs_a) + list(outs_b)):
                t["nonfinite_rows"] += 1
                continue
            max_dp = sum_dp = max_kl = sum_kl = 0.0
            mismatch = 0
            for a32, b32 in zip(pa, pb):
                a, b = a32[row].astype(np.float64), b32[row].astype(np.float64)
                d = np.abs(a - b)
                sum_dp = sum_dp + _lane_sum(d)
                max_dp = max(max_dp, float(d.max()))
                if not logits:
                    ref, got = np.maximum(b, 1e-30), np.maximum(a, 1e-30)   # (tests/gpu_helpers.kl's clip)
                    kl = _lane_sum(ref * _log_pos(ref / got))
                    sum_kl = sum_kl + kl
                    max_kl = max(max_kl, kl)
                mismatch += int(np.argmax(a32[row]) != np.argmax(b32[row]))
            max_dv = sum_dv = 0.0
            for v in range(va.shape[1]):
                d = abs(va[row, v] - vb[row, v])
                sum_dv = sum_dv + d
                max_dv = max(max_dv, d)
            t["policy_elems"] += sum(x.shape[1] for x in pa)
            t["value_elems"] += va.shape[1]
            if max_dp > t["max_abs_dp"]:
                t["max_abs_dp"], t["worst_check"], t["worst_row"] = max_dp, index, row
            t["sum_abs_dp"] = t["sum_abs_dp"] + sum_dp
            if not logits:
                t["policy_rows"] += len(pa)
                t["max_row_kl"] = max(t["max_row_kl"], max_kl)
                t["sum_row_kl"] = t["sum_row_kl"] + sum_kl
            t["argmax_mismatch"] += mismatch
            t["max_abs_dv"] = max(t["max_abs_dv"], max_dv)
            t["sum_abs_dv"] = t["sum_abs_dv"] + sum_dv
        t["checks"] += 1
        return self


def _assert_totals(got, want, what=""):
    print("%s got  %s" % (what, {k: got[k] for k in EXACT + SUMS}))
    print("%s want %s" % (what, want))
    for k in EXACT:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in SUMS:
        assert abs(got[k] - want[k]) <= SUM_RTOL * abs(want[k]), (what, k, got[k], want[k])
    assert got["device_ms"] > 0.0


def test_restated_log_is_a_log():
    """The kernel's logarithm, restated: within 1 ulp of numpy's over the quotients a comparison meets
    (1e-30 / 1 to 1 / 1e-30) and dense around 1, where the KL terms cancel."""
    rng = np.random.default_rng(5)
    x = np.concatenate([np.exp(rng.uniform(-70.0, 70.0, 200000)), 1.0 + rng.uniform(-1e-3, 1e-3, 200000),
                        1.0 + rng.uniform(-1e-7, 1e-7, 100000), [1.0, 2.0, 0.5, 1e-30, 1e30, np.sqrt(0.5), np.sqrt(2.0)]])
    mine, ref = _log_pos(x), np.log(x)
    assert _log_pos(np.array([1.0]))[0] == 0.0
    assert np.all(np.abs(mine - ref) <= np.spacing(np.abs(ref))), float(np.max(np.abs(mine - ref) / np.spacing(np.abs(ref))))


def _softmax_rows(rng, n, p):
    z = rng.normal(0.0, 2.0, (n, p))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def _crafted(sizes, seed):
    """Six rows: identical; the maximum tied at two indices on both sides; the tie the other way round
    on one side; exact zeros in a where b > 0 (the 1e-30 clip); a NaN in a's policy; an inf in b's values."""
    rng = np.random.default_rng(seed)
    n = 6
    b = [_softmax_rows(rng, n, p) for p in sizes] + [_softmax_rows(rng, n, 3)]
    a = [(x * (1.0 + rng.uniform(-1e-4, 1e-4, x.shape))).astype(np.float32) for x in b]
    for pa, pb in zip(a[:-1], b[:-1]):
        p = pa.shape[1]
        lo, hi = 3, p - 2          # (hi is not in the first lane round: 65 -> 63, 171 -> 169, 3041 -> 3039)
        pa[0] = pb[0]
        top = np.float32(0.5)
        for x in (pa, pb):         # row 1: tied at lo and hi on both sides, first maximum lo on both
            x[1] = np.minimum(x[1], np.float32(0.25))
            x[1, lo] = x[1, hi] = top
        pa[2] = np.minimum(pa[2], np.float32(0.25))
        pb[2] = np.minimum(pb[2], np.float32(0.25))
        pa[2, lo] = pa[2, hi] = top                    # a: tied, first maximum lo
        pb[2, lo], pb[2, hi] = np.nextafter(top, np.float32(0)), top   # b: the later one wins
        pa[3, 5:40] = 0.0
        pa[3, 50] = pb[3, 50] = np.float32(0.6)        # (the first maximum of both sides, outside the zeros)
        assert np.all(pb[3, 5:40] > 0)
    a[0][0] = b[0][0]
    a[-1][0] = b[-1][0]
    a[0][4, 17] = np.nan
    b[-1][5, 1] = np.inf
    return a, b


@gpu
@pytest.mark.parametrize("sizes", [[65, 171], [3041]])
def test_compare_outputs_crafted(sizes, hip_device):
    a, b = _crafted(sizes, 11)
    got = _native.compare_outputs(a, b, hip_device)
    want = Restated().check(a, b).t
    _assert_totals(got, want, "crafted %s" % sizes)
    roles = len(sizes)
    assert (got["checks"], got["rows"], got["nonfinite_rows"], got["worst_check"]) == (1, 6, 2, 0)
    assert got["policy_elems"] == 4 * sum(sizes) and got["policy_rows"] == 4 * roles and got["value_elems"] == 12
    assert got["argmax_mismatch"] == roles          # row 2, once per role
    assert got["worst_row"] == 3 and got["max_abs_dp"] == max(float(x[3, 5:40].max()) for x in b[:-1])
    # the clipped row's KL: b log(b / 1e-30) over the zeroed elements dominates
    clipped = max(float((x[3, 5:40].astype(np.float64) * np.log(x[3, 5:40].astype(np.float64) / 1e-30)).sum()) for x in b[:-1])
    assert clipped > 0.4 and got["max_row_kl"] > 0.9 * clipped
    assert got["mean_abs_dp"] == got["sum_abs_dp"] / got["policy_elems"]
    assert got["mean_row_kl"] == got["sum_row_kl"] / got["policy_rows"]
    assert got["mean_abs_dv"] == got["sum_abs_dv"] / got["value_elems"]


def _net(desc, blob, device, precision, shadow=None):
    net = _native.HipNet(desc, device, precision)
    if shadow is not None:
        net.enable_shadow(*shadow)
    if blob is not None:
        net.set_weights(blob)
    return net


def _fresh_outputs(desc, blob, x, device, precision, logits=False):
    net = _net(desc, blob, device, precision)
    if logits:
        net.set_output_logits(True)
    outs = net.forward(x)
    net.close()
    return outs


@pytest.fixture(scope="module")
def small(hip_device):
    """The 2 x 128 net's two generations of weights, 37 rows of planes and, per generation, the
    outputs of fresh bf16x3 and fp32-ieee nets on the first 16 rows (computed once, never changed)."""
    s = {"w1": to_blob(random_weights(DESC, 7921, bias_std=0.2)), "w2": to_blob(random_weights(DESC, 7922, bias_std=0.2)),
         "x": random_planes(DESC, 37, 20260101)}
    for w in ("w1", "w2"):
        for mode in ("bf16x3", "fp32-ieee"):
            s[w, mode] = _fresh_outputs(DESC, s[w], s["x"][:16], hip_device, mode)
            for o in s[w, mode]:
                o.setflags(write=False)
    for k in ("w1", "w2", "x"):
        s[k].setflags(write=False)
    return s


@gpu
def test_net_with_shadow_matches_two_nets(small, hip_device):
    """37 rows as segments [5, 20, 12] with pinned-host outputs; every = 1, max_rows = 16: one check of
    16 rows, spanning two segments, whose totals are those of two separate nets' forwards of x[:16]
    (rows are batch-invariant); the net's 37 rows are bit-identical to a net without a shadow."""
    from test_bench_shape_gpu import _segmented_forward
    x = small["x"]
    net = _net(DESC, small["w1"], hip_device, "bf16x3", ("fp32-ieee", 1, 16))
    got_rows = _segmented_forward(net, DESC, x, [5, 20, 12])
    st = net.shadow_stats()
    assert (st["checks"], st["rows"], st["nonfinite_rows"]) == (1, 16, 0)
    want = Restated().check(small["w1", "bf16x3"], small["w1", "fp32-ieee"]).t
    _assert_totals(st, want, "two nets")
    assert 0.0 < st["max_abs_dp"] < 1e-3 and st["policy_rows"] == 32
    plain = _net(DESC, small["w1"], hip_device, "bf16x3")
    for g, p in zip(got_rows, _segmented_forward(plain, DESC, x, [5, 20, 12])):
        assert np.array_equal(g, p)
    for g, p in zip(got_rows, small["w1", "bf16x3"]):
        assert np.array_equal(g[:16], p)
    net.disable_shadow()
    with pytest.raises(RuntimeError, match="shadow: the net has no shadow"):
        net.shadow_stats()
    for g, p in zip(net.forward(x), got_rows):
        assert np.array_equal(g, p)
    net.close()
    plain.close()


@gpu
def test_schedule_and_reset(small, hip_device):
    """every = 3: of seven forwards of 4 rows, the ones with index 0, 3 and 6 are checked; a reset does
    not restart the count, so forward 7 is not."""
    net = _net(DESC, small["w1"], hip_device, "bf16x3", ("fp32-ieee", 3, 256))
    x = small["x"]
    for i in range(7):
        net.forward(x[4 * i:4 * i + 4])
    st = net.shadow_stats(reset=True)
    assert (st["checks"], st["rows"]) == (3, 12)
    assert st["worst_check"] in (0, 3, 6) and 0 <= st["worst_row"] < 4
    net.forward(x[:4])
    st = net.shadow_stats()
    assert st["checks"] == 0 and st["rows"] == 0 and st["max_abs_dp"] == 0.0 and st["device_ms"] == 0.0
    net.forward(x[:4])
    net.forward(x[:4])                                  # index 9
    st = net.shadow_stats()
    assert (st["checks"], st["rows"], st["worst_check"]) == (1, 4, 9)
    with pytest.raises(RuntimeError, match="shadow: the net already has a shadow"):
        net.enable_shadow("fp32-ieee")
    net.close()


@gpu
def test_enable_refusals(small, hip_device):
    net = _net(DESC, small["w1"], hip_device, "bf16x3")
    for args, text in ((("bf16x3", 1, 1), "the net's own mode"), (("split", 1, 1), "the net's own mode"),
                       (("fp32-ieee", 0, 1), "at least 1"), (("fp32-ieee", 1, 0), "at least 1")):
        with pytest.raises(RuntimeError, match="shadow: .*" + text):
            net.enable_shadow(*args)
    with pytest.raises(RuntimeError, match="shadow: the net has no shadow"):
        net.shadow_stats()
    net.close()
    big = _native.HipNet(NetDesc(5, 19, 19, 256, 1, [362, 362]), hip_device, "bf16x3-layered")
    with pytest.raises(RuntimeError, match="shadow: unsupported network geometry F=256 H=19 W=19"):
        big.enable_shadow("bf16x3")
    big.close()


@gpu
def test_ordering_against_rolls(small, hip_device):
    """A shadow enabled on a net that has weights has none itself: no check until the next roll.  After
    set_weights(w2), and again after set_weights_device, both nets run w2: the totals are those of
    fresh nets on w2 -- which a shadow left on another generation would miss by far."""
    import torch
    x = small["x"][:16]
    want1 = Restated().check(small["w1", "bf16x3"], small["w1", "fp32-ieee"]).t
    want2 = Restated().check(small["w2", "bf16x3"], small["w2", "fp32-ieee"]).t
    # a stale shadow would show the generations' distance, not the modes'
    apart = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(small["w1", "fp32-ieee"][:-1],
                                                                               small["w2", "fp32-ieee"][:-1]))
    assert apart > 100 * max(want1["max_abs_dp"], want2["max_abs_dp"]), (apart, want1["max_abs_dp"], want2["max_abs_dp"])
    net = _net(DESC, small["w1"], hip_device, "bf16x3")
    net.enable_shadow("fp32-ieee", 1, 16)
    net.forward(x)
    assert net.shadow_stats()["checks"] == 0
    net.set_weights(small["w2"])
    net.forward(x)                                       # (forward index 1)
    want2["worst_check"] = 1
    _assert_totals(net.shadow_stats(reset=True), want2, "after set_weights(w2)")
    t = torch.from_numpy(small["w1"].copy()).to("cuda")
    net.set_weights_device(t.data_ptr(), t.numel())
    net.forward(x)
    want1["worst_check"] = 2
    _assert_totals(net.shadow_stats(reset=True), want1, "after set_weights_device(w1)")
    net.close()


@gpu
def test_refusing_shadow_changes_nothing(small, hip_device):
    """fp16x3-layered as the shadow refuses a blob with a BN-folded conv weight of 65,520 or more: the
    call fails with the shadow's message behind "shadow: " and neither net's weights change."""
    x = small["x"][:8]
    net = _net(DESC, None, hip_device, "bf16x3", ("fp16x3-layered", 1, 8))
    net.set_weights(small["w1"])
    before = net.forward(x)
    st0 = net.shadow_stats()
    assert st0["checks"] == 1
    off = 0
    for name, shape in weight_spec(DESC):
        if name == "res1_conv0":
            break
        off += int(np.prod(shape))
    bad = small["w2"].copy()
    bad[off + 3] = 1e9
    with pytest.raises(RuntimeError, match=r"shadow: trunk conv 2 \(residual block 1\).*fp16's finite range"):
        net.set_weights(bad)
    after = net.forward(x)
    for b, a in zip(before, after):
        assert np.array_equal(b, a)
    st1 = net.shadow_stats()
    assert st1["checks"] == 2 and st1["max_abs_dp"] == st0["max_abs_dp"] and st1["sum_abs_dp"] == 2 * st0["sum_abs_dp"]
    net.close()


@gpu
def test_single_image_net_with_gemm_heads(hip_device):
    """10 x 10, 256 filters, policies of 3,041 moves: bf16 with a bf16x3 shadow, 3 rows of which 2 are
    checked."""
    blob = to_blob(random_weights(AMAZONS, 7923, bias_std=0.2))
    x = random_planes(AMAZONS, 3, 20260102)
    net = _net(AMAZONS, blob, hip_device, "bf16", ("bf16x3", 1, 2))
    got = net.forward(x)
    st = net.shadow_stats()
    a = _fresh_outputs(AMAZONS, blob, x[:2], hip_device, "bf16")
    b = _fresh_outputs(AMAZONS, blob, x[:2], hip_device, "bf16x3")
    _assert_totals(st, Restated().check(a, b).t, "amazons")
    assert (st["checks"], st["rows"], st["policy_elems"]) == (1, 2, 2 * 2 * 3041) and st["max_abs_dp"] > 0.0
    for g, p in zip(got, a):
        assert np.array_equal(g[:2], p)
    net.close()


@gpu
def test_logits_mode(small, hip_device):
    x = small["x"][:16]
    net = _net(DESC, small["w1"], hip_device, "bf16x3", ("fp32-ieee", 1, 16))
    net.set_output_logits(True)
    net.forward(x)
    st = net.shadow_stats()
    a = _fresh_outputs(DESC, small["w1"], x, hip_device, "bf16x3", logits=True)
    b = _fresh_outputs(DESC, small["w1"], x, hip_device, "fp32-ieee", logits=True)
    assert float(np.abs(a[0]).max()) > 1.0               # logits, not probabilities
    _assert_totals(st, Restated().check(a, b, logits=True).t, "logits")
    assert st["policy_rows"] == 0 and st["max_row_kl"] == 0.0 and st["sum_row_kl"] == 0.0
    assert st["max_abs_dp"] > 0.0 and st["policy_elems"] == 16 * 310
    net.close()


def _stats_bytes(net, reset=True):
    raw = net.shadow_stats_raw(reset)
    return raw, bytes(bytearray(raw))[:_native.GzShadowStats.device_ms.offset]


@gpu
def test_reproducible_totals(small, hip_device):
    """The same forwards give the same bits (device_ms apart): on two shadows enabled afresh, and again
    from a reset of the second -- there worst_check, a forward index counted from the enable, moves on
    by the number of forwards and everything else is byte-identical."""
    x = small["x"]
    sizes = [5, 16, 3, 13]

    def run(net):
        r0 = 0
        for k in sizes:
            net.forward(x[r0:r0 + k])
            r0 += k

    runs = []
    net = _net(DESC, small["w1"], hip_device, "bf16x3")
    for _ in range(2):
        net.enable_shadow("fp32-ieee", 1, 8)
        net.set_weights(small["w1"])
        run(net)
        runs.append(_stats_bytes(net, reset=False))
        if len(runs) == 1:
            net.disable_shadow()
    assert runs[0][0].checks == 4 and runs[0][0].rows == 5 + 8 + 3 + 8
    assert runs[0][1] == runs[1][1]
    net.shadow_stats(reset=True)
    run(net)
    raw, _ = _stats_bytes(net)
    assert raw.worst_check == runs[1][0].worst_check + len(sizes)
    raw.worst_check -= len(sizes)
    assert bytes(bytearray(raw))[:_native.GzShadowStats.device_ms.offset] == runs[1][1]
    net.close()


@gpu
def test_last_kernel_ms_times_the_net_alone(small, hip_device):
    """gz_net_last_kernel_ms's end event is recorded before the shadow's work: with every = 1 it stays
    within the run-to-run spread of the same net without a shadow (medians of three alternating
    pairs, 2x margin), while the fp32-ieee shadow forward alone is several times the net's."""
    x = small["x"][:32]
    plain = _net(DESC, small["w1"], hip_device, "bf16x3")
    shadowed = _net(DESC, small["w1"], hip_device, "bf16x3", ("fp32-ieee", 1, 32))
    for net in (plain, shadowed):
        net.forward(x)                                   # (first launches: allocations, code load)
    shadowed.shadow_stats(reset=True)
    t_plain, t_shadow = [], []
    for _ in range(3):
        plain.forward(x)
        t_plain.append(plain.last_kernel_ms())
        shadowed.forward(x)
        t_shadow.append(shadowed.last_kernel_ms())
    st = shadowed.shadow_stats()
    per_check = st["device_ms"] / st["checks"]
    print("last_kernel_ms plain %s shadowed %s; shadow work per check %.4f ms" % (t_plain, t_shadow, per_check))
    assert st["checks"] == 3
    assert np.median(t_shadow) <= 2.0 * np.median(t_plain), (t_plain, t_shadow)
    assert per_check > np.median(t_plain)                # the check is real work, and it is not in last_kernel_ms
    plain.close()
    shadowed.close()
