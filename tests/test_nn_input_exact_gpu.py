"""The input path, bit for bit: plane staging, im2col and the initial conv at every chunk count of the
im2col row, on both staging branches, on either side of the wave-group kernels' LDS edge and from
plane pointers off a 16-byte boundary.

The nets are exact_lattice's with cover_initial: every (tap, plane) place of the initial conv is read
by a +1 that no relu hides, and tests/test_nn_exact.py asserts on the CPU that removing any one place
moves an expected logit of the first row alone (exact_lattice.initial_liveness is empty), that
check_representable holds in every mode a case runs in, and that each slip an input path can make
(exact_lattice.INPUT_FAULTS, the historical chunk swizzle of forward_kernel.h among them) moves a
logit.  Every comparison here is np.array_equal with exact_lattice.expected_logits.

One residual block everywhere: the first trunk conv reads the images' zero rows, which the in-place
kernels' staging may have covered.  The im2col row has K0 = places rounded up to 32 entries, K0 / 8
chunks; the sweep holds one plane count per chunk count from 4 to 36.

Refused by net creation for LDS (REFUSED; test_refused asserts the message), one per chunk count at most:
  in_19x19_c12_f128  bf16x3  16 chunks: 203,696 B for the two-pass split kernel (its largest C is 10), so
                             the plane block above the float4 prefetch's cap runs in bf16 alone there;
                             16 chunks run in both fused modes on 8 x 8 with 64 and with 128 filters
  in_13x13_c22_f256  bf16x3  28 chunks: 169,248 B, one plane more than the largest net of that mode
  in_13x13_c43_f256  bf16    52 chunks: 172,560 B, one plane more than the largest net of that mode
Every chunk count from 4 to 36 runs in bf16 and in bf16x3 on 8 x 8 boards with 64 and with 128 filters.
"""
import dataclasses

import numpy as np
import pytest

import exact_lattice as xl
from galvanise_zero_amd.nn.desc import NetDesc
from galvanise_zero_amd.nn.weights import to_blob
from gpu_helpers import Pinned

pytestmark = pytest.mark.gpu

FUSED = ("bf16", "bf16x3")
LAYERED = ("fp32-ieee", "bf16-layered", "bf16x3-layered", "fp16x3-layered")
ALL = FUSED + LAYERED
ROWS = (1, 2, 3, 5)
LARGE_ROWS = 300       # above large_min_rows() = 257: the large-launch default runs


@dataclasses.dataclass
class Case:
    desc: NetDesc
    modes: tuple
    seed: int = 1           # the weights' seed: the smallest at which test_nn_exact.py's conditions, liveness and faults hold


def _d(C, H, W, F, P, **kw):
    return NetDesc(C, H, W, F, 1, [P, P + 1], **kw)


# (plane count, K0) of the 3 x 3 sweep: one plane count per chunk count K0 / 8 = 4, 8, .. 36
SWEEP = ((3, 32), (7, 64), (9, 96), (14, 128), (15, 160), (21, 192), (24, 224), (28, 256), (32, 288))
CASES = {}
for _c, _k0 in SWEEP:
    for _f in (64, 128):
        CASES["in_8x8_c%d_f%d" % (_c, _f)] = Case(_d(_c, 8, 8, _f, 155), FUSED)
# the layered modes' gather_kernel pads C to a multiple of 16: both sides of 16 and of 32
CASES["in_8x8_c15_f64"].modes = ALL
for _c in (16, 17, 33):
    CASES["in_8x8_c%d_f64" % _c] = Case(_d(_c, 8, 8, 64, 155), ALL)
# a 1 x 1 initial conv (v2): K0 = 32 padded, 32 exactly, 64
for _c in (3, 32, 33):
    CASES["in_v2_8x8_c%d_f128" % _c] = Case(_d(_c, 8, 8, 128, 155, resnet_v2=True), ALL)
# plane blocks that are no whole number of float4s (210, 125 floats a plane set of 5): every board but the
# first off alignment, the scalar staging loop; C = 9 beside it, and C = 32 for the 36-chunk row
for _h, _w, _p in ((6, 7, 85), (5, 5, 50)):
    for _c in (5, 9):
        CASES["in_%dx%d_c%d_f128" % (_h, _w, _c)] = Case(_d(_c, _h, _w, 128, _p), FUSED)
CASES["in_6x7_c32_f128"] = Case(_d(32, 6, 7, 128, 85), FUSED)
# the single-image kernels
for _c in (9, 21):
    CASES["in_10x10_c%d_f256" % _c] = Case(_d(_c, 10, 10, 256, 101), FUSED)
# 13 x 13, F = 256: C = 9 and the largest C whose net is created, 21 in bf16x3 and 42 in bf16 (48 chunks)
for _c, _modes in ((9, FUSED), (21, FUSED), (42, ("bf16",))):
    CASES["in_13x13_c%d_f256" % _c] = Case(_d(_c, 13, 13, 256, 170), _modes)
# 19 x 19: 1,444 floats take the float4 prefetch, 4,332 are above its cap of 4,096 (the scalar loop)
CASES["in_19x19_c4_f128"] = Case(_d(4, 19, 19, 128, 362), FUSED)
CASES["in_19x19_c12_f128"] = Case(_d(12, 19, 19, 128, 362), ("bf16",))
# {name: (desc, mode)} that net creation refuses for LDS
REFUSED = {"in_19x19_c12_f128": (_d(12, 19, 19, 128, 362), "bf16x3"), "in_13x13_c22_f256": (_d(22, 13, 13, 256, 170), "bf16x3"),
           "in_13x13_c43_f256": (_d(43, 13, 13, 256, 170), "bf16")}
# the wave-group kernels' LDS edge at 8 x 8, F = 128, split precision: the staging of C = 12 fits a group's
# image by 96 bytes, that of C = 13 does not
EDGE_FITS, EDGE_OVER = "in_8x8_c12_f128", "in_8x8_c13_f128"
for _c in (12, 13):
    CASES["in_8x8_c%d_f128" % _c] = Case(_d(_c, 8, 8, 128, 155), FUSED)
# the in-place kernels on small plane counts, whose staging leaves the images' zero rows uncovered; 7 x 8: the
# in-place kernel with a board per group (variant 26)
for _c in (3, 9):
    CASES["in_7x8_c%d_f128" % _c] = Case(_d(_c, 7, 8, 128, 113), ("bf16x3",))
SEEDS = {"in_8x8_c21_f64": 2, "in_8x8_c24_f64": 5, "in_8x8_c32_f64": 2, "in_8x8_c32_f128": 8, "in_8x8_c17_f64": 2, "in_8x8_c33_f64": 5,
         "in_6x7_c32_f128": 8}
for _name, _seed in SEEDS.items():
    CASES[_name].seed = _seed

# the sweep on the two-board kernels that take the large launches (variant 21; 64 filters in split precision have none)
TWO_BOARDS = [("in_8x8_c%d_f%d" % (c, f), mode) for c, _ in SWEEP for f, mode in ((64, "bf16"), (128, "bf16"), (128, "bf16x3"))]
IN_PLACE = [(c, v) for c in (3, 9) for v in ("23", "25", "26")]
KERNELS = {"22": "gznn::trunk_kernel8<128, 4, 3>", "23": "gznn::trunk_kernel_h2<128, 4, 3>", "25": "gznn::trunk_kernel_h2i<128, 4, 3>",
           "26": "gznn::trunk_kernel_h2ig<128, 4, 3>"}
MISALIGNED = [("bf16x3", v) for v in ("11", "21", "23", "25")] + [("bf16", None)]

_cache = {}


def build(name, rows=None):
    """(desc, weights, planes, expected logits) of a case at 5 rows (or `rows`), computed once."""
    key = (name, rows)
    if key not in _cache:
        c = CASES[name]
        n = rows or max(ROWS)
        w = xl.lattice_weights(c.desc, c.seed, nnz=2, wmax=1, cover_initial=True)
        x = xl.input_planes(c.desc, n, 100 + n)
        _cache[key] = (c.desc, w, x, xl.expected_logits(c.desc, w, x))
    return _cache[key]


def _net(desc, w, device, mode):
    from galvanise_zero_amd._native import HipNet
    net = HipNet(desc, device, mode)
    net.set_weights(to_blob(w))
    net.set_output_logits(True)
    return net


def _assert_equal(tag, got, expected, rows):
    assert len(got) == len(expected)
    for i, (g, e) in enumerate(zip(got, expected)):
        e32 = e[rows].astype(np.float32)
        assert np.array_equal(e32.astype(np.float64), e[rows])
        assert np.array_equal(g, e32), (tag, i, int((g != e32).sum()), float(np.abs(g.astype(np.float64) - e[rows]).max()))


def _assert_exact(tag, net, x, expected, n):
    _assert_equal((tag, n), net.forward(x[:n]), expected, slice(0, n))


@pytest.mark.parametrize("name,mode", [(name, mode) for name, c in CASES.items() for mode in c.modes])
def test_exact(name, mode, hip_device, monkeypatch):
    """The logits equal the oracle's at 1, 2, 3 and 5 rows."""
    monkeypatch.delenv("GZ_KERNEL_VARIANT", raising=False)
    desc, w, x, expected = build(name)
    net = _net(desc, w, hip_device, mode)
    for n in ROWS:
        _assert_exact((name, mode), net, x, expected, n)
    net.close()


@pytest.mark.parametrize("name,mode", TWO_BOARDS)
def test_sweep_two_boards(name, mode, hip_device, monkeypatch):
    """Every chunk count on the two-board kernel, whose boards share one staging scratch and one im2col
    image: 5 rows (a dead board in the last workgroup) and 2."""
    monkeypatch.setenv("GZ_KERNEL_VARIANT", "21")
    desc, w, x, expected = build(name)
    net = _net(desc, w, hip_device, mode)
    kernel = "gznn::trunk_kernel<%d, 4, 2, 1, %d>" % (desc.cnn_filter_size, 3 if mode == "bf16x3" else 1)
    assert net.kernel_name(False) == net.kernel_name(True) == kernel
    for n in (5, 2):
        _assert_exact((name, mode, "21"), net, x, expected, n)
    net.close()


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused(name, hip_device, monkeypatch):
    """The cases that net creation refuses for LDS, by its message."""
    from galvanise_zero_amd._native import HipNet
    monkeypatch.delenv("GZ_KERNEL_VARIANT", raising=False)
    desc, mode = REFUSED[name]
    with pytest.raises(RuntimeError, match=r"network needs \d+ B of LDS per workgroup \(160 KB max\)"):
        HipNet(desc, hip_device, mode).close()


@pytest.mark.parametrize("name,kernel", [(EDGE_FITS, "gznn::trunk_kernel_h2i<128, 4, 3>"), (EDGE_OVER, "gznn::trunk_kernel<128, 4, 2, 1, 3>")])
def test_selection_edge(name, kernel, hip_device, monkeypatch):
    """C = 12: the in-place wave-group kernel takes the large launches.  C = 13: its staging is 160 bytes
    larger than a group's image, and the two-board kernel with an image set of its own takes them, still
    from 257 rows.  Both exact at 300 rows and at 5."""
    monkeypatch.delenv("GZ_KERNEL_VARIANT", raising=False)
    desc, w, x, expected = build(name, LARGE_ROWS)
    net = _net(desc, w, hip_device, "bf16x3")
    assert net.kernel_name(True) == kernel, net.kernel_name(True)
    assert net.large_min_rows() == 257 and net.kernel_name(False) == "gznn::trunk_kernel<128, 4, 1, 1, 3>"
    for n in (LARGE_ROWS, 5):
        _assert_exact((name, "selection"), net, x, expected, n)
    net.close()


@pytest.mark.parametrize("variant", ("22", "23", "25", "26"))
def test_selection_edge_refuses_forced_wave_groups(variant, hip_device, monkeypatch):
    """C = 13 under a forced wave-group variant: no kernel, not a staging that overruns the image."""
    from galvanise_zero_amd._native import HipNet
    monkeypatch.setenv("GZ_KERNEL_VARIANT", variant)
    with pytest.raises(RuntimeError, match="unsupported network geometry"):
        HipNet(CASES[EDGE_OVER].desc, hip_device, "bf16x3").close()


def test_eight_wave_groups_at_the_edge(hip_device, monkeypatch):
    """Variant 22 (two groups of four waves) has the same image as 23 and 25, so the same edge: exact at
    C = 12.  (With 64 filters there is no wave-group kernel at any plane count: test_f64_has_no_wave_groups.)"""
    monkeypatch.setenv("GZ_KERNEL_VARIANT", "22")
    desc, w, x, expected = build(EDGE_FITS)
    net = _net(desc, w, hip_device, "bf16x3")
    assert net.kernel_name(False) == net.kernel_name(True) == KERNELS["22"]
    for n in (5, 2):
        _assert_exact((EDGE_FITS, "22"), net, x, expected, n)
    net.close()


@pytest.mark.parametrize("C", (24, 25))
def test_f64_has_no_wave_groups(C, hip_device, monkeypatch):
    """F = 64, variant 22: trunk_variants.h compiles the wave-group kernels for rows of 16 chunks and
    more (F = 128), so creation is refused whatever the plane count -- there is no wg_fits edge to find."""
    from galvanise_zero_amd._native import HipNet
    monkeypatch.setenv("GZ_KERNEL_VARIANT", "22")
    with pytest.raises(RuntimeError, match="unsupported network geometry"):
        HipNet(_d(C, 8, 8, 64, 155), hip_device, "bf16x3").close()


@pytest.mark.parametrize("C,variant", IN_PLACE)
def test_in_place_small_plane_counts(C, variant, hip_device, monkeypatch):
    """C = 3 and 9 under the wave-group kernels, at 5 rows and at 2: the staging of so few planes ends
    below the image's zero rows, which the in-place kernels (25: row pairs at 8 x 8; 26: a board per
    group, on a 7 x 8 board) zero after staging all the same."""
    name = "in_%s_c%d_f128" % ("7x8" if variant == "26" else "8x8", C)
    monkeypatch.setenv("GZ_KERNEL_VARIANT", variant)
    desc, w, x, expected = build(name)
    net = _net(desc, w, hip_device, "bf16x3")
    assert net.kernel_name(False) == net.kernel_name(True) == KERNELS[variant]
    for n in (5, 2):
        _assert_exact((name, variant), net, x, expected, n)
    net.close()


def _segments(net, desc, x, cuts, offsets, placement, keep):
    """forward_segments over x cut into `cuts` rows, segment i's planes `offsets[i]` bytes behind a
    16-byte boundary, in HBM or in pinned host memory.  [policy.., value] float32, rows in order."""
    import torch
    P, V = list(desc.policy_dist_count), desc.num_values
    segs, outs, row = [], [], 0
    for n, off in zip(cuts, offsets):
        part = x[row:row + n].reshape(-1)
        row += n
        assert off % 4 == 0
        if placement == "device":
            tp = torch.zeros(part.size + 4, device="cuda")
            tp[off // 4:off // 4 + part.size] = torch.from_numpy(part.copy()).cuda()
            ptr = tp.data_ptr()
            tpol = [torch.full((n * p,), -1.0, device="cuda") for p in P]
            tval = torch.full((n * V,), -1.0, device="cuda")
            keep += [tp, tval] + tpol
            out = (lambda tpol=tpol, tval=tval: [t.cpu().numpy() for t in tpol] + [tval.cpu().numpy()])
            ptrs = ([t.data_ptr() for t in tpol], tval.data_ptr())
        else:
            bp = Pinned(part.size + 4)
            bp.a[:] = 0.0
            bp.a[off // 4:off // 4 + part.size] = part
            ptr = bp.ptr.value
            bpol = [Pinned(n * p) for p in P]
            bval = Pinned(n * V)
            for b in bpol + [bval]:
                b.a[:] = -1.0
            keep += [bp, bval] + bpol
            out = (lambda bpol=bpol, bval=bval: [b.a.copy() for b in bpol] + [bval.a.copy()])
            ptrs = ([b.ptr.value for b in bpol], bval.ptr.value)
        assert ptr % 16 == 0
        segs.append((n, ptr + off, ptrs[0], ptrs[1]))
        outs.append((n, out))
    net.forward_segments(torch.cuda.current_stream().cuda_stream, segs)
    torch.cuda.synchronize()
    parts = [[a.reshape(n, -1) for a in out()] for n, out in outs]
    return [np.concatenate([p[i] for p in parts]) for i in range(len(P) + 1)]


@pytest.mark.parametrize("mode,variant", MISALIGNED)
def test_misaligned_segments(mode, variant, hip_device, monkeypatch):
    """Plane pointers 4, 8 and 12 bytes behind a 16-byte boundary, in HBM and in pinned host memory:
    5 rows cut 1 + 2 + 2 with the middle segment off alignment and then the outer two, so that a
    two-board workgroup holds a board of each kind (boards 0 | 1, 2 | 3 and 4 | none) and the float4
    prefetch is decided per board.  The outputs equal the expected logits and the aligned flat forward."""
    if variant:
        monkeypatch.setenv("GZ_KERNEL_VARIANT", variant)
    else:
        monkeypatch.delenv("GZ_KERNEL_VARIANT", raising=False)
    desc, w, x, expected = build(EDGE_FITS)
    net = _net(desc, w, hip_device, mode)
    flat = net.forward(x)
    _assert_equal((mode, variant, "flat"), flat, expected, slice(0, 5))
    for placement in ("device", "pinned"):
        keep = []
        for off in (4, 8, 12):
            for offsets in ((0, off, 0), (off, 0, off)):
                got = _segments(net, desc, x, (1, 2, 2), offsets, placement, keep)
                _assert_equal((mode, variant, placement, offsets), got, expected, slice(0, 5))
                for g, f in zip(got, flat):
                    assert np.array_equal(g, f)
        if placement == "pinned":
            for b in keep:
                b.free()
    net.close()
