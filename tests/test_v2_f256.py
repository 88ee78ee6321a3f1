"""v2 (pre-activation, squeeze-excite) nets with up to 256 filters, without a GPU: gz_net_create's
checks in front of the device (geometry, squeeze-excite units, the 160 KB of LDS) for the new
geometries in all three arithmetic modes, and the weight image of two such nets packed by a
stand-alone host program under AddressSanitizer / UBSan (nothing sanitised is loaded into Python).

The LDS arithmetic behind the depth limits (csrc/nn/gz_nn.hip, forward_kernel.h Geo): a 256-filter
image row is 768 bytes in bf16 and in the two-pass split, 1,056 in the single-image split; each
residual block adds 2 x 256 x 4 = 2,048 bytes of bias table; squeeze-excite adds (256 + S) x 4
bytes rounded up to 16; concat_all_layers adds 16 x positions rounded up to 16.

  board    mode      image       blocks that fit (no SE / SE 85 / SE 85 + concat_all_layers)
  8 x 8    bf16      2 x 50,688  30 / 29 / 29
  8 x 8    bf16x3    50,688      55 / 54 / 54
  10 x 10  bf16      87,552      37 / 36 / 35
  10 x 10  bf16x3    121,440     20 / 20 / 19   (20 x 256 with SE 85: 64 bytes to spare)
  13 x 13  both      136,704     13 / 12 / 11
"""
import ctypes
import re

import pytest

from galvanise_zero_amd import _native
from galvanise_zero_amd.nn.desc import NetDesc, blob_size
from test_fp32_mode import _run_sanitised

MODES = ["bf16", "bf16x3", "fp32-ieee"]
V2 = dict(resnet_v2=True, global_pooling_value=True, value_bn=True)

ACCEPTED = {
    "8x8_f256": NetDesc(5, 8, 8, 256, 2, [155, 155], se_units=85, **V2),
    "10x10_f192": NetDesc(12, 10, 10, 192, 2, [3041, 3041], num_values=3, se_units=64, **V2),
    "13x13_f256": NetDesc(5, 13, 13, 256, 2, [170, 171], se_units=85, **V2),
    # the v2 twins of BASELINE cfg4 (hexLG13 12 x 256) and cfg5 (amazons 20 x 256), built the
    # reference's way: squeeze-excite with filters // 3 units, the pooling value head
    "cfg4_v2": NetDesc(5, 13, 13, 256, 12, [170, 171], se_units=256 // 3, **V2),
    "cfg5_v2": NetDesc(12, 10, 10, 256, 20, [3041, 3041], se_units=256 // 3, **V2),
}
REFUSALS = ("unsupported network geometry", "squeeze-excite units", "LDS")


def _create_error(desc, mode):
    """gz_net_create's error text, "" when it succeeded (a host with a device)."""
    lib = _native.nn_lib()
    cdesc = _native.make_net_desc(desc, _native.PRECISIONS[mode])
    h = lib.gz_net_create(ctypes.byref(cdesc), 0)
    err = "" if h else lib.gz_nn_last_error().decode()
    if h:
        lib.gz_net_destroy(h)
    return bool(h), err


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_geometry_accepted(name, mode):
    """Every refusal that needs no device comes before the first HIP call: past them gz_net_create
    needs a device, which this host may lack, so any other error (or none) means accepted."""
    created, err = _create_error(ACCEPTED[name], mode)
    print("%s %s: %s" % (name, mode, "created" if created else err))
    for text in REFUSALS:
        assert text not in err, (name, mode, err)


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_19x19_f256_refused(mode):
    """The 19 x 19 image of a 256-filter net does not fit the LDS: refused with the geometry message
    in the LDS-image modes (fp32-ieee is the path there, and accepts it)."""
    desc = NetDesc(5, 19, 19, 256, 2, [362, 362], se_units=85, **V2)
    created, err = _create_error(desc, mode)
    assert not created and "unsupported network geometry F=256 H=19 W=19" in err, err
    assert "F <= 128" not in err
    _, err32 = _create_error(desc, "fp32-ieee")
    for text in REFUSALS:
        assert text not in err32, err32


@pytest.mark.parametrize("mode", MODES)
def test_se_units_cap(mode):
    """128 units are taken (the reference's filters // 3 is 85 at 256 filters), 129 are refused with
    the cap named."""
    _, err = _create_error(NetDesc(5, 8, 8, 256, 2, [155, 155], se_units=128, **V2), mode)
    for text in REFUSALS:
        assert text not in err, err
    created, err = _create_error(NetDesc(5, 8, 8, 256, 2, [155, 155], se_units=129, **V2), mode)
    assert not created and "squeeze-excite units must be 0..128" in err, err


def test_13x13_depth_limit():
    """13 x 13 with 256 filters in bf16x3 (and bf16: the same 768-byte rows): the image's 178 rows
    take 136,704 bytes, so 13 blocks' bias table (26,624) still fits the 163,840 bytes of LDS and 14
    blocks' (28,672) do not -- reported before any device call, with the byte count.  With 85
    squeeze-excite units (1,376 bytes) the limit is 12 blocks: BASELINE cfg4's depth."""
    def desc(B, se):
        return NetDesc(5, 13, 13, 256, B, [170, 171], resnet_v2=True, se_units=se)
    for mode in ("bf16", "bf16x3"):
        for B, se, fits in ((13, 0, True), (14, 0, False), (12, 85, True), (13, 85, False)):
            created, err = _create_error(desc(B, se), mode)
            if fits:
                assert "LDS" not in err and "unsupported" not in err, (mode, B, se, err)
            else:
                assert not created and "of LDS per workgroup (160 KB max)" in err, (mode, B, se, err)
                need = 136704 + 2048 * B + (1376 if se else 0)
                assert "needs %d B" % need in err, (mode, B, se, err)
    # fp32-ieee keeps no image in the LDS: no depth limit
    _, err = _create_error(desc(14, 85), "fp32-ieee")
    assert "LDS" not in err and "unsupported" not in err, err


def test_10x10_split_depth_limit():
    """10 x 10 in bf16x3 (single-image split, 1,056-byte rows: 121,440 bytes): 20 blocks with 85
    squeeze-excite units fit by 64 bytes, 21 blocks do not."""
    def desc(B):
        return NetDesc(12, 10, 10, 256, B, [3041, 3041], se_units=85, **V2)
    _, err = _create_error(desc(20), "bf16x3")
    assert "LDS" not in err, err
    created, err = _create_error(desc(21), "bf16x3")
    assert not created and "needs %d B of LDS" % (121440 + 21 * 2048 + 1376) in err, err


def test_weight_image_v2_f256_sanitised(tmp_path):
    """tests/weight_image_v2_f256_check.cpp: the weight image of (a) v2 5 x 8 x 8, F 192 -> 256, two
    blocks, SE 64, pooling value head + BN and (b) v2 5 x 13 x 13, F = 256, two blocks, SE 85,
    concat_all_layers, packed on the CPU as bf16, bf16x3 and fp32 into heap buffers of exactly the
    image's size.  The blob plan must consume blob_size(desc) floats (passed in); the program
    asserts the rest (no write outside the image or twice, padded channels zero)."""
    descs = [
        NetDesc(5, 8, 8, 192, 2, [155, 155], value_hidden_size=6, resnet_v2=True, se_units=64,
                global_pooling_value=True, value_bn=True),
        NetDesc(5, 13, 13, 256, 2, [170, 171], value_hidden_size=6, resnet_v2=True, se_units=85,
                concat_all_layers=True),
    ]
    p = _run_sanitised(tmp_path, "weight_image_v2_f256_check", [blob_size(d) for d in descs])
    assert p.returncode == 0, p.stdout[-4000:]
    assert len(re.findall(r"^case [ab] (p2=1|p2=2|fp32): ", p.stdout, re.M)) == 6
