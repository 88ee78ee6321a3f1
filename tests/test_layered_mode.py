"""The layered arithmetic modes ("bf16-layered" / "bf16x3-layered", GZ_PRECISION_BF16_LAYERED /
GZ_PRECISION_SPLIT_LAYERED) without a GPU: their names and ABI values, gz_net_create's checks in
front of the device for the nets the fused modes refuse, and the conv kernel's index arithmetic
walked on the CPU under AddressSanitizer / UBSan (a stand-alone program: nothing sanitised is loaded
into Python)."""
import json
import os
import re
import warnings

import pytest

from galvanise_zero_amd import _native
from galvanise_zero_amd.nn.desc import NetDesc
from test_fp32_mode import _run_sanitised
from test_v2_f256 import REFUSALS, V2, _create_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["bf16-layered", "bf16x3-layered"]


def _hex19():
    with open(os.path.join(ROOT, "tests", "golden", "keras_descs.json")) as f:
        return json.load(f)["hex19/models/h2_477.json"]["desc"]


ACCEPTED = {
    # the textbook shape on a 19 x 19 board: refused by both fused modes (test_v2_f256)
    "19x19_f256": NetDesc(5, 19, 19, 256, 2, [362, 362], se_units=85, **V2),
    # one block past the fused modes' 13 x 13 limits (13 without squeeze-excite, 12 with)
    "13x13_b14": NetDesc(5, 13, 13, 256, 14, [170, 171], resnet_v2=True),
    "13x13_b13_se85": NetDesc(5, 13, 13, 256, 13, [170, 171], resnet_v2=True, se_units=85),
    # and past bf16x3's 20 blocks at 10 x 10
    "10x10_b21": NetDesc(12, 10, 10, 256, 21, [3041, 3041], se_units=85, **V2),
    "hex19_h2_477": NetDesc(**_hex19()),
}


def test_names_and_abi():
    assert _native.PRECISIONS["bf16-layered"] == _native.GZ_PRECISION_BF16_LAYERED == 5
    assert _native.PRECISIONS["bf16x3-layered"] == _native.GZ_PRECISION_SPLIT_LAYERED == 6
    for name in MODES:
        assert _native.canonical_precision(name) == name
    with open(os.path.join(ROOT, "include", "gzero_nn.h")) as f:
        header = f.read()
    for macro, value in (("GZ_PRECISION_BF16_LAYERED", 5), ("GZ_PRECISION_SPLIT_LAYERED", 6)):
        m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % macro, header, re.M)
        assert m and int(m.group(1)) == value
    with pytest.raises(ValueError) as e:
        _native.canonical_precision("fp16")
    for name in MODES + ["fp32-ieee", "bf16x3"]:
        assert name in str(e.value)
    # the existing names keep their meaning
    assert _native.PRECISIONS["bf16"] == 1 and _native.PRECISIONS["bf16x3"] == _native.PRECISIONS["split"] == 3
    assert _native.PRECISIONS["fp32-ieee"] == 4
    assert _native.canonical_precision("bf16") == "bf16"
    assert _native.canonical_precision("bf16x3") == _native.canonical_precision("split") == "bf16x3"
    assert _native.canonical_precision("fp32-ieee") == "fp32-ieee"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert _native.canonical_precision("fp32") == "bf16x3"
    assert any(issubclass(x.category, DeprecationWarning) for x in w)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_geometry_accepted(name, mode):
    """None of the refusals that need no device (they all precede the first HIP call): past them
    gz_net_create needs a device, which this host may lack, so any other error (or none) means
    accepted."""
    created, err = _create_error(ACCEPTED[name], mode)
    print("%s %s: %s" % (name, mode, "created" if created else err))
    for text in REFUSALS:
        assert text not in err, (name, mode, err)
    assert "unknown precision" not in err


@pytest.mark.parametrize("mode", MODES)
def test_refusals_that_stay(mode):
    """Boards above 19 x 19 keep the geometry message, 129 squeeze-excite units the cap's."""
    created, err = _create_error(NetDesc(**dict(_hex19(), input_columns=21, input_rows=21)), mode)
    assert not created and "unsupported network geometry F=80 H=21 W=21" in err, err
    created, err = _create_error(NetDesc(5, 8, 8, 256, 2, [155, 155], se_units=129, **V2), mode)
    assert not created and "squeeze-excite units must be 0..128" in err, err
    created, err = _create_error(NetDesc(5, 19, 19, 257, 2, [362, 362]), mode)
    assert not created and "unsupported network geometry F=257 H=19 W=19" in err, err


def test_host_check_sanitised(tmp_path):
    """tests/layered_host_check.cpp: the conv restated on the CPU from csrc/nn/layered_forward.h's
    index functions alone (LDS row of a column and tap, staged channel offset, B-fragment address,
    the wres_index / w0 A-fragment offsets) over pack_image_host's weights, against a direct
    convolution of the same bf16-rounded operands, in both part counts: a 5 x 4 legacy board with F
    40 -> 64, 19 x 19 with F = 256 at 2 rows (a tile straddles the boards) and its 1 x 1 initial
    conv, a 3 x 3 initial conv with 15 planes (K0 = 160); the layered image equals the fused one
    byte for byte; the LDS row strides are conflict-free for the B-fragment reads.  Built with
    -fsanitize=address,undefined."""
    p = _run_sanitised(tmp_path, "layered_host_check")
    assert p.returncode == 0, p.stdout[-4000:]
    assert len(re.findall(r"max rel err initial \S+ trunk \S+$", p.stdout, re.M)) == 5
    for text in ("5x4_legacy P=1", "5x4_legacy P=3", "19x19_f256 P=3", "K0=160", "image p2=1", "image p2=2"):
        assert text in p.stdout, text
