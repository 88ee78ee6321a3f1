"""The "fp16x3-layered" arithmetic mode (GZ_PRECISION_F16X3_LAYERED = 7) without a GPU: its name and
ABI value, gz_net_create's checks in front of the device -- the layered modes' geometries and
refusals -- and the mode's arithmetic restated on the CPU under AddressSanitizer / UBSan (a
stand-alone program: nothing sanitised is loaded into Python)."""
import os
import re

import pytest

from galvanise_zero_amd import _native
from galvanise_zero_amd.nn.desc import NetDesc
from test_fp32_mode import _run_sanitised
from test_layered_mode import ACCEPTED, _hex19
from test_v2_f256 import REFUSALS, V2, _create_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE = "fp16x3-layered"


def test_name_and_abi():
    assert _native.PRECISIONS[MODE] == _native.GZ_PRECISION_F16X3_LAYERED == 7
    assert _native.canonical_precision(MODE) == MODE
    with open(os.path.join(ROOT, "include", "gzero_nn.h")) as f:
        header = f.read()
    m = re.search(r"^#define\s+GZ_PRECISION_F16X3_LAYERED\s+(\d+)\s*$", header, re.M)
    assert m and int(m.group(1)) == 7
    # the existing names keep their values
    assert _native.PRECISIONS["bf16"] == 1 and _native.PRECISIONS["bf16x3"] == _native.PRECISIONS["split"] == 3
    assert _native.PRECISIONS["fp32"] == 3 and _native.PRECISIONS["fp32-ieee"] == 4
    assert _native.PRECISIONS["bf16-layered"] == 5 and _native.PRECISIONS["bf16x3-layered"] == 6
    assert len(_native.PRECISIONS) == 8 and sorted(_native._CANONICAL) == [1, 3, 4, 5, 6, 7]
    for macro, value in (("GZ_PRECISION_BF16", 1), ("GZ_PRECISION_SPLIT", 3), ("GZ_PRECISION_FP32", 4),
                         ("GZ_PRECISION_BF16_LAYERED", 5), ("GZ_PRECISION_SPLIT_LAYERED", 6)):
        m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % macro, header, re.M)
        assert m and int(m.group(1)) == value
    # plain "fp16" names no mode
    with pytest.raises(ValueError) as e:
        _native.canonical_precision("fp16")
    assert MODE in str(e.value)


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_geometry_accepted(name):
    """The nets the layered modes take get past every refusal that needs no device (they all precede
    the first HIP call): past them gz_net_create needs a device, which this host may lack, so any
    other error (or none) means accepted."""
    created, err = _create_error(ACCEPTED[name], MODE)
    print("%s %s: %s" % (name, MODE, "created" if created else err))
    for text in REFUSALS:
        assert text not in err, (name, err)
    assert "unknown precision" not in err


def test_refusals_that_stay():
    """Boards above 19 x 19, 129 squeeze-excite units and 257 filters keep the layered modes' messages."""
    created, err = _create_error(NetDesc(**dict(_hex19(), input_columns=21, input_rows=21)), MODE)
    assert not created and "unsupported network geometry F=80 H=21 W=21" in err, err
    assert "layered modes: boards up to 19 x 19, F <= 256" in err, err
    created, err = _create_error(NetDesc(5, 8, 8, 256, 2, [155, 155], se_units=129, **V2), MODE)
    assert not created and "squeeze-excite units must be 0..128" in err, err
    created, err = _create_error(NetDesc(5, 19, 19, 257, 2, [362, 362]), MODE)
    assert not created and "unsupported network geometry F=257 H=19 W=19" in err, err


def test_host_check_sanitised(tmp_path):
    """tests/fp16x3_host_check.cpp: gzlayered::conv_f16_kernel's conv restated on the CPU from
    csrc/nn/layered_forward.h's index functions, board_exponent and pack_image_host's fp16 image, in
    the mode's arithmetic, against a float64 convolution: a 5 x 4 legacy board with F 40 -> 64, 19 x 19
    with F = 256 at 2 rows (a tile straddles the boards), a 3 x 3 initial conv with K0 = 160 -- within
    4e-6 relative and more than 10 x closer than the same operands as bf16 hi + lo; inputs reaching
    1e6 stay finite at that bound and are not finite with the exponents forced to 0; board_exponent's
    edge values; a row alone equals the row in a two-board tile bit for bit; f2h rounds to nearest
    even.  Built with -fsanitize=address,undefined."""
    p = _run_sanitised(tmp_path, "fp16x3_host_check")
    assert p.returncode == 0, p.stdout[-4000:]
    assert "FAILED" not in p.stdout
    assert len(re.findall(r"^\S+ (?:initial|trunk): pointwise \S+ tensor fp16x3 \S+ bf16x3 \S+ \(ratio \S+\)$", p.stdout, re.M)) == 5
    for text in ("5x4_legacy trunk", "19x19_f256 trunk", "K0=160", "range: inputs to 1e6", "exponents forced to 0: finite 0",
                 "row invariance: a row alone == the row in a two-board tile: identical", "board_exponent:", "f2h:",
                 "range check: names the conv"):
        assert text in p.stdout, text
