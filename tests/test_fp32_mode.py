"""The exact-fp32 arithmetic mode ("fp32-ieee", GZ_PRECISION_FP32) without a GPU: the conv kernel's
index arithmetic walked on the CPU under AddressSanitizer / UBSan (a stand-alone program: nothing
sanitised is loaded into Python), the mode's names and ABI value, and gz_net_create's geometry check
(which precedes any HIP call)."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import warnings

import pytest

from galvanise_zero_amd import _native
from galvanise_zero_amd.nn.desc import NetDesc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_sanitised(tmp_path):
    """tests/fp32_host_check.cpp: csrc/nn/fp32_forward.h's helpers (neighbour / zero-row index, LDS
    row stride, weight-fragment index, chunk bounds) and host packing routine run a conv with the
    kernel's tiling on 6 x 6 .. 19 x 19 boards, F 64 / 80 -> 128 / 256, 3 / 15 / 24 planes, against
    a naive 'same' conv, every index asserted in bounds -- built with -fsanitize=address,undefined."""
    p = _run_sanitised(tmp_path, "fp32_host_check")
    assert p.returncode == 0, p.stdout[-4000:]
    assert len(re.findall(r"max rel err", p.stdout)) >= 40
    for side in (6, 8, 13, 19):
        assert "H=%d W=%d" % (side, side) in p.stdout


def _run_sanitised(tmp_path, name, args=()):
    """Builds tests/<name>.cpp with -fsanitize=address,undefined and runs it."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / name)
    # (the sanitizer runtimes linked into the program itself)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                   ["-o", exe, os.path.join(ROOT, "tests", name + ".cpp")], check=True)
    p = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(p.stdout)
    return p


def test_weight_image_host_check_sanitised(tmp_path):
    """tests/weight_image_host_check.cpp: csrc/nn/weight_image.h's job list packed on the CPU for
    four small nets -- (a) legacy v1 on a 5 x 4 board, F 40 -> 64, (b) v2 with F 96 -> 128, a bare
    3 x 3 initial conv, squeeze-excite and the pooling value head, (c) v2 concat_all_layers, (d) the
    GEMM heads' fragments of a 530-move policy on 2 HW = 50 inputs -- each as bf16, bf16x3 and fp32,
    into heap buffers of exactly the image's size.  The blob plan must consume the float count
    weight_spec gives for the same desc (passed in); the program asserts the rest."""
    from galvanise_zero_amd.nn.desc import blob_size
    descs = [
        NetDesc(3, 5, 4, 40, 1, [7, 9], value_hidden_size=6, conv_bias=True, value_bn=True, value_sigmoid=True),
        NetDesc(5, 6, 6, 96, 2, [37, 37], value_hidden_size=6, resnet_v2=True, initial_kernel_size=3, initial_bn=False,
                se_units=4, global_pooling_value=True, value_bn=True),
        NetDesc(3, 4, 3, 40, 2, [13], value_hidden_size=6, resnet_v2=True, concat_all_layers=True),
        NetDesc(3, 5, 5, 40, 1, [530], value_hidden_size=6),
    ]
    p = _run_sanitised(tmp_path, "weight_image_host_check", [blob_size(d) for d in descs])
    assert p.returncode == 0, p.stdout[-4000:]
    assert len(re.findall(r"^case [abcd] (p2=1|p2=2|fp32): ", p.stdout, re.M)) == 12


def test_names_and_abi():
    assert _native.canonical_precision("fp32-ieee") == "fp32-ieee"
    assert _native.PRECISIONS["fp32-ieee"] == _native.GZ_PRECISION_FP32 == 4
    assert _native.GZ_PRECISION_FP32 not in (_native.GZ_PRECISION_BF16, _native.GZ_PRECISION_SPLIT)
    with open(os.path.join(ROOT, "include", "gzero_nn.h")) as f:
        header = f.read()
    m = re.search(r"^#define\s+GZ_PRECISION_FP32\s+(\d+)\s*$", header, re.M)
    assert m and int(m.group(1)) == _native.GZ_PRECISION_FP32
    # the older names keep their meaning
    assert _native.canonical_precision("bf16") == "bf16"
    assert _native.canonical_precision("bf16x3") == _native.canonical_precision("split") == "bf16x3"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert _native.canonical_precision("fp32") == "bf16x3"
    assert any(issubclass(x.category, DeprecationWarning) for x in w)
    assert _native.PRECISIONS["fp32"] == _native.GZ_PRECISION_SPLIT
    with pytest.raises(ValueError, match="fp32-ieee"):
        _native.canonical_precision("fp16")


@pytest.mark.parametrize("hw,ok", [((19, 19), True), ((13, 13), True), ((21, 21), False)])
def test_geometry_check(hw, ok):
    """gz_net_create in fp32-ieee mode accepts the reference's hex19 net (19 x 19, F = 80, SE,
    concat-all-layers) -- past the geometry check it needs a device, which this host may lack -- and
    refuses 21 x 21 with the geometry message."""
    with open(os.path.join(ROOT, "tests", "golden", "keras_descs.json")) as f:
        base = json.load(f)["hex19/models/h2_477.json"]["desc"]
    desc = NetDesc(**dict(base, input_columns=hw[0], input_rows=hw[1]))
    lib = _native.nn_lib()
    cdesc = _native.make_net_desc(desc, _native.PRECISIONS["fp32-ieee"])
    assert cdesc.precision == 4
    h = lib.gz_net_create(ctypes.byref(cdesc), 0)
    err = "" if h else lib.gz_nn_last_error().decode()
    if h:
        lib.gz_net_destroy(h)
    if ok:
        assert "unsupported network geometry" not in err and "unknown precision" not in err, err
    else:
        assert not h and "unsupported network geometry F=80 H=21 W=21" in err, err
