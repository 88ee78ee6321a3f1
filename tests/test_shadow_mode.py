"""The shadow check (include/gzero_nn.h gz_net_shadow_*, gz_nn_compare_outputs) without a GPU: the
header declares it, the library exports it, _native.GzShadowStats mirrors the struct field by field,
and the refusals of a net created with GZ_NN_SHADOW in the environment -- a malformed value, the
net's own mode, a geometry the shadow's mode refuses -- come before any device call, as
tests/test_v2_f256.py's do.  With the variable unset gz_net_create answers as before."""
import ctypes
import os
import re

import pytest

from galvanise_zero_amd import _native
from galvanise_zero_amd.nn.desc import NetDesc
from test_abi import declared, exported
from test_v2_f256 import REFUSALS, V2, _create_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["gz_shadow_stats_sizeof", "gz_net_shadow_enable", "gz_net_shadow_disable", "gz_net_shadow_stats",
             "gz_nn_compare_outputs"]
CTYPES = {"long": ctypes.c_long, "double": ctypes.c_double}

SMALL = NetDesc(5, 8, 8, 128, 2, [155, 155])
BIG = NetDesc(5, 19, 19, 256, 2, [362, 362], se_units=85, **V2)


def _header_struct():
    """[(name, C type)] of gz_shadow_stats as include/gzero_nn.h declares it."""
    text = open(os.path.join(ROOT, "include", "gzero_nn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef struct gz_shadow_stats \{(.*?)\} gz_shadow_stats;", text, flags=re.S)
    assert m, "gz_shadow_stats not declared"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_header_declares_the_api():
    names = declared("gzero_nn.h")
    for f in FUNCTIONS:
        assert f in names, f
    assert len(_header_struct()) == 16


def test_library_exports_the_api():
    syms = exported(_native.lib_path("libgz_nn.so"))
    for f in FUNCTIONS:
        assert f in syms, f


def test_struct_matches_header():
    fields = _header_struct()
    assert [n for n, _ in fields] == [n for n, _ in _native.GzShadowStats._fields_]
    for (name, ctype), (_, pytype) in zip(fields, _native.GzShadowStats._fields_):
        assert CTYPES[ctype] is pytype, name
    assert ctypes.sizeof(_native.GzShadowStats) == sum(ctypes.sizeof(CTYPES[c]) for _, c in fields)
    assert _native.nn_lib().gz_shadow_stats_sizeof() == ctypes.sizeof(_native.GzShadowStats)


def test_stats_dict_has_the_means():
    st = _native.GzShadowStats(policy_elems=4, sum_abs_dp=2.0, policy_rows=2, sum_row_kl=1.0, value_elems=0, sum_abs_dv=0.0)
    d = st.as_dict()
    assert (d["mean_abs_dp"], d["mean_row_kl"], d["mean_abs_dv"]) == (0.5, 0.5, 0.0)
    assert set(n for n, _ in st._fields_) <= set(d)


@pytest.mark.parametrize("spec", ["abc", "4:0", "4:64:0", "4:", "4:64:256:1", "-1", "4x"])
def test_malformed_spec(spec, monkeypatch):
    monkeypatch.setenv("GZ_NN_SHADOW", spec)
    created, err = _create_error(SMALL, "bf16x3")
    assert not created and err.startswith("GZ_NN_SHADOW:"), err
    assert spec in err


def test_own_mode_refused(monkeypatch):
    monkeypatch.setenv("GZ_NN_SHADOW", "3")
    created, err = _create_error(SMALL, "bf16x3")
    assert not created and err.startswith("shadow:") and "the net's own mode" in err, err


def test_shadow_geometry_refused(monkeypatch):
    """bf16x3-layered takes 19 x 19 with 256 filters, bf16x3 as its shadow does not: the shadow's
    gz_net_create message follows the prefix."""
    monkeypatch.setenv("GZ_NN_SHADOW", "3")
    created, err = _create_error(BIG, "bf16x3-layered")
    assert not created and err.startswith("shadow: unsupported network geometry F=256 H=19 W=19"), err
    monkeypatch.setenv("GZ_NN_SHADOW", "9:4:4")
    created, err = _create_error(SMALL, "bf16x3")
    assert not created and err == "shadow: unknown precision", err


@pytest.mark.parametrize("spec", ["4", "4:1", "4:64:256", "7:3:16", "1"])
def test_valid_spec_accepted(spec, monkeypatch):
    """Past the refusals only the device is left (test_v2_f256.test_geometry_accepted)."""
    monkeypatch.setenv("GZ_NN_SHADOW", spec)
    created, err = _create_error(SMALL, "bf16x3")
    print("%s: %s" % (spec, "created" if created else err))
    assert "GZ_NN_SHADOW" not in err and "shadow" not in err, err
    for text in REFUSALS:
        assert text not in err, err


def test_existing_refusals_unchanged(monkeypatch):
    monkeypatch.delenv("GZ_NN_SHADOW", raising=False)
    created, err = _create_error(BIG, "bf16x3")
    assert not created and err.startswith("unsupported network geometry F=256 H=19 W=19 (split precision) (v2)"), err
    created, err = _create_error(NetDesc(5, 8, 8, 256, 2, [155, 155], se_units=129, **V2), "bf16")
    assert not created and err == "squeeze-excite units must be 0..128 on a v2 net", err
    created, err = _create_error(NetDesc(5, 13, 13, 256, 14, [170, 171], resnet_v2=True), "bf16x3")
    assert not created and err.startswith("network needs %d B of LDS per workgroup (160 KB max)" % (136704 + 2048 * 14)), err
    # the net's own refusal comes before the shadow's, whatever the variable says
    monkeypatch.setenv("GZ_NN_SHADOW", "abc")
    created, err = _create_error(BIG, "bf16x3")
    assert not created and err.startswith("unsupported network geometry"), err
