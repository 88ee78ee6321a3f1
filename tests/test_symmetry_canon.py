"""The canonical orientation without a GPU: the definition in csrc/nn/symmetry.h (a stand-alone program
under AddressSanitizer / UBSan, against a brute-force restatement) held to its numpy statement in
galvanise_zero_amd/util/symmetry.py, that statement against a pure-Python loop, the three properties
the header states on reversi's (S = 8) and breakthrough's (S = 2) tables, the refusals that need no
device, and the ABI."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from galvanise_zero_amd import _native
from galvanise_zero_amd.util import evalcache, symmetry
from test_fp32_mode import _run_sanitised

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ES = [75, 320, 1300]
SS = [1, 2, 3, 8]
SALTS = [0, 0xFFFFFFFF]
KINDS = ["lcg", "one", "negzero", "nan", "period15"]
_M32 = 0xFFFFFFFF


def make_row(kind, E):
    """tests/symmetry_canon_host_check.cpp make_row, as bit patterns."""
    bits = np.zeros(E, dtype=np.uint32)
    if kind == "one":
        bits[:] = 0x3F800000
    elif kind == "negzero":
        bits[E // 2] = 0x80000000
    elif kind == "nan":
        bits[E - 1] = 0x7FC00123
    elif kind == "period15":
        bits[np.arange(E) % 15 < 7] = 0x3F800000
    elif kind == "lcg":
        x = (12345 + E) & _M32
        for i in range(E):
            x = (x * 1664525 + 1013904223) & _M32
            bits[i] = 0x3F800000 if (x >> 16) & 1 else 0
    return bits.view(np.float32)


def rotations(E, S):
    return np.array([[(i + 3 * s) % E for i in range(E)] for s in range(S)], dtype=np.int32)


def test_host_check_sanitised_agrees_with_numpy(tmp_path):
    """tests/symmetry_canon_host_check.cpp, built with -fsanitize=address,undefined and run as a plain
    executable: the header's serial definition equals the brute force (every image materialised, tagged
    with gzcache::row_tag, the first minimum taken) for E in {75, 320, 1300}, S in {1, 2, 3, 8}, both
    salts, and rows equal to one of their images; every g and tag it prints is recomputed with numpy."""
    p = _run_sanitised(tmp_path, "symmetry_canon_host_check")
    assert p.returncode == 0, p.stdout[-4000:]
    assert "symmetry canon host check passed" in p.stdout
    lines = re.findall(r"^canon E=(\d+) S=(\d+) salt=(\d+) kind=(\w+) g=(\d+) tag=(\d+)$", p.stdout, re.M)
    assert len(lines) == len(ES) * len(SS) * len(SALTS) * len(KINDS)
    seen = set()
    for E, S, salt, kind, g, tag in lines:
        E, S, salt = int(E), int(S), int(salt)
        seen.add((E, S, salt, kind))
        got_g, got_tag = symmetry.canonical_elements(make_row(kind, E)[None, :], rotations(E, S), salt)
        assert (int(got_g[0]), int(got_tag[0])) == (int(g), int(tag)), (E, S, salt, kind)
    assert seen == {(E, S, s, k) for E in ES for S in SS for s in SALTS for k in KINDS}


def _py_fmix32(x):
    x ^= x >> 16
    x = (x * 0x85ebca6b) & _M32
    x ^= x >> 13
    x = (x * 0xc2b2ae35) & _M32
    return x ^ (x >> 16)


def _py_mix32b(x):
    x ^= x >> 15
    x = (x * 0x2c1b3c6d) & _M32
    x ^= x >> 12
    x = (x * 0x297a2d39) & _M32
    return x ^ (x >> 15)


def py_canonical(row_bits, plane_src, salt):
    """The definition as a loop over Python ints."""
    best = None
    for s, table in enumerate(plane_src):
        h1 = h2 = 0
        for i, j in enumerate(table):
            b = int(row_bits[j])
            h1 = (h1 + _py_fmix32((b + 0x9E3779B9 * (i + 1)) & _M32)) & _M32
            h2 = (h2 + _py_mix32b((b + 0x85EBCA77 * (i + 1)) & _M32)) & _M32
        tag = (h2 << 32) | h1
        key = evalcache.mix64(tag ^ (salt & _M32))
        if best is None or key < best[0]:
            best = (key, s, tag)
    return best[1], best[2]


def test_numpy_equals_a_python_loop():
    for E in ES:
        rows = np.array([make_row(k, E) for k in KINDS] + list(np.random.default_rng(E).integers(0, 2, (6, E)).astype(np.float32)))
        for S in SS:
            tables = np.array([np.random.default_rng(100 * S + s).permutation(E) for s in range(S)], dtype=np.int32)
            for salt in SALTS + [12345]:
                g, tags = symmetry.canonical_elements(rows, tables, salt)
                assert g.dtype == np.int32 and tags.dtype == np.uint64
                for r in range(rows.shape[0]):
                    assert (int(g[r]), int(tags[r])) == py_canonical(rows[r].view(np.uint32), tables, salt), (E, S, salt, r)
                x = symmetry.canonical_planes(rows, tables, salt)
                assert np.array_equal(x.view(np.uint32), np.take_along_axis(rows, tables[g], axis=1).view(np.uint32))
                # the tag is the cache's tag of the canonical image
                assert np.array_equal(tags, evalcache.tags(x))


def synthetic_forward(policy_sizes, V):
    """A row-wise "forward": every output a function of that row's words alone."""
    def forward(x):
        flat = np.ascontiguousarray(x, dtype=np.float32).reshape(x.shape[0], -1)
        E = flat.shape[1]
        w = np.float32(1) + np.arange(E, dtype=np.float32) / np.float32(E)
        outs = [flat[:, (5 * np.arange(p) + r) % E] * w[(7 * np.arange(p) + 3) % E] + (flat * w).sum(axis=1, dtype=np.float32)[:, None]
                for r, p in enumerate(policy_sizes)]
        return outs + [np.float32(2) * flat[:, np.arange(V) % E] + (flat * w[::-1]).sum(axis=1, dtype=np.float32)[:, None]]
    return forward


def images_of(X, T):
    flat = X.reshape(X.shape[0], -1)
    return [np.ascontiguousarray(flat[:, p]) for p in np.asarray(T.plane_src)]


@pytest.mark.parametrize("game", ["reversi", "breakthrough"])
def test_properties_on_a_games_tables(game):
    """200 random 0/1 rows whose S images are all distinct (asserted): every image of a row has the
    row's canonical planes, and the canonical forward of the image read through move_src[t] is the
    row's, exactly; a row OR-ed with its reflection takes the lowest s among its equal images; another
    salt changes some representative."""
    T, _, _ = symmetry.tables_for_game(game)
    S, E = T.plane_src.shape
    assert S == (8 if game == "reversi" else 2)
    X = np.random.default_rng(len(game)).integers(0, 2, (200, E)).astype(np.float32)
    imgs = images_of(X, T)
    for r in range(X.shape[0]):
        assert len({im[r].tobytes() for im in imgs}) == S, r             # a condition of what follows
    forward = synthetic_forward(T.policy_sizes, 3)
    for salt in SALTS + [7]:
        canon = symmetry.canonical_planes(X, T, salt)
        out = symmetry.canonical_forward(forward, X, T, salt)
        g, _ = symmetry.canonical_elements(X, T, salt)
        if S == 8:
            assert len(set(g.tolist())) == S                             # every element is some row's
        for t in range(S):
            assert np.array_equal(symmetry.canonical_planes(imgs[t], T, salt), canon), (salt, t)
            out_t = symmetry.canonical_forward(forward, imgs[t], T, salt)
            for r in range(len(T.move_src)):
                assert np.array_equal(out[r].view(np.uint32), out_t[r][:, T.move_src[r][t]].view(np.uint32)), (salt, t, r)
            assert np.array_equal(out[-1].view(np.uint32), out_t[-1].view(np.uint32))
    g0, _ = symmetry.canonical_elements(X, T, 0)
    g1, _ = symmetry.canonical_elements(X, T, 0xFFFFFFFF)
    assert (g0 != g1).any()

    # positions that are their own image: the lowest s among equal images
    refl = T.elements.index((True, 0))
    Y = np.maximum(X, imgs[refl])
    yimgs = images_of(Y, T)
    assert np.array_equal(yimgs[refl], yimgs[0])
    for salt in SALTS:
        g, tags = symmetry.canonical_elements(Y, T, salt)
        canon = symmetry.canonical_planes(Y, T, salt)
        for r in range(Y.shape[0]):
            equal = [s for s in range(S) if yimgs[s][r].tobytes() == yimgs[g[r]][r].tobytes()]
            assert len(equal) >= 2 and g[r] == equal[0], (salt, r, g[r], equal)
            assert canon[r].tobytes() == yimgs[g[r]][r].tobytes()
        assert np.array_equal(tags, evalcache.tags(canon))


def test_refusals_without_a_device():
    from galvanise_zero_amd.nn.network import HipModel
    from galvanise_zero_amd.runner import SelfPlayRunner
    lib = _native.runner_lib()
    T, _, _ = symmetry.tables_for_game("breakthrough")
    sym = _native.HipSymmetry(T.plane_src, T.move_src)
    x = np.zeros((1, T.plane_src.shape[1]), dtype=np.float32)
    pol = (_native._FP * 2)()
    assert lib.gz_net_forward_sym_canon(None, sym.handle, 0, None, _native._fptr(x), 1, pol, _native._fptr(x)) != 0
    assert lib.gz_nn_last_error().decode() == "symmetry: null argument"
    assert lib.gz_net_forward_sym_canon_device(None, sym.handle, 0, None, None, x.ctypes.data, 1, None, None) != 0
    assert lib.gz_nn_last_error().decode() == "symmetry: null argument"
    out = np.zeros(1, dtype=np.int32)
    assert lib.gz_symmetry_canon(None, 0, 0, x.ctypes.data, 1, out.ctypes.data_as(_native._IP), None) != 0
    assert lib.gz_nn_last_error().decode() == "symmetry: null argument"
    assert lib.gz_symmetry_canon(sym.handle, 0, 0, x.ctypes.data, 1, None, None) != 0
    assert lib.gz_nn_last_error().decode() == "symmetry: null argument"
    assert lib.gz_runner_set_canonical(None, sym.handle, 0, None) != 0
    assert lib.gz_runner_last_error().decode() == "runner: null argument"

    net = object.__new__(_native.HipNet)          # the refusals precede every use of the net
    with pytest.raises(ValueError, match="canonical= together with pick="):
        net.forward(x, symmetry=sym, pick=1, canonical=1)
    with pytest.raises(ValueError, match="cache= together with symmetry=: the two do not compose"):
        net.forward(x, symmetry=sym, cache=object())
    with pytest.raises(ValueError, match="cache= together with symmetry=: the two do not compose"):
        net.forward(x, symmetry=sym, pick=1, cache=object())
    with pytest.raises(ValueError, match="canonical=1 needs symmetry="):
        net.forward(x, canonical=1)
    sym.close()

    with pytest.raises(ValueError, match='symmetry_mode \'both\': "average" or "pick"'):
        HipModel(None, None, symmetries=T, symmetry_mode="both")
    with pytest.raises(ValueError, match='"canonical" needs symmetries='):
        HipModel(None, None, symmetry_mode="canonical")
    for mode in ("average", "pick"):
        with pytest.raises(ValueError, match="cache_entries= together with symmetries=: the two do not compose"):
            HipModel(None, None, symmetries=T, symmetry_mode=mode, cache_entries=64)
    with pytest.raises(ValueError, match='symmetry_mode \'average\': "pick" or "canonical"'):
        SelfPlayRunner(None, None, None, None, symmetry_mode="average")
    with pytest.raises(ValueError, match='"canonical" needs symmetry='):
        SelfPlayRunner(None, None, None, None, symmetry_mode="canonical")


def test_entry_points_declared_and_exported():
    names = ["gz_net_forward_sym_canon", "gz_net_forward_sym_canon_device", "gz_symmetry_canon", "gz_runner_set_canonical"]
    header = open(os.path.join(ROOT, "include", "gzero_nn.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.lib_path("libgz_nn.so")], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in names:
        assert n + "(" in header and n in exported, n
    # gz_runner_config and gz_runner_stats are ABI: the feature adds functions, not fields
    assert ctypes.sizeof(_native.GzRunnerConfig) == 56 and ctypes.sizeof(_native.GzRunnerStats) == 21 * 8
