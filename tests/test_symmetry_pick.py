"""One symmetry per row, picked from the row's own planes, without a GPU: the definition in
csrc/nn/symmetry.h (hash, pick, expand and gather index arithmetic -- a stand-alone program under
AddressSanitizer / UBSan) against its numpy statement in galvanise_zero_amd/util/symmetry.py, the
pick's uniformity over each game's own positions and two synthetic families, the salt, and the
refusals that need no device."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from galvanise_zero_amd import _native
from galvanise_zero_amd.cppinterface import create_c_transformer
from galvanise_zero_amd.util import symmetry
from test_fp32_mode import _run_sanitised

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = ["breakthrough", "breakthroughSmall", "reversi", "hexLG13", "amazons_10x10"]
ES = [1, 3, 75, 320, 5415]
SS = [1, 2, 3, 8]
SALTS = [0, 0xFFFFFFFF]
KINDS = ["zero", "one", "negzero", "nan", "lcg"]


def lcg_row(seed, E):
    """tests/symmetry_pick_host_check.cpp lcg_row: 0.0 / 1.0 from a 32-bit LCG, as bit patterns."""
    out = np.zeros(E, dtype=np.uint32)
    x = seed & 0xFFFFFFFF
    for i in range(E):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = 0x3F800000 if (x >> 16) & 1 else 0
    return out


def make_row(kind, E):
    bits = np.zeros(E, dtype=np.uint32)
    if kind == "one":
        bits[:] = 0x3F800000
    elif kind == "negzero":
        bits[0] = 0x80000000
    elif kind == "nan":
        bits[E - 1] = 0x7FC00123
    elif kind == "lcg":
        bits = lcg_row(12345 + E, E)
    return bits.view(np.float32)


class FlowTables(object):
    """The rotations of symmetry_pick_host_check.cpp check_flow."""

    def __init__(self, E, S, P):
        self.plane_src = np.array([[(i + 3 * s) % E for i in range(E)] for s in range(S)], dtype=np.int32)
        self.move_src = [np.array([[m if s == 0 else (m + 2 * s + r) % p for m in range(p)] for s in range(S)], dtype=np.int32)
                         for r, p in enumerate(P)]


def flow_digest(E, S, n, salt):
    P, V = [7, 12], 3
    X = np.array([lcg_row(1000 + 31 * r + E, E) for r in range(n)], dtype=np.uint32).view(np.float32)

    def forward(x):
        outs = [x[:, (5 * np.arange(p) + r) % E] + np.arange(p, dtype=np.float32) for r, p in enumerate(P)]
        return outs + [np.float32(2) * x[:, np.arange(V) % E] + np.arange(V, dtype=np.float32)]

    d = np.uint32(0)
    with np.errstate(over="ignore"):
        for a in symmetry.pick_forward(forward, X, FlowTables(E, S, P), salt):
            bits = np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)
            k = np.uint32(0x9E3779B9) * np.arange(1, bits.size + 1, dtype=np.uint32)
            d = d + symmetry._fmix32(bits + k).sum(dtype=np.uint32)
    return int(d)


def test_host_check_sanitised_agrees_with_numpy(tmp_path):
    """tests/symmetry_pick_host_check.cpp, built with -fsanitize=address,undefined: every hash, pick
    and expand / gather digest it prints is recomputed here with numpy and must agree exactly --
    E in {1, 3, 75, 320, 5415}; all-zero, all-one, -0.0 against 0.0, a NaN pattern and a random 0/1
    row; S in {1, 2, 3, 8}; salts 0 and 0xFFFFFFFF."""
    p = _run_sanitised(tmp_path, "symmetry_pick_host_check")
    assert p.returncode == 0, p.stdout[-4000:]
    assert "symmetry pick host check passed" in p.stdout
    picks = re.findall(r"^pick E=(\d+) kind=(\w+) S=(\d+) salt=(\d+) h=(\d+) g=(\d+)$", p.stdout, re.M)
    assert len(picks) == len(ES) * len(KINDS) * len(SS) * len(SALTS)
    seen = set()
    for E, kind, S, salt, h, g in picks:
        E, S, salt = int(E), int(S), int(salt)
        seen.add((E, kind, S, salt))
        row = make_row(kind, E)[None, :]
        assert int(symmetry.pick_hashes(row)[0]) == int(h), (E, kind)
        assert int(symmetry.pick_elements(row, S, salt)[0]) == int(g), (E, kind, S, salt)
    assert seen == {(E, k, S, s) for E in ES for k in KINDS for S in SS for s in SALTS}
    flows = re.findall(r"^flow E=(\d+) S=(\d+) n=(\d+) salt=(\d+) digest=(\d+)$", p.stdout, re.M)
    assert len(flows) == 2 * len(ES) * len(SS) + 1
    for E, S, n, salt, d in flows:
        assert flow_digest(int(E), int(S), int(n), int(salt)) == int(d), (E, S, n, salt)


def test_hash_reads_bit_patterns():
    """-0.0 is not 0.0 to the hash (planes never hold -0.0; this pins the reading), and a NaN is its bits."""
    for E in ES:
        z, nz = make_row("zero", E)[None, :], make_row("negzero", E)[None, :]
        assert np.array_equal(z, nz)                      # equal as floats
        assert symmetry.pick_hashes(z)[0] != symmetry.pick_hashes(nz)[0]
        assert symmetry.pick_hashes(make_row("nan", E)[None, :])[0] != symmetry.pick_hashes(z)[0]
    # S = 1: always the identity
    X = np.random.default_rng(3).integers(0, 2, (100, 75)).astype(np.float32)
    assert not symmetry.pick_elements(X, 1, 99).any()


def assert_uniform(X, S, what):
    for salt in (0, 12345):
        g = symmetry.pick_elements(X, S, salt)
        share = np.bincount(g, minlength=S) * float(S) / len(g)
        print("%s: %d rows, S = %d, salt %d: share x S %s" % (what, len(g), S, salt, np.round(share, 3)))
        assert share.min() >= 0.8 and share.max() <= 1.2, (what, S, salt, share)


def game_positions(game, count=4000):
    """Planes of `count` distinct positions from seeded random playouts (a position met twice -- every
    playout starts from the same one -- is one sample of the hash, so it is taken once)."""
    T, sm, t = symmetry.tables_for_game(game)
    ct = create_c_transformer(t)
    rng = random.Random(20251021 + len(game))
    seen, planes = set(), []
    while len(planes) < count:
        s, prev = sm.get_initial_state().copy(), None
        for _ in range(400):
            sm.update_bases(s)
            if sm.is_terminal():
                break
            x = ct.to_channels(s, [prev] if prev is not None else [])
            key = x.tobytes()
            if key not in seen:
                seen.add(key)
                planes.append(x)
            jm = [rng.choice(sm.get_legal_state(r)) for r in range(sm.role_count)]
            s, prev = sm.next_state(jm).copy(), s
    return T, np.array(planes[:count], dtype=np.float32)


@pytest.mark.parametrize("game", GAMES)
def test_uniform_over_a_games_positions(game):
    """4,000 distinct positions of seeded random playouts, the game's own tables: every element's share
    times S within [0.8, 1.2] for salts 0 and 12345 (binomial sigma at S = 8: 0.042)."""
    T, X = game_positions(game)
    assert X.shape[0] == 4000 and not np.signbit(X[X == 0]).any()      # planes never hold -0.0
    assert_uniform(X, T.count, game)


@pytest.mark.parametrize("E", [320, 1200, 5415])
def test_uniform_over_synthetic_boards(E):
    """4,000 random 0/1 boards, and 4,000 boards each differing from one board in two cells."""
    rng = np.random.default_rng(E)
    rand = rng.integers(0, 2, (4000, E)).astype(np.float32)
    near = np.tile(rng.integers(0, 2, E).astype(np.float32), (4000, 1))
    cells = set()
    while len(cells) < 4000:
        a, b = sorted(int(v) for v in rng.integers(0, E, 2))
        if a != b:
            cells.add((a, b))
    for r, (a, b) in enumerate(sorted(cells)):
        near[r, a] = 1 - near[r, a]
        near[r, b] = 1 - near[r, b]
    for S in (2, 3, 8):
        assert_uniform(rand, S, "random E=%d" % E)
        assert_uniform(near, S, "two-cell neighbours E=%d" % E)


def test_salt():
    """Among 64 distinct positions another salt changes at least one pick; the same salt reproduces all."""
    T, X = game_positions("reversi", 64)
    assert len({x.tobytes() for x in X}) == 64
    a = symmetry.pick_elements(X, T.count, 7)
    assert np.array_equal(a, symmetry.pick_elements(X.copy(), T.count, 7))
    assert np.array_equal(a[::-1], symmetry.pick_elements(X[::-1], T.count, 7))     # a row's pick is its own
    assert (a != symmetry.pick_elements(X, T.count, 8)).any()
    assert (a != symmetry.pick_elements(X, T.count, 7 + 2 ** 31)).any()
    assert np.array_equal(a, symmetry.pick_elements(X, T.count, 7 + 2 ** 32))       # salts are 32 bits


def test_refusals_without_a_device():
    lib = _native.runner_lib()
    T, _, _ = symmetry.tables_for_game("breakthrough")
    sym = _native.HipSymmetry(T.plane_src, T.move_src)
    x = np.zeros((1, T.plane_src.shape[1]), dtype=np.float32)
    pol = (_native._FP * 2)()
    assert lib.gz_net_forward_sym_pick(None, sym.handle, 0, _native._fptr(x), 1, pol, _native._fptr(x)) != 0
    assert lib.gz_nn_last_error().decode() == "symmetry: null argument"
    assert lib.gz_net_forward_sym_pick_device(None, sym.handle, 0, None, x.ctypes.data, 1, None, None) != 0
    assert lib.gz_nn_last_error().decode() == "symmetry: null argument"
    out = np.zeros(1, dtype=np.int32)
    assert lib.gz_symmetry_picks(None, 0, 0, x.ctypes.data, 1, out.ctypes.data_as(_native._IP)) != 0
    assert lib.gz_nn_last_error().decode() == "symmetry: null argument"
    assert lib.gz_runner_set_symmetry(None, sym.handle, 0) != 0
    assert lib.gz_runner_last_error().decode() == "runner: null argument"
    assert lib.gz_runner_sym_pick_rows(None) == 0
    sym.close()
    from galvanise_zero_amd.nn.network import HipModel
    with pytest.raises(ValueError, match='symmetry_mode \'both\': "average" or "pick"'):
        HipModel(None, None, symmetries=T, symmetry_mode="both")
    with pytest.raises(ValueError, match='"pick" needs symmetries='):
        HipModel(None, None, symmetry_mode="pick")


def test_entry_points_declared_and_exported():
    names = ["gz_net_forward_sym_pick", "gz_net_forward_sym_pick_device", "gz_symmetry_picks", "gz_runner_set_symmetry",
             "gz_runner_sym_pick_rows"]
    header = open(os.path.join(ROOT, "include", "gzero_nn.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.lib_path("libgz_nn.so")], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in names:
        assert n + "(" in header and n in exported, n
    # gz_runner_config and gz_runner_stats are ABI: the feature adds functions, not fields
    assert ctypes.sizeof(_native.GzRunnerConfig) == 56 and ctypes.sizeof(_native.GzRunnerStats) == 21 * 8
