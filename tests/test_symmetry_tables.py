"""Board symmetries without a GPU: the descriptors (galvanise_zero_amd/defs/symmetries.py) against
the reference's own (tests/golden/symmetries.json, written by tests/golden/make_symmetries_golden.py),
the tables galvanise_zero_amd/util/symmetry.py builds from them -- group properties, and that they
commute with the native state machines' rules and with the planes --, gz_symmetry_create's refusals
(validation precedes any device call) and csrc/nn/symmetry.h's validation and kernel index
arithmetic on the CPU under AddressSanitizer / UBSan (a stand-alone program)."""
import json
import os
import random
import subprocess

import attr
import numpy as np
import pytest

from galvanise_zero_amd import _native
from galvanise_zero_amd.cppinterface import create_c_transformer
from galvanise_zero_amd.defs import symmetries
from galvanise_zero_amd.util import symmetry
from test_fp32_mode import _run_sanitised

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "symmetries.json")) as _f:
    REF = json.load(_f)
GAMES = ["breakthrough", "breakthroughSmall", "reversi", "hexLG13", "amazons_10x10"]
COUNTS = {"breakthrough": 2, "breakthroughSmall": 2, "bt_7": 2, "reversi": 8, "hexLG13": 2, "amazons_10x10": 8}

_tables = {}


def tables(game):
    if game not in _tables:
        _tables[game] = symmetry.tables_for_game(game)
    return _tables[game]


@pytest.mark.parametrize("game", sorted(REF))
def test_descriptors_match_reference(game):
    assert attr.asdict(getattr(symmetries.GameSymmetries(), game)()) == REF[game]


def test_descriptor_games():
    assert sorted(REF) == sorted(COUNTS)
    assert sorted(n for n in dir(symmetries.GameSymmetries) if not n.startswith("_")) == sorted(COUNTS)


@pytest.mark.parametrize("game", sorted(COUNTS))
def test_group_properties(game):
    T, sm, t = tables(game)
    S = T.count
    assert S == COUNTS[game] and T.elements[0] == (False, 0)
    assert T.base_perm.shape == (S, sm.num_bases)
    assert T.plane_src.shape == (S, t.num_channels * t.channel_size)
    assert T.policy_sizes == list(t.policy_dist_count)
    for s in range(S):
        for tab in [T.base_perm[s], T.plane_src[s]] + [m[s] for m in T.move_src]:
            assert np.array_equal(np.sort(tab), np.arange(len(tab)))
    for tab in [T.base_perm[0], T.plane_src[0]] + [m[0] for m in T.move_src]:
        assert np.array_equal(tab, np.arange(len(tab)))
    assert len({T.base_perm[s].tobytes() for s in range(S)}) == S      # S distinct elements
    index = {T.base_perm[s].tobytes(): s for s in range(S)}
    for a in range(S):
        has_inverse = False
        for b in range(S):
            # a, then b: base x -> base_perm[a][x] -> base_perm[b][base_perm[a][x]]
            key = T.base_perm[b][T.base_perm[a]].tobytes()
            assert key in index, "not closed: %r then %r" % (T.elements[a], T.elements[b])
            c = index[key]
            has_inverse |= c == 0
            for m in T.move_src:
                assert np.array_equal(m[c], m[b][m[a]])
            # X_c = (X_a)_b:  X_c[i] = X_a[plane_src[b][i]] = X[plane_src[a][plane_src[b][i]]]
            assert np.array_equal(T.plane_src[c], T.plane_src[a][T.plane_src[b]])
        assert has_inverse


def _playout(sm, seed, max_plies=150):
    """[(state words, previous state words or None, legals per role, joint move, successor words)]"""
    rng = random.Random(seed)
    s, prev, out = sm.get_initial_state().copy(), None, []
    for _ in range(max_plies):
        sm.update_bases(s)
        if sm.is_terminal():
            break
        legals = [sm.get_legal_state(r) for r in range(sm.role_count)]
        jm = [rng.choice(l) for l in legals]
        nxt = sm.next_state(jm).copy()
        out.append((s, prev, legals, jm, nxt))
        s, prev = nxt, s
    return out, s


def _status(sm, words):
    sm.update_bases(words)
    term = sm.is_terminal()
    return term, [sm.get_goal_value(r) for r in range(sm.role_count)] if term else None


@pytest.mark.parametrize("game", GAMES)
def test_rules_and_planes_commute(game):
    """3 seeded random playouts, to the end or 150 plies; at every ply and for every element: the
    mapped state's legal set per role is move_src of the original's, its successor under the mapped
    joint move is the mapped successor, terminal flags and goals agree, and to_channels of the mapped
    state (with the mapped previous state) is X[plane_src]."""
    T, sm, t = tables(game)
    ct = create_c_transformer(t)
    roles = range(sm.role_count)
    for seed in (1, 2, 3):
        plies, last = _playout(sm, 1000 * seed + len(game))
        assert len(plies) > 5
        for s, prev, legals, jm, nxt in plies:
            bits, nbits = sm.bits(s), sm.bits(nxt)
            X = ct.to_channels(s, [prev] if prev is not None else [])
            for e in range(T.count):
                ms = sm.from_bits(T.map_state_bits(e, bits))
                sm.update_bases(ms)
                assert not sm.is_terminal()
                got = [sorted(sm.get_legal_state(r)) for r in roles]
                assert got == [sorted(int(T.move_src[r][e][m]) for m in legals[r]) for r in roles], (game, T.elements[e])
                mapped_next = sm.next_state([int(T.move_src[r][e][jm[r]]) for r in roles])
                assert sm.bits(mapped_next) == T.map_state_bits(e, nbits), (game, T.elements[e])
                mprev = [sm.from_bits(T.map_state_bits(e, sm.bits(prev)))] if prev is not None else []
                assert np.array_equal(ct.to_channels(ms, mprev), X[T.plane_src[e]]), (game, T.elements[e])
        want = _status(sm, last)
        for e in range(T.count):
            assert _status(sm, sm.from_bits(T.map_state_bits(e, sm.bits(last)))) == want, (game, T.elements[e])


def test_builder_refusals():
    T, sm, t = tables("reversi")
    good = symmetries.GameSymmetries().reversi()
    with pytest.raises(symmetry.SymmetryError, match="neither applies nor skips 'control'"):
        symmetry.build_tables(sm, t, attr.evolve(good, skip_bases=[]))
    with pytest.raises(symmetry.SymmetryError, match="neither applies nor skips 'noop'"):
        symmetry.build_tables(sm, t, attr.evolve(good, skip_actions=[]))
    with pytest.raises(symmetry.SymmetryError, match="has no term 7"):
        symmetry.build_tables(sm, t, attr.evolve(good, apply_bases=[symmetries.ApplySymmetry("cell", 1, 7)]))
    with pytest.raises(symmetry.SymmetryError, match="not coordinates"):
        symmetry.build_tables(sm, t, attr.evolve(good, apply_bases=[symmetries.ApplySymmetry("cell", 1, 3)]))
    with pytest.raises(symmetry.SymmetryError, match="not both"):
        symmetry.build_tables(sm, t, attr.evolve(good, do_rotations_180=True))

    class Oblong(object):          # quarter turns are refused before anything else is read
        x_cords, y_cords = list("12345678"), list("1234567")
    with pytest.raises(symmetry.SymmetryError, match="square"):
        symmetry.build_tables(sm, Oblong(), good)
    with pytest.raises(symmetry.SymmetryError, match="no symmetries described"):
        symmetry.tables_for_game("connect4")
    # the reflection alone is a subgroup: two elements, built from the same descriptor
    assert symmetry.build_tables(sm, t, attr.evolve(good, do_rotations_90=False)).count == 2


def test_create_refuses_bad_tables():
    """gz_symmetry_create on a host without a GPU: every refusal, and valid tables accepted (the
    device is first touched by a forward)."""
    T, _, _ = tables("reversi")
    ok = _native.HipSymmetry(T.plane_src, T.move_src)
    assert ok.lib.gz_symmetry_count(ok.handle) == 8 == ok.count
    ok.close()
    plane = T.plane_src.copy()
    plane[3, 5] = plane[3, 6]
    with pytest.raises(RuntimeError, match=r"failed: symmetry: plane table of element 3 is not a permutation"):
        _native.HipSymmetry(plane, T.move_src)
    plane = T.plane_src.copy()
    plane[7, 0] = plane.shape[1]
    with pytest.raises(RuntimeError, match=r"failed: symmetry: plane table of element 7 is not a permutation"):
        _native.HipSymmetry(plane, T.move_src)
    moves = [m.copy() for m in T.move_src]
    moves[1][2, 9] = -1
    with pytest.raises(RuntimeError, match=r"failed: symmetry: move table of element 2, role 1 is not a permutation"):
        _native.HipSymmetry(T.plane_src, moves)
    nine = np.tile(np.arange(10, dtype=np.int32), (9, 1))
    with pytest.raises(RuntimeError, match=r"failed: symmetry: count 9 outside 1\.\.8"):
        _native.HipSymmetry(nine, [nine])
    with pytest.raises(RuntimeError, match=r"failed: symmetry: count 0 outside 1\.\.8"):
        _native.HipSymmetry(nine[:0], [nine[:0]])


def test_entry_points_declared_and_exported():
    names = ["gz_symmetry_create", "gz_symmetry_destroy", "gz_symmetry_count", "gz_net_forward_sym",
             "gz_net_forward_sym_device"]
    header = open(os.path.join(ROOT, "include", "gzero_nn.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.lib_path("libgz_nn.so")], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in names:
        assert n + "(" in header and n in exported, n


def test_host_check_sanitised(tmp_path):
    """tests/symmetry_host_check.cpp: csrc/nn/symmetry.h's validation (every refusal) and both
    kernels' index arithmetic over small tables, S = 1 .. 8, on exactly-sized heap buffers, against
    a restatement of the ensemble -- built with -fsanitize=address,undefined."""
    p = _run_sanitised(tmp_path, "symmetry_host_check")
    assert p.returncode == 0, p.stdout[-4000:]
    assert "symmetry host check passed" in p.stdout
    assert p.stdout.count("chunk ok") == 24 and p.stdout.count("refusal ok") >= 30
