"""The evaluation cache without a GPU: the definition in csrc/nn/eval_cache.h (hashes, tag, slot and
the serial model of the table -- a stand-alone program under AddressSanitizer / UBSan) against its
numpy statement in galvanise_zero_amd/util/evalcache.py, the spread of slots and the distinctness of
tags over each game's own positions, and the refusals that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from galvanise_zero_amd import _native
from galvanise_zero_amd.util import evalcache
from test_fp32_mode import _run_sanitised
from test_symmetry_pick import ES, GAMES, KINDS, game_positions, lcg_row, make_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 2, 3, 64, 65536]


def script_row(spec, E):
    """tests/eval_cache_host_check.cpp build_row: lcg_row(seed) with one word changed."""
    seed, word, kind = spec.split("/")
    bits = lcg_row(int(seed), E)
    word = int(word)
    if kind == "f":
        bits[word] = 0 if bits[word] else 0x3F800000
    elif kind == "c":
        bits[word] = 0
    elif kind == "z":
        bits[word] = 0x80000000
    return bits


def test_host_check_sanitised_agrees_with_numpy(tmp_path):
    """tests/eval_cache_host_check.cpp, built with -fsanitize=address,undefined: both hashes, the tag
    and the slot for E in {1, 3, 75, 320, 5415}, five kinds of row and N in {1, 2, 3, 64, 65536}, then
    the serial model over scripted sequences -- every hit mask, table digest and insert / replaced
    count it prints is recomputed here with util/evalcache.py and must agree exactly."""
    p = _run_sanitised(tmp_path, "eval_cache_host_check")
    assert p.returncode == 0, p.stdout[-4000:]
    assert "eval cache host check passed" in p.stdout
    hashes = re.findall(r"^hash E=(\d+) kind=(\w+) h1=(\d+) h2=(\d+) tag=(\d+)$", p.stdout, re.M)
    assert {(int(E), k) for E, k, _, _, _ in hashes} == {(E, k) for E in ES for k in KINDS} and len(hashes) == len(ES) * len(KINDS)
    for E, kind, h1, h2, tag in hashes:
        row = make_row(kind, int(E))[None, :]
        assert int(evalcache.hash1(row)[0]) == int(h1), (E, kind)
        assert int(evalcache.hash2(row)[0]) == int(h2), (E, kind)
        assert int(evalcache.tags(row)[0]) == int(tag) == (int(h2) << 32 | int(h1)), (E, kind)
    slots = re.findall(r"^slot E=(\d+) kind=(\w+) N=(\d+) slot=(\d+)$", p.stdout, re.M)
    assert {(int(E), k, int(N)) for E, k, N, _ in slots} == {(E, k, N) for E in ES for k in KINDS for N in NS}
    for E, kind, N, slot in slots:
        assert evalcache.slots(make_row(kind, int(E))[None, :], int(N))[0] == int(slot), (E, kind, N)

    # the scripted sequences, replayed through CacheModel line by line
    models, masks = {}, {}
    lines = 0
    for line in p.stdout.splitlines():
        m = re.match(r"^scn (\w+) N=(\d+) E=(\d+) bits=(\d+) chunk=(\d+)$", line)
        if m:
            models[m.group(1)] = (evalcache.CacheModel(int(m.group(2)), int(m.group(4)), int(m.group(5))), int(m.group(3)))
            masks[m.group(1)] = []
            continue
        m = re.match(r"^flush (\w+)$", line)
        if m:
            models[m.group(1)][0].flush()
            continue
        m = re.match(r"^call (\w+) rows=(\S+) hits=([01]+) digest=(\d+) inserts=(\d+) replaced=(\d+)$", line)
        if m:
            model, E = models[m.group(1)]
            X = np.array([script_row(s, E) for s in m.group(2).split(",")], dtype=np.uint32).view(np.float32)
            assert np.array_equal(model.probe(X), model.probe(X))
            hit = "".join(str(v) for v in model.call(X))
            assert hit == m.group(3), line
            assert model.digest() == int(m.group(4)), line
            assert (model.inserts, model.replaced) == (int(m.group(5)), int(m.group(6))), line
            masks[m.group(1)].append(hit)
            lines += 1
    assert set(models) == {"repeat", "n1", "n2", "dups", "race", "bits0", "chunk2", "flush"} and lines >= 30
    # what each sequence is there to show
    assert masks["repeat"][:2] == ["00000", "11111"]                # a repeat of a call: all hits
    assert masks["n1"] == ["0", "0", "0", "1", "0"]                  # N = 1: only the newest key survives
    assert len(models["n2"][0].table) <= 2
    assert masks["dups"] == ["0000", "111"] and models["dups"][0].inserts == 2   # in-call duplicates: one entry
    assert masks["race"] == ["00", "0", "10", "1"]                   # the lowest row won the slot
    assert masks["bits0"] == ["0"] * 8 + ["1"]                       # one word apart: the compare separates them
    assert masks["chunk2"][0] == "00111"                             # chunk k hits what chunk k - 1 inserted
    assert masks["flush"] == ["000", "000", "111"]


def test_key_reads_bit_patterns():
    """-0.0 is not 0.0 to the key, a NaN is its bits, and the two hashes are different functions."""
    for E in ES:
        z, nz, nan = (make_row(k, E)[None, :] for k in ("zero", "negzero", "nan"))
        assert np.array_equal(z, nz)                      # equal as floats
        assert evalcache.tags(z)[0] != evalcache.tags(nz)[0] != evalcache.tags(nan)[0]
        assert evalcache.hash1(z)[0] != evalcache.hash2(z)[0]
    m = evalcache.CacheModel(1, 0)
    assert list(m.call(make_row("zero", 75)[None, :])) == [0]
    assert list(m.call(make_row("negzero", 75)[None, :])) == [0]
    assert list(m.call(make_row("negzero", 75)[None, :])) == [1]


_TAGS = {}


@pytest.mark.parametrize("game", GAMES)
def test_slots_spread_over_a_games_positions(game):
    """4,000 distinct positions of seeded random playouts at N = 4096: the fullest slot holds at most 8
    keys (the binomial expectation of the maximum is about 6), and the 64-bit tags are all distinct.
    Observed maxima with this hash: breakthrough 6, breakthroughSmall 6, reversi 6, hexLG13 6,
    amazons_10x10 6."""
    _, X = game_positions(game)
    tags = evalcache.tags(X)
    assert len(set(int(t) for t in tags)) == 4000
    _TAGS[game] = tags
    fullest = np.bincount(np.array(evalcache.slots(X, 4096)), minlength=4096).max()
    print("%s: fullest slot of 4096 holds %d of 4000 keys" % (game, fullest))
    assert fullest <= 8, (game, fullest)


def test_tags_distinct_over_all_games():
    """The 64-bit tags of the 20,000 positions of the five games are all distinct."""
    for g in GAMES:
        if g not in _TAGS:
            _TAGS[g] = evalcache.tags(game_positions(g)[1])
    allt = np.concatenate([_TAGS[g] for g in GAMES])
    assert allt.size == 20000 and np.unique(allt).size == 20000


def test_refusals_without_a_device():
    lib = _native.nn_lib()
    x = np.zeros((1, 75), dtype=np.float32)
    pol = (_native._FP * 2)()
    hit = np.zeros(1, dtype=np.int32)
    st = _native.GzEvalCacheStats()
    assert not lib.gz_eval_cache_create(None, 16)
    assert lib.gz_nn_last_error().decode() == "eval cache: null argument"
    for rc in (lib.gz_eval_cache_clear(None), lib.gz_eval_cache_stats(None, ctypes.byref(st), 0),
               lib.gz_net_forward_cached(None, None, _native._fptr(x), 1, pol, _native._fptr(x)),
               lib.gz_net_forward_cached_device(None, None, None, x.ctypes.data, 1, None, None),
               lib.gz_eval_cache_probe(None, 0, x.ctypes.data, 1, hit.ctypes.data_as(_native._IP))):
        assert rc != 0
        assert lib.gz_nn_last_error().decode() == "eval cache: null argument"
    lib.gz_eval_cache_destroy(None)
    rl = _native.runner_lib()
    assert rl.gz_runner_set_cache(None, None) != 0
    assert rl.gz_runner_last_error().decode() == "runner: null argument"
    for entries in (0, -5):
        assert not lib.gz_eval_cache_create(None, entries)
        assert lib.gz_nn_last_error().decode() == "eval cache: entries %d (at least 1)" % entries
    with pytest.raises(RuntimeError, match=r"eval cache: entries 0 \(at least 1\)"):
        _native.HipEvalCache(None, 0)
    # cache= together with symmetry= is refused before anything is touched
    with pytest.raises(ValueError, match="cache= together with symmetry="):
        _native.HipNet.forward(None, x, symmetry=object(), cache=object())
    from galvanise_zero_amd.nn.network import HipModel
    with pytest.raises(ValueError, match="cache_entries= together with symmetries="):
        HipModel(None, None, symmetries=object(), cache_entries=4)


def test_entry_points_declared_and_exported():
    names = ["gz_eval_cache_create", "gz_eval_cache_destroy", "gz_eval_cache_clear", "gz_eval_cache_stats",
             "gz_net_forward_cached", "gz_net_forward_cached_device", "gz_eval_cache_probe", "gz_runner_set_cache"]
    header = open(os.path.join(ROOT, "include", "gzero_nn.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.lib_path("libgz_nn.so")], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in names:
        assert n + "(" in header and n in exported, n
    assert ctypes.sizeof(_native.GzEvalCacheStats) == 9 * 8
    # gz_runner_config and gz_runner_stats are ABI: the feature adds functions, not fields
    assert ctypes.sizeof(_native.GzRunnerConfig) == 56 and ctypes.sizeof(_native.GzRunnerStats) == 21 * 8
