"""GPU tests of the canonical orientation (gz_net_forward_sym_canon / _device, gz_symmetry_canon,
gz_runner_set_canonical; csrc/nn/symmetry.hip sym_canon_expand_kernel).

The definition adds no floating-point operation, so everything here is bit for bit: the kernel's
elements and tags against numpy (util.symmetry.canonical_elements), a row against the plain forward of
its canonical image read through the move table (util.symmetry.canonical_forward), the cached form
against the uncached one with util.evalcache.CacheModel on the canonical planes as the judge of which
rows hit, symmetric positions sharing one entry, the self-play runner against the oracle fed by the
uncached canonical forward, and a PlayPoller against the oracle player."""
import os
import subprocess
import sys

import numpy as np
import pytest

from galvanise_zero_amd.defs import templates
from galvanise_zero_amd.nn.desc import NetDesc
from galvanise_zero_amd.nn.weights import random_weights
from galvanise_zero_amd.util import symmetry
from galvanise_zero_amd.util.evalcache import CacheModel
from puct_harness import Setup, sample_key
from test_nn_eval_cache_gpu import COUNTS, script
from test_nn_symmetry_gpu import Tables, assert_bits, random_tables
from test_nn_symmetry_pick_gpu import (MODES, RUNNER, _keys, _run, _runner_conf, _runner_net, board_planes, game_tables, make_net,
                                       net_case)
from test_runner_fp32_gpu import _oracle_conf, _suffix

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SALTS = [0, 0xFFFFFFFF]


# ---- the kernel's elements and tags -------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(5, 8, 8), (3, 5, 5), (13, 10, 10)])
def test_canon_equals_numpy(shape, hip_device):
    """gz_symmetry_canon against numpy, g and tags: E = 320 (16-byte loads), E = 75 (the scalar loop:
    rows that are not 16-byte aligned) and E = 1,300 (more than one pass per thread); n in {1, 3, 257},
    S in {1, 2, 3, 8} of arbitrary permutations, both salts, host and device pointers; a NaN with a
    payload and -0.0 among the rows."""
    import torch
    C, H, W = shape
    desc = NetDesc(C, H, W, 64, 1, [26, 31])
    net = make_net(desc, hip_device, "bf16x3")
    for n in (1, 3, 257):
        x = board_planes(desc, n, 10 * n + C)
        flat = x.reshape(n, -1).view(np.uint32)
        flat[0, -1] = 0x7FC00123                     # a NaN with a payload
        if n > 1:
            flat[1, 0] = 0x80000000                  # -0.0
        d_x = torch.from_numpy(x).to(torch.device("cuda", hip_device))
        for S in (1, 2, 3, 8):
            tables = random_tables(desc, S, 100 + S)
            sym = net.make_symmetry(tables)
            for salt in SALTS:
                want_g, want_t = symmetry.canonical_elements(x, tables, salt)
                for what, kw in (("host", dict(planes=x)), ("device", dict(device_ptr=d_x.data_ptr(), n=n))):
                    g, tags = net.symmetry_canon(sym, salt, **kw)
                    assert np.array_equal(g, want_g), (n, S, salt, what)
                    assert np.array_equal(tags, want_t), (n, S, salt, what)
            if S == 8 and n == 257:
                assert len(set(want_g.tolist())) == S           # every element met
            sym.close()
    net.close()


# ---- exactness without a cache ------------------------------------------------------------------------

EXACT = [("breakthrough", m) for m in MODES] + [(c, m) for c in ("reversi", "5x5") for m in ("bf16x3", "fp16x3-layered")]


@pytest.mark.parametrize("case,precision", EXACT)
def test_canonical_forward_bit_exact(case, precision, hip_device):
    """forward(X, symmetry, canonical=salt) is the plain forward of each row's canonical image read
    through move_src[g], values untouched: n in {1, 5, 300}, both salts."""
    desc, T = net_case(case)
    net = make_net(desc, hip_device, precision)
    sym = net.make_symmetry(T)
    for n in (1, 5, 300):
        x = board_planes(desc, n, 7 * n + len(case))
        for salt in SALTS:
            got = net.forward(x, symmetry=sym, canonical=salt)
            assert_bits(got, symmetry.canonical_forward(net.forward, x, T, salt), (case, precision, n, salt))
    sym.close()
    net.close()


def test_logits_mode_is_served(hip_device):
    desc, T = net_case("reversi")
    net = make_net(desc, hip_device, "bf16x3")
    sym = net.make_symmetry(T)
    x = board_planes(desc, 37, 37)
    net.set_output_logits(True)
    got = net.forward(x, symmetry=sym, canonical=3)
    assert_bits(got, symmetry.canonical_forward(net.forward, x, T, 3), "logits")
    assert float(np.abs(got[0].sum(axis=1) - 1.0).min()) > 1e-3      # logits, not probabilities
    net.set_output_logits(False)
    sym.close()
    net.close()


def test_a_rows_result_is_its_own(hip_device):
    """One row alone, first, last and in the middle of other batches; the host entry point, the device
    entry point and HipModel.predict_on_batch; S = 1 identity tables are the plain forward; some row
    gets g != 0 and then differs from the plain forward (the path is live)."""
    import torch
    from galvanise_zero_amd.nn.network import HipModel
    desc, T = net_case("reversi")
    w = random_weights(desc, 7919, bias_std=0.2)
    model = HipModel(desc, w, hip_device, "bf16x3", symmetries=T, symmetry_mode="canonical", symmetry_salt=99)
    assert model.cache is None
    net, sym = model.net, model.symmetry
    x = board_planes(desc, 64, 64)
    full = net.forward(x, symmetry=sym, canonical=99)
    others = board_planes(desc, 64, 65)
    for where, lo, hi, at in [("alone", 17, 18, 0), ("first", 17, 40, 0), ("last", 0, 18, 17), ("middle", 10, 30, 7)]:
        batch = others[lo:hi].copy()
        batch[at] = x[17]                                            # the neighbours changed
        got = net.forward(batch, symmetry=sym, canonical=99)
        for k in range(len(full)):
            assert np.array_equal(got[k][at], full[k][17]), where
    assert_bits(model.predict_on_batch(x), full, "HipModel.predict_on_batch")
    n = x.shape[0]
    dev = torch.device("cuda", hip_device)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        d_x = torch.from_numpy(x).to(dev)
        d_pol = [torch.full((n, p), -1.0, dtype=torch.float32, device=dev) for p in desc.policy_dist_count]
        d_val = torch.full((n, desc.num_values), -1.0, dtype=torch.float32, device=dev)
        net.forward_sym_canon_device(sym, 99, None, stream.cuda_stream, d_x.data_ptr(), n, [p.data_ptr() for p in d_pol],
                                     d_val.data_ptr())
    stream.synchronize()
    assert_bits([p.cpu().numpy() for p in d_pol] + [d_val.cpu().numpy()], full, "device entry point")

    plain = net.forward(x)
    g, _ = symmetry.canonical_elements(x, T, 99)
    moved = [r for r in range(n) if g[r] != 0 and any(not np.array_equal(full[k][r], plain[k][r]) for k in range(len(full)))]
    assert moved, "no row with g != 0 differs from the plain forward"
    for r in np.flatnonzero(g == 0):
        assert all(np.array_equal(full[k][r], plain[k][r]) for k in range(len(full)))
    one = net.make_symmetry(Tables(T.plane_src[:1], [m[:1] for m in T.move_src]))
    assert_bits(net.forward(x, symmetry=one, canonical=99), plain, "S = 1")
    one.close()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_nn_symmetry_canon_gpu as T
desc, tables = T.net_case("reversi")
net = T.make_net(desc, 0, "bf16x3")
sym = net.make_symmetry(tables)
cache = net.make_cache(4096)
x = T.board_planes(desc, 30, 505)
outs = net.forward(x, symmetry=sym, canonical=12345) + net.forward(x, symmetry=sym, canonical=12345, cache=cache)
np.savez(sys.argv[2], *outs)
"""


def test_chunking_keeps_the_bits(hip_device, tmp_path):
    """GZ_SYM_CHUNK_ROWS=7 in a fresh child process: 30 rows in chunks of 7, 7, 7, 7 and 2, without and
    with a cache."""
    desc, T = net_case("reversi")
    net = make_net(desc, hip_device, "bf16x3")
    sym = net.make_symmetry(T)
    assert "GZ_SYM_CHUNK_ROWS" not in os.environ
    want = net.forward(board_planes(desc, 30, 505), symmetry=sym, canonical=12345)
    out = str(tmp_path / "chunked.npz")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], check=True, env=dict(os.environ, GZ_SYM_CHUNK_ROWS="7"),
                   timeout=120)
    with np.load(out) as z:
        got = [z["arr_%d" % k] for k in range(2 * len(want))]
    assert_bits(got[:len(want)], want, "chunks of 7")
    assert_bits(got[len(want):], want, "chunks of 7, cached")
    sym.close()
    net.close()


# ---- with a cache: CacheModel on the canonical planes is the judge ---------------------------------------

def cached_call(net, sym, cache, model, salt, x, tables, want, what):
    """One cached canonical call: the outputs against `want`, the counters' deltas against the model
    fed the canonical planes.  Returns the model's hit mask."""
    before = cache.stats()
    was = {k: getattr(model, k) for k in COUNTS}
    hit = model.call(symmetry.canonical_planes(x, tables, salt))
    got = net.forward(x, symmetry=sym, canonical=salt, cache=cache)
    assert_bits(got, want, what)
    after = cache.stats()
    for k in COUNTS:
        assert after[k] - before[k] == getattr(model, k) - was[k], (what, k, before, after)
    assert after["rows"] - before["rows"] == x.shape[0] and after["rows"] == after["hits"] + after["forward_rows"]
    return hit


@pytest.mark.parametrize("case", ["breakthrough", "reversi"])
def test_cached_canonical_forward_and_the_model(case, hip_device):
    """tests/test_nn_eval_cache_gpu.py's scripted calls at N in {1, 64, 65536}: after every call the
    outputs equal the uncached canonical forward's, and the deltas of hits, forward_rows, inserts and
    replaced equal those of CacheModel called with the canonical planes."""
    desc, T = net_case(case)
    net = make_net(desc, hip_device, "bf16x3")
    sym = net.make_symmetry(T)
    pool, calls = script(desc, 11 + len(case))
    salt = 5
    uncached = net.forward(pool, symmetry=sym, canonical=salt)
    for N in (1, 64, 65536):
        cache, model = net.make_cache(N), CacheModel(N)
        hits = 0
        for k, idx in enumerate(calls):
            x = np.ascontiguousarray(pool[idx])
            hits += int(cached_call(net, sym, cache, model, salt, x, T, [p[idx] for p in uncached], (case, N, k)).sum())
        if N == 65536:
            assert hits > 300                                 # the repeats hit
        cache.close()
    sym.close()
    net.close()


def test_symmetric_positions_share_an_entry(hip_device):
    """Reversi's eight elements, N = 65,536.  Call 1: 64 random rows X.  Call 2: row j's image under
    element 1 + j % 7.  The model on the canonical planes reports 64 of 64 hits in call 2 (the seed was
    found on the CPU to give no slot collision), the GPU the same -- no row through the forward -- and
    call 2's outputs read through move_src[t] are call 1's, exactly.  The same two calls through the
    plain cache hit nowhere.  A row and its image inside one call both miss and are both exact."""
    desc, T = net_case("reversi")
    net = make_net(desc, hip_device, "bf16x3")
    sym = net.make_symmetry(T)
    S, salt = T.count, 99
    X = board_planes(desc, 64, 6401)
    flat = X.reshape(64, -1)
    for r in range(64):
        assert len({flat[r][p].tobytes() for p in T.plane_src}) == S
    ts = [1 + j % 7 for j in range(64)]
    Y = np.array([flat[j][T.plane_src[ts[j]]] for j in range(64)]).reshape(X.shape)
    cache, model = net.make_cache(65536), CacheModel(65536)
    uncached_x = net.forward(X, symmetry=sym, canonical=salt)
    uncached_y = net.forward(Y, symmetry=sym, canonical=salt)
    h1 = cached_call(net, sym, cache, model, salt, X, T, uncached_x, "call 1")
    f0 = cache.stats()["forward_rows"]
    h2 = cached_call(net, sym, cache, model, salt, Y, T, uncached_y, "call 2")
    assert h1.sum() == 0 and h2.sum() == 64, (h1.sum(), h2.sum())
    st = cache.stats()
    assert st["forward_rows"] == f0 == 64 and st["hits"] == 64
    for j in range(64):
        for r in range(len(T.move_src)):
            assert np.array_equal(uncached_x[r][j].view(np.uint32), uncached_y[r][j][T.move_src[r][ts[j]]].view(np.uint32)), (j, r)
        assert np.array_equal(uncached_x[-1][j].view(np.uint32), uncached_y[-1][j].view(np.uint32))

    plain_cache = net.make_cache(65536)
    assert_bits(net.forward(X, cache=plain_cache), net.forward(X), "plain cache, call 1")
    assert_bits(net.forward(Y, cache=plain_cache), net.forward(Y), "plain cache, call 2")
    pst = plain_cache.stats()
    assert pst["hits"] == 0 and pst["forward_rows"] == 128, pst
    plain_cache.close()

    # a row and its image in one call: nothing is deduplicated inside a call
    Z = board_planes(desc, 1, 6402)
    pair = np.concatenate([Z, Z.reshape(1, -1)[:, T.plane_src[3]].reshape(Z.shape)])
    before = cache.stats()
    hit = cached_call(net, sym, cache, model, salt, pair, T, net.forward(pair, symmetry=sym, canonical=salt), "a pair in one call")
    assert hit.sum() == 0 and cache.stats()["forward_rows"] - before["forward_rows"] == 2
    assert cached_call(net, sym, cache, model, salt, pair, T, net.forward(pair, symmetry=sym, canonical=salt), "the pair again").all()
    cache.close()
    sym.close()
    net.close()


def test_refusals_leave_the_net_alone(hip_device):
    desc, T = net_case("breakthrough")
    net = make_net(desc, hip_device, "bf16x3")
    other = make_net(desc, hip_device, "bf16")
    sym, foreign = net.make_symmetry(T), other.make_cache(64)
    x = board_planes(desc, 3, 703)
    before = net.forward(x)
    wrong = net.make_symmetry(random_tables(NetDesc(5, 6, 6, 64, 1, list(desc.policy_dist_count)), 2, 8))
    with pytest.raises(RuntimeError, match=r"failed: symmetry: tables of plane_elems .* are not the net's"):
        net.forward(x, symmetry=wrong, canonical=0)
    wrong.close()
    with pytest.raises(RuntimeError, match=r"gz_net_forward_sym_canon failed: eval cache: made for another net"):
        net.forward(x, symmetry=sym, canonical=0, cache=foreign)
    assert foreign.stats()["rows"] == 0
    assert_bits(net.forward(x), before, "plain forward after the refusals")
    foreign.close()
    sym.close()
    other.close()
    net.close()


# ---- runner ------------------------------------------------------------------------------------------

def _run_canon(hip_device, tables, entries):
    """test_nn_symmetry_pick_gpu._run's runner in canonical mode with a cache of `entries` entries: the
    samples per pool, the stats, the cache's stats, the pick-rows counter, the salt."""
    from galvanise_zero_amd.runner import SelfPlayRunner
    setup, desc, net = _runner_net(hip_device)
    sym, cache = net.make_symmetry(tables), net.make_cache(entries)
    c = RUNNER
    r = SelfPlayRunner(net, setup.sm, setup.transformer, _runner_conf(), device=hip_device, num_threads=c["threads"],
                       pools_per_thread=c["ppt"], batch_size=c["B"], seed=c["seed"], keep_samples=True,
                       spin_yield_playouts=c["spin"], min_launch_rows=16, max_launch_wait_us=2000, symmetry=sym,
                       symmetry_mode="canonical", cache=cache)
    assert r.symmetry_salt == c["seed"] & 0xFFFFFFFF and r.cache is cache
    r.start()
    r.wait_rows(c["rows"], timeout_s=120)
    r.stop()
    st, cst, picked = r.stats(), r.cache_stats(), r.sym_pick_rows()
    by_pool = {}
    for s in r.fetch_samples():
        by_pool.setdefault(int(s["match_identifier"].split("_")[1][1:]), []).append(s)
    r.close()
    cache.close()
    sym.close()
    net.close()
    print("canonical runner, S = %d: stats %s, cache %s, pick rows %d, samples per pool %s"
          % (tables.plane_src.shape[0], st, cst, picked, {p: len(v) for p, v in by_pool.items()}))
    return setup, by_pool, st, cst, picked


@pytest.mark.timeout(600)
def test_runner_canonical_with_a_cache_matches_oracle(hip_device):
    """Breakthrough's reflection in canonical mode through a 4,096-entry cache: one pool (the one with
    the most samples) replayed through oracle.puct_ref.Manager with the predictions of the UNCACHED
    net.forward(x, symmetry, canonical=salt) gives every runner sample of that pool; the cache hit,
    rows == hits + forward_rows, and every row went through the symmetry path."""
    from oracle import puct_ref as P
    T, _, _ = game_tables("breakthrough")
    c = RUNNER
    setup, got, st, cst, picked = _run_canon(hip_device, T, 4096)
    assert cst["hits"] > 0 and cst["rows"] == cst["hits"] + cst["forward_rows"], cst
    assert picked == st["rows"] == cst["rows"] >= c["rows"]

    _, desc, net = _runner_net(hip_device)
    sym = net.make_symmetry(T)
    salt = c["seed"] & 0xFFFFFFFF
    t = setup.transformer
    pool = max(got, key=lambda p: len(got[p]))
    mine = got[pool]
    man = P.Manager(setup.ref_sm, setup.ref_planes, c["B"], P.UniqueStates(setup.ref_planes.hash_mask(), 1000),
                    "t", c["seed"], pool * c["B"], list(t.policy_dist_count), t.num_rewards, setup.num_prev_states)
    man.start(_oracle_conf(_runner_conf(), c["spin"]))
    pred = (0, [np.zeros(0, np.float32)] * setup.sm.role_count, np.zeros(0, np.float32))
    for _ in range(c["rows"] // c["B"]):
        if len(man.samples) >= len(mine):
            break
        buf = man.poll(*pred)
        assert buf is not None
        x = buf.reshape(-1, t.num_channels, t.num_cols, t.num_rows)
        outs = net.forward(x, symmetry=sym, canonical=salt)
        pred = (x.shape[0], outs[:-1], outs[-1])
    n = len(mine)
    assert n >= 8 and len(man.samples) >= n, (n, len(man.samples))
    assert _keys(setup, mine) == [sample_key(setup, _suffix(s), False) for s in man.samples[:n]]
    print("%d samples of pool %d identical to the oracle on the uncached canonical forward" % (n, pool))
    sym.close()
    net.close()


@pytest.mark.timeout(300)
def test_runner_identity_tables_with_a_cache_change_nothing(hip_device):
    """S = 1 tables in canonical mode with a cache: every pool's samples equal the plain runner's on
    their common prefix."""
    T, _, _ = game_tables("breakthrough")
    one = Tables(T.plane_src[:1], [m[:1] for m in T.move_src])
    setup, plain, _, picked0 = _run(hip_device, None)
    _, same, st, cst, picked = _run_canon(hip_device, one, 4096)
    assert picked0 == 0 and picked == st["rows"] == cst["rows"] >= RUNNER["rows"]
    compared = 0
    for pool in range(RUNNER["ppt"]):
        n = min(len(plain.get(pool, [])), len(same.get(pool, [])))
        assert _keys(setup, plain.get(pool, [])[:n]) == _keys(setup, same.get(pool, [])[:n]), pool
        compared += n
    assert compared >= 8, compared


def test_runner_refusals(hip_device, monkeypatch):
    from galvanise_zero_amd.runner import SelfPlayRunner
    T, _, _ = game_tables("breakthrough")
    setup, desc, net = _runner_net(hip_device)
    other = make_net(desc, hip_device, "bf16")
    sym, cache, foreign = net.make_symmetry(T), net.make_cache(64), other.make_cache(64)
    wrong = net.make_symmetry(random_tables(NetDesc(5, 6, 6, 64, 1, list(desc.policy_dist_count)), 2, 8))

    def runner(**kw):
        return SelfPlayRunner(net, setup.sm, setup.transformer, _runner_conf(), device=hip_device, num_threads=1,
                              pools_per_thread=2, batch_size=8, seed=1, spin_yield_playouts=1000, **kw)
    with pytest.raises(RuntimeError, match=r"gz_runner_set_canonical: symmetry: tables of plane_elems .* are not the net's"):
        runner(symmetry=wrong, symmetry_mode="canonical")
    with pytest.raises(RuntimeError, match=r"gz_runner_set_canonical: eval cache: made for another net"):
        runner(symmetry=sym, symmetry_mode="canonical", cache=foreign)
    r = runner(symmetry=sym, symmetry_mode="canonical", cache=cache)
    with pytest.raises(RuntimeError, match=r"gz_runner_set_canonical: runner: gz_runner_set_canonical on a runner that already has a canonical setting"):
        r.set_canonical(sym, 0)
    with pytest.raises(RuntimeError, match=r"gz_runner_set_symmetry: runner: gz_runner_set_symmetry on a runner in canonical mode"):
        r.set_symmetry(sym, 0)
    with pytest.raises(RuntimeError, match=r"gz_runner_set_cache: runner: gz_runner_set_cache on a runner in canonical mode"):
        r.set_cache(cache)
    r.close()
    r = runner(symmetry=sym)
    with pytest.raises(RuntimeError, match=r"gz_runner_set_canonical: runner: gz_runner_set_canonical on a runner that already has a symmetry"):
        r.set_canonical(sym, 0)
    # the old refusals, unchanged
    with pytest.raises(RuntimeError, match=r"gz_runner_set_cache: runner: gz_runner_set_cache on a runner with a symmetry \(the two do not compose\)"):
        r.set_cache(cache)
    r.close()
    r = runner(cache=cache)
    with pytest.raises(RuntimeError, match=r"gz_runner_set_canonical: runner: gz_runner_set_canonical on a runner that already has an evaluation cache"):
        r.set_canonical(sym, 0)
    with pytest.raises(RuntimeError, match=r"gz_runner_set_symmetry: runner: gz_runner_set_symmetry on a runner with an evaluation cache \(the two do not compose\)"):
        r.set_symmetry(sym, 0)
    r.close()
    r = runner()
    r.start()
    with pytest.raises(RuntimeError, match=r"gz_runner_set_canonical: runner: gz_runner_set_canonical after gz_runner_start"):
        r.set_canonical(sym, 0, cache)
    r.wait_rows(64, timeout_s=60)
    r.stop()
    assert r.sym_pick_rows() == 0 and cache.stats()["rows"] == 0
    r.close()
    monkeypatch.setenv("GZ_RUNNER_ZERO_COPY", "1")
    with pytest.raises(RuntimeError, match=r"gz_runner_set_canonical: runner: gz_runner_set_canonical on a zero-copy runner"):
        runner(symmetry=sym, symmetry_mode="canonical")
    monkeypatch.delenv("GZ_RUNNER_ZERO_COPY")
    for s in (sym, wrong):
        s.close()
    for c in (cache, foreign):
        c.close()
    other.close()
    net.close()


# ---- player ------------------------------------------------------------------------------------------

def test_player_on_the_canonical_forward(hip_device):
    """PlayPoller at batch 32 against the oracle player, the native side fed by
    HipModel(symmetry_mode="canonical", cache_entries=4096) and every batch checked to be
    util.symmetry.canonical_forward of the plain forward: planes at every poll, moves and root visits
    identical; the searches re-meet positions, so the cache hits."""
    from galvanise_zero_amd.nn.network import HipModel
    from test_puct_parity import _player_run
    game = "breakthroughSmall"
    T, _, _ = game_tables(game)
    setup = Setup(game)
    model = HipModel(setup.desc, setup.weights, hip_device, "bf16x3", symmetries=T, symmetry_mode="canonical", symmetry_salt=17,
                     cache_entries=4096)
    d = setup.desc
    shape = (-1, d.input_channels, d.input_columns, d.input_rows)
    seen = []

    def nn(planes):
        x = np.asarray(planes, np.float32).reshape(shape)
        seen.append(symmetry.canonical_elements(x, T, 17)[0])
        got = model.predict_on_batch(x)
        assert_bits(got, symmetry.canonical_forward(model.net.forward, x, T, 17), "a search batch")
        return got
    setup.nn = nn
    conf = templates.base_puct_config(batch_size=32, choose="choose_temperature", dirichlet_noise_pct=0.25,
                                      think_time=-1, converged_visits=1)
    visits = _player_run(setup, conf, 160, 3, seed=17)
    assert sum(t for _, t, _ in visits[0]) > 100
    assert (np.concatenate(seen) != 0).any()             # the search did meet reflected evaluations
    st = model.cache.stats()
    print("player: cache stats %s" % st)
    assert st["hits"] > 0 and st["rows"] == st["hits"] + st["forward_rows"]
