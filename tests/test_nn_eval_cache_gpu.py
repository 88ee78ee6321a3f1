"""GPU tests of the evaluation cache (gz_eval_cache, gz_net_forward_cached / _device,
gz_eval_cache_probe; csrc/nn/eval_cache.hip cache_probe_kernel / cache_compact_kernel /
cache_fill_kernel).

A row's outputs are a function of the row alone, so everything here is bit for bit: a cached call
against the plain forward of the same rows, the kernel's hit mask and counters against the serial
model (util.evalcache.CacheModel), the plane compare with the tag filter switched off, chunking, the
flushes a weight roll and the output-logits switch cause, every entry point, and a PlayPoller on a
cached model against the oracle player."""
import os
import subprocess
import sys

import numpy as np
import pytest

from galvanise_zero_amd.defs import templates
from galvanise_zero_amd.nn.weights import random_weights, to_blob
from galvanise_zero_amd.util.evalcache import CacheModel
from puct_harness import Setup
from test_nn_symmetry_gpu import assert_bits
from test_nn_symmetry_pick_gpu import board_planes, make_net, net_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = [1, 2, 64, 65536]
EXACT = [("breakthrough", m) for m in ("bf16x3", "bf16", "fp32-ieee", "fp16x3-layered")] + [("reversi", "bf16x3"), ("5x5", "bf16x3")]
COUNTS = ("hits", "forward_rows", "inserts", "replaced")


def script(desc, seed):
    """The calls of the exactness test as index lists into one pool of 600 distinct rows: fresh rows,
    exact repeats, half old and half new rows interleaved, in-call duplicates; n in {1, 2, 65, 300}."""
    pool = board_planes(desc, 600, seed)
    assert len({r.tobytes() for r in pool}) == 600
    fresh = np.arange(300)
    mixed = np.empty(300, dtype=np.int64)
    mixed[0::2] = np.arange(150)                    # old
    mixed[1::2] = np.arange(300, 450)               # new
    dups = np.repeat(np.arange(450, 483), 2)[:65]   # every row twice in one call
    calls = [fresh[:1], fresh[:1], fresh[:2], fresh[:65], fresh, fresh, mixed, mixed[:65], dups, dups, np.arange(599, 600),
             np.array([483, 5, 483, 484, 5, 485, 484])]
    assert {len(c) for c in calls} >= {1, 2, 65, 300}
    return pool, calls


def check_call(net, cache, model, x, plain, what):
    """One cached call: the probe before it and the counters after it against the model, the outputs
    against the plain forward's."""
    before = cache.stats()
    seen = net.cache_probe(cache, planes=x)
    want = {k: getattr(model, k) for k in COUNTS}
    hit = model.call(x)
    got = net.forward(x, cache=cache)
    assert_bits(got, plain, what)
    assert np.array_equal(seen, hit), (what, seen, hit)
    after = cache.stats()
    for k in COUNTS:
        assert after[k] - before[k] == getattr(model, k) - want[k], (what, k, before, after)
    assert after["rows"] - before["rows"] == x.shape[0] and after["calls"] - before["calls"] == 1
    assert after["rows"] == after["hits"] + after["forward_rows"]
    return hit


@pytest.mark.parametrize("case,precision", EXACT)
def test_cached_forward_bit_exact_and_the_model(case, precision, hip_device):
    """Scripted calls at N in {1, 2, 64, 65536}: after every call the outputs equal the plain forward
    of the same rows, gz_eval_cache_probe taken before the call equals CacheModel's hit mask, and the
    deltas of hits, forward_rows, inserts and replaced equal the model's; a call that hits everywhere
    sends nothing through the forward.  E = 320 takes the 16-byte path, E = 75 (5x5) the scalar one."""
    desc, _ = net_case(case)
    net = make_net(desc, hip_device, precision)
    pool, calls = script(desc, 11 + len(case))
    plain = net.forward(pool)
    for N in ENTRIES:
        cache, model = net.make_cache(N), CacheModel(N)
        st = cache.stats()
        assert st["entries"] == N and st["entry_bytes"] % 16 == 0 and st["rows"] == 0
        all_hit = 0
        for k, idx in enumerate(calls):
            x = np.ascontiguousarray(pool[idx])
            f0 = cache.stats()["forward_rows"]
            hit = check_call(net, cache, model, x, [p[idx] for p in plain], (case, precision, N, k))
            if hit.all():
                all_hit += 1
                assert cache.stats()["forward_rows"] == f0
        if N == 65536:
            assert all_hit >= 3                               # the repeats hit everywhere
        if N == 1:
            assert model.replaced > 0 and len(model.table) == 1
        cache.close()
    net.close()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_nn_eval_cache_gpu as T
T.child(sys.argv[2], sys.argv[3])
"""


def compare_rows(desc):
    """Rows one word apart: a base row, then the base with word 0, word E - 1 and a middle word
    flipped, then word 0 as 0.0 and as -0.0; the last row once more."""
    base = board_planes(desc, 1, 321)[0].reshape(-1)
    E = base.size
    base[0] = 1.0                                  # (so that 0.0 there is another row)
    rows = [base.copy()]
    for w in (0, E - 1, E // 2):
        rows.append(base.copy())
        rows[-1][w] = 1.0 - rows[-1][w]
        rows.append(base.copy())
    zero, neg = base.copy(), base.copy()
    zero[0] = 0.0
    neg.view(np.uint32)[0] = 0x80000000
    rows += [zero, neg, neg.copy()]
    return np.array(rows, dtype=np.float32).reshape((len(rows),) + (desc.input_channels, desc.input_columns, desc.input_rows))


def child(what, out):
    """In a fresh process (the environment switches are read at creation): the cached outputs, probes
    and counters of `what`, saved for the parent to judge."""
    desc, _ = net_case("breakthrough")
    net = make_net(desc, 0, "bf16x3")
    res = {}
    if what == "compare":
        cache = net.make_cache(1)
        x = compare_rows(desc)
        for r in range(x.shape[0]):                  # one row per call: each meets the row before it
            res["probe%d" % r] = net.cache_probe(cache, planes=x[r:r + 1])
            for k, a in enumerate(net.forward(x[r:r + 1], cache=cache)):
                res["out%d_%d" % (r, k)] = a
    else:
        cache = net.make_cache(65536)
        x = chunk_rows(desc)
        for c in range(2):
            for k, a in enumerate(net.forward(x, cache=cache)):
                res["out%d_%d" % (c, k)] = a
            st = cache.stats()
            res["stats%d" % c] = np.array([st[k] for k in COUNTS])
    np.savez(out, **res)


def chunk_rows(desc):
    a = board_planes(desc, 2, 77)
    return np.ascontiguousarray(a[[0, 1, 0, 1, 0]])


def run_child(what, tmp_path, **env):
    out = str(tmp_path / (what + ".npz"))
    assert not any(k in os.environ for k in env)
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, what, out], check=True, env=dict(os.environ, **env), timeout=120)
    return np.load(out)


def test_the_compare_is_live(hip_device, tmp_path):
    """GZ_EVAL_CACHE_TAG_BITS=0 and N = 1 in a fresh child process: every probe passes the tag filter
    and meets the entry of the row before it, one word away -- word 0, word E - 1, a middle word, and
    -0.0 against 0.0 -- so only the compare of the planes can make it miss.  All miss and all equal the
    plain forward; a repeat of the last row hits."""
    desc, _ = net_case("breakthrough")
    net = make_net(desc, hip_device, "bf16x3")
    x = compare_rows(desc)
    flat = x.reshape(x.shape[0], -1).view(np.uint32)
    for r in range(1, x.shape[0] - 1):
        assert (flat[r] != flat[r - 1]).sum() == 1, r
    assert np.array_equal(x[-3], x[-2]) and not np.array_equal(flat[-3], flat[-2])       # 0.0 == -0.0 as floats
    plain = net.forward(x)
    model = CacheModel(1, tag_bits=0)
    with run_child("compare", tmp_path, GZ_EVAL_CACHE_TAG_BITS="0") as z:
        for r in range(x.shape[0]):
            want = model.call(x[r:r + 1])
            assert want[0] == (1 if r == x.shape[0] - 1 else 0)
            assert np.array_equal(z["probe%d" % r], want), r
            assert_bits([z["out%d_%d" % (r, k)] for k in range(len(plain))], [p[r:r + 1] for p in plain], ("compare", r))
    net.close()


def test_chunking_keeps_the_bits_and_the_hits(hip_device, tmp_path):
    """GZ_EVAL_CACHE_CHUNK_ROWS=2 in a fresh child process: rows a b a b a in chunks of 2, 2 and 1 --
    the second and third chunk hit what the first inserted (CacheModel with chunk_rows = 2: three hits
    where one chunk would give none), then the whole call again hits everywhere."""
    desc, _ = net_case("breakthrough")
    net = make_net(desc, hip_device, "bf16x3")
    x = chunk_rows(desc)
    plain = net.forward(x)
    model = CacheModel(65536, chunk_rows=2)
    assert list(CacheModel(65536).call(x)) == [0, 0, 0, 0, 0]
    with run_child("chunks", tmp_path, GZ_EVAL_CACHE_CHUNK_ROWS="2") as z:
        for c, want in enumerate(([0, 0, 1, 1, 1], [1, 1, 1, 1, 1])):
            assert list(model.call(x)) == want
            assert_bits([z["out%d_%d" % (c, k)] for k in range(len(plain))], plain, ("chunks", c))
            assert list(z["stats%d" % c]) == [getattr(model, k) for k in COUNTS], c
    net.close()


def test_invalidation(hip_device):
    """A filled cache after set_weights with another seed: the next call misses everywhere
    (flushes + 1) and equals the new plain forward; the same through gz_net_set_weights_device, through
    a change of set_output_logits (setting the mode it already has flushes nothing), and clear()."""
    import torch
    desc, _ = net_case("breakthrough")
    net = make_net(desc, hip_device, "bf16x3")
    cache, model = net.make_cache(65536), CacheModel(65536)
    x = board_planes(desc, 65, 909)

    def settle(what):
        """all misses, one flush more, the plain forward's bits; then all hits"""
        f0 = cache.stats()["flushes"]
        assert not net.cache_probe(cache, planes=x).any(), what
        model.flush()
        plain = net.forward(x)
        assert not check_call(net, cache, model, x, plain, what).any()
        assert cache.stats()["flushes"] == f0 + 1, what
        assert check_call(net, cache, model, x, plain, what).all()
        return plain

    plain0 = net.forward(x)
    assert not check_call(net, cache, model, x, plain0, "fill").any()
    assert check_call(net, cache, model, x, plain0, "filled").all()
    net.set_weights(to_blob(random_weights(desc, 7920, bias_std=0.2)))
    plain1 = settle("set_weights")
    assert not np.array_equal(plain0[0], plain1[0])
    blob = torch.from_numpy(to_blob(random_weights(desc, 7921, bias_std=0.2))).to(torch.device("cuda", hip_device))
    net.set_weights_device(blob.data_ptr(), blob.numel())
    plain2 = settle("set_weights_device")
    assert not np.array_equal(plain1[0], plain2[0])
    net.set_output_logits(True)
    logits = settle("logits on")
    assert float(np.abs(logits[0].sum(axis=1) - 1.0).min()) > 1e-3
    net.set_output_logits(True)                                  # no change: no flush
    f0 = cache.stats()["flushes"]
    assert check_call(net, cache, model, x, logits, "logits still on").all() and cache.stats()["flushes"] == f0
    net.set_output_logits(False)
    assert_bits(settle("logits off"), plain2, "back to probabilities")
    cache.clear()
    f0 = cache.stats()["flushes"]
    assert f0 == model.flushes + 1 and not net.cache_probe(cache, planes=x).any()
    model.table = {}
    assert not check_call(net, cache, model, x, plain2, "clear").any() and cache.stats()["flushes"] == f0
    st = cache.stats(reset=True)
    assert st["rows"] > 0 and cache.stats()["rows"] == 0 and cache.stats()["inserts"] == 0
    cache.close()
    net.close()


def test_entry_points(hip_device):
    """One row alone, first, last and in the middle of a batch, cold and warm; the host entry, the
    device entry on a torch stream (probe through a device pointer) and HipModel(cache_entries=...);
    two caches on one net are independent."""
    import torch
    from galvanise_zero_amd.nn.network import HipModel
    desc, _ = net_case("reversi")
    w = random_weights(desc, 7919, bias_std=0.2)
    hm = HipModel(desc, w, hip_device, "bf16x3", cache_entries=4096)
    net = hm.net
    x = board_planes(desc, 64, 64)
    full = net.forward(x)
    for where, lo, hi, at in [("alone", 17, 18, 0), ("first", 17, 40, 0), ("last", 0, 18, 17), ("middle", 10, 30, 7)]:
        for cache in (net.make_cache(4096), hm.cache):            # a cold table, and one that fills up
            got = net.forward(np.ascontiguousarray(x[lo:hi]), cache=cache)
            assert_bits(got, [f[lo:hi] for f in full], where)
            assert all(np.array_equal(got[k][at], full[k][17]) for k in range(len(full))), where
    assert_bits(hm.predict_on_batch(x), full, "HipModel.predict_on_batch")
    st = hm.cache.stats()
    assert st["hits"] > 0 and st["rows"] == st["hits"] + st["forward_rows"]
    assert_bits(hm.predict_on_batch(x), full, "HipModel.predict_on_batch, warm")
    assert hm.cache.stats()["forward_rows"] == st["forward_rows"]

    n = x.shape[0]
    dev = torch.device("cuda", hip_device)
    stream = torch.cuda.Stream(device=dev)
    a, b = net.make_cache(64), net.make_cache(64)
    ma, mb = CacheModel(64), CacheModel(64)
    for rnd, (cache, model) in enumerate([(a, ma), (a, ma), (b, mb)]):
        with torch.cuda.stream(stream):
            d_x = torch.from_numpy(x).to(dev)
            d_pol = [torch.full((n, p), -1.0, dtype=torch.float32, device=dev) for p in desc.policy_dist_count]
            d_val = torch.full((n, desc.num_values), -1.0, dtype=torch.float32, device=dev)
            stream.synchronize()
            seen = net.cache_probe(cache, device_ptr=d_x.data_ptr(), n=n)
            net.forward_cached_device(cache, stream.cuda_stream, d_x.data_ptr(), n, [p.data_ptr() for p in d_pol], d_val.data_ptr())
        stream.synchronize()
        assert np.array_equal(seen, model.call(x)), rnd
        assert_bits([p.cpu().numpy() for p in d_pol] + [d_val.cpu().numpy()], full, ("device entry point", rnd))
    sa, sb = a.stats(), b.stats()
    assert (sa["calls"], sa["hits"], sa["inserts"]) == (2, ma.hits, ma.inserts) and ma.hits > 0
    assert (sb["calls"], sb["hits"], sb["inserts"]) == (1, 0, mb.inserts)            # b never saw a's entries
    for c in (a, b):
        c.close()
    net.close()


def test_refusals_leave_the_net_alone(hip_device):
    from galvanise_zero_amd._native import HipSymmetry
    desc, T = net_case("breakthrough")
    net, other = make_net(desc, hip_device, "bf16x3"), make_net(desc, hip_device, "bf16")
    x = board_planes(desc, 3, 703)
    before = net.forward(x)
    foreign = other.make_cache(16)
    with pytest.raises(RuntimeError, match=r"gz_net_forward_cached failed: eval cache: made for another net"):
        net.forward(x, cache=foreign)
    with pytest.raises(RuntimeError, match=r"gz_eval_cache_create failed: eval cache: entries 0 \(at least 1\)"):
        net.make_cache(0)
    with pytest.raises(RuntimeError, match=r"gz_eval_cache_create failed: eval cache: %d entries of \d+ bytes exceed the bound of \d+ bytes" % (1 << 40)):
        net.make_cache(1 << 40)
    sym = HipSymmetry(T.plane_src, T.move_src, device=hip_device)
    with pytest.raises(ValueError, match="cache= together with symmetry="):
        net.forward(x, symmetry=sym, cache=foreign)
    sym.close()
    assert foreign.stats()["rows"] == 0
    assert_bits(net.forward(x), before, "plain forward after the refusals")
    mine = net.make_cache(16)
    assert_bits(net.forward(x, cache=mine), before, "cached forward after the refusals")
    for c in (mine, foreign):
        c.close()
    other.close()
    net.close()


def test_player_on_a_cached_model(hip_device):
    """PlayPoller at batch 32 on HipModel(cache_entries=...) against the oracle player
    (tests/test_puct_parity.py's harness, fed the plain forward's bits -- every batch is checked to be
    those): planes at every poll, moves and root visits identical, and the three searches, each
    re-meeting positions of the one before it, do hit."""
    from galvanise_zero_amd.nn.network import HipModel
    from test_puct_parity import _player_run
    setup = Setup("breakthroughSmall")
    model = HipModel(setup.desc, setup.weights, hip_device, "bf16x3", cache_entries=65536)
    d = setup.desc
    shape = (-1, d.input_channels, d.input_columns, d.input_rows)

    def nn(planes):
        x = np.asarray(planes, np.float32).reshape(shape)
        got = model.predict_on_batch(x)
        assert_bits(got, model.net.forward(x), "a search batch")
        return got
    setup.nn = nn
    conf = templates.base_puct_config(batch_size=32, choose="choose_temperature", dirichlet_noise_pct=0.25,
                                      think_time=-1, converged_visits=1)
    visits = _player_run(setup, conf, 160, 3, seed=17)
    assert sum(t for _, t, _ in visits[0]) > 100
    st = model.cache.stats()
    print("player: cache stats %s" % st)
    assert st["hits"] > 0 and st["rows"] == st["hits"] + st["forward_rows"]


# ---- runner ------------------------------------------------------------------------------------------

def _run_cached(hip_device, entries=65536):
    """test_nn_symmetry_pick_gpu._run's runner (breakthrough, 1 thread x 2 pools x 8 games, 4
    evaluations per move) with a cache set: the samples' keys per pool, the stats, the cache's stats."""
    from galvanise_zero_amd.runner import SelfPlayRunner
    from test_nn_symmetry_pick_gpu import RUNNER as c, _keys, _runner_conf, _runner_net
    setup, desc, net = _runner_net(hip_device)
    cache = net.make_cache(entries)
    r = SelfPlayRunner(net, setup.sm, setup.transformer, _runner_conf(), device=hip_device, num_threads=c["threads"],
                       pools_per_thread=c["ppt"], batch_size=c["B"], seed=c["seed"], keep_samples=True,
                       spin_yield_playouts=c["spin"], min_launch_rows=16, max_launch_wait_us=2000, cache=cache)
    r.start()
    r.wait_rows(c["rows"], timeout_s=120)
    r.stop()
    st, cst = r.stats(), r.cache_stats()
    by_pool = {}
    for s in r.fetch_samples():
        by_pool.setdefault(int(s["match_identifier"].split("_")[1][1:]), []).append(s)
    r.close()
    cache.close()
    net.close()
    print("cached runner: stats %s, cache %s, samples per pool %s" % (st, cst, {p: len(v) for p, v in by_pool.items()}))
    return setup, by_pool, {p: _keys(setup, v) for p, v in by_pool.items()}, st, cst


def _check_cached_run(setup, plain, keys, st, cst):
    """Every pool's samples equal those of the runner without a cache on their common prefix (each pool
    is deterministic; a run's last samples depend on when it stopped); the cache saw every row."""
    from test_nn_symmetry_pick_gpu import RUNNER, _keys
    compared = 0
    for pool in range(RUNNER["ppt"]):
        n = min(len(plain.get(pool, [])), len(keys.get(pool, [])))
        assert _keys(setup, plain.get(pool, [])[:n]) == keys.get(pool, [])[:n], pool
        compared += n
    assert compared >= 8, compared
    assert cst["rows"] == st["rows"] >= RUNNER["rows"]
    assert cst["rows"] == cst["hits"] + cst["forward_rows"] and cst["hits"] > 0, cst


@pytest.mark.timeout(600)
def test_runner_with_a_cache_matches_plain_and_oracle(hip_device):
    """N = 65536.  The samples of every pool equal the plain runner's on the same seed, and one pool
    replayed through oracle.puct_ref.Manager fed by the plain net.forward gives the runner's samples.
    rows == hits + forward_rows, and hits > 0 whatever the timing: the lowest row of the first launch is
    an initial position, so its key goes in then; each of the 16 slots plays several games in its 1,500
    evaluations, and every later game starts from that position, which hits unless one of the keys
    inserted meanwhile fell on the same one of 65,536 slots -- for the first restart, after some
    thousand inserts, a chance of a few per cent, and all of the tens of restarts would have to lose.
    Which positions are evaluated is the seed's doing, not the timing's."""
    from oracle import puct_ref as P
    from puct_harness import sample_key
    from test_nn_symmetry_pick_gpu import RUNNER as c, _run, _runner_conf, _runner_net
    from test_runner_fp32_gpu import _oracle_conf, _suffix
    setup, plain, _, _ = _run(hip_device, None)
    _, got, keys, st, cst = _run_cached(hip_device)
    _check_cached_run(setup, plain, keys, st, cst)

    _, desc, net = _runner_net(hip_device)
    t = setup.transformer
    pool = max(got, key=lambda p: len(got[p]))
    mine = keys[pool]
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
        outs = net.forward(x)
        pred = (x.shape[0], outs[:-1], outs[-1])
    n = len(mine)
    assert n >= 8 and len(man.samples) >= n, (n, len(man.samples))
    assert mine == [sample_key(setup, _suffix(s), False) for s in man.samples[:n]]
    print("%d samples of pool %d identical to the oracle on the plain forward" % (n, pool))
    net.close()


_RUNNER_CHILD = r"""
import pickle, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_nn_eval_cache_gpu as T
_, _, keys, st, cst = T._run_cached(0)
pickle.dump((keys, st, cst), open(sys.argv[2], "wb"))
"""


@pytest.mark.timeout(300)
def test_runner_with_a_cache_and_output_staging(hip_device, tmp_path):
    """GZ_RUNNER_OUT_STAGING=1 in a fresh child process: probe and fill write the d_out blocks and the
    third stream copies them; the same samples, the same counts' identity."""
    import pickle
    from test_nn_symmetry_pick_gpu import _run
    setup, plain, _, _ = _run(hip_device, None)
    out = str(tmp_path / "staged.pkl")
    assert "GZ_RUNNER_OUT_STAGING" not in os.environ
    subprocess.run([sys.executable, "-c", _RUNNER_CHILD, ROOT, out], check=True, env=dict(os.environ, GZ_RUNNER_OUT_STAGING="1"),
                   timeout=240)
    keys, st, cst = pickle.load(open(out, "rb"))
    _check_cached_run(setup, plain, keys, st, cst)


@pytest.mark.timeout(300)
def test_runner_roll_flushes_the_cache(hip_device):
    """A generation roll mid-play: the run completes, the launch after the roll flushes (the roll is
    applied on the launcher thread), and both generations hit -- 6,000 rows are 375 evaluations per
    slot, more than a game, so every slot restarts from the initial position on either side."""
    from galvanise_zero_amd.runner import SelfPlayRunner
    from test_nn_symmetry_pick_gpu import RUNNER as c, _runner_conf, _runner_net
    setup, desc, net = _runner_net(hip_device)
    cache = net.make_cache(65536)
    r = SelfPlayRunner(net, setup.sm, setup.transformer, _runner_conf(), device=hip_device, num_threads=c["threads"],
                       pools_per_thread=c["ppt"], batch_size=c["B"], seed=c["seed"], keep_samples=True,
                       spin_yield_playouts=c["spin"], min_launch_rows=16, max_launch_wait_us=2000, cache=cache)
    r.start()
    r.wait_rows(6000, timeout_s=60)
    info = r.update_network(to_blob(random_weights(desc, 7922)))
    s1 = r.cache_stats()
    r.wait_rows(r.stats()["rows"] + 6000, timeout_s=60)
    r.stop()
    s2, st = r.cache_stats(), r.stats()
    r.close()
    print("roll %s\nrunner %s\ncache at the roll %s\ncache at the end %s" % (info, st, s1, s2))
    assert info["launches_before"] > 0 and st["rows"] >= 12000 and s2["rows"] == st["rows"]
    assert s1["hits"] > 0 and s2["hits"] > s1["hits"] and s2["flushes"] >= 1
    assert s2["rows"] == s2["hits"] + s2["forward_rows"]
    cache.close()
    net.close()


def test_runner_refusals(hip_device, monkeypatch):
    from galvanise_zero_amd.runner import SelfPlayRunner
    from test_nn_symmetry_pick_gpu import _runner_conf, _runner_net, game_tables
    T, _, _ = game_tables("breakthrough")
    setup, desc, net = _runner_net(hip_device)
    other = make_net(desc, hip_device, "bf16")
    cache, foreign, sym = net.make_cache(64), other.make_cache(64), net.make_symmetry(T)

    def runner(**kw):
        return SelfPlayRunner(net, setup.sm, setup.transformer, _runner_conf(), device=hip_device, num_threads=1,
                              pools_per_thread=2, batch_size=8, seed=1, spin_yield_playouts=1000, **kw)
    with pytest.raises(RuntimeError, match=r"gz_runner_set_cache: eval cache: made for another net"):
        runner(cache=foreign)
    with pytest.raises(RuntimeError, match=r"gz_runner_set_cache: runner: gz_runner_set_cache on a runner with a symmetry"):
        runner(symmetry=sym, cache=cache)
    r = runner(cache=cache)
    with pytest.raises(RuntimeError, match=r"gz_runner_set_symmetry: runner: gz_runner_set_symmetry on a runner with an evaluation cache"):
        r.set_symmetry(sym, 0)
    r.close()
    r = runner()
    r.start()
    with pytest.raises(RuntimeError, match=r"gz_runner_set_cache: runner: gz_runner_set_cache after gz_runner_start"):
        r.set_cache(cache)
    r.wait_rows(64, timeout_s=60)
    r.stop()
    assert r.cache_stats() is None and cache.stats()["rows"] == 0
    r.close()
    monkeypatch.setenv("GZ_RUNNER_ZERO_COPY", "1")
    with pytest.raises(RuntimeError, match=r"gz_runner_set_cache: runner: gz_runner_set_cache on a zero-copy runner"):
        runner(cache=cache)
    monkeypatch.delenv("GZ_RUNNER_ZERO_COPY")
    sym.close()
    for c in (cache, foreign):
        c.close()
    other.close()
    net.close()
