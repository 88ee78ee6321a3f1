"""GPU tests of one symmetry per row, picked on the GPU from the row's own planes
(gz_net_forward_sym_pick / _device, gz_symmetry_picks, gz_runner_set_symmetry; csrc/nn/symmetry.hip
sym_pick_expand_kernel / sym_pick_gather_kernel).

The definition adds no floating-point operation, so everything here is bit for bit: the kernel's picks
against numpy (util.symmetry.pick_elements), a picked row against the plain forward of its permuted
planes read through the move table (util.symmetry.pick_forward), a row against itself in any batch and
through any entry point, the self-play runner against the oracle fed by the same pick forward, and a
PUCTPlayer against the oracle player."""
import os
import subprocess
import sys

import numpy as np
import pytest

from galvanise_zero_amd.defs import confs, templates
from galvanise_zero_amd.nn.desc import NetDesc
from galvanise_zero_amd.nn.weights import random_weights, to_blob
from galvanise_zero_amd.util import symmetry
from puct_harness import Setup, sample_key
from test_nn_symmetry_gpu import Tables, assert_bits, random_tables
from test_runner_fp32_gpu import _oracle_conf, _suffix

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["bf16", "bf16x3", "fp32-ieee", "bf16-layered", "bf16x3-layered", "fp16x3-layered"]
SALTS = [0, 0xFFFFFFFF]

_cache = {}


def game_tables(game):
    if game not in _cache:
        _cache[game] = symmetry.tables_for_game(game)
    return _cache[game]


def net_case(name):
    """(desc, tables): breakthrough's reflection (S = 2) and reversi's group (S = 8, three values) on
    1-block 64-filter 8 x 8 nets, and arbitrary permutations (S = 3) on a 5 x 5 net."""
    if name == "breakthrough":
        T, _, t = game_tables("breakthrough")
        desc = NetDesc(t.num_channels, t.num_cols, t.num_rows, 64, 1, list(t.policy_dist_count))
        assert T.count == 2 and T.plane_src.shape[1] == 320
    elif name == "reversi":
        T, _, t = game_tables("reversi")
        desc = NetDesc(t.num_channels, t.num_cols, t.num_rows, 64, 1, list(t.policy_dist_count), num_values=3)
        assert T.count == 8 and (desc.input_columns, desc.input_rows) == (8, 8)
    else:
        desc = NetDesc(3, 5, 5, 64, 1, [26, 31])
        T = random_tables(desc, 3, 41)
        assert T.plane_src.shape == (3, 75)
    return desc, T


def make_net(desc, device, precision, seed=7919):
    from galvanise_zero_amd._native import HipNet
    net = HipNet(desc, device, precision)
    net.set_weights(to_blob(random_weights(desc, seed, bias_std=0.2)))
    return net


def board_planes(desc, n, seed):
    """0/1 planes (what a game's planes are), every row distinct."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2, (n, desc.input_channels, desc.input_columns, desc.input_rows)).astype(np.float32)


# ---- picks -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(5, 8, 8), (3, 5, 5)])
def test_picks_equal_numpy(shape, hip_device):
    """gz_symmetry_picks (the kernel's hash: 16-byte loads on the aligned rows of E = 320, the scalar
    loop on E = 75, whose rows are not 16-byte aligned) against numpy: n in {1, 3, 257}, S in
    {1, 2, 3, 8}, both salts, host and device pointers; a NaN pattern and -0.0 among the rows."""
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
            sym = net.make_symmetry(random_tables(desc, S, 100 + S))
            for salt in SALTS:
                want = symmetry.pick_elements(x, S, salt)
                assert want.min() >= 0 and want.max() < S
                assert np.array_equal(net.symmetry_picks(sym, salt, planes=x), want), (n, S, salt, "host")
                assert np.array_equal(net.symmetry_picks(sym, salt, device_ptr=d_x.data_ptr(), n=n), want), (n, S, salt, "device")
            sym.close()
    net.close()


# ---- exactness ---------------------------------------------------------------------------------------

EXACT = [("breakthrough", m) for m in MODES] + [(c, m) for c in ("reversi", "5x5") for m in ("bf16x3", "fp16x3-layered")]


@pytest.mark.parametrize("case,precision", EXACT)
def test_pick_forward_bit_exact(case, precision, hip_device):
    """forward(X, symmetry, pick=salt) is the plain forward of each row's permuted planes read through
    move_src[g], values untouched: n in {1, 5, 300} (300 crosses the two-boards-per-workgroup
    threshold), both salts."""
    desc, T = net_case(case)
    net = make_net(desc, hip_device, precision)
    sym = net.make_symmetry(T)
    for n in (1, 5, 300):
        x = board_planes(desc, n, 7 * n + len(case))
        for salt in SALTS:
            got = net.forward(x, symmetry=sym, pick=salt)
            assert_bits(got, symmetry.pick_forward(net.forward, x, T, salt), (case, precision, n, salt))
        if n == 300:
            # row by row, as the definition states it
            S = T.plane_src.shape[0]
            g = symmetry.pick_elements(x, S, SALTS[1])
            assert len(set(g.tolist())) == S                # every element met
            for r in (0, 149, 299):
                xr = np.ascontiguousarray(x[r].reshape(-1)[T.plane_src[g[r]]]).reshape((1,) + x.shape[1:])
                plain = net.forward(xr)
                for k in range(len(T.move_src)):
                    assert np.array_equal(got[k][r], plain[k][0][T.move_src[k][g[r]]])
                assert np.array_equal(got[-1][r], plain[-1][0])
    sym.close()
    net.close()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_nn_symmetry_pick_gpu as T
desc, tables = T.net_case("breakthrough")
net = T.make_net(desc, 0, "bf16x3")
sym = net.make_symmetry(tables)
np.savez(sys.argv[2], *net.forward(T.board_planes(desc, 5, 505), symmetry=sym, pick=12345))
"""


def test_chunking_keeps_the_bits(hip_device, tmp_path):
    """GZ_SYM_CHUNK_ROWS=2 in a fresh child process: 5 rows in chunks of 2, 2 and 1."""
    desc, T = net_case("breakthrough")
    net = make_net(desc, hip_device, "bf16x3")
    sym = net.make_symmetry(T)
    assert "GZ_SYM_CHUNK_ROWS" not in os.environ
    want = net.forward(board_planes(desc, 5, 505), symmetry=sym, pick=12345)
    out = str(tmp_path / "chunked.npz")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], check=True, env=dict(os.environ, GZ_SYM_CHUNK_ROWS="2"),
                   timeout=120)
    with np.load(out) as z:
        assert_bits([z["arr_%d" % k] for k in range(len(want))], want, "chunks of 2")
    sym.close()
    net.close()


def test_logits_mode_is_served(hip_device):
    """A permutation of logits is well defined (nothing is averaged): the pick forward serves a net in
    gz_net_set_output_logits mode, bit for bit the permuted plain logits; the ensemble still refuses."""
    desc, T = net_case("reversi")
    net = make_net(desc, hip_device, "bf16x3")
    sym = net.make_symmetry(T)
    x = board_planes(desc, 37, 37)
    net.set_output_logits(True)
    got = net.forward(x, symmetry=sym, pick=3)
    assert_bits(got, symmetry.pick_forward(net.forward, x, T, 3), "logits")
    assert float(np.abs(got[0].sum(axis=1) - 1.0).min()) > 1e-3      # logits, not probabilities
    with pytest.raises(RuntimeError, match=r"failed: symmetry: .*logits"):
        net.forward(x, symmetry=sym)
    net.set_output_logits(False)
    sym.close()
    net.close()


# ---- invariance --------------------------------------------------------------------------------------

def test_a_rows_result_is_its_own(hip_device):
    """One row alone, first, last and in the middle of a batch; through the host entry point, the
    device entry point and HipModel.predict_on_batch; S = 1 tables are the plain forward; among 64 rows
    at least one gets g != 0 and then differs from the plain forward (the path is live)."""
    import torch
    from galvanise_zero_amd.nn.network import HipModel
    desc, T = net_case("reversi")
    w = random_weights(desc, 7919, bias_std=0.2)
    model = HipModel(desc, w, hip_device, "bf16x3", symmetries=T, symmetry_mode="pick", symmetry_salt=99)
    net, sym = model.net, model.symmetry
    x = board_planes(desc, 64, 64)
    full = net.forward(x, symmetry=sym, pick=99)
    for where, batch, at in [("alone", x[17:18], 0), ("first", x[17:40], 0), ("last", x[:18], 17), ("middle", x[10:30], 7)]:
        got = net.forward(np.ascontiguousarray(batch), symmetry=sym, pick=99)
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
        net.forward_sym_pick_device(sym, 99, stream.cuda_stream, d_x.data_ptr(), n, [p.data_ptr() for p in d_pol], d_val.data_ptr())
    stream.synchronize()
    assert_bits([p.cpu().numpy() for p in d_pol] + [d_val.cpu().numpy()], full, "device entry point")

    plain = net.forward(x)
    g = symmetry.pick_elements(x, T.count, 99)
    assert (g != 0).any()
    moved = [r for r in range(n) if g[r] != 0 and any(not np.array_equal(full[k][r], plain[k][r]) for k in range(len(full)))]
    assert moved, "no row with g != 0 differs from the plain forward"
    for r in np.flatnonzero(g == 0):
        assert all(np.array_equal(full[k][r], plain[k][r]) for k in range(len(full)))
    one = net.make_symmetry(Tables(T.plane_src[:1], [m[:1] for m in T.move_src]))
    assert_bits(net.forward(x, symmetry=one, pick=99), plain, "S = 1")
    one.close()


def test_refusals_leave_the_net_alone(hip_device):
    desc, T = net_case("breakthrough")
    net = make_net(desc, hip_device, "bf16x3")
    x = board_planes(desc, 3, 703)
    before = net.forward(x)
    for other in (NetDesc(5, 6, 6, 64, 1, list(desc.policy_dist_count)), NetDesc(5, 8, 8, 64, 1, [desc.policy_dist_count[0], 65])):
        wrong = net.make_symmetry(random_tables(other, 2, 8))
        with pytest.raises(RuntimeError, match=r"failed: symmetry: tables of plane_elems .* are not the net's"):
            net.forward(x, symmetry=wrong, pick=0)
        wrong.close()
    from galvanise_zero_amd._native import HipSymmetry
    elsewhere = HipSymmetry(T.plane_src, T.move_src, device=hip_device + 1)
    with pytest.raises(RuntimeError, match=r"failed: symmetry: tables made for device %d, the net is on device %d" % (hip_device + 1, hip_device)):
        net.forward(x, symmetry=elsewhere, pick=0)
    elsewhere.close()
    with pytest.raises(ValueError, match="needs symmetry="):
        net.forward(x, pick=0)
    assert_bits(net.forward(x), before, "plain forward after the refusals")
    net.close()


# ---- runner ------------------------------------------------------------------------------------------

RUNNER = dict(seed=20251021, threads=1, ppt=2, B=8, spin=1000, rows=2 * 8 * 1500)


def _runner_conf():
    conf = templates.selfplay_config_template()
    conf.evals_per_move = 4
    conf.run_to_end_evals = 2
    return conf


def _runner_net(hip_device, shadow=False):
    from galvanise_zero_amd._native import HipNet
    setup = Setup("breakthrough")
    t = setup.transformer
    desc = NetDesc(t.num_channels, t.num_cols, t.num_rows, 64, 1, list(t.policy_dist_count), num_values=t.num_rewards)
    net = HipNet(desc, hip_device, "bf16x3")
    if shadow:
        net.enable_shadow("fp32-ieee", every=4, max_rows=8)
    net.set_weights(to_blob(random_weights(desc, 7921)))
    return setup, desc, net


def _run(hip_device, tables, salt=None):
    """One runner run (breakthrough, 1 thread x 2 pools x 8 games, 4 evaluations per move): the samples
    per pool, the stats and the pick-rows counter."""
    from galvanise_zero_amd.runner import SelfPlayRunner
    key = ("run", None if tables is None else tables.plane_src.shape[0], salt)
    if key in _cache:
        return _cache[key]
    setup, desc, net = _runner_net(hip_device)
    sym = net.make_symmetry(tables) if tables is not None else None
    c = RUNNER
    r = SelfPlayRunner(net, setup.sm, setup.transformer, _runner_conf(), device=hip_device, num_threads=c["threads"],
                       pools_per_thread=c["ppt"], batch_size=c["B"], seed=c["seed"], keep_samples=True,
                       spin_yield_playouts=c["spin"], min_launch_rows=16, max_launch_wait_us=2000, symmetry=sym,
                       symmetry_salt=salt)
    assert r.symmetry_salt == (None if sym is None else (c["seed"] & 0xFFFFFFFF if salt is None else salt))
    r.start()
    r.wait_rows(c["rows"], timeout_s=120)
    r.stop()
    st, picked = r.stats(), r.sym_pick_rows()
    by_pool = {}
    for s in r.fetch_samples():
        by_pool.setdefault(int(s["match_identifier"].split("_")[1][1:]), []).append(s)    # gpu<d>_p<i>_<slot>_<count>
    r.close()
    if sym is not None:
        sym.close()
    net.close()
    print("runner, tables %s: stats %s, pick rows %d, samples per pool %s" % (key[1], st, picked, {p: len(v) for p, v in by_pool.items()}))
    _cache[key] = (setup, by_pool, st, picked)
    return _cache[key]


def _keys(setup, samples):
    return [sample_key(setup, _suffix(s), True) for s in samples]


@pytest.mark.timeout(300)
def test_runner_identity_tables_change_nothing(hip_device):
    """S = 1 tables: every sample equals, field for field, the sample of a runner without a symmetry on
    the same seed (each pool is deterministic; a run's last samples depend on when it stopped, so the
    pools' common prefixes are compared), while every row went through the pick path."""
    T, _, _ = game_tables("breakthrough")
    one = Tables(T.plane_src[:1], [m[:1] for m in T.move_src])
    setup, plain, st0, picked0 = _run(hip_device, None)
    _, same, st1, picked1 = _run(hip_device, one)
    assert picked0 == 0 and picked1 == st1["rows"] >= RUNNER["rows"]
    compared = 0
    for pool in range(RUNNER["ppt"]):
        n = min(len(plain.get(pool, [])), len(same.get(pool, [])))
        assert _keys(setup, plain.get(pool, [])[:n]) == _keys(setup, same.get(pool, [])[:n]), pool
        compared += n
    assert compared >= 8, compared


@pytest.mark.timeout(600)
def test_runner_reflection_matches_oracle(hip_device):
    """Breakthrough's reflection in pick mode, salt = the seed: the counter equals the rows evaluated,
    the samples differ from the plain run's, and one pool (the one with the most samples) replayed
    through oracle.puct_ref.Manager with the predictions of net.forward(x, symmetry, pick=salt) gives
    every runner sample of that pool."""
    from oracle import puct_ref as P
    T, _, _ = game_tables("breakthrough")
    c = RUNNER
    setup, plain, _, _ = _run(hip_device, None)
    _, got, st, picked = _run(hip_device, T)
    assert picked == st["rows"] >= c["rows"]
    differs = False
    for pool in range(c["ppt"]):
        n = min(len(plain.get(pool, [])), len(got.get(pool, [])))
        differs |= _keys(setup, plain.get(pool, [])[:n]) != _keys(setup, got.get(pool, [])[:n])
    assert differs, "the reflection changed no sample"

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
        outs = net.forward(x, symmetry=sym, pick=salt)
        pred = (x.shape[0], outs[:-1], outs[-1])
    n = len(mine)
    assert n >= 8 and len(man.samples) >= n, (n, len(man.samples))
    assert _keys(setup, mine) == [sample_key(setup, _suffix(s), False) for s in man.samples[:n]]
    print("%d samples of pool %d identical to the oracle on the pick forward" % (n, pool))
    sym.close()
    net.close()


@pytest.mark.timeout(300)
def test_runner_roll_and_shadow_with_a_symmetry(hip_device):
    """A generation roll mid-play and an fp32-ieee shadow, with the reflection set: the run completes,
    every row of both generations went through the pick path, and the shadow (which sees the permuted
    rows) has totals for both."""
    from galvanise_zero_amd.runner import SelfPlayRunner
    T, _, _ = game_tables("breakthrough")
    setup, desc, net = _runner_net(hip_device, shadow=True)
    sym = net.make_symmetry(T)
    c = RUNNER
    r = SelfPlayRunner(net, setup.sm, setup.transformer, _runner_conf(), device=hip_device, num_threads=c["threads"],
                       pools_per_thread=c["ppt"], batch_size=c["B"], seed=c["seed"], keep_samples=True,
                       spin_yield_playouts=c["spin"], min_launch_rows=16, max_launch_wait_us=2000, symmetry=sym)
    r.start()
    r.wait_rows(2000, timeout_s=60)
    st1 = r.shadow_stats()
    info = r.update_network(to_blob(random_weights(desc, 7922)))
    r.shadow_stats(reset=True)
    r.wait_rows(r.stats()["rows"] + 2000, timeout_s=60)
    r.stop()
    st2, st, picked = r.shadow_stats(), r.stats(), r.sym_pick_rows()
    r.close()
    print("roll %s\nrunner %s\nshadow, first generation %s\nshadow, second generation %s" % (info, st, st1, st2))
    assert info["launches_before"] > 0 and picked == st["rows"] >= 4000
    for s in (st1, st2):
        assert s["checks"] > 0 and 0 < s["rows"] <= 8 * s["checks"] and s["nonfinite_rows"] == 0, s
        assert s["policy_rows"] == 2 * s["rows"] and s["device_ms"] > 0.0 and s["max_abs_dp"] > 0.0, s
    sym.close()
    net.close()


def test_runner_refusals(hip_device, monkeypatch):
    from galvanise_zero_amd.runner import SelfPlayRunner
    T, _, _ = game_tables("breakthrough")
    setup, desc, net = _runner_net(hip_device)
    sym = net.make_symmetry(T)
    wrong = net.make_symmetry(random_tables(NetDesc(5, 6, 6, 64, 1, list(desc.policy_dist_count)), 2, 8))

    def runner(**kw):
        return SelfPlayRunner(net, setup.sm, setup.transformer, _runner_conf(), device=hip_device, num_threads=1,
                              pools_per_thread=2, batch_size=8, seed=1, spin_yield_playouts=1000, **kw)
    with pytest.raises(RuntimeError, match=r"gz_runner_set_symmetry: symmetry: tables of plane_elems .* are not the net's"):
        runner(symmetry=wrong)
    r = runner()
    r.start()
    with pytest.raises(RuntimeError, match=r"gz_runner_set_symmetry: runner: gz_runner_set_symmetry after gz_runner_start"):
        r.set_symmetry(sym, 0)
    r.wait_rows(64, timeout_s=60)
    r.stop()
    assert r.sym_pick_rows() == 0
    r.close()
    monkeypatch.setenv("GZ_RUNNER_ZERO_COPY", "1")
    with pytest.raises(RuntimeError, match=r"gz_runner_set_symmetry: runner: gz_runner_set_symmetry on a zero-copy runner"):
        runner(symmetry=sym)
    monkeypatch.delenv("GZ_RUNNER_ZERO_COPY")
    for s in (sym, wrong):
        s.close()
    net.close()


# ---- player ------------------------------------------------------------------------------------------

def test_player_on_the_pick_forward(hip_device):
    """PlayPoller at batch 32 against the oracle player, both fed by HipModel(symmetry_mode="pick")
    (tests/test_player_gpu.py's harness): planes at every poll, moves and root visits identical; then
    two PUCTPlayers on such models play a breakthroughSmall match to the end."""
    from galvanise_zero_amd.nn.network import HipModel, NeuralNetwork
    from galvanise_zero_amd.player.puctplayer import PUCTPlayer, play_match
    from test_player_gpu import _player_run
    game = "breakthroughSmall"
    T, _, _ = game_tables(game)
    setup = Setup(game)
    model = HipModel(setup.desc, setup.weights, hip_device, "bf16x3", symmetries=T, symmetry_mode="pick", symmetry_salt=17)
    d = setup.desc
    shape = (-1, d.input_channels, d.input_columns, d.input_rows)
    seen = []

    def nn(planes):
        x = np.asarray(planes, np.float32).reshape(shape)
        seen.append(symmetry.pick_elements(x, T.count, 17))
        return model.predict_on_batch(x)
    setup.nn = nn
    conf = templates.base_puct_config(batch_size=32, choose="choose_temperature", dirichlet_noise_pct=0.25,
                                      think_time=-1, converged_visits=1)
    visits = _player_run(setup, conf, 160, 3, seed=17)
    assert sum(t for _, t, _ in visits[0]) > 100
    assert (np.concatenate(seen) != 0).any()             # the search did meet reflected evaluations

    def player(batch, playouts, seed):
        ev = templates.base_puct_config(batch_size=batch, choose="choose_temperature", dirichlet_noise_pct=0.25,
                                        think_time=-1, converged_visits=1)
        pc = confs.PUCTPlayerConfig(name="pick%d" % batch, playouts_per_iteration=playouts, generation="test", evaluator_config=ev)
        m = HipModel(setup.desc, setup.weights, hip_device, "bf16x3", symmetries=T, symmetry_mode="pick", symmetry_salt=seed)
        return PUCTPlayer(pc, nn=NeuralNetwork(setup.transformer, m, None), seed=seed)
    goals, moves = play_match(game, [player(32, 100, 3), player(1, 32, 4)])
    assert sorted(goals) == [0, 100] and len(moves) > 5
