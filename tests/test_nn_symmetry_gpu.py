"""GPU tests of the symmetry ensemble (gz_net_forward_sym / gz_net_forward_sym_device,
csrc/nn/symmetry.hip): the forward averaged over the S <= 8 elements of a board's symmetry group.

The forward is batch-invariant, so the ensemble is specified bit for bit: permute the planes in numpy,
run the plain forward on each permuted batch, gather through the move tables, add in element order and
scale, all in float32 -- `restate` below.  Only S that is no power of two divides instead of scaling
exactly, and is allowed 1 ulp."""
import os
import subprocess
import sys

import numpy as np
import pytest

from galvanise_zero_amd.defs import confs, templates
from galvanise_zero_amd.nn.desc import BASELINE_CONFIGS, NetDesc
from galvanise_zero_amd.nn.weights import random_planes, random_weights, to_blob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V2_GAMMA = 0.3   # (tests/test_nn_v2_gpu.py: damps the v2 stream's growth)
NETS = {
    "8x8": (NetDesc(5, 8, 8, 64, 2, [155, 155]), {}),
    "13x13_v2_se": (NetDesc(5, 13, 13, 64, 1, [170, 171], resnet_v2=True, se_units=21), {"res_gamma": V2_GAMMA}),
    "10x10_amazons": (NetDesc(12, 10, 10, 64, 1, [3041, 3041]), {}),
}


class Tables(object):
    def __init__(self, plane_src, move_src):
        self.plane_src, self.move_src = plane_src, move_src


def random_tables(desc, S, seed, identity_first=False):
    """Arbitrary permutations: the kernels do not care that real tables are geometric."""
    rng = np.random.default_rng(seed)
    E = desc.input_channels * desc.input_columns * desc.input_rows

    def perms(n):
        return np.array([np.arange(n) if (identity_first and s == 0) else rng.permutation(n) for s in range(S)], dtype=np.int32)
    return Tables(perms(E), [perms(p) for p in desc.policy_dist_count])


def make_net(name, device, precision, seed=7919):
    from galvanise_zero_amd._native import HipNet
    desc, kw = NETS[name]
    net = HipNet(desc, device, precision)
    net.set_weights(to_blob(random_weights(desc, seed, bias_std=0.2, **kw)))
    return desc, net


def restate(net, x, tables):
    """The ensemble from plain forwards, in np.float32 and the kernel's order."""
    S, n = tables.plane_src.shape[0], x.shape[0]
    flat = x.reshape(n, -1)
    outs = [net.forward(np.ascontiguousarray(flat[:, tables.plane_src[s]]).reshape(x.shape)) for s in range(S)]
    res = []
    for k in range(len(outs[0])):
        def term(s):
            return outs[s][k][:, tables.move_src[k][s]] if k < len(tables.move_src) else outs[s][k]
        acc = term(0).astype(np.float32)
        for s in range(1, S):
            acc = (acc + term(s)).astype(np.float32)
        if S & (S - 1) == 0:
            res.append((acc * np.float32(1.0 / S)).astype(np.float32))
        else:
            res.append((acc / np.float32(S)).astype(np.float32))
    return res


def assert_bits(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype == np.float32 and g.shape == w.shape
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (what, k, float(np.abs(g - w).max()))


@pytest.mark.parametrize("n", [1, 37])
def test_identity_is_the_plain_forward(n, hip_device):
    desc, net = make_net("8x8", hip_device, "bf16x3")
    x = random_planes(desc, n, 100 + n)
    sym = net.make_symmetry(random_tables(desc, 1, 1, identity_first=True))
    assert_bits(net.forward(x, symmetry=sym), net.forward(x), ("identity", n))
    sym.close()
    net.close()


@pytest.mark.parametrize("n", [1, 37])
def test_eight_elements_bit_exact(n, hip_device):
    desc, net = make_net("8x8", hip_device, "bf16x3")
    x = random_planes(desc, n, 200 + n)
    tables = random_tables(desc, 8, 2)
    sym = net.make_symmetry(tables)
    got = net.forward(x, symmetry=sym)
    assert_bits(got, restate(net, x, tables), ("S=8", n))
    for g in got:
        np.testing.assert_allclose(g.sum(axis=1), 1.0, atol=1e-4)
    sym.close()
    net.close()


def test_non_finite_values_propagate(hip_device):
    """A NaN bias in role 0's policy Dense makes the plain forward's role-0 policies non-finite: the
    ensemble's are NaN wherever the restatement's are, and role 1 and the values keep their bits."""
    from galvanise_zero_amd._native import HipNet
    desc = NETS["8x8"][0]
    w = [(name, a.copy()) for name, a in random_weights(desc, 7919, bias_std=0.2)]
    dict(w)["policy0_bias"][7] = np.nan
    net = HipNet(desc, hip_device, "bf16x3")
    net.set_weights(to_blob(w))
    x = random_planes(desc, 3, 903)
    tables = random_tables(desc, 8, 9)
    sym = net.make_symmetry(tables)
    got, want = net.forward(x, symmetry=sym), restate(net, x, tables)
    print("NaN elements per output, restatement:", [int(np.isnan(a).sum()) for a in want], "ensemble:",
          [int(np.isnan(a).sum()) for a in got])
    assert np.isnan(want[0]).any() and np.isfinite(want[1]).all() and np.isfinite(want[2]).all()
    for g, r in zip(got, want):
        assert np.array_equal(np.isnan(g), np.isnan(r))
        assert np.array_equal(g[~np.isnan(r)].view(np.uint32), r[~np.isnan(r)].view(np.uint32))
    sym.close()
    net.close()


def test_two_elements_v2_fp32_ieee_bit_exact(hip_device):
    desc, net = make_net("13x13_v2_se", hip_device, "fp32-ieee")
    x = random_planes(desc, 3, 303)
    tables = random_tables(desc, 2, 3)
    sym = net.make_symmetry(tables)
    assert_bits(net.forward(x, symmetry=sym), restate(net, x, tables), "S=2 v2 fp32-ieee")
    sym.close()
    net.close()


def test_three_elements_within_one_ulp(hip_device):
    """S = 3 divides by 3 instead of scaling by a power of two: at most 1 ulp from the restatement."""
    desc, net = make_net("10x10_amazons", hip_device, "bf16")
    x = random_planes(desc, 5, 405)
    tables = random_tables(desc, 3, 4)
    sym = net.make_symmetry(tables)
    got, want = net.forward(x, symmetry=sym), restate(net, x, tables)
    for k, (g, w) in enumerate(zip(got, want)):
        ulps = np.abs(g.astype(np.float64) - w.astype(np.float64)) / np.spacing(np.abs(w)).astype(np.float64)
        print("S=3 output %d: max %.3g ulp" % (k, ulps.max()))
        assert ulps.max() <= 1.0, (k, ulps.max())
    sym.close()
    net.close()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_nn_symmetry_gpu as T
desc, net = T.make_net("8x8", 0, "bf16x3")
x = T.random_planes(desc, 5, 505)
sym = net.make_symmetry(T.random_tables(desc, 8, 5))
np.savez(sys.argv[2], *net.forward(x, symmetry=sym))
"""


def test_chunking_keeps_the_bits(hip_device, tmp_path):
    """GZ_SYM_CHUNK_ROWS=2 in a fresh child process: 5 rows in chunks of 2, 2 and 1."""
    desc, net = make_net("8x8", hip_device, "bf16x3")
    x = random_planes(desc, 5, 505)
    sym = net.make_symmetry(random_tables(desc, 8, 5))
    assert "GZ_SYM_CHUNK_ROWS" not in os.environ
    want = net.forward(x, symmetry=sym)
    out = str(tmp_path / "chunked.npz")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], check=True, env=dict(os.environ, GZ_SYM_CHUNK_ROWS="2"),
                   timeout=120)
    with np.load(out) as z:
        assert_bits([z["arr_%d" % k] for k in range(len(want))], want, "chunks of 2")
    sym.close()
    net.close()


def _positions(sm, t, seed, count=4, stride=3):
    """Planes of `count` positions of a seeded random playout, each with its previous state."""
    import random
    from galvanise_zero_amd.cppinterface import create_c_transformer
    ct = create_c_transformer(t)
    rng = random.Random(seed)
    s, prev, planes = sm.get_initial_state().copy(), None, []
    for ply in range(1, count * stride + 1):
        sm.update_bases(s)
        assert not sm.is_terminal()
        jm = [rng.choice(sm.get_legal_state(r)) for r in range(sm.role_count)]
        s, prev = sm.next_state(jm).copy(), s
        if ply % stride == 0:
            planes.append(ct.to_channels(s, [prev]))
    return np.array(planes, dtype=np.float32)


@pytest.mark.parametrize("precision", ["bf16x3", "fp32-ieee"])
@pytest.mark.parametrize("game,S", [("reversi", 8), ("hexLG13", 2)])
def test_equivariance_with_the_games_tables(game, S, precision, hip_device):
    """Builder and kernels together: the ensemble of a mapped position, read through move_src, is the
    ensemble of the original within 1e-6 absolute -- the two sides add the same S <= 8 bit-identical
    terms, each <= 1, in another order, so they differ by at most 7 roundings of a sum <= 8, 7 * 2^-21
    before the division by 8: 4.2e-7.  The plain forward is not equivariant: it must differ by more
    on at least one pair, or this test would show nothing."""
    from galvanise_zero_amd._native import HipNet
    from galvanise_zero_amd.util import symmetry
    tables, sm, t = symmetry.tables_for_game(game)
    assert tables.count == S
    desc = NetDesc(t.num_channels, t.num_cols, t.num_rows, 64, 2, list(t.policy_dist_count))
    net = HipNet(desc, hip_device, precision)
    net.set_weights(to_blob(random_weights(desc, 7919, bias_std=0.2)))
    sym = net.make_symmetry(tables)
    X = _positions(sm, t, seed=20251020)
    n = X.shape[0]
    shape = (-1, desc.input_channels, desc.input_columns, desc.input_rows)
    ens, plain = net.forward(X.reshape(shape), symmetry=sym), net.forward(X.reshape(shape))
    worst_ens = worst_plain = 0.0
    for e in range(1, S):
        Xe = np.ascontiguousarray(X[:, tables.plane_src[e]]).reshape(shape)
        ens_e, plain_e = net.forward(Xe, symmetry=sym), net.forward(Xe)
        for r in range(sm.role_count):
            worst_ens = max(worst_ens, float(np.abs(ens_e[r][:, tables.move_src[r][e]] - ens[r]).max()))
            worst_plain = max(worst_plain, float(np.abs(plain_e[r][:, tables.move_src[r][e]] - plain[r]).max()))
        worst_ens = max(worst_ens, float(np.abs(ens_e[-1] - ens[-1]).max()))
        worst_plain = max(worst_plain, float(np.abs(plain_e[-1] - plain[-1]).max()))
    print("%s %s, %d positions x %d elements: ensemble max |d| %.3g, plain forward %.3g" % (game, precision, n, S - 1, worst_ens, worst_plain))
    assert worst_ens <= 1e-6
    assert worst_plain > 1e-6
    sym.close()
    net.close()


def test_device_variant_equals_host_variant(hip_device):
    import torch
    desc, net = make_net("8x8", hip_device, "bf16x3")
    n = 37
    x = random_planes(desc, n, 637)
    sym = net.make_symmetry(random_tables(desc, 8, 6))
    want = net.forward(x, symmetry=sym)
    dev = torch.device("cuda", hip_device)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        d_x = torch.from_numpy(x).to(dev)
        d_pol = [torch.full((n, p), -1.0, dtype=torch.float32, device=dev) for p in desc.policy_dist_count]
        d_val = torch.full((n, desc.num_values), -1.0, dtype=torch.float32, device=dev)
        net.forward_sym_device(sym, stream.cuda_stream, d_x.data_ptr(), n, [p.data_ptr() for p in d_pol], d_val.data_ptr())
    stream.synchronize()
    assert_bits([p.cpu().numpy() for p in d_pol] + [d_val.cpu().numpy()], want, "device variant")
    sym.close()
    net.close()


def test_refusals_leave_the_net_alone(hip_device):
    desc, net = make_net("8x8", hip_device, "bf16x3")
    x = random_planes(desc, 3, 703)
    before = net.forward(x)
    sym = net.make_symmetry(random_tables(desc, 2, 7))
    net.set_output_logits(True)
    with pytest.raises(RuntimeError, match=r"failed: symmetry: .*logits"):
        net.forward(x, symmetry=sym)
    net.set_output_logits(False)
    for other in (NetDesc(5, 6, 6, 64, 2, [155, 155]), NetDesc(5, 8, 8, 64, 2, [155, 65]), NetDesc(5, 8, 8, 64, 2, [155])):
        wrong = net.make_symmetry(random_tables(other, 2, 8))
        with pytest.raises(RuntimeError, match=r"failed: symmetry: tables of plane_elems .* are not the net's"):
            net.forward(x, symmetry=wrong)
        wrong.close()
    assert_bits(net.forward(x), before, "plain forward after the refusals")
    assert_bits(net.forward(x, symmetry=sym), restate(net, x, Tables(sym.plane_src, sym.move_src)), "ensemble after the refusals")
    sym.close()
    net.close()


def test_through_model_and_player(hip_device):
    """HipModel(symmetries=...): predict_on_batch is HipNet.forward(X, symmetry=...); a PUCTPlayer on
    such a model (breakthroughSmall, 50 evaluations) returns a legal move, and the same root visits
    on a second run."""
    from galvanise_zero_amd._native import HipNet
    from galvanise_zero_amd.nn.network import HipModel, NeuralNetwork
    from galvanise_zero_amd.player.puctplayer import Match, PUCTPlayer
    from galvanise_zero_amd.util import symmetry
    game = "breakthroughSmall"
    tables, sm, t = symmetry.tables_for_game(game)
    desc = BASELINE_CONFIGS[1]["desc"]
    w = random_weights(desc, 5)
    model = HipModel(desc, w, hip_device, "bf16x3", symmetries=tables)
    net = HipNet(desc, hip_device, "bf16x3")
    net.set_weights(to_blob(w))
    sym = net.make_symmetry(tables)
    x = random_planes(desc, 9, 809)
    got = model.predict_on_batch(x)
    assert_bits(got, net.forward(x, symmetry=sym), "HipModel.predict_on_batch")
    assert any(not np.array_equal(g, p) for g, p in zip(got, net.forward(x)))
    sym.close()
    net.close()

    def run():
        ev = templates.base_puct_config(batch_size=32, choose="choose_temperature", dirichlet_noise_pct=0.25,
                                        think_time=-1, converged_visits=1)
        conf = confs.PUCTPlayerConfig(name="sym", playouts_per_iteration=50, generation="test", evaluator_config=ev)
        player = PUCTPlayer(conf, nn=NeuralNetwork(t, model, None), seed=11)
        player.match = Match(game, 0)
        player.on_meta_gaming(-1)
        move = player.on_next_move()
        return move, player.poller.c_player.root_children()

    move, children = run()
    sm.update_bases(sm.get_initial_state())
    assert move in sm.get_legal_state(0)
    assert sum(v for _, v, _ in children) >= 50 - 32
    assert run() == (move, children)
