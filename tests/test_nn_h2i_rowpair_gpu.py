"""The row-pair geometry of the in-place split kernel at 8 x 8 (trunk_kernel_h2i<128, 4, 3>,
csrc/nn/rowpair.h): a position tile holds one board row of each of a workgroup's two boards, so a row of
a launch shares its MFMA tiles with its neighbour.  A row's outputs must not depend on that neighbour:
any permutation of a launch permutes its outputs, and a row forwarded alone (a dead partner) equals
its paired result, bit for bit; uneven segment cuts match variant 23.  Boards of four position tiles
that are not 8 x 8 keep the in-place kernel with a board per wave group, as trunk_kernel_h2ig."""
import numpy as np
import pytest

from galvanise_zero_amd.nn.desc import NetDesc
from galvanise_zero_amd.nn.weights import random_planes, random_weights, to_blob
from test_bench_shape_gpu import _segmented_forward
from test_nn_h2i_gpu import H2I, _variant_net

pytestmark = pytest.mark.gpu

H2IG = "gznn::trunk_kernel_h2ig<128, 4, 3>"
NETS = {"12x2": NetDesc(12, 8, 8, 128, 2, [155, 155]), "5x1": NetDesc(5, 8, 8, 128, 1, [155, 155])}
PERMS = ([6, 5, 4, 3, 2, 1, 0], [1, 0, 3, 2, 5, 4, 6], [3, 6, 0, 4, 1, 5, 2])


def _rows(desc):
    """6 random rows and an all-zero board."""
    x = random_planes(desc, 7, 21)
    x[6] = 0.0
    return x


@pytest.mark.parametrize("name", list(NETS))
def test_partner_independence(name, hip_device, monkeypatch):
    desc = NETS[name]
    net = _variant_net(monkeypatch, desc, to_blob(random_weights(desc, 9, bias_std=0.2)), "25", hip_device)
    assert net.kernel_name(True) == H2I % 4
    x = _rows(desc)
    base = net.forward(x)
    for perm in PERMS:
        got = net.forward(np.ascontiguousarray(x[perm]))
        for i, (g, b) in enumerate(zip(got, base)):
            assert np.array_equal(g, b[perm]), (name, perm, i)
    for r in range(x.shape[0]):   # alone: the workgroup's second board is dead
        got = net.forward(np.ascontiguousarray(x[r:r + 1]))
        for i, (g, b) in enumerate(zip(got, base)):
            assert np.array_equal(g[0], b[r]), (name, r, i)
    net.close()


@pytest.mark.parametrize("name", list(NETS))
def test_odd_segment_cuts_identical_to_variant_23(name, hip_device, monkeypatch):
    """5 rows in segments of 1, 3 and 1: every workgroup's two boards come from different segments or
    the second is dead."""
    desc = NETS[name]
    w = to_blob(random_weights(desc, 9, bias_std=0.2))
    x = _rows(desc)[:5]
    sizes = [1, 3, 1]
    ref_net = _variant_net(monkeypatch, desc, w, "23", hip_device)
    ref = _segmented_forward(ref_net, desc, x, sizes)
    ref_net.close()
    net = _variant_net(monkeypatch, desc, w, "25", hip_device)
    assert net.kernel_name(True) == H2I % 4
    got = _segmented_forward(net, desc, x, sizes)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g, r), (name, i)
    net.close()


@pytest.mark.parametrize("blocks", [0, 2])
@pytest.mark.parametrize("board", [(7, 7), (7, 8), (8, 7)])
def test_other_four_tile_boards_keep_a_board_per_group(board, blocks, hip_device, monkeypatch):
    h, w_ = board
    desc = NetDesc(12, h, w_, 128, blocks, [99, 98])
    w = to_blob(random_weights(desc, 5, bias_std=0.2))
    x = random_planes(desc, 3, 4)
    default = _variant_net(monkeypatch, desc, w, None, hip_device)
    assert default.kernel_name(True) == H2IG
    assert default.workgroups_per_cu() == 2
    assert default.wave_rows() == 1024
    default.close()
    nets = {v: _variant_net(monkeypatch, desc, w, v, hip_device) for v in ("21", "23", "25")}
    assert nets["25"].kernel_name(True) == H2IG
    assert nets["25"].workgroups_per_cu() == 2
    for n in (1, 2, 3):
        outs = {v: net.forward(x[:n]) for v, net in nets.items()}
        for ref in ("21", "23"):
            for a, b in zip(outs[ref], outs["25"]):
                assert np.array_equal(a, b), (board, blocks, n, ref)
    for net in nets.values():
        net.close()
