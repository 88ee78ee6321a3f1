"""CPU side of the exact suite (tests/test_nn_exact_gpu.py): every net of that file meets, for every
mode it is run in, the conditions under which exactness is a theorem (exact_lattice.
check_representable); the nets are alive; and the comparison would notice a wrong kernel -- each
kernel-like slip, applied to the oracle side alone, moves at least one expected logit.  For the
squeeze-excite nets that includes the saturation conditions (every gate exactly 0, 1/2 or 1), gates
that take all three values and differ between the boards of a launch, and the slips a squeeze-excite
kernel can make (exact_lattice.SE_FAULTS).  For the input-path nets (tests/test_nn_input_exact_gpu.py):
no (tap, plane) place of the initial conv can be removed without moving a logit of the first row
(exact_lattice.initial_liveness), and each slip of plane staging and im2col (exact_lattice.INPUT_FAULTS)
moves one.  For the dense-heads nets (HEAD_CASES): no output of a
launch is zero where an untouched buffer would pass, and each slip a heads kernel can make
(exact_lattice.HEAD_FAULTS) moves a logit wherever the net's geometry lets it occur.  No GPU."""
import dataclasses

import numpy as np
import pytest

import exact_lattice as xl
from galvanise_zero_amd.nn.desc import NetDesc
from oracle import nn_ref
from test_nn_exact_gpu import (ALL, CASES, CHUNKED, HEAD_CASES, HEAD_CHUNKED, HEAD_LARGE_VARIANTS, HEAD_NO_GEMM, HEAD_VARIED,
                               LARGE_ROWS, PROBABILITY, SAT, SATURATED, SCALES, SE_CASES, SE_VARIED, _softmax64, build, saturated)
from test_nn_input_exact_gpu import CASES as INPUT_CASES, EDGE_FITS, EDGE_OVER, FUSED, LARGE_ROWS as INPUT_LARGE_ROWS, LAYERED
from test_nn_input_exact_gpu import REFUSED as INPUT_REFUSED, build as input_build

FAMILIES = {c.family: name for name, c in CASES.items() if c.family}
GEOMETRY_FAULTS = ("tap_swap", "wrap_pad", "channel_swap", "drop_last_channel")
SE_FAMILIES = {c.family: name for name, c in SE_CASES.items()}


def _pow2_board(desc):
    return xl.sig_bits(float(desc.hw)) == 1


def _se_fault_applies(name, fault):
    """gate_block_slip needs a block 1; mean_one_count is for the boards on which the mean is exact
    (elsewhere a saturated gate cannot see a small error of the mean, by construction)."""
    desc = SE_CASES[name].desc
    return not (fault == "gate_block_slip" and desc.residual_layers < 2) and not (fault == "mean_one_count" and not _pow2_board(desc))


def _last_residual_conv(desc):
    return "res%d_conv%d" % (desc.residual_layers - 1, 2 if desc.resnet_v2 else 1)


def _differs(a, b):
    return any(not np.array_equal(p, q) for p, q in zip(a, b))


def test_exact_vars():
    """The three vars are found by search, and the float32 fold's var + 1e-3f is 1, 1/4 and 4 on them."""
    v = xl.exact_vars()
    assert sorted(v) == [0.25, 1.0, 4.0]
    for t, var in v.items():
        assert var.dtype == np.float32 and np.float32(var + np.float32(1e-3)) == np.float32(t)
        assert np.float32(1.0) / np.sqrt(np.float32(var + np.float32(1e-3))) == np.float32(t ** -0.5)
    assert abs(float(v[1.0]) - 0.999) < 1e-7


def test_generator_refuses_inexact_flags():
    for flag in (dict(leaky_relu=True), dict(resnet_v2=True, se_units=42)):
        with pytest.raises(AssertionError):
            xl.lattice_weights(NetDesc(5, 8, 8, 128, 1, [155, 155], **flag), 1, nnz=2, wmax=1)
    # a squeeze-excite net that violates a condition: a gating entry of 2^4 is an unsaturated gate
    desc, w, x, _ = build(SE_VARIED)
    xl.check_representable(desc, w, x, "fp32-ieee")
    bad = [(n, (np.sign(a) * 16.0).astype(np.float32) if n == "res1_se_gating" else a) for n, a in w]
    with pytest.raises(AssertionError, match="unsaturated"):
        xl.check_representable(desc, bad, x, "fp32-ieee")


def test_generator_covers_the_lattice():
    """Sparse integer convs, all three vars, several powers of two as gamma, integer shifts."""
    desc, w, _, _ = build("8x8_f128_b2")
    w = dict(w)
    k = w["res1_conv0"]
    assert set(np.unique(k)) == {-1.0, 0.0, 1.0} and np.all((k != 0).sum(axis=(0, 1, 2)) == 2)
    assert np.all((w["policy0_conv"] != 0).sum(axis=(0, 1, 2)) == 64)      # the heads read half of the trunk each
    vars_ = np.unique(np.concatenate([a for n, a in w.items() if n.endswith("_var")]))
    assert set(vars_) == set(float(v) for v in xl.exact_vars().values())
    gammas = np.unique(np.concatenate([a for n, a in w.items() if n.endswith("_gamma")]))
    assert len(gammas) >= 3 and all(xl.sig_bits(g) == 1 for g in gammas)
    for suffix in ("_beta", "_mean", "policy0_bias", "value_hidden_bias"):
        vals = np.unique(np.concatenate([a for n, a in w.items() if n.endswith(suffix)]))
        assert set(vals) == {-1.0, 0.0, 1.0}, suffix
    assert set(np.unique(w["policy0_dense"])) == {-1.0, 0.0, 1.0}


@pytest.mark.parametrize("name", ["8x8_f128_b2", "v2_8x8_f128_b2_pool", "v2_13x13_f256_b2_concat", "6x9_legacy_f40_b2",
                                  "v2_10x10_f256_b1_bare"] + sorted(SE_CASES))
def test_walk_is_the_oracle(name):
    """exact_lattice._forward, which the conditions and the faults walk, is nn_ref.forward.  On a
    squeeze-excite net the walk's gates are the classes 0, 1/2, 1 and nn_ref's a float64 sigmoid (a
    "0" gate is about 1e-100 there), so the two are compared after the snap to the lattice."""
    desc, w, x, expected = build(name)
    ours, _ = xl._forward(desc, w, x)
    with np.errstate(over="ignore"):
        ref = nn_ref.forward(desc, xl.oracle_weights(w), x, logits=True)
    unit = 2.0 ** xl.lattice_exponent(desc, w, x)
    for a, b, e in zip(ours, ref, expected):
        if desc.se_units:
            assert np.abs(b / unit - np.rint(b / unit)).max() <= 1e-5
            b = np.rint(b / unit) * unit
        assert np.array_equal(a, b) and np.array_equal(a, e)


@pytest.mark.parametrize("name", sorted(CASES))
def test_conditions(name):
    """check_representable holds for every mode the GPU file runs the net in; where the case claims
    every mode whose conditions hold, it fails for each mode left out."""
    c = CASES[name]
    desc, w, x, _ = build(name)
    for mode in c.modes:
        xl.check_representable(desc, w, x, mode)
    if c.exhaustive:
        for mode in set(ALL) - set(c.modes):
            with pytest.raises(AssertionError):
                xl.check_representable(desc, w, x, mode)


@pytest.mark.parametrize("rows,names", [(5, ("8x8_f128_b2", CHUNKED, SE_VARIED)), (LARGE_ROWS, ("8x8_f128_b2",))])
def test_conditions_at_other_row_counts(rows, names):
    for name in names:
        desc, w, x, _ = build(name, rows)
        for mode in CASES[name].modes:
            xl.check_representable(desc, w, x, mode)


@pytest.mark.parametrize("name,rows", [(name, None) for name in sorted(SE_CASES)] + [(SE_VARIED, 5)])
def test_se_lattice(name, rows):
    """The squeeze-excite nets are what the generator says: balanced +-1 compress units, at most one
    +-K per gating column with about a quarter of the columns empty, the last unit read, K derived
    (the smallest power of two with every nonzero oracle |z| >= 256, so the smallest lies in
    [256, 512)), every gate one of 0, 1/2, 1, and the lattice unit one step lower per block; on the
    boards whose position count is a power of two some fed hidden unit sits within a lattice step
    of 0 (check_representable returns them), on the others every fed unit clears the float32 error
    bound of its sum (se_fragile_units)."""
    desc, w, x, _ = build(name, rows)
    wd = dict(w)
    S, F = desc.se_units, desc.cnn_filter_size
    zmin = np.inf
    for i, (_, u, w1, w2, info) in enumerate(xl.se_walk(desc, w, x)):
        assert np.array_equal(w1, wd["res%d_se_compress" % i]) and np.array_equal(w2, wd["res%d_se_gating" % i])
        assert w1.shape == (F, S) and set(np.unique(w1)) == {-1.0, 0.0, 1.0} and np.all(w1.sum(axis=0) == 0)
        per_column = (w2 != 0).sum(axis=0)
        assert per_column.max() == 1 and 0.1 <= (per_column == 0).mean() <= 0.4
        K = np.abs(w2).max()
        assert set(np.unique(np.abs(w2))) == {0.0, K} and xl.sig_bits(K) == 1
        assert (w2[S - 1] != 0).any() and (S <= 64 or (w2[64:] != 0).any())
        assert np.isin(info["gate"], (0.0, 0.5, 1.0)).all()
        zmin = min(zmin, np.abs(info["z"][(info["prod"] != 0).any(axis=1)]).min())
        if not _pow2_board(desc):
            fed = (w2 != 0).any(axis=1)
            for b in range(x.shape[0]):
                assert not (xl.se_fragile_units(info["sums"][b], w1, info["npos"]) & fed).any()
    assert 256 <= zmin < 512
    near = xl.check_representable(desc, w, x, CASES[name].modes[0])
    assert bool(near) == _pow2_board(desc)
    plain = [(n, a) for n, a in w if "_se_" not in n]
    lowered = xl.lattice_exponent(dataclasses.replace(desc, se_units=0), plain, x) - xl.lattice_exponent(desc, w, x)
    # (one step per block on the path to the logits; the concat head also reads the earlier layers)
    assert 1 <= lowered <= desc.residual_layers and (lowered == desc.residual_layers or desc.concat_all_layers)


def test_wide_cases_use_the_width():
    """The wide nets put the stated number of bits where they say: the initial conv's folded weights,
    the residual convs' inputs, the policy Dense's weights and features."""
    seen = {}

    def tap(kind, name, inp, k, bn, skip):
        seen[name] = (xl.sig_bits(inp), xl.sig_bits(k) if k is not None else 0)
    for bits in (16, 22, 24):
        desc, w, x, _ = build("wide_w0_%d" % bits)
        xl._forward(desc, w, x, tap=tap)
        assert seen["initial_conv"][1] == bits
        desc, w, x, _ = build("wide_stream_%d" % bits)
        xl._forward(desc, w, x, tap=tap)
        assert seen["res0_conv0"][0] == bits and seen["policy0_conv"][0] >= bits - 1
    desc, w, x, _ = build("gemm_wide_features")
    xl._forward(desc, w, x, tap=tap)
    assert 8 < seen["policy0_dense"][0] <= 16 and seen["policy0_dense"][1] == 1
    desc, w, x, _ = build("gemm_wide_weights")
    xl._forward(desc, w, x, tap=tap)
    assert seen["policy0_dense"][0] <= 8 and seen["policy0_dense"][1] == 16


@pytest.mark.parametrize("name", sorted(CASES))
def test_liveness(name):
    """Conditions on the inputs, on the oracle alone: at least 30 % of the final trunk is nonzero,
    every policy role's expected logits take at least 32 values, the value logits are not all equal."""
    desc, w, x, expected = build(name)
    assert desc.residual_layers < 6
    assert xl.trunk_alive(desc, w, x) >= 0.30
    for z in expected[:-1]:
        # (a head case's role of fewer than 32 columns: test_head_liveness)
        assert len(np.unique(z)) >= 32 or (name in HEAD_CASES and z.shape[1] < 32)
    assert len(np.unique(expected[-1])) > 1
    if name in SE_CASES:
        _se_liveness(desc, w, x)


def _se_liveness(desc, w, x):
    """In every block all three gate values occur, each on at least 10 % of the (board, channel)
    pairs, and every pair of boards in the launch differs in at least 4 channels' gates."""
    live = xl.se_liveness(desc, w, x)
    assert len(live) == desc.residual_layers
    for shares, differ in live:
        assert min(shares) >= 0.10 and abs(sum(shares) - 1.0) < 1e-12, shares
        assert differ >= 4, differ


def test_se_liveness_at_5_rows():
    desc, w, x, _ = build(SE_VARIED, 5)
    assert x.shape[0] == 5
    _se_liveness(desc, w, x)


@pytest.mark.parametrize("family,fault", [(f, fault) for f in sorted(SE_FAMILIES) for fault in xl.SE_FAULTS
                                          if _se_fault_applies(SE_FAMILIES[f], fault)])
def test_se_fault_is_seen(family, fault):
    """Each slip a squeeze-excite kernel can make, on the oracle side alone, moves a logit: a
    neighbouring board's gates, gates off by a lane group or a co tile, another block's matrices, the
    last unit dropped, no relu, the gate applied after the add, a mean one count short."""
    desc, w, x, expected = build(SE_FAMILIES[family])
    assert _differs(xl.faulty_se_logits(desc, w, x, fault), expected)


def test_se_faults_cover_every_family():
    """Every fault is shown on every SE family where it can occur (_se_fault_applies)."""
    for fault in xl.SE_FAULTS:
        on = [f for f, name in SE_FAMILIES.items() if _se_fault_applies(name, fault)]
        assert len(on) >= (4 if fault == "mean_one_count" else 6), (fault, on)
    assert len(SE_FAMILIES) == len(SE_CASES) == 8


@pytest.mark.parametrize("fault", GEOMETRY_FAULTS)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_fault_is_seen(family, fault):
    """Two taps swapped, wrap-around padding along one border, two input channels swapped, the last
    input channel dropped (F = 96 padded to 128 among the families), in the last residual conv."""
    desc, w, x, expected = build(FAMILIES[family])
    assert _differs(xl.faulty_logits(desc, w, x, fault, _last_residual_conv(desc)), expected)


@pytest.mark.parametrize("name,mode", [(name, mode) for name, c in CASES.items() if c.wide and c.wide.get("kind") in
                                       ("initial_weights", "stream") for mode in c.modes])
def test_lost_lo_part_is_seen(name, mode):
    """Wide cases: the operand of the wide conv rounded to the mode's hi format (fp32-ieee has no lo
    part: there, a rounding to bf16x3's 16 bits where the net is wider than that, else to 8)."""
    desc, w, x, expected = build(name)
    bits = xl.HI_BITS.get(mode, 16 if CASES[name].wide["bits"] > 16 else 8)
    fault, conv = ("lo_weights", "initial_conv") if CASES[name].wide["kind"] == "initial_weights" else ("lo_inputs", "res0_conv0")
    assert _differs(xl.faulty_logits(desc, w, x, fault, conv, bits=bits), expected)


@pytest.mark.parametrize("name,kind", [("gemm_wide_features", "inputs"), ("gemm_wide_weights", "weights")])
def test_lost_lo_part_of_the_policy_gemm_is_seen(name, kind):
    desc, w, x, expected = build(name)
    w2 = [(n, xl.round_bits(a, 8).astype(np.float32) if (kind == "weights" and n == "policy1_dense") else a) for n, a in w]
    if kind == "weights":
        got = xl._forward(desc, w2, x)[0]
    else:
        seen = {}

        def tap(k, n, inp, *rest):
            if n == "policy1_dense":
                seen["z"] = xl.round_bits(inp, 8) @ dict(w)["policy1_dense"].astype(np.float64) + dict(w)["policy1_bias"]
        xl._forward(desc, w, x, tap=tap)
        got = list(expected)
        got[1] = seen["z"]
    assert _differs(got, expected)


@pytest.mark.parametrize("name", ["8x8_scaled", "8x8_scaled_permuted"])
def test_neighbours_scale_is_seen(name):
    """One board of a scaled launch given its neighbour's scale."""
    desc, w, x, expected = build(name)
    for b in range(x.shape[0]):
        nb = (b + 1) % x.shape[0]
        bad = x.copy()
        bad[b] = x[b] * np.float32(np.abs(x[nb]).max() / np.abs(x[b]).max())
        got = nn_ref.forward(desc, xl.oracle_weights(w), bad, logits=True)
        assert all(not np.array_equal(g[b], e[b]) for g, e in zip(got, expected)), b


def test_scaled_boards():
    """The scaled case holds the four scales, the permuted case the same boards in another order, and
    its expected logits are the first case's rows in that order."""
    _, _, x, expected = build("8x8_scaled")
    _, _, xp, expected_p = build("8x8_scaled_permuted")
    assert tuple(float(np.abs(b).max()) for b in x) == SCALES
    order = list(CASES["8x8_scaled_permuted"].order)
    assert np.array_equal(xp, x[order])
    for e, ep in zip(expected, expected_p):
        assert np.array_equal(ep, e[order])


def test_every_mode_and_family_is_run():
    """Every arithmetic mode of the README, every kernel family, and a probability-mode forward per
    mode are in the GPU file's parametrisation."""
    import os
    readme = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "README.md")).read()
    section = readme.split("## Arithmetic modes")[1].split("\n## ")[0]
    run = {m for c in CASES.values() for m in c.modes}
    assert run == set(ALL) == set(xl.MODE_BITS)
    for mode in ALL:
        assert '"%s"' % mode in section or "`\"%s\"`" % mode in section, mode
    assert {m for _, m in PROBABILITY} == set(ALL)
    assert len(FAMILIES) >= 9 + len(SE_FAMILIES) and len(SE_FAMILIES) == 8


# ---- the dense heads ---------------------------------------------------------------------------------
def _head_fault_applies(name, fault):
    """Where a head fault can occur at all (exact_lattice.head_fault_roles has the outputs it touches):
    a neighbour's features or bias need a second role; an offset computed with the other path's
    padding, a row stride of P for P4 and a dropped partial group of 4 need a role whose size is no
    multiple of 4 (for the offset: in front of another role); swapped value outputs need two values.
    The last tile of 16, the last k and the last hidden unit exist on every net (head_last_rows makes
    every Dense read its last input)."""
    desc, w, _, _ = build(name)
    return bool(xl.head_fault_roles(desc, w, fault))


@pytest.mark.parametrize("name", sorted(HEAD_CASES))
def test_head_liveness(name):
    """On the largest launch of every head case: every role's logits and the value logits hold a
    nonzero entry in every row, no two rows are equal in any output, and every policy column and
    every value output is nonzero in some row -- a P = 1 role and a V = 1 value in every row."""
    c = CASES[name]
    desc, w, x, expected = build(name)
    assert c.head and x.shape[0] == max(c.rows or (1, 3)) and set(c.path) >= set(c.modes)
    assert xl.head_liveness(expected) == []
    for z in expected:
        if z.shape[1] == 1:
            assert (z != 0).all()
    wd = dict(w)
    for r in range(desc.role_count):
        assert wd["policy%d_dense" % r][-1, -1] != 0
    assert wd["value_hidden"][-1, -1] != 0 and (wd["value_dense"][-1] != 0).all()


def test_head_cases_cover_the_parameter_space():
    """Role counts 1 to 4, value counts 1 to 4, hidden widths of 6 and above 256 that are no multiple
    of 4, a sigmoid and a pooling value head, every heads_path the kernels can take, and the
    launches whose last heads workgroup (5 rows) and last GEMM board tile (65 rows) are partial."""
    descs = [c.desc for c in HEAD_CASES.values()]
    assert {d.role_count for d in descs} == {1, 2, 3, 4} and {d.num_values for d in descs} == {1, 2, 3, 4}
    vh = {d.value_hidden_size for d in descs}
    assert 6 in vh and any(v > 256 and v % 4 and v % 64 for v in vh)
    assert any(d.value_sigmoid for d in descs) and any(d.global_pooling_value and xl.sig_bits(float(d.hw)) == 1 for d in descs)
    assert any(1 in d.policy_dist_count for d in descs) and any(3072 in d.policy_dist_count for d in descs)
    paths = {bits for c in HEAD_CASES.values() for mode, bits in c.path.items() if mode in c.modes}
    assert paths == {0, 3, 8, 16, 24, 3 | 16, 3 | 4 | 16}
    assert any(c.rows and 5 in c.rows for c in HEAD_CASES.values()) and any(c.rows and 65 in c.rows for c in HEAD_CASES.values())
    for name in (HEAD_VARIED, HEAD_CHUNKED, HEAD_NO_GEMM) + tuple(n for n, _, _ in HEAD_LARGE_VARIANTS):
        assert build(name)[2].shape[0] >= 5


@pytest.mark.parametrize("name,fault", [(name, fault) for name in sorted(HEAD_CASES) for fault in xl.HEAD_FAULTS])
def test_head_fault_is_seen(name, fault):
    """Each slip a heads kernel can make, on the oracle side alone, moves an expected logit of every
    output it touches (exact_lattice.faulty_head_logits), on every head case where it can occur."""
    if not _head_fault_applies(name, fault):
        return
    desc, w, x, expected = build(name)
    got = xl.faulty_head_logits(desc, w, x, fault)
    for r in xl.head_fault_roles(desc, w, fault):
        assert not np.array_equal(got[r], expected[r]), (name, fault, r)
    clean = xl.head_operands(desc, w, x)
    for r in range(desc.role_count):      # (the operands the faults are applied to are the walk's own)
        xr, k, b = clean["policy%d_dense" % r]
        assert np.array_equal(xr @ k + b, expected[r])


def test_head_faults_cover_the_cases():
    """Every fault occurs on most cases; the ones that need unequal padding or two values on at least five."""
    for fault in xl.HEAD_FAULTS:
        on = [name for name in HEAD_CASES if _head_fault_applies(name, fault)]
        assert len(on) >= (len(HEAD_CASES) if fault in ("drop_last_tile16", "drop_last_k", "drop_last_hidden") else 5), (fault, on)


@pytest.mark.parametrize("tie", (False, True), ids=("one", "tie"))
@pytest.mark.parametrize("name,mode", SATURATED)
def test_saturated_conditions(name, mode, tie):
    """The saturated nets still meet the mode's conditions; the raised logits stand at least 2^11 above
    every other of their row (so float32's exp of the difference is 0, as float64's is), and the
    float64 softmax / sigmoid of the expected logits is exactly the 1, 0.5 and 0 the GPU test asserts."""
    desc, w, x, expected, probs = saturated(name, tie)
    xl.check_representable(desc, w, x, mode)
    for i, (z, p) in enumerate(zip(expected, probs)):
        if i == desc.role_count and desc.value_sigmoid:
            with np.errstate(over="ignore"):
                assert np.array_equal(1.0 / (1.0 + np.exp(-z)), p)
            continue
        assert np.array_equal(_softmax64(z), p), (name, i)
        low = np.where(p > 0, -np.inf, z).max(axis=1)
        assert (z.max(axis=1) - low >= SAT / 2).all()


# ---- the input path (tests/test_nn_input_exact_gpu.py) -------------------------------------------------
def _input_fault_rows(fault):
    return 2 if fault == "neighbour_board_planes" else 1


@pytest.mark.parametrize("name", sorted(INPUT_CASES))
def test_input_conditions(name):
    """check_representable holds in every mode the GPU file runs the case in, at its 5 rows."""
    desc, w, x, _ = input_build(name)
    assert x.shape[0] == 5 and INPUT_CASES[name].modes
    for mode in INPUT_CASES[name].modes:
        xl.check_representable(desc, w, x, mode)


def test_input_conditions_at_the_large_launch():
    for name in (EDGE_FITS, EDGE_OVER):
        desc, w, x, _ = input_build(name, INPUT_LARGE_ROWS)
        assert x.shape[0] == INPUT_LARGE_ROWS
        xl.check_representable(desc, w, x, "bf16x3")


@pytest.mark.parametrize("name", sorted(INPUT_CASES))
def test_input_liveness(name):
    """Every (tap, plane) place of the initial conv is read, and removing any one of them moves an
    expected logit of the first row alone (hence of every launch, which all hold that row); the
    relu behind the initial conv is the identity there (cover_initial), and every trunk channel is
    read by one of policy 0's two conv outputs."""
    desc, w, x, expected = input_build(name)
    k = dict(w)["initial_conv"]
    places = xl.initial_places(desc)
    assert k.shape[0] == desc.initial_kernel and len(places) == k[..., 0].size and (k.reshape(len(places), -1) != 0).any(axis=1).all()
    assert (k.reshape(len(places), -1)[np.arange(len(places)), np.arange(len(places)) % k.shape[3]] == 1).all()
    assert ((dict(w)["policy0_conv"][0, 0] != 0).sum(axis=1) == 1).all()
    assert xl.initial_liveness(desc, w, x[:1]) == []
    assert xl.trunk_alive(desc, w, x) >= 0.30
    for z in expected[:-1]:
        assert len(np.unique(z)) >= 32 and len(np.unique(z, axis=0)) == x.shape[0]


def test_input_liveness_names_a_dead_place():
    """initial_liveness on a net without the cover (the generator's two weights per channel): places
    that nothing reads, and places that are read and hidden, are named."""
    desc, _, x, _ = input_build("in_8x8_c24_f128")
    w = xl.lattice_weights(desc, 1, nnz=2, wmax=1)
    k = dict(w)["initial_conv"]
    unread = [pl for j, pl in enumerate(xl.initial_places(desc)) if not k.reshape(-1, k.shape[3])[j].any()]
    dead = xl.initial_liveness(desc, w, x[:1])
    assert unread and set(unread) < set(dead)


@pytest.mark.parametrize("name,fault", [(name, fault) for name in sorted(INPUT_CASES) for fault in xl.INPUT_FAULTS])
def test_input_fault_is_seen(name, fault):
    """Each slip an input path can make, on the oracle side alone, moves an expected logit of the first
    row (a neighbour's planes: of the first two) on every case whose geometry lets it occur."""
    desc, w, x, expected = input_build(name)
    rows = _input_fault_rows(fault)
    if not xl.input_fault_applies(desc, fault, rows):
        return
    assert _differs(xl.faulty_input_logits(desc, w, x[:rows], fault), [e[:rows] for e in expected]), (name, fault)


@pytest.mark.parametrize("offset", (1, 2, 3))
def test_input_shifted_row_at_every_offset(offset):
    """A plane block 4, 8 or 12 bytes behind a 16-byte boundary, read from the boundary."""
    desc, w, x, expected = input_build(EDGE_FITS)
    assert _differs(xl.faulty_input_logits(desc, w, x[:1], "shifted_row", offset=offset), [e[:1] for e in expected])


def test_input_cases_cover_the_parameter_space():
    """Every chunk count from 4 to 36 in both fused modes on two fused geometries at least; the swizzle
    that once spilled occurs at 12, 20, 24, 28 and 36 chunks (K0 = 96, 160, 224 among them) and the fault
    is seen there at one row (test_input_fault_is_seen); both sides of the gather's padding in the four
    layered modes; a 1 x 1 initial conv; plane blocks off alignment and above the prefetch's cap; at
    most one refused case per chunk count."""
    chunks = lambda d: xl.initial_k0(d) // 8
    for n in range(4, 37, 4):
        for mode in FUSED:
            geos = {(c.desc.hw, c.desc.cnn_filter_size) for c in INPUT_CASES.values() if chunks(c.desc) == n and mode in c.modes
                    and c.desc.initial_kernel == 3}
            assert len(geos) >= 2, (n, mode, geos)
    spills = {n for n in range(4, 37, 4) if xl.input_fault_applies(NetDesc(8 * n // 9, 8, 8, 64, 1, [9]), "swizzle_spill", 1)}
    assert spills == {12, 20, 24, 28, 36}
    assert {xl.initial_k0(c.desc) for c in INPUT_CASES.values() if c.desc.initial_kernel == 3} >= {96, 160, 224}
    layered = {c.desc.input_channels for c in INPUT_CASES.values() if set(LAYERED) <= set(c.modes) and c.desc.initial_kernel == 3}
    assert layered >= {15, 16, 17, 33}
    assert {c.desc.input_channels for c in INPUT_CASES.values() if c.desc.initial_kernel == 1} == {3, 32, 33}
    blocks = {c.desc.input_channels * c.desc.hw for c in INPUT_CASES.values()}
    assert any(b % 4 for b in blocks) and any(b % 4 == 0 and b > 4096 for b in blocks)
    refused = [chunks(d) for d, _ in INPUT_REFUSED.values()]
    assert len(refused) == len(set(refused)) <= 3


def test_heads_path_bits_match_the_header():
    """_native's HEADS_* are include/gzero_nn.h's GZ_HEADS_*."""
    import os
    import re
    from galvanise_zero_amd import _native
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gzero_nn.h")).read()
    bits = {name: int(value) for name, value in re.findall(r"#define GZ_(HEADS_\w+) (\d+)", header)}
    assert len(bits) == 5 and sorted(bits.values()) == [1, 2, 4, 8, 16]
    for name, value in bits.items():
        assert getattr(_native, name) == value
