"""Exactly representable nets: weights and planes on which every forward mode must return the float64
oracle's logits bit for bit (helper module of tests/test_nn_exact.py and tests/test_nn_exact_gpu.py;
it holds no tests).

If every operand, product, partial sum and activation of a forward is representable in the
arithmetic a mode uses, every correctly rounded operation is exact in any order, fused or not, and a
correct kernel returns the oracle's logits exactly.  lattice_weights / lattice_planes build such nets,
check_representable asserts the conditions under which that is a theorem, expected_logits is the
oracle (oracle/nn_ref.forward) snapped to the lattice, and faulty_logits applies a kernel-like slip
to the oracle side so that the CPU suite can show the comparison would notice it (faulty_se_logits:
the slips of a squeeze-excite kernel; faulty_head_logits: those of the dense heads, with
head_liveness, the conditions under which no output of a launch could pass against an untouched or
a neighbour's buffer; faulty_input_logits: the slips of plane staging, im2col and the initial conv,
on nets built with cover_initial, whose every (tap, plane) place initial_liveness shows to count).

How the BN fold is made exact: galvanise_zero_amd/csrc/nn/weight_image.h fold_element computes
scale = gamma / sqrt(fl32(var + 1e-3f)) in float32.  exact_vars() searches the float32 var for which
fl32(var + 1e-3f) is exactly 1, 1/4 and 4, so scale is gamma, 2 gamma and gamma / 2 exactly.  The
oracle adds 1e-3 to var in float64, which on those float32 vars is 1.3e-8 beside 1: a few 1e-9
relative per BN, measured 1.2e-5 to 2e-4 lattice units on the two-block nets here and half a unit on
boards scaled by 2^12 -- too much to snap.  So the oracle is given each var as the float64 v' with
v' + 1e-3 == fl32(var + 1e-3f) (oracle_weights): the same net as the float32 fold defines, on which
nn_ref.forward is exact, and expected_logits asserts both that the snap to the lattice moves nothing
by more than 1e-5 units and that the oracle on the float32 vars as they are agrees within that drift.

Squeeze-excite is in, under saturation conditions.  The gate is a sigmoid, but a float32
1.f / (1.f + exp(-z)) is exact at three points: 1 for z >= 17.4, 0 for z <= -88.8, 1/2 at z = 0 (ZSAT
below).  lattice_se_weights builds nets whose every gate is one of the three -- a +-1 compress matrix,
a gating matrix with at most one +-K per channel, K the smallest power of two that puts every nonzero
z at |z| >= 256 -- and u * 0, u * 1/2, u * 1 keep the stream on the lattice (one step lower per block).
_forward computes such gates as classes and refuses anything else; check_representable adds the
conditions under which the device's gates are those classes: on boards whose position count is a
power of two the whole gate path (sums, means, both Denses) is exact in any order, and the nets hold
a hidden unit that is exactly 0 from nonzero terms, so that a mean off by one count flips a gate; on
the other boards the mean is sum * fl32(1 / npos), and every hidden unit a gate reads must clear
twice the float32 error bound of its sum (se_fragile_units; units that do not are muted).  The gates
take all three values and differ from board to board and from channel to channel (se_liveness), so a
neighbour's gates, gates off by a lane group or a co tile, another block's matrices, a dropped unit,
a missing relu or a gate applied after the add each move a logit (faulty_se_logits).

Left out, and why:
  leaky_relu        0.03 is not dyadic: the negative side leaves every lattice
  se_units > 0 without saturating gates (lattice_weights refuses it unless given se=...)
  pooling value head on boards whose position count is no power of two (13 x 13, 10 x 10): the
                    trunk's channel mean is sum * fl32(1 / npos) (forward_kernel.h, "sm[r] * inv"),
                    a reciprocal that is not a power of two; 8 x 8 (1 / 64) is exact
  small errors in the scale of the squeeze-excite mean on boards whose position count is no power
                    of two: a saturated gate cannot see them, by construction
These stay with the tolerance tests.
"""
import numpy as np

from galvanise_zero_amd.nn.desc import weight_spec
from galvanise_zero_amd.nn.weights import random_planes
from oracle import nn_ref

# significand bits of a conv operand (BN-folded weight, input) per arithmetic mode
MODE_BITS = {"bf16": 8, "bf16-layered": 8, "bf16x3": 16, "bf16x3-layered": 16, "fp16x3-layered": 22, "fp32-ieee": 24}
# three-part modes (hi hi + hi lo + lo hi, lo lo dropped): the bits of the hi part alone
HI_BITS = {"bf16x3": 8, "bf16x3-layered": 8, "fp16x3-layered": 11}
ACC_BITS = 24            # every sum is fp32
GEMM_BITS, GEMM_HI = 16, 8   # policy_gemm_kernel: bf16 hi + lo of features and weights, in every mode that has it
GEMM_MIN_P = 512         # gz_nn.hip: gemm_heads = ... && maxP >= 512 (and no fused heads)
F16_MAX = 65504.0


# ---- bit counting -------------------------------------------------------------------------------
def _mant(a):
    """(integer significands of 53 bits, exponents) of the nonzero elements of a (exact)."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    a = np.abs(a[a != 0])
    m, e = np.frexp(a)
    return (m * 2.0 ** 53).astype(np.int64), e


def _trailing(i):
    return np.round(np.log2((i & -i).astype(np.float64))).astype(np.int64)   # (a power of two: exact)


def sig_bits(a):
    """The largest number of significant bits (first to last set bit) of any element; 0 for all zero."""
    i, _ = _mant(a)
    return int((53 - _trailing(i)).max()) if i.size else 0


def lsb_exp(a):
    """The smallest exponent of a lowest set bit: every element is a multiple of 2^lsb_exp(a).
    None for an all-zero array."""
    i, e = _mant(a)
    return int((e - 53 + _trailing(i)).min()) if i.size else None


def round_bits(a, bits):
    """a rounded to `bits` significant bits, nearest even (what keeping a hi part alone does)."""
    m, e = np.frexp(np.asarray(a, dtype=np.float64))
    return np.ldexp(np.rint(np.ldexp(m, bits)), e - bits)


def _emin(*es):
    es = [e for e in es if e is not None]
    return min(es) if es else None


def _eadd(a, b):
    return None if a is None or b is None else a + b


# ---- the generator ------------------------------------------------------------------------------
def exact_vars():
    """{t: float32 var with fl32(var + 1e-3f) == t} for t = 1, 1/4, 4, found by search around t - 1e-3:
    of the float32 that qualify, the one nearest t - 1e-3 (so the float64 oracle is nearest too)."""
    eps = np.float32(1e-3)
    out = {}
    for t in (1.0, 0.25, 4.0):
        v = np.float32(t - 1e-3)
        cand = [v]
        for _ in range(4):
            cand = [np.nextafter(cand[0], np.float32(-1))] + cand + [np.nextafter(cand[-1], np.float32(9))]
        ok = [c for c in cand if np.float32(c + eps) == np.float32(t)]
        assert ok, t
        out[t] = min(ok, key=lambda c: abs(float(c) - (t - 1e-3)))
    return out


# (gamma, fl32(var + eps)) pairs: scales 1/2 and 1 through all three vars
_SCALE_PAIRS = {0.5: ((0.5, 1.0), (0.25, 0.25), (1.0, 4.0)), 1.0: ((1.0, 1.0), (0.5, 0.25), (2.0, 4.0))}
WIDE_KINDS = ("initial_weights", "stream", "policy_dense")


def _sparse(rng, shape, nnz, wmax, force_last):
    """[kh, kw, cin, cout] (or [in, out]) with nnz signed integers of up to wmax per output, at random
    places; force_last: outputs 0-3 keep one entry on the last input channel."""
    cout = shape[-1]
    cin = shape[-2]
    places = int(np.prod(shape[:-1]))
    nnz = min(nnz, places)
    k = np.zeros((places, cout), dtype=np.float64)
    for co in range(cout):
        if force_last and co < 4 and cin > 1:
            last = int(rng.integers(0, places // cin)) * cin + cin - 1
            rest = rng.choice(places - 1, size=nnz - 1, replace=False)
            at = np.concatenate([[last], rest + (rest >= last)])
        else:
            at = rng.choice(places, size=nnz, replace=False)
        k[at, co] = rng.integers(1, wmax + 1, size=nnz) * rng.choice((-1, 1), size=nnz)
    return k.reshape(shape)


def _sparse_dense(rng, shape, nnz, lo, hi):
    """[in, out] with about nnz entries of magnitude lo..hi per output (duplicates coincide)."""
    k = np.zeros(shape, dtype=np.float64)
    rows = rng.integers(0, shape[0], size=(nnz, shape[1]))
    vals = rng.integers(lo, hi + 1, size=rows.shape) * rng.choice((-1, 1), size=rows.shape)
    k[rows, np.arange(shape[1])[None, :]] = vals
    return k


SE_PER_UNIT = 16         # entries of a compress unit: half +1, half -1
SE_READS = 0.75          # the share of the channels whose gate reads a unit (the others: a zero column, gate 1/2)


def _se_compress(rng, shape, twin):
    """[F, S]: per unit SE_PER_UNIT entries at random channels, half +1 and half -1.  twin = (c1, c2,
    unit): that unit reads +c1 - c2 alone, two channels whose conv2 kernels are the same, so that
    its pre-activation is exactly 0 from nonzero terms, and one count too few in either mean shows."""
    F, S = shape
    n = min(SE_PER_UNIT, F // 2 * 2)
    a = np.zeros(shape)
    for j in range(S):
        at = rng.choice(F, size=n, replace=False)
        a[at[:n // 2], j], a[at[n // 2:], j] = 1.0, -1.0
    if twin:
        a[:, twin[2]] = 0.0
        a[twin[0], twin[2]], a[twin[1], twin[2]] = 1.0, -1.0
    return a


def _se_gating(rng, shape, K, mute, twin):
    """[S, F]: at most one entry +-K per channel, about a quarter of the channels none; two channels
    are made to read unit S - 1 and (S > 64) a unit >= 64, a third the twin unit (_se_compress).
    mute: units whose row is zeroed.  (The draws do not depend on K or mute.)"""
    S, F = shape
    reads = rng.random(F) < SE_READS
    units = rng.integers(0, S, size=F)
    signs = rng.choice((-1.0, 1.0), size=F)
    ca, cb, cc = rng.choice(F, size=3, replace=False)
    high = int(rng.integers(min(64, S - 1), S))
    reads[ca], units[ca] = True, S - 1
    if S > 64:
        reads[cb], units[cb] = True, high
    if twin:
        reads[cc], units[cc] = True, twin[2]
    a = np.zeros(shape)
    c = np.nonzero(reads)[0]
    a[units[c], c] = signs[c] * K
    a[sorted(mute)] = 0.0
    return a


def lattice_weights(desc, seed, *, nnz, wmax, wide=None, se=None, cover_initial=False):
    """Weights in weight_spec order on which the forward is exact.

    Conv kernels: sparse, nnz signed integers of up to wmax per 3 x 3 (initial) output channel at
    random (tap, input channel) places; the heads' 1 x 1 convs, fp32 in every mode, read half of the
    trunk's channels each (2 nnz with a wide policy Dense, whose features must stay narrow).  _var: one of
    exact_vars(); _gamma: powers of two paired with the var so that the folded scale is 1/2 or 1;
    _beta, _mean, conv biases, dense biases: integers in {-1, 0, 1}; dense kernels: sparse {-1, 0, 1}.

    wide = {"kind": k, "bits": W, ...} makes one operand class use W significant bits (v1 nets):
      "initial_weights"  the initial conv has one weight A per output channel, an odd integer of W
                         bits with random bits all the way down (so that no hi + lo pair of a narrower
                         mode holds it), under gamma = 2^-8 and mean = A - 32 - (channel mod 16): its
                         output is (32 .. 47) / 256 where the plane is set, the wide part cancels in
                         the fp32 epilogue, and a lost or mis-scaled lo part of the weight shows
      "stream"           the initial BN's betas are such integers A of W bits, so the residual stream
                         is W bits wide; every conv that reads the stream (res0_conv0, the heads'
                         1 x 1 convs) is one +1 tap per output channel whose BN's mean is the A of the
                         channel it reads less 32 (1,024 in the heads), which takes the wide part off
                         again (needs value_bn and one residual block); integer lattice
                         (W = 24: A = 2^23 + d with d < 16, so that |w x| + |bias| stays below 2^24;
                         fp32's significand is one piece, so this uses its full width all the same)
      "policy_dense"     the policy Dense kernels hold odd integers of W bits, two per output, on an
                         integer lattice (gamma = 1 everywhere)
    and wide = {"integer": True} alone only sets every gamma and var-sum to 1.

    se = {"K": K, "mute": {(block, unit), ..}} is what a squeeze-excite net needs (lattice_se_weights
    derives both from the planes): resN_se_compress holds SE_PER_UNIT entries per unit, half +1 and
    half -1; resN_se_gating at most one entry +-K per channel (K a power of two), none on about a
    quarter of them and none from a muted unit, so that every gate is sigmoid(+-K hid) or
    sigmoid(0): 0, 1/2 or 1 exactly once K hid is large (module docstring).

    cover_initial: every (tap, plane) place of the initial conv is read, and nothing downstream can
    hide it wholesale.  Place j (= tap * C + plane, the im2col row's k) gets a +1 towards output
    channel j mod F, in the place of whatever sparse entry stood there; the initial BN's mean is 0
    and its beta nnz * wmax or one more, which the sparse entries of a channel (at most nnz of them,
    wmax each, on 0 / 1 planes, under a scale of at most 1) cannot outweigh, so the relu behind the
    initial conv is the identity and every output channel is linear in the planes; policy 0's two
    1 x 1 conv outputs read complementary halves of the trunk's channels, so every channel reaches
    a head.  (Needs an initial BN, no conv biases, no wide operands; initial_liveness measures what
    the later relus still hide.)

    leaky_relu, and se_units > 0 without `se`, are refused (module docstring)."""
    assert not desc.leaky_relu, "0.03 is not dyadic"
    if cover_initial:
        assert not wide and se is None and not desc.conv_bias and (desc.initial_bn or not desc.resnet_v2), "cover_initial: plain nets with an initial BN"
    assert not desc.se_units or se is not None, "the squeeze-excite gate is a sigmoid: only with saturating gates (se=...)"
    if se is not None:
        assert desc.se_units and desc.resnet_v2 and sig_bits(float(se["K"])) == 1, se
    wide = dict(wide or {})
    kind, W = wide.get("kind"), int(wide.get("bits", 0))
    assert kind in (None,) + WIDE_KINDS, kind
    integer = bool(wide.get("integer")) or kind in ("stream", "policy_dense")
    if kind == "stream":
        assert not desc.resnet_v2 and desc.residual_layers == 1 and desc.value_bn and not desc.conv_bias
    if kind == "initial_weights":
        assert not desc.resnet_v2 and not desc.conv_bias
    rng = np.random.default_rng(seed)
    var = exact_vars()
    top = 2.0 ** (W - 1)

    def wide_values(n, odd):
        if W >= 24:
            d = 2 * rng.integers(0, 8, size=n) + 1 if odd else rng.integers(3, 13, size=n)
        else:
            d = rng.integers(0, 2 ** (W - 2) - 2 ** (W - 5), size=n) * 2 + (1 if odd else rng.integers(0, 2, size=n))
        return top + d
    stream_base, last_conv = None, None
    # SE on boards whose position count is a power of two: per block (c1, c2, unit), conv2's output
    # channel c2 a copy of c1 and one compress unit reading +c1 - c2 alone (_se_compress)
    twins = {}
    # what the BN named by a prefix does: "plain", "w0" (initial_weights), "beta" (stream's initial BN),
    # ("shrink", offset) (a BN behind a conv that reads the wide stream)
    special, single = {}, set()
    if kind == "initial_weights":
        special["initial_bn"] = "w0"
        single.add("initial_conv")
    if kind == "stream":
        special["initial_bn"] = "beta"
        special["res0_bn0"] = ("shrink", 32.0)
        single.add("res0_conv0")
        for r in range(desc.role_count):
            special["policy%d_bn" % r] = ("shrink", 1024.0)
            single.add("policy%d_conv" % r)
        special["value_bn"] = ("shrink", 1024.0)
        single.add("value_conv")
    out, pairs = [], {}
    for name, shape in weight_spec(desc):
        n = shape[-1]
        prefix = name.rsplit("_", 1)[0]
        sp = special.get(prefix, "plain")
        if len(shape) == 4:
            head = shape[0] == 1 and shape[3] <= 2
            if name in single:
                k = _sparse(rng, shape, 1, 1, True)
                k = np.abs(k)
                if kind == "initial_weights":
                    k = k * wide_values(n, True)
            else:
                # (the heads' convs are fp32 whatever the mode, so they can afford to read half of the
                # stream each: a slip in any trunk channel then reaches a logit)
                dense_head = head and kind != "policy_dense"
                k = _sparse(rng, shape, shape[2] // 2 if dense_head else (2 * nnz if head else nnz), wmax, True)
            if cover_initial and name == "initial_conv":
                places = int(np.prod(shape[:-1]))
                k.reshape(places, n)[np.arange(places), np.arange(places) % n] = 1.0
            if cover_initial and name == "policy0_conv":      # output 1 reads the channels that output 0 leaves out
                rest = np.nonzero(k[0, 0, :, 0] == 0)[0]
                k[0, 0, :, 1] = 0.0
                k[0, 0, rest, 1] = rng.integers(1, wmax + 1, size=rest.size) * rng.choice((-1, 1), size=rest.size)
            if se is not None and name.startswith("res") and name.endswith("_conv2") and sig_bits(float(desc.hw)) == 1:
                c1, c2 = rng.choice(n, size=2, replace=False)
                k[..., c2] = k[..., c1]
                twins[int(name[3:name.index("_")])] = (int(c1), int(c2), int(rng.integers(0, desc.se_units - 1)))
            a = last_conv = k
        elif name.endswith("_gamma"):
            if sp == "w0":
                pairs[prefix] = [(2.0 ** -8, 1.0)] * n
            elif integer or sp != "plain":
                pairs[prefix] = [(1.0, 1.0)] * n
            else:
                sc = rng.choice((0.5, 1.0), size=n, p=(0.25, 0.75))
                pairs[prefix] = [_SCALE_PAIRS[float(s)][int(rng.integers(0, 3))] for s in sc]
            a = np.array([g for g, _ in pairs[prefix]])
        elif name.endswith("_var"):
            a = np.array([var[t] for _, t in pairs[prefix]], dtype=np.float32)
        elif name.endswith("_beta"):
            if sp == "beta":
                a = stream_base = wide_values(n, False)
            elif cover_initial and prefix == "initial_bn":
                a = nnz * wmax + rng.integers(0, 2, size=n)
            elif sp == "plain":
                a = rng.integers(-1, 2, size=n)
            else:
                a = np.zeros(n)
        elif name.endswith("_mean"):
            if cover_initial and prefix == "initial_bn":
                a = np.zeros(n)
            elif sp == "w0":
                a = last_conv.sum(axis=(0, 1, 2)) - 32.0 - np.arange(n) % 16
            elif isinstance(sp, tuple):      # the A of the stream channel each output reads
                a = stream_base[np.argmax(last_conv.sum(axis=(0, 1)), axis=0)] - sp[1]
            elif sp == "beta":
                a = np.zeros(n)
            else:
                a = rng.integers(-1, 2, size=n)
        elif name.endswith("_se_compress"):
            a = _se_compress(rng, shape, twins.get(int(name[3:name.index("_")])))
        elif name.endswith("_se_gating"):
            blk = int(name[3:name.index("_")])
            a = _se_gating(rng, shape, float(se["K"]), {j for b, j in se.get("mute", ()) if b == blk}, twins.get(blk))
        elif len(shape) == 2:
            if kind == "policy_dense" and name.startswith("policy"):
                a = _sparse_dense(rng, shape, 2, 2 ** (W - 2), 2 ** (W - 1) - 1) * 2
                a = a + np.sign(a)                     # odd, W bits
            else:
                a = _sparse_dense(rng, shape, 8, 1, 1)
        else:                                          # conv biases (legacy), dense biases
            a = rng.integers(-1, 2, size=n)
        a = np.asarray(a, dtype=np.float64).reshape(shape)
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a), name
        out.append((name, a.astype(np.float32)))
    return out


def zero_trunk_shifts(desc, weights):
    """The same weights with every trunk BN's beta and mean and every trunk conv's bias zero: the
    trunk is then positively homogeneous, so a board multiplied by a power of two keeps its
    significand widths (the heads, fp32, keep their shifts)."""
    out = []
    for name, a in weights:
        trunk = name.startswith("initial") or name.startswith("res")
        if trunk and (name.endswith("_beta") or name.endswith("_mean") or name.endswith("_bias")):
            a = np.zeros_like(a)
        out.append((name, a))
    return out


def oracle_weights(weights):
    """The same weights as the float64 oracle must read them: every _var as the float64 v' with
    v' + 1e-3 == fl32(var + 1e-3f) exactly, so that nn_ref._bn's float64 var + 1e-3 is the number the
    float32 fold (weight_image.h fold_element) divides by, and not 1.3e-8 beside it.  With the
    float32 var itself the oracle is a few 1e-9 relative off the lattice, which on logits of 2^17
    lattice units and more (boards scaled by 2^12) is no longer a fraction of a unit."""
    out = []
    for name, a in weights:
        if name.endswith("_var"):
            t = (a.astype(np.float32) + np.float32(nn_ref.EPS)).astype(np.float64)
            v = t - nn_ref.EPS
            for _ in range(8):
                v = np.where(v + nn_ref.EPS < t, np.nextafter(v, np.inf), np.where(v + nn_ref.EPS > t, np.nextafter(v, -np.inf), v))
            assert np.array_equal(v + nn_ref.EPS, t), name
            a = v
        out.append((name, a))
    return out


SE_DENSITIES = (1.0, 0.5, 0.25, 0.125)


def lattice_planes(desc, n, seed, board_scale=None, mixed_fill=False):
    """random_planes' 0 / 1 boards; board_scale: one power of two per board; mixed_fill: every set
    bit is kept with a probability of its (board, input plane), one of SE_DENSITIES at random (board 0:
    all kept).  Still 0 / 1 planes, but boards whose planes are filled differently have channel means
    of different proportions, so their squeeze-excite gates differ (random_planes' boards all look
    alike to a mean)."""
    x = random_planes(desc, n, seed)
    if mixed_fill:
        rng = np.random.default_rng([seed, 77])
        p = rng.choice(SE_DENSITIES, size=(n, desc.input_channels))
        p[0] = 1.0
        x = (x * (rng.random(x.shape) < p[:, :, None, None])).astype(np.float32)
    if board_scale is not None:
        s = np.asarray(board_scale, dtype=np.float64)
        assert s.shape == (n,) and np.all(s > 0) and sig_bits(s) == 1, s
        x = (x * s[:, None, None, None]).astype(np.float32)
    return x


# ---- the forward, restated on the oracle's own pieces, with a tap on every conv ---------------------
def _fold64(w, conv, bn):
    """(scale, bias) of the BN behind a conv as float64 arrays, scale from fold_element's float32
    formula (weight_image.h): the exact scale when var is one of exact_vars()."""
    cb = w.get(conv + "_bias") if conv else None
    if bn is None:
        n = w[conv].shape[3]
        return np.ones(n), (cb.astype(np.float64) if cb is not None else np.zeros(n))
    g, b, m, v = (w[bn + s].astype(np.float32) for s in ("_gamma", "_beta", "_mean", "_var"))
    sc32 = g / np.sqrt(v + np.float32(nn_ref.EPS))
    sc = sc32.astype(np.float64)
    assert sig_bits(sc) <= 1, (bn, "the folded scale is no power of two")
    bi = b.astype(np.float64) + ((cb.astype(np.float64) if cb is not None else 0.0) - m.astype(np.float64)) * sc
    bi32 = (b + (cb.astype(np.float32) - m) * sc32) if cb is not None else (b - m * sc32)
    assert np.array_equal(bi32.astype(np.float64), bi), (bn, "the float32 fold of the bias is not exact")
    return sc, bi


def _conv(x, k, wrap=False):
    """nn_ref._conv_same; wrap: the left padding column holds the board's last column (what reading
    position p - 1 across a row's end does) instead of zeros."""
    if not wrap:
        return nn_ref._conv_same(x, k)
    kh, kw = k.shape[0], k.shape[1]
    assert kw == 3
    N, H, Wd, _ = x.shape
    xp = np.pad(x, ((0, 0), (kh // 2, kh // 2), (1, 1), (0, 0)))
    xp[:, :, 0, :] = xp[:, :, Wd, :]
    out = np.zeros((N, H, Wd, k.shape[3]))
    for dy in range(kh):
        for dx in range(kw):
            out += xp[:, dy:dy + H, dx:dx + Wd, :] @ k[dy, dx].astype(np.float64)
    return out


# A float32 gate 1.f / (1.f + exp(-z)) is exact at three points.  It is 1 once exp(-z) <= 2^-25
# (1 + 2^-25 ties to even at 1): z >= 25 ln 2 = 17.4.  It is 0 once exp(-z) overflows to +inf (expf,
# and __expf's v_exp_f32(-z log2 e) alike: past 2^128): z <= -128 ln 2 = -88.8.  It is 1/2 at z = 0
# (exp(0) = 1).  ZSAT = 128 clears both thresholds with room to spare; the nets are built with every
# nonzero |z| >= 2 ZSAT, so that a hidden unit with a relative error of up to a half (boards whose
# position count is no power of two, check_representable) still saturates.
ZSAT = 128.0
SE_FAULTS = ("gate_board_swap", "gate_channel_shift_4", "gate_channel_shift_16", "gate_block_slip", "drop_last_unit",
             "no_relu", "gate_after_add", "mean_one_count")


def _se_gates(u, w1, w2, blk, strict, fault=None):
    """The squeeze-excite gates of conv2's output u [N, H, W, F] as classes, not as a float64 sigmoid:
    1 where z >= ZSAT, 0 where z <= -ZSAT, 1/2 where every product hid_j w2[j, c] is exactly zero;
    strict: anything else is an assertion failure (otherwise, for the generator's first walk with
    K = 1 and for faulty walks: by the sign of z).  The hidden units come from the exact channel sums
    (sums @ w1 is exact in float64 on these nets; the division by npos keeps sign and zero), so that
    a pre-activation that cancels to 0 is 0 here whatever the position count.
    Returns (gate [N, F], info)."""
    N, H, W, F = u.shape
    npos = H * W
    sums = u.sum(axis=(1, 2))
    if fault and fault[0] == "mean_one_count" and fault[1] == blk:    # one position left out of one channel's sum
        _, _, b, j = fault
        pre_j = float(sums[b] @ w1[:, j])
        delta = -(u[b].reshape(npos, F) * w1[:, j][None, :])          # what leaving (pos, c) out adds to pre_j
        pos, c = np.unravel_index(np.argmin(delta) if pre_j > 0 else np.argmax(delta), delta.shape)
        sums = sums.copy()
        sums[b, c] -= u[b].reshape(npos, F)[pos, c]
    pre = (sums @ w1) / npos
    hid = pre if (fault and fault[0] == "no_relu") else np.maximum(pre, 0.0)
    if fault and fault[0] == "drop_last_unit":
        hid = hid.copy()
        hid[:, -1] = 0.0
    prod = hid[:, :, None] * w2[None, :, :]
    z = prod.sum(axis=1)
    half = (prod == 0).all(axis=1)
    one, zero = (z >= ZSAT, z <= -ZSAT) if strict else (z > 0, z < 0)
    assert (half | one | zero).all(), ("block %d: %d unsaturated gates, smallest nonzero |z| %g" %
                                       (blk, int((~(half | one | zero)).sum()), np.abs(z[~half]).min()))
    gate = np.where(half, 0.5, np.where(one, 1.0, 0.0))
    if fault and fault[0] == "gate_board_swap":
        for b in range(0, N - 1, 2):
            gate[[b, b + 1]] = gate[[b + 1, b]]
    if fault and fault[0].startswith("gate_channel_shift"):
        gate = np.roll(gate, int(fault[0].rsplit("_", 1)[1]), axis=1)
    return gate, dict(sums=sums, pre=pre, hid=hid, prod=prod, z=z, gate=gate, npos=npos)


def _forward(desc, weights, planes, tap=None, hooks=None, se_fault=None, se_strict=True):
    """nn_ref.forward(..., logits=True) restated with nn_ref's pieces (_conv_same, _bn, _act).

    hooks: {conv name: f(inp, k) -> (inp, k, wrap)} alters one conv's operands (faulty_logits).
    tap(kind, name, inp, k, bn, skip): called for every conv ("trunk" / "head"), every v2
    pre-activation ("affine": k is None), every Dense ("dense" / "gemm": bn is the bias array), the
    pooled mean ("pool") and every squeeze-excite ("se": inp is conv2's output, k the (compress,
    gating) pair, bn _se_gates' info, skip the stream).  se_fault: a tuple whose first item is one
    of SE_FAULTS (faulty_se_logits).  Squeeze-excite gates are classes (_se_gates), so the walk of
    an SE net stays on the lattice.
    Returns (logits [policy.., value] float64, final trunk activations)."""
    w = dict(oracle_weights(weights))
    hooks = hooks or {}
    tap = tap or (lambda *a: None)
    assert not desc.leaky_relu
    act = lambda t: nn_ref._act(t, False)

    def conv(x, name, bn, kind, skip=None):
        k = w[name].astype(np.float64)
        wrap, y = False, None
        if name in hooks:
            x, k, wrap, *y = hooks[name](x, k)     # (a fourth item: the conv's output itself, faulty_input_logits)
            y = y[0] if y else None
        tap(kind, name, x, k, bn, skip)
        if y is None:
            y = _conv(x, k, wrap)
        if desc.conv_bias:
            y = y + w[name + "_bias"].astype(np.float64)
        return nn_ref._bn(y, w, bn) if bn else y

    def dense(x, name, bias, kind="dense"):
        k = w[name].astype(np.float64)
        tap(kind, name, x, k, w[bias].astype(np.float64), None)
        return x @ k + w[bias].astype(np.float64)

    x = np.transpose(planes.astype(np.float64), (0, 2, 3, 1))
    v2 = desc.resnet_v2
    has_bn0 = not v2 or desc.initial_bn
    x = conv(x, "initial_conv", "initial_bn" if has_bn0 else None, "trunk")
    if has_bn0:
        x = act(x)
    layers = [x]
    for i in range(desc.residual_layers):
        t = x
        if v2:
            tap("affine", "res%d_bn1" % i, x, None, "res%d_bn1" % i, None)
            y = act(conv(act(nn_ref._bn(x, w, "res%d_bn1" % i)), "res%d_conv1" % i, "res%d_bn2" % i, "trunk"))
            if desc.se_units:
                u = conv(y, "res%d_conv2" % i, None, "trunk")
                j = 0 if (se_fault and se_fault[0] == "gate_block_slip" and i == 1) else i
                w1, w2 = (w["res%d_se_%s" % (j, s)].astype(np.float64) for s in ("compress", "gating"))
                gate, info = _se_gates(u, w1, w2, i, se_strict and not se_fault and not hooks, se_fault)
                tap("se", "res%d_se" % i, u, (w1, w2), info, t)
                g = gate[:, None, None, :]
                x = (t + u) * g if (se_fault and se_fault[0] == "gate_after_add") else t + u * g
            else:
                x = t + conv(y, "res%d_conv2" % i, None, "trunk", skip=t)
        else:
            y = act(conv(x, "res%d_conv0" % i, "res%d_bn0" % i, "trunk"))
            x = act(t + conv(y, "res%d_conv1" % i, "res%d_bn1" % i, "trunk", skip=t))
        layers.append(x)
    gemm = max(desc.policy_dist_count) >= GEMM_MIN_P
    outs = []
    for r in range(desc.role_count):
        h = act(conv(x, "policy%d_conv" % r, "policy%d_bn" % r, "head"))
        outs.append(dense(nn_ref._flatten(h, desc.flatten_nchw), "policy%d_dense" % r, "policy%d_bias" % r,
                          "gemm" if gemm else "dense"))
    if desc.concat_all_layers:
        flat = np.concatenate([nn_ref._flatten(act(conv(l, "value%d_conv" % j, "value%d_bn" % j, "head")), desc.flatten_nchw)
                               for j, l in enumerate(layers)], axis=1)
    else:
        flat = nn_ref._flatten(act(conv(x, "value_conv", "value_bn" if desc.value_bn else None, "head")), desc.flatten_nchw)
        if desc.global_pooling_value:
            tap("pool", "trunk", x, None, None, None)
            flat = np.concatenate([x.mean(axis=(1, 2)), flat], axis=1)
    hid = act(dense(flat, "value_hidden", "value_hidden_bias"))
    outs.append(dense(hid, "value_dense", "value_bias"))
    return outs, x


def lattice_exponent(desc, weights, planes):
    """e with every logit a multiple of 2^e, from the exponents of the weights' and the planes' own
    lowest set bits alone (no activation is looked at): through a conv and its BN
    e_out = min(e_in + e(folded weights), e(folded bias)), through an add the smaller of the two."""
    w = dict(weights)

    def conv(e, name, bn):
        sc, bi = _fold64(w, name, bn)
        return _emin(_eadd(e, lsb_exp(w[name].astype(np.float64) * sc)), lsb_exp(bi))

    def dense(e, name, bias):
        return _emin(_eadd(e, lsb_exp(w[name])), lsb_exp(w[bias]))

    v2 = desc.resnet_v2
    e = conv(lsb_exp(planes), "initial_conv", "initial_bn" if (not v2 or desc.initial_bn) else None)
    layers = [e]
    for i in range(desc.residual_layers):
        if v2:
            sc, bi = _fold64(w, None, "res%d_bn1" % i)
            y = conv(_emin(_eadd(e, lsb_exp(sc)), lsb_exp(bi)), "res%d_conv1" % i, "res%d_bn2" % i)
            y = conv(y, "res%d_conv2" % i, None)
            if desc.se_units:      # a gate of 1/2 lowers the lowest set bit by one
                y = _eadd(y, -1)
        else:
            y = conv(conv(e, "res%d_conv0" % i, "res%d_bn0" % i), "res%d_conv1" % i, "res%d_bn1" % i)
        e = _emin(e, y)
        layers.append(e)
    outs = [dense(conv(e, "policy%d_conv" % r, "policy%d_bn" % r), "policy%d_dense" % r, "policy%d_bias" % r)
            for r in range(desc.role_count)]
    if desc.concat_all_layers:
        f = _emin(*[conv(l, "value%d_conv" % j, "value%d_bn" % j) for j, l in enumerate(layers)])
    else:
        f = conv(e, "value_conv", "value_bn" if desc.value_bn else None)
        if desc.global_pooling_value:
            assert sig_bits(float(desc.hw)) == 1, "the pooled mean is dyadic only where the position count is a power of two"
            f = _emin(f, _eadd(e, -int(np.log2(desc.hw))))
    outs.append(dense(dense(f, "value_hidden", "value_hidden_bias"), "value_dense", "value_bias"))
    e = _emin(*outs)
    assert e is not None
    return e


# the float32 var beside the float64 v' of oracle_weights: |var + 1e-3 - t| / t <= 2^-25 (the rounding
# of the float32 sum) + 4.8e-11 / 0.25 (1e-3f against 1e-3), half of it on the scale, per BN
ORACLE_VAR_DRIFT = 0.5 * (2.0 ** -25 + 2e-10)


def expected_logits(desc, weights, planes):
    """oracle/nn_ref.forward(oracle_weights(weights), logits=True) snapped to the lattice unit
    2^lattice_exponent; the snap must move nothing by more than 1e-5 units.  Also asserts that the
    oracle on the float32 vars as they are is the same net: within the drift of its var + 1e-3 over
    the deepest chain of BNs, relative to the largest logit.  [policy_0, .., value] float64.

    Squeeze-excite nets: the expected logits are the walk's (_forward: gates as classes, which
    asserts that every gate is saturated), which must lie on the lattice as they are; nn_ref.forward,
    whose float64 sigmoid makes a "0" gate about 1e-100 and whose channel means round where the
    position count is no power of two, must agree with them within the same 1e-5 units."""
    unit = 2.0 ** lattice_exponent(desc, weights, planes)
    with np.errstate(over="ignore"):      # (a saturated "0" gate: exp(K hid) is inf in float64 too)
        plain = nn_ref.forward(desc, weights, planes, logits=True)
        exact = nn_ref.forward(desc, oracle_weights(weights), planes, logits=True)
    depth = 2 * desc.residual_layers + 2
    walk = _forward(desc, weights, planes)[0] if desc.se_units else None
    out = []
    for i, (z, zp) in enumerate(zip(exact, plain)):
        q = np.rint(z / unit)
        moved = float(np.abs(z / unit - q).max())
        assert moved <= 1e-5, ("the oracle is %.3g units of %g off the lattice" % (moved, unit))
        if walk is not None:
            assert np.array_equal(np.rint(walk[i] / unit) * unit, walk[i]), "the walk of an SE net left the lattice"
            assert np.array_equal(q * unit, walk[i]), ("nn_ref.forward and the walk disagree", float(np.abs(z - walk[i]).max() / unit))
        out.append(q * unit)
        assert np.abs(zp - z).max() <= 8 * depth * ORACLE_VAR_DRIFT * np.abs(z).max(), (np.abs(zp - z).max(), np.abs(z).max())
    return out


def trunk_alive(desc, weights, planes):
    """The fraction of the final trunk activations that are nonzero."""
    _, x = _forward(desc, weights, planes)
    return float(np.count_nonzero(x)) / x.size


# ---- the conditions -----------------------------------------------------------------------------
def check_representable(desc, weights, planes, mode):
    """Asserts the conditions under which the forward of `mode` on these weights and planes is exact
    (walking the net with the oracle's own pieces, v1 and v2):

    * every trunk conv's BN-folded weights and inputs have at most MODE_BITS[mode] significant bits;
    * three-part modes drop lo x lo: per conv, every folded weight or every input fits the hi part
      (HI_BITS[mode]);
    * per output, sum |w x| + |bias| + |skip| < 2^24 units of the output's lattice, so fp32 partial
      sums are exact in any order, grouping or fusion; the same for the v2 pre-activations;
    * the heads' 1 x 1 convs and the Denses are fp32 from the fp32 stream: 24 bits, same sums; the
      policy Dense where policy_gemm_kernel runs it (largest policy >= 512 outside fp32-ieee and
      fp16x3-layered; on nets with fused heads this is stricter than needed): 16 bits, one side
      within 8;
    * fp16x3-layered: folded weights within fp16's range and clear of its subnormals; within one
      board the largest and the smallest nonzero |input| of a conv less than 2^20 apart, so that
      with the board's exponent (layered_forward.h board_exponent: the largest lies in [2^14, 2^15))
      hi parts and the scaled lo parts stay clear of fp16's subnormals;
    * a pooling value head only where the position count is a power of two;
    * squeeze-excite: every gate is a class (the walk refuses an unsaturated one) and every nonzero
      |z| >= 2 ZSAT; the gating matrix has at most one power of two per channel, some channel reads
      the last unit (and, S > 64, a unit >= 64); every channel sum fits 24 bits of its board's
      lattice; the gated add s + u g, with u / 2 counted on its own lower lattice, stays below 2^24
      units.  Position count a power of two: the means, both Denses' sums of |terms| and hid K fit
      24 bits too, so the gate path is exact in any order, and some hidden unit that a gate reads
      lies within one lattice step of 0 (returned: [(name, board, unit)]).  Otherwise: no unit that
      a gate reads is within twice the float32 error bound of 0 (se_fragile_units).
    """
    bits, hi = MODE_BITS[mode], HI_BITS.get(mode)
    w = dict(weights)
    gemm_mode = mode not in ("fp32-ieee", "fp16x3-layered")

    def sums(name, inp, kf, bi, skip, conv):
        a = np.abs(inp)
        s = (nn_ref._conv_same(a, np.abs(kf)) if conv else a @ np.abs(kf)) + np.abs(bi)
        if skip is not None:
            s = s + np.abs(skip)
        ek, eb = lsb_exp(kf), lsb_exp(bi)
        for b in range(inp.shape[0]):      # a board's sums are its own: so is its lattice
            e = _emin(_eadd(lsb_exp(inp[b]), ek), eb, lsb_exp(skip[b]) if skip is not None else None)
            if e is not None:
                assert s[b].max() < 2.0 ** (ACC_BITS + e), (mode, name, b, "sum of |terms| %.6g reaches 2^24 units of %g" % (s[b].max(), 2.0 ** e))

    def two_sided(name, what, kf, inp, full, part):
        bw, bx = sig_bits(kf), sig_bits(inp)
        assert bw <= full, (mode, name, "%s weights need %d bits, the mode has %d" % (what, bw, full))
        assert bx <= full, (mode, name, "%s inputs need %d bits, the mode has %d" % (what, bx, full))
        if part is not None:
            assert bw <= part or bx <= part, (mode, name, "lo x lo is dropped: weights %d bits, inputs %d, hi part %d" % (bw, bx, part))

    near_zero = []      # SE, power-of-two boards: (name, board, unit) of fed units within a lattice step of 0

    def se(name, u, w1, w2, info, t):
        npos, sums, hid, prod, z, gate = (info[s] for s in ("npos", "sums", "hid", "prod", "z", "gate"))
        assert np.isin(gate, (0.0, 0.5, 1.0)).all()
        assert ((w2 != 0).sum(axis=0) <= 1).all() and sig_bits(w2) <= 1, (name, "gating: one power of two per channel at most")
        fed = (w2 != 0).any(axis=1)
        assert np.abs(z[(prod != 0).any(axis=1)]).min() >= 2 * ZSAT, (name, "a nonzero z below 2 ZSAT")
        pow2 = sig_bits(float(npos)) == 1
        eu = [lsb_exp(u[b]) for b in range(u.shape[0])]
        for b, e in enumerate(eu):
            if e is None:
                continue
            # the channel sums are exact in any order, on every board
            assert np.abs(u[b]).sum(axis=(0, 1)).max() < 2.0 ** (ACC_BITS + e), (mode, name, b, "channel sums")
            mean = sums[b] / npos
            terms = np.abs(w1 * mean[:, None])                    # [F, S]
            if pow2:
                # means, both Denses' partial sums and hid K: 24 bits in any summation order
                em = e - int(np.log2(npos))
                assert np.array_equal(np.ldexp(sums[b], -int(np.log2(npos))), mean)
                assert terms.sum(axis=0).max() < 2.0 ** (ACC_BITS + em + lsb_exp(w1)), (mode, name, b, "compress sums")
                eh = lsb_exp(hid[b])
                if eh is not None:
                    assert np.abs(prod[b]).sum(axis=0).max() < 2.0 ** (ACC_BITS + eh + lsb_exp(w2)), (mode, name, b, "gating sums")
                    assert sig_bits(prod[b]) <= ACC_BITS
                near_zero.extend((name, b, int(j)) for j in np.nonzero(fed & (np.abs(sums[b] @ w1) <= 2.0 ** e))[0])
            else:
                bad = se_fragile_units(sums[b], w1, npos) & fed
                assert not bad.any(), (mode, name, b, "hidden units %s are within the float32 error of 0" % np.nonzero(bad)[0])
            ug = u[b] * gate[b][None, None, :]
            ea = _emin(lsb_exp(t[b]), lsb_exp(ug))
            if ea is not None:
                assert (np.abs(t[b]) + np.abs(ug)).max() < 2.0 ** (ACC_BITS + ea), (mode, name, b, "the gated add")

    def tap(kind, name, inp, k, bn, skip):
        if kind == "se":
            return se(name, inp, k[0], k[1], bn, skip)
        if kind == "pool":
            assert sig_bits(float(desc.hw)) == 1, (name, "1 / %d is not a power of two" % desc.hw)
            s = np.abs(inp).sum(axis=(1, 2))
            e = lsb_exp(inp)
            assert e is None or s.max() < 2.0 ** (ACC_BITS + e), (mode, "pooled sum")
            return
        if kind == "affine":
            sc, bi = _fold64(w, None, bn)
            e = _emin(_eadd(lsb_exp(inp), lsb_exp(sc)), lsb_exp(bi))
            s = np.abs(inp) * np.abs(sc) + np.abs(bi)
            assert e is None or s.max() < 2.0 ** (ACC_BITS + e), (mode, name, "pre-activation")
            return
        if kind in ("dense", "gemm"):
            if kind == "gemm" and gemm_mode:
                two_sided(name, "policy GEMM", k, inp, GEMM_BITS, GEMM_HI)
            else:
                two_sided(name, "Dense", k, inp, ACC_BITS, None)
            sums(name, inp, k, bn, None, False)
            return
        sc, bi = _fold64(w, name, bn)
        kf = k * sc
        assert np.array_equal((k.astype(np.float32) * sc.astype(np.float32)).astype(np.float64), kf), (name, "float32 fold")
        if kind == "head":
            two_sided(name, "head conv", kf, inp, ACC_BITS, None)
        else:
            two_sided(name, "conv", kf, inp, bits, hi)
            if mode == "fp16x3-layered":
                nz = np.abs(kf[kf != 0])
                assert nz.max() <= F16_MAX and lsb_exp(kf) >= -14, (name, "folded weights against fp16's range")
                a = np.abs(inp).reshape(inp.shape[0], -1)
                for b in range(a.shape[0]):
                    pos = a[b][a[b] > 0]
                    assert pos.size == 0 or pos.max() / pos.min() < 2.0 ** 20, (name, b, "input range within the board")
        sums(name, inp, kf, bi, skip, True)

    _forward(desc, weights, planes, tap=tap)
    if desc.se_units:
        S = desc.se_units
        for i in range(desc.residual_layers):
            reads = np.nonzero(w["res%d_se_gating" % i])[0]
            assert S - 1 in reads and (S <= 64 or (reads >= 64).any()), (i, "some channel must read the last unit, and a unit >= 64")
        if sig_bits(float(desc.hw)) == 1:
            assert near_zero, "no fed hidden unit sits at 0 or within one lattice step of it: a mean off by one count would not show"
    return near_zero


def se_fragile_units(sums, w1, npos):
    """Boards whose position count is no power of two: the mean is sum * fl32(1 / npos), so the
    hidden units carry a rounding error.  [S] bool: the units of one board (channel sums [F]) whose
    pre-activation does not exceed twice the float32 error bound
        (F + 2) 2^-24 sum_c |w1[c, j] mean_c|
    (fl32(1 / npos) and the product by it: 2 roundings; each product w1 mean: exact for +-1, at most 1;
    F - 1 additions, serial or in four partial sums; first order, hence "twice") although some term
    is nonzero: such a unit could come out with the wrong sign, or as +-tiny where the oracle has 0,
    and tiny * K is an unsaturated gate.  It must feed no channel."""
    F = w1.shape[0]
    mean = sums / npos
    mag = np.abs(w1 * mean[:, None]).sum(axis=0)
    pre = np.abs(sums @ w1) / npos
    return (mag > 0) & (pre <= 2.0 * (F + 2) * 2.0 ** -24 * mag)


def se_walk(desc, weights, planes, strict=True):
    """[(name, u, w1, w2, info)] per squeeze-excite block of the (clean) walk."""
    seen = []

    def tap(kind, name, inp, k, bn, skip):
        if kind == "se":
            seen.append((name, inp, k[0], k[1], bn))
    _forward(desc, weights, planes, tap=tap, se_strict=strict)
    return seen


def lattice_se_weights(desc, seed, planes, *, nnz, wmax, homogeneous=False):
    """lattice_weights for a squeeze-excite net on these planes, K and the muted units derived, not
    tuned: walks the net with K = 1 and gates by the sign of z; on boards whose position count is no
    power of two, mutes (zeroes the gating row of) every fed unit that se_fragile_units names on any
    board, until none is left; K is then the smallest power of two for which every nonzero oracle
    z has |z| >= 2 ZSAT = 256.  (Gates by sign are the saturated gates, so K changes no gate.)
    homogeneous: with zero_trunk_shifts, as the walks see them."""
    def make(K):
        w = lattice_weights(desc, seed, nnz=nnz, wmax=wmax, se={"K": K, "mute": mute})
        return zero_trunk_shifts(desc, w) if homogeneous else w
    mute = set()
    pow2 = sig_bits(float(desc.hw)) == 1
    for _ in range(8):
        w = make(1.0)
        walk = se_walk(desc, w, planes, strict=False)
        new = set()
        if not pow2:
            for i, (_, u, w1, w2, info) in enumerate(walk):
                fed = (w2 != 0).any(axis=1)
                for b in range(u.shape[0]):
                    new |= {(i, int(j)) for j in np.nonzero(se_fragile_units(info["sums"][b], w1, info["npos"]) & fed)[0]}
        if not new:
            break
        mute |= new
    else:
        raise AssertionError("muting fragile units did not settle")
    zmin = min(np.abs(info["z"][(info["prod"] != 0).any(axis=1)]).min() for _, _, _, _, info in walk)
    K = 2.0 ** int(np.ceil(np.log2(2 * ZSAT / zmin)))
    return make(K)


def se_liveness(desc, weights, planes):
    """Per squeeze-excite block, on the oracle alone: (the shares of the (board, channel) pairs whose
    gate is 0, 1/2 and 1, the smallest number of channels in which two boards' gates differ)."""
    out = []
    for _, _, _, _, info in se_walk(desc, weights, planes):
        g = info["gate"]
        diff = min([int((g[a] != g[b]).sum()) for a in range(len(g)) for b in range(a)] or [g.shape[1]])
        out.append(([float((g == v).mean()) for v in (0.0, 0.5, 1.0)], diff))
    return out


def faulty_se_logits(desc, weights, planes, fault):
    """The logits of a forward whose squeeze-excite slips the way a wrong kernel would (oracle side
    only): boards 2k and 2k + 1 exchange gate vectors; the gate vector rotated by a lane group (4) or a
    co tile (16); block 1 with block 0's compress and gating matrices; the last hidden unit dropped;
    negative hidden values passed; (s + u) g for s + u g; one position's value left out of one
    channel's sum (in the block and board whose fed hidden unit is nearest 0, at the position and
    channel that move it furthest towards or across 0)."""
    assert fault in SE_FAULTS, fault
    f = (fault,)
    if fault == "mean_one_count":
        best = None
        for i, (_, u, w1, w2, info) in enumerate(se_walk(desc, weights, planes)):
            fed = np.nonzero((w2 != 0).any(axis=1))[0]
            for b in range(u.shape[0]):
                e = lsb_exp(u[b])
                if e is None:
                    continue
                d = np.abs(info["sums"][b] @ w1[:, fed]) / 2.0 ** e
                j = int(np.argmin(d))
                if best is None or d[j] < best[0]:
                    best = (float(d[j]), i, b, int(fed[j]))
        f = (fault,) + best[1:]
    return _forward(desc, weights, planes, se_fault=f)[0]


# ---- faults, on the oracle side only ------------------------------------------------------------------
FAULTS = ("tap_swap", "wrap_pad", "channel_swap", "drop_last_channel", "lo_weights", "lo_inputs")


def faulty_logits(desc, weights, planes, fault, conv, bits=8):
    """The logits of a forward whose conv `conv` slips the way a wrong kernel or packer would:
    two taps swapped, wrap-around for zero padding along the left border, two input channels
    swapped, the last input channel dropped, the weights' / the inputs' lo part lost (the operand
    rounded to `bits` significant bits)."""
    def hook(inp, k):
        k = k.copy()
        if fault == "tap_swap":
            k[[0, k.shape[0] - 1], [0, k.shape[1] // 2]] = k[[k.shape[0] - 1, 0], [k.shape[1] // 2, 0]]
        elif fault == "channel_swap":
            a, b = int(np.argmax((k != 0).sum(axis=(0, 1, 3))[:-1])), k.shape[2] - 1   # the busiest and the last
            k[:, :, [a, b]] = k[:, :, [b, a]]
        elif fault == "drop_last_channel":
            k[:, :, -1] = 0.0
        elif fault == "lo_weights":
            k = round_bits(k, bits)
        elif fault == "lo_inputs":
            inp = round_bits(inp, bits)
        else:
            assert fault == "wrap_pad", fault
        return inp, k, fault == "wrap_pad"
    return _forward(desc, weights, planes, hooks={conv: hook})[0]


# ---- the input path: plane staging, im2col, the initial conv ---------------------------------------------
def input_planes(desc, n, seed):
    """[n, C, H, W] float32 planes of 0 / 1, every cell of every plane set with probability 1/2 on its
    own (random_planes leaves whole planes of a board empty, and a place of the initial conv that
    reads an empty plane cannot show); the last cell of every board is set, so that the last float4
    of its plane block holds something."""
    rng = np.random.default_rng([seed, 31])
    x = (rng.random((n, desc.input_channels, desc.input_columns, desc.input_rows)) < 0.5).astype(np.float32)
    x[:, -1, -1, -1] = 1.0
    return x


def initial_places(desc):
    """[(tap, plane)] of the initial conv in the order of the im2col row's k = tap * C + plane."""
    return [(t, c) for t in range(desc.initial_kernel ** 2) for c in range(desc.input_channels)]


def initial_k0(desc):
    """The im2col row's length: the places rounded up to the initial GEMM's k-step of 32."""
    return (len(initial_places(desc)) + 31) // 32 * 32


def initial_liveness(desc, weights, planes):
    """The (tap, plane) places of the initial conv whose removal -- every weight of the place set to
    zero -- moves no expected logit on these planes: what a slip confined to that place could do
    unseen.  Empty: the comparison sees the whole initial conv.  (A place that no weight reads is
    dead by definition.)"""
    base = _forward(desc, weights, planes)[0]
    k0 = dict(weights)["initial_conv"]
    dead = []
    for j, place in enumerate(initial_places(desc)):
        k = k0.copy()
        k.reshape(-1, k.shape[3])[j] = 0.0
        if np.array_equal(k, k0):
            dead.append(place)
            continue
        got = _forward(desc, [(n, k if n == "initial_conv" else a) for n, a in weights], planes)[0]
        if all(np.array_equal(g, b) for g, b in zip(got, base)):
            dead.append(place)
    return dead


def _im2col(desc, planes):
    """The initial conv as the kernels run it: (rows [N, npos, K0] with k = tap * C + plane, zero
    beyond the places and at off-board taps; the weights as [K0, F] taken from `k`, by a function)."""
    N, C, H, W = planes.shape
    ks = desc.initial_kernel
    pad = ks // 2
    xp = np.pad(planes.astype(np.float64), ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    taps = [np.transpose(xp[:, :, dy:dy + H, dx:dx + W], (0, 2, 3, 1)).reshape(N, H * W, C) for dy in range(ks) for dx in range(ks)]
    im = np.concatenate(taps, axis=2)
    K0 = initial_k0(desc)
    im = np.pad(im, ((0, 0), (0, 0), (0, K0 - im.shape[2])))

    def matrix(k):
        return np.pad(k.astype(np.float64).reshape(-1, k.shape[3]), ((0, K0 - ks * ks * C), (0, 0)))
    return im, matrix


INPUT_FAULTS = ("swizzle_spill", "chunk_swap", "drop_tail_float4", "neighbour_board_planes", "shifted_row", "pad_reads_next_tap")


def input_fault_applies(desc, fault, rows):
    """Where the geometry lets an input fault occur: the old swizzle spills only where some chunk
    index XORed with a position's low bits leaves the row; a neighbour's planes need a second board; padded k exist only where
    the places are no multiple of 32.  The others occur everywhere."""
    assert fault in INPUT_FAULTS, fault
    nch = initial_k0(desc) // 8
    if fault == "swizzle_spill":      # (no power of two, and no multiple of 16 either: 12, 20, 24, 28, 36 chunks of the sweep)
        m = min(nch, 16) - 1
        return any(j ^ (p & m) >= nch for j in range(nch) for p in range(16))
    if fault == "neighbour_board_planes":
        return rows >= 2
    if fault == "pad_reads_next_tap":
        return initial_k0(desc) > len(initial_places(desc))
    return True


def faulty_input_logits(desc, weights, planes, fault, offset=None):
    """The logits of a forward whose input path slips the way a wrong kernel would (oracle side only):
      swizzle_spill          forward_kernel.h's first chunk swizzle, restated: chunk j of position p's
                             im2col row lies at chunk j ^ (p & (min(chunks, 16) - 1)) of the row; where
                             that leaves the row it lands in position p + 1's row, and what is read
                             back there is the chunk that position p + 1 itself put in that slot
                             (behind the last position: the zero row)
      chunk_swap             chunk 0 and the last chunk that holds a place (if that is chunk 0: chunk 1) change places in every row
      drop_tail_float4       the last four floats of every board's plane block read as zero
      neighbour_board_planes boards 2k + 1 read board 2k's planes (a workgroup's second board, the first's)
      shifted_row            every board's plane block is read from its address rounded down to 16
                             bytes, the launch's planes lying `offset` floats (default 1) behind a
                             16-byte boundary, with zeros in front
      pad_reads_next_tap     the row's padding k = places .. K0 - 1 holds the row's first entries over
                             again instead of zeros, and the weights there are +1 (towards channel
                             k mod F) instead of zero"""
    assert fault in INPUT_FAULTS, fault
    N = planes.shape[0]
    block = planes[0].size
    x = planes.astype(np.float64).copy()
    if fault == "drop_tail_float4":
        x.reshape(N, -1)[:, -4:] = 0.0
    elif fault == "neighbour_board_planes":
        x[1::2] = x[0:N - 1:2][:len(x[1::2])]
    elif fault == "shifted_row":
        off = 1 if offset is None else offset
        flat = np.concatenate([np.zeros(off), x.reshape(-1), np.zeros(4)])
        x = np.stack([flat[(off + b * block) // 4 * 4:][:block] for b in range(N)]).reshape(x.shape)
    im, matrix = _im2col(desc, x)
    nch, places = im.shape[2] // 8, len(initial_places(desc))

    def hook(inp, k):
        w0 = matrix(k)
        assert fault in ("drop_tail_float4", "neighbour_board_planes", "shifted_row") or np.array_equal(im @ w0, nn_ref._conv_same(inp, k).reshape(N, -1, k.shape[3]))
        rows = im
        if fault == "swizzle_spill":
            m = min(nch, 16) - 1
            npos = im.shape[1]
            ch = np.concatenate([im, np.zeros((N, 1, im.shape[2]))], axis=1).reshape(N, npos + 1, nch, 8)
            rows = np.zeros((N, npos, nch, 8))
            for p in range(npos):
                for j in range(nch):
                    at = j ^ (p & m)
                    theirs = (at - nch) ^ ((p + 1) & m)      # the chunk position p + 1 keeps in that slot
                    if at >= nch and p + 1 == npos:
                        rows[:, p, j] = 0.0
                    else:
                        rows[:, p, j] = ch[:, p + 1, theirs] if (at >= nch and theirs < nch) else ch[:, p, j]
            rows = rows.reshape(im.shape)
        elif fault == "chunk_swap":
            b = (places - 1) // 8
            a = 0 if b else 1       # (a single chunk of places: with the padding chunk behind it)
            rows = im.reshape(N, -1, nch, 8).copy()
            rows[:, :, [a, b]] = rows[:, :, [b, a]]
            rows = rows.reshape(im.shape)
        elif fault == "pad_reads_next_tap":
            rows, w0 = im.copy(), w0.copy()
            rows[:, :, places:] = im[:, :, :im.shape[2] - places]
            w0[np.arange(places, im.shape[2]), np.arange(places, im.shape[2]) % k.shape[3]] = 1.0
        return inp, k, False, (rows @ w0).reshape(N, desc.input_columns, desc.input_rows, k.shape[3])
    return _forward(desc, weights, x.astype(np.float32), hooks={"initial_conv": hook})[0]


# ---- the dense heads: faults on the oracle side only -------------------------------------------------
HEAD_FAULTS = ("role_features_slip", "logit_offset_padding", "dense_row_stride", "drop_last_group4", "drop_last_tile16",
               "drop_last_k", "drop_last_hidden", "bias_from_other_role", "value_swap")


def head_last_rows(desc, weights):
    """The same weights with the last row of every head Dense made to count, without a random draw
    (the generator's sparse Denses seldom reach it): policy r's last output reads the last of its
    features, the last value hidden unit reads the last value feature, and every value output reads
    the last hidden unit -- each with a +1 where the generator left a 0.  A dropped last k, a dropped
    last hidden unit or a Dense whose padded last k-tile is misread then has something to lose."""
    out = []
    for name, a in weights:
        if name.endswith("_dense") and name.startswith("policy") or name == "value_hidden":
            a = a.copy()
            a[-1, -1] = a[-1, -1] or 1.0
        elif name == "value_dense":
            a = a.copy()
            a[-1] = np.where(a[-1] == 0, 1.0, a[-1])
        out.append((name, a))
    return out


def head_operands(desc, weights, planes):
    """{Dense name: (inputs [N, K], kernel [K, n], bias [n])} of the clean walk, float64."""
    seen = {}

    def tap(kind, name, inp, k, bn, skip):
        if kind in ("dense", "gemm"):
            seen[name] = (inp, k, bn)
    _forward(desc, weights, planes, tap=tap)
    return seen


def head_fault_roles(desc, weights, fault):
    """The outputs (role indices; role_count: the value output) that a head fault touches on this net,
    from the geometry and the weights alone; [] where the fault cannot occur:
      role_features_slip, bias_from_other_role   roles 1.. of a net with at least two roles
      logit_offset_padding   roles behind one whose P is no multiple of 4 (elsewhere P and P4 offsets agree)
      dense_row_stride, drop_last_group4   roles whose P is no multiple of 4 (elsewhere P4 = P, no partial group)
      drop_last_tile16       every role
      drop_last_k            roles whose Dense reads its last feature (head_last_rows: all), and the value output
      drop_last_hidden       the value output
      value_swap             the value output of a net with at least two values"""
    R, P = desc.role_count, list(desc.policy_dist_count)
    assert fault in HEAD_FAULTS, fault
    if fault in ("role_features_slip", "bias_from_other_role"):
        return list(range(1, R))
    if fault == "logit_offset_padding":
        return [r for r in range(1, R) if any(p % 4 for p in P[:r])]
    if fault in ("dense_row_stride", "drop_last_group4"):
        return [r for r in range(R) if P[r] % 4]
    if fault == "drop_last_tile16":
        return list(range(R))
    w = dict(weights)
    if fault == "drop_last_k":
        return [r for r in range(R) if w["policy%d_dense" % r][-1].any()] + ([R] if w["value_hidden"][-1].any() else [])
    if fault == "drop_last_hidden":
        return [R] if w["value_dense"][-1].any() else []
    return [R] if desc.num_values >= 2 else []


def faulty_head_logits(desc, weights, planes, fault):
    """The logits of a forward whose dense heads slip the way a wrong kernel or packer would (oracle
    side only; the trunk and the heads' 1 x 1 convs are the clean walk's):
      role_features_slip     role r reads role r - 1's features
      logit_offset_padding   the boards' logit rows are laid out with one padding (every role's P rounded
                             up to 4, as in the LDS row; or none, as in the policy GEMM's scratch) and
                             read back with the other's offsets; padding holds 0, as does what lies past
                             the last board
      dense_row_stride       the Dense weights, stored [K][P4], are read with a row stride of P
      drop_last_group4       the outputs of the last partial group of 4 are never written (0)
      drop_last_tile16       the outputs of the last tile of 16 are never written (0)
      drop_last_k            the last feature of every policy Dense and of the value hidden Dense is left out
      drop_last_hidden       the last value hidden unit is left out of the value Dense
      bias_from_other_role   role r's bias of column j is role r - 1's (column j mod its P)
      value_swap             value outputs 0 and 1 change places"""
    assert fault in HEAD_FAULTS, fault
    R, P = desc.role_count, list(desc.policy_dist_count)
    ops = head_operands(desc, weights, planes)
    pol = [ops["policy%d_dense" % r] for r in range(R)]
    outs = [x @ k + b for x, k, b in pol]
    xh, kh, bh = ops["value_hidden"]
    xv, kv, bv = ops["value_dense"]
    value = xv @ kv + bv
    N = planes.shape[0]
    if fault == "role_features_slip":
        outs = [outs[0]] + [pol[r - 1][0] @ pol[r][1] + pol[r][2] for r in range(1, R)]
    elif fault == "logit_offset_padding":
        P4 = [(p + 3) & ~3 for p in P]
        for stored, read in ((P4, P), (P, P4)):
            buf = np.zeros((N + 1) * sum(stored))
            for r in range(R):
                for b in range(N):
                    at = b * sum(stored) + sum(stored[:r])
                    buf[at:at + P[r]] = outs[r][b]
            got = [np.stack([buf[b * sum(stored) + sum(read[:r]):][:P[r]] for b in range(N)]) for r in range(R)]
            if stored is P4:
                lds = got
        # (either direction of the slip: the one shown is the LDS row's, read with the GEMM scratch's offsets,
        # unless only the other moves something)
        outs = lds if any(not np.array_equal(a, b) for a, b in zip(lds, outs)) else got
    elif fault == "dense_row_stride":
        for r in range(R):
            x, k, b = pol[r]
            kp = np.zeros((k.shape[0], (P[r] + 3) & ~3))
            kp[:, :P[r]] = k
            outs[r] = x @ kp.reshape(-1)[:k.shape[0] * P[r]].reshape(k.shape[0], P[r]) + b
    elif fault in ("drop_last_group4", "drop_last_tile16"):
        g = 4 if fault == "drop_last_group4" else 16
        for r in range(R):
            if fault == "drop_last_tile16" or P[r] % g:
                outs[r] = outs[r].copy()
                outs[r][:, (P[r] - 1) // g * g:] = 0.0
    elif fault == "drop_last_k":
        outs = [x[:, :-1] @ k[:-1] + b for x, k, b in pol]
        hid = nn_ref._act(xh[:, :-1] @ kh[:-1] + bh, False)
        value = hid @ kv + bv
    elif fault == "drop_last_hidden":
        value = xv[:, :-1] @ kv[:-1] + bv
    elif fault == "bias_from_other_role":
        outs = [outs[0]] + [pol[r][0] @ pol[r][1] + pol[r - 1][2][np.arange(P[r]) % P[r - 1]] for r in range(1, R)]
    elif fault == "value_swap" and desc.num_values >= 2:
        value = value.copy()
        value[:, [0, 1]] = value[:, [1, 0]]
    return outs + [value]


def head_liveness(expected):
    """What the expected logits of a launch must be for the comparison with a device buffer to mean
    something, as a list of violations (empty: alive): every output of every row holds a nonzero
    entry; no two rows of the launch are equal in any output; every policy column and every value
    output is nonzero in some row (an output that is identically 0 would pass against an untouched
    buffer)."""
    bad = []
    for i, z in enumerate(expected):
        if not (z != 0).any(axis=1).all():
            bad.append((i, "a row of zeros"))
        if len(np.unique(z, axis=0)) != len(z):
            bad.append((i, "two equal rows"))
        if not (z != 0).any(axis=0).all():
            bad.append((i, "%d columns that are 0 in every row" % int((~(z != 0).any(axis=0)).sum())))
    return bad
