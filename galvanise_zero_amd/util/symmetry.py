"""Index tables of a game's board symmetries, from its descriptor (defs/symmetries.py) and the
state machine's base and action names alone -- no per-game code.

The group a descriptor generates: the identity first, then in the order of the reference's
Prescription (src/ggpzero/util/symmetry.py:227-253) -- quarter turns 0..3 (or the half turn: 0, 2)
without, then with, the reflection.  A coordinate pair (x, y) of x_cords / y_cords indices (i, j) maps,
as there (:4-20), by the reflection to (W - 1 - i, j) and by one anti-clockwise quarter turn to
(j, W - 1 - i); the half turn is two quarter-turn steps taken per axis, (W - 1 - i, H - 1 - j), which
needs no square board.

Per element s (SymmetryTables):
  base_perm[s][b]     base b of a state is base base_perm[s][b] of the transformed state
  move_src[r][s][m]   move m of role r is move move_src[r][s][m] in the transformed position
  plane_src[s][i]     the transformed position's planes are X_s[i] = X[plane_src[s][i]]
so a network's policy for the transformed position, read at move_src[r][s][m], is its opinion of move
m in the original -- what gz_net_forward_sym (include/gzero_nn.h) averages.
"""
import numpy as np

from ..nn.bases import parse_terms


class SymmetryError(ValueError):
    pass


class SymmetryTables(object):
    """count elements, the identity first.  elements[s] = (reflect, quarter_turns)."""

    def __init__(self, elements, base_perm, move_src, plane_src):
        self.elements = list(elements)
        self.count = len(self.elements)
        self.base_perm = np.ascontiguousarray(base_perm, dtype=np.int32)          # [S][num_bases]
        self.move_src = [np.ascontiguousarray(m, dtype=np.int32) for m in move_src]   # per role [S][P_r]
        self.plane_src = np.ascontiguousarray(plane_src, dtype=np.int32)          # [S][C * H * W]
        assert self.base_perm.shape[0] == self.plane_src.shape[0] == self.count
        assert all(m.shape[0] == self.count for m in self.move_src)

    @property
    def policy_sizes(self):
        return [m.shape[1] for m in self.move_src]

    def map_state_bits(self, s, bits):
        """bits (0/1 over the bases) of the position transformed by element s."""
        out = np.zeros(len(bits), dtype=np.int64)
        out[self.base_perm[s]] = np.asarray(bits, dtype=np.int64)
        return tuple(int(b) for b in out)


def group_elements(game_symmetries):
    """[(reflect, quarter_turns)], identity first (Prescription, symmetry.py:227-253)."""
    gs = game_symmetries
    if gs.do_rotations_90 and gs.do_rotations_180:
        raise SymmetryError("a descriptor asks for do_rotations_90 or do_rotations_180, not both")
    if gs.do_rotations_90 or gs.do_rotations_180:
        rots = (0, 2) if gs.do_rotations_180 else (0, 1, 2, 3)
        out = [(False, r) for r in rots]
        if gs.do_reflection:
            out += [(True, r) for r in rots]
        return out
    if gs.do_reflection:
        return [(False, 0), (True, 0)]
    return [(False, 0)]


def _map_xy(i, j, W, H, reflect, turns):
    if reflect:
        i = W - 1 - i
    if turns == 2:
        return W - 1 - i, H - 1 - j
    for _ in range(turns):       # (square boards only: checked by build_tables)
        i, j = j, W - 1 - i
    return i, j


def _as_list(v):
    return list(v) if isinstance(v, (list, tuple)) else [v]


def _translate(terms, apply, x_cords, y_cords, element, what):
    xs, ys = _as_list(apply.x_terms_idx), _as_list(apply.y_terms_idx)
    if len(xs) != len(ys):
        raise SymmetryError("%s: x_terms_idx %r and y_terms_idx %r differ in length" % (apply.base_term, xs, ys))
    out = list(terms)
    for xi, yi in zip(xs, ys):
        if max(xi, yi) >= len(terms):
            raise SymmetryError("%s %r has no term %d" % (what, " ".join(terms), max(xi, yi)))
        if terms[xi] not in x_cords or terms[yi] not in y_cords:
            raise SymmetryError("%s %r: terms %d, %d are not coordinates of the board" % (what, " ".join(terms), xi, yi))
        i, j = _map_xy(x_cords.index(terms[xi]), y_cords.index(terms[yi]), len(x_cords), len(y_cords), *element)
        out[xi], out[yi] = x_cords[i], y_cords[j]
    return tuple(out)


def _name_perm(names, applies, skips, x_cords, y_cords, element, what):
    """index -> index of the translated name, over one list of GDL names."""
    terms = [tuple(parse_terms(n)) for n in names]
    index = {t: i for i, t in enumerate(terms)}
    by_root = {a.base_term: a for a in applies}
    perm = np.empty(len(names), dtype=np.int32)
    for i, t in enumerate(terms):
        if t[0] in skips:
            perm[i] = i
            continue
        if t[0] not in by_root:
            raise SymmetryError("%s %r: the descriptor neither applies nor skips %r" % (what, names[i], t[0]))
        new = _translate(t, by_root[t[0]], x_cords, y_cords, element, what)
        if new not in index:
            raise SymmetryError("%s %r maps to %r, which the state machine does not have" % (what, names[i], " ".join(new)))
        perm[i] = index[new]
    check_permutation(perm, "%s table of element %r" % (what, element))
    return perm


def _fmix32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x85ebca6b)
    x = x ^ (x >> np.uint32(13))
    x = x * np.uint32(0xc2b2ae35)
    return x ^ (x >> np.uint32(16))


def pick_hashes(X):
    """The row hash h of csrc/nn/symmetry.h for every row of X (float32 [n, ...], read as the 32-bit
    patterns stored: -0.0 is not 0.0): sum over i of fmix(b_i + 0x9E3779B9 * (i + 1)) mod 2^32."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    bits = X.reshape(X.shape[0], -1).view(np.uint32)
    with np.errstate(over="ignore"):
        k = np.uint32(0x9E3779B9) * np.arange(1, bits.shape[1] + 1, dtype=np.uint32)
        return _fmix32(bits + k[None, :]).sum(axis=1, dtype=np.uint32)


def pick_elements(X, S, salt):
    """The table element g in [0, S) under which gz_net_forward_sym_pick evaluates each row of X:
    g = (uint64(fmix(h ^ salt)) * S) >> 32, the numpy statement of the GPU kernel's hash (the reference
    for tests and for oracle-side model wrappers).  Returns int32 [n]."""
    with np.errstate(over="ignore"):
        f = _fmix32(pick_hashes(X) ^ np.uint32(int(salt) & 0xFFFFFFFF))
    return ((f.astype(np.uint64) * np.uint64(S)) >> np.uint64(32)).astype(np.int32)


def pick_forward(forward, X, tables, salt):
    """The pick forward from a plain one, in numpy: `forward(X) -> [policy_0 .. policy_{R-1}, values]`
    applied to each row permuted by its element, the policies read back through move_src.  What
    gz_net_forward_sym_pick computes, for oracle-side wrappers and tests."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n = X.shape[0]
    plane_src, move_src = np.asarray(tables.plane_src), [np.asarray(m) for m in tables.move_src]
    g = pick_elements(X, plane_src.shape[0], salt)
    flat = X.reshape(n, -1)
    outs = forward(np.ascontiguousarray(np.take_along_axis(flat, plane_src[g], axis=1)).reshape(X.shape))
    return [np.ascontiguousarray(np.take_along_axis(o, move_src[r][g], axis=1)) for r, o in enumerate(outs[:-1])] + [outs[-1]]


def canonical_elements(X, tables, salt):
    """The table element g under which gz_net_forward_sym_canon evaluates each row of X, and the
    cache tag of that image (csrc/nn/symmetry.h, "canonical"): with X_s = X[plane_src[s]] and t_s its
    64-bit row tag (util.evalcache.tags -- the one numpy statement of the tag), g is the s with the
    smallest (mix64(t_s ^ salt), s).  `tables`: an object with plane_src [S][E], or that array.
    Returns (int32 [n], uint64 [n])."""
    from .evalcache import mix64, tags          # (evalcache imports this module)
    X = np.ascontiguousarray(X, dtype=np.float32)
    n = X.shape[0]
    flat = X.reshape(n, -1)
    plane_src = np.asarray(getattr(tables, "plane_src", tables))
    salt = int(salt) & 0xFFFFFFFF
    t = np.stack([tags(np.ascontiguousarray(flat[:, p])) for p in plane_src])        # [S][n]
    keys = np.array([[mix64(int(v) ^ salt) for v in row] for row in t], dtype=np.uint64).reshape(len(plane_src), n)
    g = np.argmin(keys, axis=0).astype(np.int32)                                      # (the first minimum: the lowest s)
    return g, t[g, np.arange(n)]


def canonical_planes(X, tables, salt):
    """Every row of X as its class's canonical image X[plane_src[g]], in X's shape."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    plane_src = np.asarray(getattr(tables, "plane_src", tables))
    g, _ = canonical_elements(X, plane_src, salt)
    return np.ascontiguousarray(np.take_along_axis(X.reshape(X.shape[0], -1), plane_src[g], axis=1)).reshape(X.shape)


def canonical_forward(forward, X, tables, salt):
    """The canonical forward from a plain one, in numpy, as pick_forward is the pick's: `forward`
    applied to each row's canonical image, the policies read back through move_src[r][g].  What
    gz_net_forward_sym_canon computes without a cache (and, the cache being exact, with one)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    move_src = [np.asarray(m) for m in tables.move_src]
    g, _ = canonical_elements(X, tables, salt)
    outs = forward(canonical_planes(X, tables, salt))
    return [np.ascontiguousarray(np.take_along_axis(o, move_src[r][g], axis=1)) for r, o in enumerate(outs[:-1])] + [outs[-1]]


def check_permutation(table, what):
    t = np.asarray(table)
    if t.ndim != 1 or not np.array_equal(np.sort(t), np.arange(len(t))):
        raise SymmetryError("%s is not a permutation" % what)


def _plane_src(transformer, base_perm, element):
    t = transformer
    size = t.channel_size
    per_state = t.raw_channels_per_state * size
    at = {b.base_indx: size * b.channel_id + b.y_idx * t.num_rows + b.x_idx for b in t.board_space}
    block = np.full(per_state, -1, dtype=np.int64)          # within one state's board channels
    for b, i in at.items():
        to = int(base_perm[b])
        if to not in at:
            raise SymmetryError("base %d has a board plane, its image %d under element %r has none" % (b, to, element))
        block[at[to]] = i
    free = np.flatnonzero(block < 0)                         # positions no base writes map to themselves
    block[free] = free
    check_permutation(block, "plane table of element %r" % (element,))
    out = np.arange(t.num_channels * size, dtype=np.int32)  # control planes: themselves
    for k in range(t.num_previous_states + 1):               # previous states move like the current one
        out[k * per_state:(k + 1) * per_state] = block + k * per_state
    return out


def build_tables(sm, transformer, game_symmetries):
    """SymmetryTables of the group `game_symmetries` generates, for state machine `sm` and the planes
    of `transformer` (nn/bases.py GdlBasesTransformer).  Raises SymmetryError for a descriptor that
    does not cover a base or an action, names a coordinate term a name does not have, maps a name
    to one the state machine lacks, asks for quarter turns on a board that is not square, or gives
    a table that is not a permutation."""
    x_cords, y_cords = list(transformer.x_cords), list(transformer.y_cords)
    if game_symmetries.do_rotations_90 and len(x_cords) != len(y_cords):
        raise SymmetryError("do_rotations_90 on a %d x %d board: quarter turns need a square board"
                            % (len(y_cords), len(x_cords)))
    elements = group_elements(game_symmetries)
    gs = game_symmetries
    base_names = [sm.base_name(i) for i in range(sm.num_bases)]
    action_names = [[sm.legal_to_move(r, a) for a in range(sm.action_count(r))] for r in range(sm.role_count)]
    base_perm, plane_src, move_src = [], [], [[] for _ in range(sm.role_count)]
    for e in elements:
        bp = _name_perm(base_names, gs.apply_bases, set(gs.skip_bases), x_cords, y_cords, e, "base")
        base_perm.append(bp)
        plane_src.append(_plane_src(transformer, bp, e))
        for r in range(sm.role_count):
            move_src[r].append(_name_perm(action_names[r], gs.apply_actions, set(gs.skip_actions), x_cords, y_cords, e,
                                          "action of role %d" % r))
    for what, tabs in [("base", base_perm), ("plane", plane_src)] + [("move", m) for m in move_src]:
        if not np.array_equal(tabs[0], np.arange(len(tabs[0]))):
            raise SymmetryError("the first %s table is not the identity" % what)
    return SymmetryTables(elements, np.array(base_perm), [np.array(m) for m in move_src], np.array(plane_src))


def tables_for_game(game, num_previous_states=1, game_symmetries=None):
    """State machine, transformer and GameSymmetries of `game` in one call: returns
    (tables, sm, transformer)."""
    from ..defs import symmetries, templates
    from ..nn.bases import GdlBasesTransformer
    from ..sm import get_sm
    if game_symmetries is None:
        if not hasattr(symmetries.GameSymmetries, game):
            raise SymmetryError("no symmetries described for game %r" % game)
        game_symmetries = getattr(symmetries.GameSymmetries(), game)()
    sm = get_sm(game)
    transformer = GdlBasesTransformer(sm, templates.default_generation_desc(game, num_previous_states=num_previous_states))
    return build_tables(sm, transformer, game_symmetries), sm, transformer
