"""Per-game board symmetries (reference src/ggpzero/defs/gamedesc.py:73-110 ApplySymmetry /
Symmetries, :497-593 GameSymmetries), for the games this package has state machines for: which GDL
bases and actions carry board coordinates (and at which term indices), which are left alone, and
which of reflection / quarter turns / the half turn the game is invariant under.
galvanise_zero_amd/util/symmetry.py turns a descriptor into index tables."""
import attr


@attr.s
class ApplySymmetry(object):
    base_term = attr.ib(default="cell")
    # indices of the terms holding the coordinates: an int, or a list of them (one per coordinate pair)
    x_terms_idx = attr.ib(factory=list)
    y_terms_idx = attr.ib(factory=list)


@attr.s
class Symmetries(object):
    apply_bases = attr.ib(factory=list)       # list of ApplySymmetry
    skip_bases = attr.ib(factory=list)        # list of root terms
    apply_actions = attr.ib(factory=list)     # list of ApplySymmetry
    skip_actions = attr.ib(factory=list)      # list of root terms
    do_reflection = attr.ib(default=False)    # x -> mirrored x
    do_rotations_90 = attr.ib(default=False)  # the four quarter turns (square boards)
    do_rotations_180 = attr.ib(default=False) # the half turn


class GameSymmetries(object):
    """A namespace, like defs.gamedesc.Games."""

    def breakthroughSmall(self):
        return Symmetries(skip_bases=["control"],
                          apply_bases=[ApplySymmetry("cell", 1, 2)],
                          skip_actions=["noop"],
                          apply_actions=[ApplySymmetry("move", [1, 3], [2, 4])],
                          do_reflection=True)

    def breakthrough(self):
        return Symmetries(skip_bases=["control"],
                          apply_bases=[ApplySymmetry("cellHolds", 1, 2)],
                          skip_actions=["noop"],
                          apply_actions=[ApplySymmetry("move", [1, 3], [2, 4])],
                          do_reflection=True)

    bt_7 = breakthrough

    def reversi(self):
        return Symmetries(skip_bases=["control"],
                          apply_bases=[ApplySymmetry("cell", 1, 2)],
                          skip_actions=["noop"],
                          apply_actions=[ApplySymmetry("move", 1, 2)],
                          do_rotations_90=True,
                          do_reflection=True)

    def hexLG13(self):
        return Symmetries(skip_bases=["control", "step", "owner", "canSwap"],
                          apply_bases=[ApplySymmetry("cell", 1, 2),
                                       ApplySymmetry("connected", 2, 3)],
                          skip_actions=["noop", "swap"],
                          apply_actions=[ApplySymmetry("place", 1, 2)],
                          do_rotations_180=True)

    def amazons_10x10(self):
        return Symmetries(skip_bases=["turn"],
                          apply_bases=[ApplySymmetry("cell", 1, 2),
                                       ApplySymmetry("justMoved", 1, 2)],
                          skip_actions=["noop"],
                          apply_actions=[ApplySymmetry("move", [1, 3], [2, 4]),
                                         ApplySymmetry("fire", 1, 2)],
                          do_rotations_90=True,
                          do_reflection=True)
