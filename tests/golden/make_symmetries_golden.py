"""Generates tests/golden/symmetries.json from the REFERENCE's own ggpzero.defs.gamedesc.

Run on the development machine only, with the reference's sources on the path:
    PYTHONPATH=<reference>/src python tests/golden/make_symmetries_golden.py

Regenerating executes the reference's module code (third-party, untrusted): run it only in an
isolated sandbox.  The committed symmetries.json is the pin; tests never
import the reference.

Records attr.asdict(GameSymmetries().<game>()) (gamedesc.py:73-110, 497-593) for the games this
package has state machines for: the bases and actions a board symmetry moves (root term and the
indices of their coordinate terms), the ones it leaves alone, and which of reflection / quarter
turns / half turn the game has.  galvanise_zero_amd/defs/symmetries.py restates them.
"""
import json
import os

import attr

from ggpzero.defs import gamedesc

HERE = os.path.dirname(os.path.abspath(__file__))
GAMES = ["breakthrough", "breakthroughSmall", "bt_7", "reversi", "hexLG13", "amazons_10x10"]


def main():
    g = gamedesc.GameSymmetries()
    out = {name: attr.asdict(getattr(g, name)()) for name in GAMES}
    with open(os.path.join(HERE, "symmetries.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", len(out), "symmetry descriptions")


if __name__ == "__main__":
    main()
