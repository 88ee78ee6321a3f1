"""Records tests/golden/weight_image_sha256.json: the digests (tests/test_weight_roll_gpu.py
image_digest) of the device weight image the host path builds for every net of that module's NETS in
every precision.  Run it on the build whose images are the reference -- the parent commit's, through
GZ_LIB_DIR -- never on the code under test:
    GZ_LIB_DIR=<parent build>/lib python tools/record_weight_image_digests.py [OUT.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from galvanise_zero_amd._native import LIB_DIR, HipNet  # noqa: E402
from galvanise_zero_amd.nn.weights import random_weights, to_blob  # noqa: E402
from test_weight_roll_gpu import DIGESTS, NETS, PRECISIONS, image_digest  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else DIGESTS
print("libraries: %s" % LIB_DIR)
rec = {}
for name in sorted(NETS):
    blob = to_blob(random_weights(NETS[name], 7922, bias_std=0.2))
    for precision in PRECISIONS:
        net = HipNet(NETS[name], 0, precision)
        net.set_weights(blob)
        rec["%s/%s" % (name, precision)] = d = image_digest(net.weight_image())
        net.close()
        print("%s %s: %d bytes %s" % (name, precision, d["bytes"], d["sha256"]), flush=True)
with open(out, "w") as f:
    json.dump(rec, f, indent=0, sort_keys=True)
    f.write("\n")
