#!/usr/bin/env python
"""Forward time of the layered modes ("bf16-layered" / "bf16x3-layered") against fp32-ieee, the only
other mode that runs the nets they are for, and against the fused modes where those run.

Per net (1,024 rows): the median of --reps isolated forwards after --warmup warm-ups (device time of
the forward's kernels between two HIP events, HipNet.last_kernel_ms), min in brackets.
  19x19 v1 4 x 256   bf16x3-layered, bf16-layered, fp32-ieee.  Accepted when bf16x3-layered <=
                     0.5 x fp32-ieee and bf16-layered < bf16x3-layered (the split issues 3/16 of
                     fp32-ieee's MFMA time; conv_f32_kernel runs at 0.69 of its peak, so 0.5 asks the
                     bf16 conv for 0.26 of its own).
  cfg4's 13x13 12 x 256, cfg2's 8x8 6 x 128   layered against fused in both arithmetic classes: the
                     price of the activations crossing HBM between layers.  Recorded, no threshold.
One process on the GPU; prints one line per net and a verdict.

    python tools/layered_times.py [--device 0] [--rows 1024] [--reps 20] [--warmup 5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from galvanise_zero_amd._native import HipNet  # noqa: E402
from galvanise_zero_amd.nn.desc import BASELINE_CONFIGS, NetDesc  # noqa: E402
from galvanise_zero_amd.nn.weights import random_planes, random_weights, to_blob  # noqa: E402

TARGET = 0.5


def median_ms(desc, precision, args):
    net = HipNet(desc, args.device, precision)
    net.set_weights(to_blob(random_weights(desc, 7919, bias_std=0.2, res_gamma=0.3)))
    x = random_planes(desc, args.rows, 11)
    for _ in range(args.warmup):
        net.forward(x)
    ms = []
    for _ in range(args.reps):
        net.forward(x)
        ms.append(net.last_kernel_ms())
    name = net.kernel_name(True)
    net.close()
    return float(np.median(ms)), float(np.min(ms)), name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    print("rows %d, median of %d forwards after %d warm-ups (min in brackets), ms" % (args.rows, args.reps, args.warmup))
    desc = NetDesc(5, 19, 19, 256, 4, [362, 362])
    t = {p: median_ms(desc, p, args) for p in ("bf16x3-layered", "bf16-layered", "fp32-ieee")}
    flops = desc.flops_per_eval() * args.rows
    for p, (med, mn, name) in t.items():
        print("19x19 v1 4x256  %-15s %8.4f (%8.4f)  %6.1f TFLOP/s (model flops)  %s" % (p, med, mn, flops / med * 1e-9, name))
    ratio = t["bf16x3-layered"][0] / t["fp32-ieee"][0]
    faster = t["bf16-layered"][0] < t["bf16x3-layered"][0]
    print("19x19 v1 4x256  bf16x3-layered / fp32-ieee %.3f (target <= %.2f)  bf16-layered / bf16x3-layered %.3f" %
          (ratio, TARGET, t["bf16-layered"][0] / t["bf16x3-layered"][0]))
    sys.stdout.flush()
    for tag, d in (("cfg4 13x13 12x256", BASELINE_CONFIGS[4]["desc"]), ("cfg2 8x8 6x128", BASELINE_CONFIGS[2]["desc"])):
        for fused in ("bf16x3", "bf16"):
            a, b = median_ms(d, fused + "-layered", args), median_ms(d, fused, args)
            print("%-18s %-6s layered %8.4f (%8.4f)  fused %8.4f (%8.4f)  layered / fused %.2f" %
                  (tag, fused, a[0], a[1], b[0], b[1], a[0] / b[0]))
            sys.stdout.flush()
    ok = ratio <= TARGET and faster
    print("verdict: bf16x3-layered <= %.2f x fp32-ieee and bf16-layered faster than bf16x3-layered: %s" %
          (TARGET, "yes" if ok else "NO"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
