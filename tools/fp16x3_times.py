#!/usr/bin/env python
"""Forward time of "fp16x3-layered" against fp32-ieee (whose accuracy class it shares), against
bf16x3-layered (whose layer loop and MFMA count it shares) and against the fused bf16x3.

Per net (1,024 rows) every mode's net is built once and the modes take turns, forward by forward, in
one process: the median of --reps forwards per mode after --warmup warm-up rounds (device time of the
forward's kernels between two HIP events, HipNet.last_kernel_ms), min in brackets.
  19x19 v1 4 x 256   fp16x3-layered, bf16x3-layered, fp32-ieee.  Accepted when fp16x3-layered <=
                     0.5 x fp32-ieee, the layered modes' own target.  fp16x3-layered / bf16x3-layered
                     is the price of the exponent pass and the second accumulator set: recorded.
  cfg2's 8x8 6 x 128, cfg4's 13x13 12 x 256   fp16x3-layered against fp32-ieee and the fused bf16x3:
                     recorded, no threshold.
--only MODE runs the 19 x 19 net in that mode alone (for a kernel trace: board_exp_kernel's share of
the forward is its share of the trace's kernel time).

    python tools/fp16x3_times.py [--device 0] [--rows 1024] [--reps 20] [--warmup 5] [--only MODE]
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
MODE = "fp16x3-layered"


def alternate(desc, modes, args):
    """{mode: (median ms, min ms, kernel name)} with the modes taking turns."""
    blob = to_blob(random_weights(desc, 7919, bias_std=0.2, res_gamma=0.3))
    x = random_planes(desc, args.rows, 11)
    nets = {}
    for m in modes:
        nets[m] = HipNet(desc, args.device, m)
        nets[m].set_weights(blob)
    ms = {m: [] for m in modes}
    for i in range(args.warmup + args.reps):
        for m in modes:
            nets[m].forward(x)
            if i >= args.warmup:
                ms[m].append(nets[m].last_kernel_ms())
    out = {m: (float(np.median(ms[m])), float(np.min(ms[m])), nets[m].kernel_name(True)) for m in modes}
    for n in nets.values():
        n.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    print("rows %d, median of %d forwards per mode after %d warm-ups, modes alternating (min in brackets), ms" %
          (args.rows, args.reps, args.warmup))
    desc = NetDesc(5, 19, 19, 256, 4, [362, 362])
    flops = desc.flops_per_eval() * args.rows
    if args.only:
        med, mn, name = alternate(desc, [args.only], args)[args.only]
        print("19x19 v1 4x256  %-15s %8.4f (%8.4f)  %s" % (args.only, med, mn, name))
        return 0
    t = alternate(desc, [MODE, "bf16x3-layered", "fp32-ieee"], args)
    for p, (med, mn, name) in t.items():
        print("19x19 v1 4x256  %-15s %8.4f (%8.4f)  %6.1f TFLOP/s (model flops)  %s" % (p, med, mn, flops / med * 1e-9, name))
    ratio = t[MODE][0] / t["fp32-ieee"][0]
    print("19x19 v1 4x256  fp16x3-layered / fp32-ieee %.3f (target <= %.2f)  fp16x3-layered / bf16x3-layered %.3f" %
          (ratio, TARGET, t[MODE][0] / t["bf16x3-layered"][0]))
    sys.stdout.flush()
    for tag, d in (("cfg2 8x8 6x128", BASELINE_CONFIGS[2]["desc"]), ("cfg4 13x13 12x256", BASELINE_CONFIGS[4]["desc"])):
        u = alternate(d, [MODE, "fp32-ieee", "bf16x3"], args)
        print("%-18s fp16x3-layered %8.4f (%8.4f)  fp32-ieee %8.4f (%8.4f)  bf16x3 %8.4f (%8.4f)  / fp32-ieee %.3f  / bf16x3 %.2f" %
              (tag, u[MODE][0], u[MODE][1], u["fp32-ieee"][0], u["fp32-ieee"][1], u["bf16x3"][0], u["bf16x3"][1],
               u[MODE][0] / u["fp32-ieee"][0], u[MODE][0] / u["bf16x3"][0]))
        sys.stdout.flush()
    print("verdict: fp16x3-layered <= %.2f x fp32-ieee at 19x19 v1 4x256: %s" % (TARGET, "yes" if ratio <= TARGET else "NO"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
