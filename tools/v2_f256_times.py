#!/usr/bin/env python
"""Forward time of the 256-filter v2 kernels against the v1 kernels of the same geometry.

Per cell (bf16 / bf16x3, 10 x 10 / 13 x 13, four residual blocks, 1,024 rows): the median of
--reps forwards after --warmup warm-ups (device time of the forward's kernels, HipNet.last_kernel_ms)
for v1 and v2 (no squeeze-excite) at 256 and at 128 filters, and the ratios
r256 = t(v2, 256) / t(v1, 256) and r128 = t(v2, 128) / t(v1, 128).  r128 is what the v2 epilogue
costs on the 128-filter kernels; the 256-filter kernels are accepted when r256 <= r128 + 0.05 in
every cell.  The cost of squeeze-excite (85 units at 256 filters) is reported beside them.
One process on the GPU; prints one line per cell and a verdict.

    python tools/v2_f256_times.py [--device 0] [--rows 1024] [--reps 20] [--warmup 5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from galvanise_zero_amd._native import HipNet  # noqa: E402
from galvanise_zero_amd.nn.desc import NetDesc  # noqa: E402
from galvanise_zero_amd.nn.weights import random_planes, random_weights, to_blob  # noqa: E402

BOARDS = {"10x10": (12, 10, 10, [3041, 3041]), "13x13": (5, 13, 13, [170, 171])}
BLOCKS = 4
MARGIN = 0.05


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
    net.close()
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    print("rows %d, %d blocks, median of %d forwards after %d warm-ups (min in brackets), ms" %
          (args.rows, BLOCKS, args.reps, args.warmup))
    ok = True
    for board, (C, H, W, pol) in BOARDS.items():
        for precision in ("bf16", "bf16x3"):
            t = {}
            for F in (256, 128):
                t["v1", F] = median_ms(NetDesc(C, H, W, F, BLOCKS, pol), precision, args)
                t["v2", F] = median_ms(NetDesc(C, H, W, F, BLOCKS, pol, resnet_v2=True), precision, args)
            t["se", 256] = median_ms(NetDesc(C, H, W, 256, BLOCKS, pol, resnet_v2=True, se_units=85), precision, args)
            r256 = t["v2", 256][0] / t["v1", 256][0]
            r128 = t["v2", 128][0] / t["v1", 128][0]
            cell_ok = r256 <= r128 + MARGIN
            ok = ok and cell_ok
            print("%s %-6s  v1/256 %.4f (%.4f)  v2/256 %.4f (%.4f)  v1/128 %.4f (%.4f)  v2/128 %.4f (%.4f)  | "
                  "r256 %.3f  r128 %.3f  r256 - r128 %+.3f  %s | v2/256 + SE 85 %.4f (%.4f): x%.3f of v2/256" %
                  ((board, precision) + t["v1", 256] + t["v2", 256] + t["v1", 128] + t["v2", 128] +
                   (r256, r128, r256 - r128, "ok" if cell_ok else "MISS") + t["se", 256] +
                   (t["se", 256][0] / t["v2", 256][0],)))
            sys.stdout.flush()
    print("verdict: r256 <= r128 + %.2f in every cell: %s" % (MARGIN, "yes" if ok else "NO"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
