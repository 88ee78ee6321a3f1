#!/usr/bin/env python
"""Device time of the symmetry ensemble (gz_net_forward_sym_device) at the match player's launch
shape, against the plain forward, which is unchanged code and so the yardstick.

cfg2's net (8 x 8, 6 x 128) in bf16x3 and fp16x3-layered, n = 32 rows (PUCTPlayer's batch).  Per mode
one net, one stream and device buffers; the variants take turns, call by call, in one process:
  plain n          gz_net_forward_device of n rows
  plain n*S        gz_net_forward_device of n * S rows, S in {2, 8}: what the ensemble's inner forward costs
  sym S            gz_net_forward_sym_device of n rows with S in {1, 2, 8} elements (expand, inner
                   forward of n * S rows, reduce)
Each call is timed between two HIP events on the stream; the median of --reps calls per variant after
--warmup warm-up rounds, min in brackets.  The tables are random permutations: the kernels' work
does not depend on the tables being geometric.  Ratios: sym S / plain n (the price of the ensemble
to a player) and sym S / plain n*S (what expand and reduce add to the inner forward).

    python tools/sym_times.py [--device 0] [--rows 32] [--reps 200] [--warmup 20]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from galvanise_zero_amd._native import HipNet, HipSymmetry  # noqa: E402
from galvanise_zero_amd.nn.desc import BASELINE_CONFIGS  # noqa: E402
from galvanise_zero_amd.nn.weights import random_planes, random_weights, to_blob  # noqa: E402

COUNTS = (1, 2, 8)


def tables(desc, S, seed):
    rng = np.random.default_rng(seed)
    E = desc.input_channels * desc.input_columns * desc.input_rows

    def perms(n):
        return np.array([np.arange(n) if s == 0 else rng.permutation(n) for s in range(S)], dtype=np.int32)
    return perms(E), [perms(p) for p in desc.policy_dist_count]


def measure(desc, mode, args):
    """{variant: (median ms, min ms)} with the variants taking turns."""
    import torch
    dev = torch.device("cuda", args.device)
    net = HipNet(desc, args.device, mode)
    net.set_weights(to_blob(random_weights(desc, 7921)))
    n, big = args.rows, args.rows * max(COUNTS)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        d_x = torch.from_numpy(random_planes(desc, big, 11)).to(dev)
        d_pol = [torch.empty((big, p), dtype=torch.float32, device=dev) for p in desc.policy_dist_count]
        d_val = torch.empty((big, desc.num_values), dtype=torch.float32, device=dev)
    stream.synchronize()
    pol, val, sp = [p.data_ptr() for p in d_pol], d_val.data_ptr(), stream.cuda_stream
    variants = {"plain n": lambda: net.forward_device(sp, d_x.data_ptr(), n, pol, val)}
    syms = []
    for S in COUNTS:
        if S > 1:
            variants["plain n*%d" % S] = (lambda S=S: net.forward_device(sp, d_x.data_ptr(), n * S, pol, val))
        sym = HipSymmetry(*tables(desc, S, S), device=args.device)
        syms.append(sym)
        variants["sym %d" % S] = (lambda sym=sym: net.forward_sym_device(sym, sp, d_x.data_ptr(), n, pol, val))
    ms = {k: [] for k in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(args.warmup + args.reps):
        for k, call in variants.items():
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            if i >= args.warmup:
                ms[k].append(e0.elapsed_time(e1))
    for sym in syms:
        sym.close()
    net.close()
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    desc = BASELINE_CONFIGS[2]["desc"]
    print("cfg2 8x8 6x128, n = %d rows, median of %d calls per variant after %d warm-ups, variants alternating "
          "(min in brackets), ms between HIP events on the stream" % (args.rows, args.reps, args.warmup))
    for mode in ("bf16x3", "fp16x3-layered"):
        t = measure(desc, mode, args)
        for k, (med, mn) in t.items():
            print("%-15s %-10s %8.4f (%8.4f)" % (mode, k, med, mn))
        for S in COUNTS:
            inner = t["plain n*%d" % S][0] if S > 1 else t["plain n"][0]
            print("%-15s sym %d / plain n %.3f   sym %d / plain n*%d %.3f" %
                  (mode, S, t["sym %d" % S][0] / t["plain n"][0], S, S, t["sym %d" % S][0] / inner))
        sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
