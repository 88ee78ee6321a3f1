#!/usr/bin/env python
"""What one symmetry per row (gz_net_forward_sym_pick, gz_runner_set_symmetry) costs.

(a) Device time of the pick forward against the plain forward, which is unchanged code and so the
    yardstick: cfg2's net (8 x 8, 6 x 128) in bf16x3 and fp16x3-layered at 32 rows (PUCTPlayer's batch)
    and 1,024 rows (a self-play launch).  Per mode one net, one stream and device buffers; the variants
    take turns, call by call, in one process; each call is timed between two HIP events on the stream;
    median of --reps calls per variant after --warmup warm-up rounds, min in brackets.
      plain        gz_net_forward_device
      pick S       gz_net_forward_sym_pick_device with S in {2, 8} elements (hash + permute, the same
                   forward, gather)
      hash         sym_pick_expand_kernel without the permuted copy (gz_symmetry_picks on device memory:
                   wall time of a synchronous call, launch and copy-back included)
    pick - plain is what the two kernels add to a launch, gaps included.
(b) The self-play runner on cfg2 in bench.py's configuration (16 engine threads x 2 pools x 256 games,
    800 evaluations per move, launches of 1,024 rows / 3 ms, spin yield 1,000), leaf-evals/s over
    --seconds after --settle seconds, each run in a fresh process, three rounds of
      old      the parent commit's build, loaded through GZ_LIB_DIR (--old-lib; skipped when absent)
      plain    this build without a symmetry
      pick     this build with breakthrough's reflection in pick mode
      staged   this build without a symmetry but with GZ_RUNNER_OUT_STAGING=1: the output staging the
               pick path forces on (outputs to HBM, then per-segment copies on a third stream), alone
    taking turns.  Existing behaviour may not change: `plain` must lie within the spread of `old`.
    `staged` says how much of pick's cost is the staging's and how much the two kernels'.

    python tools/sym_pick_times.py [--out profiles/sym_pick_times.txt] [--old-lib tools/ab_old_lib]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = (2, 8)


def tables(desc, S, seed):
    rng = np.random.default_rng(seed)
    E = desc.input_channels * desc.input_columns * desc.input_rows

    def perms(n):
        return np.array([np.arange(n) if s == 0 else rng.permutation(n) for s in range(S)], dtype=np.int32)
    return perms(E), [perms(p) for p in desc.policy_dist_count]


def measure_forward(desc, mode, n, args):
    """{variant: (median ms, min ms)} with the variants taking turns."""
    import torch
    from galvanise_zero_amd._native import HipNet, HipSymmetry
    from galvanise_zero_amd.nn.weights import random_weights, to_blob
    dev = torch.device("cuda", args.device)
    net = HipNet(desc, args.device, mode)
    net.set_weights(to_blob(random_weights(desc, 7921)))
    stream = torch.cuda.Stream(device=dev)
    x = np.random.default_rng(11).integers(0, 2, (n, desc.input_channels, desc.input_columns, desc.input_rows)).astype(np.float32)
    with torch.cuda.stream(stream):
        d_x = torch.from_numpy(x).to(dev)
        d_pol = [torch.empty((n, p), dtype=torch.float32, device=dev) for p in desc.policy_dist_count]
        d_val = torch.empty((n, desc.num_values), dtype=torch.float32, device=dev)
    stream.synchronize()
    pol, val, sp = [p.data_ptr() for p in d_pol], d_val.data_ptr(), stream.cuda_stream
    variants = {"plain": lambda: net.forward_device(sp, d_x.data_ptr(), n, pol, val)}
    syms = []
    for S in COUNTS:
        sym = HipSymmetry(*tables(desc, S, S), device=args.device)
        syms.append(sym)
        variants["pick %d" % S] = (lambda sym=sym: net.forward_sym_pick_device(sym, 12345, sp, d_x.data_ptr(), n, pol, val))
    ms = {k: [] for k in variants}
    ms["hash"] = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(args.warmup + args.reps):
        for k, call in variants.items():
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            if i >= args.warmup:
                ms[k].append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        net.symmetry_picks(syms[-1], 12345, device_ptr=d_x.data_ptr(), n=n)
        if i >= args.warmup:
            ms["hash"].append((time.perf_counter() - t0) * 1e3)
    for sym in syms:
        sym.close()
    net.close()
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in ms.items()}


def runner_child(args):
    """One runner run; prints one JSON line."""
    import bench
    from galvanise_zero_amd._native import HipNet
    from galvanise_zero_amd.nn.desc import BASELINE_CONFIGS
    from galvanise_zero_amd.nn.weights import random_weights, to_blob
    from galvanise_zero_amd.runner import SelfPlayRunner
    sm, transformer, desc = bench.setup_game(2)
    net = HipNet(desc, args.device, "bf16x3")
    net.set_weights(to_blob(random_weights(desc, 7921)))
    kw = {}
    if args.runner_child == "pick":
        from galvanise_zero_amd.util import symmetry
        T, _, _ = symmetry.tables_for_game("breakthrough")
        kw["symmetry"] = net.make_symmetry(T)
    r = SelfPlayRunner(net, sm, transformer, bench.selfplay_conf("template", BASELINE_CONFIGS[2]["evals"]), device=args.device,
                       num_threads=args.threads, pools_per_thread=2, batch_size=256, seed=20251015, spin_yield_playouts=1000,
                       min_launch_rows=1024, max_launch_wait_us=3000, **kw)
    r.start()
    time.sleep(args.settle)
    s0, t0 = r.stats(), time.perf_counter()
    time.sleep(args.seconds)
    s1, t1 = r.stats(), time.perf_counter()
    r.stop()
    s2 = r.stats()
    picked = r.sym_pick_rows() if kw else 0
    r.close()
    rows, launches = s1["rows"] - s0["rows"], s1["kernel_launches"] - s0["kernel_launches"]
    print(json.dumps({"variant": args.runner_child, "leaf_evals_per_s": rows / (t1 - t0), "rows_per_launch": rows / max(1, launches),
                      "kernel_ms_per_launch": (s1["kernel_ms"] - s0["kernel_ms"]) / max(1, launches),
                      "pick_rows": picked, "rows": s2["rows"]}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--settle", type=float, default=5.0)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--old-lib", default=os.path.join(ROOT, "tools", "ab_old_lib"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sym_pick_times.txt"))
    ap.add_argument("--skip-runner", action="store_true", help="(a) alone, e.g. under a kernel trace")
    ap.add_argument("--runner-child", choices=["old", "plain", "pick", "staged"], default=None)
    args = ap.parse_args()
    if args.runner_child:
        return runner_child(args)
    from galvanise_zero_amd.nn.desc import BASELINE_CONFIGS
    desc = BASELINE_CONFIGS[2]["desc"]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("(a) cfg2 8x8 6x128, median of %d calls per variant after %d warm-ups, variants alternating (min in brackets), "
        "ms between HIP events on the stream; hash: wall ms of a synchronous gz_symmetry_picks" % (args.reps, args.warmup))
    for mode in ("bf16x3", "fp16x3-layered"):
        for n in (32, 1024):
            t = measure_forward(desc, mode, n, args)
            for k, (med, mn) in t.items():
                say("%-15s n %-5d %-8s %8.4f (%8.4f)" % (mode, n, k, med, mn))
            for S in COUNTS:
                say("%-15s n %-5d pick %d / plain %.3f   pick %d - plain %.4f ms" %
                    (mode, n, S, t["pick %d" % S][0] / t["plain"][0], S, t["pick %d" % S][0] - t["plain"][0]))
    if args.skip_runner:
        return 0
    variants = (["old"] if os.path.isdir(args.old_lib) else []) + ["plain", "pick", "staged"]
    say("(b) runner, cfg2 breakthrough, %d threads x 2 pools x 256 games, 800 evals/move, launches of 1,024 rows / 3 ms: "
        "leaf-evals/s over %.0f s after %.0f s, a fresh process per run, %d rounds of %s taking turns"
        % (args.threads, args.seconds, args.settle, args.rounds, ", ".join(variants)))
    if "old" not in variants:
        say("    (no build of the parent commit at %s: `old` skipped)" % args.old_lib)
    rates = {v: [] for v in variants}
    for rnd in range(args.rounds):
        for v in variants:
            env = dict(os.environ)
            if v == "old":
                env["GZ_LIB_DIR"] = args.old_lib
            if v == "staged":
                env["GZ_RUNNER_OUT_STAGING"] = "1"
            cmd = [sys.executable, os.path.abspath(__file__), "--runner-child", v, "--device", str(args.device), "--threads",
                   str(args.threads), "--settle", str(args.settle), "--seconds", str(args.seconds)]
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, universal_newlines=True, timeout=args.settle + args.seconds + 120)
            if p.returncode != 0:
                say("    round %d %s: exit status %d" % (rnd, v, p.returncode))
                return 1
            d = json.loads(p.stdout.strip().splitlines()[-1])
            rates[v].append(d["leaf_evals_per_s"])
            say("    round %d %-5s %10.0f leaf-evals/s  (%.0f rows and %.4f ms of forward per launch, pick rows %d of %d)"
                % (rnd, v, d["leaf_evals_per_s"], d["rows_per_launch"], d["kernel_ms_per_launch"], d["pick_rows"], d["rows"]))
    for v in variants:
        say("    %-5s median %10.0f  min %10.0f  max %10.0f" % (v, np.median(rates[v]), min(rates[v]), max(rates[v])))
    base = "old" if "old" in variants else "plain"
    for v in variants:
        if v != base:
            say("    %s / %s (medians) %.4f" % (v, base, np.median(rates[v]) / np.median(rates[base])))
    if "old" in variants:
        inside = min(rates["old"]) <= np.median(rates["plain"]) <= max(rates["old"])
        say("    plain's median %s the spread of old's runs" % ("lies within" if inside else "LIES OUTSIDE"))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
