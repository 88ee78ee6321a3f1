#!/usr/bin/env python
"""What the canonical orientation (gz_net_forward_sym_canon, gz_runner_set_canonical) costs and what it
shares, measured.  Nothing here is a threshold.

(a) Kernel and forward: cfg2's net with breakthrough's reflection (E = 320, S = 2) and cfg5's net with
    amazons' group (E = 1,200, S = 8), bf16x3, at 32 and 1,024 rows.  Per net one stream and device
    buffers; the variants take turns, call by call, in one process; each call is timed between two HIP
    events on the stream; median of --reps calls per variant after --warmup warm-up rounds, min in
    brackets.
      plain        gz_net_forward_device
      pick         gz_net_forward_sym_pick_device (unchanged code: the parent commit's pick)
      canon        gz_net_forward_sym_canon_device without a cache
      hash pick    sym_pick_expand_kernel without the permuted copy (gz_symmetry_picks on device memory:
                   wall time of a synchronous call, allocation, launch and copy-back included)
      hash canon   sym_canon_expand_kernel likewise (gz_symmetry_canon on device memory)
    canon - plain and pick - plain are what the two kernels of each form add to a launch, gaps
    included; hash canon - hash pick is the expand kernels' difference without the permuted copy.
(b) The self-play runner in bench.py's configuration (16 engine threads x 2 pools x 256 games, the
    config's evaluations per move, launches of 1,024 rows / 3 ms, spin yield 1,000, bf16x3):
    leaf-evals/s and the cache's hit rate over --seconds after --settle seconds, each run in a fresh
    process, --rounds rounds of
      old      the parent commit's build, loaded through GZ_LIB_DIR (--old-lib; skipped when absent),
               without a cache or a symmetry
      cache    this build with a plain cache of --entries entries (gz_runner_set_cache)
      canon    this build in canonical mode with a cache of --entries entries (gz_runner_set_canonical)
    taking turns.  The window is the opening: every game is within its first moves.

    python tools/sym_canon_times.py [--out profiles/sym_canon_times.txt] [--old-lib tools/ab_old_lib]
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


def measure_forward(config, n, args):
    """{variant: (median ms, min ms)} with the variants taking turns."""
    import torch
    from galvanise_zero_amd._native import HipNet
    from galvanise_zero_amd.nn.desc import BASELINE_CONFIGS
    from galvanise_zero_amd.nn.weights import random_weights, to_blob
    from galvanise_zero_amd.util import symmetry
    cfg = BASELINE_CONFIGS[config]
    desc = cfg["desc"]
    T, _, _ = symmetry.tables_for_game(cfg["game"])
    dev = torch.device("cuda", args.device)
    net = HipNet(desc, args.device, "bf16x3")
    net.set_weights(to_blob(random_weights(desc, 7921)))
    sym = net.make_symmetry(T)
    stream = torch.cuda.Stream(device=dev)
    x = np.random.default_rng(11).integers(0, 2, (n, desc.input_channels, desc.input_columns, desc.input_rows)).astype(np.float32)
    with torch.cuda.stream(stream):
        d_x = torch.from_numpy(x).to(dev)
        d_pol = [torch.empty((n, p), dtype=torch.float32, device=dev) for p in desc.policy_dist_count]
        d_val = torch.empty((n, desc.num_values), dtype=torch.float32, device=dev)
    stream.synchronize()
    pol, val, sp = [p.data_ptr() for p in d_pol], d_val.data_ptr(), stream.cuda_stream
    variants = {"plain": lambda: net.forward_device(sp, d_x.data_ptr(), n, pol, val),
                "pick": lambda: net.forward_sym_pick_device(sym, 12345, sp, d_x.data_ptr(), n, pol, val),
                "canon": lambda: net.forward_sym_canon_device(sym, 12345, None, sp, d_x.data_ptr(), n, pol, val)}
    hashes = {"hash pick": lambda: net.symmetry_picks(sym, 12345, device_ptr=d_x.data_ptr(), n=n),
              "hash canon": lambda: net.symmetry_canon(sym, 12345, device_ptr=d_x.data_ptr(), n=n)}
    ms = {k: [] for k in list(variants) + list(hashes)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(args.warmup + args.reps):
        for k, call in variants.items():
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            if i >= args.warmup:
                ms[k].append(e0.elapsed_time(e1))
        for k, call in hashes.items():
            t0 = time.perf_counter()
            call()
            if i >= args.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    sym.close()
    net.close()
    return T.count, T.plane_src.shape[1], {k: (float(np.median(v)), float(np.min(v))) for k, v in ms.items()}


def runner_child(args):
    """One runner run; prints one JSON line."""
    import bench
    from galvanise_zero_amd._native import HipNet
    from galvanise_zero_amd.nn.desc import BASELINE_CONFIGS
    from galvanise_zero_amd.nn.weights import random_weights, to_blob
    from galvanise_zero_amd.runner import SelfPlayRunner
    sm, transformer, desc = bench.setup_game(args.config)
    net = HipNet(desc, args.device, "bf16x3")
    net.set_weights(to_blob(random_weights(desc, 7921)))
    kw = {}
    if args.runner_child in ("cache", "canon"):
        kw["cache"] = net.make_cache(args.entries)
    if args.runner_child == "canon":
        from galvanise_zero_amd.util import symmetry
        T, _, _ = symmetry.tables_for_game(BASELINE_CONFIGS[args.config]["game"])
        kw.update(symmetry=net.make_symmetry(T), symmetry_mode="canonical")
    r = SelfPlayRunner(net, sm, transformer, bench.selfplay_conf("template", BASELINE_CONFIGS[args.config]["evals"]),
                       device=args.device, num_threads=args.threads, pools_per_thread=2, batch_size=256, seed=20251015,
                       spin_yield_playouts=1000, min_launch_rows=1024, max_launch_wait_us=3000, **kw)
    r.start()
    time.sleep(args.settle)
    s0, c0, t0 = r.stats(), (r.cache_stats() if kw else None), time.perf_counter()
    time.sleep(args.seconds)
    s1, c1, t1 = r.stats(), (r.cache_stats() if kw else None), time.perf_counter()
    r.stop()
    r.close()
    rows, launches = s1["rows"] - s0["rows"], s1["kernel_launches"] - s0["kernel_launches"]
    out = {"variant": args.runner_child, "leaf_evals_per_s": rows / (t1 - t0), "rows_per_launch": rows / max(1, launches),
           "kernel_ms_per_launch": (s1["kernel_ms"] - s0["kernel_ms"]) / max(1, launches)}
    if kw:
        out.update(hit_rate=(c1["hits"] - c0["hits"]) / max(1, c1["rows"] - c0["rows"]), entries=c1["entries"],
                   table_bytes=c1["entries"] * c1["entry_bytes"])
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--settle", type=float, default=4.0)
    ap.add_argument("--seconds", type=float, default=8.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--entries", type=int, default=1 << 18)
    ap.add_argument("--configs", default="4,3,2")
    ap.add_argument("--config", type=int, default=2, help="(of a --runner-child)")
    ap.add_argument("--old-lib", default=os.path.join(ROOT, "tools", "ab_old_lib"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sym_canon_times.txt"))
    ap.add_argument("--skip-runner", action="store_true", help="(a) alone")
    ap.add_argument("--skip-forward", action="store_true", help="(b) alone, appended to --out")
    ap.add_argument("--runner-child", choices=["old", "cache", "canon"], default=None)
    args = ap.parse_args()
    if args.runner_child:
        return runner_child(args)
    from galvanise_zero_amd.nn.desc import BASELINE_CONFIGS
    out = open(args.out, "a" if args.skip_forward else "w")

    def say(s):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()
    if not args.skip_forward:
        say("(a) bf16x3, median of %d calls per variant after %d warm-ups, variants alternating (min in brackets), ms between "
            "HIP events on the stream; hash pick / hash canon: wall ms of a synchronous gz_symmetry_picks / gz_symmetry_canon"
            % (args.reps, args.warmup))
        for config in (2, 5):
            for n in (32, 1024):
                S, E, t = measure_forward(config, n, args)
                what = "cfg%d %s E %d S %d" % (config, BASELINE_CONFIGS[config]["game"], E, S)
                for k, (med, mn) in t.items():
                    say("%-34s n %-5d %-10s %8.4f (%8.4f)" % (what, n, k, med, mn))
                say("%-34s n %-5d canon / plain %.3f  pick / plain %.3f  canon - plain %.4f ms  pick - plain %.4f ms  "
                    "hash canon - hash pick %.4f ms" %
                    (what, n, t["canon"][0] / t["plain"][0], t["pick"][0] / t["plain"][0], t["canon"][0] - t["plain"][0],
                     t["pick"][0] - t["plain"][0], t["hash canon"][0] - t["hash pick"][0]))
    if args.skip_runner:
        return 0
    for config in [int(c) for c in args.configs.split(",")]:
        cfg = BASELINE_CONFIGS[config]
        variants = (["old"] if os.path.isdir(args.old_lib) else []) + ["cache", "canon"]
        say("(b) runner, cfg%d %s, %d threads x 2 pools x 256 games, %d evals/move, launches of 1,024 rows / 3 ms, bf16x3, caches "
            "of %d entries: leaf-evals/s over %.0f s after %.0f s, a fresh process per run, %d rounds of %s taking turns"
            % (config, cfg["game"], args.threads, cfg["evals"], args.entries, args.seconds, args.settle, args.rounds,
               ", ".join(variants)))
        if "old" not in variants:
            say("    (no build of the parent commit at %s: `old` skipped)" % args.old_lib)
        rates, hit = {v: [] for v in variants}, {v: [] for v in variants}
        for rnd in range(args.rounds):
            for v in variants:
                env = dict(os.environ)
                if v == "old":
                    env["GZ_LIB_DIR"] = args.old_lib
                cmd = [sys.executable, os.path.abspath(__file__), "--runner-child", v, "--device", str(args.device), "--threads",
                       str(args.threads), "--settle", str(args.settle), "--seconds", str(args.seconds), "--config", str(config),
                       "--entries", str(args.entries)]
                p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, universal_newlines=True, timeout=args.settle + args.seconds + 180)
                if p.returncode != 0:
                    say("    round %d %s: exit status %d" % (rnd, v, p.returncode))
                    return 1
                d = json.loads(p.stdout.strip().splitlines()[-1])
                rates[v].append(d["leaf_evals_per_s"])
                extra = ""
                if "hit_rate" in d:
                    hit[v].append(d["hit_rate"])
                    extra = ", hit rate %.4f over the window, %.0f MB" % (d["hit_rate"], d["table_bytes"] / 1e6)
                say("    round %d %-6s %10.0f leaf-evals/s  (%.0f rows and %.4f ms on the stream per launch%s)"
                    % (rnd, v, d["leaf_evals_per_s"], d["rows_per_launch"], d["kernel_ms_per_launch"], extra))
        for v in variants:
            say("    %-6s median %10.0f  min %10.0f  max %10.0f%s" % (v, np.median(rates[v]), min(rates[v]), max(rates[v]),
                                                                       "  median hit rate %.4f" % np.median(hit[v]) if hit[v] else ""))
        for v in variants[1:]:
            say("    %s / %s (medians) %.4f" % (v, variants[0], np.median(rates[v]) / np.median(rates[variants[0]])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
