#!/usr/bin/env python
"""What the evaluation cache (gz_eval_cache, gz_net_forward_cached, gz_runner_set_cache) costs and
what it saves, measured.  Nothing here is a threshold.

(a) Forward level: cfg2's net (8 x 8, 6 x 128) in bf16x3 and fp16x3-layered at 32 rows (PUCTPlayer's
    batch) and 1,024 rows (a self-play launch), one net, one stream and device buffers per mode, the
    cases taking turns call by call in one process.  Per call the wall time (perf_counter around the
    call and a stream synchronize: the host's wait for the count of misses is part of the price) and
    the device time (two HIP events on the stream); median of --reps calls per case after --warmup
    warm-up rounds, min in brackets.
      plain      gz_net_forward_device
      all new    gz_net_forward_cached_device, every row new (the table cleared before the call): the
                 overhead at hit rate 0 -- probe, compact, count wait, forward of all rows, fill
      all hit    the same rows again: probe, compact, count wait, no forward
      half       every second row new, the others hits (the table cleared and refilled with the even
                 rows before the call; the refill is not timed)
    --skip-runner runs (a) alone, e.g. under a kernel trace for the three kernels' own times.
(b) The self-play runner in bench.py's configuration (16 engine threads x 2 pools x 256 games, the
    config's evaluations per move, launches of 1,024 rows / 3 ms, spin yield 1,000) on cfg2
    (host-bound) and cfg4 (hexLG13 12 x 256, GPU-bound): leaf-evals/s over --seconds after --settle
    seconds, each run in a fresh process, --rounds rounds of
      old      the parent commit's build, loaded through GZ_LIB_DIR (--old-lib; skipped when absent)
      plain    this build without a cache
      cached   this build with a cache of --entries entries
    taking turns, and the cache's hit rate over the window.  Existing behaviour may not change: `plain`
    must lie within the spread of `old`.

    python tools/eval_cache_times.py [--out profiles/eval_cache_times.txt] [--old-lib tools/ab_old_lib]
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


def measure_forward(desc, mode, n, args):
    """{case: (median wall ms, min wall ms, median device ms, min device ms)} with the cases taking turns."""
    import torch
    from galvanise_zero_amd._native import HipNet
    from galvanise_zero_amd.nn.weights import random_weights, to_blob
    dev = torch.device("cuda", args.device)
    net = HipNet(desc, args.device, mode)
    net.set_weights(to_blob(random_weights(desc, 7921)))
    cache = net.make_cache(65536)
    stream = torch.cuda.Stream(device=dev)
    from galvanise_zero_amd.util.evalcache import slots
    x = np.random.default_rng(11).integers(0, 2, (2 * n, desc.input_channels, desc.input_columns, desc.input_rows)).astype(np.float32)
    # rows with a slot each: two rows of a call that share a slot evict each other and never both hit
    _, first = np.unique(np.array(slots(x, 65536)), return_index=True)
    x = np.ascontiguousarray(x[np.sort(first)[:n]])
    assert x.shape[0] == n
    even = np.ascontiguousarray(x[0::2])
    with torch.cuda.stream(stream):
        d_x, d_even = torch.from_numpy(x).to(dev), torch.from_numpy(even).to(dev)
        d_pol = [torch.empty((n, p), dtype=torch.float32, device=dev) for p in desc.policy_dist_count]
        d_val = torch.empty((n, desc.num_values), dtype=torch.float32, device=dev)
    stream.synchronize()
    pol, val, sp = [p.data_ptr() for p in d_pol], d_val.data_ptr(), stream.cuda_stream

    def cached(ptr=None, rows=n):
        net.forward_cached_device(cache, sp, d_x.data_ptr() if ptr is None else ptr, rows, pol, val)

    def prepare(case):
        if case in ("all new", "half"):
            cache.clear()
        if case == "half":
            cached(d_even.data_ptr(), even.shape[0])
        stream.synchronize()
    calls = {"plain": lambda: net.forward_device(sp, d_x.data_ptr(), n, pol, val), "all new": cached, "all hit": cached, "half": cached}
    wall, devms, fwd = {k: [] for k in calls}, {k: [] for k in calls}, {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(args.warmup + args.reps):
        for k, call in calls.items():
            prepare(k)
            t0 = time.perf_counter()
            e0.record(stream)
            call()
            e1.record(stream)
            stream.synchronize()
            t1 = time.perf_counter()
            if i >= args.warmup:
                wall[k].append((t1 - t0) * 1e3)
                devms[k].append(e0.elapsed_time(e1))
        if i == args.warmup + args.reps - 1:       # what the last round's calls sent through the forward
            for k, call in calls.items():
                if k != "plain":
                    prepare(k)
                    f0 = cache.stats()["forward_rows"]
                    call()
                    fwd[k] = cache.stats()["forward_rows"] - f0
    st = cache.stats()
    st["case_forward_rows"] = fwd
    cache.close()
    net.close()
    return {k: (float(np.median(wall[k])), float(np.min(wall[k])), float(np.median(devms[k])), float(np.min(devms[k])))
            for k in calls}, st


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
    if args.runner_child == "cached":
        kw["cache"] = net.make_cache(args.entries)
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
                   table_bytes=c1["entries"] * c1["entry_bytes"], replaced=c1["replaced"], inserts=c1["inserts"], flushes=c1["flushes"])
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--settle", type=float, default=5.0)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--entries", type=int, default=1 << 18)
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--variants", default="old,plain,cached", help="the runs of a round of (b)")
    ap.add_argument("--config", type=int, default=2, help="(of a --runner-child)")
    ap.add_argument("--old-lib", default=os.path.join(ROOT, "tools", "ab_old_lib"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_cache_times.txt"))
    ap.add_argument("--skip-runner", action="store_true", help="(a) alone, e.g. under a kernel trace")
    ap.add_argument("--skip-forward", action="store_true", help="(b) alone")
    ap.add_argument("--runner-child", choices=["old", "plain", "cached"], default=None)
    args = ap.parse_args()
    if args.runner_child:
        return runner_child(args)
    from galvanise_zero_amd.nn.desc import BASELINE_CONFIGS
    desc = BASELINE_CONFIGS[2]["desc"]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def save():
        with open(args.out, "a" if args.skip_forward else "w") as f:
            f.write("\n".join(lines) + "\n")
    if not args.skip_forward:
        say("(a) cfg2 8x8 6x128, median of %d calls per case after %d warm-ups, cases alternating (min in brackets): "
            "wall ms of call + stream synchronize | device ms between HIP events" % (args.reps, args.warmup))
        for mode in ("bf16x3", "fp16x3-layered"):
            for n in (32, 1024):
                t, st = measure_forward(desc, mode, n, args)
                for k, (w, wmin, d, dmin) in t.items():
                    say("%-15s n %-5d %-8s wall %8.4f (%8.4f) | device %8.4f (%8.4f)" % (mode, n, k, w, wmin, d, dmin))
                say("%-15s n %-5d wall: all new / plain %.3f, all hit / plain %.3f, half / plain %.3f   (entry %d bytes; rows through "
                    "the forward per call: %s)" %
                    (mode, n, t["all new"][0] / t["plain"][0], t["all hit"][0] / t["plain"][0], t["half"][0] / t["plain"][0],
                     st["entry_bytes"], ", ".join("%s %d" % kv for kv in st["case_forward_rows"].items())))
    if args.skip_runner:
        save()
        return 0
    for config in [int(c) for c in args.configs.split(",")]:
        cfg = BASELINE_CONFIGS[config]
        variants = [v for v in args.variants.split(",") if v != "old" or os.path.isdir(args.old_lib)]
        say("(b) runner, cfg%d %s, %d threads x 2 pools x 256 games, %d evals/move, launches of 1,024 rows / 3 ms, bf16x3: "
            "leaf-evals/s over %.0f s after %.0f s, a fresh process per run, %d rounds of %s taking turns"
            % (config, cfg["game"], args.threads, cfg["evals"], args.seconds, args.settle, args.rounds, ", ".join(variants)))
        if "old" in args.variants.split(",") and "old" not in variants:
            say("    (no build of the parent commit at %s: `old` skipped)" % args.old_lib)
        rates, hit = {v: [] for v in variants}, []
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
                    save()
                    return 1
                d = json.loads(p.stdout.strip().splitlines()[-1])
                rates[v].append(d["leaf_evals_per_s"])
                extra = ""
                if v == "cached":
                    hit.append(d["hit_rate"])
                    extra = ", hit rate %.4f over the window, %d entries = %.0f MB, %d inserts of which %d replaced an entry, %d flushes" % (
                        d["hit_rate"], d["entries"], d["table_bytes"] / 1e6, d["inserts"], d["replaced"], d["flushes"])
                say("    round %d %-6s %10.0f leaf-evals/s  (%.0f rows and %.4f ms on the stream per launch%s)"
                    % (rnd, v, d["leaf_evals_per_s"], d["rows_per_launch"], d["kernel_ms_per_launch"], extra))
        for v in variants:
            say("    %-6s median %10.0f  min %10.0f  max %10.0f" % (v, np.median(rates[v]), min(rates[v]), max(rates[v])))
        base = "old" if "old" in variants else "plain"
        for v in variants:
            if v != base:
                say("    %s / %s (medians) %.4f" % (v, base, np.median(rates[v]) / np.median(rates[base])))
        if hit:
            say("    cached: median hit rate %.4f" % np.median(hit))
        if "old" in variants and "plain" in variants:
            inside = min(rates["old"]) <= np.median(rates["plain"]) <= max(rates["old"])
            say("    plain's median %s the spread of old's runs" % ("lies within" if inside else "LIES OUTSIDE"))
    save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
