"""bench.py's own paths on the GPU: the single-rank line carries the contract's keys, and
`--gpus 2` starts two ranks itself (torch.distributed.run) that broadcast the weight blob, load it
with gz_net_set_weights_device, run the native runner on disjoint global game ranges, roll the live
runners to a second broadcast generation (--roll) and report n_gpus = 2.  The two ranks share GPU 0 over gloo here (one GPU per box; RCCL needs one GPU per
rank); the driver's 8-GPU run uses RCCL.  Reference: distributed/worker.py:107-160, SURVEY 8e."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SMALL = ["--age-seconds", "0", "--warmup", "1", "--steps", "2", "--step-rows", "65536", "--threads", "2",
         "--pools", "2", "--batch", "64", "--no-cpu-baseline"]


def _run(args, timeout=300):
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py")] + args, cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_single_rank_line(hip_device, tmp_path):
    import numpy as np
    from galvanise_zero_amd._native import HipNet
    from galvanise_zero_amd.nn.desc import BASELINE_CONFIGS
    from galvanise_zero_amd.nn.tolerance import SPLIT_TOLERANCE
    from galvanise_zero_amd.nn.weights import random_weights
    from oracle import nn_ref
    # 2 threads x 4 pools x 64 games: the pools together pass the large-launch kernel's threshold
    args = ["--gpus", "1"] + SMALL + ["--pools", "4"]
    out = _run(args + ["--dump-outputs", str(tmp_path / "a")])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "games_per_sec", "steady_state"):
        assert k in out, k
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["value"] > 0
    assert out["roofline"]["bound"] == "mfma" and 0 < out["roofline"]["frac"] < 1
    # a plain run: no aging, no CPU baseline
    assert out["full"] is False and out["steady_state"]["aged"] is False and "cpu_baseline" not in out
    # ms_per_step is the timed window over its steps (65,536 leaf evaluations each at `value` per second)
    assert out["ms_per_step"] == pytest.approx(1e3 * 65536 / out["value"], rel=0.1)
    # --dump-outputs: the run's 8 pools replayed to batch 384 (3 steps x 65,536 rows over 512 game
    # slots), every round one segmented launch big enough for the large-launch trunk kernel -- the
    # kernel the headline figure runs on
    desc = BASELINE_CONFIGS[2]["desc"]
    net = HipNet(desc, hip_device, "bf16x3")
    d = out["dump_outputs"]
    assert (d["pools"], d["batch"]) == (8, 384)
    assert net.large_min_rows() <= d["launch_rows"] <= 512 and d["large_min_rows"] == net.large_min_rows()
    assert d["kernel"] == net.kernel_name(True)
    arrays = {f[:-4]: np.load(str(tmp_path / "a" / f)) for f in sorted(os.listdir(str(tmp_path / "a")))}
    assert sorted(arrays) == ["planes", "policy_0", "policy_1", "value"]
    rows = d["launch_rows"]
    assert all(a.dtype == np.float32 and a.shape[0] == rows and np.all(np.isfinite(a)) for a in arrays.values())
    for k in ("policy_0", "policy_1"):
        assert np.allclose(arrays[k].sum(axis=1), 1.0, atol=1e-4), k
    assert arrays["value"].min() >= 0.0 and arrays["value"].max() <= 1.0
    # every output row belongs to its planes row (the launch's segment mapping): the bench's network
    # (cfg2, random_weights(desc, 7921), bf16x3) on every 8th row -- rows of all 8 segments -- against
    # the float64 oracle within the stated cfg2 tolerance
    ref = nn_ref.forward(desc, random_weights(desc, 7921), arrays["planes"][::8])
    for k, r in zip(("policy_0", "policy_1", "value"), ref):
        assert float(np.abs(arrays[k][::8] - r).max()) <= SPLIT_TOLERANCE["cfg2"]["max"], k
    # the same arguments again: the same files, byte for byte
    out2 = _run(args + ["--dump-outputs", str(tmp_path / "b")])
    assert out2["dump_outputs"]["arrays"] == d["arrays"]
    for k, a in arrays.items():
        assert np.array_equal(a, np.load(str(tmp_path / "b" / (k + ".npy")))), k


def test_bench_two_ranks(hip_device):
    out = _run(["--gpus", "2", "--backend", "gloo", "--device", "0", "--roll"] + SMALL, timeout=400)
    assert out["n_gpus"] == 2
    assert out["config"]["weights_broadcast"]["identical_on_all_ranks"] is True
    # the mid-run generation roll: broadcast to both ranks, applied by both live runners
    assert out["generation_roll"]["identical_on_all_ranks"] is True
    rng = out["config"]["game_ranges"]
    assert rng["disjoint"] is True and len(rng["per_rank"]) == 2
    assert rng["per_rank"][0][1] - rng["per_rank"][0][0] == out["config"]["games_per_gpu"]
    assert out["value"] > 0
