#!/usr/bin/env python
"""Forward time of the three arithmetic modes side by side: fp32-ieee, bf16x3, bf16.

One process; per shape the three nets' forwards (gz_net_forward_device on device-resident planes)
alternate on one stream, each timed with HIP events; the median of --reps timed forwards after
--warmup untimed ones is reported, with the fp32-ieee / bf16x3 ratio (target on cfg2 at 1,024 rows:
<= 8, include/gzero_nn.h GZ_PRECISION_FP32).  For information, a torch float32 forward of the same v1
net on the GPU (its conv backend may not run offline: reported as unavailable then).

    python tools/precision_forward_time.py [--reps 30] [--warmup 5] [--torch]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2, 1), (2, 32), (2, 1024), (4, 256)]   # (BASELINE config, rows)
MODES = ["fp32-ieee", "bf16x3", "bf16"]


def torch_forward(desc, weights):
    """The v1 net in torch float32 on the GPU (oracle/nn_torch.py's layers)."""
    import torch
    import torch.nn.functional as tF
    w = {k: torch.tensor(np.asarray(v), dtype=torch.float32, device="cuda") for k, v in weights}
    k4 = {n: t.permute(3, 2, 0, 1).contiguous() for n, t in w.items() if t.dim() == 4}

    def bn(x, p):
        return tF.batch_norm(x, w[p + "_mean"], w[p + "_var"], w[p + "_gamma"], w[p + "_beta"], training=False, eps=1e-3)

    def conv(x, n):
        return tF.conv2d(x, k4[n], padding=k4[n].shape[-1] // 2)

    def fwd(x):
        with torch.inference_mode():
            x = tF.relu(bn(conv(x, "initial_conv"), "initial_bn"))
            for i in range(desc.residual_layers):
                y = tF.relu(bn(conv(x, "res%d_conv0" % i), "res%d_bn0" % i))
                x = tF.relu(x + bn(conv(y, "res%d_conv1" % i), "res%d_bn1" % i))
            outs = []
            for r in range(len(desc.policy_dist_count)):
                h = tF.relu(bn(conv(x, "policy%d_conv" % r), "policy%d_bn" % r)).permute(0, 2, 3, 1)
                outs.append(torch.softmax(h.reshape(h.shape[0], -1) @ w["policy%d_dense" % r] + w["policy%d_bias" % r], 1))
            return outs
    return fwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch", action="store_true", help="also time a torch float32 forward on the GPU (information)")
    args = ap.parse_args()
    assert args.reps >= 20
    import torch
    from galvanise_zero_amd._native import HipNet
    from galvanise_zero_amd.nn.desc import BASELINE_CONFIGS
    from galvanise_zero_amd.nn.weights import random_planes, random_weights, to_blob
    stream = torch.cuda.current_stream().cuda_stream
    print("device: %s" % torch.cuda.get_device_name(0))
    for cfg, n in SHAPES:
        desc = BASELINE_CONFIGS[cfg]["desc"]
        weights = random_weights(desc, 7921)
        blob = to_blob(weights)
        x = torch.from_numpy(random_planes(desc, n, 5)).cuda()
        pols = [torch.empty((n, p), device="cuda") for p in desc.policy_dist_count]
        val = torch.empty((n, desc.num_values), device="cuda")
        nets = {}
        for m in MODES:
            nets[m] = HipNet(desc, 0, m)
            nets[m].set_weights(blob)
        ms = {m: [] for m in MODES}
        for it in range(args.warmup + args.reps):
            for m in MODES:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                nets[m].forward_device(stream, x.data_ptr(), n, [p.data_ptr() for p in pols], val.data_ptr())
                e1.record()
                e1.synchronize()
                if it >= args.warmup:
                    ms[m].append(e0.elapsed_time(e1))
        med = {m: float(np.median(ms[m])) for m in MODES}
        flops = desc.flops_per_eval() * n
        print("cfg%d n=%d  " % (cfg, n) + "  ".join("%s %.4f ms (min %.4f)" % (m, med[m], min(ms[m])) for m in MODES) +
              "  | fp32-ieee / bf16x3 = %.2f  | fp32-ieee %.1f TFLOP/s" % (med["fp32-ieee"] / med["bf16x3"],
                                                                            flops / (med["fp32-ieee"] * 1e-3) / 1e12))
        for m in MODES:
            nets[m].close()
    if not args.torch:
        return
    for cfg, n in SHAPES:
        desc = BASELINE_CONFIGS[cfg]["desc"]
        weights = random_weights(desc, 7921)
        x = torch.from_numpy(random_planes(desc, n, 5)).cuda()
        try:
            fwd = torch_forward(desc, weights)
            t = []
            for it in range(3 + 20):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fwd(x)
                e1.record()
                e1.synchronize()
                if it >= 3:
                    t.append(e0.elapsed_time(e1))
            print("cfg%d n=%d  torch float32 on the GPU (trunk + policy heads, for information): %.4f ms" % (cfg, n, float(np.median(t))))
        except Exception as e:   # noqa: BLE001 -- the conv backend needs its kernel database
            print("cfg%d n=%d  torch float32 on the GPU: unavailable (%s: %s)" % (cfg, n, type(e).__name__, str(e).splitlines()[0][:120]))


if __name__ == "__main__":
    main()
