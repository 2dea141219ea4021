#!/usr/bin/env python3
"""Throughput of the HIP I3D forward (the FVD / KVD embedding, mebt_amd/i3d.py) on one GPU: one JSON line per compute dtype with
clips/s and ms per batch (HIP events around each forward after warm-up; median, min, max), the algorithmic TFLOP/s of the
convolutions (shape table of mebt_amd.i3d.plan_flops: 55.6 GFLOP per 16-frame clip) and its fraction of the dtype's dense peak
(fp16 MFMA 2.5 PFLOP/s, fp32 157 TFLOP/s), plus one comparison line: the same batch through torch eager fp32 (F.conv3d on the
GPU, tf32 off) — the reference's arithmetic (mebt/fvd/pytorch_i3d.py).  Weights are random (timing does not depend on them).

Usage:  python tools/fvd_bench.py [--batch 32] [--frames 16] [--steps 10] [--warmup 3] [--dtypes f16,f32] [--no-eager]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.nn.functional as F

from mebt_amd import i3d as I

PEAK = {"f16": 2.5e15, "f32": 157e12}


def same_pad(x, k, s):
    pads = []
    for d, kk, ss in zip(x.shape[2:], k, s):
        f, b, _ = I.same_pad(d, kk, ss)
        pads.append((f, b))
    return F.pad(x, (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1]))


def eager_unit(u, x):
    x = F.conv3d(same_pad(x, u._kernel_shape, u._stride), u.conv3d.weight, u.conv3d.bias, stride=u._stride)
    if u._use_batch_norm:
        x = F.batch_norm(x, u.bn.running_mean, u.bn.running_var, u.bn.weight, u.bn.bias, False, 0.0, u.bn.eps)
    return F.relu(x) if u._relu else x


def eager_forward(m, x):
    """the reference's forward (pytorch_i3d.py:173-338) as torch eager fp32 ops, for the comparison line only"""
    for ep, kind, a in I._ENDPOINTS:
        mod = getattr(m, ep)
        if kind == 'unit':
            x = eager_unit(mod, x)
        elif kind == 'pool':
            x = F.max_pool3d(same_pad(x, a['k'], a['s']), a['k'], a['s'])
        else:
            b3 = F.max_pool3d(same_pad(x, (3, 3, 3), (1, 1, 1)), 3, 1)
            x = torch.cat([eager_unit(mod.b0, x), eager_unit(mod.b1b, eager_unit(mod.b1a, x)),
                           eager_unit(mod.b2b, eager_unit(mod.b2a, x)), eager_unit(mod.b3b, b3)], 1)
    x = eager_unit(m.logits, F.avg_pool3d(x, (2, 7, 7), 1))
    return x.squeeze(3).squeeze(3).mean(2)


def time_it(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return np.array(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="f16,f32")
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(0)
    m = I.InceptionI3d(400).cuda().eval()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm3d):
                mod.running_mean.uniform_(-0.05, 0.05)
                mod.running_var.uniform_(0.75, 1.25)
    B, T = a.batch, a.frames
    flops = I.plan_flops(T, B=B)
    g = torch.Generator(device="cuda").manual_seed(0)
    videos = torch.randint(0, 256, (B, T, 128, 128, 3), device="cuda", dtype=torch.uint8, generator=g)
    for dt in a.dtypes.split(","):
        m.compute_dtype = dt
        m.forward_uint8(videos)
        ms = time_it(lambda: m.forward_uint8(videos), a.steps, a.warmup)
        med = float(np.median(ms))
        tf = flops / (med * 1e-3) / 1e12
        print(json.dumps({"metric": "i3d_forward", "dtype": dt, "batch": B, "frames": T, "input_hw": [128, 128],
                          "ms_per_batch": round(med, 3), "ms_min": round(float(ms.min()), 3), "ms_max": round(float(ms.max()), 3),
                          "clips_per_s": round(B / (med * 1e-3), 1), "gflop_per_clip": round(flops / B / 1e9, 2),
                          "tflops": round(tf, 1), "frac_of_peak": round(tf * 1e12 / PEAK[dt], 4), "peak_tflops": PEAK[dt] / 1e12}),
              flush=True)
    if not a.no_eager:
        def eager():
            with torch.no_grad():
                x = F.interpolate(videos.flatten(0, 1).permute(0, 3, 1, 2).float(), size=(224, 224), mode="bilinear",
                                  align_corners=False)
                x = (2. * x / 255. - 1).view(B, T, 3, 224, 224).transpose(1, 2).contiguous()
                return eager_forward(m, x)
        ms = time_it(eager, max(2, a.steps // 2), 1)
        med = float(np.median(ms))
        tf = flops / (med * 1e-3) / 1e12
        print(json.dumps({"metric": "i3d_forward", "dtype": "torch_eager_f32", "batch": B, "frames": T, "input_hw": [128, 128],
                          "ms_per_batch": round(med, 3), "ms_min": round(float(ms.min()), 3), "ms_max": round(float(ms.max()), 3),
                          "clips_per_s": round(B / (med * 1e-3), 1), "tflops": round(tf, 1),
                          "frac_of_peak": round(tf * 1e12 / PEAK["f32"], 4), "peak_tflops": PEAK["f32"] / 1e12}), flush=True)


if __name__ == "__main__":
    main()
