#!/usr/bin/env python3
"""Times the LPIPS kernels (csrc/lpips/lpips.hip) on the GPU at 64 images of 128 x 128 (32 pairs: a sixteenth of one measure_recon batch
of 32 clips x 16 frames).  Legs (`--legs`, any of):

  a  the 13-convolution + 4-pool VGG-16 stack on mebt_op_conv2d_3x3, fp16 and fp32
  b  the same stack, same prepared weights, through mebt_op_i3d_conv (k = (1, 3, 3)): the only other in-tree route, the baseline;
     a and b alternate inside every round
  l  the per-layer table of a and b (fp16)
  c  the stack as F.conv2d / F.max_pool2d in torch eager (channels-last), fp16 and fp32, for context
  d  lpips_head on the five slices against the twin's arithmetic written as torch ops on the GPU
  e  the whole LPIPS.__call__ on 32 pairs

Device events around `--iters` back-to-back calls after `--warmup` calls, `--rounds` rounds; every figure is the median with the
min - max over the rounds.  TFLOP/s from the multiply-add count of the 13 convolutions, recomputed here from the shapes
(mebt_amd.lpips.plan_flops: 2 * H * W * Cout * Cin * 9 per layer); the fraction is of the dtype's dense peak (fp16 MFMA 2500 TFLOP/s,
fp32 157.3 TFLOP/s).  Prints a text report (profiles/lpips_bench.txt is one).

    python tools/lpips_bench.py [--images 64] [--size 128] [--iters 10] [--rounds 5] [--legs abdel]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from mebt_amd import lpips as LP

PEAK = {"f16": 2500.0, "f32": 157.3}            # dense TFLOP/s


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters          # ms per call


def spread(xs):
    return f"{statistics.median(xs):9.4f} ms  ({min(xs):.4f} - {max(xs):.4f})"


def random_state_dict(seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in LP.expected_shapes().items():
        if k.startswith("lin"):
            sd[k] = torch.rand(shp, generator=g) * 4 / shp[1]
        elif k.endswith(".weight"):
            sd[k] = torch.randn(shp, generator=g) * (2.0 / (shp[1] * 9)) ** 0.5
        else:
            sd[k] = torch.randn(shp, generator=g) * 0.05
    return sd


def stack(net, conv, x0, bufs, feats=None):
    """the 13 convolutions and 4 pools on `x0` [n, H, W, 3] through `conv`; `feats`: a list that receives the slice outputs (views)"""
    n, h, w = int(x0.shape[0]), int(x0.shape[1]), int(x0.shape[2])
    cur, dst, other, c, k = x0, bufs[0], bufs[1], 3, 0
    for s, ((_, idxs), cout) in enumerate(zip(LP.SLICE_CONVS, LP.CHANNELS)):
        if s > 0:
            nxt = dst[:n * (h // 2) * (w // 2) * c].view(n, h // 2, w // 2, c)
            LP.maxpool_2x2(cur, nxt, net.dtype)
            cur, dst, other, h, w = nxt, other, dst, h // 2, w // 2
        for _i in idxs:
            wgt, b, cin, co = net.convs[k]
            nxt = dst[:n * h * w * cout].view(n, h, w, cout)
            conv(cur, wgt, b, nxt, cin, co, net.dtype)
            cur, dst, other, c, k = nxt, other, dst, cout, k + 1
        if feats is not None:
            feats.append(cur.clone())
    return cur


def torch_stack(sd, x, dtype):
    h = x
    for s, idxs in LP.SLICE_CONVS:
        if s > 1:
            h = F.max_pool2d(h, 2, 2)
        for i in idxs:
            h = F.relu(F.conv2d(h, sd[f"net.slice{s}.{i}.weight"], sd[f"net.slice{s}.{i}.bias"], padding=1))
    return h


def torch_head(f, w):
    """the twin's arithmetic on the GPU in fp32: f [2n, h, w, C] channels-last -> [n]"""
    n = f.shape[0] // 2
    f = f.float()
    nf = f / (torch.sqrt((f * f).sum(-1, keepdim=True)) + 1e-10)
    return (((nf[:n] - nf[n:]) ** 2) * w).sum(-1).mean((1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--legs", type=str, default="abdel")
    args = ap.parse_args()
    dev = torch.device("cuda")
    n, R = args.images, args.size
    if n % 2:
        raise SystemExit("--images must be even (pairs)")
    sd = random_state_dict()
    own_sd = LP.extract(sd)
    total, per = LP.plan_flops(R, R, n)
    g = torch.Generator().manual_seed(1)
    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"{n} images of {R} x {R}: {total / n / 1e9:.3f} GFLOP per image, {total / 1e9:.1f} GFLOP per stack; {args.iters} calls per timing after "
          f"{args.warmup} warm-up calls, {args.rounds} rounds, median (min - max)")
    x_raw = (torch.rand(n, R, R, 3, generator=g) - 0.5) / 0.45

    nets, outs = {}, {}
    for dt in ("f16", "f32"):
        nets[dt] = LP.LPIPS(own_sd, dtype=dt, device=dev)
    if set(args.legs) & set("ab"):
        for dt in ("f16", "f32"):
            net = nets[dt]
            tdt = torch.float16 if dt == "f16" else torch.float32
            x0 = x_raw.to(dev, tdt).contiguous()
            bufs = [torch.empty(n * R * R * 64, device=dev, dtype=tdt) for _ in range(2)]
            a = stack(net, LP.conv2d_3x3, x0, bufs).clone()
            b = stack(net, LP.conv2d_3x3_i3d, x0, bufs).clone()
            print(f"[{dt}] same results: max |own - i3d| on relu5_3 {float((a.float() - b.float()).abs().max()):.3e} (max |value| "
                  f"{float(a.float().abs().max()):.3f})")
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(timed(lambda: stack(net, LP.conv2d_3x3, x0, bufs), args.iters, args.warmup))
                tb.append(timed(lambda: stack(net, LP.conv2d_3x3_i3d, x0, bufs), args.iters, args.warmup))
            ma, mb = statistics.median(ta), statistics.median(tb)
            outs[dt] = (ta, tb)
            print(f"(a) [{dt}] stack on conv2d_3x3: {spread(ta)}  {total / ma / 1e9:7.1f} TFLOP/s  {total / ma / 1e9 / PEAK[dt]:.3f} of peak")
            print(f"(b) [{dt}] stack on i3d_conv  : {spread(tb)}  {total / mb / 1e9:7.1f} TFLOP/s  {total / mb / 1e9 / PEAK[dt]:.3f} of peak")
            print(f"    [{dt}] a over b: {mb / ma:.2f}x faster; ranges {'do not overlap' if max(ta) < min(tb) or max(tb) < min(ta) else 'OVERLAP'}")
    if "l" in args.legs:
        net = nets["f16"]
        print("per-layer, fp16 (each layer alone on its own input; pools apart):")
        print(f"  {'layer':<16}{'map':>9}{'Cin':>5}{'Cout':>6}{'GFLOP':>9}{'own ms':>10}{'TFLOP/s':>9}{'i3d ms':>10}{'TFLOP/s':>9}{'own/i3d':>9}")
        for k, (stem, h, w, cin, cout, fl) in enumerate(per):
            wgt, b, _, _ = net.convs[k]
            x = (torch.rand(n, h, w, cin, generator=g) - 0.3).to(dev, torch.float16)
            out = torch.empty(n, h, w, cout, device=dev, dtype=torch.float16)
            t_own = [timed(lambda: LP.conv2d_3x3(x, wgt, b, out, cin, cout, "f16"), args.iters * 2, args.warmup) for _ in range(args.rounds)]
            t_i3d = [timed(lambda: LP.conv2d_3x3_i3d(x, wgt, b, out, cin, cout, "f16"), args.iters * 2, args.warmup) for _ in range(args.rounds)]
            mo, mi = statistics.median(t_own), statistics.median(t_i3d)
            print(f"  {stem:<16}{f'{h}x{w}':>9}{cin:>5}{cout:>6}{fl / 1e9:>9.2f}{mo:>10.4f}{fl / mo / 1e9:>9.1f}{mi:>10.4f}{fl / mi / 1e9:>9.1f}{mi / mo:>8.2f}x")
        for s, c in enumerate(LP.CHANNELS[:4]):
            h = R >> s
            x = torch.rand(n, h, h, c, generator=g).to(dev, torch.float16)
            out = torch.empty(n, h // 2, h // 2, c, device=dev, dtype=torch.float16)
            t = [timed(lambda: LP.maxpool_2x2(x, out, "f16"), args.iters * 2, args.warmup) for _ in range(args.rounds)]
            print(f"  maxpool_2x2 {h}x{h}x{c}: {spread(t)}  {(x.numel() + out.numel()) * 2 / statistics.median(t) / 1e6:.0f} GB/s")
    if "d" in args.legs:
        for dt in ("f16", "f32"):
            net = nets[dt]
            tdt = torch.float16 if dt == "f16" else torch.float32
            tk, tt = [], []
            feats = []
            stack(net, LP.conv2d_3x3, x_raw.to(dev, tdt).contiguous(), [torch.empty(n * R * R * 64, device=dev, dtype=tdt) for _ in range(2)], feats)
            m = n // 2
            out = torch.zeros(m, device=dev, dtype=torch.float64)
            scratch = torch.empty(LP.head_scratch_bytes(m, R * R) // 8, device=dev, dtype=torch.float64)

            def heads():
                for s, f in enumerate(feats):
                    LP.lpips_head(f, net.lins[s], out, m, f.shape[1] * f.shape[2], f.shape[3], scratch, dtype=dt)

            def torch_heads():
                return sum(torch_head(f, net.lins[s]) for s, f in enumerate(feats))

            out.zero_()
            heads()
            ref = torch_heads()
            print(f"(d) [{dt}] same results: max rel |head - torch fp32| {float(((out - ref.double()).abs() / ref.double()).max()):.2e}")
            for _ in range(args.rounds):
                tk.append(timed(heads, args.iters, args.warmup))
                tt.append(timed(torch_heads, args.iters, args.warmup))
            nbytes = sum(f.numel() * f.element_size() for f in feats)
            print(f"(d) [{dt}] lpips_head, five slices: {spread(tk)}  {nbytes / statistics.median(tk) / 1e6:.0f} GB/s of features")
            print(f"(d) [{dt}] torch ops, five slices : {spread(tt)}  -> {statistics.median(tt) / statistics.median(tk):.1f}x")
    if "e" in args.legs:
        m = n // 2
        x = (torch.rand(m, 3, 1, R, R, generator=g) - 0.5).to(dev)
        y = (x + 0.05 * torch.randn(x.shape, generator=g).to(dev)).contiguous()
        for dt in ("f16", "f32"):
            t = [timed(lambda: nets[dt](x, y), args.iters, args.warmup) for _ in range(args.rounds)]
            med = statistics.median(t)
            print(f"(e) [{dt}] LPIPS.__call__ on {m} pairs: {spread(t)}  {total / med / 1e9:7.1f} TFLOP/s end to end; one measure_recon batch of "
                  f"32 clips x 16 frames = 512 pairs: {med * 512 / m:.1f} ms (derived: {512 // m} x this call)")
    if "c" in args.legs:
        for dt in ("f16", "f32"):
            tdt = torch.float16 if dt == "f16" else torch.float32
            tsd = {k: v.to(dev, tdt) for k, v in own_sd.items()}
            for k in list(tsd):
                if k.endswith(".weight") and tsd[k].dim() == 4:
                    tsd[k] = tsd[k].contiguous(memory_format=torch.channels_last)
            x = x_raw.permute(0, 3, 1, 2).to(dev, tdt).contiguous(memory_format=torch.channels_last)
            with torch.no_grad():
                t = [timed(lambda: torch_stack(tsd, x, tdt), max(2, args.iters // 2), 2) for _ in range(args.rounds)]
            med = statistics.median(t)
            print(f"(c) [{dt}] torch eager F.conv2d stack (channels-last): {spread(t)}  {total / med / 1e9:7.1f} TFLOP/s  "
                  f"{total / med / 1e9 / PEAK[dt]:.3f} of peak")


if __name__ == "__main__":
    main()
