#!/usr/bin/env python3
"""Times the discriminators' forward (csrc/disc/disc_conv.hip, mebt_amd.discriminator.DiscRunner) on the GPU at the workload shape:
ndf 64, L 3, clips [B, 3, 16, 128, 128] for the video network and frames [B, 3, 128, 128] for the image network, fp16 and fp32.
Legs (`--legs`, any of):

  a  this forward: the whole call of both networks in eval and training mode, and every stage alone on its own input (ingest,
     convolution with and without the BatchNorm slots, the normalise pass, the one-channel stage)
  b  the same arranged weights through mebt_op_i3d_conv (padding 2 front and back) for the stages its LDS tap table admits: the only
     other in-tree route; a and b alternate inside every round
  c  the reference's definition in torch eager on the same card, channels-last, fp16 and fp32, eval and training mode

Device events around `--iters` back-to-back calls after `--warmup` calls, `--rounds` rounds; every figure is the median with the
min - max over the rounds.  TFLOP/s from discriminator.plan_flops (2 per multiply-add, computed from the shapes); GB/s of the ingest
and the normalise pass from the bytes they read and write.  Prints a text report (profiles/disc_bench.txt is one).

    python tools/disc_bench.py [--batch 4] [--iters 5] [--rounds 5] [--legs abc]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn as nn

from mebt_amd import _lib
from mebt_amd import discriminator as D

PEAK = {"f16": 2500.0, "f32": 157.3}            # dense TFLOP/s
I3D_MAX_TAB = 2048                              # csrc/i3d/i3d.hip


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


def holder(three_d, seed=0):
    net = (D.NLayerDiscriminator3D if three_d else D.NLayerDiscriminator)(3, 64, 3)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            if k.endswith(".0.weight"):
                v.copy_(torch.randn(v.shape, generator=g) * (2.0 / v[0].numel()) ** 0.5)
            elif k.endswith("running_var"):
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
            elif v.dtype.is_floating_point:
                v.copy_(torch.randn(v.shape, generator=g) * 0.1 + (1.0 if k.endswith(".1.weight") else 0.0))
    return net.cuda().eval()


def i3d_admits(e, cin_store, dt):
    vec = 8 if dt == "f16" else 4
    kpad = -(-(e["kt"] * 16 * cin_store) // 32) * 32
    return (kpad // vec if cin_store % vec == 0 else kpad) <= I3D_MAX_TAB


def i3d_conv(dt, h, w, bias, out, kt, stride):
    from mebt_amd.i3d import _ConvDesc
    d = _ConvDesc()
    d.in_, d.w, d.bias = h.data_ptr(), w.data_ptr(), bias.data_ptr()
    d.B, d.Ti, d.Hi, d.Wi, d.Cin = h.shape
    d.To, d.Ho, d.Wo, d.Cout = out.shape[1:]
    for a in range(3):
        one = a == 0 and kt == 1
        d.k[a], d.s[a], d.pad_front[a], d.pad_back[a] = (1, 1, 0, 0) if one else (4, stride, 2, 2)
    d.relu, d.nseg = 0, 1
    d.seg[0].out, d.seg[0].n0, d.seg[0].n1, d.seg[0].cstride, d.seg[0].coff = out.data_ptr(), 0, out.shape[-1], out.shape[-1], 0
    _lib.check(_lib.load().mebt_op_i3d_conv(_lib.dtype_code(dt), C.byref(d), _lib.cur_stream()))


def torch_reference(three_d, net, tdt):
    conv, norm = (nn.Conv3d, nn.BatchNorm3d) if three_d else (nn.Conv2d, nn.BatchNorm2d)
    mods = []
    for n, (cin, cout, s, bn, act) in enumerate(D.stage_channels(3, 64, 3)):
        mods.append(conv(cin, cout, 4, stride=s, padding=2))
        if bn:
            mods.append(norm(cout))
        if act:
            mods.append(nn.LeakyReLU(0.2, True))
    ref = nn.Sequential(*mods)
    own = [v for v in net.state_dict().values()]
    with torch.no_grad():
        for dst, src in zip(ref.state_dict().values(), own):
            dst.copy_(src)
    return ref.cuda().to(tdt).to(memory_format=torch.channels_last_3d if three_d else torch.channels_last)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4, help="clips per call (and frames per call of the image network)")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--legs", type=str, default="abc")
    args = ap.parse_args()
    B = args.batch
    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"ndf 64, L 3, batch {B}: clips [{B}, 3, 16, 128, 128], frames [{B}, 3, 128, 128]; {args.iters} calls per timing after {args.warmup} "
          f"warm-up calls, {args.rounds} rounds, median (min - max)")
    g = torch.Generator().manual_seed(1)
    for three_d in (True, False):
        name = "video" if three_d else "image"
        net = holder(three_d)
        shape = (B, 3, 16, 128, 128) if three_d else (B, 3, 128, 128)
        x = (torch.rand(shape, generator=g) - 0.5).cuda()
        plan = net.plan(shape)
        total = D.plan_flops(plan, B)
        print(f"\n== {name} network: {total / B / 1e9:.2f} GFLOP per {'clip' if three_d else 'frame'}, {total / 1e9:.1f} GFLOP per call")
        for dt in ("f16", "f32"):
            tdt = _lib.torch_dtype(dt)
            r = D.DiscRunner(net, dt)
            eb = 2 if dt == "f16" else 4
            if "a" in args.legs:
                for training in (False, True):
                    net.train(training)
                    t = [timed(lambda: r(x, update_running=False), args.iters, args.warmup) for _ in range(args.rounds)]
                    med = statistics.median(t)
                    print(f"(a) [{dt}] {name} whole call, {'training' if training else 'eval'} mode: {spread(t)}  {total / med / 1e9:7.1f} TFLOP/s  "
                          f"{total / med / 1e9 / PEAK[dt]:.3f} of peak")
                net.eval()
            if set(args.legs) & set("ab"):
                t = [timed(lambda: D.ingest(x, dt), args.iters, args.warmup) for _ in range(args.rounds)]
                h = D.ingest(x, dt)
                print(f"    [{dt}] ingest: {spread(t)}  {(x.numel() * 4 + h.numel() * eb) / statistics.median(t) / 1e6:.0f} GB/s")
                print(f"    {'stage':<8}{'out map':>14}{'Cin':>5}{'Cout':>6}{'K':>7}{'GFLOP':>9}{'own ms':>10}{'TFLOP/s':>9}{'+slots ms':>11}{'i3d ms':>10}"
                      f"{'TFLOP/s':>9}{'own/i3d':>9}{'bn_act ms':>11}{'GB/s':>7}")
                for e, st in zip(plan, r.stages):
                    fl = D.plan_flops([e], B)
                    cin_store = h.shape[-1]
                    od = "x".join(str(v) for v in e["out_dims"])
                    if st["cout"] == 1:
                        t_own = [timed(lambda: D.head_stage(h, st["w"], st["bias"], r.kt), args.iters, args.warmup) for _ in range(args.rounds)]
                        mo = statistics.median(t_own)
                        print(f"    {e['stage']:<8}{od:>14}{cin_store:>5}{1:>6}{e['kt'] * 16 * cin_store:>7}{fl / 1e9:>9.2f}{mo:>10.4f}{fl / mo / 1e9:>9.1f}"
                              f"{'':>11}{'':>10}{'':>9}{'':>9}{'':>11}{'':>7}   (one wave per voxel; min {min(t_own):.4f} max {max(t_own):.4f})")
                        continue
                    conv = lambda slots=False: D.conv_stage(h, st["w"], st["bias"], r.kt, st["stride"], st["cout"], act=not st["bn"], slots=slots)
                    out = conv()
                    admits = "b" in args.legs and i3d_admits(e, cin_store, dt)
                    other = torch.empty_like(out)
                    t_own, t_sl, t_i3d, t_bn = [], [], [], []
                    for _ in range(args.rounds):
                        t_own.append(timed(conv, args.iters, args.warmup))
                        if admits:
                            t_i3d.append(timed(lambda: i3d_conv(dt, h, st["w"], st["bias"], other, r.kt, st["stride"]), args.iters, args.warmup))
                        if st["bn"]:
                            t_sl.append(timed(lambda: conv(True), args.iters, args.warmup))
                    mo = statistics.median(t_own)
                    line = (f"    {e['stage']:<8}{od:>14}{cin_store:>5}{st['cout']:>6}{e['kt'] * 16 * cin_store:>7}{fl / 1e9:>9.2f}{mo:>10.4f}"
                            f"{fl / mo / 1e9:>9.1f}")
                    line += f"{statistics.median(t_sl):>11.4f}" if t_sl else f"{'':>11}"
                    if admits:
                        mi = statistics.median(t_i3d)
                        plain = out if st["bn"] else D.conv_stage(h, st["w"], st["bias"], r.kt, st["stride"], st["cout"])     # i3d leg: no activation
                        same = float((plain.float() - other.float()).abs().max())
                        line += f"{mi:>10.4f}{fl / mi / 1e9:>9.1f}{mi / mo:>8.2f}x"
                    else:
                        same = None
                        line += f"{'':>10}{'':>9}{'':>9}"
                    if st["bn"]:
                        stats = torch.stack([st["norm"].running_mean, torch.rsqrt(st["norm"].running_var + 1e-5)]).contiguous()
                        t_bn = [timed(lambda: D.bn_act(out, stats, st["gamma"], st["beta"]), args.iters, args.warmup) for _ in range(args.rounds)]
                        mb = statistics.median(t_bn)
                        line += f"{mb:>11.4f}{2 * out.numel() * eb / mb / 1e6:>7.0f}"
                    else:
                        line += f"{'':>11}{'':>7}"
                    line += f"   own {min(t_own):.4f}-{max(t_own):.4f}"
                    if admits:
                        line += f", i3d {min(t_i3d):.4f}-{max(t_i3d):.4f}, max |own - i3d| {same:.2e}"
                    print(line)
                    h = conv()
                    if st["bn"]:
                        D.bn_act(h, stats, st["gamma"], st["beta"])
            if "c" in args.legs:
                ref = torch_reference(three_d, net, tdt)
                xc = x.to(tdt).contiguous(memory_format=torch.channels_last_3d if three_d else torch.channels_last)
                with torch.no_grad():
                    for training in (False, True):
                        ref.train(training)
                        t = [timed(lambda: ref(xc), max(2, args.iters // 2), 2) for _ in range(args.rounds)]
                        med = statistics.median(t)
                        print(f"(c) [{dt}] {name} torch eager (channels-last), {'training' if training else 'eval'} mode: {spread(t)}  "
                              f"{total / med / 1e9:7.1f} TFLOP/s  {total / med / 1e9 / PEAK[dt]:.3f} of peak")


if __name__ == "__main__":
    main()
