#!/usr/bin/env python3
"""Times the LPIPS backward (csrc/lpips/lpips_bwd.hip, mebt_op_conv2d_3x3_dgrad, `LPIPS.value_and_grad`) on the GPU at 16 and 32 pairs of
128 x 128, fp16 and fp32.  Legs (`--legs`, any of):

  a  `LPIPS.value_and_grad` (taped forward of 2 n images + backward of n) next to `LPIPS.__call__` (the forward as it was) and to torch
     eager autograd of the same network on channels-last tensors (forward of both sides, backward into the reconstruction); the three
     alternate inside every round
  l  the backward alone, per layer: every convolution's data gradient (with the fused ReLU mask where the walk uses one) next to
     F.conv_transpose2d of the same operands in torch eager (channels-last) with the mask applied, the five head_bwd launches, the four
     pool_bwd launches and input_bwd; n images, not 2 n: the real frames take no gradient
  s  `VQGAN.train_step` at the `vq_c5` geometry, batch 16, perceptual_weight 1 against 0

Device events around `--iters` back-to-back calls after `--warmup` calls, `--rounds` rounds; every figure is the median with the
min - max over the rounds.  TFLOP/s from the multiply-add count of the 13 data gradients (mebt_amd.lpips.plan_flops on n images: a data
gradient multiplies what its forward multiplies).  Prints a text report (profiles/lpips_grad_bench.txt is one).

    python tools/lpips_grad_bench.py [--pairs 16,32] [--size 128] [--dtypes f16,f32] [--iters 5] [--rounds 5] [--legs als]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from mebt_amd import lpips as LP

DEV = "cuda"


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


def med(xs):
    return statistics.median(xs)


def spread(xs):
    return f"{med(xs):9.4f} ms  ({min(xs):.4f} - {max(xs):.4f})"


def rounds_of(fns, args, iters=None):
    out = [[] for _ in fns]
    for _ in range(args.rounds):
        for i, fn in enumerate(fns):
            out[i].append(timed(fn, iters or args.iters, args.warmup))
    return out


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


def eager_value_and_grad(tsd, lins, shift, scale, a, b):
    """torch eager autograd of the same network: a, b [n, 3, H, W] channels-last -> d(sum values)/db"""
    b = b.detach().requires_grad_(True)

    def feats(x):
        h, out = (x - shift) / scale, []
        for s, idxs in LP.SLICE_CONVS:
            if s > 1:
                h = F.max_pool2d(h, 2, 2)
            for i in idxs:
                h = F.relu(F.conv2d(h, tsd[f"net.slice{s}.{i}.weight"], tsd[f"net.slice{s}.{i}.bias"], padding=1))
            out.append(h)
        return out
    with torch.no_grad():
        fa = feats(a)
    fb = feats(b)
    val = 0
    for k in range(5):
        n0 = fa[k].float() / (torch.sqrt((fa[k].float() ** 2).sum(1, keepdim=True)) + 1e-10)
        n1 = fb[k].float() / (torch.sqrt((fb[k].float() ** 2).sum(1, keepdim=True)) + 1e-10)
        val = val + (((n0 - n1) ** 2) * lins[k].view(1, -1, 1, 1)).sum(1).mean((1, 2))
    val.sum().backward()
    return b.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=str, default="16,32")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--dtypes", type=str, default="f16,f32")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--legs", type=str, default="als")
    args = ap.parse_args()
    R = args.size
    own = LP.extract(random_state_dict())
    gen = torch.Generator().manual_seed(1)
    print(f"device: {torch.cuda.get_device_name(0)}; {R} x {R}; {args.iters} calls per timing after {args.warmup} warm-up calls, {args.rounds} "
          f"rounds, median (min - max)", flush=True)
    for dt in args.dtypes.split(","):
        tdt = torch.float16 if dt == "f16" else torch.float32
        net = LP.LPIPS(own, dtype=dt, device=DEV)
        tsd = {k: v.to(DEV, tdt) for k, v in own.items()}
        for k in list(tsd):
            if k.endswith(".weight") and tsd[k].dim() == 4:
                tsd[k] = tsd[k].contiguous(memory_format=torch.channels_last)
        lins = [w.to(DEV) for w in net.lins]
        shift, scale = tsd["scaling_layer.shift"].view(1, 3, 1, 1), tsd["scaling_layer.scale"].view(1, 3, 1, 1)
        for n in [int(v) for v in args.pairs.split(",")]:
            total, per = LP.plan_flops(R, R, n)
            tag = f"[{dt} n={n}]"
            if "a" in args.legs:
                x = (torch.rand(n, 3, 1, R, R, generator=gen) - 0.5).to(DEV)
                y = (x + 0.05 * torch.randn(x.shape, generator=gen).to(DEV)).contiguous()
                fr = torch.zeros(n, dtype=torch.int64)
                seed = torch.zeros_like(y)
                xa = x[:, :, 0].to(tdt).contiguous(memory_format=torch.channels_last)
                ya = y[:, :, 0].to(tdt).contiguous(memory_format=torch.channels_last)
                net.value_and_grad(x, y, fr, seed, 1.0)
                ge = eager_value_and_grad(tsd, lins, shift, scale, xa, ya).float()
                print(f"(a) {tag} same gradient: max |kernels - eager| {float((seed[:, :, 0] - ge).abs().max()):.3e} of max |g| "
                      f"{float(ge.abs().max()):.3e}", flush=True)
                tv, tf, te = rounds_of([lambda: net.value_and_grad(x, y, fr, seed, 1.0), lambda: net(x, y, fr),
                                        lambda: eager_value_and_grad(tsd, lins, shift, scale, xa, ya)], args)
                print(f"(a) {tag} LPIPS.value_and_grad         : {spread(tv)}", flush=True)
                print(f"(a) {tag} LPIPS.__call__ (forward only): {spread(tf)}  the tape and the backward add {med(tv) - med(tf):.3f} ms "
                      f"({total / (med(tv) - med(tf)) / 1e9:.1f} TFLOP/s of data gradient)", flush=True)
                print(f"(a) {tag} torch eager autograd         : {spread(te)}  = {med(te) / med(tv):.2f} x value_and_grad; ranges "
                      f"{'do not overlap' if max(tv) < min(te) or max(te) < min(tv) else 'OVERLAP'}", flush=True)
            if "l" in args.legs:
                wd = net._dgrad_weights()
                print(f"(l) {tag} backward per layer ({n} images; eager: F.conv_transpose2d, channels-last, times the mask):", flush=True)
                print(f"  {'layer':<16}{'map':>9}{'dy C':>6}{'dx C':>6}{'GFLOP':>9}{'own ms':>10}{'TFLOP/s':>9}{'eager ms':>10}{'eager/own':>10}", flush=True)
                first = {0, 2, 4, 7, 10}
                for k, (stem, h, w, cin, cout, fl) in reversed(list(enumerate(per))):
                    dy = torch.randn(n, h, w, cout, generator=gen).to(DEV, tdt)
                    yp = None if k in first else torch.randn(n, h, w, cin, generator=gen).to(DEV, tdt)
                    dx = torch.empty(n, h, w, cin, device=DEV, dtype=tdt)
                    wt = tsd[stem + ".weight"]
                    dyc = dy.permute(0, 3, 1, 2)
                    ypc = None if yp is None else yp.permute(0, 3, 1, 2)

                    def eager():
                        r = F.conv_transpose2d(dyc, wt, padding=1)
                        return r if ypc is None else r * (ypc > 0)
                    to, te = rounds_of([lambda: LP.conv2d_3x3_dgrad(dy, wd[k], yp, dx, cout, cin, dt), eager], args, args.iters * 2)
                    print(f"  {stem:<16}{f'{h}x{w}':>9}{cout:>6}{cin:>6}{fl / 1e9:>9.2f}{med(to):>10.4f}{fl / med(to) / 1e9:>9.1f}{med(te):>10.4f}"
                          f"{med(te) / med(to):>9.2f}x{'   LOSES to eager' if med(te) < med(to) else ''}", flush=True)
                for s, c in enumerate(LP.CHANNELS):
                    h = R >> s
                    f = torch.relu(torch.randn(2 * n, h, h, c, generator=gen)).to(DEV, tdt)
                    add = torch.randn(n, h, h, c, generator=gen).to(DEV, tdt)
                    out = torch.empty(n, h, h, c, device=DEV, dtype=tdt)
                    t = rounds_of([lambda: LP.lpips_head_bwd(f, net.lins[s], out, n, h * h, c, 1.0, add, dt)], args, args.iters * 2)[0]
                    nbytes = (f.numel() + add.numel() + out.numel()) * f.element_size()
                    print(f"  head_bwd slice {s + 1} {h}x{h}x{c}: {spread(t)}  {nbytes / med(t) / 1e6:.0f} GB/s", flush=True)
                for s, c in enumerate(LP.CHANNELS[:4]):
                    h = R >> s
                    x = torch.relu(torch.randn(n, h, h, c, generator=gen)).to(DEV, tdt)
                    dy = torch.randn(n, h // 2, h // 2, c, generator=gen).to(DEV, tdt)
                    dx = torch.empty_like(x)
                    t = rounds_of([lambda: LP.maxpool_2x2_bwd(x, dy, dx, dt)], args, args.iters * 2)[0]
                    nbytes = (2 * x.numel() + dy.numel()) * x.element_size()
                    print(f"  maxpool_2x2_bwd {h}x{h}x{c}: {spread(t)}  {nbytes / med(t) / 1e6:.0f} GB/s", flush=True)
                d = torch.randn(n, R, R, 3, generator=gen).to(DEV, tdt)
                seed = torch.zeros(n, 3, 1, R, R, device=DEV)
                host = torch.stack([torch.arange(n), torch.zeros(n, dtype=torch.int64)], -1).to(torch.int32)
                fdev = host.to(DEV)
                t = rounds_of([lambda: LP.lpips_input_bwd(d, fdev, host, seed, LP.SCALE, 1.0, dt)], args, args.iters * 2)[0]
                print(f"  lpips_input_bwd {R}x{R}x3: {spread(t)}", flush=True)
    if "s" in args.legs:
        from mebt_amd.vqgan import VQGAN
        B = 16
        x = (torch.rand(B, 3, 16, 128, 128, generator=torch.Generator().manual_seed(B)) - 0.5).to(DEV)
        for dt in args.dtypes.split(","):
            res = {}
            for pw in (0.0, 1.0):
                a = argparse.Namespace(n_hiddens=32, downsample=(4, 8, 8), image_channels=3, embedding_dim=256, n_codes=16384, sequence_length=16,
                                       sample_every_n_frames=1, resolution=128, l1_weight=4.0, perceptual_weight=pw, lr=3e-4)
                torch.manual_seed(0)
                m = VQGAN(a)
                m.compute_dtype = dt
                m.lpips_weights = own
                m = m.to(DEV).train()
                opt = m.configure_optimizers()
                g = torch.Generator(device=DEV).manual_seed(1)
                m.train_step(x, opt, generator=g)                      # the initialisation, Adam's state
                res[pw] = (m, opt, g)
            fns = [lambda pw=pw: res[pw][0].train_step(x, res[pw][1], generator=res[pw][2]) for pw in (0.0, 1.0)]
            print(f"(s) [{dt} B={B}] timing {args.rounds} rounds of 2 x {args.iters + args.warmup} steps ...", flush=True)
            t0, t1 = rounds_of(fns, args)
            print(f"(s) [{dt} B={B}] train_step, perceptual_weight 0: {spread(t0)}", flush=True)
            print(f"(s) [{dt} B={B}] train_step, perceptual_weight 1: {spread(t1)}  the term adds {med(t1) - med(t0):.3f} ms "
                  f"({100 * (med(t1) - med(t0)) / med(t0):.2f} %)", flush=True)
            del res
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
