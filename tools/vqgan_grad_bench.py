#!/usr/bin/env python3
"""Times the first-stage backward (csrc/vqgan_bwd/vqgan_bwd.hip, `VQGAN.recon_backward`) on the GPU at the `vq_c5` geometry (n_hiddens 32, downsample
(4, 8, 8), 16384 codes of 256 dims, clips of 16 x 128 x 128).  Legs (`--legs`, any of):

  w  the whole `recon_backward` (training forward + backward + the gradient accumulation), and `encode` + `decode` alone for the ratio
  l  every distinct layer of the tape on its own: the convolution's weight gradient (mebt_op_conv3d_wgrad, all classes) and data gradient
     (mebt_op_pad_zero + mebt_op_conv3d per class + mebt_op_halo_fold), the GroupNorm + SiLU backward; next to each, torch eager autograd of
     the same layer (F.pad replicate + F.conv3d / F.conv_transpose3d, F.group_norm + SiLU; channels-last-3d) as backward = (forward +
     backward) - forward
  t  torch eager autograd of the whole stack on the same GPU: forward + backward of the same objective, the outside baseline

Device events around `--iters` back-to-back calls after `--warmup` calls, `--rounds` alternating rounds; every figure is the median with
the min - max over the rounds.  Prints a text report (profiles/vqgrad_bench.txt is one).

    python tools/vqgan_grad_bench.py [--batches 4,16] [--dtypes f16,f32] [--legs wlt] [--iters 2] [--rounds 3]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch
import torch.nn.functional as F

from mebt_amd.vqgan import VQGAN, SamePadConv3d, SamePadConvTranspose3d

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
    return f"{med(xs):10.3f} ms  ({min(xs):.3f} - {max(xs):.3f})"


def rounds_of(fns, args):
    """alternating rounds over several callables -> one list of per-call ms each"""
    out = [[] for _ in fns]
    for _ in range(args.rounds):
        for i, fn in enumerate(fns):
            out[i].append(timed(fn, args.iters, args.warmup))
    return out


def build(dtype):
    a = argparse.Namespace(n_hiddens=32, downsample=(4, 8, 8), image_channels=3, embedding_dim=256, n_codes=16384, sequence_length=16,
                           sample_every_n_frames=1, resolution=128, l1_weight=4.0, perceptual_weight=0.0, lr=3e-4)
    torch.manual_seed(0)
    m = VQGAN(a)
    m.compute_dtype = dtype
    return m.to(DEV).eval()


def same_pad(kernel, stride):
    pad = []
    for k, s in zip(kernel[::-1], stride[::-1]):
        p = k - s
        pad += [p // 2 + p % 2, p // 2]
    return tuple(pad)


def torch_conv(mod, x):
    if isinstance(mod, SamePadConv3d):
        return F.conv3d(F.pad(x, same_pad(mod.kernel_size, mod.stride), mode="replicate"), mod.conv.weight.to(x.dtype), mod.conv.bias.to(x.dtype), stride=mod.stride)
    return F.conv_transpose3d(F.pad(x, same_pad(mod.kernel_size, mod.stride), mode="replicate"), mod.convt.weight.to(x.dtype), mod.convt.bias.to(x.dtype),
                              stride=mod.stride, padding=tuple(k - 1 for k in mod.kernel_size))


def torch_ns(gn, x):
    h = F.group_norm(x, 32, gn.weight.to(x.dtype), gn.bias.to(x.dtype), eps=1e-6)
    return h * torch.sigmoid(h)


def torch_objective(m, x, tdt):
    """the same stack in torch eager (channels-last-3d activations of `tdt`, the ids from the codebook search in fp32) -> loss"""
    cl = torch.channels_last_3d

    def res(r, h):
        t = torch_conv(r.conv1, torch_ns(r.norm1, h))
        return h + torch_conv(r.conv2, torch_ns(r.norm2, t))

    h = torch_conv(m.encoder.conv_first, x.to(tdt).contiguous(memory_format=cl))
    for blk in m.encoder.conv_blocks:
        h = res(blk.res, torch_conv(blk.down, h))
    z = torch_conv(m.pre_vq_conv, torch_ns(m.encoder.final_block[0], h)).float()
    flat = z.permute(0, 2, 3, 4, 1).reshape(-1, z.shape[1])
    e = m.codebook.embeddings
    with torch.no_grad():
        ids = ((flat ** 2).sum(1, keepdim=True) - 2 * flat @ e.t() + (e ** 2).sum(1)[None]).argmin(1)
    q = e[ids].view(z.shape[0], *z.shape[2:], -1).permute(0, 4, 1, 2, 3)
    commit = 0.25 * F.mse_loss(z, q)
    h = (z + (q - z).detach()).to(tdt)
    h = torch_ns(m.decoder.final_block[0], torch_conv(m.post_vq_conv, h))
    for blk in m.decoder.conv_blocks:
        h = res(blk.res2, res(blk.res1, torch_conv(blk.up, h)))
    rec = torch_conv(m.decoder.conv_last, h).float()
    return F.l1_loss(rec, x) * 4.0 + commit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=str, default="4,16")
    ap.add_argument("--dtypes", type=str, default="f16,f32")
    ap.add_argument("--legs", type=str, default="wlt")
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}; vq_c5 geometry; {args.iters} calls per timing after {args.warmup} warm-up, {args.rounds} rounds, "
          f"median (min - max)", flush=True)
    for dtype in args.dtypes.split(","):
        tdt = torch.float16 if dtype == "f16" else torch.float32
        m = build(dtype)
        for B in (int(b) for b in args.batches.split(",")):
            g = torch.Generator().manual_seed(B)
            x = (torch.rand(B, 3, 16, 128, 128, generator=g) - 0.5).to(DEV)
            tag = f"[{dtype} B={B}]"
            if "w" in args.legs:
                out = m.recon_backward(x)
                tf, tb = rounds_of([lambda: m.decode(m.encode(x)), lambda: m.recon_backward(x)], args)
                for p in m.parameters():
                    p.grad = None
                print(f"(w) {tag} encode + decode  : {spread(tf)}", flush=True)
                print(f"(w) {tag} recon_backward   : {spread(tb)}  = {med(tb) / med(tf):.2f} x the forward; backward alone {med(tb) - med(tf):.3f} ms; "
                      f"grad_scale {out['grad_scale']:g}, finite {out['finite']}", flush=True)
            if "l" in args.legs:
                m._prepare()
                m._tape = {}
                ids = m.encode(x)
                m.decode(ids)
                tape, m._tape = m._tape, None
                nbytes = sum(v[0].numel() * v[0].element_size() for v in tape.values()) + sum(v[1].numel() * 4 for k, v in tape.items() if not isinstance(k, str))
                print(f"(l) {tag} tape: {len(tape)} entries, {nbytes / 2 ** 30:.2f} GiB (convolution and GroupNorm inputs, statistics)", flush=True)
                print(f"  {'layer':<40}{'in dims':>14}{'wgrad ms':>10}{'dgrad ms':>10}{'torch bwd ms':>14}{'ours/torch':>11}")
                seen, flags, lose = set(), [], []
                mods = dict(m.named_modules())
                for key, val in tape.items():
                    if isinstance(key, str):
                        xin, dims, in_mode, out_mode = val
                        cv, mod = m._prepared["convs"][key], mods[key]
                        sig = ("c", cv.transposed, cv.kernel, cv.stride, cv.cin, cv.cout, dims)
                        if sig in seen:
                            continue
                        seen.add(sig)
                        od = cv.out_dims(dims)
                        if out_mode == 2:
                            dy = torch.randn(B, cv.cout, *od, device=DEV) * 0.05
                        else:
                            dy = (torch.randn(B, *od, cv.cout, device=DEV) * 0.05).to(tdt if out_mode == 0 else torch.float32)
                        tw, = rounds_of([lambda: m._conv_wgrad(key, xin, dy, B, dims, in_mode, out_mode, 1.0)], args)
                        td = [0.0]
                        if key != "encoder.conv_first":
                            td, = rounds_of([lambda: m._conv_dgrad(key, dy, B, dims, out_mode)], args)
                        xt = (xin if in_mode == 1 else xin.permute(0, 4, 1, 2, 3)).to(tdt).detach().requires_grad_(key != "encoder.conv_first")
                        dyt = (dy if out_mode == 2 else dy.permute(0, 4, 1, 2, 3)).to(tdt)
                        wts = [p for p in mod.parameters()]

                        def t_fwd():
                            with torch.no_grad():
                                torch_conv(mod, xt)

                        def t_both():
                            torch.autograd.grad(torch_conv(mod, xt), ([xt] if xt.requires_grad else []) + wts, dyt)
                        t1, t2 = rounds_of([t_fwd, t_both], args)
                        ours, theirs = med(tw) + med(td), med(t2) - med(t1)
                        name = key
                    else:
                        xin, stats, _, dims = val
                        gn = next(mm for mm in m.modules() if id(mm) == key)
                        sig = ("g", xin.shape[-1], dims)
                        if sig in seen:
                            continue
                        seen.add(sig)
                        dy = (torch.randn_like(xin.float()) * 0.05).to(tdt)
                        tape1 = {key: val}
                        tw, = rounds_of([lambda: m._norm_silu_bwd(gn, dy, tape1, 1.0, flags)], args)
                        td = [0.0]
                        xt = xin.permute(0, 4, 1, 2, 3).detach().requires_grad_(True)
                        dyt = dy.permute(0, 4, 1, 2, 3)

                        def t_fwd():
                            with torch.no_grad():
                                torch_ns(gn, xt)

                        def t_both():
                            torch.autograd.grad(torch_ns(gn, xt), [xt, gn.weight, gn.bias], dyt)
                        t1, t2 = rounds_of([t_fwd, t_both], args)
                        ours, theirs = med(tw), med(t2) - med(t1)
                        name = f"groupnorm_silu C={xin.shape[-1]}"
                    for p in m.parameters():
                        p.grad = None
                    flags.clear()
                    if ours > theirs:
                        lose.append(f"{name} {tuple(dims)}")
                    print(f"  {name:<40}{str(tuple(dims)):>14}{med(tw):>10.3f}{med(td):>10.3f}{theirs:>14.3f}{ours / max(theirs, 1e-6):>10.2f}x", flush=True)
                print(f"(l) {tag} slower than torch eager: {', '.join(lose) if lose else 'none'}", flush=True)
            if "t" in args.legs:
                def t_fwd():
                    with torch.no_grad():
                        torch_objective(m, x, tdt)

                def t_both():
                    torch_objective(m, x, tdt).backward()
                    for p in m.parameters():
                        p.grad = None
                try:
                    t1, t2 = rounds_of([t_fwd, t_both], args)
                    print(f"(t) {tag} torch eager forward           : {spread(t1)}", flush=True)
                    print(f"(t) {tag} torch eager forward + backward: {spread(t2)}  backward alone {med(t2) - med(t1):.3f} ms", flush=True)
                except RuntimeError as err:          # e.g. out of memory in a library workspace: say so, do not stop the report
                    print(f"(t) {tag} torch eager did not run: {str(err).splitlines()[0]}", flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
