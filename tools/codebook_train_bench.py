#!/usr/bin/env python3
"""Times the EMA codebook update (csrc/codebook/codebook_train.hip, `Codebook.update`) and `VQGAN.train_step` on the GPU at the `vq_c5`
geometry (16384 codes of 256 dims; batch 4 and 16 of 16 x 128 x 128 clips: M = 4096 and 16384 latent rows).  Legs (`--legs`, any of):

  u  the update alone on random z and ids: mebt_op_codebook_sums, mebt_op_codebook_restart_rows and mebt_op_codebook_ema one by one and
     `Codebook.update` as a whole, next to the torch eager form of reference codebook.py:68-89 on the same device (the one-hot matrix, the
     d x M x n_codes product, `_tile` where M < n_codes, randperm, the restart blend); also with every row on ONE code (a collapsed
     codebook: the longest list one wave can get)
  s  `train_step` (zero_grad + recon_backward(update_codebook=True) + Adam) next to `recon_backward` + `optimizer.step()` with the codebook
     frozen, which is what the parent of this operator could do

Device events around `--iters` back-to-back calls after `--warmup` calls, `--rounds` alternating rounds; every figure is the median with
the min - max over the rounds.  Prints a text report (profiles/codebook_train_bench.txt is one).

    python tools/codebook_train_bench.py [--batches 4,16] [--dtypes f16] [--legs us] [--iters 5] [--rounds 3]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from mebt_amd.vqgan import VQGAN, Codebook

DEV = "cuda"
N_CODES, D = 16384, 256


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
    out = [[] for _ in fns]
    for _ in range(args.rounds):
        for i, fn in enumerate(fns):
            out[i].append(timed(fn, args.iters, args.warmup))
    return out


def eager_update(cb, z, ids):
    """reference codebook.py:68-89 in torch eager on the buffers' device (single rank)"""
    n_codes = cb.n_codes
    onehot = F.one_hot(ids, n_codes).type_as(z)
    n_total = onehot.sum(dim=0)
    encode_sum = z.t() @ onehot
    cb.N.mul_(0.99).add_(n_total, alpha=0.01)
    cb.z_avg.mul_(0.99).add_(encode_sum.t(), alpha=0.01)
    n = cb.N.sum()
    weights = (cb.N + 1e-7) / (n + n_codes * 1e-7) * n
    cb.embeddings.copy_(cb.z_avg / weights.unsqueeze(1))
    y = z
    if z.shape[0] < n_codes:
        y = z.repeat((n_codes + z.shape[0] - 1) // z.shape[0], 1)
        y = y + torch.randn_like(y) * (0.01 / D ** 0.5)
    k_rand = y[torch.randperm(y.shape[0], device=z.device)][:n_codes]
    usage = (cb.N.view(n_codes, 1) >= cb.restart_thres).float()
    cb.embeddings.mul_(usage).add_(k_rand * (1 - usage))


def build(dtype):
    a = argparse.Namespace(n_hiddens=32, downsample=(4, 8, 8), image_channels=3, embedding_dim=D, n_codes=N_CODES, sequence_length=16,
                           sample_every_n_frames=1, resolution=128, l1_weight=4.0, perceptual_weight=0.0, lr=3e-4)
    torch.manual_seed(0)
    m = VQGAN(a)
    m.compute_dtype = dtype
    return m.to(DEV).train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=str, default="4,16")
    ap.add_argument("--dtypes", type=str, default="f16")
    ap.add_argument("--legs", type=str, default="us")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}; vq_c5 geometry, {N_CODES} codes of {D} dims; {args.iters} calls per timing after {args.warmup} "
          f"warm-up, {args.rounds} rounds, median (min - max)", flush=True)
    batches = [int(b) for b in args.batches.split(",")]
    if "u" in args.legs:
        for B in batches:
            M = B * 4 * 16 * 16
            g = torch.Generator(device=DEV).manual_seed(B)
            z = torch.randn(M, D, device=DEV, generator=g)
            for what, ids in (("random ids", torch.randint(0, N_CODES, (M,), device=DEV, generator=g)),
                              ("one code", torch.full((M,), 7, device=DEV, dtype=torch.int64))):
                cb = Codebook(N_CODES, D).to(DEV)
                cb.init_from(z, generator=g)
                ref = Codebook(N_CODES, D).to(DEV)
                ref.load_state_dict(cb.state_dict())
                tag = f"[M={M} {what}]"
                n_total, encode_sum = Codebook.code_sums(ids, z, N_CODES)
                k_rand = cb.restart_rows(z, generator=g)
                src = torch.randperm(M * max(1, -(-N_CODES // M)), device=DEV, generator=g)[:N_CODES]
                noise = torch.randn(N_CODES, D, device=DEV, generator=g) if M < N_CODES else None
                from mebt_amd import _lib
                lib = _lib.load()
                nbytes = int(lib.mebt_codebook_ema_scratch_bytes(N_CODES))
                scratch = torch.empty(nbytes // 8 + 1, device=DEV, dtype=torch.float64)
                restarted = torch.empty(1, device=DEV, dtype=torch.int32)

                def ema():
                    _lib.check(lib.mebt_op_codebook_ema(_lib.ptr(cb.N), _lib.ptr(cb.z_avg), _lib.ptr(cb.embeddings), _lib.ptr(n_total), _lib.ptr(encode_sum),
                                                        _lib.ptr(k_rand), _lib.ptr(restarted), N_CODES, D, 1.0, _lib.ptr(scratch), nbytes, _lib.cur_stream()))
                ts, tr, te, tu, tt = rounds_of([lambda: Codebook.code_sums(ids, z, N_CODES), lambda: cb.restart_rows(z, src, noise), ema,
                                                lambda: cb.update(z, ids, generator=g), lambda: eager_update(ref, z, ids)], args)
                print(f"(u) {tag} codebook_sums (with its allocations)       : {spread(ts)}", flush=True)
                print(f"(u) {tag} codebook_restart_rows (draws handed in)    : {spread(tr)}", flush=True)
                print(f"(u) {tag} codebook_ema                               : {spread(te)}", flush=True)
                print(f"(u) {tag} Codebook.update (sums + draws + rows + ema): {spread(tu)}", flush=True)
                print(f"(u) {tag} torch eager codebook.py:68-89 (one-hot)    : {spread(tt)}  = {med(tt) / med(tu):.1f} x Codebook.update", flush=True)
    if "s" in args.legs:
        for dtype in args.dtypes.split(","):
            for B in batches:
                x = (torch.rand(B, 3, 16, 128, 128, generator=torch.Generator().manual_seed(B)) - 0.5).to(DEV)
                tag = f"[{dtype} B={B}]"
                m = build(dtype)
                opt = m.configure_optimizers()
                g = torch.Generator(device=DEV).manual_seed(1)
                m.train_step(x, opt, generator=g)                      # the initialisation, Adam's state

                def frozen():
                    opt.zero_grad()
                    m.recon_backward(x)
                    opt.step()
                tf, tt = rounds_of([frozen, lambda: m.train_step(x, opt, generator=g)], args)
                print(f"(s) {tag} zero_grad + recon_backward + Adam, codebook frozen: {spread(tf)}", flush=True)
                print(f"(s) {tag} train_step (the same with update_codebook=True)   : {spread(tt)}  the update adds {med(tt) - med(tf):.3f} ms "
                      f"({100 * (med(tt) - med(tf)) / med(tf):.2f} %)", flush=True)
                del m, opt
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
