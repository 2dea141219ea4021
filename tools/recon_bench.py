#!/usr/bin/env python3
"""Times the reconstruction-metric kernels (csrc/recon/recon.hip) on the GPU at the size of one measure_fvd batch of config-5 clips:
clip_quality_u8 on uint8 [32 * 16, 128, 128, 3] against the same arithmetic written as torch ops in fp32 on the same GPU (the twin of
mebt_amd/recon.py with float32 in place of float64: five windowed moments through conv2d, the SSIM map, the means), plus abs_diff_sum
and code_stats at the matching sizes.  Device events around `--iters` back-to-back calls after `--warmup` calls, the two SSIM versions
alternating over `--rounds` rounds; prints a text report (profiles/recon_kernels.txt is one).

    python tools/recon_bench.py [--frames 512] [--size 128] [--iters 50] [--rounds 5]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from mebt_amd import recon


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


def torch_quality_f32(a, b, w):
    """the twin's arithmetic as fp32 torch ops on the GPU: (sq_err [N], ssim [N])"""
    d = a.to(torch.int32) - b.to(torch.int32)
    sq = (d * d).sum((1, 2, 3))
    u = a.permute(0, 3, 1, 2).float() - 128.0
    v = b.permute(0, 3, 1, 2).float() - 128.0
    n, c, h, ww = u.shape
    blur = lambda t: F.conv2d(t.reshape(n * c, 1, h, ww), w).reshape(n, c, h - 10, ww - 10)
    mu, mv = blur(u), blur(v)
    var_a, var_b, cov = blur(u * u) - mu * mu, blur(v * v) - mv * mv, blur(u * v) - mu * mv
    ma, mb = mu + 128.0, mv + 128.0
    s = ((2 * ma * mb + recon.C1) * (2 * cov + recon.C2)) / ((ma * ma + mb * mb + recon.C1) * (var_a + var_b + recon.C2))
    return sq, s.mean((1, 2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    N, R = args.frames, args.size
    a = torch.randint(0, 256, (N, R, R, 3), generator=g, dtype=torch.uint8)
    b = (a.float() + 12 * torch.randn(a.shape, generator=g)).round().clamp(0, 255).to(torch.uint8)
    a, b = a.to(dev), b.to(dev)
    gw = torch.from_numpy(recon.ssim_window()).float().to(dev)
    w = (gw[:, None] * gw[None, :])[None, None]

    sq, ssim = recon.clip_quality_u8(a, b)
    sq_t, ssim_t = torch_quality_f32(a, b, w)
    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"clip_quality_u8 on uint8 [{N}, {R}, {R}, 3] x 2; {args.iters} calls per timing after {args.warmup} warm-up calls, {args.rounds} rounds, "
          "kernel and torch baseline alternating")
    print(f"same results: sq_err equal {bool(torch.equal(sq, sq_t.long()))}, max |ssim kernel - torch fp32| {float((ssim - ssim_t.double()).abs().max()):.2e}")
    k_ms, t_ms = [], []
    for _ in range(args.rounds):
        k_ms.append(timed(lambda: recon.clip_quality_u8(a, b), args.iters, args.warmup))
        t_ms.append(timed(lambda: torch_quality_f32(a, b, w), max(1, args.iters // 5), 2))
    nbytes = 2 * a.numel()
    best_k, best_t = min(k_ms), min(t_ms)
    print("HIP kernel (two launches) ms per call:   " + " ".join(f"{x:.4f}" for x in k_ms))
    print("torch fp32 ops on the GPU  ms per call:   " + " ".join(f"{x:.4f}" for x in t_ms))
    print(f"best of rounds: kernel {best_k:.4f} ms, torch {best_t:.4f} ms -> {best_t / best_k:.1f}x; the kernel reads {nbytes / 1e6:.1f} MB "
          f"(both clips once): {nbytes / best_k / 1e6:.1f} GB/s achieved")
    # the other two operators at the matching sizes: 32 clips of [3, 16, 128, 128] floats; 32 * 1024 latent rows of 256, 16384 codes
    x = torch.rand(32, 3 * 16 * R * R, generator=g).to(dev)
    y = torch.rand(32, 3 * 16 * R * R, generator=g).to(dev)
    ms = min(timed(lambda: recon.abs_diff_sum(x, y), args.iters, args.warmup) for _ in range(args.rounds))
    ms_t = min(timed(lambda: (x - y).abs().sum(1, dtype=torch.float64), args.iters, args.warmup) for _ in range(args.rounds))
    print(f"abs_diff_sum on fp32 [32, {x.shape[1]}] x 2: {ms:.4f} ms ({2 * x.numel() * 4 / ms / 1e6:.0f} GB/s); torch (x - y).abs().sum(1) "
          f"in fp64 accumulate: {ms_t:.4f} ms")
    M, d, n_codes = 32 * 1024, 256, 16384
    z, e = torch.randn(M, d, generator=g).to(dev), torch.randn(n_codes, d, generator=g).to(dev)
    ids = torch.randint(0, n_codes, (M,), generator=g).to(dev)
    hist = torch.zeros(n_codes, dtype=torch.int64, device=dev)
    ms = min(timed(lambda: recon.code_stats(ids, z, e, hist=hist), args.iters, args.warmup) for _ in range(args.rounds))
    ms_t = min(timed(lambda: (torch.bincount(ids, minlength=n_codes), ((z - e[ids]) ** 2).sum(dtype=torch.float64)), args.iters, args.warmup)
               for _ in range(args.rounds))
    print(f"code_stats on {M} rows of {d}, {n_codes} codes: {ms:.4f} ms ({2 * M * d * 4 / ms / 1e6:.0f} GB/s); torch bincount + gathered "
          f"squared difference: {ms_t:.4f} ms")


if __name__ == "__main__":
    main()
