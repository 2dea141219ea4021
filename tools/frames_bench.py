#!/usr/bin/env python3
"""Frame-folder training costs on one GPU, one JSON line per measurement:

  ingest   the frame-ingest kernel (csrc/frames/frames.hip) on B x T uint8 frames -> [B, 3, T, R, R] fp32: median / min time per
           launch from HIP events around `--reps` back-to-back launches, and the effective GB/s (uint8 bytes read once +
           fp32 bytes written, over the kernel time), for 128x128 -> 128 and 240x320 -> 128 (UCF frames)
  ingest_u8  the same launches with the uint8 output of the FVD real side, [B, T, R, R, 3] (a quarter of the bytes written), timed
           right after the float output of the same shape
  step     ms per training step at the Sky-16f geometry (B 6, 16 x 128 x 128 pixels -> 4 x 16 x 16 tokens, bf16): the pixel
           path (raw uint8 240x320 frames -> ingest -> VQGAN.encode -> token step) against the token step on the ids of the
           same clips, one model, the two paths alternating step by step; medians of `--steps` pairs after `--warmup`
  loader   FrameListDataset(raw=True) + collate_raw through a DataLoader with `--workers` workers on PNG frames written to a
           temporary directory: decoded frames per second, next to the frames per second one step of each path consumes

The transformer and the VQGAN have random weights (time does not depend on them); the PNGs are smooth random images.

Usage:  python tools/frames_bench.py [--steps 10] [--warmup 3] [--reps 50] [--workers 8] [--no-step] [--no-loader]
"""
import argparse
import json
import os
import random
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from mebt_amd import frames as F

DEV = "cuda"


def bench_ingest(B, T, H, W, R, reps, u8=False):
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.randint(0, 256, (B, T, H, W, 3)).astype(np.uint8)).to(DEV)
    ingest = F.frames_to_clip_u8 if u8 else F.frames_to_video
    out = ingest(x, R)
    for _ in range(5):
        ingest(x, R, out=out)
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ingest(x, R, out=out)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / reps * 1e3)
    nbytes = x.numel() + out.numel() * out.element_size()
    med = statistics.median(times)
    return {"bench": "ingest_u8" if u8 else "ingest", "frames": B * T, "src": [H, W], "R": R, "us_median": round(med, 2), "us_min": round(min(times), 2),
            "MB_moved": round(nbytes / 1e6, 2), "GBps": round(nbytes / (med * 1e-6) / 1e9, 1)}


def smooth_frames(rs, n, H, W):
    """random low-frequency RGB frames (PNG-compressible like natural images, unlike uniform noise)"""
    small = rs.randint(0, 256, (n, H // 8 + 1, W // 8 + 1, 3)).astype(np.float32)
    big = small.repeat(8, 1).repeat(8, 2)[:, :H, :W]
    return np.clip(big + rs.randint(-6, 7, big.shape), 0, 255).astype(np.uint8)


def bench_step(steps, warmup):
    from mebt_amd import presets
    from mebt_amd.trainer import TrainLoop
    from mebt_amd.vqgan import VQGAN
    B, T, H, W, R = 6, 16, 240, 320, 128
    torch.manual_seed(0)
    vq = VQGAN(presets.vqgan_args()).to(DEV).eval()
    cfg = presets.sky_16f(vtokens=False)
    model = presets.build_model(cfg, compute_dtype="bf16")
    model.first_stage_model = vq
    model = model.to(DEV).train()
    loop = TrainLoop(model, max_steps=10 ** 6)
    rs = np.random.RandomState(1)
    raw = torch.from_numpy(smooth_frames(rs, B * T, H, W).reshape(B, T, H, W, 3)).pin_memory()
    batch = F.RawVideoBatch([(raw, torch.arange(B, dtype=torch.int32).pin_memory())], B, R)
    idx = torch.stack([torch.randperm(4 * 16 * 16) for _ in range(B)]).to(DEV)
    ids = vq.encode(batch.to(DEV).to_video())
    random.seed(0)

    def run(kind):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = batch.to(DEV, non_blocking=True) if kind == "pixel" else ids
        loop.step(x, idx)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(warmup):
        run("pixel"), run("token")
    px, tk = [], []
    for i in range(steps):                  # alternate which path goes first in each pair
        if i % 2 == 0:
            px.append(run("pixel")); tk.append(run("token"))
        else:
            tk.append(run("token")); px.append(run("pixel"))
    # the pieces the pixel path adds, timed alone with events
    xd = batch.to(DEV)
    video = xd.to_video()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    enc = []
    for _ in range(5):
        e[0].record(); vq.encode(video); e[1].record(); e[1].synchronize()
        enc.append(e[0].elapsed_time(e[1]))
    h2d = []
    for _ in range(5):
        torch.cuda.synchronize()
        e[0].record(); batch.to(DEV, non_blocking=True); e[1].record(); e[1].synchronize()
        h2d.append(e[0].elapsed_time(e[1]))
    return {"bench": "step", "geometry": "sky_16f B6 16x128x128 bf16, frames 240x320", "pixel_ms_median": round(statistics.median(px), 3),
            "token_ms_median": round(statistics.median(tk), 3),
            "pixel_minus_token_ms": round(statistics.median([a - b for a, b in zip(px, tk)]), 3),
            "pixel_ms": [round(v, 3) for v in px], "token_ms": [round(v, 3) for v in tk],
            "vqgan_encode_ms_median": round(statistics.median(enc), 3), "h2d_uint8_ms_median": round(statistics.median(h2d), 3),
            "h2d_MB": round(raw.numel() / 1e6, 2)}


def bench_loader(workers, videos=24, frames=40, batches=12):
    from PIL import Image
    from mebt_amd.data import VideoData
    from mebt_amd.config import AttrDict
    root = tempfile.mkdtemp(prefix="frames_bench_")
    try:
        rs = np.random.RandomState(2)
        paths = []
        for v in range(videos):
            for k, f in enumerate(smooth_frames(rs, frames, 240, 320)):
                p = os.path.join(root, f"v{v:03d}_{k + 1:04d}.png")    # zero-padded: the list is sorted as strings
                Image.fromarray(f).save(p, compress_level=1)
                paths.append(p)
        paths.append(os.path.join(root, "zz_1.png"))                 # the last video of a list is never flushed
        Image.fromarray(f).save(paths[-1])
        with open(os.path.join(root, "train.txt"), "w") as fh:
            fh.write("\n".join(paths) + "\n")
        a = AttrDict(data_path=root, image_folder=True, sequence_length=16, resolution=128, latent_shape=[4, 16, 16], batch_size=6,
                     num_workers=workers)
        loader = VideoData(a, raw=True).train_dataloader()
        n, t0, it = 0, None, iter(loader)
        for b in range(batches + 2):
            try:
                batch = next(it)
            except StopIteration:
                it = iter(loader)
                batch = next(it)
            if b == 1:                                               # after the workers' start-up
                t0 = time.perf_counter()
            elif b > 1:
                n += sum(int(f.shape[0] * f.shape[1]) for f, _ in batch["video"].groups)
        dt = time.perf_counter() - t0
        return {"bench": "loader", "workers": workers, "src": [240, 320], "png_bytes_per_frame": os.path.getsize(paths[0]),
                "frames_per_s": round(n / dt, 1), "batches_per_s": round(batches / dt, 2), "frames_per_batch": 96}
    finally:
        shutil.rmtree(root)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-loader", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frames_bench measures on the GPU: no device visible")
    for shape in ((6, 16, 128, 128, 128), (6, 16, 240, 320, 128)):
        for u8 in (False, True):
            print(json.dumps(bench_ingest(*shape, args.reps, u8=u8)), flush=True)
    if not args.no_step:
        print(json.dumps(bench_step(args.steps, args.warmup)), flush=True)
    if not args.no_loader:
        print(json.dumps(bench_loader(args.workers)), flush=True)


if __name__ == "__main__":
    main()
