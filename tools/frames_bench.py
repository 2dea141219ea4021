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

  gather   the packed-dataset gather (csrc/frames/frames.hip: pack_gather_kernel) of 96 frames at R 128 with contiguous ids, float and
           uint8 output, against the copy kernel (the 128 -> 128 `ingest` case) on the same 96 frames laid out contiguously: the two
           alternate round by round, each round event-timed over `--reps` launches; medians, the copy kernel's own run-to-run
           spread, effective GB/s.  The 4.7 MB input stays in the Infinity Cache: these are not HBM figures.
  pack_build / packed_loader   `packed.build_pack` (8 decode workers + the ingest kernel) on the loader leg's PNG folder, then the
           packed loader in host and in resident mode on that pack: frames per second of the batches alone (comparable with
           `loader`) and with the move to the device, the gather and a synchronise per batch
  step     with the pack at hand also `packed`: next(loader) + move + step from the resident pack, in the same rotation as the pixel
           and token steps; `packed_minus_pixel_ms` is the median of the paired differences, next to the pairs' spread

  video_u8 the decoded-video -> uint8-clip kernel (csrc/frames/frames.hip: video_to_clip_kernel) on [16, 3, 16, 128, 128] and
           [4, 3, 128, 128, 128] fp32, event-timed over `--reps` launches, against the host route it replaces on the same tensor
           (`.cpu().numpy()`, `* 255`, `astype(uint8)`, transpose to [B, T, H, W, 3], wall clock around a synchronise); the two
           alternate round by round and their bytes are compared once.  GB/s = fp32 bytes read + uint8 bytes written over the
           kernel time; the host route's figure is its wall time only
  evaluate_stage  one draft stage of `python -m mebt_amd.evaluate` against the two processes it replaces (`mebt_amd.sample`, then
           `mebt_amd.measure_fvd` on its .npy) on a micro model (6 layers, 64 wide, 64 tokens, 16 frames of 32 x 32, 64 clips, the real
           side read from a file of embeddings): wall seconds per route, alternating.  At this size process start, torch's import
           and the three model loads are nearly all of it: it measures those fixed costs, not a sweep at the shipped geometry

The transformer and the VQGAN have random weights (time does not depend on them); the PNGs are smooth random images.

Usage:  python tools/frames_bench.py [--steps 10] [--warmup 3] [--reps 50] [--workers 8 16] [--no-step] [--no-loader] [--no-packed]
        python tools/frames_bench.py --only-video-u8 [--no-evaluate]
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


def clocks():
    """the device's current clocks as rocm-smi shows them (read only), for the record"""
    import subprocess
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        return [" ".join(ln.split()) for ln in out.splitlines() if "sclk" in ln or "mclk" in ln or "fclk" in ln]
    except Exception as e:                                           # noqa: BLE001
        return [f"not read: {e}"]


def bench_gather(reps, rounds=9, B=6, T=16, R=128):
    """B x T frames; B 6 is the training batch, where a launch is shorter than the host takes to issue the next (see
    `host_us_per_launch`: event time per launch then equals the launch rate), B 96 makes both kernels run longer than that"""
    from mebt_amd import packed as P
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.randint(0, 256, (B, T, R, R, 3)).astype(np.uint8)).to(DEV)
    pack = x.view(B * T, R, R, 3)
    ids = torch.arange(B * T, device=DEV).view(B, T)
    out = []
    for u8 in (False, True):
        copy_out = (F.frames_to_clip_u8 if u8 else F.frames_to_video)(x, R)
        assert torch.equal(copy_out, (P.pack_to_clip_u8 if u8 else P.pack_to_video)(pack, ids, R))

        def copy():
            (F.frames_to_clip_u8 if u8 else F.frames_to_video)(x, R, out=copy_out)

        gather_out = torch.empty_like(copy_out)

        def gather():
            (P.pack_to_clip_u8 if u8 else P.pack_to_video)(pack, ids, R, out=gather_out)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / reps * 1e3

        def host(fn):                                                # host time to issue one launch, queue never full
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                fn()
            dt = (time.perf_counter() - t0) / 20 * 1e6
            torch.cuda.synchronize()
            return dt

        for _ in range(3):
            timed(copy), timed(gather)
        tc, tg = [], []
        for r in range(rounds):                                      # alternate which kernel goes first
            if r % 2 == 0:
                tc.append(timed(copy)); tg.append(timed(gather))
            else:
                tg.append(timed(gather)); tc.append(timed(copy))
        nbytes = x.numel() + copy_out.numel() * copy_out.element_size()
        mc, mg = statistics.median(tc), statistics.median(tg)
        out.append({"bench": "gather_u8" if u8 else "gather", "frames": B * T, "R": R, "reps": reps, "rounds": rounds,
                    "copy_us_median": round(mc, 2), "gather_us_median": round(mg, 2),
                    "copy_us_min_max": [round(min(tc), 2), round(max(tc), 2)], "gather_us_min_max": [round(min(tg), 2), round(max(tg), 2)],
                    "gather_minus_copy_us_paired_median": round(statistics.median([g - c for g, c in zip(tg, tc)]), 2),
                    "copy_spread_us": round(max(tc) - min(tc), 2), "MB_moved": round(nbytes / 1e6, 2),
                    "host_us_per_launch": {"copy": round(host(copy), 2), "gather": round(host(gather), 2)},
                    "copy_GBps": round(nbytes / (mc * 1e-6) / 1e9, 1), "gather_GBps": round(nbytes / (mg * 1e-6) / 1e9, 1),
                    "note": "back-to-back launches into a preallocated output, each wrapper's host path included; the input stays in the Infinity Cache"})
    return out


def bench_video_u8(B, Td, H, W, reps, rounds=5):
    """the kernel and the host route on the same decoded tensor; the host route starts from the float `samples` the drivers log"""
    g = torch.Generator(device=DEV).manual_seed(0)
    x = (torch.rand(B, 3, Td, H, W, device=DEV, generator=g) - 0.5) * 1.3
    samples = torch.clamp(x, -0.5, 0.5) + 0.5
    out = F.video_to_clip_u8(x)

    def kernel():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            F.video_to_clip_u8(x, out=out)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3                      # us per launch

    def host():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = samples.cpu().numpy()
        d = np.ascontiguousarray(np.transpose((d * 255).astype(np.uint8), (0, 2, 3, 4, 1)))
        return (time.perf_counter() - t0) * 1e3, d                   # ms

    assert np.array_equal(host()[1], out.cpu().numpy())              # the same bytes
    kernel()
    tk, th = [], []
    for r in range(rounds):
        if r % 2 == 0:
            tk.append(kernel()); th.append(host()[0])
        else:
            th.append(host()[0]); tk.append(kernel())
    nbytes = x.numel() * 4 + out.numel()
    mk, mh = statistics.median(tk), statistics.median(th)
    return {"bench": "video_u8", "shape": [B, 3, Td, H, W], "reps": reps, "rounds": rounds, "kernel_us_median": round(mk, 2),
            "kernel_us_min_max": [round(min(tk), 2), round(max(tk), 2)], "MB_moved": round(nbytes / 1e6, 2),
            "kernel_GBps": round(nbytes / (mk * 1e-6) / 1e9, 1), "host_route_ms_median": round(mh, 2),
            "host_route_ms_min_max": [round(min(th), 2), round(max(th), 2)], "host_over_kernel": round(mh * 1e3 / mk, 1),
            "float32_MB_over_pcie": round(x.numel() * 4 / 1e6, 2), "uint8_MB_kept": round(out.numel() / 1e6, 2)}


def bench_evaluate_stage(rounds=2):
    """wall time of one draft stage: `evaluate --stages draft --runs 0` against `sample` + `measure_fvd`, fresh processes each"""
    import subprocess
    from mebt_amd import presets
    from mebt_amd.config import AttrDict
    from mebt_amd.i3d import InceptionI3d
    from mebt_amd.vqgan import VQGAN
    root = tempfile.mkdtemp(prefix="evaluate_bench_")
    try:
        torch.manual_seed(0)
        vq_args = presets.vqgan_args(n_hiddens=16, embedding_dim=64, n_codes=512, sequence_length=16, resolution=32)
        torch.save({"state_dict": VQGAN(vq_args).state_dict(), "hyper_parameters": {"args": vq_args}}, os.path.join(root, "vq.ckpt"))
        cfg = presets.tiny(vtokens=False)
        p, m = cfg.model.params, cfg.model.mask.params
        p.block_size, p.n_layer, p.n_head, p.n_embd, p.sos_emb, p.vocab_size, p.first_stage_vocab_size = 64, 6, 2, 64, 8, 512, 512
        p.mode = ["latent_enc", "latent_self", "latent_enc", "latent_dec", "lt2l", "latent_dec"]
        m.max_token, m.shape, m.budget = 64, [4, 4, 4], 64
        cfg.model.vqvae = AttrDict(params=AttrDict(ckpt_path=os.path.join(root, "vq.ckpt")))
        model = presets.build_model(cfg, compute_dtype="bf16")
        torch.save({"state_dict": {k: v for k, v in model.state_dict().items() if not k.startswith("first_stage_model.")},
                    "hyper_parameters": model.hparams, "global_step": 0, "epoch": 0}, os.path.join(root, "gpt.ckpt"))
        torch.save(InceptionI3d(400, in_channels=3).state_dict(), os.path.join(root, "i3d.pt"))
        np.save(os.path.join(root, "real_emb.npy"), np.random.RandomState(0).randn(64, 400).astype(np.float32))
        sampling = ("--gpt_ckpt gpt.ckpt --batch_size 16 --n_sample 64 --total_length 16 --step_size 16 --context_size 16 --vid_n_steps 8 "
                    "--vid_c_temp 2.0 --no_phase --dataset stl --resolution 32 --save_codemap").split()
        scoring = "--n_sample 64 --sequence_length 16 --i3d_ckpt i3d.pt --real_embeddings real_emb.npy".split()
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

        def py(*argv):
            r = subprocess.run([sys.executable, "-m", *argv], cwd=root, env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"{argv[0]} failed:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")

        def one():
            t0 = time.perf_counter()
            py("mebt_amd.evaluate", *sampling, *scoring, "--exp_name", "one", "--runs", "0", "--stages", "draft")
            return time.perf_counter() - t0

        def two():
            t0 = time.perf_counter()
            py("mebt_amd.sample", *sampling, "--exp_name", "two")
            t1 = time.perf_counter()
            py("mebt_amd.measure_fvd", *scoring, "--np_file",
               "results/two/numpy_files_16/stl/VID_n_steps8_temp1.0_ctemp2.0linear_maskgit_cosine_no_phase_run0.npy")
            return time.perf_counter() - t0, t1 - t0

        one(), two()                                                  # warm the file cache and the code object cache
        t_one, t_two, t_sample = [], [], []
        for r in range(rounds):
            if r % 2 == 0:
                t_one.append(one()); a, b = two()
            else:
                a, b = two(); t_one.append(one())
            t_two.append(a); t_sample.append(b)
        return {"bench": "evaluate_stage", "model": "micro 6L d64 block 64, 16 x 32 x 32, 64 clips, batch 16, 8 steps", "rounds": rounds,
                "evaluate_s": [round(v, 2) for v in t_one], "two_process_s": [round(v, 2) for v in t_two],
                "of_which_sample_s": [round(v, 2) for v in t_sample],
                "note": "fresh processes; at this size start-up, imports and model loads dominate both routes"}
    finally:
        shutil.rmtree(root)


def smooth_frames(rs, n, H, W):
    """random low-frequency RGB frames (PNG-compressible like natural images, unlike uniform noise)"""
    small = rs.randint(0, 256, (n, H // 8 + 1, W // 8 + 1, 3)).astype(np.float32)
    big = small.repeat(8, 1).repeat(8, 2)[:, :H, :W]
    return np.clip(big + rs.randint(-6, 7, big.shape), 0, 255).astype(np.uint8)


def bench_step(steps, warmup, packed_loader=None):
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

    pk_it = [iter(packed_loader)] if packed_loader is not None else None

    def run(kind):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "packed":                # the loop a run from a resident pack executes: draw + collate, ids to the device, step
            try:
                pb = next(pk_it[0])
            except StopIteration:
                pk_it[0] = iter(packed_loader)
                pb = next(pk_it[0])
            loop.step(pb["video"].to(DEV, non_blocking=True), pb["indices"].to(DEV, non_blocking=True))
        else:
            x = batch.to(DEV, non_blocking=True) if kind == "pixel" else ids
            loop.step(x, idx)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    kinds = ["pixel", "token"] + (["packed"] if packed_loader is not None else [])
    for _ in range(warmup):
        for k in kinds:
            run(k)
    times = {k: [] for k in kinds}
    for i in range(steps):                  # rotate which path goes first in each round
        for k in kinds[i % len(kinds):] + kinds[:i % len(kinds)]:
            times[k].append(run(k))
    px, tk = times["pixel"], times["token"]
    packed = {}
    if packed_loader is not None:
        diff = sorted(a - b for a, b in zip(times["packed"], px))
        packed = {"packed_ms_median": round(statistics.median(times["packed"]), 3), "packed_ms": [round(v, 3) for v in times["packed"]],
                  "packed_minus_pixel_ms": round(statistics.median(diff), 3), "packed_minus_pixel_ms_min_max": [round(diff[0], 3), round(diff[-1], 3)],
                  "pixel_ms_min_max": [round(min(px), 3), round(max(px), 3)]}
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
            "h2d_MB": round(raw.numel() / 1e6, 2), "pixel_frames_per_s": round(B * T / (statistics.median(px) * 1e-3), 1), **packed}


def write_folder(root, videos=24, frames=40):
    """the loader legs' synthetic frame folder: `videos` videos of `frames` 240x320 PNGs, listed in train.txt"""
    from PIL import Image
    rs = np.random.RandomState(2)
    paths = []
    for v in range(videos):
        for k, f in enumerate(smooth_frames(rs, frames, 240, 320)):
            p = os.path.join(root, f"v{v:03d}_{k + 1:04d}.png")        # zero-padded: the list is sorted as strings
            Image.fromarray(f).save(p, compress_level=1)
            paths.append(p)
    paths.append(os.path.join(root, "zz_1.png"))                     # the last video of a list is never flushed
    Image.fromarray(f).save(paths[-1])
    with open(os.path.join(root, "train.txt"), "w") as fh:
        fh.write("\n".join(paths) + "\n")
    return paths


def loader_args(root, workers, **more):
    from mebt_amd.config import AttrDict
    return AttrDict(data_path=root, image_folder=True, sequence_length=16, resolution=128, latent_shape=[4, 16, 16], batch_size=6,
                    num_workers=workers, **more)


def bench_loader(root, workers, batches=12):
    from mebt_amd.data import VideoData
    loader = VideoData(loader_args(root, workers), raw=True).train_dataloader()
    n, t0, it = 0, None, iter(loader)
    for b in range(batches + 2):
        try:
            batch = next(it)
        except StopIteration:
            it = iter(loader)
            batch = next(it)
        if b == 1:                                                   # after the workers' start-up
            t0 = time.perf_counter()
        elif b > 1:
            n += sum(int(f.shape[0] * f.shape[1]) for f, _ in batch["video"].groups)
    dt = time.perf_counter() - t0
    first = os.path.join(root, "v000_0001.png")
    return {"bench": "loader", "workers": workers, "src": [240, 320], "png_bytes_per_frame": os.path.getsize(first),
            "frames_per_s": round(n / dt, 1), "batches_per_s": round(batches / dt, 2), "frames_per_batch": 96}


def bench_pack_build(root, pack_dir, workers=8):
    from mebt_amd import packed as P
    t0 = time.perf_counter()
    n = P.build_pack(root, pack_dir, 128, splits=["train"], resize=P.gpu_resize, num_workers=workers)["train"]
    dt = time.perf_counter() - t0
    return {"bench": "pack_build", "workers": workers, "frames": n, "src": [240, 320], "R": 128, "seconds": round(dt, 2),
            "frames_per_s": round(n / dt, 1), "pack_bytes": os.path.getsize(os.path.join(pack_dir, "train_frames.npy"))}


def packed_loader(root, pack_dir, resident):
    from mebt_amd.data import VideoData
    return VideoData(loader_args(root, 0, packed_path=pack_dir, packed_resident=resident), raw=True).train_dataloader()


def bench_packed_loader(root, pack_dir, resident, batches=200):
    loader = packed_loader(root, pack_dir, resident)

    def walk(device):
        n, it = 0, iter(loader)
        next(it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(batches):
            try:
                batch = next(it)
            except StopIteration:
                it = iter(loader)
                batch = next(it)
            if device:
                batch["video"].to(DEV, non_blocking=True).to_video()
                torch.cuda.synchronize()
            n += batch["video"].shape[0] * batch["video"].shape[2]
        return n / (time.perf_counter() - t0)

    walk(True)
    host = [walk(False) for _ in range(3)]
    dev = [walk(True) for _ in range(3)]
    return {"bench": "packed_loader", "mode": "resident" if resident else "host", "batches": batches, "frames_per_batch": 96,
            "frames_per_s": round(statistics.median(host), 1), "clips_per_s": round(statistics.median(host) / 16, 1),
            "frames_per_s_to_device": round(statistics.median(dev), 1), "frames_per_s_to_device_min_max": [round(min(dev), 1), round(max(dev), 1)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--workers", type=int, nargs="+", default=[8])
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-loader", action="store_true")
    ap.add_argument("--no-packed", action="store_true")
    ap.add_argument("--only-video-u8", action="store_true", help="the video_u8 and evaluate_stage legs alone")
    ap.add_argument("--no-evaluate", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frames_bench measures on the GPU: no device visible")
    print(json.dumps({"bench": "clocks", "when": "start", "rocm_smi": clocks()}), flush=True)
    for shape in ((16, 16, 128, 128), (4, 128, 128, 128)):
        print(json.dumps(bench_video_u8(*shape, args.reps)), flush=True)
    if not args.no_evaluate:
        print(json.dumps(bench_evaluate_stage()), flush=True)
    if args.only_video_u8:
        print(json.dumps({"bench": "clocks", "when": "end", "rocm_smi": clocks()}), flush=True)
        return
    for shape in ((6, 16, 128, 128, 128), (6, 16, 240, 320, 128)):
        for u8 in (False, True):
            print(json.dumps(bench_ingest(*shape, args.reps, u8=u8)), flush=True)
    if not args.no_packed:
        for B in (6, 96):                                              # 96 frames (the step's batch), then 1536: kernel-bound
            for row in bench_gather(args.reps if B == 6 else max(10, args.reps // 4), B=B):
                print(json.dumps(row), flush=True)
    root = tempfile.mkdtemp(prefix="frames_bench_")
    try:
        pack_dir = None
        if not (args.no_loader and args.no_packed):
            write_folder(root)
        if not args.no_packed:
            pack_dir = os.path.join(root, "pack")
            print(json.dumps(bench_pack_build(root, pack_dir)), flush=True)
            for resident in (False, True):
                print(json.dumps(bench_packed_loader(root, pack_dir, resident)), flush=True)
        if not args.no_step:
            print(json.dumps(bench_step(args.steps, args.warmup, packed_loader(root, pack_dir, True) if pack_dir else None)), flush=True)
        if not args.no_loader:
            for w in args.workers:
                print(json.dumps(bench_loader(root, w)), flush=True)
    finally:
        shutil.rmtree(root)
    print(json.dumps({"bench": "clocks", "when": "end", "rocm_smi": clocks()}), flush=True)


if __name__ == "__main__":
    main()
