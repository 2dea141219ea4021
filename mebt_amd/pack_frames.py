#!/usr/bin/env python3
"""`python -m mebt_amd.pack_frames` — decode a frame folder once into a pack (mebt_amd/packed.py).

  python -m mebt_amd.pack_frames --data_path FRAMES --out DIR --resolution 128 [--split train test] [--num_workers N]
                                 [--frames_per_launch N]

The images are decoded in DataLoader workers, grouped by source size, and every group goes through the frame-ingest kernel
(center crop + PIL's bilinear resize, identity byte table); the rows land in `DIR/<split>_frames.npy`.  Train or measure from it with
`data.packed_path=DIR` (mebt_amd.train) or `--packed_path DIR` (mebt_amd.measure_fvd, mebt_amd.measure_sliding_fvd).
"""
import argparse
import os
import sys
import time

MAX_WORKERS = 16            # a fixed ceiling: hosts report far more cores than a job may use


def main(argv=None):
    ap = argparse.ArgumentParser(description="pack a frame folder: every frame after crop + resize, uint8 [F, R, R, 3]")
    ap.add_argument("--data_path", required=True, help="the frame folder (holds train.txt / test.txt)")
    ap.add_argument("--out", required=True, help="directory of the pack")
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--split", nargs="+", default=["train", "test"], choices=["train", "test"])
    ap.add_argument("--num_workers", type=int, default=8, help=f"decode workers (at most {MAX_WORKERS})")
    ap.add_argument("--frames_per_launch", type=int, default=256, help="frames of one source size per ingest launch (at most 65535)")
    args = ap.parse_args(argv)
    import torch
    from . import packed
    if not torch.cuda.is_available():
        raise SystemExit("pack_frames resizes on the GPU (the product never resizes on the CPU): no device visible")
    workers = max(0, min(args.num_workers, MAX_WORKERS))
    for split in args.split:
        t0 = time.perf_counter()
        n = packed.build_pack(args.data_path, args.out, args.resolution, splits=[split], resize=packed.gpu_resize, num_workers=workers,
                              frames_per_launch=args.frames_per_launch)[split]
        dt = time.perf_counter() - t0
        nbytes = os.path.getsize(os.path.join(args.out, f"{split}_frames.npy"))
        print(f"{split}: {n} frames, {nbytes} bytes, {n / dt:.1f} frames/s ({workers} workers)", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
