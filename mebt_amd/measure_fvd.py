"""`python -m mebt_amd.measure_fvd` — the FVD / KVD stage of the reference's driver scripts (reference measure_fvd_with_numpy.py,
called by scripts/valid_dnr_*.sh after every sampling and revision run) on the HIP I3D.

Flags: the reference script's (`--np_file --score_file --n_sample --n_neighbor --dataset --compute_fvd --train
--sample_fake_n_frames` and the data flags of VideoData), plus `--real_embeddings FILE.npy` (load the real set's [N, 400] logits
if the file exists, else compute and write them), `--i3d_ckpt`, `--i3d_dtype {f16,f32}` and `--i3d_batch`.

Fake side, as the reference: the batch size is forced to 32, batches are cycled until `n_sample` clips are embedded, `--score_file`
keeps the top-`n_sample` videos by score, and when T != sequence_length * sample_fake_n_frames every batch takes a random start and
every `sample_fake_n_frames`-th frame.

Real side, the first that applies:
  1. `--real_embeddings FILE` exists: its logits.
  2. `--image_folder` and `--data_path` is a frame folder (a directory with train.txt under `--train`, else test.txt): the reference's
     route.  `VideoData(args, True)` is walked again and again (every pass a new shuffle and new start frames) in batches of 32; a
     batch counts only if its size is a multiple of 16 (the reference's MAX_BATCH), every batch that counts counts as 32 towards
     `n_sample`, and the result is cut to `n_sample`.  The workers only decode; crop, resize and the reference's
     `((video + 0.5) * 255).byte()` run in the frame-ingest kernel (mebt_amd/frames.py:frames_to_clip_u8) and the clip goes to the
     I3D without visiting the host.  Unlike the reference this warns when fewer than `n_sample` clips result and exits when a
     whole pass yields no batch (the reference loops forever).  With `--packed_path DIR` the same batches are drawn by the same
     rule from the folder's pack (mebt_amd/packed.py) and gathered on the GPU: the same bytes in the same order, nothing decoded.
  3. `--data_path` names a uint8 [N, T, H, W, C] .npy of real clips (the first `sequence_length` frames of the first `n_sample`
     clips).
Output: `<np_file>_consq_set_<n_neighbor>.csv` with pandas' to_csv layout (`,FVD,KVD` / `0,<fvd>,<kvd>`).
"""
import argparse
import csv
import os
import random
import sys

import numpy as np
import torch

from .data import TokenData

REF_MAX_BATCH = 16          # the reference's fvd.MAX_BATCH: its real loop skips a batch whose size is no multiple of it


def build_parser(sliding=False):
    parser = argparse.ArgumentParser(
        description=("sliding-window FVD / KVD of 128-frame samples (reference measure_sliding_fvd_with_numpy.py); the CSV has "
                     "the columns t, fvd, kvd (the reference's empty p, r, d, c columns are not written)") if sliding else
        "FVD / KVD of sampled videos against real clips (reference measure_fvd_with_numpy.py)")
    parser = TokenData.add_data_specific_args(parser)
    parser.add_argument('--np_file', type=str, default='')
    parser.add_argument('--score_file', type=str, default='')
    if sliding:
        parser.add_argument('--slide', type=int, default=8)
    parser.add_argument('--n_sample', type=int, default=512 if sliding else 2048)
    parser.add_argument('--dataset', type=str, default='mshapes', choices=['mshapes', 'ucf101', 'sky', 'taichi', 'stl'])
    return add_scoring_args(parser)


def add_scoring_args(parser):
    """the flags of the scoring itself: the real side, the I3D, the CSV's name (mebt_amd/evaluate.py takes them too)"""
    parser.add_argument('--n_neighbor', type=int, default=5)
    parser.add_argument('--compute_fvd', action='store_true')
    parser.add_argument('--train', action='store_true')
    parser.add_argument('--sample_fake_n_frames', type=int, default=1)
    parser.add_argument('--real_embeddings', type=str, default='',
                        help='.npy of the real set\'s [N, 400] I3D logits: loaded if it exists, else computed and written')
    parser.add_argument('--packed_path', type=str, default='',
                        help='with --image_folder: the pack of --data_path (python -m mebt_amd.pack_frames); the real clips are gathered '
                             'from it instead of decoded')
    parser.add_argument('--i3d_ckpt', type=str, default=None,
                        help='I3D state_dict (default: $MEBT_I3D_CKPT, then mebt/fvd/i3d_pretrained_400.pt)')
    parser.add_argument('--i3d_dtype', type=str, default='f16', choices=['f16', 'f32'])
    parser.add_argument('--i3d_batch', type=int, default=None, help='clips per I3D forward (default: mebt_amd.fvd.MAX_BATCH)')
    return parser


def consq_csv_name(np_file, n_neighbor):
    return np_file.replace('.npy', f'_consq_set_{n_neighbor}.csv')


def sliding_csv_name(np_file, slide, sequence_length, n_neighbor):
    return np_file.replace('.npy', f'_slide{slide}_clip{sequence_length}_{n_neighbor}.csv')


def write_csv(path, columns, rows):
    """pandas DataFrame(...).to_csv(path) layout: an unnamed integer index, float cells as repr(float)"""
    with open(path, 'w', newline='') as f:
        w = csv.writer(f, lineterminator='\n')
        w.writerow([''] + list(columns))
        for i, r in enumerate(rows):
            w.writerow([i] + [repr(float(v)) if isinstance(v, (float, np.floating)) else v for v in r])


def load_fake(args):
    all_data_np = np.load(args.np_file, mmap_mode='r')
    if args.score_file:
        score_np = np.load(args.score_file)
        indices = np.argsort(score_np[:len(all_data_np)])[-args.n_sample:]       # ascending order: the top n_sample
        all_data_np = all_data_np[indices, :]
    return all_data_np


def frame_folder(args):
    """--image_folder with --data_path a directory that holds the list file of the chosen split"""
    return bool(args.image_folder and os.path.isfile(os.path.join(args.data_path, 'train.txt' if args.train else 'test.txt')))


def real_batches(args):
    """the batches of the reference's real loop (measure_fvd_with_numpy.py:55-67) as `frames.RawVideoBatch`es on the host (with
    --packed_path: `packed.PackedVideoBatch`es, the same surface)"""
    from .config import AttrDict
    from .data import VideoData
    if args.sequence_length < 1:
        raise SystemExit(f'--sequence_length {args.sequence_length}: whole-video clips differ in length and do not stack')
    data = VideoData(AttrDict(vars(args)), True, raw=True)
    loader = data.train_dataloader() if args.train else data.val_dataloader()
    used = clips = 0
    while True:
        before = used
        for batch in loader:
            if len(batch['video']) % REF_MAX_BATCH == 0:
                used += 1
                clips += len(batch['video'])
                yield batch['video']
            if used * args.batch_size >= args.n_sample:         # every batch that counts counts as a full one
                if clips < args.n_sample:
                    print(f'warning: the real set holds {clips} clips, fewer than --n_sample {args.n_sample}')
                return
        if used == before:
            raise SystemExit(f'--data_path {args.data_path}: a whole pass over the {"train" if args.train else "test"} list gave no batch '
                             f'of a multiple of {REF_MAX_BATCH} clips (batches of {args.batch_size}); it needs at least '
                             f'{REF_MAX_BATCH} videos')


def real_embeddings(args, i3d, device):
    from .fvd import get_fvd_logits
    if args.real_embeddings and os.path.isfile(args.real_embeddings):
        emb = np.load(args.real_embeddings)
        print(f'loaded real embeddings {emb.shape} from {args.real_embeddings}')
        if len(emb) < args.n_sample:
            raise SystemExit(f'{args.real_embeddings} holds {len(emb)} embeddings, fewer than --n_sample {args.n_sample}')
        return torch.from_numpy(emb[:args.n_sample]).to(device)
    path = args.data_path
    if frame_folder(args):
        print('computing fvd embeddings for real videos')
        emb = [get_fvd_logits(raw.to(device, non_blocking=True).to_clip_u8(), i3d=i3d, device=device, batch=args.i3d_batch)
               for raw in real_batches(args)]
        emb = torch.cat(emb, 0)[:args.n_sample]
    elif path.endswith('.npy') and os.path.isfile(path):
        real = np.load(path, mmap_mode='r')
        if real.dtype != np.uint8 or real.ndim != 5:
            raise SystemExit(f'--data_path {path}: expected uint8 [N, T, H, W, C], got {real.dtype} {real.shape}')
        if real.shape[1] < args.sequence_length:
            raise SystemExit(f'--data_path {path}: clips of {real.shape[1]} frames, shorter than --sequence_length {args.sequence_length}')
        n = min(args.n_sample, len(real))
        print('computing fvd embeddings for real videos')
        emb = get_fvd_logits(real[:n, :args.sequence_length], i3d=i3d, device=device, batch=args.i3d_batch)
    else:
        raise SystemExit(f"--data_path {path!r}: the real side reads --real_embeddings FILE.npy if it exists, else a frame folder "
                         "(--image_folder with a directory holding train.txt under --train, else test.txt), else a uint8 "
                         "[N, T, H, W, C] .npy of real clips")
    if args.real_embeddings:
        np.save(args.real_embeddings, emb.cpu().numpy())
        print(f'wrote real embeddings {tuple(emb.shape)} to {args.real_embeddings}')
    return emb


def fake_embeddings(args, all_data_np, i3d, device, t0=None):
    """the reference's fake loop: batches of args.batch_size (32), cycled until n_sample clips; t0 = the sliding window start.
    `all_data_np`: uint8 [N, T, H, W, C], a numpy array or a torch tensor on the host or the device (mebt_amd/evaluate.py scores the
    clips where the sampler left them)"""
    from .fvd import get_fvd_logits
    n_batch = all_data_np.shape[0] // args.batch_size
    if n_batch == 0:
        raise SystemExit(f'{args.np_file}: {all_data_np.shape[0]} videos, fewer than one batch of {args.batch_size}')
    out, n = [], 0
    while n < args.n_sample:
        for i in range(n_batch):
            sl = slice(i * args.batch_size, (i + 1) * args.batch_size)
            if t0 is not None:
                clip = all_data_np[sl, t0:t0 + args.sequence_length]
            elif all_data_np.shape[1] != args.sequence_length * args.sample_fake_n_frames:
                length = args.sequence_length * args.sample_fake_n_frames
                start_t = random.randint(0, all_data_np.shape[1] - length)
                clip = all_data_np[sl, start_t:start_t + length:args.sample_fake_n_frames]
            else:
                clip = all_data_np[sl]
            clip = clip.contiguous() if torch.is_tensor(clip) else np.ascontiguousarray(clip)
            out.append(get_fvd_logits(clip, i3d=i3d, device=device, batch=args.i3d_batch))
            n += args.batch_size
            if n >= args.n_sample:
                break
    return torch.cat(out, 0)[:args.n_sample]


def load_model(args, device):
    from .fvd import load_fvd_model
    i3d = load_fvd_model(device, path=args.i3d_ckpt, compute_dtype=args.i3d_dtype)
    print(f'I3D compute dtype: {args.i3d_dtype}')
    return i3d


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(args)
    from .fvd import frechet_distance, polynomial_mmd
    args.batch_size = 32
    print('loading numpy file from %s...' % args.np_file)
    all_data_np = load_fake(args)
    device = torch.device('cuda')
    i3d = load_model(args, device)
    real = real_embeddings(args, i3d, device)
    print('computing fvd embeddings for fake videos')
    fake = fake_embeddings(args, all_data_np, i3d, device)
    fvd = frechet_distance(fake, real)
    kvd = polynomial_mmd(fake, real)
    print('FVD = %.2f' % fvd)
    print('KVD = %.2f' % kvd)
    out = consq_csv_name(args.np_file, args.n_neighbor)
    write_csv(out, ['FVD', 'KVD'], [[fvd, kvd]])
    print(f'wrote {out}')
    return fvd, kvd


if __name__ == '__main__':
    main(sys.argv[1:])
