"""`python -m mebt_amd.measure_recon` — how good is a first-stage checkpoint on a data set: the reference's three validation figures
(`VQGAN.validation_step`, mebt/vqgan.py:190-196: recon_loss, commitment_loss, perplexity) plus the reconstruction's PSNR, SSIM and, with
`--compute_fvd`, rFVD / rKVD (FVD / KVD between the real clips and their own reconstructions: the floor under every sample's FVD).

Flags: the data flags of VideoData (as `mebt_amd.measure_fvd` takes them), `--vqgan_ckpt`, `--n_sample` (2048), `--train`,
`--packed_path`, `--vqgan_dtype {f16,f32}`, `--seed`, `--out FILE.csv`, `--save_np FILE.npy` (the reconstructed uint8 clips
[N, T, H, W, 3]), `--compute_fvd` with the I3D flags of measure_fvd (`--i3d_ckpt --i3d_dtype --i3d_batch`), and `--lpips` with
`--lpips_ckpt FILE` (default: the `perceptual_model.*` tensors inside `--vqgan_ckpt`), `--lpips_dtype {f16,f32}` and `--lpips_every K`
(every K-th frame of a clip, default 1): the VGG-16 perceptual distance between the float clips and their reconstructions
(mebt_amd/lpips.py), the mean over all scored frames.  `--disc` adds the thirteen values the reference logs in its GAN phase
(vqgan.py:118-141,156-165: g_image_loss ... discloss, `discriminator.G_KEYS + D_KEYS`), computed per batch from the checkpoint's two
PatchGAN discriminators on the clips and their reconstructions and averaged over the batches: `--disc_dtype {f16,f32}` is the compute
dtype, `--disc_stats {batch,running}` the BatchNorm mode (`batch`, the default: batch statistics with the buffers left untouched, as
the reference logs these values in training mode; `running`: eval mode); one frame per clip is drawn per batch from a generator seeded
by `--seed`, and `global_step` is the checkpoint's (0 when it has none).

Real side: `--image_folder` with `--data_path` a frame folder (train.txt under `--train`, else test.txt) is read through
`VideoData(..., raw=True)`: the workers only decode, crop / resize / normalisation run in the frame-ingest kernel; with
`--packed_path DIR` the folder's pack is gathered on the GPU instead (the same bytes in the same order).  Otherwise `--data_path` names
a uint8 [N, T, H, W, C] .npy of square clips.  One seeded pass over the split in batches of `--batch_size`, cut at `--n_sample` clips; a
split that ends sooner ends the run there and the count is printed.  Every batch gives the float clip for the encoder and the byte
clip for the metrics on the device; the clips, their reconstructions and every sum stay in HBM (mebt_amd/recon.py), one row of scalars
is read back at the end.

Output: one CSV row (pandas' to_csv layout, `measure_fvd.write_csv`) with the columns of `recon.FIELDS` (+ LPIPS) (+ rFVD, rKVD), also
printed.
"""
import argparse
import os
import random
import sys

import numpy as np
import torch

from .data import TokenData
from .measure_fvd import add_scoring_args, frame_folder, write_csv


from .discriminator import D_KEYS, G_KEYS

LPIPS_DTYPE_DEFAULT = 'f16'
DISC_COLUMNS = list(G_KEYS + D_KEYS)


def build_parser():
    parser = argparse.ArgumentParser(description="reconstruction quality of a 3D-VQGAN checkpoint: recon loss, commitment loss, perplexity, "
                                                 "PSNR, SSIM and (--compute_fvd) rFVD / rKVD")
    parser = TokenData.add_data_specific_args(parser)
    parser.add_argument('--vqgan_ckpt', type=str, default='')
    parser.add_argument('--n_sample', type=int, default=2048)
    parser.add_argument('--vqgan_dtype', type=str, default='f16', choices=['f16', 'f32'])
    parser.add_argument('--seed', type=int, default=0, help='seeds the one pass over the split (shuffle and start frames)')
    parser.add_argument('--out', type=str, default='recon.csv', help='the CSV the row is written to')
    parser.add_argument('--save_np', type=str, default='', help='.npy for the reconstructed uint8 clips [N, T, H, W, 3]')
    parser.add_argument('--lpips', action='store_true', help='add the LPIPS column (VGG-16 perceptual distance of the reconstructions)')
    parser.add_argument('--lpips_ckpt', type=str, default='', help="a state dict with the LPIPS tensors; default: those inside --vqgan_ckpt")
    parser.add_argument('--lpips_dtype', type=str, default=LPIPS_DTYPE_DEFAULT, choices=['f16', 'f32'])
    parser.add_argument('--lpips_every', type=int, default=1, help='score every K-th frame of a clip')
    parser.add_argument('--disc', action='store_true', help="add the thirteen GAN-phase values of the checkpoint's discriminators")
    parser.add_argument('--disc_dtype', type=str, default='f16', choices=['f16', 'f32'])
    parser.add_argument('--disc_stats', type=str, default='batch', choices=['batch', 'running'],
                        help='BatchNorm statistics: of the batch (buffers untouched) or the running buffers (eval mode)')
    return add_scoring_args(parser)              # --train --packed_path --compute_fvd --i3d_ckpt --i3d_dtype --i3d_batch


def seed_everything(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


class DiscTerms:
    """The function behind --disc: the thirteen GAN-phase values per batch from a checkpoint's discriminators (discriminator.gan_terms,
    generator and discriminator side), kept on the device; `result()` reads the means over the batches back once."""

    def __init__(self, ckpt, device, dtype='f16', stats='batch', seed=0):
        from . import discriminator as D
        from .lightning_shim import load_checkpoint_file
        try:
            nets = D.load_discriminators(ckpt, device, dtype)
        except ValueError as e:
            raise SystemExit(f'--disc: {e}')
        ck = load_checkpoint_file(ckpt, map_location='cpu')
        hp = ck.get('hyper_parameters', {}) if isinstance(ck.get('hyper_parameters', {}), dict) else {}
        self.hp = hp.get('args', hp)
        self.global_step = int(ck.get('global_step', 0) or 0)
        for net in nets:
            net.train(stats == 'batch')
        self.runners = tuple(D.DiscRunner(net, dtype) for net in nets)
        self.gen = torch.Generator().manual_seed(int(seed))
        self.frame_idx, self.rows = [], []

    @torch.no_grad()
    def add(self, x, x_recon):
        """x, x_recon fp32 [B, 3, T, H, W] on the GPU: draws this batch's frames and appends its thirteen values (fp64 [13], device)"""
        from .discriminator import gan_terms
        fidx = torch.randint(0, x.shape[2], [x.shape[0]], generator=self.gen)
        self.frame_idx.append(fidx)
        x, x_recon = x.to(torch.float32).contiguous(), x_recon.to(torch.float32).contiguous()
        vals = {}
        for which in ('generator', 'discriminator'):
            vals.update(gan_terms(self.hp, self.runners[0], self.runners[1], x, x_recon, fidx, self.global_step, which, update_running=False))
        self.rows.append(torch.stack([vals[k] for k in DISC_COLUMNS]))
        return self.rows[-1]

    def result(self):
        mean = torch.stack(self.rows).mean(0).cpu().tolist()
        return dict(zip(DISC_COLUMNS, mean))


def real_batches(args, device):
    """(float clip [B, 3, T, R, R], byte clip [B, T, R, R, 3]) pairs on the device, one pass over the split"""
    if frame_folder(args):
        from .config import AttrDict
        from .data import VideoData
        if args.sequence_length < 1:
            raise SystemExit(f'--sequence_length {args.sequence_length}: whole-video clips differ in length and do not stack')
        data = VideoData(AttrDict(vars(args)), True, raw=True)
        for batch in (data.train_dataloader() if args.train else data.val_dataloader()):
            raw = batch['video'].to(device, non_blocking=True)
            yield raw.to_video(), raw.to_clip_u8()
        return
    path = args.data_path
    if not (path.endswith('.npy') and os.path.isfile(path)):
        raise SystemExit(f"--data_path {path!r}: expected a frame folder (--image_folder with a directory holding train.txt under --train, "
                         "else test.txt) or a uint8 [N, T, H, W, C] .npy of real clips")
    from .packed import pack_to_clip_u8, pack_to_video
    real = np.load(path, mmap_mode='r')
    if real.dtype != np.uint8 or real.ndim != 5 or real.shape[-1] != 3 or real.shape[2] != real.shape[3]:
        raise SystemExit(f'--data_path {path}: expected uint8 [N, T, R, R, 3], got {real.dtype} {real.shape}')
    T, R = args.sequence_length, int(real.shape[2])
    if real.shape[1] < T:
        raise SystemExit(f'--data_path {path}: clips of {real.shape[1]} frames, shorter than --sequence_length {T}')
    order = torch.randperm(len(real)).tolist()
    for i in range(0, len(order), args.batch_size):
        rows = sorted(order[i:i + args.batch_size])
        u8 = torch.from_numpy(np.ascontiguousarray(real[rows, :T])).to(device)
        ids = torch.arange(len(rows) * T, device=device).view(len(rows), T)
        pack = u8.view(-1, R, R, 3)
        yield pack_to_video(pack, ids, R), pack_to_clip_u8(pack, ids, R)


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(args if args.disc else argparse.Namespace(**{k: v for k, v in vars(args).items() if not k.startswith('disc')}))
    from . import recon
    from .vqgan import load_vqgan
    device = torch.device('cuda')
    vqgan = load_vqgan(args.vqgan_ckpt, device)
    vqgan.compute_dtype = args.vqgan_dtype
    print(f'VQGAN compute dtype: {args.vqgan_dtype}')
    if args.lpips:
        if args.lpips_every < 1:
            raise SystemExit(f'--lpips_every {args.lpips_every}: expected a positive integer')
        if args.lpips_ckpt:
            from .lpips import read_file
            try:
                vqgan.lpips_weights = read_file(args.lpips_ckpt)
            except (ValueError, OSError) as e:
                raise SystemExit(f'--lpips_ckpt {args.lpips_ckpt}: {e}')
        if vqgan.lpips_weights is None:
            raise SystemExit(f'--lpips: {args.vqgan_ckpt} holds no perceptual_model.* tensors; name a state dict that has the 13 VGG-16 '
                             'convolutions and the five lin layers with --lpips_ckpt')
        vqgan.lpips_dtype = args.lpips_dtype
        print(f'LPIPS compute dtype: {args.lpips_dtype}, every {args.lpips_every} frame(s)')
    i3d = None
    if args.compute_fvd:
        from .fvd import frechet_distance, get_fvd_logits, polynomial_mmd
        from .measure_fvd import load_model
        i3d = load_model(args, device)
    disc = DiscTerms(args.vqgan_ckpt, device, args.disc_dtype, args.disc_stats, args.seed) if args.disc else None
    if disc is not None:
        print(f'discriminators: compute dtype {args.disc_dtype}, {args.disc_stats} statistics, global_step {disc.global_step}')
    seed_everything(args.seed)
    acc = recon.ReconAccumulator(vqgan.n_codes, l1_weight=vqgan._hp("l1_weight", 4.0), device=device)
    saved, emb_real, emb_fake = [], [], []
    for x, u8 in real_batches(args, device):
        left = args.n_sample - acc.n_clips
        if len(x) > left:
            x, u8 = x[:left].contiguous(), u8[:left].contiguous()
        st = vqgan.reconstruct_stats(x, clip_u8=u8, lpips_every=args.lpips_every if args.lpips else 0)
        acc.add(st)
        if disc is not None:
            disc.add(x, st["recon"])
        if args.save_np:
            saved.append(st["recon_u8"])
        if i3d is not None:
            emb_real.append(get_fvd_logits(u8, i3d=i3d, device=device, batch=args.i3d_batch))
            emb_fake.append(get_fvd_logits(st["recon_u8"], i3d=i3d, device=device, batch=args.i3d_batch))
        if acc.n_clips >= args.n_sample:
            break
    if acc.n_clips == 0:
        raise SystemExit(f'--data_path {args.data_path}: the {"train" if args.train else "test"} split gave no clip')
    if acc.n_clips < args.n_sample:
        print(f'the split ended after {acc.n_clips} clips, fewer than --n_sample {args.n_sample}')
    row = acc.result()
    columns = list(recon.FIELDS) + (["LPIPS"] if args.lpips else [])
    if disc is not None:
        row.update(disc.result())
        columns += DISC_COLUMNS
    if i3d is not None:
        real, fake = torch.cat(emb_real, 0), torch.cat(emb_fake, 0)
        row["rFVD"], row["rKVD"] = float(frechet_distance(fake, real)), float(polynomial_mmd(fake, real))
        columns += ["rFVD", "rKVD"]
    if args.save_np:
        np.save(args.save_np, torch.cat(saved, 0).cpu().numpy())
        print(f'wrote {acc.n_clips} reconstructed clips to {args.save_np}')
    write_csv(args.out, columns, [[row[c] for c in columns]])
    print(','.join(columns))
    print(','.join(repr(row[c]) for c in columns))
    print(f'wrote {args.out}')
    return row


if __name__ == '__main__':
    main(sys.argv[1:])
