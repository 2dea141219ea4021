"""`python -m mebt_amd.train_vqgan` — the reconstruction phase of first-stage training: what the reference's `train_vqgan.py` computes
during its first `--discriminator_iter_start` steps (default 50 000), when both GAN terms are multiplied by a zero `disc_factor`: the L1
reconstruction loss, the commitment loss, with `--perceptual_weight` above 0 the LPIPS term on one drawn frame per clip
(vqgan.py:104-116; csrc/lpips/lpips_bwd.hip), Adam on the autoencoder (vqgan.py:198-206) and the EMA codebook with random restarts
(modules/codebook.py:34-46,66-89).  Every step is `VQGAN.train_step` on the HIP operators; the GAN phase (discriminators) is not built, so
`--max_steps` beyond `--discriminator_iter_start` ends the run with a message before anything is loaded.

`--perceptual_weight` above 0 needs the perceptual weights (13 VGG-16 convolutions + five `lin` layers; nothing here fetches them): from
`--lpips_ckpt` (any file `mebt_amd.lpips.read_file` takes: a bare state dict or a first-stage checkpoint of the reference), or from the
`perceptual_model.*` tensors of the checkpoint resumed with `--vqgan_ckpt`.  Without either the run ends with a message.  Checkpoints
written while the model holds them carry them under `perceptual_model.*`, as the reference's do, so a resume needs no `--lpips_ckpt`.

Flags: the model flags of the reference's `VQGAN.add_model_specific_args`, the data flags of VideoData (`--data_path --image_folder
--resolution --sequence_length --batch_size --num_workers ...`, as `mebt_amd.measure_recon` takes them; `--data_path` is a frame folder
with train.txt), and `--max_steps`, `--log_every`, `--ckpt_every`, `--default_root_dir`, `--vqgan_ckpt` (resume: weights, codebook
buffers and step count), `--dtype {f16,f32}`, `--seed`.  The loader is cycled until `--max_steps`; one EMA update per batch (the
reference, under Lightning's two optimizers, runs `forward` and with it the update twice per batch: DESIGN.md §9f).

Checkpoints are the Lightning layout `{'state_dict', 'hyper_parameters': {'args': Namespace}, 'global_step'}` under
`<default_root_dir>/checkpoints/` (`step=<n>.ckpt` every `--ckpt_every` steps, `last.ckpt` at the end); `state_dict` holds the codebook's
`embeddings`, `N` and `z_avg`, so `load_vqgan`, `mebt_amd.measure_recon`, `python -m mebt_amd.train` and the reference read them.  The
optimizer's moments are not saved: a resumed run starts Adam afresh.
"""
import argparse
import os
import sys

import torch

from .data import TokenData


def add_model_specific_args(parser):
    """reference vqgan.py:229-252"""
    parser.add_argument('--embedding_dim', type=int, default=256)
    parser.add_argument('--n_codes', type=int, default=2048)
    parser.add_argument('--n_hiddens', type=int, default=240)
    parser.add_argument('--lr', type=float, default=3e-4)
    parser.add_argument('--downsample', nargs='+', type=int, default=(4, 4, 4))
    parser.add_argument('--disc_channels', type=int, default=64)
    parser.add_argument('--disc_layers', type=int, default=3)
    parser.add_argument('--discriminator_iter_start', type=int, default=50000)
    parser.add_argument('--disc_loss_type', type=str, default='hinge', choices=['hinge', 'vanilla'])
    parser.add_argument('--image_gan_weight', type=float, default=1.0)
    parser.add_argument('--video_gan_weight', type=float, default=1.0)
    parser.add_argument('--l1_weight', type=float, default=4.0)
    parser.add_argument('--gan_feat_weight', type=float, default=0.0)
    parser.add_argument('--perceptual_weight', type=float, default=0.0)
    parser.add_argument('--i3d_feat', action='store_true')
    parser.add_argument('--restart_thres', type=float, default=1.0)
    parser.add_argument('--no_random_restart', action='store_true')
    parser.add_argument('--norm_type', type=str, default='group', choices=['batch', 'group'])
    parser.add_argument('--padding_type', type=str, default='replicate', choices=['replicate', 'constant', 'reflect', 'circular'])
    return parser


def build_parser():
    parser = argparse.ArgumentParser(description="first-stage training, reconstruction phase: L1 + commitment loss, Adam, EMA codebook")
    parser = TokenData.add_data_specific_args(parser)
    parser = add_model_specific_args(parser)
    parser.add_argument('--max_steps', type=int, default=50000)
    parser.add_argument('--log_every', type=int, default=50)
    parser.add_argument('--ckpt_every', type=int, default=5000)
    parser.add_argument('--default_root_dir', type=str, default='vqgan_run')
    parser.add_argument('--vqgan_ckpt', type=str, default='', help='resume from this checkpoint (its hyper-parameters replace the model flags)')
    parser.add_argument('--lpips_ckpt', type=str, default='', help='the perceptual weights for --perceptual_weight > 0 (a state dict or a '
                        'reference first-stage checkpoint); not needed when --vqgan_ckpt carries perceptual_model.*')
    parser.add_argument('--dtype', type=str, default='f16', choices=['f16', 'f32'])
    parser.add_argument('--seed', type=int, default=0)
    return parser


def check_args(args, lpips_available=None):
    """what cannot run ends here, before data or model are touched.  lpips_available: whether the model holds the perceptual weights;
    None before anything is loaded, when only the flags can be judged"""
    if args.perceptual_weight > 0.0:
        ckpt = getattr(args, "lpips_ckpt", "")
        if ckpt and not os.path.isfile(ckpt):
            raise SystemExit(f"--lpips_ckpt {ckpt!r}: no such file")
        if lpips_available is None:
            lpips_available = bool(ckpt) or bool(getattr(args, "vqgan_ckpt", ""))
        if not lpips_available:
            raise SystemExit("--perceptual_weight > 0: the LPIPS backward needs the perceptual weights (13 VGG-16 convolutions, five `lin` layers): pass "
                             "--lpips_ckpt, or resume a --vqgan_ckpt that carries perceptual_model.* tensors; or set perceptual_weight to 0")
    if args.max_steps > args.discriminator_iter_start:
        raise SystemExit(f"--max_steps {args.max_steps} runs past --discriminator_iter_start {args.discriminator_iter_start}: the GAN phase "
                         "(discriminators, GAN and feature-matching losses) is not built; this command trains the reconstruction phase only")
    if args.max_steps < 1 or args.log_every < 1 or args.ckpt_every < 1:
        raise SystemExit("--max_steps, --log_every and --ckpt_every must be positive")
    if not (args.image_folder and os.path.isdir(args.data_path)):
        raise SystemExit(f"--data_path {args.data_path!r}: expected --image_folder with a frame folder that holds train.txt")


def checkpoint_dict(model, step):
    """the Lightning layout the reference's `load_from_checkpoint` and this package's `VQGAN.load_from_checkpoint` read"""
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    own = model.lpips_weights
    if own is not None:                                 # under the reference's keys and shapes: a resume, and the reference, read them
        from .lpips import PREFIX
        for k, v in own.items():
            sd[PREFIX + k] = v.detach().cpu().reshape(1, 3, 1, 1) if k.startswith("scaling_layer.") else v.detach().cpu()
    return {"state_dict": sd, "hyper_parameters": {"args": model.args}, "global_step": int(step)}


def save_checkpoint(model, step, path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(checkpoint_dict(model, step), path)
    return path


def batches(args, device):
    """float clips [B, 3, T, R, R] on the device, the training split cycled for ever"""
    from .config import AttrDict
    from .data import VideoData
    data = VideoData(AttrDict(vars(args)), True, raw=True)
    while True:
        n = 0
        for batch in data.train_dataloader():
            n += 1
            yield batch['video'].to(device, non_blocking=True).to_video()
        if n == 0:
            raise SystemExit(f'--data_path {args.data_path}: the train split gave no clip')


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_args(args)
    print(args)
    from .measure_recon import seed_everything
    from .vqgan import VQGAN
    device = torch.device('cuda')
    seed_everything(args.seed)
    step = 0
    if args.vqgan_ckpt:
        ck = torch.load(args.vqgan_ckpt, map_location='cpu', weights_only=False)
        model = VQGAN.load_from_checkpoint(args.vqgan_ckpt)
        step = int(ck.get("global_step", 0))
        print(f'resumed {args.vqgan_ckpt} at step {step}')
    else:
        hp = argparse.Namespace(**{k: v for k, v in vars(args).items()
                                   if k not in ("max_steps", "log_every", "ckpt_every", "default_root_dir", "vqgan_ckpt", "dtype", "seed")})
        hp.downsample = tuple(hp.downsample)
        del hp.lpips_ckpt
        model = VQGAN(hp)
    pw = float(model._hp("perceptual_weight", 0.0))
    if args.lpips_ckpt and pw > 0.0:
        from .lpips import read_file
        model.lpips_weights = read_file(args.lpips_ckpt)
    check_args(argparse.Namespace(**{**vars(args), "perceptual_weight": pw}), lpips_available=model.lpips_weights is not None)
    model = model.to(device).train()
    model.compute_dtype = args.dtype
    optimizer = model.configure_optimizers()
    generator = torch.Generator(device=device).manual_seed(args.seed + step)
    ckpt_dir = os.path.join(args.default_root_dir, "checkpoints")
    stream = batches(args, device)
    while step < args.max_steps:
        out = model.train_step(next(stream), optimizer, generator=generator)
        step += 1
        if step % args.log_every == 0 or step == args.max_steps:
            extra = ""
            if "perceptual_loss" in out:
                model.log("train/perceptual_loss", out["perceptual_loss"])
                extra = f" train/perceptual_loss {float(out['perceptual_loss']):.6f}"
            print(f"step {step}: recon_loss {float(out['recon_loss']):.6f} commitment_loss {float(out['commitment_loss']):.6e} "
                  f"perplexity {float(out['perplexity']):.2f} codes_restarted {int(out['codes_restarted'])} grad_scale {out['grad_scale']:g}{extra}",
                  flush=True)
        if step % args.ckpt_every == 0 and step < args.max_steps:
            print(f"wrote {save_checkpoint(model, step, os.path.join(ckpt_dir, f'step={step}.ckpt'))}")
    print(f"wrote {save_checkpoint(model, step, os.path.join(ckpt_dir, 'last.ckpt'))}")
    return model


if __name__ == '__main__':
    main(sys.argv[1:])
