#!/usr/bin/env python3
"""`python -m mebt_amd.evaluate` — the sweep of the reference's scripts/valid_dnr_*.sh in one process: for every run, sample the
draft clips, score them, revise the code maps just written, score again.

  python -m mebt_amd.evaluate --base cfg.yaml --gpt_ckpt run.ckpt --exp_name ucf --runs 0-9 --total_length 16 --step_size 16 \\
      --context_size 16 --vid_n_steps 128 --vid_c_temp 6.0 --no_phase --decoding_strategy maskgit --batch_size 16 --n_sample 2048 \\
      --n_revise 4 --M 4 --revise_t 0.7 --dataset ucf101 --data_path datasets/vqgan_data/ucf_128 --image_folder --train \\
      --real_embeddings results/ucf/real_ucf_16.npy

The shipped scripts start four processes per run (sample, measure FVD, draft-and-revise, measure FVD); each loads the checkpoint, the
first stage and the I3D, embeds the real set again, moves its pixel samples to the host as float32 and reads them back from a file.
Here the transformer, the first stage and the I3D are loaded once, the real set is embedded once (`measure_fvd.real_embeddings`, so
`--real_embeddings FILE` caches it across invocations too), and the clips stay where the decoder left them: the decode is turned
into the uint8 clips of the .npy on the GPU (mebt_amd/frames.py:video_to_clip_u8) inside a `scripts_common.ClipStore`, and the I3D
reads the selected clips from it.

Flags: those of `mebt_amd.sample`, the revise flags of `mebt_amd.draft_and_revise` (`--n_revise --revise_t --revise_k --revise_p
--M`) and the scoring flags of `mebt_amd.measure_fvd` (`--data_path --image_folder --train --packed_path --real_embeddings --i3d_ckpt
--i3d_dtype --i3d_batch --n_neighbor --sample_fake_n_frames`; `--sequence_length` defaults to `--total_length`), plus
  --runs 0-9             the runs, a range or a comma list (instead of --run)
  --stages draft,revise  either or both; `revise` alone revises the code maps an earlier draft stage wrote
  --keep_np              also write the `.npy` video files (default: only the code maps, which are always written)

Every stage is the command line it replaces, on the same model: the draft stage is `mebt_amd.sample.run`, the revise stage is
`mebt_amd.draft_and_revise.run` given `--np_draft <the draft's code map file>`, so the file names (and what `apply_np_draft` parses
from them) are the reference's.  Output: per run and stage the CSV `measure_fvd` would write for that stage's `.npy` name, the
summary `results/<exp_name>/evaluate_<total_length>_<dataset>.csv` (run,stage,FVD,KVD) and one line per stage with the mean and
the sample standard deviation over the runs."""
import argparse
import copy
import csv
import os
import sys

import numpy as np
import torch

from . import draft_and_revise, measure_fvd, sample
from .scripts_common import ClipStore, data_resolution, load_model, resolve_checkpoint

STAGES = ("draft", "revise")


def parse_runs(text):
    """'0-9' -> 0..9, '0,2,5' -> those, '3' -> [3]; ranges and single runs mix ('0-2,7')"""
    runs = []
    for part in str(text).split(','):
        part = part.strip()
        if '-' in part:
            lo, hi = part.split('-', 1)
            if int(hi) < int(lo):
                raise argparse.ArgumentTypeError(f"--runs {text!r}: {part!r} is empty")
            runs += list(range(int(lo), int(hi) + 1))
        elif part:
            runs.append(int(part))
    if not runs:
        raise argparse.ArgumentTypeError(f"--runs {text!r}: no run")
    return runs


def parse_stages(text):
    stages = [s.strip() for s in str(text).split(',') if s.strip()]
    if not stages or any(s not in STAGES for s in stages) or len(set(stages)) != len(stages):
        raise argparse.ArgumentTypeError(f"--stages {text!r}: draft, revise or draft,revise")
    return [s for s in STAGES if s in stages]


def build_parser():
    parser = sample.build_parser()
    parser.description = "sample, revise and score a checkpoint in one process (the sweep of the reference's scripts/valid_dnr_*.sh)"
    # the revise phase (the draft phase is the sample stage's code map, as in the shipped scripts), then the scoring
    draft_and_revise.add_revise_args(parser)
    measure_fvd.add_scoring_args(parser)
    # the sweep
    parser.add_argument('--runs', type=parse_runs, default=parse_runs('0-9'), help="a range or a comma list, e.g. 0-9 or 0,3,4")
    parser.add_argument('--stages', type=parse_stages, default=list(STAGES), help="draft, revise or draft,revise")
    parser.add_argument('--keep_np', action='store_true', help="also write the .npy video files")
    parser.set_defaults(sequence_length=None)
    return parser


def parse_args(argv=None):
    args, unknown = build_parser().parse_known_args(argv)
    if args.sequence_length is None:
        args.sequence_length = args.total_length
    return args, unknown


def draft_args(args, run):
    """the namespace `mebt_amd.sample` would have parsed for this run"""
    a = copy.copy(args)
    a.run, a.save_codemap, a.no_np = run, True, False
    return a


def revise_args(args, run):
    """the namespace `mebt_amd.draft_and_revise --np_draft <the draft stage's code map>` would have parsed for this run (before
    `apply_np_draft`)"""
    a = draft_and_revise.build_parser().parse_args([])
    for k, v in vars(args).items():
        if hasattr(a, k):
            setattr(a, k, v)
    a.save = args.save
    a.run, a.save_codemap, a.no_np = run, True, False
    a.np_draft = sample.output_names(draft_args(args, run))[1] + '_codemap.npy'
    return a


def stage_csv_names(args, run):
    """{stage: the CSV `measure_fvd --np_file <that stage's .npy>` writes}; parses the draft file's name only, reads nothing"""
    a = revise_args(args, run)
    out = {"draft": measure_fvd.consq_csv_name(a.np_draft.replace('_codemap.npy', '.npy'), args.n_neighbor)}
    _, postfix = draft_and_revise.apply_np_draft(a, load=False)
    out["revise"] = measure_fvd.consq_csv_name(draft_and_revise.output_names(a, postfix)[1] + '.npy', args.n_neighbor)
    return out


def fvd_args(args, np_file):
    """the namespace `mebt_amd.measure_fvd` works from (its main forces the batch size to 32)"""
    a = copy.copy(args)
    a.batch_size, a.np_file, a.score_file = 32, np_file, ''
    return a


def summary_path(args):
    return f'{args.save}/evaluate_{args.total_length}_{args.dataset}.csv'


def main(argv=None):
    from .fvd import frechet_distance, polynomial_mmd
    args, unknown = parse_args(argv)
    resolution = data_resolution(args, unknown)
    resolve_checkpoint(args)
    print(args.gpt_ckpt)
    os.makedirs(args.save, exist_ok=True)
    gpt = load_model(args)
    if gpt.first_stage_model is None:
        raise SystemExit("evaluate: the checkpoint has no first stage (a vtokens model): no pixel samples, nothing to score")
    model_schedule = gpt.mask_sampler.schedule
    device = torch.device('cuda')
    i3d = measure_fvd.load_model(args, device)
    real = measure_fvd.real_embeddings(fvd_args(args, ''), i3d, device)

    n_rows = max(sample.n_clips(args) if "draft" in args.stages else 0, draft_and_revise.n_clips(args, None) if "revise" in args.stages else 0)
    store = ClipStore(n_rows, args.total_length, resolution, resolution, where=args.u8_store)
    print(f'clip store: {store.nbytes / 2 ** 20:.1f} MiB on the {store.where}')

    rows = []
    for run in args.runs:
        for stage in args.stages:
            store.reset()
            if stage == "draft":
                a = draft_args(args, run)
                gpt.mask_sampler.schedule = args.schedule                       # sample.py main
                save_np, clips = sample.run(a, gpt, resolution, store, keep_np=args.keep_np)
            else:
                a = revise_args(args, run)
                if not os.path.isfile(a.np_draft):
                    raise SystemExit(f"--stages revise: {a.np_draft} not found (the draft stage of run {run} writes it)")
                gpt.mask_sampler.schedule = model_schedule
                draft, postfix = draft_and_revise.apply_np_draft(a)
                save_np, clips = draft_and_revise.run(a, gpt, resolution, draft, postfix, store, keep_np=args.keep_np)
            fa = fvd_args(args, save_np + '.npy')
            print('computing fvd embeddings for fake videos')
            fake = measure_fvd.fake_embeddings(fa, clips, i3d, device)
            fvd, kvd = frechet_distance(fake, real), polynomial_mmd(fake, real)
            print(f'run {run} {stage}: FVD = {fvd:.2f} KVD = {kvd:.2f}')
            out = measure_fvd.consq_csv_name(fa.np_file, args.n_neighbor)
            measure_fvd.write_csv(out, ['FVD', 'KVD'], [[fvd, kvd]])
            print(f'wrote {out}')
            rows.append((run, stage, float(fvd), float(kvd)))
    with open(summary_path(args), 'w', newline='') as f:
        w = csv.writer(f, lineterminator='\n')
        w.writerow(['run', 'stage', 'FVD', 'KVD'])
        for run, stage, fvd, kvd in rows:
            w.writerow([run, stage, repr(fvd), repr(kvd)])
    print(f'wrote {summary_path(args)}')
    for stage in args.stages:
        v = np.array([(r[2], r[3]) for r in rows if r[1] == stage], dtype=np.float64)
        sd = v.std(0, ddof=1) if len(v) > 1 else np.full(2, np.nan)
        print(f'{stage}: FVD {v[:, 0].mean():.2f} +- {sd[0]:.2f}  KVD {v[:, 1].mean():.2f} +- {sd[1]:.2f}  ({len(v)} runs)')
    return rows


if __name__ == '__main__':
    main(sys.argv[1:])
