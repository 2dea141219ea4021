"""`python -m mebt_amd.measure_sliding_fvd` — FVD / KVD of every `sequence_length`-frame window of long (128-frame) samples, one
window start t every `--slide` frames over range(0, 128 - sequence_length) (reference measure_sliding_fvd_with_numpy.py), on the
HIP I3D.  Flags and the real side as `mebt_amd.measure_fvd`: saved embeddings, a frame folder (`--image_folder`, or its pack
with `--packed_path`) or an .npy of clips.

Output: `<np_file>_slide<slide>_clip<sequence_length>_<n_neighbor>.csv` in pandas' to_csv layout with the columns t, fvd, kvd.
The reference builds its DataFrame from these plus four empty columns (p, r, d, c) of another length, which pandas rejects;
those columns are not written.
"""
import sys

import numpy as np
import torch

from .measure_fvd import build_parser, load_model, real_embeddings, fake_embeddings, write_csv, sliding_csv_name

TOTAL_FRAMES = 128          # the reference's window range: range(0, 128 - sequence_length, slide)


def main(argv=None):
    args = build_parser(sliding=True).parse_args(argv)
    print(args)
    from .fvd import frechet_distance, polynomial_mmd
    args.batch_size = 32
    print('loading numpy file from %s...' % args.np_file)
    all_data_np = np.load(args.np_file, mmap_mode='r')
    if all_data_np.shape[1] < TOTAL_FRAMES - 1:
        raise SystemExit(f'{args.np_file}: {all_data_np.shape[1]} frames; the sliding windows span {TOTAL_FRAMES}')
    device = torch.device('cuda')
    i3d = load_model(args, device)
    real = real_embeddings(args, i3d, device)
    rows = []
    for t in range(0, TOTAL_FRAMES - args.sequence_length, args.slide):
        print(f'computing fvd embeddings for fake videos, frames {t}..{t + args.sequence_length - 1}')
        fake = fake_embeddings(args, all_data_np, i3d, device, t0=t)
        fvd = frechet_distance(fake, real)
        kvd = polynomial_mmd(fake, real)
        print('FVD = %.2f' % fvd)
        print('KVD = %.2f' % kvd)
        rows.append([t, fvd, kvd])
    out = sliding_csv_name(args.np_file, args.slide, args.sequence_length, args.n_neighbor)
    write_csv(out, ['t', 'fvd', 'kvd'], rows)
    print(f'wrote {out}')
    return rows


if __name__ == '__main__':
    main(sys.argv[1:])
