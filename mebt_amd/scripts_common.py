"""What the two sampling command lines share (reference sample_vqgan_transformer_videos.py:160-297 and
draft_and_revise_videos.py:64-198): the common flags, checkpoint resolution, the output naming scheme and the writers."""
import math
import os
from glob import glob

import numpy as np


def add_common_args(parser):
    """flags both reference scripts define with the same meaning (+ the data flags they inherit from VideoData and the two
    Lightning trainer flags their bodies read)"""
    from .data import TokenData
    parser.add_argument('--base', nargs='*', default=[], metavar="base_config.yaml")
    parser = TokenData.add_data_specific_args(parser)
    parser.add_argument('--default_root_dir', type=str, default=None)          # pl.Trainer.add_argparse_args (the only trainer flags the scripts read)
    parser.add_argument('--gpus', default=None)
    parser.add_argument('--gpt_ckpt', type=str, default='')
    parser.add_argument('--exp_name', type=str, default='')
    parser.add_argument('--save', type=str, default='./results/mebt')
    parser.add_argument('--total_length', type=int, default=None)
    parser.add_argument('--context_size', type=int, default=12)
    parser.add_argument('--step_size', type=int, default=16)
    parser.add_argument('--run', type=int, default=0)
    parser.add_argument('--n_sample', type=int, default=2048)
    parser.add_argument('--dataset', type=str, default='mshapes', choices=['ucf101', 'stl', 'taichi', 'mshapes'])
    parser.add_argument('--format', type=str, default='gif', choices=['webp', 'mp4', 'gif', 'avi'])
    parser.add_argument('--save_videos', action='store_true')
    parser.add_argument('--save_n', type=int, default=5)
    parser.add_argument('--save_codemap', action='store_true')
    parser.add_argument('--no_np', action='store_true')
    parser.add_argument('--latest', action='store_true')
    parser.add_argument('-v', '--verbose', action='store_true')
    parser.add_argument('--device_u8', action='store_true',
                        help="make the uint8 clips of the .npy on the GPU (mebt_amd/frames.py:video_to_clip_u8) instead of moving float32 "
                             "samples to the host: the same file, a quarter of the bytes over PCIe and no float copies in host memory")
    parser.add_argument('--u8_store', default='auto', choices=['auto', 'device', 'host'],
                        help="with --device_u8: where the uint8 clips wait for the writer (auto: in HBM when they take at most a "
                             "quarter of the free device memory, else in pinned host memory)")
    parser.add_argument('--dtype', default=None, choices=['bf16', 'f32'], help="engine precision (default: MEBT_COMPUTE_DTYPE or bf16)")
    return parser


def resolve_checkpoint(args):
    """--gpt_ckpt, or the experiment's best / latest checkpoint under logs/<exp_name>/ (reference :201-210 / :107-116); sets
    args.save = results/<exp_name>[_latest] exactly like the scripts do"""
    ver = args.exp_name
    args.save = f'results/{ver}'
    if args.gpt_ckpt == '':
        if not args.latest:
            found = glob(f'logs/{ver}/lightning_logs/version_0/checkpoints/best_checkpoint.ckpt')
            if not found:
                raise FileNotFoundError(f"no --gpt_ckpt and no logs/{ver}/lightning_logs/version_0/checkpoints/best_checkpoint.ckpt")
            args.gpt_ckpt = found[0]
        else:
            ckpts = glob(f'logs/{ver}/lightning_logs/version_0/checkpoints/*/loss=*.ckpt')
            iters = [int(ckpt.split('step=')[-1].split('-train')[0]) for ckpt in ckpts]
            if not iters:
                raise FileNotFoundError(f"--latest: no logs/{ver}/lightning_logs/version_0/checkpoints/*/loss=*.ckpt")
            max_iter = max(iters)
            args.gpt_ckpt = glob(f'logs/{ver}/lightning_logs/version_0/checkpoints/*step={max_iter}-train/loss=*.ckpt')[0]
            args.save += '_latest'
    return args.gpt_ckpt


def load_model(args):
    """load_transformer(args.gpt_ckpt, vqgan_ckpt=None).cuda().eval() of the scripts (:218 / :138) through the restricted unpickler"""
    import torch
    from .transformer import Net2NetTransformer
    model = Net2NetTransformer.load_from_checkpoint(args.gpt_ckpt)
    if args.dtype:
        model.compute_dtype = args.dtype
    if not torch.cuda.is_available():
        raise RuntimeError("mebt_amd has no CPU path: the sampling scripts need the MI355X (cuda) device")
    return model.cuda().eval()


def data_resolution(args, unknown):
    """the resolution of the samples as the command lines take it (:195-199 / :101-105): `data.resolution` of the `--base` configs
    (with the key=value overrides among the unknown flags) when they describe an image folder, else --resolution"""
    from .config import load_config
    config = load_config(args.base, [u for u in unknown if "=" in u])
    return config.data.resolution if ("data" in config and config.data.get("image_folder", False)) else args.resolution


def save_video_grid(video, fname, nrow=None, fps=10):
    """reference mebt/utils.py:149-171: [B, C, T, H, W] in [0, 1] -> one animated grid file"""
    from PIL import Image
    b, c, t, h, w = video.shape
    video = (video.permute(0, 2, 3, 4, 1).cpu().numpy() * 255).astype('uint8')
    if nrow is None:
        nrow = math.ceil(math.sqrt(b))
    ncol = math.ceil(b / nrow)
    pad = 1
    grid = np.zeros((t, (pad + h) * nrow + pad, (pad + w) * ncol + pad, c), dtype='uint8')
    for i in range(b):
        r, cc = i // ncol, i % ncol
        grid[:, (pad + h) * r:(pad + h) * r + h, (pad + w) * cc:(pad + w) * cc + w] = video[i]
    frames = [Image.fromarray(f, 'RGB') for f in grid]
    frames[0].save(fname, quality=95, save_all=True, append_images=frames[1:], duration=1000 / fps, loop=0, optimize=False)
    print('saved videos to', fname)


def write_codemap(args, save_np, all_code, codemap_limit=None):
    """the first half of both writers: the directory of the outputs, and `<save_np>_codemap.npy` (token ids) with --save_codemap"""
    os.makedirs(os.path.dirname(save_np), exist_ok=True)
    if args.save_codemap:
        print('saving code_map numpy file to %s...' % (save_np + '_codemap'))
        code = np.concatenate(all_code, 0)
        np.save(save_np + '_codemap', code if codemap_limit is None else code[:codemap_limit])


def write_outputs(args, save_np, all_data, all_code, resolution, codemap_limit=None):
    """the tail of both scripts (:275-291 / :180-198): `<save_np>_codemap.npy` (token ids) and `<save_np>.npy` (uint8 videos
    [n, T, H, W, C], a random subset of n_sample) — the video file only when a first stage produced pixel samples"""
    write_codemap(args, save_np, all_code, codemap_limit)
    if not args.no_np:
        if not all_data:
            print('no first stage attached (vtokens model): no pixel samples to save, token ids only (--save_codemap)')
            return
        print('saving numpy file to %s...' % save_np)
        data = np.concatenate(all_data, 0)               # (the reference stacks with np.array: the same for equal batches, an error for a short last one)
        data = np.transpose(data.reshape(-1, 3, args.total_length, resolution, resolution), (0, 2, 3, 4, 1))      # B T H W C
        n_total = data.shape[0]
        data = (data * 255).astype(np.uint8)[np.random.permutation(n_total)[:args.n_sample]]
        np.save(save_np, data)


class ClipStore:
    """the uint8 clips [n_total, T, H, W, 3] of one sampling run, preallocated and filled row block by row block from the decoded
    batches (mebt_amd/frames.py:video_to_clip_u8) in place of the reference's list of float32 arrays on the host.
      where='device': the buffer lives in HBM; `target(b)` is the view of the next b rows for the kernel to write (no copy).
      where='host':   a pinned host buffer filled with `non_blocking` copies; one synchronisation before the first read.
      where='auto':   'device' when the buffer takes at most a quarter of the free device memory (the sampler's workspace and the
                      key / value cache need the rest: the rule of `data.packed_resident: auto`), else 'host'."""

    AUTO_FRACTION = 0.25

    def __init__(self, n_total, T, H, W, where="auto", device="cuda"):
        import torch
        if where not in ("auto", "device", "host"):
            raise ValueError(f"ClipStore: where={where!r} (auto, device or host)")
        self.shape = (int(n_total), int(T), int(H), int(W), 3)
        self.nbytes = int(np.prod(self.shape))
        if where == "auto":
            where = self.placement(self.nbytes)
        self.where = where
        if where == "device":
            self.buf = torch.empty(self.shape, dtype=torch.uint8, device=device)
        else:
            self.buf = torch.empty(self.shape, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        self.n = 0
        self._pending = False

    @classmethod
    def placement(cls, nbytes):
        """what where='auto' chooses for a store of `nbytes`"""
        import torch
        return "device" if torch.cuda.is_available() and nbytes <= cls.AUTO_FRACTION * torch.cuda.mem_get_info()[0] else "host"

    def reset(self):
        """empty the store for the next run; the buffer is kept"""
        self.sync()
        self.n = 0

    def target(self, b):
        """what a driver's `samples_u8=` gets for a batch of b clips: the next b rows (device), or True (host: a clip of its own)"""
        if self.n + b > self.shape[0]:
            raise ValueError(f"ClipStore: {self.n} + {b} clips exceed the {self.shape[0]} rows it was made for")
        return self.buf[self.n:self.n + b] if self.where == "device" else True

    def put(self, clip):
        """append uint8 clips [b, T, H, W, 3] (a device or host tensor, or a numpy array); rows handed out by `target` are in place"""
        import torch
        clip = torch.as_tensor(clip)
        b = int(clip.shape[0])
        if clip.dtype != torch.uint8 or tuple(clip.shape[1:]) != self.shape[1:]:
            raise ValueError(f"ClipStore: expected uint8 [b, {', '.join(map(str, self.shape[1:]))}], got {clip.dtype} {tuple(clip.shape)}")
        rows = self.target(b)
        if self.where == "device":
            if clip.data_ptr() != rows.data_ptr():
                rows.copy_(clip, non_blocking=True)
        else:
            self.buf[self.n:self.n + b].copy_(clip, non_blocking=True)
            self._pending = self._pending or clip.is_cuda
        self.n += b

    def sync(self):
        if self._pending:
            import torch
            torch.cuda.synchronize()
            self._pending = False

    def select(self, idx):
        """rows `idx` (an integer numpy array) of the filled part, in that order: a device tensor or a host tensor, like the store"""
        import torch
        self.sync()
        idx = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64))
        return self.buf[:self.n].index_select(0, idx.to(self.buf.device))


def write_outputs_u8(args, save_np, store, all_code, codemap_limit=None, keep_np=True):
    """`write_outputs` for clips that are already bytes in a ClipStore: the same `<save_np>_codemap.npy`, the same
    `np.random.permutation(n_total)[:args.n_sample]` call at the same point, the same `<save_np>.npy` (not written with
    keep_np=False).  Returns the selected clips uint8 [n, T, H, W, C], on the device when the store is (None without pixel samples)."""
    write_codemap(args, save_np, all_code, codemap_limit)
    if not args.no_np:
        if store is None or store.n == 0:
            print('no first stage attached (vtokens model): no pixel samples to save, token ids only (--save_codemap)')
            return None
        n_total = store.n
        data = store.select(np.random.permutation(n_total)[:args.n_sample])
        if keep_np:
            print('saving numpy file to %s...' % save_np)
            np.save(save_np, data.cpu().numpy())
        return data
    return None


def make_store(args, gpt, n_clips, resolution):
    """--device_u8: the ClipStore for the `n_clips` clips of one run, when a first stage decodes pixel samples and the .npy is wanted"""
    if args.device_u8 and gpt.first_stage_model is not None and not args.no_np:
        return ClipStore(n_clips, args.total_length, resolution, resolution, where=args.u8_store)
    return None


class BatchSink:
    """where both `run`s leave a batch's logs: the grids of the first --save_n batches (--save_videos) under `save_dir`, the pixel
    samples as uint8 clips in `store` (without one: in `all_data` as float32 arrays on the host, like the reference), the code maps
    in `all_code` and the --verbose line"""

    def __init__(self, args, save_dir, n_row, n_batch, store=None):
        self.args, self.save_dir, self.n_row, self.n_batch, self.store = args, save_dir, n_row, n_batch, store
        self.all_data, self.all_code = [], []
        print('generating and saving video to %s...' % save_dir)
        os.makedirs(save_dir, exist_ok=True)

    def target(self, b):
        """the keyword a driver gets for a batch of b clips: `samples_u8=` the store's next rows, or nothing"""
        return dict(samples_u8=self.store.target(b)) if self.store is not None else {}

    def put(self, sample_id, logs, fps=10):
        if "samples" in logs:
            if self.args.save_videos and sample_id < self.args.save_n:
                save_video_grid(logs['samples'], os.path.join(self.save_dir, 'generation_%d.%s' % (sample_id, self.args.format)), self.n_row, fps=fps)
            if self.store is not None:
                self.store.put(logs['samples_u8'])
            else:
                self.all_data.append(logs['samples'].cpu().numpy())
        self.all_code.append(logs['code_maps'].cpu().numpy())
        if self.args.verbose:
            print(f"batch {sample_id + 1}/{self.n_batch}: code map {tuple(logs['code_maps'].shape)}", flush=True)
