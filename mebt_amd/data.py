"""Token-grid data contract of the hot path — counterpart of the `vtokens` branch of reference mebt/data.py:
`HDF5Dataset_vtokens` (:330-414, items `{'video' [T,H,W] int64, 'cbox', 'indices' = randperm(prod(latent_shape))}`)
and the sharding `VideoData._dataloader` gets from `DistributedSampler` (:271-292).  Token files are `.npz` (or HDF5
when h5py is installed) with the reference's keys: `{train,test}_data` [frames,H,W] and `{train,test}_idx` (start frame
of every video plus a trailing sentinel).  Random draws use torch's global generator with the same calls in the same
order as the reference, so a seeded run picks the same clips, crops and permutations.

The frame-folder branch (`image_folder`, FrameListDataset, VideoData) sits at the end of the module."""
import functools
import os
import random

import numpy as np
import torch


def _open(path):
    if str(path).endswith((".h5", ".hdf5")):
        import h5py                                    # optional dependency, exactly the reference's container
        return h5py.File(path, "r")
    return np.load(path)


class TokenClipDataset(torch.utils.data.Dataset):
    """reference HDF5Dataset_vtokens (data.py:330-414)"""

    def __init__(self, data_file, sequence_length, train=True, resolution=15, spatial_length=15, sample_every_n_frames=1,
                 latent_shape=()):
        super().__init__()
        self.train, self.sequence_length = train, sequence_length
        self.resolution, self.spatial_length = resolution, spatial_length
        self.sample_every_n_frames = sample_every_n_frames
        self.latent_shape = list(latent_shape)
        self.data_file = data_file
        self.prefix = "train" if train else "test"
        f = _open(data_file)
        self._tokens = np.array(f[f"{self.prefix}_data"])
        self._idx = np.array(f[f"{self.prefix}_idx"][:-1])       # data.py:361 (the sentinel is dropped)
        self.size = len(self._idx)
        if self.resolution is None:                               # token files carry their own grid size
            self.resolution = int(self._tokens.shape[1])
        if self.spatial_length is None:
            self.spatial_length = self.resolution
        ends = np.append(self._idx[1:], len(self._tokens))
        if self.size == 0 or int((ends - self._idx).max()) <= sequence_length:   # the reference would resample forever
            raise ValueError(f"{data_file}: no {self.prefix} video is longer than sequence_length={sequence_length} token frames")

    n_classes = 0                                                 # unconditional token sets (data.py:368-370)

    def __len__(self):
        return self.size

    def __getitem__(self, idx):
        start = self._idx[idx]
        end = self._idx[idx + 1] if idx < len(self._idx) - 1 else len(self._tokens)
        if end - start <= self.sequence_length:                   # clip too short: draw another video (data.py:391-392)
            return self.__getitem__(torch.randint(low=0, high=self.size, size=(1,)).item())
        start = start + torch.randint(low=0, high=int(end - start - self.sequence_length), size=(1,)).item()
        if self.spatial_length == self.resolution:
            video = torch.tensor(self._tokens[start:start + self.sequence_length]).long()
            box = 0
        else:
            y0 = torch.randint(low=0, high=self.resolution - self.spatial_length + 1, size=(1,)).item()
            x0 = torch.randint(low=0, high=self.resolution - self.spatial_length + 1, size=(1,)).item()
            video = torch.tensor(self._tokens[start:start + self.sequence_length, y0:y0 + self.spatial_length,
                                              x0:x0 + self.spatial_length]).long()
            box = np.array([y0, y0 + self.spatial_length, x0, x0 + self.spatial_length])
        if self.sample_every_n_frames > 1:
            video = video[::self.sample_every_n_frames]
        return dict(video=video, cbox=box, indices=torch.randperm(int(np.prod(self.latent_shape))))


class SyntheticTokenDataset(torch.utils.data.Dataset):
    """uniform random token grids of `shape` (what bench.py and the launcher use without a token file)"""

    def __init__(self, shape, size=1 << 16, vocab=16384):
        self.shape, self.size, self.vocab = tuple(shape), size, vocab

    def __len__(self):
        return self.size

    def __getitem__(self, idx):
        return dict(video=torch.randint(0, self.vocab, self.shape), cbox=0, indices=torch.randperm(int(np.prod(self.shape))))


class ShardedSampler(torch.utils.data.Sampler):
    """torch.utils.data.distributed.DistributedSampler semantics without a process group: shuffle with seed + epoch,
    pad by wrapping to a multiple of `num_replicas`, rank r takes positions r, r + R, r + 2R, ..."""

    def __init__(self, dataset_len, num_replicas=1, rank=0, shuffle=True, seed=0, drop_last=False):
        self.n, self.R, self.rank, self.shuffle, self.seed, self.drop_last = dataset_len, num_replicas, rank, shuffle, seed, drop_last
        self.epoch = 0
        self.num_samples = (self.n // self.R) if (drop_last and self.n % self.R) else -(-self.n // self.R)
        self.total_size = self.num_samples * self.R

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return self.num_samples

    def __iter__(self):
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            idx = torch.randperm(self.n, generator=g).tolist()
        else:
            idx = list(range(self.n))
        if not self.drop_last:
            pad = self.total_size - len(idx)
            idx += idx[:pad] if pad <= len(idx) else (idx * -(-pad // len(idx)))[:pad]
        else:
            idx = idx[:self.total_size]
        return iter(idx[self.rank:self.total_size:self.R])


class TokenData:
    """`VideoData` for token grids (data.py:236-305): `args` carries data_path, sequence_length, resolution,
    spatial_length, sample_every_n_frames, latent_shape, batch_size, num_workers like the reference's config `data:` node."""

    def __init__(self, args, shuffle=True, world_size=1, rank=0):
        self.args, self.shuffle, self.world_size, self.rank = args, shuffle, world_size, rank

    def _dataset(self, train):
        a = self.args
        g = (lambda k, d: a[k] if (hasattr(a, "__contains__") and k in a) else getattr(a, k, d))
        if not g("data_path", None):
            return SyntheticTokenDataset(g("latent_shape", [4, 16, 16]))
        return TokenClipDataset(g("data_path", None), g("sequence_length", 4), train=train, resolution=g("resolution", 16),
                                spatial_length=g("spatial_length", g("resolution", 16)),
                                sample_every_n_frames=g("sample_every_n_frames", 1), latent_shape=g("latent_shape", [1]))

    def _dataloader(self, train):
        ds = self._dataset(train)
        a = self.args
        g = (lambda k, d: a[k] if (hasattr(a, "__contains__") and k in a) else getattr(a, k, d))
        sampler = ShardedSampler(len(ds), self.world_size, self.rank) if self.world_size > 1 else None
        nw = g("num_workers", 0)
        return torch.utils.data.DataLoader(ds, batch_size=g("batch_size", 6), num_workers=nw, pin_memory=True, sampler=sampler,
                                           shuffle=sampler is None and self.shuffle, persistent_workers=bool(train and nw > 0))

    def train_dataloader(self):
        return self._dataloader(True)

    def val_dataloader(self):
        return self._dataloader(False)

    test_dataloader = val_dataloader

    @staticmethod
    def add_data_specific_args(parent_parser):
        """the data flags of the reference's scripts (data.py:307-327), so that their command lines parse unchanged"""
        import argparse
        parser = argparse.ArgumentParser(parents=[parent_parser], add_help=False)
        parser.add_argument('--data_path', type=str, default='')
        parser.add_argument('--sequence_length', type=int, default=16)
        parser.add_argument('--resolution', type=int, default=128)
        parser.add_argument('--batch_size', type=int, default=32)
        parser.add_argument('--num_workers', type=int, default=8)
        parser.add_argument('--image_channels', type=int, default=3)
        parser.add_argument('--smap_cond', type=int, default=0)
        parser.add_argument('--smap_only', action='store_true')
        parser.add_argument('--text_cond', action='store_true')
        parser.add_argument('--vtokens', action='store_true')
        parser.add_argument('--vtokens_pos', action='store_true')
        parser.add_argument('--spatial_length', type=int, default=15)
        parser.add_argument('--sample_every_n_frames', type=int, default=1)
        parser.add_argument('--image_folder', action='store_true')
        parser.add_argument('--stft_data', action='store_true')
        parser.add_argument('--preprocessed_hdf5', action='store_true')
        return parser


# ---- pixel-space data: the reference's `image_folder` branch (mebt/data.py:419-521) --------------------------------------
IMG_EXTENSIONS = ['.jpg', '.JPG', '.jpeg', '.JPEG', '.png', '.PNG']


def is_image_file(filename):
    return any(filename.endswith(extension) for extension in IMG_EXTENSIONS)


def _open_rgb(path):
    from PIL import Image
    img = Image.open(path)
    if img.mode != "RGB":       # the reference would fail later, in the first stage's 3-channel convolution
        raise ValueError(f"{path}: frame mode {img.mode!r}, the frame datasets take 8-bit RGB images only (convert them to RGB)")
    return img


class FrameListDataset(torch.utils.data.Dataset):
    """reference FrameListDataset (data.py:431-521): frames `[VIDEO_ID]_[FRAME_NUM].png` listed in `data_folder`/train.txt or
    test.txt.  Items are {'video' float32 [3, T, R, R] in [-0.5, 0.5], 'indices' randperm(prod(latent_shape))}, made with the
    same random calls in the same order (`random.randint` for the start frame, then torch's randperm).

    raw=True: the same random calls, but no crop / resize / normalisation: 'video' is the decoded uint8 [T, Hs, Ws, 3] at the
    source size, for the GPU ingest (mebt_amd/frames.py, collate with `frames.collate_raw`)."""

    def load_video_frames(self, dataroot):
        list_file = os.path.join(dataroot, 'train.txt' if self.train else 'test.txt')
        with open(list_file, "r") as f:
            paths = f.read().splitlines()
        paths = sorted(paths)                       # string order: v_10.png before v_2.png (a break starts a new video)
        data_all = []
        video_id = ''
        video_frames = []
        last_frame = 0
        cnt = 0
        for path in paths:
            file_name = path.split('/')[-1]
            cur_video = ''.join(path.split('/')[:-1]) + ''.join(file_name.split('_')[:-1])
            cur_frame = int(file_name.split('_')[-1].split('.')[0])     # parsed before the extension check, as the reference does
            if video_id != cur_video or cur_frame != (last_frame + 1):
                if video_id == cur_video and cur_frame != (last_frame + 1):
                    cnt += 1
                video_id = cur_video
                if len(video_frames) > 0:
                    if len(video_frames) >= max(0, self.sequence_length * self.sample_every_n_frames):
                        data_all.append(video_frames)
                    video_frames = []
            if is_image_file(path):
                video_frames.append(path)
            last_frame = cur_frame
        # the last video of the list is never flushed (reference behaviour)
        self.video_num = len(data_all)
        self.discontinuities = cnt
        print(f"Total num of videos: {self.video_num}")
        print(f"Total num of discontinuous videos: {cnt}")
        return data_all

    def __init__(self, data_folder, sequence_length, resolution=64, sample_every_n_frames=1, train=True, latent_shape=[],
                 raw=False):
        self.resolution = resolution
        self.sequence_length = sequence_length
        self.sample_every_n_frames = sample_every_n_frames
        self.train = train
        self.raw = raw
        self.data_all = self.load_video_frames(data_folder)
        self.latent_shape = latent_shape

    n_classes = 0

    def __getitem__(self, index):
        batch_data = self.getTensor(index)
        return {'video': batch_data, 'indices': torch.randperm(int(np.prod(self.latent_shape)))}

    def _clip_range(self, video_len):
        if self.sequence_length == -1:              # the whole video
            assert self.sample_every_n_frames == 1
            return 0, video_len
        n_frames_interval = self.sequence_length * self.sample_every_n_frames
        start_idx = random.randint(0, video_len - n_frames_interval)
        return start_idx, start_idx + n_frames_interval

    def getTensor(self, index):
        from PIL import Image
        video = self.data_all[index]
        start_idx, end_idx = self._clip_range(len(video))
        img = _open_rgb(video[0])
        h, w = img.height, img.width
        if h > w:
            half = (h - w) // 2
            cropsize = (0, half, w, half + w)       # left, upper, right, lower
        elif w > h:
            half = (w - h) // 2
            cropsize = (half, 0, half + h, h)
        images = []
        for i in range(start_idx, end_idx, self.sample_every_n_frames):
            img = _open_rgb(video[i])
            if self.raw:
                if (img.height, img.width) != (h, w):
                    raise ValueError(f"{video[i]}: {img.height}x{img.width} frame in a clip of {h}x{w} frames")
                images.append(np.asarray(img, dtype=np.uint8))
                continue
            if h != w:
                img = img.crop(cropsize)
            if h != self.resolution or w != self.resolution:       # the uncropped size decides, as in the reference
                img = img.resize((self.resolution, self.resolution), Image.BILINEAR)
            img = np.asarray(img, dtype=np.float32)
            img /= 255.
            images.append(torch.from_numpy(img - 0.5).unsqueeze(0))
        if self.raw:
            return torch.from_numpy(np.stack(images))
        return torch.cat(images).permute(3, 0, 1, 2)

    def __len__(self):
        return self.video_num


def _arg(a, k, d):
    return a[k] if (hasattr(a, "__contains__") and k in a) else getattr(a, k, d)


class VideoData(TokenData):
    """reference VideoData._dataset (data.py:248-273): `vtokens` -> token clips (TokenClipDataset, in latent units as the
    launcher passes them), `image_folder` -> FrameListDataset (in pixel units).  raw=True makes the frame loader return
    uint8 source-size clips collated by `frames.collate_raw` for the GPU ingest.  `packed_path` (with `image_folder`) reads the
    folder's pack instead of its images (mebt_amd/packed.py): PackedFrameDataset, batches of pack rows."""

    def __init__(self, args, shuffle=True, world_size=1, rank=0, raw=False):
        super().__init__(args, shuffle=shuffle, world_size=world_size, rank=rank)
        self.raw = raw
        self._packs = {}                    # train / test -> the opened (and, resident, uploaded) pack: one upload per split

    def _dataset(self, train):
        a = self.args
        if _arg(a, "vtokens", False):
            return super()._dataset(train)
        if _arg(a, "image_folder", False) and _arg(a, "packed_path", None):
            from .packed import PackedFrameDataset
            return PackedFrameDataset(_arg(a, "data_path", None), _arg(a, "packed_path", None), _arg(a, "sequence_length", 16),
                                      resolution=_arg(a, "resolution", 128), sample_every_n_frames=_arg(a, "sample_every_n_frames", 1),
                                      train=train, latent_shape=_arg(a, "latent_shape", [1]))
        if _arg(a, "image_folder", False):
            return FrameListDataset(_arg(a, "data_path", None), _arg(a, "sequence_length", 16), resolution=_arg(a, "resolution", 128),
                                    sample_every_n_frames=_arg(a, "sample_every_n_frames", 1), train=train,
                                    latent_shape=_arg(a, "latent_shape", [1]), raw=self.raw)
        if _arg(a, "preprocessed_hdf5", False):
            raise NotImplementedError("HDF5Dataset_preprocessed (preprocessed_hdf5: True) is not available: it needs h5py and "
                                      "pixel-space HDF5 files; use image_folder: True with a frame folder, or vtokens: True")
        raise NotImplementedError("VideoDataset (video files, the reference's default branch) is not available: it needs "
                                  "torchvision's VideoClips; use image_folder: True with a frame folder, or vtokens: True")

    def _dataloader(self, train):
        ds = self._dataset(train)
        if _arg(self.args, "packed_path", None) and not hasattr(ds, "pack"):
            raise ValueError("packed_path is the pack of a frame folder: it needs image_folder (--image_folder) and no vtokens")
        if not isinstance(ds, FrameListDataset):
            return super()._dataloader(train)
        a = self.args
        sampler = ShardedSampler(len(ds), self.world_size, self.rank) if self.world_size > 1 else None
        nw = _arg(a, "num_workers", 0)
        if hasattr(ds, "pack"):
            # a packed split (mebt_amd/packed.py): nothing to decode, so the loader runs in this process; resident mode uploads the
            # split to this rank's device once and the batches carry row numbers only
            from .packed import choose_resident, collate_packed
            if train in self._packs:
                ds.pack, resident = self._packs[train]
            else:
                resident, why = choose_resident(ds.pack, _arg(a, "packed_resident", "auto"))
                print(why)
                print(f"packed frames: the loader runs in-process, data.num_workers={nw} is ignored")
                if resident:
                    ds.pack.upload(torch.device("cuda", torch.cuda.current_device()))
                self._packs[train] = (ds.pack, resident)
            return torch.utils.data.DataLoader(ds, batch_size=_arg(a, "batch_size", 6), num_workers=0, pin_memory=True, sampler=sampler,
                                               shuffle=sampler is None and self.shuffle,
                                               collate_fn=functools.partial(collate_packed, pack=ds.pack, resident=resident))
        collate = None
        if self.raw:
            from .frames import collate_raw
            collate = functools.partial(collate_raw, resolution=ds.resolution)
        return torch.utils.data.DataLoader(ds, batch_size=_arg(a, "batch_size", 6), num_workers=nw, pin_memory=True, sampler=sampler,
                                           shuffle=sampler is None and self.shuffle, persistent_workers=bool(train and nw > 0),
                                           collate_fn=collate)
