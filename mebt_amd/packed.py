"""Packed frame datasets: a frame folder decoded, cropped and resized ONCE, its clips gathered on the GPU every step.

The crop and the resize of the reference's FrameListDataset.getTensor do not depend on the random clip window, so the bytes of a
frame after them are a pure function of the frame and of `resolution`.  A pack stores those bytes for one split of one folder:

  <split>_frames.npy   uint8 [F, R, R, 3] (numpy.lib.format.open_memmap): row i = frame i after crop + resize, PIL's bytes, no table
  <split>_index.npz    version, resolution, paths [F] (row i is paths[i]: the split's image paths in the sorted order of
                       FrameListDataset.load_video_frames), list_sha1 (sha1 of the sorted lines of train.txt / test.txt), sizes
                       [F, 2] (the source (h, w) that decided the frame's crop box: the first frame of its video)

`build_pack` writes one (python -m mebt_amd.pack_frames: PNG decode in DataLoader workers, crop + resize in the frame-ingest
kernel with an identity byte table).  `PackedFrameDataset` draws the reference's random numbers in the reference's order and
returns pack rows instead of pixels; `PackedVideoBatch` turns a batch of rows into the reference's float clip or the FVD
script's uint8 clip with one gather kernel (csrc/frames/frames.hip: `mebt_op_pack_to_video`, `mebt_op_pack_to_clip_u8`), from a
pack resident in device memory or from the batch's rows copied out of the host memmap.
"""
import hashlib
import os

import numpy as np
import torch

from . import _lib, frames
from .data import FrameListDataset

VERSION = 1
MAX_FRAMES_PER_LAUNCH = 65535               # the ingest entry's limit (csrc/frames/frames.hip)
UPLOAD_CHUNK_BYTES = 256 << 20              # host -> device copies of a resident pack


def _files(out_dir, split):
    return os.path.join(out_dir, f"{split}_frames.npy"), os.path.join(out_dir, f"{split}_index.npz")


def list_lines(data_path, split):
    """the sorted lines of the split's list file, as FrameListDataset.load_video_frames reads them"""
    with open(os.path.join(data_path, f"{split}.txt"), "r") as f:
        return sorted(f.read().splitlines())


def list_sha1(data_path, split):
    return hashlib.sha1("\n".join(list_lines(data_path, split)).encode()).hexdigest()


def rebuild_command(data_path, out_dir, resolution, split):
    return f"python -m mebt_amd.pack_frames --data_path {data_path} --out {out_dir} --resolution {resolution} --split {split}"


# ---- builder ---------------------------------------------------------------------------------------------------------------
class _DecodeDataset(torch.utils.data.Dataset):
    """row -> (row, decoded uint8 [Hs, Ws, 3]); a frame whose size differs from its video's first frame raises, as raw=True does"""

    def __init__(self, paths, sizes, firsts):
        self.paths, self.sizes, self.firsts = paths, sizes, firsts

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        from .data import _open_rgb
        img = _open_rgb(self.paths[i])
        h, w = (int(v) for v in self.sizes[i])
        if (img.height, img.width) != (h, w):
            raise ValueError(f"{self.paths[i]}: {img.height}x{img.width} frame in a video of {h}x{w} frames ({self.firsts[i]})")
        return i, np.asarray(img, dtype=np.uint8)


def _videos(data_path, split, resolution):
    """every video `load_video_frames` flushes (threshold 0: group boundaries do not depend on sequence_length)"""
    ds = FrameListDataset(data_path, 0, resolution=resolution, sample_every_n_frames=1, train=split == "train", latent_shape=[1], raw=True)
    return ds.data_all


def build_pack(data_path, out_dir, resolution, splits=("train", "test"), resize=None, num_workers=0, frames_per_launch=256):
    """Write the packs of `splits`.  `resize(frames, R)`: uint8 [n, Hs, Ws, 3] numpy frames of ONE source size -> uint8 [n, R, R, 3],
    the reference's center crop and `Image.resize((R, R), BILINEAR)` (the product passes `gpu_resize`, the tests the numpy twin).
    Files are written under temporary names and renamed at the end: an interrupted build leaves no pack that loads.  Returns
    {split: frames}."""
    from .data import _open_rgb
    if resize is None:
        resize = gpu_resize
    R = int(resolution)
    if not 1 <= int(frames_per_launch) <= MAX_FRAMES_PER_LAUNCH:
        raise ValueError(f"frames_per_launch {frames_per_launch}: the ingest takes 1..{MAX_FRAMES_PER_LAUNCH} frames per launch")
    os.makedirs(out_dir, exist_ok=True)
    done = {}
    for split in splits:
        videos = _videos(data_path, split, R)
        paths = [p for v in videos for p in v]
        if not paths:
            raise ValueError(f"{data_path}/{split}.txt: no video to pack (the last video of a list is never flushed)")
        sizes = np.zeros((len(paths), 2), np.int32)
        firsts, row = [], 0
        for v in videos:                                   # the crop box of a video comes from its first frame (getTensor: video[0])
            img = _open_rgb(v[0])
            sizes[row:row + len(v)] = (img.height, img.width)
            firsts += [v[0]] * len(v)
            row += len(v)
        frames_file, index_file = _files(out_dir, split)
        tmp_frames, tmp_index = frames_file + f".tmp{os.getpid()}", index_file + f".tmp{os.getpid()}"
        try:
            rows = np.lib.format.open_memmap(tmp_frames, mode="w+", dtype=np.uint8, shape=(len(paths), R, R, 3))
            pending = {}                                   # source size -> [(row, frame)]

            def flush(key):
                items = pending.pop(key)
                out = np.asarray(resize(np.stack([f for _, f in items]), R))
                if out.dtype != np.uint8 or out.shape != (len(items), R, R, 3):
                    raise ValueError(f"resize returned {out.dtype} {out.shape} for {len(items)} frames of {key[0]}x{key[1]}")
                for (i, _), o in zip(items, out):
                    rows[i] = o

            loader = torch.utils.data.DataLoader(_DecodeDataset(paths, sizes, firsts), batch_size=16, shuffle=False, num_workers=num_workers,
                                                 collate_fn=list)
            for batch in loader:
                for i, f in batch:
                    key = f.shape[:2]
                    pending.setdefault(key, []).append((i, f))
                    if len(pending[key]) >= frames_per_launch:
                        flush(key)
            for key in list(pending):
                flush(key)
            rows.flush()
            del rows
            with open(tmp_index, "wb") as f:
                np.savez(f, version=np.int64(VERSION), resolution=np.int64(R), paths=np.array(paths), list_sha1=np.array(list_sha1(data_path, split)),
                         sizes=sizes)
            if os.path.exists(index_file):                 # a rebuild: the old index must not name the new rows
                os.remove(index_file)
            os.replace(tmp_frames, frames_file)
            os.replace(tmp_index, index_file)              # the index is what makes a pack loadable: last
        finally:
            for t in (tmp_frames, tmp_index):
                if os.path.exists(t):
                    os.remove(t)
        done[split] = len(paths)
    return done


def identity_table(device):
    """uint8 [256] identity on `device`: the ingest's byte table that leaves PIL's bytes as they are"""
    return frames.table("identity", device)


def gpu_resize(frames_u8, R, device="cuda"):
    """build_pack's `resize` on the GPU: the frame-ingest kernel with an identity table.  h == w == R is a copy."""
    n, h, w, _ = frames_u8.shape
    if h == R and w == R:
        return frames_u8.copy()
    x = torch.from_numpy(np.ascontiguousarray(frames_u8)).unsqueeze(0).to(device)
    return frames.frames_to_clip_u8(x, R, lut=identity_table(x.device))[0].cpu().numpy()


# ---- the gather ------------------------------------------------------------------------------------------------------------
def _gather(pack, ids, R, u8, out=None):
    if pack.dtype != torch.uint8 or pack.dim() != 4 or pack.shape[-1] != 3 or pack.shape[1] != pack.shape[2]:
        raise ValueError(f"pack gather: expected a uint8 pack [F, R, R, 3], got {pack.dtype} {tuple(pack.shape)}")
    if not pack.is_cuda:
        raise ValueError("pack gather runs on the GPU: move the pack to the device first")
    if pack.shape[1] != R:
        raise ValueError(f"pack gather: the pack holds {pack.shape[1]}x{pack.shape[2]} frames, not resolution {R}")
    if not pack.is_contiguous():
        raise ValueError("pack gather: the pack must be contiguous")
    if ids.dtype != torch.int64 or ids.dim() != 2 or ids.device != pack.device:
        raise ValueError(f"pack gather: `ids` must be int64 [B, T] on the pack's device, got {ids.dtype} {tuple(ids.shape)} on {ids.device}")
    ids = ids.contiguous()
    B, T = ids.shape
    shape, dtype = ((B, T, R, R, 3), torch.uint8) if u8 else ((B, 3, T, R, R), torch.float32)
    out = frames.take_out("pack gather", out, shape, dtype, pack.device)
    if B * T == 0 or pack.shape[0] == 0:
        return out
    lib = _lib.load()
    _lib.check((lib.mebt_op_pack_to_clip_u8 if u8 else lib.mebt_op_pack_to_video)(
        _lib.ptr(pack), int(pack.shape[0]), _lib.ptr(ids), _lib.ptr(out), B, T, R, _lib.ptr(frames.table("byte" if u8 else "norm", pack.device)),
        _lib.cur_stream()))
    return out


def pack_to_video(pack, ids, R, out=None):
    """pack uint8 [F, R, R, 3] and ids int64 [B, T], both on the GPU -> the reference's float32 clip [B, 3, T, R, R] of the rows
    `ids`: what `frames.frames_to_video` makes of the same bytes.  A row outside [0, F) is left unwritten: callers check their
    ids on the host first (PackedVideoBatch does)."""
    return _gather(pack, ids, R, u8=False, out=out)


def pack_to_clip_u8(pack, ids, R, out=None):
    """the same rows as the uint8 clip [B, T, R, R, 3] of the FVD real side: what `frames.frames_to_clip_u8` makes of them"""
    return _gather(pack, ids, R, u8=True, out=out)


def check_rows(ids, F):
    """host-side range check of pack rows before a gather or a memmap read: the kernel leaves a row outside [0, F) unwritten"""
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= F):
        raise IndexError(f"packed batch: frame rows {int(ids.min())}..{int(ids.max())} outside the pack's [0, {F})")


class PackedVideoBatch(frames.RawVideoBatch):
    """a batch of clips as rows of a pack, with RawVideoBatch's surface (every caller that takes a raw batch takes this one).
    `pack`: uint8 [F, R, R, 3], either the batch's own rows gathered from the host memmap (host mode: `ids` are arange, `to` moves
    the bytes) or the whole split resident on the device (resident mode: `to` moves the ids only).  `host_ids` stay on the host
    so that the range check before a launch costs no device sync."""

    def __init__(self, pack, ids, resolution, host_ids=None):
        self.pack, self.ids, self.resolution = pack, ids, int(resolution)
        self.host_ids = ids if host_ids is None else host_ids
        self.batch_size = int(ids.shape[0])

    @property
    def shape(self):
        return (self.batch_size, 3, int(self.ids.shape[1]), self.resolution, self.resolution)

    def pin_memory(self):
        pack = self.pack if self.pack.is_cuda else self.pack.pin_memory()
        return PackedVideoBatch(pack, self.ids if self.ids.is_cuda else self.ids.pin_memory(), self.resolution, self.host_ids)

    def to(self, device, non_blocking=False):
        device = torch.device(device)
        if self.pack.is_cuda and device.type == "cuda" and device.index not in (None, self.pack.device.index):
            raise ValueError(f"the pack is resident on {self.pack.device}, the batch was asked for on {device}")
        pack = self.pack if self.pack.is_cuda else self.pack.to(device, non_blocking=non_blocking)
        return PackedVideoBatch(pack, self.ids.to(pack.device if pack.is_cuda else device, non_blocking=non_blocking), self.resolution,
                                self.host_ids)

    def _ingest(self, u8):
        check_rows(self.host_ids, int(self.pack.shape[0]))
        return _gather(self.pack, self.ids, self.resolution, u8)


class Pack:
    """one split's pack, opened: `rows` (the host memmap [F, R, R, 3]), the index arrays, and after `upload` the copy on a device"""

    def __init__(self, out_dir, split):
        frames_file, index_file = _files(out_dir, split)
        if not (os.path.isfile(frames_file) and os.path.isfile(index_file)):
            raise FileNotFoundError(f"{out_dir}: no {split} pack ({os.path.basename(frames_file)}, {os.path.basename(index_file)})")
        with np.load(index_file) as z:
            self.version, self.resolution = int(z["version"]), int(z["resolution"])
            self.paths, self.list_sha1, self.sizes = [str(p) for p in z["paths"]], str(z["list_sha1"]), z["sizes"]
        self.rows = np.load(frames_file, mmap_mode="r")
        self.dir, self.split, self.device_rows = out_dir, split, None

    @property
    def nbytes(self):
        return int(self.rows.size)

    def upload(self, device):
        """the whole split to `device`, in chunks through two pinned staging buffers (the memmap is read into one while the
        other is in flight)"""
        dev = torch.empty(self.rows.shape, dtype=torch.uint8, device=device)
        step = max(1, UPLOAD_CHUNK_BYTES // max(1, int(np.prod(self.rows.shape[1:]))))
        step = min(step, max(1, len(self.rows)))
        stage = [torch.empty((step,) + tuple(self.rows.shape[1:]), dtype=torch.uint8).pin_memory() for _ in range(2)]
        done = [torch.cuda.Event(), torch.cuda.Event()]
        with torch.cuda.device(dev.device):
            for k, a in enumerate(range(0, len(self.rows), step)):
                buf, n = stage[k % 2], min(step, len(self.rows) - a)
                if k >= 2:
                    done[k % 2].synchronize()              # the copy that last read this buffer
                np.copyto(buf[:n].numpy(), self.rows[a:a + n])
                dev[a:a + n].copy_(buf[:n], non_blocking=True)
                done[k % 2].record()
            torch.cuda.synchronize()
        self.device_rows = dev
        return dev


class PackedFrameDataset(FrameListDataset):
    """FrameListDataset on a pack: the same list files, videos and random calls (`random.randint` for the start, then
    `torch.randperm`), items {'video': int64 [T] pack rows, 'indices'}.  Only train.txt / test.txt and the pack are read: the
    images may be gone.  Opening checks the pack against the list and the resolution and names the command that rebuilds it."""

    def __init__(self, data_folder, packed_path, sequence_length, resolution=64, sample_every_n_frames=1, train=True, latent_shape=[]):
        super().__init__(data_folder, sequence_length, resolution=resolution, sample_every_n_frames=sample_every_n_frames, train=train,
                         latent_shape=latent_shape, raw=True)
        split = "train" if train else "test"
        cmd = rebuild_command(data_folder, packed_path, resolution, split)
        try:
            pack = Pack(packed_path, split)
        except FileNotFoundError as e:
            raise ValueError(f"{e}; build it with: {cmd}") from None
        why = None
        if pack.version != VERSION:
            why = f"pack format version {pack.version}, this code reads version {VERSION}"
        elif pack.resolution != int(resolution):
            why = f"the pack holds resolution {pack.resolution}, the run asks for data.resolution {resolution}"
        elif pack.list_sha1 != list_sha1(data_folder, split):
            why = f"{split}.txt changed since the pack was built"
        elif pack.rows.shape != (len(pack.paths), pack.resolution, pack.resolution, 3) or pack.rows.dtype != np.uint8:
            why = f"{split}_frames.npy is {pack.rows.dtype} {pack.rows.shape}, the index lists {len(pack.paths)} frames"
        else:
            row = {p: i for i, p in enumerate(pack.paths)}
            missing = next((p for v in self.data_all for p in v if p not in row), None)
            if missing is not None:
                why = f"{missing} is not in the pack"
        if why:
            raise ValueError(f"{packed_path}: stale {split} pack: {why}; rebuild it with: {cmd}")
        self.pack = pack
        self.video_rows = [torch.tensor([row[p] for p in v], dtype=torch.int64) for v in self.data_all]

    def getTensor(self, index):
        rows = self.video_rows[index]
        start_idx, end_idx = self._clip_range(len(rows))
        return rows[start_idx:end_idx:self.sample_every_n_frames].clone()


def collate_packed(items, pack, resident):
    """collate of PackedFrameDataset items.  Resident mode: the batch carries the rows' numbers.  Host mode: the rows themselves
    are copied out of the memmap into one uint8 tensor [B * T, R, R, 3] and the ids become arange."""
    ids = torch.stack([it["video"] for it in items])
    if resident:
        video = PackedVideoBatch(pack.device_rows, ids, pack.resolution)
    else:
        check_rows(ids, len(pack.rows))
        rows = torch.from_numpy(pack.rows[ids.reshape(-1).numpy()])
        video = PackedVideoBatch(rows, torch.arange(ids.numel(), dtype=torch.int64).view_as(ids), pack.resolution)
    return frames.collate_rest({"video": video}, items)


def choose_resident(pack, setting="auto", device=None):
    """data.packed_resident: True / False, or 'auto' = resident when the split's bytes are at most half of the free device memory.
    Returns (resident, the line that says why)."""
    name = f"{pack.split} pack ({len(pack.rows)} frames, {pack.nbytes / 1e9:.3f} GB)"
    if isinstance(setting, str) and setting.lower() in ("true", "false"):
        setting = setting.lower() == "true"
    if setting is True or setting is False:
        return setting, f"{name}: {'resident in device memory' if setting else 'host memmap'} (data.packed_resident: {setting})"
    if setting != "auto":
        raise ValueError(f"data.packed_resident: {setting!r}: expected auto, True or False")
    if not torch.cuda.is_available():
        return False, f"{name}: host memmap (auto: no device visible)"
    free, _ = torch.cuda.mem_get_info(device)
    ok = pack.nbytes * 2 <= free
    return ok, (f"{name}: {'resident in device memory' if ok else 'host memmap'} (auto: {pack.nbytes / 1e9:.3f} GB "
                f"{'<=' if ok else '>'} half of the {free / 1e9:.1f} GB free)")
