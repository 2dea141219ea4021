"""Frame ingest: uint8 RGB frames -> the reference's float clip [B, 3, T, R, R], on the GPU.

The reference prepares every frame with PIL in its DataLoader workers (mebt/data.py FrameListDataset.getTensor): center
crop to the shorter side (the box comes from the clip's first frame), `Image.resize((R, R), Image.BILINEAR)`, then
`np.float32(u) / 255. - 0.5`.  Here the workers only decode (`FrameListDataset(raw=True)`) and the crop, the resize and the
normalisation run in one HIP kernel (csrc/frames/frames.hip, `mebt_op_frames_to_video`) that is bit-identical to PIL.

Pillow's 8-bit resampler (Resample.c) is integer arithmetic once its coefficients are fixed, so the host builds them exactly
as Pillow does and the kernel only multiplies and adds int32:

  per axis, in -> out:  scale = in / out, fs = max(scale, 1), support = fs (triangle filter of support 1), ss = 1 / fs
  output xx:            center = (xx + 0.5) * scale
                        xmin = max(int(center - support + 0.5), 0), n = min(int(center + support + 0.5), in) - xmin
                        w_x = tri((x + xmin - center + 0.5) * ss), x < n;  w /= sum(w) (double);  k = int(0.5 + w * 2**22)
  two passes, horizontal first, each: acc = 1 << 21; acc += sum(k * px) (int32); px' = clamp(acc >> 22, 0, 255) (uint8)

A same-size resize is a copy (the tables degenerate to one weight of 2**22).  The crop is square, so one table serves both
axes.  `resize_twin` is the numpy statement of the same algorithm: the documented definition the tests hold the tables to
(against PIL) and the kernel to; the product never computes frames on the CPU.

The real side of FVD / KVD wants the same clips as bytes: the reference turns the loader's float clip back into uint8 with
`((video + 0.5) * 255).byte()` (measure_fvd_with_numpy.py:63), which truncates and so moves some levels down by one.
`frames_to_clip_u8` (`mebt_op_frames_to_clip_u8`) is the same kernel with that 256-entry byte table (`byte_table`) in place of the
float one and the I3D path's clip layout [B, T, R, R, 3] as output; `clip_u8_twin` is its numpy statement.

The fake side of FVD / KVD starts from a decode: the sampling scripts keep `torch.clamp(img, -0.5, 0.5) + 0.5` of the first stage's
output as float32, and their writer makes bytes of it with numpy's float32 `* 255` and `.astype(np.uint8)`.  `video_to_clip_u8`
(`mebt_op_video_to_clip_u8`) writes those bytes from the decoded tensor on the device, in the same clip layout, so a sample never
visits the host as floats; `video_u8_twin` is its numpy statement.
"""
import functools
import math

import numpy as np
import torch

from . import _lib

PRECISION_BITS = 22                         # Pillow: 32 - 8 (pixel) - 2 (headroom)
MAX_LDS_BYTES = 60 * 1024                   # dynamic LDS of one workgroup: uint8 rows of the horizontal pass (FR_MAX_LDS)
MAX_TILE_ROWS = 16                          # output rows per workgroup


def _tri(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def axis_coeffs(n_in, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter: (xmin [n_out], n [n_out], k [n_out, K])
    int32, K = the widest window; taps past n have weight 0 and are never read."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    K = int(math.ceil(support)) * 2 + 1
    xmin = np.zeros(n_out, np.int32)
    cnt = np.zeros(n_out, np.int32)
    k = np.zeros((n_out, K), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        w = [_tri((x + lo - center + 0.5) * ss) for x in range(hi - lo)]
        tot = sum(w)
        for x in range(hi - lo):
            wx = w[x] / tot if tot != 0.0 else w[x]
            k[xx, x] = int(-0.5 + wx * (1 << PRECISION_BITS)) if wx < 0 else int(0.5 + wx * (1 << PRECISION_BITS))
        xmin[xx], cnt[xx] = lo, hi - lo
    K = max(1, int(cnt.max()))
    return xmin, cnt, np.ascontiguousarray(k[:, :K])


def crop_box(h, w):
    """the reference's center crop of an h x w frame: (y0, x0, side); h == w is no crop"""
    if h > w:
        return (h - w) // 2, 0, w
    if w > h:
        return 0, (w - h) // 2, h
    return 0, 0, h


def norm_table():
    """uint8 -> float32 exactly as the reference computes it: np.float32(u) / 255. then - 0.5, both in float32"""
    t = np.arange(256, dtype=np.float32)
    t /= 255.
    return t - 0.5


def byte_table():
    """uint8 -> uint8 as the reference's FVD script turns the loader's float clip back into bytes: its own expression, on CPU
    torch.  Not the identity: float32(u) / 255 - 0.5 + 0.5 can land below u / 255 and `.byte()` truncates."""
    return ((torch.from_numpy(norm_table()) + 0.5) * 255).byte().numpy()


def _pass(src, xmin, cnt, k, axis):
    """one Pillow pass along `axis` of an [H, W, C] uint8 image"""
    src = np.moveaxis(src, axis, 0).astype(np.int64)
    out = np.empty((len(xmin),) + src.shape[1:], np.int64)
    for i in range(len(xmin)):
        n = int(cnt[i])
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        acc += np.tensordot(k[i, :n].astype(np.int64), src[xmin[i]:xmin[i] + n], axes=(0, 0))
        out[i] = acc
    out = np.clip(out >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_twin(img, R):
    """numpy twin of `Image.resize((R, R), BILINEAR)` on a square uint8 [S, S, 3] image (tests only)"""
    S = img.shape[0]
    if img.shape[0] == R and img.shape[1] == R:
        return img.copy()
    xmin, cnt, k = axis_coeffs(S, R)
    xmin_w, cnt_w, k_w = axis_coeffs(img.shape[1], R)
    return _pass(_pass(img, xmin_w, cnt_w, k_w, 1), xmin, cnt, k, 0)


def clip_twin(frames, R):
    """numpy twin of the whole ingest of one clip: uint8 [T, Hs, Ws, 3] -> float32 [3, T, R, R] (tests only)"""
    y0, x0, S = crop_box(frames.shape[1], frames.shape[2])
    lut = norm_table()
    out = [lut[resize_twin(np.ascontiguousarray(f[y0:y0 + S, x0:x0 + S]), R)] for f in frames]
    return np.stack(out).transpose(3, 0, 1, 2)


def clip_u8_twin(frames, R):
    """numpy twin of the uint8 ingest of one clip: uint8 [T, Hs, Ws, 3] -> uint8 [T, R, R, 3] (tests only)"""
    y0, x0, S = crop_box(frames.shape[1], frames.shape[2])
    lut = byte_table()
    return np.stack([lut[resize_twin(np.ascontiguousarray(f[y0:y0 + S, x0:x0 + S]), R)] for f in frames])


def video_u8_twin(video, T):
    """numpy twin of `video_to_clip_u8`: float32 [B, 3, Td, H, W] -> uint8 [B, T, H, W, 3] (tests only).  The scripts' own two
    statements; fmax / fmin drop a NaN like the kernel does (NaN -> 0)."""
    x = np.asarray(video.cpu() if torch.is_tensor(video) else video, dtype=np.float32)[:, :, :T]
    with np.errstate(invalid="ignore"):
        y = np.fmin(np.fmax(x, np.float32(-0.5)), np.float32(0.5)) + np.float32(0.5)
        return np.ascontiguousarray(np.transpose((y * np.float32(255)).astype(np.uint8), (0, 2, 3, 4, 1)))


# ---- device side ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(kind, device):
    """the 256-entry table the kernels look a byte up in, "norm", "byte" or "identity", on `device`: uploaded once per device"""
    return torch.from_numpy({"norm": norm_table, "byte": byte_table, "identity": lambda: np.arange(256, dtype=np.uint8)}[kind]()).to(device)


def take_out(who, out, shape, dtype, device, any_batch=False):
    """the `out=` of an entry point: None makes the tensor, anything else must be a contiguous `dtype` tensor of `shape` on `device`
    (any_batch: of any size along the first axis)"""
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype)
    got = tuple(getattr(out, "shape", ()))
    if (not torch.is_tensor(out) or out.dtype != dtype or got[any_batch:] != tuple(shape)[any_batch:] or len(got) != len(shape)
            or out.device != device or not out.is_contiguous()):
        raise ValueError(f"{who}: `out` must be contiguous {str(dtype).split('.')[-1]} [{'*, ' * any_batch}{', '.join(map(str, shape[any_batch:]))}] "
                         f"on {device}, got {getattr(out, 'dtype', type(out))} {got} on {getattr(out, 'device', 'the host')}")
    return out


class _Plan:
    """everything the kernel needs for one (Hs, Ws, R), on one device"""

    def __init__(self, Hs, Ws, R, device):
        self.y0, self.x0, self.S = crop_box(Hs, Ws)
        self.R = R
        self.resize = self.S != R
        if self.resize:
            xmin, cnt, k = axis_coeffs(self.S, R)
            self.K = k.shape[1]
            tab = np.concatenate([xmin, cnt, k.reshape(-1)]).astype(np.int32)
            # rows per workgroup: at most MAX_TILE_ROWS, and the source rows of the widest tile must fit the LDS
            rows = MAX_TILE_ROWS
            while True:
                span = max(int(xmin[min(r + rows, R) - 1] + cnt[min(r + rows, R) - 1] - xmin[r]) for r in range(0, R, rows))
                if span * R * 3 <= MAX_LDS_BYTES or rows == 1:
                    break
                rows //= 2
            if span * R * 3 > MAX_LDS_BYTES:
                raise ValueError(f"frame ingest: {Hs}x{Ws} -> {R} needs {span} source rows of {R * 3} B in LDS for one output row")
            self.rows, self.span = rows, span
        else:
            self.K, self.rows, self.span = 0, 0, 0
            tab = np.zeros(1, np.int32)
        self.tab = torch.from_numpy(tab).to(device)


@functools.lru_cache(maxsize=None)
def plan(Hs, Ws, R, device):
    return _Plan(Hs, Ws, R, device)


def _ingest(frames, R, out, slots, u8, lut=None):
    """argument checks and launch of both outputs: float32 [B, 3, T, R, R], or (u8) uint8 [B, T, R, R, 3]; `lut` replaces the
    256-entry table of the output's dtype (`table`: "byte" or "norm")"""
    if frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3:
        raise ValueError(f"frame ingest: expected uint8 [B, T, H, W, 3], got {frames.dtype} {tuple(frames.shape)}")
    if not frames.is_cuda:
        raise ValueError("frame ingest runs on the GPU: move the frames to the device first")
    frames = frames.contiguous()
    B, T, Hs, Ws, _ = frames.shape
    p = plan(Hs, Ws, R, frames.device)
    dtype, shape = (torch.uint8, (T, R, R, 3)) if u8 else (torch.float32, (3, T, R, R))
    if out is None and slots is not None:
        raise ValueError("frame ingest: `slots` needs `out`")
    out = take_out("frame ingest", out, (B,) + shape, dtype, frames.device, any_batch=True)
    if slots is None and out.shape[0] != B:
        raise ValueError("frame ingest: `out` has another batch size and no `slots` were given")
    if slots is not None:
        if slots.dtype != torch.int32 or slots.numel() != B or slots.device != frames.device:
            raise ValueError("frame ingest: `slots` must be int32 [B] on the frames' device")
    if lut is None:
        lut = table("byte" if u8 else "norm", frames.device)
    elif lut.dtype != dtype or lut.numel() != 256 or lut.device != frames.device or not lut.is_contiguous():
        raise ValueError(f"frame ingest: `lut` must be contiguous {str(dtype).split('.')[-1]} [256] on the frames' device")
    if B == 0:
        return out
    lib = _lib.load()
    _lib.check((lib.mebt_op_frames_to_clip_u8 if u8 else lib.mebt_op_frames_to_video)(
        _lib.ptr(frames), _lib.ptr(out), B * T, T, Hs, Ws, p.y0, p.x0, p.S, R, _lib.ptr(p.tab), p.K, p.rows, p.span,
        _lib.ptr(lut), _lib.ptr(slots), int(out.shape[0]), _lib.cur_stream()))
    return out


def frames_to_video(frames, R, out=None, slots=None):
    """uint8 frames [B, T, Hs, Ws, 3] on the GPU -> the reference's float32 clip [B, 3, T, R, R].  With `out`
    [Bout, 3, T, R, R] and `slots` (int32 [B] on the device), clip i is written to out[slots[i]] (mixed-size batches)."""
    return _ingest(frames, R, out, slots, u8=False)


def frames_to_clip_u8(frames, R, out=None, slots=None, lut=None):
    """uint8 frames [B, T, Hs, Ws, 3] on the GPU -> the uint8 clip [B, T, R, R, 3] that the reference's FVD script feeds the
    I3D: `((video + 0.5) * 255).byte()` of the float clip, channels last.  `out` [Bout, T, R, R, 3] and `slots` as above.
    `lut` (uint8 [256] on the device) replaces `byte_table`: the identity gives PIL's own bytes (mebt_amd/packed.py)."""
    return _ingest(frames, R, out, slots, u8=True, lut=lut)


def video_to_clip_u8(video, T=None, out=None):
    """a decoded video, float32 [B, 3, Td, H, W] on the GPU (VQGAN.decode) -> the uint8 clip [B, T, H, W, 3] of its first `T` frames
    (default: all) that the sampling scripts save and the I3D reads: `(uint8)((clamp(x, -0.5, 0.5) + 0.5) * 255)` in float32, the
    scripts' bytes.  `out`: a contiguous uint8 [B, T, H, W, 3] tensor or view on the same device (rows of a larger store)."""
    if not torch.is_tensor(video) or video.dtype != torch.float32 or video.dim() != 5 or video.shape[1] != 3:
        raise ValueError(f"video_to_clip_u8: expected float32 [B, 3, T, H, W], got {getattr(video, 'dtype', type(video))} "
                         f"{tuple(getattr(video, 'shape', ()))}")
    if not video.is_cuda:
        raise ValueError("video_to_clip_u8 runs on the GPU: move the video to the device first")
    if not video.is_contiguous():
        raise ValueError("video_to_clip_u8: the video must be contiguous")
    B, _, Td, H, W = video.shape
    T = Td if T is None else int(T)
    if not 1 <= T <= Td:
        raise ValueError(f"video_to_clip_u8: T = {T} outside [1, {Td}]")
    out = take_out("video_to_clip_u8", out, (B, T, H, W, 3), torch.uint8, video.device)
    if B * H * W == 0:
        return out
    _lib.check(_lib.load().mebt_op_video_to_clip_u8(_lib.ptr(video), _lib.ptr(out), B, Td, T, H, W, _lib.cur_stream()))
    return out


class RawVideoBatch:
    """a collated batch of raw clips: `groups` = [(uint8 [b, T, Hs, Ws, 3], batch slots [b])], one group per source size, in
    order of first appearance; `to_video()` runs the ingest once per group into one [B, 3, T, R, R] tensor, `to_clip_u8()` into
    one uint8 [B, T, R, R, 3] tensor."""

    def __init__(self, groups, batch_size, resolution):
        self.groups, self.batch_size, self.resolution = groups, int(batch_size), int(resolution)

    @property
    def shape(self):
        T = self.groups[0][0].shape[1]
        return (self.batch_size, 3, T, self.resolution, self.resolution)

    def __len__(self):
        return self.batch_size

    def pin_memory(self):
        return RawVideoBatch([(f.pin_memory(), s.pin_memory()) for f, s in self.groups], self.batch_size, self.resolution)

    def to(self, device, non_blocking=False):
        return RawVideoBatch([(f.to(device, non_blocking=non_blocking), s.to(device, non_blocking=non_blocking))
                              for f, s in self.groups], self.batch_size, self.resolution)

    def _ingest(self, u8):
        f0 = self.groups[0][0]
        if len(self.groups) == 1 and self.groups[0][1].numel() == self.batch_size:
            return _ingest(f0, self.resolution, None, None, u8)   # one size: the collate keeps batch order
        B, C, T, R, _ = self.shape
        out = torch.empty((B, T, R, R, C) if u8 else self.shape, device=f0.device, dtype=torch.uint8 if u8 else torch.float32)
        for f, s in self.groups:
            _ingest(f, self.resolution, out, s, u8)
        return out

    def to_video(self):
        return self._ingest(False)

    def to_clip_u8(self):
        return self._ingest(True)


def collate_rest(batch, items):
    """the tail of both collates: every key of the items but `video`, stacked in batch order like the default collate"""
    for k in items[0]:
        if k != "video":
            batch[k] = torch.utils.data.default_collate([it[k] for it in items])
    return batch


def collate_raw(items, resolution):
    """collate for FrameListDataset(raw=True) items: clips that share a source size are stacked together (one ingest
    launch per size); `indices` are stacked in batch order like the default collate"""
    groups = {}
    for i, it in enumerate(items):
        v = it["video"]
        groups.setdefault(tuple(v.shape), []).append(i)
    out = []
    for key, slots in groups.items():
        out.append((torch.stack([items[i]["video"] for i in slots]), torch.tensor(slots, dtype=torch.int32)))
    return collate_rest({"video": RawVideoBatch(out, len(items), resolution)}, items)


def to_device_video(x, device, non_blocking=True):
    """a batch's `video` on the device, as the model consumes it: token grids and float clips are moved as they are, a raw
    batch is moved as uint8 and run through the ingest kernel"""
    if isinstance(x, RawVideoBatch):
        return x.to(device, non_blocking=non_blocking).to_video()
    return x.to(device, non_blocking=non_blocking)

