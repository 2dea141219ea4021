"""LPIPS — the VGG-16 perceptual distance of reference mebt/modules/lpips.py (`LPIPS.forward`), on the HIP operators of
csrc/lpips/lpips.hip.  The reference's first stage holds `self.perceptual_model = LPIPS().eval()` as a sub-module, so its checkpoints
carry the whole set under `perceptual_model.*`: 13 VGG-16 convolutions (weight + bias), five 1x1 `lin` layers and the two scaling
buffers.  `VQGAN.load_state_dict` keeps them (mebt_amd/vqgan.py); a stand-alone file of the same tensors loads with `LPIPS.load`.
Nothing here fetches weights: a file that holds only the `lin*` tensors (the public `vgg.pth`) is refused, the VGG tensors are needed.

  lpips_input    (x - shift) / scale of chosen frames of the fp32 video [B, 3, T, H, W] -> channels-last [N, H, W, 3]
  conv2d_3x3     3x3 convolution, zero padding 1, bias, ReLU: patch + halo staged in LDS, nine taps from shifted windows (MFMA)
  maxpool_2x2    nn.MaxPool2d(2, 2)
  lpips_head     normalise over channels, squared difference, `lin` weights, spatial mean -> fp64, accumulated over the five slices

`LPIPS.__call__` runs both sides of every pair as one batch of 2 n images per layer, applies the head after each slice and keeps two
ping-pong activation buffers; pairs are walked in chunks sized to a byte budget, and neither the chunk size nor the batch changes a bit
of a pair's value (the convolution's accumulation order is fixed per output, the head is reproducible).  `lpips_twin` is the plain
torch statement of the same definition: what the tests hold the kernels to; the product never calls it.

MEBT_LPIPS_CONV=own|i3d picks the convolution: `own` (default) is mebt_op_conv2d_3x3, `i3d` routes the same prepared weights through
mebt_op_i3d_conv (k = (1, 3, 3)), the gather-per-tap kernel it is measured against (tools/lpips_bench.py).
"""
import ctypes as C
import os
import types

import torch
import torch.nn.functional as F

from . import _lib

PREFIX = "perceptual_model."
# torchvision's vgg16().features indices of the convolutions of each slice (lpips.py:118-137) and their (Cin, Cout)
SLICE_CONVS = [(1, [0, 2]), (2, [5, 7]), (3, [10, 12, 14]), (4, [17, 19, 21]), (5, [24, 26, 28])]
CHANNELS = [64, 128, 256, 512, 512]
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
HEAD_ROWS = 16                    # MEBT_LPIPS_HEAD_ROWS
MIN_SIZE = 16                     # four pools must leave at least 1 x 1


def conv_keys():
    """[(state-dict stem, Cin, Cout)] of the 13 convolutions in forward order"""
    out, cin = [], 3
    for (s, idxs), cout in zip(SLICE_CONVS, CHANNELS):
        for i in idxs:
            out.append((f"net.slice{s}.{i}", cin, cout))
            cin = cout
    return out


def expected_shapes():
    """the 26 + 5 tensors a usable set must hold: {key: shape}"""
    shp = {}
    for stem, cin, cout in conv_keys():
        shp[stem + ".weight"] = (cout, cin, 3, 3)
        shp[stem + ".bias"] = (cout,)
    for k, c in enumerate(CHANNELS):
        shp[f"lin{k}.model.1.weight"] = (1, c, 1, 1)
    return shp


def extract(state_dict, what="state dict"):
    """The LPIPS tensors of a state dict, with or without the `perceptual_model.` prefix, as CPU float32 tensors under the un-prefixed
    keys; None when it holds none.  A partial set raises, naming what is missing."""
    own = {}
    shp = expected_shapes()
    pref = any(k.startswith(PREFIX) for k in state_dict)
    for k, v in state_dict.items():
        if pref and not k.startswith(PREFIX):
            continue
        name = k[len(PREFIX):] if pref else k
        if (name in shp or name in ("scaling_layer.shift", "scaling_layer.scale")) and torch.is_tensor(v):
            own[name] = v
    if not any(k in own for k in shp):
        return None
    missing = [k for k in shp if k not in own]
    if missing:
        if all(k.startswith("net.") for k in missing) and len(missing) == 26:
            raise ValueError(f"LPIPS: the {what} holds only the `lin*` tensors; the 13 VGG-16 convolutions (net.slice*.N.weight / .bias) are "
                             "needed as well — a first-stage checkpoint of the reference carries them under perceptual_model.*")
        raise ValueError(f"LPIPS: the {what} holds a partial set, missing {len(missing)} of 31 tensors: {', '.join(missing[:6])}"
                         f"{', ...' if len(missing) > 6 else ''}")
    bad = [f"{k} {tuple(own[k].shape)} (expected {s})" for k, s in shp.items() if tuple(own[k].shape) != s]
    if bad:
        raise ValueError(f"LPIPS: the {what} has tensors of the wrong shape: {', '.join(bad[:4])}")
    out = {k: own[k].detach().to("cpu", torch.float32).contiguous() for k in shp}
    for name, const in (("shift", SHIFT), ("scale", SCALE)):
        t = own.get("scaling_layer." + name)
        out["scaling_layer." + name] = (torch.tensor(const, dtype=torch.float32) if t is None
                                        else t.detach().to("cpu", torch.float32).reshape(-1).contiguous())
        if out["scaling_layer." + name].numel() != 3:
            raise ValueError(f"LPIPS: scaling_layer.{name} must hold 3 values")
    return out


def arrange_weight(w, dtype):
    """[Cout, Cin, 3, 3] -> [Cout rounded up to 64][Kpad] of `dtype`, K = 9 Cin as (tap, ci) with ci fastest, Kpad = K rounded up to
    32, zeros in the padding: what mebt_op_conv2d_3x3 and mebt_op_i3d_conv (k = (1, 3, 3)) read"""
    cout, cin = int(w.shape[0]), int(w.shape[1])
    K = 9 * cin
    wl = torch.zeros(-(-cout // 64) * 64, -(-K // 32) * 32, device=w.device, dtype=torch.float32)
    wl[:cout, :K] = w.to(torch.float32).permute(0, 2, 3, 1).reshape(cout, K)
    return wl.to(dtype).contiguous()


def plan_flops(H, W, n_images=1):
    """multiply-add FLOPs (2 per MAC) of the 13 convolutions on `n_images` images of H x W, and the per-layer list"""
    per, h, w, k = [], H, W, 0
    for (s, idxs), _ in zip(SLICE_CONVS, CHANNELS):
        if s > 1:
            h, w = h // 2, w // 2
        for _i in idxs:
            stem, cin, cout = conv_keys()[k]
            per.append((stem, h, w, cin, cout, 2 * n_images * h * w * cout * cin * 9))
            k += 1
    return sum(p[-1] for p in per), per


def _code(dtype):
    return _lib.F16 if dtype == "f16" else _lib.F32


def _tdt(dtype):
    return torch.float16 if dtype == "f16" else torch.float32


# ---- operators (device) --------------------------------------------------------------------------------------------------------------------
def lpips_input(video, frames, out, shift=SHIFT, scale=SCALE, dtype="f16"):
    """video fp32 [B, 3, T, H, W], frames int32 [n, 2] of (b, t) on the device, out [n, H, W, 3] of the compute dtype (written)"""
    B, _, T, H, W = video.shape
    sh, sc = (C.c_float * 3)(*[float(v) for v in shift]), (C.c_float * 3)(*[float(v) for v in scale])
    _lib.check(_lib.load().mebt_op_lpips_input(_code(dtype), _lib.ptr(video), _lib.ptr(frames), _lib.ptr(out), B, T, H, W, int(frames.shape[0]),
                                               sh, sc, _lib.cur_stream()))
    return out


def conv2d_3x3(x, w, bias, out, cin, cout, dtype="f16", relu=True):
    """x [N, H, W, cin] -> out [N, H, W, cout] (written); w from `arrange_weight`, bias fp32 [cout] or None"""
    N, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    _lib.check(_lib.load().mebt_op_conv2d_3x3(_code(dtype), _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), N, H, W, cin, cout, int(relu),
                                              _lib.cur_stream()))
    return out


def conv2d_3x3_i3d(x, w, bias, out, cin, cout, dtype="f16", relu=True):
    """the same convolution through mebt_op_i3d_conv with k = (1, 3, 3): the gather-per-tap route (MEBT_LPIPS_CONV=i3d, the benchmark)"""
    from .i3d import conv_launch
    N, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    cv = types.SimpleNamespace(w=w, bias=bias, cin=cin, cout=cout, widths=[cout], k=(1, 3, 3), s=(1, 1, 1), relu=relu)
    conv_launch(dtype, x, cv, N, (1, H, W), [(out, cout, 0)])
    return out


def maxpool_2x2(x, out, dtype="f16"):
    """x [N, H, W, C] -> out [N, H // 2, W // 2, C] (written)"""
    N, H, W, Cc = (int(v) for v in x.shape)
    _lib.check(_lib.load().mebt_op_maxpool_2x2(_code(dtype), _lib.ptr(x), _lib.ptr(out), N, H, W, Cc, _lib.cur_stream()))
    return out


def head_scratch_bytes(n_pairs, P):
    return 8 * n_pairs * (-(-P // HEAD_ROWS))


def lpips_head(feats, w, out, n_pairs, P, Cc, scratch, layer_out=None, layer_stride=1, dtype="f16"):
    """feats [2 n_pairs, P, Cc]; out float64 [n_pairs] += the slice's term; layer_out (a view whose element n sits n * layer_stride
    doubles on) receives the term itself"""
    _lib.check(_lib.load().mebt_op_lpips_head(_code(dtype), _lib.ptr(feats), _lib.ptr(w), _lib.ptr(out), _lib.ptr(layer_out), layer_stride, n_pairs,
                                              P, Cc, _lib.ptr(scratch), scratch.numel() * scratch.element_size(), _lib.cur_stream()))
    return out


class LPIPS:
    """The prepared network on one device.  `sd`: the un-prefixed tensors of `extract`."""

    def __init__(self, sd, dtype="f16", device="cuda"):
        if dtype not in ("f16", "f32"):
            raise ValueError(f"LPIPS: dtype must be 'f16' or 'f32', not {dtype!r}")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("mebt_amd.lpips runs on MI355X only: there is no CPU path in the product (lpips_twin is the tests' statement)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        route = os.environ.get("MEBT_LPIPS_CONV", "own")
        if route not in ("own", "i3d"):
            raise ValueError(f"MEBT_LPIPS_CONV must be 'own' or 'i3d', not {route!r}")
        self.dtype, self.device, self.route = dtype, device, route
        self.budget_bytes = 1 << 30           # live activations of one chunk (two ping-pong buffers + the head's scratch)
        tdt = _tdt(dtype)
        self.convs = []                       # (arranged weight, bias, Cin, Cout) in forward order
        for stem, cin, cout in conv_keys():
            self.convs.append((arrange_weight(sd[stem + ".weight"].to(device), tdt), sd[stem + ".bias"].to(device, torch.float32).contiguous(),
                               cin, cout))
        self.lins = [sd[f"lin{k}.model.1.weight"].to(device, torch.float32).reshape(-1).contiguous() for k in range(5)]
        self.shift = [float(v) for v in sd["scaling_layer.shift"]]
        self.scale = [float(v) for v in sd["scaling_layer.scale"]]

    @classmethod
    def from_state_dict(cls, sd, dtype="f16", device="cuda"):
        own = extract(sd)
        if own is None:
            raise ValueError("LPIPS: the state dict holds no LPIPS tensors (net.slice*.N.weight / .bias, lin*.model.1.weight)")
        return cls(own, dtype, device)

    @classmethod
    def load(cls, path, dtype="f16", device="cuda"):
        return cls(read_file(path), dtype, device)

    # ---- one chunk ----------------------------------------------------------------------------------------------------------------------
    def pairs_per_chunk(self, H, W):
        es = 2 if self.dtype == "f16" else 4
        per_pair = 2 * 2 * H * W * 64 * es + 8 * (-(-H * W // HEAD_ROWS))       # two buffers x two images at the widest layer + scratch
        return max(1, self.budget_bytes // per_pair)

    def _conv(self, x, out, k):
        w, b, cin, cout = self.convs[k]
        return (conv2d_3x3 if self.route == "own" else conv2d_3x3_i3d)(x, w, b, out, cin, cout, self.dtype)

    def _chunk(self, x, y, frames, out, lay, bufs, scratch, tap):
        m = int(frames.shape[0])
        H, W = int(x.shape[3]), int(x.shape[4])

        def view(buf, h, w, c):
            return buf[:2 * m * h * w * c].view(2 * m, h, w, c)

        src, dst = bufs
        cur = view(src, H, W, 3)
        lpips_input(x, frames, cur[:m], self.shift, self.scale, self.dtype)
        lpips_input(y, frames, cur[m:], self.shift, self.scale, self.dtype)
        h, w, c, k = H, W, 3, 0
        for s, ((_, idxs), cout) in enumerate(zip(SLICE_CONVS, CHANNELS)):
            if s > 0:
                nxt = view(dst, h // 2, w // 2, c)
                maxpool_2x2(cur, nxt, self.dtype)
                cur, src, dst, h, w = nxt, dst, src, h // 2, w // 2
            for _i in idxs:
                nxt = view(dst, h, w, cout)
                self._conv(cur, nxt, k)
                cur, src, dst, c, k = nxt, dst, src, cout, k + 1
            if tap is not None:
                tap(s, cur)
            lpips_head(cur, self.lins[s], out, m, h * w, c, scratch, None if lay is None else lay[:, s], 5, self.dtype)

    def _pairs(self, frames, B, T):
        if frames is None:
            pairs = torch.stack(torch.meshgrid(torch.arange(B), torch.arange(T), indexing="ij"), -1).reshape(-1, 2)
        else:
            f = torch.as_tensor(frames).detach().to("cpu")
            if f.is_floating_point() or f.dtype == torch.bool:
                raise ValueError("LPIPS: `frames` must hold integers")
            if f.dim() == 1:
                if f.numel() != B:
                    raise ValueError(f"LPIPS: a 1-d `frames` names one frame per clip: expected [{B}], got {tuple(f.shape)}")
                pairs = torch.stack([torch.arange(B), f.to(torch.int64)], -1)
            elif f.dim() == 2 and f.shape[1] == 2 and f.shape[0] > 0:
                pairs = f.to(torch.int64)
            else:
                raise ValueError(f"LPIPS: `frames` must be None, an int tensor [B] or a list of (b, t) pairs, got {tuple(f.shape)}")
        if pairs[:, 0].min() < 0 or pairs[:, 0].max() >= B or pairs[:, 1].min() < 0 or pairs[:, 1].max() >= T:
            raise ValueError(f"LPIPS: a frame index lies outside the {B} clips of {T} frames")
        return pairs.to(torch.int32).contiguous()

    @torch.no_grad()
    def __call__(self, x, y, frames=None, layers=False, tap=None):
        """x, y fp32 [B, 3, T, H, W] on the GPU (the VQGAN's boundary tensors) -> float64 [n_pairs] on the device: LPIPS(x[b, :, t],
        y[b, :, t]) of every chosen frame.  `frames`: an int tensor [B] (one frame per clip), None (all frames, clip-major) or an
        explicit list of (b, t).  layers=True: also the five per-slice terms [n_pairs, 5].  `tap(s, feats)`, tests only, sees every
        slice's features [2 n, h, w, C] of a chunk (the n real images, then the n reconstructions)."""
        for name, t in (("x", x), ("y", y)):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 5 or t.shape[1] != 3:
                raise ValueError(f"LPIPS: {name} must be float32 [B, 3, T, H, W], got {getattr(t, 'dtype', type(t))} "
                                 f"{tuple(getattr(t, 'shape', ()))}")
            if t.device != self.device:
                raise ValueError(f"LPIPS: {name} is on {t.device}, the network on {self.device}")
        if x.shape != y.shape:
            raise ValueError(f"LPIPS: shapes {tuple(x.shape)} and {tuple(y.shape)} differ")
        x, y = x.contiguous(), y.contiguous()
        B, _, T, H, W = (int(v) for v in x.shape)
        if H < MIN_SIZE or W < MIN_SIZE:
            raise ValueError(f"LPIPS: frames of {H} x {W}: four 2 x 2 pools need H, W >= {MIN_SIZE}")
        pairs = self._pairs(frames, B, T).to(self.device)
        n = int(pairs.shape[0])
        out = torch.zeros(n, device=self.device, dtype=torch.float64)
        lay = torch.zeros(n, 5, device=self.device, dtype=torch.float64) if layers else None
        per = min(n, self.pairs_per_chunk(H, W))
        bufs = [torch.empty(2 * per * H * W * 64, device=self.device, dtype=_tdt(self.dtype)) for _ in range(2)]
        scratch = torch.empty(max(1, head_scratch_bytes(per, H * W) // 8), device=self.device, dtype=torch.float64)
        for s in range(0, n, per):
            self._chunk(x, y, pairs[s:s + per], out[s:s + per], None if lay is None else lay[s:s + per], bufs, scratch, tap)
        return (out, lay) if layers else out


def read_file(path):
    """the LPIPS tensors of a `torch.load`-able file: a state dict, or a checkpoint with one under 'state_dict'; with or without the
    `perceptual_model.` prefix.  Loaded with weights_only=True."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and isinstance(sd.get("state_dict"), dict):
        sd = sd["state_dict"]
    if not isinstance(sd, dict):
        raise ValueError(f"LPIPS: {path} does not hold a state dict")
    own = extract(sd, what=f"file {path}")
    if own is None:
        raise ValueError(f"LPIPS: {path} holds no LPIPS tensors (net.slice*.N.weight / .bias, lin*.model.1.weight)")
    return own


# ---- the definition in plain torch (any device; tests only) ------------------------------------------------------------------------------
def twin_features(sd, a, dtype=torch.float64):
    """a [N, 3, H, W] (raw, as the VQGAN sees it) -> the five slice outputs [N, C, h, w] of lpips.py:142-155 after its ScalingLayer"""
    own = extract(sd)
    h = (a.to(dtype) - own["scaling_layer.shift"].to(dtype).view(1, 3, 1, 1)) / own["scaling_layer.scale"].to(dtype).view(1, 3, 1, 1)
    feats = []
    for s, idxs in SLICE_CONVS:
        if s > 1:
            h = F.max_pool2d(h, 2, 2)
        for i in idxs:
            h = F.relu(F.conv2d(h, own[f"net.slice{s}.{i}.weight"].to(dtype), own[f"net.slice{s}.{i}.bias"].to(dtype), padding=1))
        feats.append(h)
    return feats


def head_twin(f0, f1, w):
    """one slice's term from features [N, C, h, w] (lpips.py:88-92,158-164): float tensor [N]"""
    n0 = f0 / (torch.sqrt((f0 ** 2).sum(1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt((f1 ** 2).sum(1, keepdim=True)) + 1e-10)
    return (((n0 - n1) ** 2) * w.to(f0.dtype).view(1, -1, 1, 1)).sum(1).mean((1, 2))


def lpips_twin(sd, a, b, dtype=torch.float64):
    """a, b [N, 3, H, W] -> (value [N], per-slice terms [N, 5]) of `dtype`: LPIPS.forward of the reference in plain torch"""
    own = extract(sd)
    fa, fb = twin_features(own, a, dtype), twin_features(own, b, dtype)
    lay = torch.stack([head_twin(fa[k], fb[k], own[f"lin{k}.model.1.weight"].reshape(-1)) for k in range(5)], 1)
    return lay.sum(1), lay
