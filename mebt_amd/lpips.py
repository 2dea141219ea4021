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

`LPIPS.value_and_grad` is the perceptual term of first-stage training (`VQGAN.recon_backward` with `perceptual_weight > 0`):
the same forward with the 13 convolution outputs kept, then the backward into the reconstruction on csrc/lpips/lpips_bwd.hip.  The network
is frozen, so only data gradients exist:

  lpips_head_bwd     d(slice term)/d(reconstruction features) + the gradient from the deeper slice, masked with the features' sign
  conv2d_3x3_dgrad   the forward's kernel on flipped, transposed weights (`arrange_weight_dgrad`), the ReLU mask of the layer below fused
  maxpool_2x2_bwd    the gradient to the first maximum of each window, where it is positive
  lpips_input_bwd    factor * d / scale added into the fp32 seed video at the chosen frames

MEBT_LPIPS_CONV=own|i3d picks the forward's convolution (`value_and_grad` runs on `own` only): `own` (default) is mebt_op_conv2d_3x3, `i3d` routes the same prepared weights through
mebt_op_i3d_conv (k = (1, 3, 3)), the gather-per-tap kernel it is measured against (tools/lpips_bench.py).
"""
import ctypes as C
import math
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


def arrange_weight_dgrad(w, dtype):
    """[Cout, Cin, 3, 3] -> the weights of the data gradient as a forward convolution from Cout to Cin channels: [Cin rounded up to
    64][Kpad], K = 9 Cout as (tap, co) with co fastest and the taps flipped (dx[y, x] meets dy[y - (dh - 1), x - (dw - 1)] under
    w[:, :, dh, dw], which is tap (2 - dh, 2 - dw) of a convolution over dy): what mebt_op_conv2d_3x3_dgrad reads"""
    return arrange_weight(w.flip(2, 3).transpose(0, 1), dtype)


# max |d (sum_n LPIPS_n) / d activation| of the float64 twin on the fixture's `full` case (one 128 x 128 pair, closed-form weights):
# at the scaled input, then at each of the 13 convolution outputs in forward order (tests/golden/lpips_grad/make_golden_lpips_grad.py
# prints it).  Every slice's term is a spatial mean, so the figures fall as 1 / (H W).  Unmeasured on the real VGG weights.
GRAD_MAX_INPUT = 1.21e-5
GRAD_MAX_TABLE = (2.29e-6, 4.51e-6, 8.13e-7, 1.10e-6, 2.59e-7, 2.41e-7, 6.10e-7, 1.62e-7, 1.66e-7, 2.44e-7, 2.39e-7, 1.97e-7, 4.55e-7)
GRAD_TABLE_PIXELS = 128 * 128
GRAD_TARGET = 2.0 ** 8            # where the branch's largest stored gradient is put: 2^8 below fp16's largest finite value


def default_branch_scale(coef, H, W):
    """the power of two S_p that puts |coef| * S_p * (the largest figure of the table, carried to H x W by 1 / (H W)) at or just below
    GRAD_TARGET"""
    top = abs(float(coef)) * max(max(GRAD_MAX_TABLE), GRAD_MAX_INPUT) * GRAD_TABLE_PIXELS / float(H * W)
    if not (top > 0.0 and math.isfinite(top)):
        return 1.0
    return 2.0 ** math.floor(math.log2(GRAD_TARGET / top))


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


# ---- operators (device) --------------------------------------------------------------------------------------------------------------------
def lpips_input(video, frames, out, shift=SHIFT, scale=SCALE, dtype="f16"):
    """video fp32 [B, 3, T, H, W], frames int32 [n, 2] of (b, t) on the device, out [n, H, W, 3] of the compute dtype (written)"""
    B, _, T, H, W = video.shape
    sh, sc = (C.c_float * 3)(*[float(v) for v in shift]), (C.c_float * 3)(*[float(v) for v in scale])
    _lib.check(_lib.load().mebt_op_lpips_input(_lib.dtype_code(dtype), _lib.ptr(video), _lib.ptr(frames), _lib.ptr(out), B, T, H, W, int(frames.shape[0]),
                                               sh, sc, _lib.cur_stream()))
    return out


def conv2d_3x3(x, w, bias, out, cin, cout, dtype="f16", relu=True):
    """x [N, H, W, cin] -> out [N, H, W, cout] (written); w from `arrange_weight`, bias fp32 [cout] or None"""
    N, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    _lib.check(_lib.load().mebt_op_conv2d_3x3(_lib.dtype_code(dtype), _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), N, H, W, cin, cout, int(relu),
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
    _lib.check(_lib.load().mebt_op_maxpool_2x2(_lib.dtype_code(dtype), _lib.ptr(x), _lib.ptr(out), N, H, W, Cc, _lib.cur_stream()))
    return out


def head_scratch_bytes(n_pairs, P):
    return 8 * n_pairs * (-(-P // HEAD_ROWS))


def lpips_head(feats, w, out, n_pairs, P, Cc, scratch, layer_out=None, layer_stride=1, dtype="f16"):
    """feats [2 n_pairs, P, Cc]; out float64 [n_pairs] += the slice's term; layer_out (a view whose element n sits n * layer_stride
    doubles on) receives the term itself"""
    _lib.check(_lib.load().mebt_op_lpips_head(_lib.dtype_code(dtype), _lib.ptr(feats), _lib.ptr(w), _lib.ptr(out), _lib.ptr(layer_out), layer_stride, n_pairs,
                                              P, Cc, _lib.ptr(scratch), scratch.numel() * scratch.element_size(), _lib.cur_stream()))
    return out


def lpips_head_bwd(feats, w, d_feats, n_pairs, P, Cc, coef, add=None, dtype="f16"):
    """feats [2 n_pairs, P, Cc] -> d_feats [n_pairs, P, Cc] (written): coef * d(slice term)/d(reconstruction features) + add, masked with
    the features' sign (include/mebt_hip.h)"""
    _lib.check(_lib.load().mebt_op_lpips_head_bwd(_lib.dtype_code(dtype), _lib.ptr(feats), _lib.ptr(w), _lib.ptr(add), _lib.ptr(d_feats), n_pairs, P, Cc,
                                                  float(coef), _lib.cur_stream()))
    return d_feats


def maxpool_2x2_bwd(x, dy, dx, dtype="f16"):
    """x [N, H, W, C] (the pool's input), dy [N, H // 2, W // 2, C] -> dx [N, H, W, C] (every element written)"""
    N, H, W, Cc = (int(v) for v in x.shape)
    _lib.check(_lib.load().mebt_op_maxpool_2x2_bwd(_lib.dtype_code(dtype), _lib.ptr(x), _lib.ptr(dy), _lib.ptr(dx), N, H, W, Cc, _lib.cur_stream()))
    return dx


def conv2d_3x3_dgrad(dy, w_dgrad, y_prev, dx, cin, cout, dtype="f16"):
    """dy [N, H, W, cin] (cin: the forward's Cout) -> dx [N, H, W, cout] (written), kept where y_prev > 0 when y_prev is given;
    w_dgrad from `arrange_weight_dgrad`"""
    N, H, W = int(dy.shape[0]), int(dy.shape[1]), int(dy.shape[2])
    _lib.check(_lib.load().mebt_op_conv2d_3x3_dgrad(_lib.dtype_code(dtype), _lib.ptr(dy), _lib.ptr(w_dgrad), _lib.ptr(y_prev), _lib.ptr(dx), N, H, W, cin, cout,
                                                    _lib.cur_stream()))
    return dx


def lpips_input_bwd(d_in, frames, frames_host, seed, scale=SCALE, factor=1.0, dtype="f16"):
    """seed fp32 [B, 3, T, H, W] += factor * d_in [n, H, W, 3] / scale at the (b, t) of `frames` (int32 [n, 2] on the device;
    `frames_host` the same tensor on the CPU, checked to hold distinct pairs)"""
    B, _, T, H, W = (int(v) for v in seed.shape)
    fh = frames_host.to(torch.int32).contiguous()
    sc = (C.c_float * 3)(*[float(v) for v in scale])
    _lib.check(_lib.load().mebt_op_lpips_input_bwd(_lib.dtype_code(dtype), _lib.ptr(d_in), _lib.ptr(frames), C.c_void_p(fh.data_ptr()), _lib.ptr(seed), B, T, H,
                                                   W, int(fh.shape[0]), sc, float(factor), _lib.cur_stream()))
    return seed


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
        tdt = _lib.torch_dtype(dtype)
        self.convs = []                       # (arranged weight, bias, Cin, Cout) in forward order
        for stem, cin, cout in conv_keys():
            self.convs.append((arrange_weight(sd[stem + ".weight"].to(device), tdt), sd[stem + ".bias"].to(device, torch.float32).contiguous(),
                               cin, cout))
        self._w_raw = [sd[stem + ".weight"] for stem, _, _ in conv_keys()]       # for the data-gradient weights of `value_and_grad`
        self._wd = None
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
        bufs = [torch.empty(2 * per * H * W * 64, device=self.device, dtype=_lib.torch_dtype(self.dtype)) for _ in range(2)]
        scratch = torch.empty(max(1, head_scratch_bytes(per, H * W) // 8), device=self.device, dtype=torch.float64)
        for s in range(0, n, per):
            self._chunk(x, y, pairs[s:s + per], out[s:s + per], None if lay is None else lay[s:s + per], bufs, scratch, tap)
        return (out, lay) if layers else out

    # ---- value and gradient (training: the perceptual term of the first stage) -------------------------------------------
    def _dgrad_weights(self):
        """the 13 data-gradient weights, prepared at the first backward"""
        if self.__dict__.get("_wd") is None:
            tdt = _lib.torch_dtype(self.dtype)
            self._wd = [arrange_weight_dgrad(self._w_raw[k].to(self.device), tdt) for k in range(len(self.convs))]
        return self._wd

    @staticmethod
    def _tape_elems(H, W):
        """elements of the 13 convolution outputs of one image, and of the largest of them"""
        _, per = plan_flops(H, W)
        sizes = [h * w * cout for (_s, h, w, _ci, cout, _f) in per]
        return sum(sizes), max(sizes)

    def pairs_per_chunk_grad(self, H, W):
        es = 2 if self.dtype == "f16" else 4
        total, widest = self._tape_elems(H, W)
        # the tape of both images, the pooled input of the running slice (both images), two gradient buffers (one image), the scratch
        per_pair = es * (2 * total + 2 * widest + 2 * widest) + 8 * (-(-H * W // HEAD_ROWS))
        return max(1, self.budget_bytes // per_pair)

    def _chunk_grad(self, x, y, frames, frames_host, out, seed, coef_p, factor, scratch, flags, keep):
        m = int(frames.shape[0])
        H, W = int(x.shape[3]), int(x.shape[4])
        tdt, dev = _lib.torch_dtype(self.dtype), self.device
        # forward, every convolution output kept
        cur = torch.empty(2 * m, H, W, 3, device=dev, dtype=tdt)
        lpips_input(x, frames, cur[:m], self.shift, self.scale, self.dtype)
        lpips_input(y, frames, cur[m:], self.shift, self.scale, self.dtype)
        tape, dims, last, first = [], [], [], []
        h, w, c, k = H, W, 3, 0
        for s, ((_, idxs), cout) in enumerate(zip(SLICE_CONVS, CHANNELS)):
            if s > 0:
                nxt = torch.empty(2 * m, h // 2, w // 2, c, device=dev, dtype=tdt)
                maxpool_2x2(cur, nxt, self.dtype)
                cur, h, w = nxt, h // 2, w // 2
            first.append(k)
            for _i in idxs:
                nxt = torch.empty(2 * m, h, w, cout, device=dev, dtype=tdt)
                self._conv(cur, nxt, k)
                tape.append(nxt)
                dims.append((h, w))
                cur, c, k = nxt, cout, k + 1
            last.append(k - 1)
            lpips_head(cur, self.lins[s], out, m, h * w, c, scratch, None, 5, self.dtype)
        del cur, nxt
        # backward, slice by slice from the deepest
        wd = self._dgrad_weights()
        d_feats = [None] * 5
        add = None
        for s in reversed(range(5)):
            kl = last[s]
            h, w = dims[kl]
            cc = self.convs[kl][3]
            g = torch.empty(m, h, w, cc, device=dev, dtype=tdt)
            lpips_head_bwd(tape[kl], self.lins[s], g, m, h * w, cc, coef_p, add, self.dtype)
            if keep:
                d_feats[s] = g
            for k in range(kl, first[s] - 1, -1):
                _, _, cin, cout = self.convs[k]
                y_prev = tape[k - 1][m:] if k > first[s] else None     # below a slice's first convolution lies the pool (or the input)
                dx = torch.empty(m, h, w, cin, device=dev, dtype=tdt)
                conv2d_3x3_dgrad(g, wd[k], y_prev, dx, cout, cin, self.dtype)
                g = dx
            if s > 0:
                below = tape[last[s - 1]][m:]
                add = torch.empty(m, *below.shape[1:], device=dev, dtype=tdt)
                maxpool_2x2_bwd(below, g, add, self.dtype)
        flags.append(torch.isfinite(g).all())
        lpips_input_bwd(g, frames, frames_host, seed, self.scale, factor, self.dtype)
        return tape, d_feats

    @torch.no_grad()
    def value_and_grad(self, x, y, frames, seed, coef, grad_scale=None, keep_tape=False, flags=None):
        """The values of `__call__(x, y, frames)` (float64 [n]), and seed += coef * d(sum_n value_n)/dy.  x, y: the fp32 boundary tensors
        [B, 3, T, H, W]; `frames`: an int tensor [B] (one frame per clip) or distinct (b, t) pairs; seed: fp32, y's shape, the tensor
        mebt_op_l1_seed wrote (`coef` already carries its gradient scale).  The forward keeps the 13 convolution outputs of a chunk (a
        chunk's live bytes stay under `budget_bytes`); the backward is head_bwd at each slice output, the data gradients down the
        slice's convolutions with the ReLU masks fused, pool_bwd into the slice below, then input_bwd into the seed.  The branch runs at
        its own power-of-two scale `grad_scale` = S_p (None: `default_branch_scale(coef, H, W)`): head_bwd sees coef * S_p, input_bwd
        multiplies by 1 / S_p, so the seed receives its own scale exactly.  `flags` (a list) receives one 0-dim bool tensor per chunk:
        whether the gradient arriving at the input was finite.  keep_tape=True (tests only; one chunk): -> (values, the 13 forward
        outputs [2 n, h, w, C], the five d_feats [n, h, w, C] at scale coef * S_p)."""
        for name, t in (("x", x), ("y", y), ("seed", seed)):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 5 or t.shape[1] != 3:
                raise ValueError(f"LPIPS: {name} must be float32 [B, 3, T, H, W], got {getattr(t, 'dtype', type(t))} "
                                 f"{tuple(getattr(t, 'shape', ()))}")
            if t.device != self.device:
                raise ValueError(f"LPIPS: {name} is on {t.device}, the network on {self.device}")
        if x.shape != y.shape or seed.shape != y.shape:
            raise ValueError(f"LPIPS: shapes {tuple(x.shape)}, {tuple(y.shape)} and {tuple(seed.shape)} differ")
        if not seed.is_contiguous():
            raise ValueError("LPIPS: seed must be contiguous (it is added into in place)")
        if self.route != "own":
            raise RuntimeError("LPIPS.value_and_grad runs on mebt_op_conv2d_3x3 only (MEBT_LPIPS_CONV=own)")
        x, y = x.contiguous(), y.contiguous()
        B, _, T, H, W = (int(v) for v in x.shape)
        if H < MIN_SIZE or W < MIN_SIZE:
            raise ValueError(f"LPIPS: frames of {H} x {W}: four 2 x 2 pools need H, W >= {MIN_SIZE}")
        if frames is None:
            raise ValueError("LPIPS.value_and_grad: `frames` must name one frame per clip or distinct (b, t) pairs")
        host = self._pairs(frames, B, T)
        if len({(int(b), int(t)) for b, t in host.tolist()}) != host.shape[0]:
            raise ValueError("LPIPS.value_and_grad: the (b, t) pairs must be distinct")
        coef = float(coef)
        Sp = float(grad_scale) if grad_scale is not None else default_branch_scale(coef, H, W)
        if not (Sp > 0.0 and math.isfinite(Sp) and math.frexp(Sp)[0] == 0.5):
            raise ValueError(f"LPIPS.value_and_grad: grad_scale must be a positive power of two, got {grad_scale}")
        pairs = host.to(self.device)
        n = int(pairs.shape[0])
        out = torch.zeros(n, device=self.device, dtype=torch.float64)
        per = min(n, self.pairs_per_chunk_grad(H, W))
        if keep_tape and per < n:
            raise ValueError("LPIPS.value_and_grad: keep_tape needs the pairs to fit one chunk")
        scratch = torch.empty(max(1, head_scratch_bytes(per, H * W) // 8), device=self.device, dtype=torch.float64)
        flags = [] if flags is None else flags
        kept = None
        for s in range(0, n, per):
            kept = self._chunk_grad(x, y, pairs[s:s + per], host[s:s + per], out[s:s + per], seed, coef * Sp, 1.0 / Sp, scratch, flags, keep_tape)
        return (out, kept[0], kept[1]) if keep_tape else out


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
