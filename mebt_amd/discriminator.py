"""The first stage's PatchGAN discriminators — what is built of reference mebt/vqgan.py:416-520 (`NLayerDiscriminator`,
`NLayerDiscriminator3D`), :27-37 (`hinge_d_loss`, `vanilla_d_loss`) and the GAN / feature-matching arithmetic of :118-141,156-165
(DESIGN.md §9i):

- the two networks as nn.Modules that HOLD parameters and buffers under the reference's keys (`model{n}.0.weight`,
  `model{n}.1.running_var`, ...), so a state dict loads with strict=True in both directions (the reference's `nn.SyncBatchNorm` and the
  `nn.BatchNorm{2,3}d` holders here carry the same five entries), with their launch geometry (`layer_plan`) and torch's refusal of a
  training-mode BatchNorm over one value per channel.  A holder's own `forward` raises: the compute lives in `DiscRunner`;
- the forward on the HIP kernels of csrc/disc/disc_conv.hip (`arrange_weight`, `ingest`, `conv_stage`, `bn_act`, `head_stage`,
  `DiscRunner`): ingest to channels-last, the 4^d strided convolutions with their BatchNorm partials, the normalise + LeakyReLU pass
  and the one-channel last stage; and `gan_terms`, the reference's thirteen logged GAN values from the two runners;
- reading the two networks out of a first-stage checkpoint (`extract`, `read_file`, `load_discriminators`); `VQGAN.load_state_dict`
  keeps skipping these keys;
- on the HIP reductions of csrc/disc/disc.hip: BatchNorm batch statistics with the running-buffer update (`batch_stats`) and the loss
  values (`disc_losses`, `hinge_d_loss`, `vanilla_d_loss`, `feature_matching`), fp64 in fixed order;
- `disc_twin` and `gan_terms_twin`: the definition in plain torch, checked against the real reference classes
  (tests/golden/disc).  They are for tests; the product never calls them.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import check, ptr, cur_stream

BN_EPS, BN_MOMENTUM, SLOPE = 1e-5, 0.1, 0.2
IMAGE_PREFIX, VIDEO_PREFIX = "image_discriminator.", "video_discriminator."
BN_ROWS = 128                          # MEBT_DISC_BN_ROWS of include/mebt_hip.h

G_KEYS = ("g_image_loss", "g_video_loss", "image_gan_feat_loss", "video_gan_feat_loss", "aeloss", "gan_feat_loss")
D_KEYS = ("logits_image_real", "logits_image_fake", "logits_video_real", "logits_video_fake", "d_image_loss", "d_video_loss", "discloss")


# ---- the definition's geometry (host only) ---------------------------------------------------------------------------------------------------
def stage_channels(input_nc, ndf, n_layers):
    """[(cin, cout, stride, has_bn, has_act)] of the n_layers + 2 stages (vqgan.py:423-444)"""
    st = [(input_nc, ndf, 2, False, True)]
    nf = ndf
    for _ in range(1, n_layers):
        prev, nf = nf, min(nf * 2, 512)
        st.append((prev, nf, 2, True, True))
    prev, nf = nf, min(nf * 2, 512)
    st.append((prev, nf, 1, True, True))
    st.append((nf, 1, 1, False, False))
    return st


def layer_plan(input_nc, ndf, n_layers, dims, three_d):
    """The launch plan for an input of extents dims = (T, H, W) (T = 1 for an image): one dict per stage with cin, cout, stride, bn, act,
    kt, in_dims, out_dims (a stride-2 stage maps n -> n // 2 + 1, a stride-1 stage n -> n + 1; T only when three_d) and K = taps * cin."""
    plan = []
    for n, (cin, cout, s, bn, act) in enumerate(stage_channels(input_nc, ndf, n_layers)):
        out = tuple((d // s + 1) if (three_d or a > 0) else 1 for a, d in enumerate(dims))
        kt = 4 if three_d else 1
        plan.append(dict(stage=n, cin=cin, cout=cout, stride=s, bn=bn, act=act, kt=kt, in_dims=tuple(dims), out_dims=out, K=kt * 16 * cin))
        dims = out
    return plan


def plan_flops(plan, B):
    """multiply-add FLOPs (2 per MAC) of the plan's convolutions for a batch of B"""
    return sum(2 * B * e["out_dims"][0] * e["out_dims"][1] * e["out_dims"][2] * e["cout"] * e["K"] for e in plan)


# ---- operators (device) --------------------------------------------------------------------------------------------------------------------
def _code_of(t):
    if t.device.type != "cuda" or t.dtype not in (torch.float16, torch.float32):
        raise RuntimeError(f"the discriminator reductions take fp16 or fp32 tensors on the GPU, got {t.dtype} on {t.device}")
    return "f16" if t.dtype == torch.float16 else "f32"


def _check_buffer(name, t, dtype, numel):
    """a tensor a kernel writes through its raw pointer: dtype, size and contiguity (and, next, the device) are refused before any launch"""
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise ValueError(f"{name} must be a {dtype} tensor, got {t.dtype if torch.is_tensor(t) else type(t).__name__}")
    if t.numel() != numel or not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous with {numel} element(s), got shape {tuple(t.shape)}"
                         f"{'' if t.is_contiguous() else ' (not contiguous)'}")


def _check_on_gpu(name, t):
    if t.device.type != "cuda":
        raise RuntimeError(f"{name} must live on the GPU, got {t.device}")


def batch_stats(x, running_mean=None, running_var=None, num_batches=None, update=False):
    """x: channels-last [..., C] on the GPU -> stats fp32 [2, C] = (mean, 1 / sqrt(biased var + 1e-5)) over everything but the last axis;
    update=True moves running_mean / running_var (fp32 [C]; momentum 0.1, unbiased variance) and adds 1 to num_batches (int64, one
    element, may be None), as nn.BatchNorm does in training mode.  The buffers are written in place through their pointers, so they
    must be contiguous and on x's device.  One value per channel raises ValueError, as torch does.  Every refusal comes before any launch."""
    Cc = x.shape[-1] if torch.is_tensor(x) and x.dim() else 0
    if update and (running_mean is None or running_var is None):
        raise ValueError("update=True needs running_mean and running_var")
    bufs = [(n, t, d, c) for n, t, d, c in (("running_mean", running_mean, torch.float32, Cc), ("running_var", running_var, torch.float32, Cc),
                                            ("num_batches", num_batches, torch.int64, 1)) if t is not None]
    for name, t, want, numel in bufs:
        _check_buffer(name, t, want, numel)
    for name, t, _, _ in bufs:
        _check_on_gpu(name, t)
    dt = _code_of(x)
    if any(t is not None and t.device != x.device for t in (running_mean, running_var, num_batches)):
        raise RuntimeError(f"the BatchNorm buffers must live on x's device {x.device}")
    x = x.contiguous()
    M = x.numel() // Cc
    if M <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {list(x.shape)}")
    n_slots = -(-M // BN_ROWS)
    slots = torch.empty(Cc * 2 * n_slots, device=x.device, dtype=torch.float64)
    stats = torch.empty(2, Cc, device=x.device, dtype=torch.float32)
    lib = _lib.load()
    check(lib.mebt_op_disc_bn_partials(_lib.dtype_code(dt), ptr(x), M, Cc, ptr(slots), slots.numel() * 8, cur_stream()))
    check(lib.mebt_op_disc_bn_finish(ptr(slots), n_slots, Cc, M, ptr(stats), ptr(running_mean), ptr(running_var), ptr(num_batches), int(update),
                                     cur_stream()))
    return stats


def disc_losses(logits=None, feat_a=None, feat_b=None, out=None):
    """fp64 [6] on the device: mean l, mean relu(1 - l), mean relu(1 + l), mean softplus(-l), mean softplus(l) of `logits`, and
    mean |a - b| of the feature pair; entries not asked for are 0 (or what a caller's `out`, fp64 [6] on the same device, held).
    Tensors of one dtype (fp16 or fp32) on the GPU, any shape.  Every refusal comes before any launch."""
    ref = logits if logits is not None else feat_a
    if ref is None or (feat_a is None) != (feat_b is None):
        raise ValueError("disc_losses needs logits, or a pair of feature tensors, or both")
    if out is not None:
        _check_buffer("out", out, torch.float64, 6)
        _check_on_gpu("out", out)
    dt = _code_of(ref)
    if out is not None and out.device != ref.device:
        raise RuntimeError(f"out must live on the inputs' device {ref.device}")
    given = [t for t in (logits, feat_a, feat_b) if t is not None]
    if any(_code_of(t) != dt or t.device != ref.device for t in given):
        raise ValueError("disc_losses: every tensor must have the same dtype and device")
    if feat_a is not None and feat_a.shape != feat_b.shape:
        raise ValueError(f"feature matching needs equal shapes, got {tuple(feat_a.shape)} and {tuple(feat_b.shape)}")
    logits, feat_a, feat_b = (None if t is None else t.contiguous() for t in (logits, feat_a, feat_b))
    nl = 0 if logits is None else logits.numel()
    nf = 0 if feat_a is None else feat_a.numel()
    if out is None:
        out = torch.zeros(6, device=ref.device, dtype=torch.float64)
    lib = _lib.load()
    scratch = _lib.scratch(int(lib.mebt_disc_losses_scratch_bytes(nl, nf)), ref.device)
    check(lib.mebt_op_disc_losses(_lib.dtype_code(dt), ptr(logits), nl, ptr(feat_a), ptr(feat_b), nf, ptr(out), ptr(scratch), scratch.numel() * 8,
                                  cur_stream()))
    return out


# ---- modules ---------------------------------------------------------------------------------------------------------------------------------
class _PatchDiscriminator(nn.Module):
    three_d = False

    def __init__(self, input_nc, ndf=64, n_layers=3):
        super().__init__()
        conv, norm = (nn.Conv3d, nn.BatchNorm3d) if self.three_d else (nn.Conv2d, nn.BatchNorm2d)
        self.input_nc, self.ndf, self.n_layers = input_nc, ndf, n_layers
        for n, (cin, cout, s, bn, act) in enumerate(stage_channels(input_nc, ndf, n_layers)):
            mods = [conv(cin, cout, kernel_size=4, stride=s, padding=2)]
            if bn:
                mods.append(norm(cout, eps=BN_EPS, momentum=BN_MOMENTUM))
            if act:
                mods.append(nn.LeakyReLU(SLOPE, True))
            setattr(self, f"model{n}", nn.Sequential(*mods))
        self.compute_dtype = "f16"

    def plan(self, shape):
        """the layer plan for an input of the reference's shape [B, C, (T,) H, W]; ValueError for what the planned kernels will not take"""
        want = 5 if self.three_d else 4
        if len(shape) != want:
            raise ValueError(f"{type(self).__name__} expects a {want}-D input [B, C, {'T, ' if self.three_d else ''}H, W], got {tuple(shape)}")
        if shape[1] != self.input_nc or self.input_nc != 3:
            raise ValueError(f"{type(self).__name__}: 3 input channels are supported, got input_nc {self.input_nc} and input {tuple(shape)}")
        if self.ndf % 8 or self.ndf < 8 or self.n_layers < 1:
            raise ValueError(f"{type(self).__name__}: ndf must be a positive multiple of 8 and n_layers >= 1, got {self.ndf}, {self.n_layers}")
        if min(shape) < 1:
            raise ValueError(f"{type(self).__name__}: empty input {tuple(shape)}")
        dims = tuple(shape[2:]) if self.three_d else (1,) + tuple(shape[2:])
        return layer_plan(self.input_nc, self.ndf, self.n_layers, dims, self.three_d)

    def check_batch(self, shape):
        """the plan, after torch's own refusal of a training-mode BatchNorm over one value per channel (before any launch)"""
        plan = self.plan(shape)
        if self.training:
            for e in plan:
                if e["bn"] and shape[0] * e["out_dims"][0] * e["out_dims"][1] * e["out_dims"][2] <= 1:
                    raise ValueError(f"Expected more than 1 value per channel when training, got input size "
                                     f"{[shape[0], e['cout']] + list(e['out_dims'][0 if self.three_d else 1:])}")
        return plan

    def forward(self, input, update_running=True):
        raise NotImplementedError(f"{type(self).__name__}.forward is not built: this module holds the reference's parameters and buffers; "
                                  "DiscRunner(net) runs the forward on the HIP kernels (DESIGN.md §9i)")


class NLayerDiscriminator(_PatchDiscriminator):
    """vqgan.py:416-466 (getIntermFeat=True, no sigmoid)"""
    three_d = False


class NLayerDiscriminator3D(_PatchDiscriminator):
    """vqgan.py:471-520"""
    three_d = True


# ---- losses ------------------------------------------------------------------------------------------------------------------------------------
def adopt_weight(global_step, threshold=0, value=0.):
    """mebt/utils.py:120-124"""
    return value if global_step < threshold else 1


def hinge_d_loss(logits_real, logits_fake):
    """vqgan.py:27-31 on the HIP reduction: 0-dim fp64 on the device"""
    return 0.5 * (disc_losses(logits=logits_real)[1] + disc_losses(logits=logits_fake)[2])


def vanilla_d_loss(logits_real, logits_fake):
    """vqgan.py:33-37"""
    return 0.5 * (disc_losses(logits=logits_real)[3] + disc_losses(logits=logits_fake)[4])


def feature_matching(fake, real):
    """sum over all stage outputs but the last of feat_weights * mean |fake - real|, feat_weights = 4 / (3 + 1) (vqgan.py:131-139):
    0-dim fp64 on the device"""
    tot = torch.zeros((), device=fake[0].device, dtype=torch.float64)
    for f, r in zip(fake[:-1], real[:-1]):
        tot = tot + (4.0 / (3 + 1)) * disc_losses(feat_a=f, feat_b=r)[5]
    return tot


def _hp(args, name, default=None):
    if isinstance(args, dict):
        return args.get(name, default)
    return getattr(args, name, default)


# ---- the forward (device) ------------------------------------------------------------------------------------------------------------------
TILE_ROWS = {"f16": 128, "f32": 64}    # TileCfg<T>::BM of csrc/mfma_tile.h: rows per BatchNorm slot of the convolution's epilogue


def _dtype_name(dtype):
    if dtype in ("f16", "f32"):
        return dtype
    if dtype in (torch.float16, torch.float32):
        return "f16" if dtype == torch.float16 else "f32"
    raise ValueError(f"dtype must be 'f16' or 'f32', not {dtype!r}")


def arrange_weight(w, dtype, cin_store=None):
    """[Cout, Cin, (4,) 4, 4] -> [Npad, Kpad] of `dtype` in the kernels' K order: k = tap * cin_store + ci, tap = (dt * 4 + dh) * 4 + dw;
    cin_store (default Cin rounded up to 4) is the channel count as stored, the extra channels' columns are zero, as are the rows
    from Cout to Npad (a multiple of 64) and the columns from K to Kpad (a multiple of 32).  Host torch, any device."""
    tdt = _lib.torch_dtype(_dtype_name(dtype))
    if not torch.is_tensor(w) or w.dim() not in (4, 5) or any(k != 4 for k in w.shape[2:]):
        raise ValueError(f"arrange_weight expects [Cout, Cin, (4,) 4, 4], got {tuple(w.shape) if torch.is_tensor(w) else type(w).__name__}")
    cout, cin = int(w.shape[0]), int(w.shape[1])
    cs = -(-cin // 4) * 4 if cin_store is None else int(cin_store)
    if cs < cin or cs % 4:
        raise ValueError(f"cin_store must be a multiple of 4 and at least Cin = {cin}, got {cin_store}")
    taps = w[0, 0].numel()
    K = taps * cs
    body = torch.zeros(cout, taps, cs, dtype=tdt, device=w.device)
    body[:, :, :cin] = w.detach().reshape(cout, cin, taps).permute(0, 2, 1).to(tdt)
    out = torch.zeros(-(-cout // 64) * 64, -(-K // 32) * 32, dtype=tdt, device=w.device)
    out[:cout, :K] = body.reshape(cout, K)
    return out


def _check_map(name, x, dt=None):
    """a channels-last map [B, T, H, W, C] a kernel reads through its raw pointer"""
    if not torch.is_tensor(x) or x.dim() != 5 or not x.is_contiguous():
        raise ValueError(f"{name} must be a contiguous channels-last [B, T, H, W, C] tensor")
    code = _code_of(x)
    if dt is not None and code != dt:
        raise ValueError(f"{name} must be {dt}, got {x.dtype}")
    return code


def _nbytes(t):
    return t.numel() * t.element_size()


def ingest(x, dtype, frame_idx=None):
    """fp32 [B, 3, T, H, W] (or [B, 3, H, W]) on the GPU -> channels-last [B, To, H, W, 4] of `dtype`, fourth channel 0.  frame_idx
    (int64 [B] on x's device, each in [0, T): the caller has checked) picks that frame of every clip, To = 1 (vqgan.py:104-108)."""
    dt = _dtype_name(dtype)
    if not torch.is_tensor(x) or x.dim() not in (4, 5) or x.shape[1] != 3 or x.dtype != torch.float32:
        raise ValueError(f"ingest expects fp32 [B, 3, (T,) H, W], got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    _check_on_gpu("x", x)
    x = x.contiguous()
    B, T, H, W = (x.shape[0], 1, x.shape[2], x.shape[3]) if x.dim() == 4 else (x.shape[0], x.shape[2], x.shape[3], x.shape[4])
    if frame_idx is not None:
        _check_buffer("frame_idx", frame_idx, torch.int64, B)
        if frame_idx.device != x.device:
            raise RuntimeError(f"frame_idx must live on x's device {x.device}")
    out = torch.empty(B, 1 if frame_idx is not None else T, H, W, 4, device=x.device, dtype=_lib.torch_dtype(dt))
    check(_lib.load().mebt_op_disc_ingest(_lib.dtype_code(dt), ptr(x), ptr(frame_idx), ptr(out), _nbytes(out), B, T, H, W, cur_stream()))
    return out


def _stage_dims(x, kt, stride):
    B, Ti, Hi, Wi, Cin = x.shape
    ext = (lambda n: n // 2 + 1) if stride == 2 else (lambda n: n + 1)
    return B, Ti, Hi, Wi, Cin, (ext(Ti) if kt == 4 else 1), ext(Hi), ext(Wi)


def conv_stage(x, w, bias, kt, stride, cout, act=False, slots=False):
    """One 4^d convolution (kt 1: 4 x 4 on maps with T = 1; kt 4: 4 x 4 x 4), zero padding 2, on a channels-last map x [B, T, H, W, Cin]
    with `w` from arrange_weight and fp32 bias [cout]: the map [B, To, Ho, Wo, cout] in x's dtype, with LeakyReLU(0.2) when `act`.
    slots=True: also the fp64 BatchNorm partials [cout * 2 * n_slots] of the unrounded values, for mebt_op_disc_bn_finish."""
    dt = _check_map("x", x)
    if w.dtype != x.dtype or w.device != x.device or not w.is_contiguous() or bias.dtype != torch.float32 or bias.device != x.device \
            or bias.numel() != cout or not bias.is_contiguous():
        raise ValueError("conv_stage: w must be arrange_weight's tensor in x's dtype and bias fp32 [cout], both on x's device")
    B, Ti, Hi, Wi, Cin, To, Ho, Wo = _stage_dims(x, kt, stride)
    out = torch.empty(B, To, Ho, Wo, cout, device=x.device, dtype=x.dtype)
    sl = None
    if slots:
        sl = torch.empty(cout * 2 * -(-(B * To * Ho * Wo) // TILE_ROWS[dt]), device=x.device, dtype=torch.float64)
    check(_lib.load().mebt_op_disc_conv(_lib.dtype_code(dt), ptr(x), _nbytes(x), ptr(w), _nbytes(w), ptr(bias), ptr(out), _nbytes(out), ptr(sl),
                                        0 if sl is None else sl.numel() * 8, B, Ti, Hi, Wi, Cin, kt, stride, To, Ho, Wo, cout, int(bool(act)),
                                        cur_stream()))
    return (out, sl) if slots else out


def head_stage(x, w, bias, kt):
    """The last stage (one output channel, stride 1, no activation): [B, To, Ho, Wo, 1] in x's dtype"""
    dt = _check_map("x", x)
    if w.dtype != x.dtype or w.device != x.device or not w.is_contiguous() or bias.dtype != torch.float32 or bias.device != x.device \
            or bias.numel() != 1:
        raise ValueError("head_stage: w must be arrange_weight's tensor in x's dtype and bias fp32 [1], both on x's device")
    B, Ti, Hi, Wi, Cin, To, Ho, Wo = _stage_dims(x, kt, 1)
    out = torch.empty(B, To, Ho, Wo, 1, device=x.device, dtype=x.dtype)
    check(_lib.load().mebt_op_disc_head(_lib.dtype_code(dt), ptr(x), _nbytes(x), ptr(w), _nbytes(w), ptr(bias), ptr(out), _nbytes(out), B, Ti, Hi,
                                        Wi, Cin, kt, To, Ho, Wo, cur_stream()))
    return out


def slot_stats(slots, count, cout, running_mean=None, running_var=None, num_batches=None, update=False):
    """the convolution's slots -> stats fp32 [2, cout] = (mean, rstd) through mebt_op_disc_bn_finish, which also moves the running
    buffers (fp32 [cout], int64 [1] on the slots' device, contiguous) when `update`"""
    if count <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got {count} value(s)")
    for name, t, want, numel in (("running_mean", running_mean, torch.float32, cout), ("running_var", running_var, torch.float32, cout),
                                 ("num_batches", num_batches, torch.int64, 1)):
        if t is not None:
            _check_buffer(name, t, want, numel)
            if t.device != slots.device:
                raise RuntimeError(f"{name} must live on the GPU with the map, got {t.device}")
    if update and (running_mean is None or running_var is None):
        raise ValueError("update=True needs running_mean and running_var")
    stats = torch.empty(2, cout, device=slots.device, dtype=torch.float32)
    check(_lib.load().mebt_op_disc_bn_finish(ptr(slots), slots.numel() // (2 * cout), cout, count, ptr(stats), ptr(running_mean), ptr(running_var),
                                             ptr(num_batches), int(bool(update)), cur_stream()))
    return stats


def bn_act(x, stats, gamma, beta):
    """in place on a channels-last map: (x - mean) * rstd * gamma + beta, then LeakyReLU(0.2); stats fp32 [2, C], gamma / beta fp32 [C]"""
    _check_map("x", x)
    Cc = x.shape[-1]
    for name, t, numel in (("stats", stats, 2 * Cc), ("gamma", gamma, Cc), ("beta", beta, Cc)):
        _check_buffer(name, t, torch.float32, numel)
        if t.device != x.device:
            raise RuntimeError(f"{name} must live on the GPU with the map, got {t.device}")
    check(_lib.load().mebt_op_disc_bn_act(_lib.dtype_code(_code_of(x)), ptr(x), x.numel() // Cc, Cc, ptr(stats), ptr(gamma), ptr(beta), cur_stream()))
    return x


def _frame_index(frame_idx, B, T, device):
    """frame_idx (a sequence or an integer tensor [B]) checked against [0, T) on the host, as int64 on `device`.  A tensor that already
    lives on a GPU is read back for the check (one synchronisation); hand over a host tensor to avoid it."""
    fi = torch.as_tensor(frame_idx)
    if fi.dtype.is_floating_point or fi.dtype == torch.bool or fi.dim() != 1 or fi.numel() != B:
        raise ValueError(f"frame_idx must hold {B} integer(s), one per clip, got {tuple(fi.shape)} of {fi.dtype}")
    host = fi.detach().to("cpu", torch.int64)
    if int(host.min()) < 0 or int(host.max()) >= T:
        raise ValueError(f"frame_idx must lie in [0, {T}), got {host.tolist()[:8]}")
    return fi.to(device, torch.int64).contiguous() if fi.device.type == "cuda" else host.to(device)


class _CheckedFrames:
    """a frame index that `_frame_index` has checked and moved to the device (gan_terms checks once for its four calls)"""
    def __init__(self, dev_idx):
        self.dev_idx = dev_idx


class DiscRunner:
    """The forward of one PatchGAN holder on the HIP kernels.  Holds the arranged weights, biases and BatchNorm affine tensors on the
    holder's device in the compute dtype (`dtype`, default the holder's `compute_dtype`); `refresh()` re-derives them and runs by
    itself whenever a parameter's `_version` has moved (an optimizer step, a `load_state_dict`).  The running buffers are read from,
    and in training mode written to, the holder itself."""

    def __init__(self, net, dtype=None):
        if not isinstance(net, _PatchDiscriminator):
            raise TypeError(f"DiscRunner expects an NLayerDiscriminator or NLayerDiscriminator3D, got {type(net).__name__}")
        self.net = net
        self.dtype = _dtype_name(dtype if dtype is not None else net.compute_dtype)
        self.kt = 4 if net.three_d else 1
        self.refresh()

    def _params(self):
        return list(self.net.parameters())

    def refresh(self):
        net = self.net
        self.stages = []
        with torch.no_grad():
            for n, (cin, cout, stride, bn, act) in enumerate(stage_channels(net.input_nc, net.ndf, net.n_layers)):
                seq = getattr(net, f"model{n}")
                e = dict(cout=cout, stride=stride, bn=bn, act=act, w=arrange_weight(seq[0].weight, self.dtype, 4 if n == 0 else None),
                         bias=seq[0].bias.detach().to(torch.float32).clone().contiguous())
                if bn:
                    e["gamma"] = seq[1].weight.detach().to(torch.float32).clone().contiguous()
                    e["beta"] = seq[1].bias.detach().to(torch.float32).clone().contiguous()
                    e["norm"] = seq[1]
                self.stages.append(e)
        self._seen = [(p, p._version, p.device) for p in self._params()]

    def _stale(self):
        now = self._params()
        return len(now) != len(self._seen) or any(p is not q or p._version != v or p.device != d for p, (q, v, d) in zip(now, self._seen))

    def _eval_stats(self, st):
        """fp32 [2, C] = (running_mean, 1 / sqrt(running_var + eps)), computed in fp64; kept until a buffer's `_version` moves"""
        norm = st["norm"]
        rm, rv = norm.running_mean, norm.running_var
        held = st.get("eval_stats")
        if held is None or held[0] is not rm or held[1] is not rv or held[2] != (rm._version, rv._version, rm.device):
            with torch.no_grad():
                stats = torch.stack([rm.double(), 1.0 / torch.sqrt(rv.double() + BN_EPS)]).to(torch.float32).contiguous()
            st["eval_stats"] = held = (rm, rv, (rm._version, rv._version, rm.device), stats)
        return held[3]

    def _logical_shape(self, x, frame_idx):
        if not torch.is_tensor(x):
            raise ValueError(f"DiscRunner expects a tensor, got {type(x).__name__}")
        if frame_idx is None:
            return tuple(x.shape)
        if self.net.three_d or x.dim() != 5:
            raise ValueError("frame_idx picks one frame per clip for the image network: it needs NLayerDiscriminator and x [B, 3, T, H, W], "
                             f"got {type(self.net).__name__} and {tuple(x.shape)}")
        return tuple(x.shape[:2]) + tuple(x.shape[3:])

    def forward_buffers(self, x, frame_idx=None, update_running=None):
        """the stage outputs as the channels-last buffers [B, T, H, W, C] the kernels wrote (the last one is the logits)"""
        net = self.net
        plan = net.check_batch(self._logical_shape(x, frame_idx))          # every shape refusal and torch's ValueError: before any launch
        if x.dtype != torch.float32:
            raise ValueError(f"DiscRunner takes the fp32 input of the reference, got {x.dtype}")
        fidx = None
        if isinstance(frame_idx, _CheckedFrames):
            fidx = frame_idx.dev_idx
        elif frame_idx is not None:
            fidx = _frame_index(frame_idx, x.shape[0], x.shape[2], x.device)
        _check_on_gpu("x", x)
        held = self._params()[0]
        _check_on_gpu(f"{type(net).__name__} (DiscRunner's holder)", held)
        if held.device != x.device:
            raise RuntimeError(f"x must live on the holder's device {held.device}, got {x.device}")
        if self._stale():
            self.refresh()
        training = net.training
        update = training and update_running is not False
        h = ingest(x, self.dtype, fidx)
        bufs = []
        for e, st in zip(plan, self.stages):
            if st["cout"] == 1 and not st["act"]:
                h = head_stage(h, st["w"], st["bias"], self.kt)
            elif not st["bn"]:
                h = conv_stage(h, st["w"], st["bias"], self.kt, st["stride"], st["cout"], act=st["act"])
            else:
                norm = st["norm"]
                if training:
                    h, slots = conv_stage(h, st["w"], st["bias"], self.kt, st["stride"], st["cout"], slots=True)
                    nbt = norm.num_batches_tracked
                    stats = slot_stats(slots, h.numel() // st["cout"], st["cout"], norm.running_mean, norm.running_var,
                                       nbt.view(1) if update else None, update)
                    if update:                          # the kernel wrote them through raw pointers: say so, as an in-place op would
                        for t in (norm.running_mean, norm.running_var, nbt):
                            torch.autograd.graph.increment_version(t)
                else:
                    h = conv_stage(h, st["w"], st["bias"], self.kt, st["stride"], st["cout"])
                    stats = self._eval_stats(st)
                bn_act(h, stats, st["gamma"], st["beta"])
            bufs.append(h)
        return bufs

    def __call__(self, x, frame_idx=None, update_running=None):
        """x fp32 [B, 3, T, H, W] (video network), [B, 3, H, W] (image network), or [B, 3, T, H, W] with frame_idx (image network: frame
        frame_idx[b] of clip b) -> (logits, [stage outputs]) in the reference's logical shapes, as views of the channels-last buffers.
        The mode follows net.training; training uses batch statistics and advances the running buffers unless update_running=False."""
        bufs = self.forward_buffers(x, frame_idx, update_running)
        feats = [b.permute(0, 4, 1, 2, 3) if self.net.three_d else b[:, 0].permute(0, 3, 1, 2) for b in bufs]
        return feats[-1], feats


def gan_terms(args, image_runner, video_runner, x, x_recon, frame_idx, global_step, which, update_running=True):
    """The values the reference logs in its GAN phase (vqgan.py:118-141 for which="generator", :156-165 for "discriminator"), from the
    two runners and the HIP reductions: a dict of 0-dim fp64 device tensors under G_KEYS or D_KEYS; same contract as gan_terms_twin.
    x, x_recon fp32 [B, 3, T, H, W] on the GPU; frame_idx [B] (a host sequence or tensor: checked on the host, no synchronisation).
    Real and fake go through the networks as separate calls, each a BatchNorm batch of its own, in the reference's order; the
    real-side feature passes run only where the matching GAN weight is > 0.  The mode follows the holders' `training`."""
    if which not in ("generator", "discriminator"):
        raise ValueError(f"which must be 'generator' or 'discriminator', not {which!r}")
    for name, t in (("x", x), ("x_recon", x_recon)):
        if not torch.is_tensor(t) or t.dim() != 5:
            raise ValueError(f"gan_terms: {name} must be [B, 3, T, H, W], got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    if x.shape != x_recon.shape:
        raise ValueError(f"gan_terms: x and x_recon differ in shape, {tuple(x.shape)} and {tuple(x_recon.shape)}")
    if image_runner.net.three_d or not video_runner.net.three_d:
        raise ValueError("gan_terms expects (image runner, video runner) in this order")
    frame_shape = tuple(x.shape[:2]) + tuple(x.shape[3:])
    image_runner.net.check_batch(frame_shape)
    video_runner.net.check_batch(tuple(x.shape))
    fidx = _frame_index(frame_idx, x.shape[0], x.shape[2], x.device)
    _check_on_gpu("x", x)
    _check_on_gpu("x_recon", x_recon)
    frames = _CheckedFrames(fidx)
    iw, vw = float(_hp(args, "image_gan_weight", 1.0)), float(_hp(args, "video_gan_weight", 1.0))
    factor = adopt_weight(global_step, threshold=int(_hp(args, "discriminator_iter_start", 50000)))
    image = lambda v: image_runner.forward_buffers(v, frames, update_running)
    video = lambda v: video_runner.forward_buffers(v, None, update_running)
    if which == "generator":
        pi, pv = image(x_recon), video(x_recon)
        out = {"g_image_loss": -disc_losses(logits=pi[-1])[0], "g_video_loss": -disc_losses(logits=pv[-1])[0]}
        out["aeloss"] = factor * (iw * out["g_image_loss"] + vw * out["g_video_loss"])
        zero = torch.zeros((), device=x.device, dtype=torch.float64)
        out["image_gan_feat_loss"] = feature_matching(pi, image(x)) if iw > 0 else zero
        out["video_gan_feat_loss"] = feature_matching(pv, video(x)) if vw > 0 else zero
        out["gan_feat_loss"] = factor * float(_hp(args, "gan_feat_weight", 0.0)) * (out["image_gan_feat_loss"] + out["video_gan_feat_loss"])
        return out
    d_loss = hinge_d_loss if _hp(args, "disc_loss_type", "hinge") == "hinge" else vanilla_d_loss
    ir, vr = image(x)[-1], video(x)[-1]
    if_, vf = image(x_recon)[-1], video(x_recon)[-1]
    out = {"logits_image_real": disc_losses(logits=ir)[0], "logits_image_fake": disc_losses(logits=if_)[0],
           "logits_video_real": disc_losses(logits=vr)[0], "logits_video_fake": disc_losses(logits=vf)[0],
           "d_image_loss": d_loss(ir, if_), "d_video_loss": d_loss(vr, vf)}
    out["discloss"] = factor * (iw * out["d_image_loss"] + vw * out["d_video_loss"])
    return out


# ---- checkpoint access ---------------------------------------------------------------------------------------------------------------------
def expected_keys(ndf, n_layers, three_d, input_nc=3):
    """{key: shape} of one network's state dict"""
    shp = {}
    kk = (4, 4, 4) if three_d else (4, 4)
    for n, (cin, cout, s, bn, act) in enumerate(stage_channels(input_nc, ndf, n_layers)):
        shp[f"model{n}.0.weight"], shp[f"model{n}.0.bias"] = (cout, cin) + kk, (cout,)
        if bn:
            for name in ("weight", "bias", "running_mean", "running_var"):
                shp[f"model{n}.1.{name}"] = (cout,)
            shp[f"model{n}.1.num_batches_tracked"] = ()
    return shp


def _one_network(sd, prefix, what):
    own = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix) and torch.is_tensor(v)}
    if not own:
        return None
    stages = sorted({int(k[5:k.index(".")]) for k in own if k.startswith("model") and k[5:k.index(".")].isdigit()})
    if "model0.0.weight" not in own:
        raise ValueError(f"discriminators: the {what} holds a partial set, missing {prefix}model0.0.weight")
    w0 = own["model0.0.weight"]
    shp = expected_keys(int(w0.shape[0]), max(stages) - 1, w0.dim() == 5, int(w0.shape[1]))
    missing = [k for k in shp if k not in own]
    if missing:
        raise ValueError(f"discriminators: the {what} holds a partial set, missing {len(missing)} of {len(shp)} tensors of {prefix[:-1]}: "
                         f"{', '.join(prefix + k for k in missing[:6])}{', ...' if len(missing) > 6 else ''}")
    bad = [f"{prefix}{k} {tuple(own[k].shape)} (expected {s})" for k, s in shp.items() if tuple(own[k].shape) != s]
    if bad:
        raise ValueError(f"discriminators: the {what} has tensors of the wrong shape: {', '.join(bad[:4])}")
    return {k: own[k].detach().to("cpu").contiguous() for k in shp}


def extract(state_dict, what="state dict"):
    """(image sub-dict, video sub-dict) of a first-stage state dict, under the networks' own keys; None when it holds no
    `image_discriminator.*` / `video_discriminator.*` tensor at all.  A partial set raises and names what is missing."""
    img = _one_network(state_dict, IMAGE_PREFIX, what)
    vid = _one_network(state_dict, VIDEO_PREFIX, what)
    if img is None and vid is None:
        return None
    if img is None or vid is None:
        gone = IMAGE_PREFIX if img is None else VIDEO_PREFIX
        raise ValueError(f"discriminators: the {what} holds a partial set, missing every {gone}* tensor (first: {gone}model0.0.weight)")
    return img, vid


def _load_file(path):
    from .lightning_shim import load_checkpoint_file
    ck = load_checkpoint_file(path, map_location="cpu")
    if not isinstance(ck, dict):
        raise ValueError(f"discriminators: {path} does not hold a state dict")
    sd = ck["state_dict"] if isinstance(ck.get("state_dict"), dict) else ck
    return ck, sd


def read_file(path):
    """`extract` on a `torch.load`-able file: a state dict, or a Lightning checkpoint with one under 'state_dict'"""
    return extract(_load_file(path)[1], what=f"file {path}")


def load_discriminators(path, device, dtype="f16"):
    """(NLayerDiscriminator, NLayerDiscriminator3D) parameter holders in eval mode on `device`, `compute_dtype` = dtype ("f16" / "f32":
    what a forward will compute in; the parameters stay fp32), built from the checkpoint's hyper_parameters
    (`disc_channels`, `disc_layers`, `image_channels`) and loaded strictly; ValueError when the file holds no discriminator tensors."""
    if dtype not in ("f16", "f32"):
        raise ValueError(f"dtype must be 'f16' or 'f32', not {dtype!r}")
    ck, sd = _load_file(path)
    own = extract(sd, what=f"file {path}")
    if own is None:
        raise ValueError(f"discriminators: {path} holds no image_discriminator.* / video_discriminator.* tensors")
    hp = ck.get("hyper_parameters", {}) if isinstance(ck.get("hyper_parameters", {}), dict) else {}
    args = hp.get("args", hp)
    ndf, layers, nc = _hp(args, "disc_channels"), _hp(args, "disc_layers"), _hp(args, "image_channels", 3)
    if ndf is None or layers is None:                 # a bare state dict: the shapes say the same
        ndf, layers = int(own[0]["model0.0.weight"].shape[0]), sum(k.endswith(".0.weight") for k in own[0]) - 2
    nets = (NLayerDiscriminator(int(nc), int(ndf), int(layers)), NLayerDiscriminator3D(int(nc), int(ndf), int(layers)))
    for net, part in zip(nets, own):
        net.load_state_dict(part, strict=True)
        net.to(device).eval()
        net.compute_dtype = dtype
    return nets


# ---- the definition in plain torch (any device; tests only) -----------------------------------------------------------------------------
def disc_twin(sd, x, n_layers, training=False, dtype=torch.float64, storage=None, update=True):
    """One network's forward from its state dict `sd` on x [B, C, (T,) H, W]: (logits, [stage outputs], {updated BatchNorm buffers}).
    Arithmetic in `dtype`.  storage=torch.float16 states an fp16-storage pipeline: input, weights and every stored map are rounded
    to fp16, the batch statistics are taken before the convolution's result is rounded, the normalisation reads the rounded map."""
    three_d = x.dim() == 5
    conv = F.conv3d if three_d else F.conv2d
    rd = (lambda t: t.to(storage).to(dtype)) if storage is not None else (lambda t: t)
    h = rd(x.to(dtype))
    red = (0, 2, 3, 4) if three_d else (0, 2, 3)
    shape = (1, -1, 1, 1, 1) if three_d else (1, -1, 1, 1)
    feats, bufs = [], {}
    for n in range(n_layers + 2):
        stride = 2 if n < n_layers else 1
        h = conv(h, rd(sd[f"model{n}.0.weight"].to(dtype)), sd[f"model{n}.0.bias"].to(dtype), stride=stride, padding=2)
        if f"model{n}.1.weight" in sd:
            pre = f"model{n}.1."
            if training:
                count = h.numel() // h.shape[1]
                if count <= 1:
                    raise ValueError(f"Expected more than 1 value per channel when training, got input size {list(h.shape)}")
                mean = h.mean(red)
                var = ((h - mean.view(shape)) ** 2).mean(red)
                rstd = 1.0 / torch.sqrt(var + BN_EPS)
                if update:
                    bufs[pre + "running_mean"] = (1 - BN_MOMENTUM) * sd[pre + "running_mean"].to(dtype) + BN_MOMENTUM * mean
                    bufs[pre + "running_var"] = (1 - BN_MOMENTUM) * sd[pre + "running_var"].to(dtype) + BN_MOMENTUM * var * count / (count - 1)
                    bufs[pre + "num_batches_tracked"] = sd[pre + "num_batches_tracked"] + 1
            else:
                mean = sd[pre + "running_mean"].to(dtype)
                rstd = 1.0 / torch.sqrt(sd[pre + "running_var"].to(dtype) + BN_EPS)
            if storage is not None:
                mean, rstd = mean.to(torch.float32).to(dtype), rstd.to(torch.float32).to(dtype)
            h = (rd(h) - mean.view(shape)) * rstd.view(shape) * sd[pre + "weight"].to(dtype).view(shape) + sd[pre + "bias"].to(dtype).view(shape)
        if n < n_layers + 1:
            h = F.leaky_relu(h, SLOPE)
        h = rd(h)
        feats.append(h)
    return h, feats, bufs


def gan_terms_twin(args, image_sd, video_sd, n_layers, x, x_recon, frame_idx, global_step, which, training=False, dtype=torch.float64,
                   storage=None):
    """The values the reference logs in its GAN phase, in plain torch from the two state dicts, under its log names.  x, x_recon
    [B, 3, T, H, W]; frame_idx int [B], drawn by the caller (vqgan.py:104); args carries image_gan_weight, video_gan_weight,
    gan_feat_weight, discriminator_iter_start and disc_loss_type.  which="generator": vqgan.py:118-141 (the real sides only where the
    matching GAN weight is > 0); which="discriminator": vqgan.py:156-165.  BatchNorm buffers are read, not advanced."""
    iw, vw = float(_hp(args, "image_gan_weight", 1.0)), float(_hp(args, "video_gan_weight", 1.0))
    disc_factor = adopt_weight(global_step, threshold=int(_hp(args, "discriminator_iter_start", 50000)))
    B, Cc, T, H, W = x.shape
    sel = torch.as_tensor(frame_idx).reshape(-1, 1, 1, 1, 1).repeat(1, Cc, 1, H, W)
    frames, frames_recon = torch.gather(x, 2, sel).squeeze(2), torch.gather(x_recon, 2, sel).squeeze(2)
    image = lambda v: disc_twin(image_sd, v, n_layers, training, dtype, storage)[:2]
    video = lambda v: disc_twin(video_sd, v, n_layers, training, dtype, storage)[:2]
    l1 = lambda a, b: (a - b).abs().mean()
    if which == "generator":
        li, pi = image(frames_recon)
        lv, pv = video(x_recon)
        out = {"g_image_loss": -li.mean(), "g_video_loss": -lv.mean()}
        out["aeloss"] = disc_factor * (iw * out["g_image_loss"] + vw * out["g_video_loss"])
        zero = torch.zeros((), dtype=dtype)
        out["image_gan_feat_loss"] = sum(l1(a, b) for a, b in zip(pi[:-1], image(frames)[1][:-1])) if iw > 0 else zero
        out["video_gan_feat_loss"] = sum(l1(a, b) for a, b in zip(pv[:-1], video(x)[1][:-1])) if vw > 0 else zero
        out["gan_feat_loss"] = disc_factor * float(_hp(args, "gan_feat_weight", 0.0)) * (out["image_gan_feat_loss"] + out["video_gan_feat_loss"])
        return out
    hinge = _hp(args, "disc_loss_type", "hinge") == "hinge"
    d_loss = (lambda r, f: 0.5 * (F.relu(1. - r).mean() + F.relu(1. + f).mean())) if hinge else \
        (lambda r, f: 0.5 * (F.softplus(-r).mean() + F.softplus(f).mean()))
    ir, vr, if_, vf = image(frames)[0], video(x)[0], image(frames_recon)[0], video(x_recon)[0]
    out = {"logits_image_real": ir.mean(), "logits_image_fake": if_.mean(), "logits_video_real": vr.mean(), "logits_video_fake": vf.mean(),
           "d_image_loss": d_loss(ir, if_), "d_video_loss": d_loss(vr, vf)}
    out["discloss"] = disc_factor * (iw * out["d_image_loss"] + vw * out["d_video_loss"])
    return out
