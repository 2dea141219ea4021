"""The first stage's PatchGAN discriminators — what is built of reference mebt/vqgan.py:416-520 (`NLayerDiscriminator`,
`NLayerDiscriminator3D`), :27-37 (`hinge_d_loss`, `vanilla_d_loss`) and the GAN / feature-matching arithmetic of :118-141,156-165
(DESIGN.md §9i):

- the two networks as nn.Modules that HOLD parameters and buffers under the reference's keys (`model{n}.0.weight`,
  `model{n}.1.running_var`, ...), so a state dict loads with strict=True in both directions (the reference's `nn.SyncBatchNorm` and the
  `nn.BatchNorm{2,3}d` holders here carry the same five entries), with their launch geometry (`layer_plan`) and torch's refusal of a
  training-mode BatchNorm over one value per channel.  Their `forward` is NOT built: the convolution and normalisation kernels are
  separate work, and calling it raises;
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
        raise NotImplementedError(f"{type(self).__name__}.forward is not built: this module holds the reference's parameters and buffers; the "
                                  "convolution and normalisation kernels of the discriminators are separate work (DESIGN.md §9i)")


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
