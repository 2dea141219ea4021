#!/usr/bin/env python3
"""Generate the discriminator golden vectors under tests/golden/disc/ by running the *real* reference classes
`NLayerDiscriminator` / `NLayerDiscriminator3D` and its `hinge_d_loss`, `vanilla_d_loss` and `adopt_weight` (mebt/vqgan.py, mebt/utils.py).

Runs ONLY where the reference tree is available (read-only, on the CPU).  Its Python never travels with the repository: what is committed
is data plus this script.  The reference is loaded the way tests/golden/make_golden.py does it (`install_stubs`, then stand-ins for
`mebt.modules.Codebook` / `LPIPS`, which the discriminators never touch).  The networks are built with `norm_layer=nn.BatchNorm{2,3}d`:
the default `nn.SyncBatchNorm` has the same five state-dict entries and the same arithmetic on one rank, but refuses CPU tensors in training
mode.  `VQGAN.forward` itself moves `frame_idx` to a GPU, so the GAN terms are assembled here from the reference's own networks and loss
functions in the order and with the weights of vqgan.py:118-141,156-165.

Weights are closed-form (oracle/closed_form.py; `closed_form_state_dict` below is what the tests import): He-scaled convolutions, biases
of std 0.05, BatchNorm gamma 1 + N(0, 0.1), beta N(0, 0.1), running_mean N(0, 0.2), running_var in [0.5, 1.5], num_batches_tracked 7.
Inputs are structured (`structured_clip`).  Before anything is written the maker asserts that every BatchNorm channel's batch variance is
>= 100 eps, every stage's RMS is in [0.02, 4] and float32 is within 1e-5 (of the tensor's maximum) of a float64 run of the same module.

Output (MEBT_GOLDEN_OUT overrides the directory): disc_golden.npz.  Per case c of CASES and mode m in (eval, train):
  c_m_logits, c_m_cmean{n} (per-channel means of stage n), c_m_feat{n} (the whole stage output, ndf 8 cases only), c_m_stats [L + 2, 3] =
  per stage (fp32-vs-float64 distance, fp16-twin-vs-float64 distance, max |float64|), distances relative to that maximum;
  c_train_buf_{key} the BatchNorm buffers after one training-mode call and c_train_bufstats [n_buf, 3] = (fp32-vs-float64 distance, fp16-twin-vs-float64 distance, max).
Per case g of GAN_CASES and mode m: g_m_callstats [4, L + 2, 3] (the four discriminator calls image real / fake, video real / fake),
g_m_{kind}_{feat weight}_{step}_ref [13] in the order G_KEYS + D_KEYS and ..._f64 likewise; g_frame_idx.  Also the state-dict keys and
shapes of SD_CONFIGS.

Usage:  python tests/golden/disc/make_golden_disc.py
"""
import os
import sys

sys.dont_write_bytecode = True            # never write __pycache__ into the reference tree
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import closed_form as cf

CASES = {
    "img8": dict(three_d=False, ndf=8, L=3, shape=(3, 3, 20, 12)),
    "vid8": dict(three_d=True, ndf=8, L=3, shape=(2, 3, 5, 20, 12)),
    "vid8t1": dict(three_d=True, ndf=8, L=2, shape=(2, 3, 1, 8, 6)),
    "img64": dict(three_d=False, ndf=64, L=3, shape=(2, 3, 16, 16)),
    "vid64": dict(three_d=True, ndf=64, L=3, shape=(2, 3, 4, 16, 16)),
}
GAN_CASES = {"gan8": dict(ndf=8, L=3, shape=(2, 3, 5, 20, 12)), "gan64": dict(ndf=64, L=3, shape=(2, 3, 4, 16, 16))}
SD_CONFIGS = [(8, 2), (8, 3), (64, 3), (64, 4), (64, 5)]
ITER_START = 10
GAN_CONFIGS = [(kind, gfw, step) for kind in ("hinge", "vanilla") for gfw in (0.0, 1.0) for step in (ITER_START - 1, ITER_START)]
G_KEYS = ("g_image_loss", "g_video_loss", "image_gan_feat_loss", "video_gan_feat_loss", "aeloss", "gan_feat_loss")
D_KEYS = ("logits_image_real", "logits_image_fake", "logits_video_real", "logits_video_fake", "d_image_loss", "d_video_loss", "discloss")
EPS32 = float(np.finfo(np.float32).eps) / 2       # one rounding to fp32, relative
BN_EPS = 1e-5


def gan_args(kind, gfw, image_gan_weight=1.0, video_gan_weight=1.0):
    return dict(disc_loss_type=kind, gan_feat_weight=gfw, image_gan_weight=image_gan_weight, video_gan_weight=video_gan_weight,
                discriminator_iter_start=ITER_START)


def closed_form_state_dict(ndf, n_layers, three_d, prefix="", shapes=None):
    """{key: tensor} of one network's closed-form state dict; `shapes` defaults to mebt_amd.discriminator.expected_keys"""
    if shapes is None:
        from mebt_amd.discriminator import expected_keys
        shapes = expected_keys(ndf, n_layers, three_d)
    tag = f"disc{'3d' if three_d else '2d'}.{ndf}.{n_layers}."
    sd = {}
    for k, shp in shapes.items():
        shp = tuple(shp)
        if k.endswith("num_batches_tracked"):
            sd[prefix + k] = torch.tensor(7, dtype=torch.int64)
            continue
        if k.endswith(".0.weight"):
            v = cf.pseudo_normal(tag + k, shp, std=float(np.sqrt(2.0 / np.prod(shp[1:]))))
        elif k.endswith(".0.bias"):
            v = cf.pseudo_normal(tag + k, shp, std=0.05)
        elif k.endswith(".1.weight"):
            v = 1.0 + cf.pseudo_normal(tag + k, shp, std=0.1)
        elif k.endswith(".1.bias"):
            v = cf.pseudo_normal(tag + k, shp, std=0.1)
        elif k.endswith("running_mean"):
            v = cf.pseudo_normal(tag + k, shp, std=0.2)
        elif k.endswith("running_var"):
            v = 0.5 + cf.uniform01(tag + k, shp)
        else:
            raise KeyError(k)
        sd[prefix + k] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return sd


def structured_clip(shape, variant=0):
    """float32 [B, 3, T, H, W] in [-0.5, 0.5] (a 4-D shape gives [B, 3, H, W]): gradients and a bright block that moves with the frame;
    variant 1 adds structured noise whose amplitude grows with the sample (a stand-in for a reconstruction)"""
    full = shape if len(shape) == 5 else (shape[0], shape[1], 1, shape[2], shape[3])
    B, Cc, T, H, W = full
    b, c, t, y, x = np.meshgrid(np.arange(B), np.arange(Cc), np.arange(T), np.arange(H), np.arange(W), indexing="ij")
    a = (x * (19 + 7 * b) + y * (31 + 12 * c) + 40 * c + 61 * b + 23 * t) % 256
    sq = (np.abs(x - (W // 3 + 2 * t + 3 * b) % W) < 3) & (np.abs(y - H // 2) < 3)
    a = np.where(sq, 255 - c * 60, a)
    if variant:
        amp = 30 + 25 * b
        a = np.clip(a + ((x * 7 + y * 13 + c * 29 + t * 17 + (x * y) % 11 * 5) % (2 * amp + 1)) - amp, 0, 255)
    v = torch.from_numpy((a.astype(np.float64) / 255.0 - 0.5).astype(np.float32))
    return v if len(shape) == 5 else v[:, :, 0].contiguous()


def load_reference():
    """(mebt.vqgan, mebt.utils.adopt_weight) of the reference"""
    import importlib
    sys.path.insert(0, os.path.dirname(HERE))
    import make_golden as mg
    mg.install_stubs()
    mods = sys.modules["mebt.modules"]
    mods.Codebook = getattr(mods, "Codebook", type("Codebook", (nn.Module,), {}))
    mods.LPIPS = getattr(mods, "LPIPS", type("LPIPS", (nn.Module,), {}))
    return importlib.import_module("mebt.vqgan"), importlib.import_module("mebt.utils").adopt_weight


def build(ref, ndf, L, three_d, dtype=torch.float32):
    cls, norm = (ref.NLayerDiscriminator3D, nn.BatchNorm3d) if three_d else (ref.NLayerDiscriminator, nn.BatchNorm2d)
    net = cls(3, ndf, L, norm_layer=norm)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert shapes == {k: tuple(v.shape) for k, v in cls(3, ndf, L).state_dict().items()}          # the default SyncBatchNorm: same entries
    net.load_state_dict(closed_form_state_dict(ndf, L, three_d, shapes=shapes), strict=True)
    return net.to(dtype), shapes


def dist(a, b64):
    return float((a.double() - b64).abs().max() / b64.abs().max())


def run_modes(ref, ndf, L, three_d, x):
    """per mode: fp32 (logits, feats), float64 (logits, feats), stats [L + 2, 3]; and the buffers after the training-mode call"""
    from mebt_amd.discriminator import disc_twin
    out = {}
    sd = closed_form_state_dict(ndf, L, three_d)
    for mode in ("eval", "train"):
        net32, _ = build(ref, ndf, L, three_d)
        net64, _ = build(ref, ndf, L, three_d, torch.float64)
        net32.train(mode == "train")
        net64.train(mode == "train")
        pre = {}
        hooks = [getattr(net64, f"model{n}")[1].register_forward_pre_hook(lambda m, a, n=n: pre.__setitem__(n, a[0].detach().clone()))
                 for n in range(1, L + 1)]
        with torch.no_grad():
            l32, f32 = net32(x)
            l64, f64 = net64(x.double())
            _, f16, b16 = disc_twin(sd, x, L, training=mode == "train", dtype=torch.float64, storage=torch.float16)
        for h in hooks:
            h.remove()
        red = (0, 2, 3, 4) if three_d else (0, 2, 3)
        if mode == "train":
            for n, h in pre.items():
                assert float(h.var(red, unbiased=False).min()) >= 100 * BN_EPS, (n, float(h.var(red, unbiased=False).min()))
        stats = []
        for n in range(L + 2):
            rms = float(f64[n].pow(2).mean().sqrt())
            assert 0.02 <= rms <= 4.0, (mode, n, rms)
            d32 = dist(f32[n], f64[n])
            assert d32 <= 1e-5, (mode, n, d32)
            stats.append((d32, dist(f16[n], f64[n]), float(f64[n].abs().max())))
        out[mode] = dict(f32=f32, f64=f64, stats=np.array(stats, dtype=np.float64))
        if mode == "train":
            b32, b64 = net32.state_dict(), net64.state_dict()
            keys = [k for k in b32 if k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
            out["buffers"] = {k: b32[k].clone() for k in keys}
            out["bufstats"] = np.array([(dist(b32[k], b64[k]), dist(b16[k], b64[k]), float(b64[k].abs().max())) for k in keys
                                        if not k.endswith("tracked")])
    return out


def scalar_tolerances(callstats, args, global_step, fp16):
    """Bound on |value - float64 value| for the 13 scalars (order G_KEYS + D_KEYS), from the recorded distances of the four discriminator
    calls (callstats [4, L + 2, 3]: image real, image fake, video real, video fake; per stage distance32, distance16, max).  A stage's
    element error is e = 4 * max(distance, one fp32 rounding) * max; every scalar is a mean of 1-Lipschitz functions of the logits (or of
    |a - b| of two stage outputs), so it moves by at most the e of what it reads; sums and weights carry over linearly."""
    col = 1 if fp16 else 0
    e = 4.0 * np.maximum(callstats[:, :, col], EPS32) * callstats[:, :, 2]
    ir, if_, vr, vf = (e[i, -1] for i in range(4))
    iw, vw, gfw = args["image_gan_weight"], args["video_gan_weight"], args["gan_feat_weight"]
    f = 0.0 if global_step < args["discriminator_iter_start"] else 1.0
    fi = float((e[0, :-1] + e[1, :-1]).sum()) if iw > 0 else 0.0
    fv = float((e[2, :-1] + e[3, :-1]).sum()) if vw > 0 else 0.0
    di, dv = 0.5 * (ir + if_), 0.5 * (vr + vf)
    g = [if_, vf, fi, fv, f * (iw * if_ + vw * vf), f * gfw * (fi + fv)]
    d = [ir, if_, vr, vf, di, dv, f * (iw * di + vw * dv)]
    return np.array(g + d, dtype=np.float64)


def assemble(ref, adopt_weight, calls, args, global_step):
    """the 13 logged values from the four calls' (logits, feats), with the reference's functions, in the order G_KEYS + D_KEYS"""
    (lir, pir), (lif, pif), (lvr, pvr), (lvf, pvf) = calls
    iw, vw = args["image_gan_weight"], args["video_gan_weight"]
    factor = adopt_weight(global_step, threshold=args["discriminator_iter_start"])
    g_image, g_video = -torch.mean(lif), -torch.mean(lvf)
    fw = 4.0 / (3 + 1)
    fi = sum(fw * F.l1_loss(a, b) for a, b in zip(pif[:-1], pir[:-1])) if iw > 0 else torch.zeros(())
    fv = sum(fw * F.l1_loss(a, b) for a, b in zip(pvf[:-1], pvr[:-1])) if vw > 0 else torch.zeros(())
    d_loss = ref.hinge_d_loss if args["disc_loss_type"] == "hinge" else ref.vanilla_d_loss
    di, dv = d_loss(lir, lif), d_loss(lvr, lvf)
    vals = [g_image, g_video, fi, fv, factor * (iw * g_image + vw * g_video), factor * args["gan_feat_weight"] * (fi + fv),
            lir.mean(), lif.mean(), lvr.mean(), lvf.mean(), di, dv, factor * (iw * di + vw * dv)]
    return np.array([float(v) for v in vals], dtype=np.float64)


def main():
    out_dir = os.environ.get("MEBT_GOLDEN_OUT", HERE)
    torch.set_num_threads(4)                       # fixed reduction split of the CPU convolutions on every machine
    ref, adopt_weight = load_reference()
    res = {}
    for ndf, L in SD_CONFIGS:
        for three_d in (False, True):
            _, shapes = build(ref, ndf, L, three_d)
            tag = f"sd_{ndf}_{L}_{'3d' if three_d else '2d'}"
            res[tag + "_keys"] = np.array(list(shapes.keys()))
            res[tag + "_shapes"] = np.array([list(s) + [-1] * (5 - len(s)) for s in shapes.values()], dtype=np.int64)
    for c, cfg in CASES.items():
        x = structured_clip(cfg["shape"])
        r = run_modes(ref, cfg["ndf"], cfg["L"], cfg["three_d"], x)
        red = (0, 2, 3, 4) if cfg["three_d"] else (0, 2, 3)
        for mode in ("eval", "train"):
            f32 = r[mode]["f32"]
            res[f"{c}_{mode}_logits"] = f32[-1].numpy()
            res[f"{c}_{mode}_stats"] = r[mode]["stats"]
            for n, f in enumerate(f32):
                res[f"{c}_{mode}_cmean{n}"] = f.mean(red).numpy()
                res[f"{c}_{mode}_shape{n}"] = np.array(f.shape, dtype=np.int64)
                if cfg["ndf"] == 8:
                    res[f"{c}_{mode}_feat{n}"] = f.numpy()
        for k, v in r["buffers"].items():
            res[f"{c}_train_buf_{k}"] = v.numpy()
        res[f"{c}_train_bufstats"] = r["bufstats"]
        print(c, "eval stats", r["eval"]["stats"].tolist())
    from mebt_amd.discriminator import disc_twin
    for g, cfg in GAN_CASES.items():
        ndf, L = cfg["ndf"], cfg["L"]
        x, xr = structured_clip(cfg["shape"]), structured_clip(cfg["shape"], 1)
        B, Cc, T, H, W = x.shape
        fidx = torch.from_numpy(cf.randint(g + ".frame_idx", (B,), T))
        sel = fidx.reshape(-1, 1, 1, 1, 1).repeat(1, Cc, 1, H, W)
        fr, frr = torch.gather(x, 2, sel).squeeze(2), torch.gather(xr, 2, sel).squeeze(2)
        res[f"{g}_frame_idx"] = fidx.numpy()
        sds = closed_form_state_dict(ndf, L, False), closed_form_state_dict(ndf, L, True)
        for mode in ("eval", "train"):
            calls32, calls64, stats = [], [], []
            for three_d, inp in ((False, fr), (False, frr), (True, x), (True, xr)):
                n32, _ = build(ref, ndf, L, three_d)
                n64, _ = build(ref, ndf, L, three_d, torch.float64)
                n32.train(mode == "train")
                n64.train(mode == "train")
                with torch.no_grad():
                    c32, c64 = n32(inp), n64(inp.double())
                    _, f16, _ = disc_twin(sds[three_d], inp, L, training=mode == "train", dtype=torch.float64, storage=torch.float16)
                calls32.append(c32)
                calls64.append(c64)
                stats.append([(dist(c32[1][n], c64[1][n]), dist(f16[n], c64[1][n]), float(c64[1][n].abs().max())) for n in range(L + 2)])
            res[f"{g}_{mode}_callstats"] = np.array(stats, dtype=np.float64)
            for kind, gfw, step in GAN_CONFIGS:
                a = gan_args(kind, gfw)
                tag = f"{g}_{mode}_{kind}_{int(gfw)}_{step}"
                res[tag + "_ref"] = assemble(ref, adopt_weight, calls32, a, step)
                res[tag + "_f64"] = assemble(ref, adopt_weight, calls64, a, step)
                tol = scalar_tolerances(res[f"{g}_{mode}_callstats"], a, step, False)
                assert (np.abs(res[tag + "_ref"] - res[tag + "_f64"]) <= tol).all(), (tag, res[tag + "_ref"], res[tag + "_f64"], tol)
            print(g, mode, res[f"{g}_{mode}_hinge_1_{ITER_START}_ref"].tolist())
    path = os.path.join(out_dir, "disc_golden.npz")
    np.savez_compressed(path, **res)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
