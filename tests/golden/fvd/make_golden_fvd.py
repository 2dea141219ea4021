#!/usr/bin/env python3
"""Generate the FVD / KVD golden vectors under tests/golden/fvd/ by running the *real* reference I3D and FVD code.

Runs ONLY where the reference tree is available (read-only; MEBT_REFERENCE, default /root/reference).  Its Python never travels
with the repository: what is committed is data plus this script.  The reference's `mebt/__init__.py` pulls in packages this
project does not ship, so `mebt` and `mebt.fvd` are registered as empty namespace packages whose __path__ points at the reference
dirs, and `pytorch_i3d.py` / `fvd.py` are loaded with `spec_from_file_location` (pytorch_i3d first: fvd.py imports it by name).

Weights are closed-form (oracle/closed_form.py, import only): He-scaled pseudo-normal convolution weights, BatchNorm gamma near 1,
small beta / running mean, running variance in [0.75, 1.25].  The network is checked not to be degenerate (every endpoint's RMS in
[0.1, 10], distinct logits per clip) before anything is written.

Outputs (MEBT_GOLDEN_OUT overrides the directory):
  i3d_golden.npz  structured uint8 clips (3 x 16 x 48 x 64, 2 x 12 x 40 x 56), their reference logits, per-endpoint output shapes
                  and per-channel means of clip 0, the state-dict keys and shapes
  fvd_golden.npz  two closed-form embedding sets (N >= 2 d) and the reference's frechet_distance (on float64 and on float32
                  tensors) / polynomial_mmd on them

Usage:  python tests/golden/fvd/make_golden_fvd.py
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True            # never write __pycache__ into the reference tree
REF = os.environ.get("MEBT_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from oracle import closed_form as cf

CLIP_SETS = {"a": (3, 16, 48, 64), "b": (2, 12, 40, 56)}
FVD_N, FVD_D = 96, 32                     # embedding sets for the FVD / KVD scalars: N >= 2 d


def load_reference():
    for name, sub in (("mebt", "mebt"), ("mebt.fvd", "mebt/fvd")):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = [os.path.join(REF, sub)]
            sys.modules[name] = m
    mods = {}
    for name in ("pytorch_i3d", "fvd"):
        spec = importlib.util.spec_from_file_location(f"mebt.fvd.{name}", os.path.join(REF, "mebt", "fvd", f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"mebt.fvd.{name}"] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods["pytorch_i3d"], mods["fvd"]


def closed_form_state_dict(shapes):
    """{name: shape} -> {name: tensor}: the closed-form I3D weights shared by this script and the tests"""
    sd = {}
    for k, shp in shapes.items():
        shp = tuple(shp)
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(0, dtype=torch.int64)
            continue
        if k.endswith("conv3d.weight"):
            fan_in = int(np.prod(shp[1:]))
            gain = 1.0 if k.startswith("logits.") else 2.0
            v = cf.pseudo_normal(k, shp, std=float(np.sqrt(gain / fan_in)))
        elif k.endswith("bn.weight"):
            v = (1.0 + cf.pseudo_normal(k, shp, std=0.05)).astype(np.float32)
        elif k.endswith("bn.running_var"):
            v = (0.75 + 0.5 * cf.uniform01(k, shp)).astype(np.float32)
        elif k.endswith("bn.running_mean") or k.endswith("bn.bias"):
            v = cf.pseudo_normal(k, shp, std=0.05)
        elif k.endswith("conv3d.bias"):
            v = cf.pseudo_normal(k, shp, std=0.1)
        else:
            raise KeyError(k)
        sd[k] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return sd


def structured_clips(tag, shape):
    """uint8 [N, T, H, W, 3]: moving gradients and a bright square per clip (exact integer arithmetic)"""
    N, T, H, W = shape
    n, t, y, x, c = np.meshgrid(np.arange(N), np.arange(T), np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    v = (x * (3 + n) + y * (5 + 2 * c) + t * (7 + 3 * n) + 40 * c + 61 * n) % 256
    sq = (np.abs(x - (W // 3 + 2 * t + 5 * n) % W) < 6) & (np.abs(y - (H // 2 + t) % H) < 5)
    v = np.where(sq, 255 - c * 60, v)
    return v.astype(np.uint8)


def endpoint_outputs(model, x):
    """run the reference forward endpoint by endpoint: {endpoint: output [B, C, T, H, W]}"""
    out = {}
    for ep in model.VALID_ENDPOINTS:
        if ep in model.end_points:
            x = model._modules[ep](x)
            out[ep] = x
    return out


def main():
    out_dir = os.environ.get("MEBT_GOLDEN_OUT", HERE)
    torch.set_num_threads(4)                       # fixed reduction split of the CPU convolutions on every machine
    pti3d, fvd = load_reference()
    model = pti3d.InceptionI3d(400, in_channels=3)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(closed_form_state_dict(shapes), strict=True)
    model.eval()
    res = {"sd_keys": np.array(list(shapes.keys())),
           "sd_shapes": np.array([list(s) + [-1] * (5 - len(s)) for s in shapes.values()], dtype=np.int64)}
    with torch.no_grad():
        for tag, shp in CLIP_SETS.items():
            clips = structured_clips(tag, shp)
            x = fvd.preprocess(clips, fvd.TARGET_RESOLUTION)
            logits = model(x)
            eps = endpoint_outputs(model, x[:1])
            names = list(eps)
            for ep, y in eps.items():
                rms = float(y.pow(2).mean().sqrt())
                assert 0.1 <= rms <= 10.0, (tag, ep, rms)
            lg = logits.numpy()
            assert np.isfinite(lg).all()
            d = np.abs(lg[:, None, :] - lg[None, :, :]).max(-1)
            assert (d + np.eye(len(lg)) * 1e9).min() > 1e-3 * np.abs(lg).max(), ("logits not distinct across clips", d)
            res[f"clips_{tag}"] = clips
            res[f"logits_{tag}"] = lg.astype(np.float32)
            res[f"endpoints_{tag}"] = np.array(names)
            res[f"endpoint_shapes_{tag}"] = np.array([list(eps[n].shape[1:]) for n in names], dtype=np.int64)   # [C, T, H, W]
            res[f"endpoint_means_{tag}"] = np.concatenate([eps[n][0].mean(dim=(1, 2, 3)).numpy() for n in names]).astype(np.float32)
    np.savez_compressed(os.path.join(out_dir, "i3d_golden.npz"), **res)

    # FVD / KVD scalars on two closed-form embedding sets (correlated features, different means / scales)
    base = cf.pseudo_normal("fvd_mix", (FVD_D, FVD_D), std=1.0).astype(np.float64)
    e1 = cf.pseudo_normal("fvd_x1", (FVD_N, FVD_D), std=1.0).astype(np.float64) @ base
    e2 = (cf.pseudo_normal("fvd_x2", (FVD_N, FVD_D), std=1.0).astype(np.float64) @ (0.8 * base)) + 0.3
    e1, e2 = e1.astype(np.float32), e2.astype(np.float32)
    # the reference's functions on float64 tensors (its formula), and on float32 tensors as its scripts call them
    fd = float(fvd.frechet_distance(torch.from_numpy(e1).double(), torch.from_numpy(e2).double()))
    fd32 = float(fvd.frechet_distance(torch.from_numpy(e1), torch.from_numpy(e2)))
    kd = float(fvd.polynomial_mmd(e1.astype(np.float64), e2.astype(np.float64)))
    np.savez_compressed(os.path.join(out_dir, "fvd_golden.npz"), emb1=e1, emb2=e2, fvd=np.float64(fd), fvd_f32=np.float64(fd32),
                        kvd=np.float64(kd))
    print(f"wrote {out_dir}: fvd {fd:.6f} kvd {kd:.6f}")


if __name__ == "__main__":
    main()
