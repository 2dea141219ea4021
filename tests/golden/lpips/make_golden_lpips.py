#!/usr/bin/env python3
"""Generate the LPIPS golden vectors under tests/golden/lpips/ by running the *real* reference module mebt/modules/lpips.py.

Runs ONLY where the reference tree is available (read-only; MEBT_REFERENCE, default /root/reference).  Its Python never travels with
the repository: what is committed is data plus this script.  `lpips.py` is loaded with `spec_from_file_location`.  Stand-ins are for
third-party modules only: a `torchvision.models.vgg16` that builds the standard `features` Sequential (cfg 64,64,M,128,128,M,256,256,
256,M,512,512,512,M,512,512,512,M; the reference slices it by index), empty `requests` / `tqdm` when they are not installed, and
`LPIPS.load_from_pretrained` replaced by a no-op, since it would download.

Weights are closed-form (oracle/closed_form.py, import only; `closed_form_state_dict` below is what the tests import): He-scaled
pseudo-normal convolution weights, biases of std 0.05, `lin` weights |N(0, 1)| * 4 / C (the real ones are non-negative).  The network is
checked not to be degenerate (every slice's RMS in [0.02, 4], max |activation| < 10, every value >= 1e-3, float32 within 1e-5 of a float64
run of the same module) before anything is written.

Output (MEBT_GOLDEN_OUT overrides the directory): lpips_golden.npz with, per case `t` of CASES: the uint8 image pairs `a_t`, `b_t`
[N, H, W, 3] (the network sees u / 255 - 0.5), the reference's value per pair `val_t` [N], its five per-slice terms `layers_t` [N, 5],
the per-channel means of each slice output for pair 0 `means_t` [2, 1472] (image a, image b); and the state-dict keys and shapes.

Usage:  python tests/golden/lpips/make_golden_lpips.py
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

CASES = {"s16": (2, 16, 16), "odd": (3, 36, 20), "mid": (2, 32, 48), "full": (1, 128, 128)}
VGG_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]


def _vgg16_stand_in(pretrained=False, **kw):
    """torchvision.models.vgg16 as far as the reference uses it: an object whose `.features` is the standard Sequential"""
    layers, cin = [], 3
    for v in VGG_CFG:
        if v == "M":
            layers.append(torch.nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [torch.nn.Conv2d(cin, v, kernel_size=3, padding=1), torch.nn.ReLU(inplace=True)]
            cin = v
    return types.SimpleNamespace(features=torch.nn.Sequential(*layers))


def load_reference():
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.vgg16 = _vgg16_stand_in
    saved = {k: sys.modules.get(k) for k in ("torchvision", "torchvision.models")}
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, tv.models
    for name in ("requests", "tqdm"):
        try:
            __import__(name)
        except ImportError:
            m = types.ModuleType(name)
            m.tqdm = None
            sys.modules[name] = m
    try:
        spec = importlib.util.spec_from_file_location("mebt_reference_lpips", os.path.join(REF, "mebt", "modules", "lpips.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    mod.LPIPS.load_from_pretrained = lambda self, name="vgg_lpips": None
    return mod


def closed_form_state_dict(shapes=None, prefix=""):
    """{key: tensor} of the closed-form LPIPS weights (33 tensors with the scaling buffers); `shapes` defaults to the schema of
    mebt_amd.lpips.expected_shapes()"""
    if shapes is None:
        from mebt_amd.lpips import expected_shapes
        shapes = dict(expected_shapes())
        shapes["scaling_layer.shift"], shapes["scaling_layer.scale"] = (1, 3, 1, 1), (1, 3, 1, 1)
    sd = {}
    for k, shp in shapes.items():
        shp = tuple(shp)
        if k == "scaling_layer.shift":
            v = np.array([-.030, -.088, -.188], dtype=np.float32).reshape(shp)
        elif k == "scaling_layer.scale":
            v = np.array([.458, .448, .450], dtype=np.float32).reshape(shp)
        elif k.startswith("lin"):
            v = np.abs(cf.pseudo_normal(k, shp, std=1.0)) * np.float32(4.0 / shp[1])
        elif k.endswith(".weight"):
            v = cf.pseudo_normal(k, shp, std=float(np.sqrt(2.0 / np.prod(shp[1:]))))
        elif k.endswith(".bias"):
            v = cf.pseudo_normal(k, shp, std=0.05)
        else:
            raise KeyError(k)
        sd[prefix + k] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return sd


def structured_pairs(shape):
    """uint8 [N, H, W, 3] x 2: gradients and a bright square, and the same plus structured noise whose amplitude grows with n"""
    N, H, W = shape
    n, y, x, c = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    a = (x * (3 + n) + y * (5 + 2 * c) + 40 * c + 61 * n) % 256
    sq = (np.abs(x - (W // 3 + 5 * n) % W) < 4) & (np.abs(y - H // 2) < 3)
    a = np.where(sq, 255 - c * 60, a)
    amp = 40 + 30 * n
    noise = ((x * 7 + y * 13 + c * 29 + (x * y) % 11 * 5) % (2 * amp + 1)) - amp
    b = np.clip(a + noise, 0, 255)
    return a.astype(np.uint8), b.astype(np.uint8)


def to_input(u8):
    """uint8 [N, H, W, 3] -> float32 [N, 3, H, W] = u / 255 - 0.5"""
    return (torch.from_numpy(u8).permute(0, 3, 1, 2).to(torch.float32) / 255.0 - 0.5).contiguous()


def reference_terms(ref, model, a, b):
    """the reference's forward, and its terms slice by slice with its own functions: (value [N], terms [N, 5], slice outputs of a, of b)"""
    val = model(a, b).reshape(-1)
    fa, fb = model.net(model.scaling_layer(a)), model.net(model.scaling_layer(b))
    lins = [model.lin0, model.lin1, model.lin2, model.lin3, model.lin4]
    terms = []
    for k in range(5):
        diff = (ref.normalize_tensor(fa[k]) - ref.normalize_tensor(fb[k])) ** 2
        terms.append(ref.spatial_average(lins[k].model(diff), keepdim=True).reshape(-1))
    return val, torch.stack(terms, 1), fa, fb


def main():
    out_dir = os.environ.get("MEBT_GOLDEN_OUT", HERE)
    torch.set_num_threads(4)                       # fixed reduction split of the CPU convolutions on every machine
    ref = load_reference()
    model = ref.LPIPS().eval()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert len(shapes) == 33, len(shapes)
    model.load_state_dict(closed_form_state_dict(shapes), strict=True)
    model64 = ref.LPIPS().eval()
    model64.load_state_dict(closed_form_state_dict(shapes), strict=True)
    model64 = model64.double()
    res = {"sd_keys": np.array(list(shapes.keys())),
           "sd_shapes": np.array([list(s) + [-1] * (4 - len(s)) for s in shapes.values()], dtype=np.int64)}
    with torch.no_grad():
        for tag, shp in CASES.items():
            a8, b8 = structured_pairs(shp)
            a, b = to_input(a8), to_input(b8)
            val, terms, fa, fb = reference_terms(ref, model, a, b)
            val64 = model64(a.double(), b.double()).reshape(-1)
            assert torch.isfinite(val).all() and float(val.min()) >= 1e-3, (tag, val)
            assert float(((val.double() - val64).abs() / val64).max()) <= 1e-5, (tag, val, val64)
            assert float((terms.sum(1) - val).abs().max()) <= 1e-5 * float(val.max()), (tag, terms, val)
            for k in range(5):
                rms, top = float(fa[k].pow(2).mean().sqrt()), float(max(fa[k].abs().max(), fb[k].abs().max()))
                assert 0.02 <= rms <= 4.0 and top < 10.0, (tag, k, rms, top)
            res[f"a_{tag}"], res[f"b_{tag}"] = a8, b8
            res[f"val_{tag}"] = val.numpy().astype(np.float32)
            res[f"layers_{tag}"] = terms.numpy().astype(np.float32)
            res[f"means_{tag}"] = np.stack([np.concatenate([f[k][0].mean(dim=(1, 2)).numpy() for k in range(5)]) for f in (fa, fb)]).astype(np.float32)
            print(f"{tag}: values {val.tolist()}")
    np.savez_compressed(os.path.join(out_dir, "lpips_golden.npz"), **res)
    print(f"wrote {os.path.join(out_dir, 'lpips_golden.npz')}")


if __name__ == "__main__":
    main()
