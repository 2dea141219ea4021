#!/usr/bin/env python3
"""Generate tests/golden/vqgrad/vqgrad_golden*.npz by running the *real* reference first stage (build container only: needs the
reference checkout, see tests/golden/make_golden.py for the stand-ins of its third-party imports).

`vq_micro` on the closed-form weights: the autoencoder objective of mebt/vqgan.py:98-102,183-184 before discriminator_iter_start with
perceptual_weight 0, loss = recon_loss + commitment_loss, composed from the model's own submodules in the order of vqgan.py:98-102
(`VQGAN.forward` moves a tensor to CUDA), `loss.backward()`, and the gradient of all 68 parameters of encoder, decoder, pre_vq_conv and
post_vq_conv.  Then two `torch.optim.SGD` steps (linear in the gradient; Adam's first step is a sign and would amplify the noise of
near-zero entries) with the losses and ids after each.  Also, per tensor, how far an fp16-storage twin of the objective
(tests/vqgrad_common.py) lies from float64: the f16 gate of the GPU test is four times that.

The video is a closed-form variant of make_golden.vqgan_video chosen so that at every recorded step (i) the smallest relative gap between
the best and the second-best code distance is at least 2e-3 (the ids do not hang on fp32 rounding) and (ii) no element has
|x_recon - x| < 1e-4 (no sign of the L1 seed does).  Both are asserted.

A file stays under the repository's 1 MiB limit: the gradients are spread over vqgrad_golden.npz, vqgrad_golden_1.npz, ...

Usage:  python tests/golden/vqgrad/make_golden_vqgrad.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.nn.functional as F

from oracle import closed_form as cf
from tests import vqgrad_common as vc
from tests.golden.make_golden import VQGAN_CONFIGS, build_reference_vqgan, install_stubs

NAME = "vq_micro"
SGD_LR = 2e-3
MIN_GAP, MIN_ABS = 2e-3, 1e-4
SHARD_BYTES = 900 * 1024
VARIANTS = [(a, s) for s in range(8) for a in (1.0, 0.8, 1.2, 0.6, 1.4, 0.4)]          # base amplitude, noise stream


def video(a, stream):
    """make_golden.vqgan_video's smooth structure times `a` plus 0.3 (u - 0.5)"""
    B, C, T, H, W = VQGAN_CONFIGS[NAME]["video"]
    u = cf.uniform01(f"vqgrad-video/{NAME}/{stream}", (B, C, T, H, W)).astype(np.float32)
    t = np.linspace(0, 1, T, dtype=np.float32)[None, None, :, None, None]
    y = np.linspace(0, 1, H, dtype=np.float32)[None, None, None, :, None]
    xg = np.linspace(0, 1, W, dtype=np.float32)[None, None, None, None, :]
    c = np.arange(C, dtype=np.float32)[None, :, None, None, None]
    base = 0.3 * np.sin(6.0 * xg + 2.0 * c + 3.0 * t) * np.cos(5.0 * y - t)
    return torch.from_numpy(np.clip(base * a + 0.3 * (u - 0.5), -0.5, 0.5).astype(np.float32))


def step(model, x):
    """one evaluation of the objective on the reference's modules -> (recon_loss, commitment_loss, ids, gap, min |x_recon - x|)"""
    z = model.pre_vq_conv(model.encoder(x))
    vq_output = model.codebook(z)
    x_recon = model.decoder(model.post_vq_conv(vq_output['embeddings']))
    recon_loss = F.l1_loss(x_recon, x) * model.l1_weight
    with torch.no_grad():
        flat = z.permute(0, 2, 3, 4, 1).reshape(-1, z.shape[1])
        e = model.codebook.embeddings
        d = (flat ** 2).sum(1, keepdim=True) - 2 * flat @ e.t() + (e.t() ** 2).sum(0, keepdim=True)
        b2 = torch.topk(d, 2, dim=1, largest=False).values
        gap = float(((b2[:, 1] - b2[:, 0]) / b2[:, 0].abs()).min())
        near = float((x_recon - x).abs().min())
    return recon_loss, vq_output['commitment_loss'], vq_output['encodings'], gap, near


def record(a, stream):
    model, cfg, P = build_reference_vqgan(NAME)
    x = video(a, stream)
    params = {k: p for k, p in model.named_parameters() if k.startswith(vc.TRAINED)}
    assert len(params) == 68, len(params)
    opt = torch.optim.SGD(list(params.values()), lr=SGD_LR)
    out, losses, ok = {"x": x.numpy(), "l1_weight": np.float64(model.l1_weight), "sgd_lr": np.float64(SGD_LR)}, [], True
    for k in range(3):
        opt.zero_grad()
        rl, cl, ids, gap, near = step(model, x)
        (rl + cl).backward()
        print(f"  variant ({a}, {stream}) step {k}: recon {float(rl.detach()):.6f} commitment {float(cl.detach()):.6f} gap {gap:.2e} min|x_recon - x| {near:.2e}")
        ok = ok and gap >= MIN_GAP and near >= MIN_ABS
        losses.append([float(rl.detach()), float(cl.detach())])
        out[f"ids_{k}"] = ids.numpy()
        if k == 0:
            for name, p in params.items():
                out["grad/" + name] = p.grad.detach().numpy().copy()
        opt.step()
    out["step_losses"] = np.array(losses, dtype=np.float64)
    ok = ok and sum(losses[2]) < sum(losses[1]) < sum(losses[0])
    return ok, out, cfg, P, x


def main():
    install_stubs()
    torch.manual_seed(0)
    for a, stream in VARIANTS:
        ok, out, cfg, P, x = record(a, stream)
        if ok:
            break
    else:
        raise SystemExit("no video variant meets the conditions")
    print(f"video variant ({a}, {stream})")
    ids = torch.from_numpy(out["ids_0"])
    ref = vc.fixture_grads(out)
    g64, rl, cl = vc.objective_grads(P, cfg, x, ids)
    worst = max(np.abs(ref[k] - g64[k]).max() / vc.scale_of(k, g64) for k in g64)
    print(f"reference fp32 gradients vs float64 oracle autograd: {worst:.2e} of the tensor's maximum (losses {rl:.6f} {cl:.6f})")
    assert worst < 1e-5
    S = vc.default_scale(float(out["l1_weight"]), x.numel())
    g16, _, _ = vc.objective_grads(P, cfg, x, ids, fp16_storage=True, grad_scale=S)
    devs, cos = [], []
    for k in g64:
        dev = np.abs(g16[k] - g64[k]).max() / vc.scale_of(k, g64)
        out["twin_dev/" + k] = np.float64(dev)
        devs.append(dev)
        if k not in vc.ZERO_BIAS:
            cos.append(float((g16[k] * g64[k]).sum() / np.sqrt((g16[k] ** 2).sum() * (g64[k] ** 2).sum())))
    out["twin_scale"] = np.float64(S)
    print(f"fp16-storage twin (scale {S:g}) vs float64: {min(devs):.2e} .. {max(devs):.2e} of the tensor's maximum, cosine >= {min(cos):.6f}")
    # shards under the file-size limit
    dest = os.environ.get("MEBT_GOLDEN_OUT", HERE)
    shards, size = [{}], 0
    for k in sorted(out, key=lambda k: (k.startswith("grad/"), k)):
        nb = np.asarray(out[k]).nbytes
        if size + nb > SHARD_BYTES and shards[-1]:
            shards.append({})
            size = 0
        shards[-1][k] = out[k]
        size += nb
    for i, sh in enumerate(shards):
        path = os.path.join(dest, "vqgrad_golden.npz" if i == 0 else f"vqgrad_golden_{i}.npz")
        np.savez_compressed(path, **sh)
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB, {len(sh)} arrays)")


if __name__ == "__main__":
    main()
