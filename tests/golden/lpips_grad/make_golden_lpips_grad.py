#!/usr/bin/env python3
"""Generate tests/golden/lpips_grad/lpips_grad_golden*.npz by running the *real* reference modules (build container only: needs the
reference checkout; the stand-ins for third-party imports are those of tests/golden/lpips/make_golden_lpips.py and
tests/golden/make_golden.py).

(i) Per case of the LPIPS fixture's CASES (its images, its closed-form weights): the reference's float32 autograd gradient of
`model(a, b).mean()` with respect to b, `grad_<case>` [N, 3, H, W], and `dev_<case>`, its largest deviation from a float64 run of the
same module as a share of max |g|.  Asserted <= 1e-4 (measured 6e-7 .. 6e-5: the gate of the GPU test is safe against the reference's own
rounding).  Also `flipdev_<case>`: how far the float64 gradient moves, as a share of its maximum, when the weights are perturbed by 1e-6
relative: where a ReLU or pool decision flips this is ~5e-3, where none does ~2e-6, which is why only some cases are gated elementwise.

(ii) The reference VQGAN at `vq_micro` with perceptual_weight 1, the closed-form LPIPS weights and the vqgrad fixture's video: the
autoencoder objective recon + commitment + perceptual composed from the model's own submodules in the order of vqgan.py:98-116
(`VQGAN.forward` moves a tensor to CUDA), with `frame_idx` fixed and recorded.  Per gradient of the 68 trained tensors: `vqmax/<name>` =
max |g|, `vqdot/<name>` = the float64 dot product with tests/lpips_grad_common.probe(name), `vqgrad/<name>` in full where the tensor is
under 64 KiB, and `twin_dev/<name>`: the deviation of the fp16-storage twin of the whole objective from float64 as a share of the
tensor's maximum (the f16 gate of the GPU test is four times that).

Also printed, for DESIGN.md §9g and `mebt_amd.lpips.GRAD_MAX_TABLE`: the per-layer maxima of the float64 gradient on `full`.

Usage:  python tests/golden/lpips_grad/make_golden_lpips_grad.py
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

from tests import lpips_grad_common as lg
from tests import vqgrad_common as vc
from tests.golden.lpips.make_golden_lpips import CASES, closed_form_state_dict, load_reference, structured_pairs, to_input

NAME = "vq_micro"
FRAME_IDX = (1, 3)
FULL_BYTES = 64 * 1024
SHARD_BYTES = 900 * 1024
REL_PERTURB = 1e-6


def ref_grad(model, a, b, dtype):
    bq = b.to(dtype).clone().requires_grad_(True)
    model(a.to(dtype), bq).mean().backward()
    return bq.grad.detach()


def build_lpips(ref, dtype=torch.float32, perturb=0.0):
    model = ref.LPIPS().eval()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = closed_form_state_dict(shapes)
    if perturb:
        from oracle import closed_form as cf
        sd = {k: (v.double() * (1.0 + perturb * torch.from_numpy(np.sign(cf.pseudo_normal("perturb/" + k, tuple(v.shape), std=1.0)).astype(np.float64)))
                  if k.startswith("net.") else v) for k, v in sd.items()}
        model = model.double()
    model.load_state_dict(sd, strict=True)
    for p in model.parameters():
        p.requires_grad_(False)
    return model.to(dtype), shapes


def layer_maxima(sd, a, b):
    """max |d(sum_n value_n)/d activation| of the float64 twin at the scaled input and at each of the 13 convolution outputs"""
    from mebt_amd import lpips as L
    own = L.extract(sd)
    bq = b.double().clone().requires_grad_(True)
    with torch.no_grad():
        fa, _, _ = lg.features_at(own, a, None)
    fb, acts, _ = lg.features_at(own, bq, None)
    for t in acts:
        t.retain_grad()
    torch.stack([L.head_twin(fa[k], fb[k], own[f"lin{k}.model.1.weight"].reshape(-1)) for k in range(5)], 1).sum().backward()
    scale = own["scaling_layer.scale"].double().view(1, 3, 1, 1)
    return float((bq.grad * scale).abs().max()), [float(t.grad.abs().max()) for t in acts]


def part_one(ref, out):
    m32, shapes = build_lpips(ref)
    m64, _ = build_lpips(ref, torch.float64)
    mp, _ = build_lpips(ref, torch.float64, REL_PERTURB)
    sd = closed_form_state_dict(shapes)
    for tag, shp in CASES.items():
        a8, b8 = structured_pairs(shp)
        a, b = to_input(a8), to_input(b8)
        g32, g64, gp = ref_grad(m32, a, b, torch.float32), ref_grad(m64, a, b, torch.float64), ref_grad(mp, a, b, torch.float64)
        assert torch.isfinite(g32).all() and torch.isfinite(g64).all(), tag
        top = float(g64.abs().max())
        dev = float((g32.double() - g64).abs().max()) / top
        flip = float((gp - g64).abs().max()) / top
        flip_l2 = float((gp - g64).norm() / g64.norm())
        _, gt, _, _ = lg.twin_at(sd, a, b)
        tw = float((gt / shp[0] - g64).abs().max()) / top
        print(f"{tag}: max |g| {top:.3e} median {float(g64.abs().median()):.3e}; float32 vs float64 {dev:.2e} of max; weights moved by "
              f"{REL_PERTURB:g}: {flip:.2e} of max, {flip_l2:.2e} relative L2; twin vs the reference in float64 {tw:.2e}")
        assert dev <= 1e-4, (tag, dev)
        assert tw <= 1e-9, (tag, tw)
        out[f"grad_{tag}"] = g32.numpy().astype(np.float32)
        out[f"dev_{tag}"], out[f"flipdev_{tag}"], out[f"flipl2_{tag}"] = np.float64(dev), np.float64(flip), np.float64(flip_l2)
        if tag == "full":
            gin, per = layer_maxima(sd, a, b)
            print("full: max |d sum LPIPS / d activation| at the scaled input and the 13 convolution outputs:")
            print("  " + ", ".join(f"{v:.2e}" for v in [gin] + per))
            out["layer_max_full"] = np.array([gin] + per, dtype=np.float64)
    return sd


def part_two(ref, sd, out):
    from tests.golden.make_golden import build_reference_vqgan, install_stubs
    from mebt_amd import lpips as L
    install_stubs()
    model, cfg, P = build_reference_vqgan(NAME)
    lp, _ = build_lpips(ref)
    model.perceptual_model = lp
    model.perceptual_weight = 1.0
    x = torch.from_numpy(vc.load_fixture()["x"])
    B, Cc, T, H, W = x.shape
    params = {k: p for k, p in model.named_parameters() if k.startswith(vc.TRAINED)}
    assert len(params) == 68, len(params)
    for p in params.values():
        p.grad = None
    # vqgan.py:98-116 on the model's own submodules
    z = model.pre_vq_conv(model.encoder(x))
    vq_output = model.codebook(z)
    x_recon = model.decoder(model.post_vq_conv(vq_output['embeddings']))
    recon_loss = F.l1_loss(x_recon, x) * model.l1_weight
    frame_idx = torch.tensor(FRAME_IDX)
    sel = frame_idx.reshape(-1, 1, 1, 1, 1).repeat(1, Cc, 1, H, W)
    frames, frames_recon = torch.gather(x, 2, sel).squeeze(2), torch.gather(x_recon, 2, sel).squeeze(2)
    perceptual_loss = model.perceptual_model(frames, frames_recon).mean() * model.perceptual_weight
    (recon_loss + vq_output['commitment_loss'] + perceptual_loss).backward()
    ids = vq_output['encodings']
    losses = [float(recon_loss.detach()), float(vq_output['commitment_loss'].detach()), float(perceptual_loss.detach())]
    print(f"vq_micro: recon {losses[0]:.6f} commitment {losses[1]:.6f} perceptual {losses[2]:.6f}, frame_idx {FRAME_IDX}")
    ref_g = {k: p.grad.detach().double().numpy() for k, p in params.items()}
    g64, rl, cl, pl = lg.vq_objective_grads(P, cfg, sd, x, ids, frame_idx)
    worst = max(np.abs(ref_g[k] - g64[k]).max() / vc.scale_of(k, g64) for k in g64)
    print(f"reference fp32 gradients vs the float64 twin objective: {worst:.2e} of the tensor's maximum (losses {rl:.6f} {cl:.6f} {pl:.6f})")
    assert worst < 1e-5, worst
    g0, _, _ = vc.objective_grads(P, cfg, x, ids)
    share = max(np.abs(g64[k] - g0[k]).max() / vc.scale_of(k, g64) for k in g64 if k.startswith("decoder."))
    print(f"the perceptual term moves the decoder's gradients by up to {share:.2e} of their maximum")
    S = vc.default_scale(float(model.l1_weight), x.numel())
    Sp = L.default_branch_scale(S * 1.0 / B, H, W)
    g16, _, _, _ = lg.vq_objective_grads(P, cfg, sd, x, ids, frame_idx, fp16_storage=True, grad_scale=S, branch_scale=Sp)
    devs = []
    for k in g64:
        dev = np.abs(g16[k] - g64[k]).max() / vc.scale_of(k, g64)
        out["twin_dev/" + k] = np.float64(dev)
        devs.append(dev)
        out["vqmax/" + k] = np.float64(np.abs(ref_g[k]).max())
        out["vqdot/" + k] = np.float64((ref_g[k] * lg.probe(k, ref_g[k].shape)).sum())
        if ref_g[k].size * 4 < FULL_BYTES:
            out["vqgrad/" + k] = ref_g[k].astype(np.float32)
    print(f"fp16-storage twin (scale {S:g}, branch scale {Sp:g}) vs float64: {min(devs):.2e} .. {max(devs):.2e} of the tensor's maximum")
    out["vq_losses"] = np.array(losses, dtype=np.float64)
    out["vq_frame_idx"] = np.array(FRAME_IDX, dtype=np.int64)
    out["vq_ids"] = ids.numpy()
    out["vq_twin_scale"], out["vq_twin_branch_scale"] = np.float64(S), np.float64(Sp)


def main():
    torch.set_num_threads(4)                       # fixed reduction split of the CPU convolutions on every machine
    torch.manual_seed(0)
    ref = load_reference()
    out = {}
    sd = part_one(ref, out)
    part_two(ref, sd, out)
    dest = os.environ.get("MEBT_GOLDEN_OUT", HERE)
    shards, size = [{}], 0
    for k in sorted(out):
        nb = np.asarray(out[k]).nbytes
        if size + nb > SHARD_BYTES and shards[-1]:
            shards.append({})
            size = 0
        shards[-1][k] = out[k]
        size += nb
    for i, sh in enumerate(shards):
        path = os.path.join(dest, "lpips_grad_golden.npz" if i == 0 else f"lpips_grad_golden_{i}.npz")
        np.savez_compressed(path, **sh)
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB, {len(sh)} arrays)")


if __name__ == "__main__":
    main()
