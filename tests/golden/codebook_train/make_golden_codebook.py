#!/usr/bin/env python3
"""Generate tests/golden/codebook_train/codebook_golden*.npz by running the *real* reference first stage in train() mode (build container
only: needs the reference checkout, see tests/golden/make_golden.py for the stand-ins of its third-party imports).

`vq_micro` on the closed-form weights, video [2, 3, 4, 16, 16]: M = 64 latent rows, 512 codes of dimension 64, so M < n_codes and the
reference's `_tile` (eight noised copies of z) is exercised.  The objective is the one of make_golden_vqgrad.py (recon_loss +
commitment_loss, perceptual_weight 0, before discriminator_iter_start), composed from the model's own submodules; the codebook is the
real `mebt.modules.codebook.Codebook`: `_init_embeddings` (codebook.py:34-46) before the first arg-min, then in every forward the EMA
update with random restarts (codebook.py:66-89).  Recorded: the initialisation, three forwards each followed by `loss.backward()` and a
`torch.optim.SGD` step, and a fourth forward (the ids after the third update, the losses after the third step).

The draws are torch's own (seed 0); `torch.randperm` and `torch.randn_like` are wrapped so that what they returned is recorded: per
draw `src` = randperm[:n_codes] and `noise` = the rows of randn_like at those positions, which is all of both that the reference uses.
Per forward k: z_k (the latent rows), ids_k, n_total_k, src_k / noise_k, and N_k, z_avg_k, embeddings_k after the update; the losses.

`restart_thres`: with the default 1.0 a code used once after the initialisation lands on 0.99 + 0.01, exactly on the rounding edge of
`N >= restart_thres`.  The generator sets `model.codebook.restart_thres` from a short list and asserts that every |N - restart_thres| of
every recorded step is at least 1e-4.  It also asserts, trying video variants until all hold: the relative gap between the best and the
second-best code distance is at least 2e-3 in every forward AND the absolute gap is at least 8 times the largest deviation of the
reference's fp32 distances from float64 ones (after the initialisation the codes are z's own rows plus noise of 1.25e-3 per element:
the best distance is about 1e-4 and comes out of a cancellation, so a relative gap alone does not keep the ids off fp32 rounding);
min |x_recon - x| >= 1e-4; at least one forward restarts a code and at least one keeps a code.

Also recorded, per forward and buffer, `twin_dev/*`: how far the reference's fp32 buffers lie from a float64 twin of the whole run (the
oracle's layers and autograd in float64 with the same ids and draws, tests/codebook_common.py's statements for the codebook), as a
fraction of the buffer's maximum.  The whole-model gate of the GPU test is 8 times that.

Usage:  python tests/golden/codebook_train/make_golden_codebook.py
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

from tests import codebook_common as cc
from tests import vqgrad_common as vc
from tests.golden.make_golden import build_reference_vqgan, install_stubs
from tests.golden.vqgrad.make_golden_vqgrad import video

NAME = "vq_micro"
SGD_LR = 1e-4
MIN_GAP, MIN_ABS, MIN_EDGE = 2e-3, 1e-4, 1e-4
THRESHOLDS = (0.995, 0.9975, 0.9925)
SHARD_BYTES = 900 * 1024
PRE_VQ_SCALE = 2.0 ** -6
ATTEMPTS = 64
VARIANTS = [(a, s) for s in range(8) for a in (1.0, 0.8, 1.2, 0.6, 1.4, 0.4)]          # base amplitude, noise stream


class Draws:
    """torch.randperm / torch.randn_like, recording what they return"""

    def __init__(self):
        self.real = (torch.randperm, torch.randn_like)
        self.perms, self.noises = [], []

    def __enter__(self):
        def randperm(n, *a, **k):
            p = self.real[0](n, *a, **k)
            self.perms.append(p.clone())
            return p

        def randn_like(t, *a, **k):
            r = self.real[1](t, *a, **k)
            self.noises.append(r.clone())
            return r
        torch.randperm, torch.randn_like = randperm, randn_like
        return self

    def __exit__(self, *exc):
        torch.randperm, torch.randn_like = self.real

    def take(self, n_codes):
        """the one (randn_like, randperm) pair drawn since the last call -> (src, noise rows)"""
        assert len(self.perms) == 1 and len(self.noises) == 1, (len(self.perms), len(self.noises))
        src = self.perms.pop()[:n_codes]
        return src, self.noises.pop()[src]


def gaps(flat, e):
    """-> (whether the fp32 and the float64 arg-min agree, relative gap, absolute gap, largest |fp32 distance - float64 distance|) of the arg-min of codebook.py:53-57"""
    d32 = (flat ** 2).sum(1, keepdim=True) - 2 * flat @ e.t() + (e.t() ** 2).sum(0, keepdim=True)
    f64, e64 = flat.double(), e.double()
    d64 = (f64 ** 2).sum(1, keepdim=True) - 2 * f64 @ e64.t() + (e64.t() ** 2).sum(0, keepdim=True)
    b2 = torch.topk(d64, 2, dim=1, largest=False).values
    same = torch.equal(d32.argmin(1), d64.argmin(1))
    return same, float(((b2[:, 1] - b2[:, 0]) / b2[:, 0].abs()).min()), float((b2[:, 1] - b2[:, 0]).min()), float((d32.double() - d64).abs().max())


def scaled_params(P):
    """the closed-form weights with pre_vq_conv (weight and bias) times PRE_VQ_SCALE: z, and with it the rounding error of the fp32
    code distances (proportional to |z|^2), shrinks while the restart noise keeps its absolute size 0.01 / sqrt(d)"""
    return {k: (v * PRE_VQ_SCALE if k.startswith("pre_vq_conv.") else v).clone() for k, v in P.items()}


def snapshot(cb):
    return [t.detach().clone() for t in (cb.embeddings, cb.N, cb.z_avg)]


def restore(cb, snap):
    for t, s_ in zip((cb.embeddings, cb.N, cb.z_avg), snap):
        t.data.copy_(s_)


def forward_ok(model, x, z):
    """the conditions on one forward at the codebook as it stands -> (ok, text)"""
    with torch.no_grad():
        flat = z.detach().permute(0, 2, 3, 4, 1).reshape(-1, z.shape[1])
        e = model.codebook.embeddings.detach()
        same, gap, absgap, noise32 = gaps(flat, e)
        d = (flat ** 2).sum(1, keepdim=True) - 2 * flat @ e.t() + (e.t() ** 2).sum(0, keepdim=True)
        ids = d.argmin(1).view(z.shape[0], *z.shape[2:])
        q = F.embedding(ids, e).permute(0, 4, 1, 2, 3)
        near = float((model.decoder(model.post_vq_conv(q)) - x).abs().min())
    ok = same and gap >= MIN_GAP and absgap >= 8 * noise32 and near >= MIN_ABS
    return ok, f"gap {gap:.2e} (absolute {absgap:.2e}, fp32 distance error {noise32:.2e}) min|x_recon - x| {near:.2e}"


def record(a, stream, thres):
    """The codes a forward searches are written by the draws of the update before it (the initialisation for the first), and whether
    its ids and L1 signs stay clear of rounding hangs on those draws alone: each such draw is repeated under torch.manual_seed(100 * k +
    attempt), attempt = 0, 1, ..., from the same state until the forward after it meets the conditions."""
    model, cfg, P = build_reference_vqgan(NAME)
    model.load_state_dict(scaled_params(P), strict=False)
    model.train()
    cb = model.codebook
    cb._need_init, cb.restart_thres = False, thres
    x = video(a, stream)
    params = {k: p for k, p in model.named_parameters() if k.startswith(vc.TRAINED)}
    opt = torch.optim.SGD(list(params.values()), lr=SGD_LR)
    out = {"x": x.numpy(), "l1_weight": np.float64(model.l1_weight), "sgd_lr": np.float64(SGD_LR), "restart_thres": np.float64(thres),
           "pre_vq_scale": np.float64(PRE_VQ_SCALE)}
    losses, restarted, kept, seeds = [], 0, 0, []
    z_prev = pre = None

    def keep_update(k, src, noise):
        out[f"src_{k}"], out[f"noise_{k}"] = src.numpy(), noise.numpy()
        out[f"N_{k}"], out[f"z_avg_{k}"], out[f"embeddings_{k}"] = cb.N.numpy().copy(), cb.z_avg.numpy().copy(), cb.embeddings.numpy().copy()

    with Draws() as draws:
        for k in range(cc.STEPS):
            opt.zero_grad()
            z = model.pre_vq_conv(model.encoder(x))
            flat = z.detach().permute(0, 2, 3, 4, 1).reshape(-1, z.shape[1])
            before = snapshot(cb) if k == 0 else pre
            for attempt in range(ATTEMPTS):
                restore(cb, before)
                torch.manual_seed(100 * k + attempt)
                if k == 0:
                    cb._init_embeddings(z.detach())                                  # codebook.py:50-51, its first statement in forward
                else:
                    with torch.no_grad():
                        cb(z_prev)                                                   # forward k - 1 again: the same ids, new draws
                src, noise = draws.take(cb.n_codes)
                ok, text = forward_ok(model, x, z)
                if ok:
                    break
            else:
                print(f"  variant ({a}, {stream}, {thres}): no draw in {ATTEMPTS} lets forward {k} meet the conditions ({text})")
                return False, out, cfg, P, x
            seeds.append(attempt)
            if k == 0:
                out["src_init"], out["noise_init"] = src.numpy(), noise.numpy()
            else:
                keep_update(k - 1, src, noise)
            assert not cb._need_init
            pre = snapshot(cb)
            torch.manual_seed(100 * (k + 1))
            vq_output = cb(z)
            src, noise = draws.take(cb.n_codes)
            if k == cc.STEPS - 1:
                keep_update(k, src, noise)
            x_recon = model.decoder(model.post_vq_conv(vq_output['embeddings']))
            rl, cl = F.l1_loss(x_recon, x) * model.l1_weight, vq_output['commitment_loss']
            ids = vq_output['encodings']
            edge = float((cb.N - thres).abs().min())
            r = int((cb.N < thres).sum())
            restarted, kept = restarted + r, kept + cb.n_codes - r
            print(f"  variant ({a}, {stream}, {thres}) forward {k} (draw attempt {attempt}): recon {float(rl):.6f} commitment {float(cl):.3e} {text} "
                  f"min|N - thres| {edge:.2e} restarted {r}")
            if edge < MIN_EDGE:
                return False, out, cfg, P, x
            losses.append([float(rl), float(cl)])
            out[f"z_{k}"], out[f"ids_{k}"] = flat.numpy().copy(), ids.numpy().copy()
            out[f"n_total_{k}"] = torch.bincount(ids.reshape(-1), minlength=cb.n_codes).float().numpy()
            z_prev = z.detach()
            if k < cc.STEPS - 1:
                (rl + cl).backward()
                opt.step()
    out["step_losses"] = np.array(losses, dtype=np.float64)
    out["draw_attempts"] = np.array(seeds)
    ok = restarted > 0 and kept > 0 and sum(losses[3]) < sum(losses[0])
    return ok, out, cfg, P, x


def float64_twin(out, cfg, P, x):
    """the same run in float64: the oracle's layers and autograd, the reference's ids and draws, the codebook statements of
    tests/codebook_common.py -> out['twin_dev/<buffer>_<k>'], the fixture's deviation as a fraction of the buffer's maximum"""
    Q = {k: v.detach().double().clone().requires_grad_(k.startswith(vc.TRAINED)) for k, v in scaled_params(P).items()}
    x64 = x.double()
    thres, n_codes = float(out["restart_thres"]), cfg.n_codes
    N = zavg = None
    for k in range(cc.STEPS):
        ids = torch.from_numpy(out[f"ids_{k}"])
        if k == 0:
            with torch.no_grad():
                _, _, _, z = vc.objective(Q, cfg, x64, ids)
                flat = z.permute(0, 2, 3, 4, 1).reshape(-1, z.shape[1])
                k0 = cc.restart_rows_twin(flat, torch.from_numpy(out["src_init"]), torch.from_numpy(out["noise_init"]))
            Q["codebook.embeddings"] = k0.clone()
            N, zavg = torch.ones(n_codes, dtype=torch.float64), k0.clone()
        rl, cl, _, z = vc.objective(Q, cfg, x64, ids)
        flat = z.detach().permute(0, 2, 3, 4, 1).reshape(-1, z.shape[1])
        n_total, encode_sum, _ = cc.sums_twin(ids, flat, n_codes)
        k_rand = cc.restart_rows_twin(flat, torch.from_numpy(out[f"src_{k}"]), torch.from_numpy(out[f"noise_{k}"]))
        emb, usage = cc.ema_statements(N, zavg, n_total, encode_sum, k_rand, thres, False)
        assert torch.equal(usage, torch.from_numpy(out[f"N_{k}"]) >= thres)
        for name, t in (("N", N), ("z_avg", zavg), ("embeddings", emb)):
            ref = torch.from_numpy(out[f"{name}_{k}"]).double()
            out[f"twin_dev/{name}_{k}"] = np.float64(float((ref - t).abs().max() / t.abs().max()))
        for i, key in enumerate(("recon_loss", "commitment_loss")):
            assert abs(float((rl, cl)[i]) - out["step_losses"][k, i]) <= 1e-4 * out["step_losses"][k, i] + 1e-9, (k, key)
        if k < cc.STEPS - 1:
            (rl + cl).backward()
            with torch.no_grad():
                for name in vc.trained_names(Q):
                    Q[name] -= SGD_LR * Q[name].grad
                    Q[name].grad = None
        Q["codebook.embeddings"] = emb.clone()
        print(f"  float64 twin, forward {k}: fixture deviates by " + ", ".join(f"{n} {float(out[f'twin_dev/{n}_{k}']):.2e}" for n in ("N", "z_avg", "embeddings")))


def main():
    install_stubs()
    for a, stream in VARIANTS:
        for thres in THRESHOLDS:
            ok, out, cfg, P, x = record(a, stream, thres)
            if ok:
                break
        if ok:
            break
    else:
        raise SystemExit("no video variant meets the conditions")
    print(f"video variant ({a}, {stream}), restart_thres {thres}")
    float64_twin(out, cfg, P, x)
    dest = os.environ.get("MEBT_GOLDEN_OUT", HERE)
    shards, size = [{}], 0
    for k in sorted(out, key=lambda k: (np.asarray(out[k]).nbytes > 65536, k)):
        nb = np.asarray(out[k]).nbytes
        if size + nb > SHARD_BYTES and shards[-1]:
            shards.append({})
            size = 0
        shards[-1][k] = out[k]
        size += nb
    for i, sh in enumerate(shards):
        path = os.path.join(dest, "codebook_golden.npz" if i == 0 else f"codebook_golden_{i}.npz")
        np.savez_compressed(path, **sh)
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB, {len(sh)} arrays)")


if __name__ == "__main__":
    main()
