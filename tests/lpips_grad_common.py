"""Shared by the LPIPS-backward tests and by tests/golden/lpips_grad/make_golden_lpips_grad.py: the float64 twin AT GIVEN DECISIONS, its
fp16-storage form, the closed formulas of the single operators and the fixture loader.  Test infrastructure only.

A ReLU mask and a pool winner are discrete outcomes of the forward.  One that flips (an activation within rounding of zero, two window
entries within rounding of each other) moves the gradient by far more than any rounding does, so the kernels' arithmetic
is held to a twin that takes every mask and every winner from SUPPLIED activations, the kernels' own tape, and computes everything else
itself in float64.  With its own activations supplied it is plain autograd (tests/test_lpips_grad_host.py)."""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

from mebt_amd import lpips as L

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_grad")
REF_GATE = 1e-4                     # of max |g|: the project's gate against the reference where no decision can flip
FLIP_L2 = 4e-3                      # relative L2 against the reference where single decisions may flip (about four flips)


def load_fixture():
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN_DIR, "lpips_grad_golden*.npz"))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


class _Round16(torch.autograd.Function):
    """value and gradient rounded to fp16: a tensor stored as fp16 whose gradient is stored as fp16"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.float16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.float16).to(g.dtype)


def _windows(t):
    """[N, C, H, W] -> [N, C, H // 2, W // 2, 4]: the 2 x 2 windows in row-major order"""
    Ho, Wo = t.shape[2] // 2, t.shape[3] // 2
    t = t[:, :, :2 * Ho, :2 * Wo]
    return torch.stack([t[:, :, 0::2, 0::2], t[:, :, 0::2, 1::2], t[:, :, 1::2, 0::2], t[:, :, 1::2, 1::2]], -1)


def pool_at(act, dec):
    """MaxPool2d(2, 2) of `act` with the winner of every window taken from `dec`: its first maximum in row-major order (torch's rule)"""
    idx = _windows(dec).argmax(-1, keepdim=True)
    return _windows(act).gather(-1, idx).squeeze(-1)


def features_at(own, img, decisions=None, dtype=torch.float64, fp16_storage=False):
    """img [N, 3, H, W] (raw) -> (the five slice outputs, the 13 convolution outputs after their ReLU, the 13 masks), differentiable in `img`.
    decisions: 13 tensors [N, C, h, w] whose sign is every ReLU's mask and whose windows give every pool's winner; None: the run's own."""
    r = _Round16.apply if fp16_storage else (lambda t: t)
    h = r((img.to(dtype) - own["scaling_layer.shift"].to(dtype).view(1, 3, 1, 1)) / own["scaling_layer.scale"].to(dtype).view(1, 3, 1, 1))
    feats, acts, masks, k = [], [], [], 0
    for s, idxs in L.SLICE_CONVS:
        if s > 1:
            h = r(pool_at(h, acts[-1].detach() if decisions is None else decisions[k - 1].to(dtype)))
        for i in idxs:
            w = own[f"net.slice{s}.{i}.weight"]
            w = w.to(torch.float16).to(dtype) if fp16_storage else w.to(dtype)
            pre = F.conv2d(h, w, own[f"net.slice{s}.{i}.bias"].to(dtype), padding=1)
            mask = (pre.detach() if decisions is None else decisions[k].to(dtype)) > 0
            h = r(pre * mask)
            acts.append(h)
            masks.append(mask)
            k += 1
        feats.append(h)
    return feats, acts, masks


def twin_at(sd, a, b, decisions=None, dtype=torch.float64, fp16_storage=False, scale=1.0):
    """a, b [N, 3, H, W] raw -> (value [N], d(sum_n value_n)/db [N, 3, H, W], the gradients at the five slice outputs' pre-activations
    [N, C, h, w], the 13 activations of b), all of `dtype`, detached.  decisions: as `features_at`, for b's side (a takes no gradient and
    runs on its own).  fp16_storage: every stored activation, every convolution weight and every stored activation gradient goes through
    fp16 and the backward runs at the power-of-two `scale`, removed afterwards: the storage rounding of the f16 mode alone."""
    own = L.extract(sd)
    bq = b.detach().to(dtype).clone().requires_grad_(True)
    with torch.no_grad():
        fa, _, _ = features_at(own, a, None, dtype, fp16_storage)
    fb, acts, masks = features_at(own, bq, decisions, dtype, fp16_storage)
    lay = torch.stack([L.head_twin(fa[k], fb[k], own[f"lin{k}.model.1.weight"].reshape(-1)) for k in range(5)], 1)
    val = lay.sum(1)
    for t in fb:
        t.retain_grad()
    (val.sum() * scale).backward()
    last = [sum(len(i) for _, i in L.SLICE_CONVS[:s + 1]) - 1 for s in range(5)]
    return val.detach(), bq.grad / scale, [fb[s].grad * masks[last[s]] / scale for s in range(5)], [t.detach() for t in acts]


def tape_decisions(tape, n):
    """the kernels' 13 forward outputs [2 n, h, w, C] -> the reconstruction half as [n, C, h, w] float64 on the CPU"""
    return [t[n:].permute(0, 3, 1, 2).double().cpu() for t in tape]


# ---- single operators, float64 -----------------------------------------------------------------------------------------------------------
def head_bwd_formula(f0, f1, w, coef, add=None):
    """f0, f1 [n, P, C], w [C] float64 -> d_feats [n, P, C] of include/mebt_hip.h's mebt_op_lpips_head_bwd; a zero f1 takes only its
    first term (which is 0 under the mask)"""
    P = f0.shape[1]
    n0, n1 = f0.pow(2).sum(-1, keepdim=True).sqrt(), f1.pow(2).sum(-1, keepdim=True).sqrt()
    d0, d1 = n0 + 1e-10, n1 + 1e-10
    g = -2.0 * coef / P * w * (f0 / d0 - f1 / d1)
    dot = (g * f1).sum(-1, keepdim=True)
    back = torch.where(n1 > 0, dot / (n1 * d1 * d1).clamp_min(1e-300), torch.zeros_like(dot))
    out = g / d1 - f1 * back
    if add is not None:
        out = out + add
    return torch.where(f1 > 0, out, torch.zeros_like(out))


def pool_bwd_rule(x, dy):
    """x [N, H, W, C], dy [N, H // 2, W // 2, C] -> dx [N, H, W, C]: dy at the first maximum of each window where it is positive"""
    N, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    xc = x.permute(0, 3, 1, 2)
    win = _windows(xc)
    idx = win.argmax(-1, keepdim=True)
    top = win.gather(-1, idx)
    routed = torch.zeros_like(win).scatter_(-1, idx, torch.where(top > 0, dy.permute(0, 3, 1, 2).unsqueeze(-1), torch.zeros_like(top)))
    dx = torch.zeros_like(xc)
    dx[:, :, 0:2 * Ho:2, 0:2 * Wo:2], dx[:, :, 0:2 * Ho:2, 1:2 * Wo:2] = routed[..., 0], routed[..., 1]
    dx[:, :, 1:2 * Ho:2, 0:2 * Wo:2], dx[:, :, 1:2 * Ho:2, 1:2 * Wo:2] = routed[..., 2], routed[..., 3]
    return dx.permute(0, 2, 3, 1).contiguous()


def conv_as_forward_layout(x, wl, cin, cout):
    """the statement of the layout mebt_op_conv2d_3x3 reads: x [N, H, W, cin], wl [cout pad 64][Kpad] with K = (tap, ci), ci fastest ->
    [N, H, W, cout], zero padding 1, no bias"""
    w = wl[:cout, :9 * cin].reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    return F.conv2d(x.permute(0, 3, 1, 2), w.to(x.dtype), padding=1).permute(0, 2, 3, 1)


# ---- the first-stage objective with the perceptual term ------------------------------------------------------------------------------------
class _ScaleGrad(torch.autograd.Function):
    """identity whose gradient is multiplied by `k` (the exact power-of-two factor of mebt_op_lpips_input_bwd)"""

    @staticmethod
    def forward(ctx, x, k):
        ctx.k = k
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return g * ctx.k, None


def probe(name, shape):
    """the fixed direction a gradient tensor is projected on where the fixture does not hold it in full"""
    from oracle import closed_form as cf
    return np.asarray(cf.pseudo_normal("lpips-grad-probe/" + name, tuple(shape), std=1.0), dtype=np.float64)


def vq_objective_grads(P, cfg, sd, x, ids, frame_idx, pw=1.0, dtype=torch.float64, fp16_storage=False, grad_scale=1.0, branch_scale=1.0,
                       l1_signs=None, decisions=None):
    """recon + commitment (tests/vqgrad_common.objective) + pw * mean_b LPIPS(x[b, :, idx_b], x_recon[b, :, idx_b]) with the ids fixed
    -> ({name: gradient, numpy float64}, recon_loss, commitment_loss, perceptual_loss).  fp16_storage: both parts store through fp16;
    the whole backward runs at `grad_scale`, the LPIPS branch at `grad_scale * branch_scale` down to the frames (LPIPS.value_and_grad's
    S_p), both removed exactly.  l1_signs / decisions: the discrete outcomes taken as given."""
    from tests import vqgrad_common as vc
    own = L.extract(sd)
    Q = {k: v.detach().to(dtype).clone().requires_grad_(k.startswith(vc.TRAINED)) for k, v in P.items()}
    xd = x.to(dtype)
    rl, cl, rec, _ = vc.objective(Q, cfg, xd, ids, vc.L1_WEIGHT, fp16_storage, l1_signs)
    B = x.shape[0]
    bi = torch.arange(B)
    fi = torch.as_tensor(frame_idx).long()
    a, b = xd[bi, :, fi], _ScaleGrad.apply(rec[bi, :, fi], 1.0 / branch_scale)
    with torch.no_grad():
        fa, _, _ = features_at(own, a, None, dtype, fp16_storage)
    fb, _, _ = features_at(own, b, decisions, dtype, fp16_storage)
    val = torch.stack([L.head_twin(fa[k], fb[k], own[f"lin{k}.model.1.weight"].reshape(-1)) for k in range(5)], 1).sum(1)
    pl = val.mean() * pw
    ((rl + cl) * grad_scale + pl * (grad_scale * branch_scale)).backward()
    grads = {k: (Q[k].grad / grad_scale).double().numpy() for k in vc.trained_names(Q)}
    return grads, float(rl.detach()), float(cl.detach()), float(pl.detach())
