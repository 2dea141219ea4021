"""Shared by the first-stage backward tests and by tests/golden/vqgrad/make_golden_vqgrad.py: the reconstruction objective on the CPU
oracle's differentiable layer functions (oracle/vqgan_oracle.py) with the token ids held fixed, its fp16-storage twin, the fixture
loader, and a numpy walk of the data-gradient plan of `mebt_amd.vqgan._Conv.dgrad_plan`.  Test infrastructure only."""
import glob
import itertools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vqgan_oracle as vq

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vqgrad")
TRAINED = ("encoder.", "decoder.", "pre_vq_conv.", "post_vq_conv.")
# GroupNorm with one channel per group in front: dx is orthogonal to the constant, the bias gradient is exactly zero.  Judged against
# the maximum of the same layer's weight gradient.
ZERO_BIAS = ("encoder.conv_blocks.0.res.conv1.conv.bias", "decoder.conv_blocks.1.res1.conv1.conv.bias",
             "decoder.conv_blocks.1.res2.conv1.conv.bias")
L1_WEIGHT = 4.0


def trained_names(P):
    return [k for k in P if k.startswith(TRAINED)]


def scale_of(name, ref):
    """the magnitude a gradient tensor's error is judged against: its own maximum, or the weight gradient's for ZERO_BIAS"""
    key = name[:-len("bias")] + "weight" if name in ZERO_BIAS else name
    return float(np.abs(np.asarray(ref[key], dtype=np.float64)).max())


def load_fixture():
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN_DIR, "vqgrad_golden*.npz"))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def fixture_grads(fx):
    return {k[len("grad/"):]: v for k, v in fx.items() if k.startswith("grad/")}


# ---- the objective on the oracle's layers ------------------------------------------------------------------------------------------
class _Round16(torch.autograd.Function):
    """value and gradient rounded to fp16 (what a tensor stored as fp16 and its stored gradient go through)"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.float16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.float16).to(g.dtype)


class _GradRound16(torch.autograd.Function):
    """identity whose gradient is rounded to fp16 (an fp32 tensor whose gradient is stored as fp16)"""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.float16).to(g.dtype)


def objective(P, cfg, x, ids, l1_weight=L1_WEIGHT, fp16_storage=False, l1_signs=None):
    """recon_loss + commitment_loss of reference vqgan.py:98-102,183-184 (perceptual_weight 0, before discriminator_iter_start) with the
    codebook frozen and `ids` fixed, in the dtype of `P` / `x`.  fp16_storage: every stored activation, every convolution weight and
    every activation gradient goes through fp16, the arithmetic stays in the tensors' dtype: the storage rounding of the f16 mode
    alone.  l1_signs: the L1 term differentiated at a GIVEN sign pattern, sum signs * (x_recon - x) in place of sum |x_recon - x| (equal
    where the signs are the reconstruction's own).  -> (recon_loss, commitment_loss, x_recon, z)"""
    r = _Round16.apply if fp16_storage else (lambda t: t)
    gr = _GradRound16.apply if fp16_storage else (lambda t: t)

    def W(name):
        return r(P[name]) if fp16_storage else P[name]

    def conv(name, h, stride=(1, 1, 1)):
        return vq.same_pad_conv3d(h, W(name + ".conv.weight"), P[name + ".conv.bias"], stride)

    def ns(name, h):
        return r(vq.norm_silu(h, P[name + ".weight"], P[name + ".bias"]))

    def res(pre, h):
        t = r(conv(pre + ".conv1", ns(pre + ".norm1", h)))
        return r(h + conv(pre + ".conv2", ns(pre + ".norm2", t)))

    strides = vq._strides(cfg.n_times)
    h = r(conv("encoder.conv_first", x))
    for i, st in enumerate(strides):
        h = r(conv(f"encoder.conv_blocks.{i}.down", h, st))
        h = res(f"encoder.conv_blocks.{i}.res", h)
    h = ns("encoder.final_block.0", h)
    z = gr(conv("pre_vq_conv", h))
    e = F.embedding(ids, P["codebook.embeddings"]).permute(0, 4, 1, 2, 3)
    commitment = 0.25 * F.mse_loss(z, e)
    h = z + ((r(e) if fp16_storage else e) - z).detach()                      # straight-through (codebook.py:91)
    h = r(conv("post_vq_conv", h))
    h = ns("decoder.final_block.0", h)
    for i, st in enumerate(strides):
        name = f"decoder.conv_blocks.{i}.up"
        h = r(vq.same_pad_conv_transpose3d(h, W(name + ".convt.weight"), P[name + ".convt.bias"], st))
        h = res(f"decoder.conv_blocks.{i}.res1", h)
        h = res(f"decoder.conv_blocks.{i}.res2", h)
    rec = gr(conv("decoder.conv_last", h))
    if l1_signs is not None:
        return (l1_signs.to(rec.dtype) * (rec - x)).mean() * l1_weight, commitment, rec, z
    return F.l1_loss(rec, x) * l1_weight, commitment, rec, z


def objective_grads(P, cfg, x, ids, l1_weight=L1_WEIGHT, dtype=torch.float64, fp16_storage=False, grad_scale=1.0, l1_signs=None):
    """-> ({name: gradient, numpy float64}, recon_loss, commitment_loss) by autograd; the loss is multiplied by `grad_scale` before
    the backward and the gradients divided by it afterwards (a power of two: exact)"""
    Q = {k: v.detach().to(dtype).clone().requires_grad_(k.startswith(TRAINED)) for k, v in P.items()}
    rl, cl, _, _ = objective(Q, cfg, x.to(dtype), ids, l1_weight, fp16_storage, l1_signs)
    ((rl + cl) * grad_scale).backward()
    return {k: (Q[k].grad / grad_scale).double().numpy() for k in trained_names(Q)}, float(rl.detach()), float(cl.detach())


def default_scale(l1_weight, n_video):
    """mebt_amd.vqgan.VQGAN.default_grad_scale"""
    return 2.0 ** math.floor(math.log2(0.125 / (l1_weight / n_video)))


# ---- the data-gradient plan, walked in numpy ---------------------------------------------------------------------------------------------
def run_dgrad_plan(cv, dims, dy):
    """`cv` a `_Conv` (CPU, fp32), dy float64 numpy [B, *out_dims, Cout] -> dx [B, *dims, Cin] through the plan exactly as the GPU path
    walks it: zero box (mebt_op_pad_zero), one clamped-gather convolution per class onto the lattice (mebt_op_conv3d's descriptor rule,
    out_mode 1), fold (mebt_op_halo_fold)."""
    plan = cv.dgrad_plan(dims)
    B = dy.shape[0]
    od = cv.out_dims(dims)
    fz, zd, pd, fr = plan["fz"], plan["zd"], plan["pd"], plan["front"]
    dyz = np.zeros((B, *zd, cv.cout))
    dyz[:, fz[0]:fz[0] + od[0], fz[1]:fz[1] + od[1], fz[2]:fz[2] + od[2]] = dy
    dxp = np.zeros((B, *pd, cv.cin))
    written = np.zeros(pd, dtype=np.int64)
    for c in plan["classes"]:
        if c["w"] is None:
            continue
        w = c["w"].double().numpy()                                               # [Cin][n][Cout]
        for q in itertools.product(*[range(n) for n in c["cq"]]):
            acc = np.zeros((B, cv.cin))
            for j, t in enumerate(c["taps"]):
                pos = [min(max(q[k] * c["sm"][k] + t[k], 0), zd[k] - 1) for k in range(3)]
                assert all(0 <= q[k] * c["sm"][k] + t[k] < zd[k] for k in range(3)), "a tap leaves the zero box: the clamp would act"
                acc += dyz[:, pos[0], pos[1], pos[2]] @ w[:, j, :].T
            o = tuple(q[k] * c["os"][k] + c["pi"][k] for k in range(3))
            dxp[:, o[0], o[1], o[2]] = acc
            written[o] += 1
    live = np.ones(pd, dtype=bool)
    for c in plan["classes"]:
        if c["w"] is None:                                                          # a parity no tap reaches stays zero
            sl = tuple(slice(c["pi"][k], None, c["os"][k]) for k in range(3))
            live[sl] = False
    assert (written[live] == 1).all() and (written[~live] == 0).all(), "the classes must tile the lattice"
    dx = np.zeros((B, *dims, cv.cin))
    for q in itertools.product(*[range(n) for n in pd]):
        i = tuple(min(max(q[k] - fr[k], 0), dims[k] - 1) for k in range(3))
        dx[:, i[0], i[1], i[2]] += dxp[:, q[0], q[1], q[2]]
    return dx


def scatter_dgrad(cv, dims, dy):
    """the same gradient by scattering through the FORWARD's own rule: every (output voxel, tap) adds w^T dy onto clamp(o' sm + tap)"""
    B = dy.shape[0]
    od = cv.out_dims(dims)
    dx = np.zeros((B, *dims, cv.cin))
    for pi, taps, w in cv.classes:
        wn = w.double().numpy()                                                    # [Cout][n][Cin]
        for o in itertools.product(*[range(n) for n in cv.class_counts(od, pi)]):
            ov = tuple(o[k] * cv.os[k] + pi[k] for k in range(3))
            g = dy[:, ov[0], ov[1], ov[2]]
            for j, t in enumerate(taps):
                i = tuple(min(max(o[k] * cv.sm[k] + t[k], 0), dims[k] - 1) for k in range(3))
                dx[:, i[0], i[1], i[2]] += g @ wn[:, j, :]
    return dx
