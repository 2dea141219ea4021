"""Reading an attention-dropout mask out of the attention outputs, exactly (shared by tests/test_gpu_attention_ops.py and the CPU
proof in tests/test_host_attention_readout.py; test infrastructure, no GPU needed to import).

Every softmax probability is strictly positive, so with a one-hot selector as one operand an output element is non-zero exactly
where ONE chosen mask element keeps.  With W = the head size and w a window of W keys (or queries):

  o[q, e]     V[key, e] = 1 iff key == W w + e                                   = P[q, W w + e] keep(q, W w + e)
  dQ[q, e]    K[key, e] = 1 iff key == W w + e, V and dO all ones, o given as 0  = P keep(q, W w + e) dP / sqrt(W),  dP = W
  dV[key, e]  dO[q, e] = 1 iff q == W w + e                                      = P[W w + e, key] keep(W w + e, key)
  dK[key, e]  Q[q, e] = 1 iff q == W w + e, V and dO all ones, o given as 0      = P keep(W w + e, key) dP / sqrt(W)

The backward is handed o = 0, which makes delta = rowsum(dO o O) = 0 and dS = P keep dP / sqrt(W): every kernel of this project
computes delta from the o it is given (attention.hip attn_bwd_dq_generic, which also writes it for attn_bwd_dkv_generic;
attention_mfma.hip bwd_dq_block and, in the one-grid backward, bwd_dkv_block<OWN_DELTA> through row_delta).

`fwd(q, k, v) -> (o, lse)` and `bwd(q, k, v, o, lse, do) -> (dq, dk, dv)` take and return float tensors [B, N, H * W] (lse in
whatever form the pair agrees on)."""
import math

import numpy as np
import torch


def selector(B, rows, H, W, w):
    """[B, rows, H * W]: 1 where row == W w + e (every sample, every head)"""
    s = torch.zeros(B, rows, H, W)
    for e in range(W):
        if W * w + e < rows:
            s[:, W * w + e, :, e] = 1.0
    return s.reshape(B, rows, H * W)


def heads(x, H):
    """[B, N, H * W] -> [B, H, N, W]"""
    B, N, C = x.shape
    return x.reshape(B, N, H, C // H).transpose(1, 2)


def read_masks(fwd, bwd, B, H, NQ, NK, W, seed=0):
    """The keep pattern [B, H, NQ, NK] (bool) as read from o, dQ, dK and dV: a dict of four arrays.  2 * ceil(NK / W) forwards +
    ceil(NK / W) backwards for o and dQ, 1 + ceil(NQ / W) forwards + 2 * ceil(NQ / W) backwards for dK and dV."""
    g = torch.Generator().manual_seed(1000 + seed)
    C = H * W
    # small magnitudes: the probabilities stay within a small factor of uniform, nothing underflows in bf16
    qr, kr, vr = (0.1 * torch.randn(B, n, C, generator=g) for n in (NQ, NK, NK))
    ones_q, ones_k, zero_o = torch.ones(B, NQ, C), torch.ones(B, NK, C), torch.zeros(B, NQ, C)
    got = {name: torch.zeros(B, H, NQ, NK, dtype=torch.bool) for name in ("o", "dq", "dk", "dv")}
    for w in range((NK + W - 1) // W):
        n = min(W, NK - W * w)
        sel = selector(B, NK, H, W, w)
        o, _ = fwd(qr, kr, sel)
        got["o"][..., W * w:W * w + n] = heads(o, H)[..., :n] != 0
        _, lse = fwd(qr, sel, ones_k)
        dq, _, _ = bwd(qr, sel, ones_k, zero_o, lse, ones_q)
        got["dq"][..., W * w:W * w + n] = heads(dq, H)[..., :n] != 0
    _, lse_r = fwd(qr, kr, vr)
    for w in range((NQ + W - 1) // W):
        n = min(W, NQ - W * w)
        sel = selector(B, NQ, H, W, w)
        _, _, dv = bwd(qr, kr, vr, zero_o, lse_r, sel)
        got["dv"][:, :, W * w:W * w + n, :] = (heads(dv, H)[..., :n] != 0).transpose(-1, -2)
        _, lse = fwd(sel, kr, ones_k)
        _, dk, _ = bwd(sel, kr, ones_k, zero_o, lse, ones_q)
        got["dk"][:, :, W * w:W * w + n, :] = (heads(dk, H)[..., :n] != 0).transpose(-1, -2)
    return got


def ref_attention(qq, kk, vv, H, mask=None):
    """softmax(q k^T / sqrt(hd)) [* mask] v in the operands' precision (fp64 in the tests): tests/test_gpu_ops.py attn_ref with the
    reference's attention dropout (gpt.py:135, a 0 / inv_keep mask [B, H, NQ, NK] on the normalised probabilities)"""
    B, NQ, C = qq.shape
    qh, kh, vh = heads(qq, H), heads(kk, H), heads(vv, H)
    att = torch.softmax(qh @ kh.transpose(-2, -1) / math.sqrt(C // H), dim=-1)
    if mask is not None:
        att = att * mask
    return (att @ vh).transpose(1, 2).reshape(B, NQ, C)


def ref_pair(mask, H):
    """(fwd, bwd) of the fp64 reference with dropout mask `mask`, in the flash form the kernels use: the forward returns the
    log-sum-exp, the backward recomputes P from it and takes delta from the o it is GIVEN."""
    mask = mask.double()

    def fwd(q, k, v):
        q, k, v = q.double(), k.double(), v.double()
        s = heads(q, H) @ heads(k, H).transpose(-2, -1) / math.sqrt(q.shape[-1] // H)
        return ref_attention(q, k, v, H, mask), torch.logsumexp(s, dim=-1)

    def bwd(q, k, v, o, lse, do):
        B, NQ, C = q.shape
        scale = 1.0 / math.sqrt(C // H)
        qh, kh, vh, oh, gh = (heads(x.double(), H) for x in (q, k, v, o, do))
        p = torch.exp(qh @ kh.transpose(-2, -1) * scale - lse[..., None])
        delta = (gh * oh).sum(-1, keepdim=True)
        ds = p * ((gh @ vh.transpose(-2, -1)) * mask - delta) * scale
        back = lambda x: x.transpose(1, 2).reshape(B, -1, C)
        return back(ds @ kh), back(ds.transpose(-2, -1) @ qh), back((p * mask).transpose(-2, -1) @ gh)

    return fwd, bwd


def decode_dmask(words, B, H, NQ, NK):
    """AttnParams::dmask (csrc/kernels.h) as a [B, H, NQ, NK] boolean array: 16-bit fields [(b * H + h)][q][key tile of 64, padded to
    a multiple of 4 tiles][g = 0..3], field bit 4 kb + r <-> key 64 tile + 16 kb + 4 g + r.  `words`: the buffer as a flat integer
    array of 16-bit fields."""
    mt = 4 * ((NK + 255) // 256)
    f = np.asarray(words).astype(np.int64).reshape(B, H, NQ, mt, 4) & 0xFFFF
    bits = (f[..., None] >> np.arange(16)) & 1                           # [B, H, NQ, tile, g, 4 kb + r]
    bits = bits.reshape(B, H, NQ, mt, 4, 4, 4).transpose(0, 1, 2, 3, 5, 4, 6)    # -> [.., tile, kb, g, r]
    return bits.reshape(B, H, NQ, mt * 64)[..., :NK].astype(bool)

