"""CPU proof of the constructions tests/test_gpu_attention_ops.py relies on (tests/attn_readout.py): the one-hot selectors read an
arbitrary attention-dropout mask back from o, dQ, dK and dV of the fp64 reference exactly, the reference's flash-form backward is the
autograd backward, and the keep-bit decode follows the layout csrc/kernels.h documents.  No GPU."""
import numpy as np
import pytest
import torch

from tests.attn_readout import decode_dmask, read_masks, ref_attention, ref_pair


@pytest.mark.parametrize("B,H,NQ,NK,W", [(1, 3, 200, 1, 64), (2, 2, 33, 63, 64), (2, 2, 33, 65, 64), (1, 2, 129, 257, 64), (2, 2, 70, 45, 32)])
def test_selectors_read_a_random_mask_back_exactly(B, H, NQ, NK, W):
    g = torch.Generator().manual_seed(NQ * 7919 + NK)
    keep = torch.rand(B, H, NQ, NK, generator=g) >= 0.25
    assert 0 < int(keep.sum()) < keep.numel() or NK == 1
    fwd, bwd = ref_pair(keep * (4.0 / 3.0), H)
    got = read_masks(fwd, bwd, B, H, NQ, NK, W)
    for name in ("o", "dq", "dk", "dv"):
        assert torch.equal(got[name], keep), name
    # and a read-out does notice one wrong element: the same mask with one element flipped is not what is read
    other = keep.clone()
    other[-1, -1, NQ // 2, NK // 2] ^= True
    assert not torch.equal(got["dv"], other)


def test_reference_flash_backward_is_the_autograd_backward():
    """ref_pair's backward (P recomputed from the log-sum-exp, delta = rowsum(dO o O) of the o it is given) equals autograd through
    softmax(...) * mask @ v when it is given the forward's own o"""
    B, H, NQ, NK, W = 2, 2, 37, 71, 32
    g = torch.Generator().manual_seed(5)
    q, k, v, do = (torch.randn(B, n, H * W, generator=g, dtype=torch.float64) for n in (NQ, NK, NK, NQ))
    mask = (torch.rand(B, H, NQ, NK, generator=g) >= 0.25) * (4.0 / 3.0)
    fwd, bwd = ref_pair(mask, H)
    o, lse = fwd(q, k, v)
    dq, dk, dv = bwd(q, k, v, o, lse, do)
    qa, ka, va = (x.clone().requires_grad_(True) for x in (q, k, v))
    (ref_attention(qa, ka, va, H, mask.double()) * do).sum().backward()
    for got, ref in ((dq, qa.grad), (dk, ka.grad), (dv, va.grad)):
        assert (got - ref).abs().max() < 1e-12


def test_decode_dmask_follows_the_documented_layout():
    """field [(b H + h)][q][tile, padded to 4][g], bit 4 kb + r <-> key 64 tile + 16 kb + 4 g + r: single keys by hand"""
    B, H, NQ, NK = 2, 3, 5, 365 + 1
    mt = 8                                            # ceil(366 / 256) chunks of 4 tiles
    words = np.zeros((B * H, NQ, mt, 4), dtype=np.uint16)
    # key 365 = 64 * 5 + 16 * 2 + 4 * 3 + 1 of (b 1, h 2, q 4); key 0 of (b 0, h 0, q 0); key 79 = 64 + 0 + 4 * 3 + 3 of (b 0, h 1, q 2)
    words[1 * H + 2, 4, 5, 3] = 1 << (4 * 2 + 1)
    words[0, 0, 0, 0] = 1
    words[1, 2, 1, 3] = 1 << 3
    words[1, 2, 6, :] = 0xFFFF                        # a padding tile: keys 384 .. 447 are beyond NK and must not appear
    keep = decode_dmask(words.reshape(-1), B, H, NQ, NK)
    assert keep.shape == (B, H, NQ, NK) and keep.sum() == 3
    assert keep[1, 2, 4, 365] and keep[0, 0, 0, 0] and keep[0, 1, 2, 79]
