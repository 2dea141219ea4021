"""Launch forms of the bf16 MFMA attention: the XCD-local block order and the one-grid backward compute exactly what the linear
order and the two-launch backward compute (bit for bit, with and without attention dropout), and the block order is a bijection
for any grid size.  GPU only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from mebt_amd import _lib
from mebt_amd._lib import check, ptr, cur_stream

DEV = "cuda"
HD = 64


def lib():
    return _lib.load()


def run(B, H, NQ, NK, p_drop, legacy):
    """forward + backward under the launch form `legacy` (mebt_debug_attn_legacy bits); fixed seeded inputs"""
    L = lib()
    C = H * HD
    g = torch.Generator().manual_seed(NQ * 7919 + NK)
    q = torch.randn(B, NQ, C, generator=g).bfloat16().to(DEV)
    kv = torch.randn(B, NK, 2 * C, generator=g).bfloat16().to(DEV)
    do = torch.randn(B, NQ, C, generator=g).bfloat16().to(DEV)
    o = torch.full((B, NQ, C), float("nan"), device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(B, H, NQ, device=DEV)
    dq = torch.full((B, NQ, C), float("nan"), device=DEV, dtype=torch.bfloat16)
    dkv = torch.full((B, NK, 2 * C), float("nan"), device=DEV, dtype=torch.bfloat16)
    delta = torch.empty(B, H, NQ, device=DEV)
    dmask = torch.zeros(B * H * NQ * 32 * ((NK + 255) // 256), dtype=torch.uint8, device=DEV)
    vp, dvp = kv.data_ptr() + C * 2, dkv.data_ptr() + C * 2
    L.mebt_debug_attn_legacy(legacy)
    L.mebt_debug_attn_dropout(4321, p_drop, ptr(dmask))
    try:
        check(L.mebt_op_attention_fwd(_lib.BF16, ptr(q), ptr(kv), vp, ptr(o), ptr(lse), B, H, NQ, NK, HD, C, 2 * C, 2 * C, C, 0, cur_stream()))
        check(L.mebt_op_attention_bwd(_lib.BF16, ptr(q), ptr(kv), vp, ptr(o), ptr(lse), ptr(do), ptr(dq), ptr(dkv), dvp, ptr(delta),
                                      B, H, NQ, NK, HD, C, 2 * C, 2 * C, C, 0, cur_stream()))
        torch.cuda.synchronize()
    finally:
        L.mebt_debug_attn_dropout(0, 0.0, None)
        L.mebt_debug_attn_legacy(-1)
    return o.cpu(), lse.cpu(), dq.cpu(), dkv.cpu(), dmask.cpu()


def same_bits(a, b):
    return torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                       b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32))


# the four Sky-16f train-step routings (B = 6, H = 16) and ragged shapes
SHAPES = [(6, 16, 256, 512), (6, 16, 256, 256), (6, 16, 512, 256), (6, 16, 256, 768), (5, 16, 300, 769), (9, 16, 128, 200),
          (1, 2, 600, 70)]


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("B,H,NQ,NK", SHAPES)
def test_launch_forms_bit_identical(B, H, NQ, NK, p_drop):
    ref = run(B, H, NQ, NK, p_drop, 3)                     # linear order, two-launch backward
    for legacy in (0, 1, 2):
        got = run(B, H, NQ, NK, p_drop, legacy)
        for name, a, b in zip(("o", "lse", "dq", "dkv", "dmask"), ref, got):
            assert not torch.isnan(b.float()).any(), (legacy, name)
            assert same_bits(a, b), (legacy, name)


def test_block_order_bijective():
    """every (x, h, b) of a T-block grid is taken by exactly one workgroup, for T = 1 .. 4096; in the XCD-local order the ids of
    one XCD (id & 7) take one contiguous run of the linear order"""
    L = lib()
    for T in range(1, 4097):
        for X, H in ((1, 1), (T, 1), (1, T)) + (((2, T // 2),) if T % 2 == 0 else ()) + (((3, T // 3),) if T % 3 == 0 else ()):
            for xcd in (0, 1):
                out = torch.full((T,), -1, dtype=torch.int32, device=DEV)
                check(L.mebt_debug_attn_block_order(T, X, H, xcd, ptr(out), cur_stream()))
                ids = out.cpu()
                assert torch.equal(ids.sort().values, torch.arange(T, dtype=torch.int32)), (T, X, H, xcd)
                if xcd:
                    assert bool(((ids & 7)[1:] >= (ids & 7)[:-1]).all()), (T, X, H)
                else:
                    assert torch.equal(ids, torch.arange(T, dtype=torch.int32))
