"""The attention operators where the rest of the suite cannot see an error: attention dropout element by element (the keep bits the
MFMA forward writes, and the mask every kernel really applied, read out of o / dQ / dK / dV exactly), values with dropout against
fp64, the 64-bit hash path, gathered keys (AttnParams::kidx) at operator level in every forward form, and the forward forms that
only a switch selects.  The constructions are proved on the CPU in tests/test_host_attention_readout.py.  GPU only."""
import ctypes
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mebt_amd import _lib
from mebt_amd._lib import ptr, cur_stream
from tests.attn_readout import decode_dmask, read_masks, ref_attention
from tests.helpers import record_measured
from tests.test_gpu_dropout import kernel_mask
from tests.test_gpu_ops import q as quant, rnd, tdt

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = _lib.F32, _lib.BF16
ESHAPE = 2                           # include/mebt_hip.h MEBT_STATUS_ESHAPE
SEED, P_DROP, INV_KEEP = 0x1234ABCD5, 0.25, 4.0 / 3.0        # p = 0.25 is exact in the 16-bit threshold

# (B, H, NQ, NK), head size 64, and the forward form launch_attn_fwd_mfma selects: (waves per group, ring stages, split)
FORM_42, FORM_PP, FORM_81, FORM_82 = (4, 2, 0), (4, 2, 1), (8, 1, 0), (8, 2, 0)
SHAPES = [(1, 3, 200, 1), (2, 2, 33, 63), (2, 2, 33, 64), (2, 2, 33, 65), (1, 2, 129, 257), (1, 1, 300, 769), (1, 2, 200, 3001),
          (9, 16, 128, 200), (5, 16, 300, 769)]
FORM = {(1, 2, 200, 3001): FORM_PP, (9, 16, 128, 200): FORM_81, (5, 16, 300, 769): FORM_82, (2, 1, 64, 1025): FORM_PP, (1, 1, 64, 8192): FORM_PP}
SMALL = SHAPES[:5]
READOUT_SHAPES = [(1, 3, 200, 1), (2, 2, 33, 63), (2, 2, 33, 65), (1, 2, 129, 257), (1, 1, 130, 769)]
GATHER_SHAPES = [(2, 2, 70, 130), (1, 3, 200, 1), (1, 2, 129, 257), (2, 1, 64, 1025), (1, 2, 200, 3001), (9, 16, 128, 200),
                 (5, 16, 300, 769), (1, 1, 64, 8192)]


def lib():
    return _lib.load()


def form_of(shape):
    return FORM.get(tuple(shape), FORM_42)


def last_form():
    """(MFMA forward launches since the previous call, (waves, stages, split) of the last, its grid)"""
    out = (ctypes.c_int32 * 4)()
    n = lib().mebt_debug_attn_last_launch(out)
    return n, tuple(out[:3]), out[3]


def dmask_buffer(B, H, NQ, NK):
    """the keep-bit buffer of a shape (mebt_debug_attn_dropout's size), prefilled with a bit pattern: what a kernel leaves unwritten is not zero"""
    return torch.full((B * H * NQ * 32 * ((NK + 255) // 256),), 0xA5, dtype=torch.uint8, device=DEV)


def dmask_words(dmask):
    return dmask.cpu().numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def mask_of(shape):
    """the 0 / inv_keep attention-dropout mask [B, H, NQ, NK] of (SEED, site 0, P_DROP), from the elementwise kernel's hash"""
    return kernel_mask(SEED, 0, P_DROP, tuple(shape))


class Op:
    """mebt_op_attention_fwd / _bwd of one shape and path on CPU float tensors [B, N, H * hd]; k|v (and dk|dv) interleaved per row
    as the engine packs them.  p > 0: attention dropout under SEED, with a keep-bit buffer (`bits`) or hashed everywhere; `legacy`:
    mebt_debug_attn_legacy bits (2 = the two-launch backward)."""

    def __init__(self, dtype, generic, B, H, NQ, NK, HD=64, p=0.0, bits=False, legacy=0):
        self.dtype, self.generic, self.dims, self.p, self.legacy = dtype, generic, (B, H, NQ, NK, HD), p, legacy
        self.dmask = dmask_buffer(B, H, NQ, NK) if bits else None
        self.t = tdt(dtype)

    def _call(self, fn):
        L = lib()
        L.mebt_debug_attn_legacy(self.legacy)
        L.mebt_debug_attn_dropout(SEED, self.p, ptr(self.dmask))
        try:
            rc = fn(L)
            torch.cuda.synchronize()
        finally:
            L.mebt_debug_attn_dropout(0, 0.0, None)
            L.mebt_debug_attn_legacy(-1)
        _lib.check(rc)

    def fwd_dev(self, qd, kvd, kidx=None, kidx_rows=0):
        """device tensors in, (o, lse) on the device out (NaN-prefilled); kidx: gathered keys (mebt_op_attention_fwd_gather)"""
        B, H, NQ, NK, HD = self.dims
        C = H * HD
        o = torch.full((B, NQ, C), float("nan"), device=DEV, dtype=self.t)
        lse = torch.full((B, H, NQ), float("nan"), device=DEV)
        vp = kvd.data_ptr() + C * kvd.element_size()
        if kidx is None:
            self._call(lambda L: L.mebt_op_attention_fwd(self.dtype, ptr(qd), ptr(kvd), vp, ptr(o), ptr(lse), B, H, NQ, NK, HD, C, 2 * C, 2 * C, C,
                                                         self.generic, cur_stream()))
        else:
            self._call(lambda L: L.mebt_op_attention_fwd_gather(self.dtype, ptr(qd), ptr(kvd), vp, ptr(o), ptr(lse), B, H, NQ, NK, HD, C, 2 * C,
                                                                2 * C, C, self.generic, ptr(kidx), kidx_rows, cur_stream()))
        return o, lse

    def bwd_dev(self, qd, kvd, o, lse, dod):
        B, H, NQ, NK, HD = self.dims
        C = H * HD
        dq = torch.full((B, NQ, C), float("nan"), device=DEV, dtype=self.t)
        dkv = torch.full((B, NK, 2 * C), float("nan"), device=DEV, dtype=self.t)
        delta = torch.empty(B, H, NQ, device=DEV)
        vp, dvp = kvd.data_ptr() + C * kvd.element_size(), dkv.data_ptr() + C * dkv.element_size()
        self._call(lambda L: L.mebt_op_attention_bwd(self.dtype, ptr(qd), ptr(kvd), vp, ptr(o), ptr(lse), ptr(dod), ptr(dq), ptr(dkv), dvp, ptr(delta),
                                                     B, H, NQ, NK, HD, C, 2 * C, 2 * C, C, self.generic, cur_stream()))
        return dq, dkv

    def dev(self, x):
        return x.to(DEV, self.t).contiguous()

    # the (fwd, bwd) pair of tests/attn_readout.py
    def fwd(self, qq, kk, vv):
        o, lse = self.fwd_dev(self.dev(qq), self.dev(torch.cat([kk, vv], -1)))
        return o.float().cpu(), lse

    def bwd(self, qq, kk, vv, o, lse, do):
        C = qq.shape[-1]
        dq, dkv = self.bwd_dev(self.dev(qq), self.dev(torch.cat([kk, vv], -1)), self.dev(o), lse, self.dev(do))
        dkv = dkv.float().cpu()
        return dq.float().cpu(), dkv[..., :C], dkv[..., C:]


def inputs(B, H, NQ, NK, dtype, HD=64):
    """random operands quantised as in test_attention_fwd_bwd: q, k|v, dO"""
    C = H * HD
    return quant(rnd(B, NQ, C, seed=1), dtype), quant(rnd(B, NK, 2 * C, seed=2), dtype), quant(rnd(B, NQ, C, seed=3), dtype)


@functools.lru_cache(maxsize=None)
def reference(shape, dtype):
    """fp64: o = (softmax(q k^T / 8) * mask) v on the operands of inputs(), and the gradients of sum(o * dO) by autograd"""
    B, H, NQ, NK = shape
    C = H * 64
    qq, kv, do = inputs(B, H, NQ, NK, dtype)
    qr, kvr = qq.double().requires_grad_(True), kv.double().requires_grad_(True)
    o = ref_attention(qr, kvr[..., :C], kvr[..., C:], H, mask_of(shape).double())
    (o * do.double()).sum().backward()
    return o.detach(), qr.grad, kvr.grad


# ---- (a) the keep bits the MFMA forward writes are the hash's ------------------------------------------------------------------------

def test_shapes_select_every_default_form():
    assert {form_of(s) for s in SHAPES} == {FORM_42, FORM_PP, FORM_81, FORM_82}


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_keep_bits_are_the_hash(shape):
    """AttnParams::dmask decoded by the layout csrc/kernels.h documents equals the elementwise kernel's mask of the same (seed, site,
    p) for every key below NK; the form that ran is the one the shape list counts on"""
    B, H, NQ, NK = shape
    op = Op(BF16, 0, B, H, NQ, NK, p=P_DROP, bits=True)
    qq, kv, _ = inputs(B, H, NQ, NK, BF16)
    last_form()
    op.fwd_dev(op.dev(qq), op.dev(kv))
    n, form, grid = last_form()
    print("forward form of", shape, ":", form, "grid", grid)
    assert (n, form) == (1, form_of(shape))
    keep = torch.from_numpy(decode_dmask(dmask_words(op.dmask), B, H, NQ, NK))
    want = mask_of(shape) > 0
    assert abs(want.float().mean().item() - 0.75) < 0.05 or want.numel() < 5000
    assert torch.equal(keep, want), (keep != want).nonzero()[:8]


# ---- (b) the mask every kernel applied, read out of its outputs ----------------------------------------------------------------------

PATHS = {       # dtype, force_generic, keep-bit buffer, mebt_debug_attn_legacy
    "generic-f32": (F32, 1, False, 0), "generic-bf16": (BF16, 1, False, 0),
    "mfma-bits-one-grid": (BF16, 0, True, 0), "mfma-hash-one-grid": (BF16, 0, False, 0),
    "mfma-bits-two-launch": (BF16, 0, True, 2), "mfma-hash-two-launch": (BF16, 0, False, 2),
}


READOUT_CASES = [(path, s + (64,)) for path in PATHS for s in READOUT_SHAPES] + [(path, (2, 2, 70, 45, 32)) for path in PATHS if PATHS[path][1]]


@pytest.mark.parametrize("path,shape", READOUT_CASES, ids=str)
def test_mask_read_out_of_the_outputs(path, shape):
    """o, dQ, dK and dV are non-zero exactly where the hash keeps (tests/attn_readout.py).  Every kernel takes delta from the o it is
    given, so the one construction fits all of them.  Head size 32 exists on the generic kernels only."""
    B, H, NQ, NK, HD = shape
    dtype, generic, bits, legacy = PATHS[path]
    op = Op(dtype, generic, B, H, NQ, NK, HD, p=P_DROP, bits=bits, legacy=legacy)
    got = read_masks(op.fwd, op.bwd, B, H, NQ, NK, HD)
    want = mask_of((B, H, NQ, NK)) > 0
    for name in ("o", "dq", "dk", "dv"):
        assert torch.equal(got[name], want), (name, (got[name] != want).nonzero()[:8])


# ---- (c) values with dropout against fp64 --------------------------------------------------------------------------------------------

def assert_values(tag, shape, dtype, tol, o, dq, dkv):
    """test_attention_fwd_bwd's bounds times inv_keep: each kept probability is scaled by exactly that factor, so the absolute error
    of a sum grows by at most that factor"""
    ro, rdq, rdkv = reference(tuple(shape), dtype)
    errs = {"o": ((o.float().cpu().double() - ro).abs().max().item(), tol * INV_KEEP),
            "dq": ((dq.float().cpu().double() - rdq).abs().max().item(), tol * 4 * max(1.0, rdq.abs().max().item()) * INV_KEEP),
            "dkv": ((dkv.float().cpu().double() - rdkv).abs().max().item(), tol * 4 * max(1.0, rdkv.abs().max().item()) * INV_KEEP)}
    for name, (err, gate) in errs.items():
        print(f"{tag} {shape} {name}: max error {err:.3e}, bound {gate:.3e}")
        record_measured(f"attn_dropout/{tag}/{'x'.join(map(str, shape))}/{name}", err, gate)
    for name, (err, gate) in errs.items():
        assert err < gate, (name, err, gate)


def run_values(op, shape, dtype):
    qq, kv, do = inputs(*shape, dtype)
    qd, kvd = op.dev(qq), op.dev(kv)
    o, lse = op.fwd_dev(qd, kvd)
    dq, dkv = op.bwd_dev(qd, kvd, o, lse, op.dev(do))
    return o, lse, dq, dkv


@pytest.mark.parametrize("shape", SMALL, ids=str)
@pytest.mark.parametrize("dtype,tol", [(F32, 2e-5), (BF16, 2e-2)])
def test_dropout_values_generic(dtype, tol, shape):
    op = Op(dtype, 1, *shape, p=P_DROP)
    o, _, dq, dkv = run_values(op, shape, dtype)
    assert_values("generic-f32" if dtype == F32 else "generic-bf16", shape, dtype, tol, o, dq, dkv)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_dropout_values_mfma(shape):
    """with the keep-bit buffer and with the hash everywhere: both within the bound of fp64, and equal bit for bit (either way a
    probability is multiplied by the same inv_keep or by 0)"""
    hashed = run_values(Op(BF16, 0, *shape, p=P_DROP), shape, BF16)
    staged = run_values(Op(BF16, 0, *shape, p=P_DROP, bits=True), shape, BF16)
    assert_values("mfma-hash", shape, BF16, 2e-2, hashed[0], hashed[2], hashed[3])
    assert_values("mfma-bits", shape, BF16, 2e-2, staged[0], staged[2], staged[3])
    for name, a, b in zip(("o", "lse", "dq", "dkv"), hashed, staged):
        assert torch.equal(a, b), name


# ---- (d) the 64-bit hash path --------------------------------------------------------------------------------------------------------

def bits16(x):
    return x.cpu().view(torch.int16).numpy() if x.dtype == torch.bfloat16 else x.cpu().numpy()


def dropout_run(shape):
    """o, lse, dq, dkv, dmask of the MFMA kernels at p = P_DROP, as integer / fp32 arrays"""
    op = Op(BF16, 0, *shape, p=P_DROP, bits=True)
    o, lse, dq, dkv = run_values(op, shape, BF16)
    return {"o": bits16(o), "lse": bits16(lse), "dq": bits16(dq), "dkv": bits16(dkv), "dmask": op.dmask.cpu().numpy()}


def run_child(mode, env):
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, mode + ".npz")
        out = subprocess.run([sys.executable, "-m", "tests.test_gpu_attention_ops", mode, path], cwd=ROOT, env=dict(os.environ, **env),
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        with np.load(path) as f:
            return {k: f[k] for k in f.files}


def test_drop_small_off_is_bit_identical():
    """MEBT_DROP_SMALL=0 (read once per process: a child) hashes with the 64-bit pair index, the path sites of 2^33 elements and more
    take; at a small site it must give what the 32-bit path gives"""
    shape = (1, 1, 300, 769)
    child = run_child("drop_small", {"MEBT_DROP_SMALL": "0"})
    here = dropout_run(shape)
    for name, a in here.items():
        assert np.array_equal(a, child[name]), name


# ---- (e) gathered keys ---------------------------------------------------------------------------------------------------------------

def gather_case(B, H, NQ, NK, seed=11):
    """q [B, NQ, C]; a cache of R = NK + 37 rows of k|v per sample; kidx [B, NK], a different random selection per sample in random
    order that contains row 0 and row R - 1 (NK = 1: row R - 1 alone), sample 0's with one repeated row (NK >= 4); every cache row
    that no list names is NaN.  Returns also the pre-gathered contiguous k|v."""
    C, R = H * 64, NK + 37
    g = torch.Generator().manual_seed(seed * 100003 + NK)
    qq = quant(rnd(B, NQ, C, seed=seed), BF16)
    cache = quant(torch.randn(B, R, 2 * C, generator=g), BF16)
    kidx = torch.empty(B, NK, dtype=torch.int64)
    for b in range(B):
        if NK == 1:
            rows = torch.tensor([R - 1])
        else:
            inner = torch.randperm(R - 2, generator=g)[:NK - 2] + 1
            if b == 0 and NK >= 4:
                inner[1] = inner[0]
            rows = torch.cat([torch.tensor([0, R - 1]), inner])[torch.randperm(NK, generator=g)]
        kidx[b] = rows
        unused = torch.ones(R, dtype=torch.bool)
        unused[rows] = False
        cache[b, unused] = float("nan")
    kv = torch.stack([cache[b, kidx[b]] for b in range(B)])
    assert not torch.isnan(kv).any() and torch.isnan(cache).any()
    return qq, cache, kidx.int(), kv


def gathered_and_plain(shape):
    """(o, lse) of the gathered forward and of the plain forward on the pre-gathered copy, and the forms that ran"""
    B, H, NQ, NK = shape
    qq, cache, kidx, kv = gather_case(B, H, NQ, NK)
    op = Op(BF16, 0, B, H, NQ, NK)
    qd = op.dev(qq)
    last_form()
    plain = op.fwd_dev(qd, op.dev(kv))
    form_plain = last_form()
    # the lists sit at the front of B * kidx_rows zeroed entries: a kernel that strides them by kidx_rows instead of NK reads other
    # samples' entries or row 0, never beyond the allocation
    pool = torch.zeros(B * (NK + 37), dtype=torch.int32, device=DEV)
    pool[:B * NK] = kidx.reshape(-1).to(DEV)
    gathered = op.fwd_dev(qd, op.dev(cache), pool, NK + 37)
    form_gathered = last_form()
    return gathered, plain, form_gathered, form_plain


@pytest.mark.parametrize("shape", GATHER_SHAPES, ids=str)
def test_gathered_keys(shape):
    """mebt_op_attention_fwd_gather on a cache with NaN in every row no list names: o and lse bit for bit those of the plain forward
    on the pre-gathered copy (the same form, by the hook), and o within the bf16 bound of fp64 on the gathered rows"""
    B, H, NQ, NK = shape
    (o, lse), (o_p, lse_p), form, form_p = gathered_and_plain(shape)
    print("forward form of", shape, "gathered:", form[1], "grid", form[2])
    assert form == form_p and form[:2] == (1, form_of(shape))
    assert not torch.isnan(o.float()).any() and not torch.isnan(lse).any()
    assert torch.equal(o, o_p) and torch.equal(lse, lse_p)
    qq, _, _, kv = gather_case(B, H, NQ, NK)
    C = H * 64
    ref = ref_attention(qq.double(), kv[..., :C].double(), kv[..., C:].double(), H)
    assert (o.float().cpu().double() - ref).abs().max() < 2e-2


def test_gathered_keys_argument_checks():
    L = lib()
    B, H, NQ, C = 1, 1, 64, 64

    def call(dtype, NK, generic):
        t = tdt(dtype)
        qd = torch.zeros(B, NQ, C, device=DEV, dtype=t)
        cache = torch.zeros(B, NK + 37, 2 * C, device=DEV, dtype=t)
        kidx = torch.zeros(B, NK, device=DEV, dtype=torch.int32)
        o = torch.zeros(B, NQ, C, device=DEV, dtype=t)
        lse = torch.zeros(B, H, NQ, device=DEV)
        rc = L.mebt_op_attention_fwd_gather(dtype, ptr(qd), ptr(cache), cache.data_ptr() + C * cache.element_size(), ptr(o), ptr(lse), B, H, NQ, NK,
                                            64, C, 2 * C, 2 * C, C, generic, ptr(kidx), NK + 37, cur_stream())
        torch.cuda.synchronize()
        return rc, L.mebt_last_error().decode()

    assert call(BF16, 8193, 0) == (ESHAPE, "mfma attention: a gathered key set holds at most 8192 keys")
    generic_msg = "attention: gathered keys / values (kidx) need the MFMA forward (bf16, head size 64)"
    assert call(BF16, 130, 1) == (ESHAPE, generic_msg)
    assert call(F32, 130, 0) == (ESHAPE, generic_msg)


# ---- (f) the forward forms behind switches -------------------------------------------------------------------------------------------

SWITCH_SHAPE = (1, 2, 200, 3001)
SWITCH_FORMS = {"split0": ("0", (4, 4, 0)), "split2": ("2", (4, 2, 2))}


def switched_run(want):
    """child: the plain forward on the pre-gathered keys, the gathered forward, and the plain forward at p = P_DROP with keep bits"""
    (o_g, lse_g), (o_p, lse_p), form_g, form_p = gathered_and_plain(SWITCH_SHAPE)
    assert form_g[:2] == form_p[:2] == (1, want), (form_g, form_p, want)
    B, H, NQ, NK = SWITCH_SHAPE
    qq, _, _, kv = gather_case(B, H, NQ, NK)
    op = Op(BF16, 0, B, H, NQ, NK, p=P_DROP, bits=True)
    o_d, lse_d = op.fwd_dev(op.dev(qq), op.dev(kv))
    assert last_form()[:2] == (1, want)
    return {"o": bits16(o_p), "lse": bits16(lse_p), "o_gather": bits16(o_g), "lse_gather": bits16(lse_g), "o_drop": bits16(o_d),
            "lse_drop": bits16(lse_d), "dmask": op.dmask.cpu().numpy()}


def bf16_of(a):
    return torch.from_numpy(a).view(torch.bfloat16).float().double()


@pytest.mark.parametrize("mode", list(SWITCH_FORMS))
def test_forward_forms_behind_switches(mode):
    """attn_fwd_mfma<4, 4> (MEBT_ATTN_FWD_SPLIT=0) and attn_fwd_mfma<4, 2, 2> (=2) at 3001 keys: values against fp64 without and with
    dropout, the keep bits, and gathered keys bit for bit.  Each child asserts through mebt_debug_attn_last_launch that the form ran.

    <4, 4> cannot be selected without a switch: the 4-wave branch of launch_attn_fwd_mfma needs ceil(NQ / 128) * H * B <= 128, which
    forces ceil(NQ / 64) * H * B <= 2 * ceil(NQ / 128) * H * B <= 256, and at more than 1024 keys that always takes the split branch
    (attn_fwd_pp by default) in front of it."""
    env, _ = SWITCH_FORMS[mode]
    got = run_child(mode, {"MEBT_ATTN_FWD_SPLIT": env})
    B, H, NQ, NK = SWITCH_SHAPE
    C = H * 64
    qq, _, _, kv = gather_case(B, H, NQ, NK)
    k, v = kv[..., :C].double(), kv[..., C:].double()
    mask = mask_of(SWITCH_SHAPE)
    err = (bf16_of(got["o"]) - ref_attention(qq.double(), k, v, H)).abs().max().item()
    err_d = (bf16_of(got["o_drop"]) - ref_attention(qq.double(), k, v, H, mask.double())).abs().max().item()
    print(f"{mode}: max error {err:.3e} (bound 2e-2), with dropout {err_d:.3e} (bound {2e-2 * INV_KEEP:.3e})")
    assert err < 2e-2 and err_d < 2e-2 * INV_KEEP
    assert np.array_equal(got["lse"], got["lse_drop"])            # the row sums stay undropped
    assert torch.equal(torch.from_numpy(decode_dmask(got["dmask"].view(np.uint16), B, H, NQ, NK)), mask > 0)
    assert np.array_equal(got["o_gather"], got["o"]) and np.array_equal(got["lse_gather"], got["lse"])
    assert not np.isnan(got["lse"]).any()


if __name__ == "__main__":          # the child processes of (d) and (f): the switches are read once per process
    mode, path = sys.argv[1], sys.argv[2]
    np.savez(path, **(dropout_run((1, 1, 300, 769)) if mode == "drop_small" else switched_run(SWITCH_FORMS[mode][1])))
