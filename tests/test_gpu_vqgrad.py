"""First-stage backward on MI355X: the operators of csrc/vqgan_bwd/vqgan_bwd.hip against float64 autograd of the oracle's layers
(oracle/vqgan_oracle.py), and `VQGAN.recon_backward` against the gradients of the real reference (tests/golden/vqgrad).  GPU only.

Gates.  Convolutions: the summation bound of DESIGN.md §9d, |err| <= K 2^-23 sum |a||b| with K the number of products summed into the
element and sum |a||b| taken by the float64 twin on absolute values, plus 2^-11 |y| where the output is stored as fp16; in f16 mode
x, w and dy are rounded to fp16 before either side sees them, so only accumulation and the store differ.  GroupNorm: 8 times the
deviation of torch's own fp32 CPU backward from float64 at the same inputs (the factor covers another summation order), plus 2^-11 |dx|
in f16.  Whole model: 2e-5 of the tensor's maximum in f32 (the gate of the forward operator test, about 7 times the reference's own
deviation from float64); in f16, 4 times the deviation of the fp16-storage twin from float64 recorded in the fixture."""
import argparse

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import vqgan_oracle as vq
from tests import vqgrad_common as vc
from tests.golden import make_golden as mg

DEV = "cuda"
U32, U16 = 2.0 ** -23, 2.0 ** -11


def _host(dtype):
    from mebt_amd.vqgan import VQGAN
    host = VQGAN(argparse.Namespace(n_hiddens=32, downsample=(2, 2, 2), image_channels=3, embedding_dim=32, n_codes=32))
    host.compute_dtype, host.use_mfma = dtype, dtype == "f16"
    return host


def _r16(t):
    return t.to(torch.float16).to(t.dtype)


def _layer(kind):
    return vq.same_pad_conv3d if kind == "conv" else vq.same_pad_conv_transpose3d


def _conv_reference(kind, stride, x, w, dy):
    """float64 autograd -> dx, dw, db, and the per-element bounds K * sum |a||b| of each (K = the number of products in the element)"""
    fn = _layer(kind)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    bd = torch.zeros(dy.shape[1], dtype=torch.float64, requires_grad=True)
    fn(xd, wd, bd, stride).backward(dy.double())
    xa, wa, ba = x.double().abs().requires_grad_(True), w.double().abs().requires_grad_(True), torch.zeros_like(bd).requires_grad_(True)
    fn(xa, wa, ba, stride).backward(dy.double().abs())
    xo, wo = torch.ones_like(xa).requires_grad_(True), torch.ones_like(wa).requires_grad_(True)
    fn(xo, wo, None, stride).backward(torch.ones_like(dy, dtype=torch.float64))
    # with all-ones operands the gradient counts the products: K per element
    return (xd.grad, wd.grad, bd.grad), (xo.grad * xa.grad, wo.grad * wa.grad, float(dy[:, 0].numel()) * ba.grad)


def _run_conv(host, kind, k, stride, x, w, dy, in_mode=0, dy_mode=0, need_dx=True):
    """-> (dx [B, C, T, H, W] or None, dw in the module's shape, db) from the operators"""
    from mebt_amd.vqgan import _Conv
    B, dims = x.shape[0], tuple(x.shape[2:])
    cv = _Conv(w.to(DEV), None, (k, k, k), stride, kind == "convt", host.compute_dtype)
    host._prepared = {"convs": {"t": cv}}
    xin = x.to(DEV).contiguous() if in_mode == 1 else x.permute(0, 2, 3, 4, 1).contiguous().to(DEV, host._tdt())
    if dy_mode == 2:
        dyin = dy.to(DEV).contiguous()
    else:
        dyin = dy.permute(0, 2, 3, 4, 1).contiguous().to(DEV, host._tdt() if dy_mode == 0 else torch.float32)
    dw, db = host._conv_wgrad("t", xin, dyin, B, dims, in_mode, dy_mode, 1.0)
    dx = host._conv_dgrad("t", dyin, B, dims, dy_mode).float().permute(0, 4, 1, 2, 3).cpu() if need_dx else None
    return dx, dw.cpu(), db.cpu()


def _check_conv(kind, k, stride, cin, cout, B, dims, g, in_mode=0, dy_mode=0, need_dx=True):
    x = torch.randn(B, cin, *dims, generator=g)
    fan = cin * (k ** 3 if kind == "conv" else 8)
    w = torch.randn(*((cout, cin) if kind == "conv" else (cin, cout)), k, k, k, generator=g) / np.sqrt(fan)
    od = tuple(_layer(kind)(x[:1, :, :, :, :], w, None, stride).shape[2:])
    dy = torch.randn(B, cout, *od, generator=g)
    for dtype in ("f32", "f16"):
        xs, ws, dys = (x, w, dy) if dtype == "f32" else (_r16(x), _r16(w), _r16(dy))
        (dx_r, dw_r, db_r), (dx_b, dw_b, db_b) = _conv_reference(kind, stride, xs, ws, dys)
        host = _host(dtype)
        got = _run_conv(host, kind, k, stride, xs, ws, dys, in_mode, dy_mode, need_dx)
        again = _run_conv(host, kind, k, stride, xs, ws, dys, in_mode, dy_mode, need_dx)
        for name, a, b_, ref, bound, stored16 in (("dx", got[0], again[0], dx_r, dx_b, dtype == "f16"), ("dw", got[1], again[1], dw_r, dw_b, False),
                                                  ("db", got[2], again[2], db_r, db_b, False)):
            if a is None:
                continue
            assert torch.equal(a, b_), (name, dtype, dims, "two runs differ")
            assert tuple(a.shape) == tuple(ref.shape), (name, a.shape, ref.shape)
            lim = U32 * bound + (U16 * ref.abs() if stored16 else 0.0) + 1e-30
            ratio = float(((a.double() - ref).abs() / lim).max())
            print(f"[vqgrad conv {kind} k{k} s{stride} {cin}->{cout} {dims} {dtype}] {name}: err / bound {ratio:.3f}")
            assert ratio <= 1.0, (name, dtype, dims, ratio)


CASES = [("conv", 3, (1, 1, 1), 32, 64), ("conv", 4, (2, 2, 2), 32, 64), ("conv", 4, (1, 2, 2), 64, 128), ("conv", 1, (1, 1, 1), 64, 64),
         ("conv", 3, (1, 1, 1), 16, 24), ("conv", 3, (1, 1, 1), 64, 64), ("conv", 3, (1, 1, 1), 128, 256),
         ("convt", 4, (2, 2, 2), 64, 64), ("convt", 4, (1, 2, 2), 128, 64), ("convt", 4, (2, 2, 2), 16, 8)]


@pytest.mark.parametrize("kind,k,stride,cin,cout", CASES)
def test_conv3d_backward_operators(kind, k, stride, cin, cout):
    """data, weight and bias gradient of the ten layer shapes of test_conv3d_operator at its B = 2, (4, 6, 10) (480 voxels: ragged for any
    tile); both halos of a k = 3 layer on a two-voxel axis ((2, 3, 5), or (2, 4, 6) where a stride-2 convolution needs even axes); a
    one-voxel axis (1, 4, 4); fewer voxels than one K tile (B = 1, (1, 2, 2)).  A stride-2 convolution cannot halve a one-voxel axis: it
    takes the last two shapes on the axes it does not halve only."""
    g = torch.Generator().manual_seed(k * 100 + cin)
    strided = kind == "conv" and max(stride) > 1
    shapes = [(2, (4, 6, 10)), (2, (2, 4, 6) if strided else (2, 3, 5)), (2, (1, 4, 4)), (1, (1, 2, 2))]
    for B, dims in shapes:
        if kind == "conv" and any(d % s for d, s in zip(dims, stride)):
            continue
        _check_conv(kind, k, stride, cin, cout, B, dims, g)


def test_conv3d_backward_boundary_layouts():
    """the two layers at the video: 3 -> 32 reading the fp32 [B, C, T, H, W] video (weight gradient only: the video needs none), and
    32 -> 3 whose dy is the fp32 [B, C, T, H, W] seed (data and weight gradient)"""
    g = torch.Generator().manual_seed(77)
    for B, dims in ((2, (4, 6, 10)), (2, (2, 3, 5)), (1, (1, 2, 2))):
        _check_conv("conv", 3, (1, 1, 1), 3, 32, B, dims, g, in_mode=1, need_dx=False)
        _check_conv("conv", 3, (1, 1, 1), 32, 3, B, dims, g, dy_mode=2)


def test_conv3d_backward_argument_checks_and_empty_shapes():
    import ctypes as C
    from mebt_amd import _lib
    from mebt_amd.vqgan import _Desc
    lib = _lib.load()
    d = _Desc()
    d.Cin, d.Cout, d.ntaps = 4, 4, 1
    dw, db = torch.full((16,), 7.0, device=DEV), torch.full((4,), 7.0, device=DEV)
    assert lib.mebt_op_conv3d_wgrad(_lib.F32, C.byref(d), _lib.ptr(dw), _lib.ptr(db), 1.0, 1, None, 0, _lib.cur_stream()) == 0     # B = 0
    torch.cuda.synchronize()
    assert float(dw.abs().max()) == 0.0 and float(db.abs().max()) == 0.0
    assert lib.mebt_op_conv3d_wgrad(_lib.BF16, C.byref(d), _lib.ptr(dw), None, 1.0, 1, None, 0, _lib.cur_stream()) != 0
    d.B = d.cT = d.cH = d.cW = 1
    assert lib.mebt_op_conv3d_wgrad(_lib.F32, C.byref(d), _lib.ptr(dw), None, 1.0, 1, None, 0, _lib.cur_stream()) != 0              # no operands
    assert b"null" in lib.mebt_last_error()
    d.ntaps = 65
    assert lib.mebt_op_conv3d_wgrad(_lib.F32, C.byref(d), _lib.ptr(dw), None, 1.0, 1, None, 0, _lib.cur_stream()) != 0
    assert lib.mebt_op_pad_zero(_lib.F32, None, None, 0, 2, 2, 2, 0, 0, 0, 2, 2, 2, 4, 0, _lib.cur_stream()) == 0
    assert lib.mebt_op_pad_zero(_lib.F32, None, None, 1, 2, 2, 2, 1, 0, 0, 2, 2, 2, 4, 0, _lib.cur_stream()) != 0                   # box too small
    assert lib.mebt_op_halo_fold(_lib.F32, None, None, None, 0, 2, 2, 2, 2, 2, 2, 0, 0, 0, 4, 0, _lib.cur_stream()) == 0
    assert lib.mebt_op_halo_fold(_lib.F32, None, None, None, 1, 2, 2, 2, 2, 2, 2, 1, 0, 0, 4, 0, _lib.cur_stream()) != 0
    assert lib.mebt_op_groupnorm_silu_bwd(_lib.F32, None, None, None, None, None, None, None, _lib.ptr(dw), _lib.ptr(db), 1.0, 1, 8, 48, None, 0,
                                          _lib.cur_stream()) != 0                                                                   # 48 channels
    assert lib.mebt_op_l1_seed(None, None, None, 0, 1.0, _lib.cur_stream()) == 0
    assert lib.mebt_op_vq_seed(None, None, None, None, None, 0, 4, 4, 1.0, _lib.cur_stream()) == 0


@pytest.mark.parametrize("C", [32, 64, 256])
def test_groupnorm_silu_backward_operator(C):
    from mebt_amd import _lib
    g = torch.Generator().manual_seed(C)
    B, dims = 2, (3, 5, 7)
    vox = int(np.prod(dims))
    x0 = torch.randn(B, C, *dims, generator=g) * 1.7 + 0.4
    w, b = torch.randn(C, generator=g) * 0.2 + 1, torch.randn(C, generator=g) * 0.2
    dy0 = torch.randn(B, C, *dims, generator=g)
    add0 = torch.randn(B, C, *dims, generator=g)
    lib = _lib.load()
    for code, tdt in ((_lib.F32, torch.float32), (_lib.F16, torch.float16)):
        x, dy, add = (x0, dy0, add0) if tdt == torch.float32 else (_r16(x0), _r16(dy0), _r16(add0))

        def grads(dt):
            xs, ws, bs = (t.to(dt).clone().requires_grad_(True) for t in (x, w, b))
            vq.norm_silu(xs, ws, bs).backward(dy.to(dt))
            return xs.grad.double(), ws.grad.double(), bs.grad.double()
        ref, f32 = grads(torch.float64), grads(torch.float32)
        floor = [float((a - r).abs().max()) for a, r in zip(f32, ref)]
        cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous().to(DEV, tdt)
        xc, dyc, addc = cl(x), cl(dy), cl(add)
        y, stats = torch.empty_like(xc), torch.empty(B * 64, device=DEV)
        wd, bd = w.to(DEV), b.to(DEV)
        _lib.check(lib.mebt_op_groupnorm_silu(code, _lib.ptr(xc), _lib.ptr(y), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(stats), B, vox, C, _lib.cur_stream()))
        nbytes = int(lib.mebt_groupnorm_silu_bwd_scratch_bytes(B, vox, C))
        outs = []
        for addp, scale in ((None, 1.0), (None, 1.0), (addc, 0.25)):
            scratch = torch.empty(nbytes // 8 + 1, device=DEV, dtype=torch.float64)
            dx, dg, db = torch.empty_like(xc), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
            _lib.check(lib.mebt_op_groupnorm_silu_bwd(code, _lib.ptr(xc), _lib.ptr(stats), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(dyc), _lib.ptr(addp),
                                                      _lib.ptr(dx), _lib.ptr(dg), _lib.ptr(db), scale, B, vox, C, _lib.ptr(scratch), nbytes,
                                                      _lib.cur_stream()))
            outs.append((dx.float().permute(0, 4, 1, 2, 3).cpu().double(), dg.cpu().double(), db.cpu().double()))
        assert all(torch.equal(a, b_) for a, b_ in zip(outs[0], outs[1])), "two runs differ"
        store = U16 * ref[0].abs() if tdt == torch.float16 else 0.0
        for name, got, r, fl, extra in (("dx", outs[0][0], ref[0], floor[0], store), ("dgamma", outs[0][1], ref[1], floor[1], 0.0),
                                        ("dbeta", outs[0][2], ref[2], floor[2], 0.0)):
            ratio = float(((got - r).abs() / (8 * fl + extra)).max())
            print(f"[vqgrad groupnorm C={C} {tdt}] {name}: torch fp32 floor {fl:.2e}, err / gate {ratio:.3f}")
            assert ratio <= 1.0, (name, tdt, ratio)
        # the residual input is added to dx, the scale multiplies the parameter gradients (a power of two: exactly)
        store3 = U16 * (ref[0] + add.double()).abs() if tdt == torch.float16 else 0.0
        assert float(((outs[2][0] - (ref[0] + add.double())).abs() / (8 * floor[0] + store3 + U32 * add.double().abs())).max()) <= 1.0
        assert torch.equal(outs[2][1], outs[0][1] * 0.25) and torch.equal(outs[2][2], outs[0][2] * 0.25)


def test_seed_operators():
    from mebt_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(4)
    a, b = torch.randn(3001, generator=g), torch.randn(3001, generator=g)
    b[::7] = a[::7]                                                            # sign(0) = 0, as in torch
    ad, bd, out = a.to(DEV), b.to(DEV), torch.empty(3001, device=DEV)
    _lib.check(lib.mebt_op_l1_seed(_lib.ptr(ad), _lib.ptr(bd), _lib.ptr(out), 3001, 0.375, _lib.cur_stream()))
    assert torch.equal(out.cpu(), 0.375 * torch.sign(a - b))
    M, d, n = 70, 64, 50
    z, e, gst = torch.randn(M, d, generator=g), torch.randn(n, d, generator=g), torch.randn(M, d, generator=g)
    ids = torch.randint(0, n, (M,), generator=g)
    zd, ed, gd, idd, dz = z.to(DEV), e.to(DEV), gst.to(DEV), ids.to(DEV), torch.empty(M, d, device=DEV)
    _lib.check(lib.mebt_op_vq_seed(_lib.ptr(zd), _lib.ptr(ed), _lib.ptr(idd), _lib.ptr(gd), _lib.ptr(dz), M, d, n, 0.5, _lib.cur_stream()))
    assert torch.equal(dz.cpu(), 0.5 * (z - e[ids]) + gst)
    _lib.check(lib.mebt_op_vq_seed(_lib.ptr(zd), _lib.ptr(ed), _lib.ptr(idd), None, _lib.ptr(dz), M, d, n, 0.5, _lib.cur_stream()))
    assert torch.equal(dz.cpu(), 0.5 * (z - e[ids]))


# ---- whole model ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return vc.load_fixture()


def build(dtype, l1_weight=4.0):
    from mebt_amd.vqgan import VQGAN
    c = mg.VQGAN_CONFIGS["vq_micro"]
    args = argparse.Namespace(n_hiddens=c["n_hiddens"], downsample=c["downsample"], image_channels=3, embedding_dim=c["embedding_dim"],
                              n_codes=c["n_codes"], sequence_length=c["video"][2], sample_every_n_frames=1, resolution=c["video"][3],
                              l1_weight=l1_weight, perceptual_weight=0.0, lr=3e-4)
    m = VQGAN(args)
    m.load_state_dict(vq.closed_form_params(mg.vqgan_cfg("vq_micro")), strict=False)
    m.compute_dtype = dtype
    return m.to(DEV).eval()


def grads_of(m):
    return {k: p.grad.detach().cpu().double().numpy() for k, p in m.named_parameters() if k.startswith(vc.TRAINED)}


def test_recon_backward_f32_matches_the_reference_gradients_and_its_sgd_steps(fx):
    """every gradient within 2e-5 of its tensor's maximum of the reference's, losses to 1e-5, ids equal; `.grad` accumulates; after one
    and two SGD steps the returned losses are the reference's (1e-4): the prepared weights follow the in-place updates"""
    m = build("f32")
    x = torch.from_numpy(fx["x"]).to(DEV)
    ref = vc.fixture_grads(fx)
    assert all(p.grad is None for p in m.parameters())
    out = m.recon_backward(x)
    assert sorted(out) == ["commitment_loss", "encodings", "finite", "grad_scale", "perplexity", "recon_loss", "x_recon"]
    assert out["finite"] is True and out["grad_scale"] == vc.default_scale(4.0, x.numel())
    assert np.array_equal(out["encodings"].cpu().numpy(), fx["ids_0"]), "the ids differ from the reference's: nothing below would compare like with like"
    for key, want in (("recon_loss", fx["step_losses"][0, 0]), ("commitment_loss", fx["step_losses"][0, 1])):
        assert abs(float(out[key]) - want) <= 1e-5 * want, (key, float(out[key]), want)
    got = grads_of(m)
    assert sorted(got) == sorted(ref)
    worst = 0.0
    for k in ref:
        err = np.abs(got[k] - ref[k]).max() / vc.scale_of(k, ref)
        worst = max(worst, err)
        assert err <= 2e-5, (k, err)
    print(f"[vqgrad model f32] worst gradient deviation from the reference {worst:.2e} of the tensor's maximum")
    assert all(p.grad is None for p in m.codebook.parameters()) and m.codebook.embeddings.grad is None
    # accumulate semantics: a second call without zero_grad doubles .grad.  The forward's GroupNorm statistics are summed with float
    # atomics (csrc/vqgan.hip), so two calls agree to fp32 rounding of those sums, not bitwise: the f32 gate again.
    m.recon_backward(x)
    twice = grads_of(m)
    for k in ref:
        assert np.abs(twice[k] - 2 * got[k]).max() <= 2e-5 * 2 * vc.scale_of(k, ref), k
    # two SGD steps: the losses follow the reference's
    opt = torch.optim.SGD([p for n, p in m.named_parameters() if n.startswith(vc.TRAINED)], lr=float(fx["sgd_lr"]))
    for step in (1, 2):
        if step == 1:
            opt.zero_grad()
            m.recon_backward(x)
        opt.step()
        opt.zero_grad()
        out = m.recon_backward(x)
        assert np.array_equal(out["encodings"].cpu().numpy(), fx[f"ids_{step}"])
        for key, want in (("recon_loss", fx["step_losses"][step, 0]), ("commitment_loss", fx["step_losses"][step, 1])):
            assert abs(float(out[key]) - want) <= 1e-4 * want, (step, key, float(out[key]), want)


def f16_reference(fx, x_recon):
    """The gradients the f16 run is held to.  Like the ids, the signs of the L1 seed are a discrete outcome of the forward: the fixture's
    video keeps every |x_recon - x| above 1e-4, which shields them from fp32 rounding, but the f16 forward's error reaches 7.8e-3 here
    (rms 1.7e-3, the fp16-storage twin's too) and no video keeps 6144 residuals clear of that.  Measured: ONE sign differs from the
    reference's, at the element with the smallest residual (4.4e-4), and that alone moves gradients by up to 2.5e-2 of their maximum
    (one seed in 6144 adding incoherently: 2 / sqrt(6144)).  So where signs differ the reference is float64 autograd of the oracle at
    the f16 forward's OWN sign pattern (tests/test_vqgrad_host.py pins that oracle to the fixture within 1e-5); a sign may differ only
    where the reference's residual is inside the f16 gate of the forward test (3e-3 of the reconstruction's maximum), else the test
    fails and says so.  Without differing signs the reference is the fixture itself.  The pattern is read from the `x_recon` the call
    returns: a second f16 forward need not repeat it (the GroupNorm statistics' float atomics move single fp16 roundings, and a
    residual within that noise of zero changes sign from run to run)."""
    ref = vc.fixture_grads(fx)
    cfg = mg.vqgan_cfg("vq_micro")
    P = vq.closed_form_params(cfg)
    x = torch.from_numpy(fx["x"])
    _, _, rec64, _ = vc.objective({k: v.double() for k, v in P.items()}, cfg, x.double(), torch.from_numpy(fx["ids_0"]))
    signs = torch.sign(x_recon.cpu().double() - x)
    differ = signs != torch.sign(rec64 - x)
    n = int(differ.sum())
    if n == 0:
        return ref
    worst = float((rec64 - x).abs()[differ].max())
    print(f"[vqgrad model f16] {n} L1 sign(s) differ from the reference's, largest reference residual among them {worst:.2e}")
    assert worst <= 3e-3 * float(rec64.abs().max()), f"an L1 sign differs where the reference's residual is {worst:.2e}: outside the f16 forward gate"
    g, _, _ = vc.objective_grads(P, cfg, x, torch.from_numpy(fx["ids_0"]), l1_signs=signs)
    return g


def test_recon_backward_f16_within_four_times_the_storage_twin(fx):
    m = build("f16")
    x = torch.from_numpy(fx["x"]).to(DEV)
    out = m.recon_backward(x)
    assert np.array_equal(out["encodings"].cpu().numpy(), fx["ids_0"]), "the f16 ids differ from the fixture's: the gradients would not compare like with like"
    assert out["finite"] is True and out["grad_scale"] == float(fx["twin_scale"])
    ref = f16_reference(fx, out["x_recon"])
    got = grads_of(m)
    worst = 0.0
    for k in ref:
        err, gate = np.abs(got[k] - ref[k]).max() / vc.scale_of(k, ref), 4 * float(fx["twin_dev/" + k])
        worst = max(worst, err / gate)
        print(f"[vqgrad model f16] {k}: {err:.2e} (gate {gate:.2e})")
        assert err <= gate, (k, err, gate)
    print(f"[vqgrad model f16] worst err / gate {worst:.3f}")


def test_grad_scale_keeps_small_l1_weights_out_of_fp16_underflow(fx):
    """l1_weight 1e-4: the unscaled seed 1e-4 / 6144 = 1.6e-8 is below half of fp16's smallest subnormal.  With the default scale the
    decoder's gradients are 1e-4 / 4 times those at l1_weight 4 within the f16 gate; with a unit scale they are all zero."""
    x = torch.from_numpy(fx["x"]).to(DEV)
    small = build("f16", 1e-4)
    out = small.recon_backward(x)
    assert out["finite"] is True and out["grad_scale"] == vc.default_scale(1e-4, x.numel())
    gs = grads_of(small)
    # the decoder's gradients are linear in l1_weight (the commitment term does not reach it): those at l1_weight 4, taken like the f16
    # test's at the sign pattern of THIS run's reconstruction (a separate f16 run at l1_weight 4 need not repeat the pattern)
    ref = f16_reference(fx, out["x_recon"])
    dec = [k for k in ref if k.startswith("decoder.")]
    assert len(dec) == 40
    for k in dec:
        err, gate = np.abs(gs[k] / (1e-4 / 4) - ref[k]).max() / vc.scale_of(k, ref), 4 * float(fx["twin_dev/" + k])
        assert err <= gate, (k, err, gate)
    unit = build("f16", 1e-4)
    out = unit.recon_backward(x, grad_scale=1.0)
    assert out["grad_scale"] == 1.0
    gu = grads_of(unit)
    assert all(np.abs(gu[k]).max() == 0.0 for k in dec)
    with pytest.raises(ValueError):
        unit.recon_backward(x, grad_scale=3.0)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_encode_and_decode_are_untouched_by_a_backward_call(fx, dtype):
    """unchanged weights: bit-identical encode / decode before and after.  The clip is the fixture's first 2 x 8 x 8 corner: no GroupNorm
    of the model then sees more than 128 voxels per sample, so at most two workgroups add (with float atomics, csrc/vqgan.hip) to one
    statistic and their order cannot matter; on larger inputs the forward itself is not bitwise repeatable from run to run."""
    m = build(dtype)
    x = torch.from_numpy(fx["x"][:, :, :2, :8, :8].copy()).to(DEV)
    ids0 = m.encode(x)
    rec0 = m.decode(ids0)
    prepared = m._prepared
    m.recon_backward(x)
    assert m._prepared is prepared and m._tape is None                          # versions did not move: nothing is re-laid out
    ids1 = m.encode(x)
    rec1 = m.decode(ids1)
    assert torch.equal(ids0, ids1) and torch.equal(rec0, rec1)
    # an in-place update is noticed
    with torch.no_grad():
        m.decoder.conv_last.conv.bias.add_(0.125)
    rec2 = m.decode(ids1)
    assert m._prepared is not prepared
    assert (rec2 - rec1 - 0.125).abs().max().item() <= 1e-5


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_adam_on_a_reference_format_checkpoint_lowers_the_reconstruction_loss(fx, dtype, tmp_path):
    """a Lightning-format checkpoint of the reference ({'state_dict', 'hyper_parameters': {'args'}}) -> `load_from_checkpoint` ->
    `recon_backward` + the optimizer of `configure_optimizers()` (Adam, lr 3e-4, betas (0.5, 0.9)): the reconstruction loss falls
    over five steps on the frozen codebook, every step reading the weights the previous one wrote"""
    from mebt_amd.vqgan import VQGAN
    c = mg.VQGAN_CONFIGS["vq_micro"]
    args = argparse.Namespace(n_hiddens=c["n_hiddens"], downsample=c["downsample"], image_channels=3, embedding_dim=c["embedding_dim"],
                              n_codes=c["n_codes"], sequence_length=c["video"][2], sample_every_n_frames=1, resolution=c["video"][3],
                              l1_weight=4.0, perceptual_weight=0.0, lr=3e-4)
    path = str(tmp_path / "vqgan.ckpt")
    torch.save({"state_dict": vq.closed_form_params(mg.vqgan_cfg("vq_micro")), "hyper_parameters": {"args": args}}, path)
    m = VQGAN.load_from_checkpoint(path).to(DEV)
    m.compute_dtype = dtype
    x = torch.from_numpy(fx["x"]).to(DEV)
    opt = m.configure_optimizers()
    losses = []
    for _ in range(6):
        opt.zero_grad()
        out = m.recon_backward(x)
        assert out["finite"] is True
        losses.append(float(out["recon_loss"]))
        opt.step()
    print(f"[vqgrad adam {dtype}] recon_loss over the steps: {' '.join(f'{v:.4f}' for v in losses)}")
    assert abs(losses[0] - fx["step_losses"][0, 0]) <= (1e-5 if dtype == "f32" else 3e-3) * losses[0]
    assert losses[-1] < losses[0]                       # Adam's steps need not fall one by one: over the six they do
