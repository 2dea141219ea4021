"""The discriminators' forward on the GPU (csrc/disc/disc_conv.hip, mebt_amd/discriminator.py: DiscRunner, gan_terms): the single
convolution and the one-channel stage against float64 torch within a derived bound, the BatchNorm slots of the epilogue, the whole
forward and the thirteen GAN values against the golden of the real reference classes (tests/golden/disc), bit determinism, the
automatic refresh, a cross-check against mebt_op_i3d_conv, and the function behind `measure_recon --disc`.

The bound of a convolution (derived, not tuned): inputs and weights are already rounded to the storage dtype, so their products are
exact in fp32 (fp16) or rounded once (fp32); every one of the K - 1 additions of a row, the flushes into the second accumulator, the
bias and the fp32 store each round once, relative to a partial sum no larger than sum |x||w| + |bias|.  That is at most
(K + 3) * 2^-24 * (|x| conv |w| + |bias|) element-wise; the fp16 store adds 2^-11 |y|."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from mebt_amd import _lib  # noqa: E402
from mebt_amd import discriminator as D  # noqa: E402
from tests.disc_common import (CASES, D_KEYS, G_KEYS, GAN_CASES, GAN_CONFIGS, case_input, case_sd, check_against_golden,  # noqa: E402
                               closed_form_state_dict, gan_args, gold, scalar_tolerances, structured_clip)

DEV = "cuda"
TDT = {"f16": torch.float16, "f32": torch.float32}


def cl(t):
    """logical [B, C, (T,) H, W] -> contiguous channels-last [B, T, H, W, C] (T = 1 for an image)"""
    if t.dim() == 4:
        t = t.unsqueeze(2)
    return t.permute(0, 2, 3, 4, 1).contiguous()


def logical(buf, three_d):
    return buf.permute(0, 4, 1, 2, 3) if three_d else buf[:, 0].permute(0, 3, 1, 2)


def conv_case(seed, three_d, B, dims, cin, cout, stride, dtype):
    """x (rounded to the storage dtype, float64), w, bias, the float64 convolution and its element-wise bound"""
    g = torch.Generator().manual_seed(seed)
    shape = (B, cin) + (tuple(dims) if three_d else tuple(dims[1:]))
    x = (torch.rand(shape, generator=g) - 0.5).to(TDT[dtype])
    w = (torch.randn((cout, cin) + ((4, 4, 4) if three_d else (4, 4)), generator=g) * (2.0 / (16 * cin)) ** 0.5).to(TDT[dtype]).float()
    bias = torch.randn(cout, generator=g) * 0.05
    conv = F.conv3d if three_d else F.conv2d
    y = conv(x.double(), w.double(), bias.double(), stride=stride, padding=2)
    mag = conv(x.double().abs(), w.double().abs(), bias.double().abs(), stride=stride, padding=2)
    K = (64 if three_d else 16) * cin
    bound = (K + 3) * 2.0 ** -24 * mag
    return x, w, bias, y, bound


def store_bound(bound, y, dtype):
    return bound + (2.0 ** -11 * y.abs() if dtype == "f16" else 0.0)


def report(name, got, want, bound):
    err = (got.double().cpu() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: largest distance {float(err.max()):.3e}, {worst:.3f} of its bound (largest bound {float(bound.max()):.3e})")
    assert bool((err <= bound).all()), (name, float(err.max()), worst)


# ---- the single convolution -----------------------------------------------------------------------------------------------------------------
CONV_CASES = {                     # three_d, B, (T, H, W), cin, cout, stride
    "stage0_2d_5x3": (False, 2, (1, 5, 3), 3, 8, 2),
    "stage0_3d_3x5x3": (True, 2, (3, 5, 3), 3, 8, 2),
    "c8_c8_s1_2d": (False, 2, (1, 5, 3), 8, 8, 1),
    "c8_c8_s2_2d": (False, 2, (1, 5, 3), 8, 8, 2),
    "c8_c8_s1_3d": (True, 2, (3, 5, 3), 8, 8, 1),
    "c8_c8_s2_3d": (True, 2, (3, 5, 3), 8, 8, 2),
    "c8_c72": (False, 2, (1, 5, 3), 8, 72, 2),
    "c24_c8": (False, 2, (1, 5, 3), 24, 8, 2),             # Cin no power of two: the tap decode divides
    "3d_with_t1": (True, 2, (1, 5, 3), 8, 16, 2),
}


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_convolution_vs_float64(name, dtype):
    three_d, B, dims, cin, cout, stride = CONV_CASES[name]
    x, w, bias, y, bound = conv_case(len(name), three_d, B, dims, cin, cout, stride, dtype)
    kt = 4 if three_d else 1
    if cin == 3:                                    # through the ingest: the stored fourth channel is zero
        h = D.ingest(x.float().to(DEV), dtype)
        assert tuple(h.shape) == (B,) + tuple(dims) + (4,) and float(h[..., 3].abs().sum()) == 0
        assert torch.equal(h[..., :3].cpu(), cl(x)), "the ingest rounds to the storage dtype and nothing else"
        wa = D.arrange_weight(w, dtype, cin_store=4).to(DEV)
    else:
        h = cl(x).to(DEV)
        wa = D.arrange_weight(w, dtype).to(DEV)
    for act in (False, True):
        out = D.conv_stage(h, wa, bias.to(DEV), kt, stride, cout, act=act)
        want = F.leaky_relu(y, 0.2) if act else y
        got = logical(out, three_d)
        assert tuple(got.shape) == tuple(want.shape)
        report(f"conv {name} {dtype} act={act}", got, want, store_bound(bound, want, dtype))


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_convolution_on_1x1_inputs_around_one_tile_of_rows(delta, dtype):
    """stride 2 on 1 x 1 inputs: M equals B, and all taps but one fall in the padding"""
    B = D.TILE_ROWS[dtype] + delta
    x, w, bias, y, bound = conv_case(B, False, B, (1, 1, 1), 8, 8, 2, dtype)
    out, slots = D.conv_stage(cl(x).to(DEV), D.arrange_weight(w, dtype).to(DEV), bias.to(DEV), 1, 2, 8, slots=True)
    assert tuple(out.shape) == (B, 1, 1, 1, 8) and slots.numel() == 8 * 2 * (1 if delta <= 0 else 2)
    report(f"conv 1x1 B={B} {dtype}", logical(out, False), y, store_bound(bound, y, dtype))
    stats = D.slot_stats(slots, B, 8).double().cpu()
    mean = y.mean((0, 2, 3))
    assert float((stats[0] - mean).abs().max()) <= float(bound.mean((0, 2, 3)).max()) + 2.0 ** -23 * float(mean.abs().max())


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("three_d,dims,cin", [(False, (1, 5, 3), 8), (True, (2, 3, 4), 24)])
def test_one_channel_stage_vs_float64(three_d, dims, cin, dtype):
    """K 128 (fewer 16-byte chunks than lanes) and K 1536"""
    x, w, bias, y, bound = conv_case(cin, three_d, 3, dims, cin, 1, 1, dtype)
    out = D.head_stage(cl(x).to(DEV), D.arrange_weight(w, dtype).to(DEV), bias.to(DEV), 4 if three_d else 1)
    report(f"one-channel stage K={(64 if three_d else 16) * cin} {dtype}", logical(out, three_d), y, store_bound(bound, y, dtype))


# ---- BatchNorm slots of the epilogue ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("three_d,B,dims", [(False, 3, (1, 20, 12)), (True, 2, (3, 9, 7))])
def test_epilogue_slots_give_the_batch_statistics(three_d, B, dims, dtype):
    """M = 3 x 11 x 7 = 231 and 2 x 2 x 5 x 4 = 80 rows: no multiple of either dtype's tile; 72 channels cross a column tile"""
    cin, cout = 8, 72
    x, w, bias, y, bound = conv_case(7, three_d, B, dims, cin, cout, 2, dtype)
    out, slots = D.conv_stage(cl(x).to(DEV), D.arrange_weight(w, dtype).to(DEV), bias.to(DEV), 4 if three_d else 1, 2, cout, slots=True)
    M = out.numel() // cout
    assert M % D.TILE_ROWS[dtype] != 0 and slots.numel() == cout * 2 * -(-M // D.TILE_ROWS[dtype])
    rm, rv, nbt = torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV), torch.tensor([7], device=DEV)
    stats = D.slot_stats(slots, M, cout, rm, rv, nbt, True)
    assert int(nbt) == 8
    red = (0, 2, 3, 4) if three_d else (0, 2, 3)
    if dtype == "f32":
        # the same fp64 sums of the same fp32 values in another grouping, each rounded once to fp32
        rm2, rv2 = torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV)
        want = D.batch_stats(out, rm2, rv2, None, True)
        rel = float(((stats - want).abs() / want.abs()).max())
        print(f"slots {dtype} M={M}: largest relative distance from batch_stats {rel:.3e}, gate {2.0 ** -22:.3e}")
        assert torch.allclose(stats, want, rtol=2.0 ** -22, atol=0.0)
        assert torch.allclose(rm, rm2, rtol=2.0 ** -22, atol=0.0) and torch.allclose(rv, rv2, rtol=2.0 ** -22, atol=0.0)
        return
    # fp16: the statistics are taken before the store rounds, so they are compared with the float64 convolution's.  With e the
    # element bound: |mean - mean64| <= mean(e); |var - var64| <= mean(2 |y| e + e^2) + 2 |mean64| mean(e) + mean(e)^2; and
    # rstd = (var + eps)^-1/2 moves by at most |dvar| / 2 / (var64 - |dvar| + eps)^1.5.  One fp32 rounding each on top.
    mean64, var64 = y.mean(red), y.var(red, unbiased=False)
    e_mean = bound.mean(red)
    d_var = (2 * y.abs() * bound + bound ** 2).mean(red) + 2 * mean64.abs() * e_mean + e_mean ** 2
    got = stats.double().cpu()
    g_mean = e_mean + 2.0 ** -24 * mean64.abs()
    rstd64 = 1 / torch.sqrt(var64 + D.BN_EPS)
    g_rstd = 0.5 * d_var / (var64 - d_var + D.BN_EPS).clamp_min(1e-12) ** 1.5 + 2.0 ** -23 * rstd64
    print(f"slots {dtype} M={M}: mean distance {float((got[0] - mean64).abs().max()):.3e} (gate {float(g_mean.max()):.3e}), "
          f"rstd distance {float((got[1] - rstd64).abs().max()):.3e} (gate {float(g_rstd.max()):.3e})")
    assert bool(((got[0] - mean64).abs() <= g_mean).all()) and bool(((got[1] - rstd64).abs() <= g_rstd).all())


# ---- the whole forward against the golden -----------------------------------------------------------------------------------------------------
def holder(c_or_cfg, three_d=None, training=False):
    cfg = CASES[c_or_cfg] if isinstance(c_or_cfg, str) else c_or_cfg
    three_d = cfg["three_d"] if three_d is None else three_d
    net = (D.NLayerDiscriminator3D if three_d else D.NLayerDiscriminator)(3, cfg["ndf"], cfg["L"])
    net.load_state_dict(closed_form_state_dict(cfg["ndf"], cfg["L"], three_d), strict=True)
    return net.to(DEV).train(training)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("c", list(CASES))
def test_forward_equals_the_reference(c, mode, dtype):
    g, sd = gold(), case_sd(c)
    net = holder(c, training=mode == "train")
    logits, feats = D.DiscRunner(net, dtype)(case_input(c).to(DEV))
    assert all(f.dtype == TDT[dtype] and f.is_cuda for f in feats) and logits is feats[-1]
    check_against_golden(c, mode, dtype, logits, feats)
    names = [k for k in sd if k.endswith(("running_mean", "running_var"))]
    for k, v in net.state_dict().items():
        if not k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            continue
        if mode == "eval":
            assert torch.equal(v.cpu(), sd[k]), k            # eval mode reads the buffers and leaves them alone
        elif k.endswith("tracked"):
            assert int(v) == int(g[f"{c}_train_buf_{k}"]) == 8
        else:
            d32, d16, mx = g[f"{c}_train_bufstats"][names.index(k)]
            gate = 4 * (max(d32, 2.0 ** -24) if dtype == "f32" else d16) * mx
            err = float((v.double().cpu() - torch.from_numpy(g[f"{c}_train_buf_{k}"]).double()).abs().max())
            print(f"forward {c} {dtype} {k}: distance {err / mx:.3e} of the maximum, gate {gate / mx:.3e}")
            assert err <= gate, (k, err, gate)


# ---- the thirteen logged values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("gcase", list(GAN_CASES))
def test_gan_terms_equal_the_references(gcase, mode, dtype):
    cfg, g = GAN_CASES[gcase], gold()
    x, xr = structured_clip(cfg["shape"]).to(DEV), structured_clip(cfg["shape"], 1).to(DEV)
    fidx = torch.from_numpy(g[f"{gcase}_frame_idx"])
    nets = holder(cfg, False, mode == "train"), holder(cfg, True, mode == "train")
    ri, rv = D.DiscRunner(nets[0], dtype), D.DiscRunner(nets[1], dtype)
    before = [{k: v.clone() for k, v in n.state_dict().items()} for n in nets]
    for kind, gfw, step in GAN_CONFIGS:
        a = gan_args(kind, gfw)
        got = {}
        for which in ("generator", "discriminator"):
            got.update(D.gan_terms(a, ri, rv, x, xr, fidx, step, which, update_running=False))
        assert set(got) == set(G_KEYS + D_KEYS)
        assert all(v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda for v in got.values())
        want = g[f"{gcase}_{mode}_{kind}_{int(gfw)}_{step}_ref"]
        tol = scalar_tolerances(g[f"{gcase}_{mode}_callstats"], a, step, dtype == "f16")
        for i, k in enumerate(G_KEYS + D_KEYS):
            print(f"gan_terms {gcase} {mode} {dtype} {kind} {gfw} {step} {k}: {float(got[k]):.7f} vs {want[i]:.7f}, bound {tol[i]:.2e}")
            assert abs(float(got[k]) - want[i]) <= tol[i], (k, kind, gfw, step, float(got[k]), want[i], tol[i])
    for n, b in zip(nets, before):                       # update_running=False: the buffers keep their bits
        assert all(torch.equal(v, b[k]) for k, v in n.state_dict().items())
    if mode == "train":                                  # the default advances them, on the generator's calls too (as the reference)
        D.gan_terms(gan_args("hinge", 0.0), ri, rv, x, xr, fidx, 0, "generator")
        assert int(nets[0].model1[1].num_batches_tracked) == 9 and int(nets[1].model1[1].num_batches_tracked) == 9
        D.gan_terms(gan_args("hinge", 0.0, image_gan_weight=0.0), ri, rv, x, xr, fidx, 0, "generator")      # no real-side image pass
        assert int(nets[0].model1[1].num_batches_tracked) == 10 and int(nets[1].model1[1].num_batches_tracked) == 11


# ---- determinism ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("c", ["img8", "vid8"])
def test_forward_is_bit_identical_and_independent_of_the_batch(c, dtype):
    cfg = CASES[c]
    shape = (3,) + tuple(cfg["shape"][1:])
    x = structured_clip(shape).to(DEV)
    for training in (False, True):
        r = D.DiscRunner(holder(c, training=training), dtype)
        a = [f.clone() for f in r(x, update_running=False)[1]]
        b = r(x, update_running=False)[1]
        assert all(torch.equal(p, q) for p, q in zip(a, b)), (c, dtype, training)
    r = D.DiscRunner(holder(c), dtype)                  # eval mode: a clip's logits are the same bits at B = 1 and inside B = 3
    inside = r(x)[0][1].clone()
    alone = r(x[1:2].contiguous())[0][0]
    assert torch.equal(inside, alone)


def test_runner_picks_up_an_in_place_parameter_change():
    net = holder("img8")
    r = D.DiscRunner(net, "f32")
    x = case_input("img8").to(DEV)
    first = r(x)[0].clone()
    with torch.no_grad():
        net.model1[0].weight.mul_(1.5)
        net.model2[1].bias.add_(0.25)
    second = r(x)[0].clone()                            # no explicit refresh()
    assert not torch.equal(first, second)
    assert torch.equal(second, D.DiscRunner(net, "f32")(x)[0])
    net.train()
    r(x)                                                # a training-mode call moves the running buffers through raw pointers
    net.eval()
    third = r(x)[0].clone()                             # the eval-mode statistics kept by the runner follow them
    assert int(net.model1[1].num_batches_tracked) == 8 and not torch.equal(second, third)
    assert torch.equal(third, D.DiscRunner(net, "f32")(x)[0])


# ---- cross-check against the I3D convolution ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_stage_1_agrees_with_the_i3d_convolution(dtype):
    """a stage 1 convolution (8 -> 16, 4 x 4 x 4, stride 2; K 512 fits mebt_op_i3d_conv's table) through both kernels on the same arranged
    weights, padding 2 front and back: both inside the derived bound"""
    from mebt_amd.i3d import _ConvDesc
    B, dims, cin, cout = 2, (3, 10, 6), 8, 16
    x, w, bias, y, bound = conv_case(11, True, B, dims, cin, cout, 2, dtype)
    h, wa, bd = cl(x).to(DEV), D.arrange_weight(w, dtype).to(DEV), bias.to(DEV)
    ours = D.conv_stage(h, wa, bd, 4, 2, cout)
    theirs = torch.empty_like(ours)
    d = _ConvDesc()
    d.in_, d.w, d.bias = h.data_ptr(), wa.data_ptr(), bd.data_ptr()
    d.B, d.Ti, d.Hi, d.Wi, d.Cin = B, dims[0], dims[1], dims[2], cin
    d.To, d.Ho, d.Wo, d.Cout = ours.shape[1], ours.shape[2], ours.shape[3], cout
    for a in range(3):
        d.k[a], d.s[a], d.pad_front[a], d.pad_back[a] = 4, 2, 2, 2
    d.relu, d.nseg = 0, 1
    d.seg[0].out, d.seg[0].n0, d.seg[0].n1, d.seg[0].cstride, d.seg[0].coff = theirs.data_ptr(), 0, cout, cout, 0
    _lib.check(_lib.load().mebt_op_i3d_conv(_lib.dtype_code(dtype), C.byref(d), _lib.cur_stream()))
    gate = store_bound(bound, y, dtype)
    report(f"stage 1 {dtype}: this convolution", logical(ours, True), y, gate)
    report(f"stage 1 {dtype}: mebt_op_i3d_conv", logical(theirs, True), y, gate)


# ---- rejected arguments -------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_return_the_status_without_launching():
    lib, s = _lib.load(), _lib.cur_stream()
    x = torch.zeros(2, 1, 5, 3, 8, device=DEV, dtype=torch.float16)
    w = torch.zeros(64, 128, device=DEV, dtype=torch.float16)
    b = torch.zeros(8, device=DEV)
    out = torch.full((2, 1, 3, 2, 8), 7.0, device=DEV, dtype=torch.float16)
    slots = torch.zeros(16, device=DEV, dtype=torch.float64)
    nb = lambda t: t.numel() * t.element_size()
    conv = lambda **k: lib.mebt_op_disc_conv(k.get("dtype", _lib.F16), k.get("x", x.data_ptr()), k.get("xb", nb(x)), w.data_ptr(), k.get("wb", nb(w)),
                                             b.data_ptr(), k.get("out", out.data_ptr()), k.get("ob", nb(out)), k.get("slots", None), k.get("sb", 0), 2, 1,
                                             5, 3, k.get("cin", 8), k.get("kt", 1), k.get("stride", 2), 1, k.get("Ho", 3), 2, 8, 0, s)
    for rc, call in [(1, lambda: conv(x=None)), (5, lambda: conv(dtype=_lib.BF16)), (2, lambda: conv(kt=2)), (2, lambda: conv(stride=3)),
                     (2, lambda: conv(Ho=4)), (2, lambda: conv(cin=6)), (1, lambda: conv(x=x.data_ptr() + 8)), (4, lambda: conv(xb=nb(x) - 2)),
                     (4, lambda: conv(wb=nb(w) - 2)), (4, lambda: conv(wb=nb(w) + 64)), (4, lambda: conv(ob=nb(out) - 2)),
                     (1, lambda: conv(slots=None, sb=256)), (4, lambda: conv(slots=slots.data_ptr(), sb=120)),
                     (1, lambda: conv(slots=slots.data_ptr() + 4, sb=256))]:
        assert call() == rc, lib.mebt_last_error()
        assert lib.mebt_last_error().startswith(b"disc_conv: ")
    assert lib.mebt_op_disc_head(_lib.F16, x.data_ptr(), nb(x), w.data_ptr(), nb(w), b.data_ptr(), out.data_ptr(), nb(out), 2, 1, 5, 3, 8, 1, 1, 6, 5, s) == 2
    assert lib.mebt_last_error().startswith(b"disc_head: ")
    assert lib.mebt_op_disc_bn_act(_lib.F16, out.data_ptr(), 12, 6, b.data_ptr(), b.data_ptr(), b.data_ptr(), s) == 2
    assert lib.mebt_op_disc_bn_act(_lib.F16, None, 12, 8, b.data_ptr(), b.data_ptr(), b.data_ptr(), s) == 1
    assert lib.mebt_op_disc_ingest(_lib.F16, b.data_ptr(), None, out.data_ptr(), 8, 2, 1, 5, 3, s) == 4
    assert lib.mebt_last_error().startswith(b"disc_ingest: ")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and float(slots.abs().sum()) == 0
    with pytest.raises(ValueError, match="frame_idx must lie in"):          # also for an index that already lives on the GPU
        D.DiscRunner(holder("img8"))(torch.zeros(2, 3, 4, 8, 8, device=DEV), frame_idx=torch.tensor([0, 4], device=DEV))


# ---- measure_recon --disc -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,stats", [("f32", "batch"), ("f16", "batch"), ("f32", "running")])
def test_measure_recon_disc_terms_equal_the_twin(tmp_path, dtype, stats):
    """the function behind --disc on a synthetic checkpoint (closed-form discriminators) and two tiny batches, against gan_terms_twin
    in float64 (no storage rounding: the bound is on the distance from float64) on the frames it drew.  The bound is the golden's for
    these shapes and weights: scalar_tolerances of gan8's recorded call distances; the second batch holds the same clips in the other
    order."""
    from mebt_amd.measure_recon import DISC_COLUMNS, DiscTerms
    from tests.helpers import tiny_vqgan
    cfg, g = GAN_CASES["gan8"], gold()
    a = gan_args("hinge", 1.0)
    vqm, args = tiny_vqgan(n_codes=64)
    args.disc_channels, args.disc_layers, args.image_channels = cfg["ndf"], cfg["L"], 3
    for k, v in a.items():
        setattr(args, k, v)
    sd = dict(vqm.state_dict())
    sds = closed_form_state_dict(cfg["ndf"], cfg["L"], False), closed_form_state_dict(cfg["ndf"], cfg["L"], True)
    sd.update({D.IMAGE_PREFIX + k: v for k, v in sds[0].items()})
    sd.update({D.VIDEO_PREFIX + k: v for k, v in sds[1].items()})
    path = str(tmp_path / "gan.ckpt")
    torch.save({"state_dict": sd, "hyper_parameters": {"args": args}, "global_step": 12}, path)
    x, xr = structured_clip(cfg["shape"]), structured_clip(cfg["shape"], 1)
    batches = [(x, xr), (x.flip(0).contiguous(), xr.flip(0).contiguous())]
    terms = DiscTerms(path, torch.device(DEV), dtype, stats, seed=3)
    assert terms.global_step == 12
    for p, q in batches:
        terms.add(p.to(DEV), q.to(DEV))
    got = terms.result()
    assert list(got) == DISC_COLUMNS == list(G_KEYS + D_KEYS)
    training = stats == "batch"
    for net in (r.net for r in terms.runners):          # batch statistics leave the buffers untouched
        assert net.training == training and int(net.model1[1].num_batches_tracked) == 7
    want = np.zeros(13)
    for (p, q), fidx in zip(batches, terms.frame_idx):
        vals = {}
        for which in ("generator", "discriminator"):
            vals.update(D.gan_terms_twin(a, sds[0], sds[1], cfg["L"], p, q, fidx, 12, which, training=training, dtype=torch.float64))
        want += np.array([float(vals[k]) for k in DISC_COLUMNS]) / len(batches)
    tol = scalar_tolerances(g[f"gan8_{'train' if training else 'eval'}_callstats"], a, 12, dtype == "f16")
    for i, k in enumerate(DISC_COLUMNS):
        print(f"measure_recon --disc {dtype} {stats} {k}: {got[k]:.7f} vs {want[i]:.7f}, bound {tol[i]:.2e}")
        assert abs(got[k] - want[i]) <= tol[i], (k, got[k], want[i], tol[i])
    plain = str(tmp_path / "plain.ckpt")
    torch.save({"state_dict": vqm.state_dict(), "hyper_parameters": {"args": args}}, plain)
    with pytest.raises(SystemExit, match="holds no image_discriminator"):
        DiscTerms(plain, torch.device(DEV))
