"""The discriminators' reductions on the GPU (csrc/disc/disc.hip, mebt_amd/discriminator.py): BatchNorm batch statistics and the loss
values against fp64 torch and against the golden of the real reference classes (tests/golden/disc), bit determinism and the argument
checks."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from mebt_amd import _lib  # noqa: E402
from mebt_amd import discriminator as D  # noqa: E402
from tests.disc_common import (CASES, D_KEYS, G_KEYS, GAN_CASES, GAN_CONFIGS, case_input, case_sd, closed_form_state_dict, gan_args,  # noqa: E402
                               gold, scalar_tolerances, structured_clip)

DEV = "cuda"
TDT = {"f16": torch.float16, "f32": torch.float32}


def cl(t):
    """logical [B, C, (T,) H, W] -> contiguous channels-last [B, (T,) H, W, C]"""
    return t.permute(0, *range(2, t.dim()), 1).contiguous()


# ---- BatchNorm statistics ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("M,Cc", [(2, 3), (127, 8), (128, 37), (129, 512), (5000, 24)])
def test_batch_stats_vs_fp64_torch(M, Cc, dtype):
    g = torch.Generator().manual_seed(M)
    x = (torch.randn(M, Cc, generator=g) * 1.5 + torch.randn(Cc, generator=g)).to(TDT[dtype])
    x[:, 0] = 0.75                                                    # a constant channel: variance 0, clamped, rstd = 1 / sqrt(eps)
    rm0, rv0 = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    x64 = x.double()
    mean, var = x64.mean(0), x64.var(0, unbiased=False)
    for update in (False, True):
        rm, rv, nbt = rm0.clone().to(DEV), rv0.clone().to(DEV), torch.tensor(7, device=DEV)
        stats = D.batch_stats(x.to(DEV), rm, rv, nbt, update).cpu().double()
        # fp64 sums of the stored values and one rounding to fp32; E[x^2] - mean^2 in fp64 loses about 2^-52 (mean^2 + var) / var
        assert torch.allclose(stats[0], mean, rtol=2.0 ** -23, atol=1e-12)
        assert torch.allclose(stats[1], 1 / torch.sqrt(var + 1e-5), rtol=2.0 ** -22)
        assert float(stats[1][0]) == pytest.approx(1 / np.sqrt(1e-5), rel=1e-6)
        if update:
            assert torch.allclose(rm.cpu().double(), 0.9 * rm0.double() + 0.1 * mean, rtol=2.0 ** -22, atol=1e-8)
            assert torch.allclose(rv.cpu().double(), 0.9 * rv0.double() + 0.1 * var * M / (M - 1), rtol=2.0 ** -22, atol=1e-8)
            assert int(nbt) == 8
        else:
            assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0) and int(nbt) == 7
    assert torch.equal(D.batch_stats(x.to(DEV)), D.batch_stats(x.to(DEV)))          # two runs: the same bits


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("c", list(CASES))
def test_batch_stats_reproduce_the_references_buffers(c, dtype):
    """the pre-BatchNorm map of every stage (the twin's, float64, rounded to the storage dtype) through the kernels: the running
    buffers after one training-mode call against the golden.  fp32: four times the recorded fp32-vs-float64 distance (at least one
    fp32 rounding); fp16: four times the recorded distance of the fp16-storage twin.  Both relative to the buffer's maximum."""
    cfg, g, sd = CASES[c], gold(), case_sd(c)
    three_d = cfg["three_d"]
    storage = torch.float16 if dtype == "f16" else None
    _, feats, _ = D.disc_twin(sd, case_input(c), cfg["L"], training=True, dtype=torch.float64, storage=storage)
    conv = F.conv3d if three_d else F.conv2d
    names = [k for k in sd if k.endswith(("running_mean", "running_var"))]
    for n in range(1, cfg["L"] + 1):
        w = sd[f"model{n}.0.weight"].to(TDT[dtype]).double()
        pre = conv(feats[n - 1], w, sd[f"model{n}.0.bias"].double(), stride=2 if n < cfg["L"] else 1, padding=2)
        rm, rv = sd[f"model{n}.1.running_mean"].clone().to(DEV), sd[f"model{n}.1.running_var"].clone().to(DEV)
        nbt = sd[f"model{n}.1.num_batches_tracked"].clone().to(DEV)
        D.batch_stats(cl(pre).to(DEV, TDT[dtype]), rm, rv, nbt, True)
        for k, got in ((f"model{n}.1.running_mean", rm), (f"model{n}.1.running_var", rv)):
            d32, d16, mx = g[f"{c}_train_bufstats"][names.index(k)]
            gate = 4 * (max(d32, 2.0 ** -24) if dtype == "f32" else d16) * mx
            err = float((got.double().cpu() - torch.from_numpy(g[f"{c}_train_buf_{k}"]).double()).abs().max())
            print(f"batch_stats {c} {dtype} {k}: distance {err / mx:.3e} of the maximum, gate {gate / mx:.3e}")
            assert err <= gate, (k, err, gate)
        assert int(nbt) == int(g[f"{c}_train_buf_model{n}.1.num_batches_tracked"]) == 8


def test_batch_stats_refuses_one_value_per_channel():
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        D.batch_stats(torch.zeros(1, 1, 1, 8, device=DEV))
    with pytest.raises(ValueError, match="running_mean"):
        D.batch_stats(torch.zeros(4, 8, device=DEV), update=True)
    # buffers the kernel would write through host pointers, or past their end: refused before the launch
    x, f, nbt = torch.zeros(4, 8, device=DEV), torch.zeros(8, device=DEV), torch.tensor(7, device=DEV)
    with pytest.raises(RuntimeError, match="running_var must live on the GPU"):
        D.batch_stats(x, f, f.cpu(), nbt, True)
    with pytest.raises(RuntimeError, match="num_batches must live on the GPU"):
        D.batch_stats(x, f, f, nbt.cpu(), True)
    with pytest.raises(ValueError, match="num_batches must be a torch.int64"):
        D.batch_stats(x, f, f, nbt.to(torch.int32), True)
    with pytest.raises(ValueError, match="contiguous with 8"):
        D.batch_stats(x, f, torch.zeros(4, device=DEV), nbt, True)
    with pytest.raises(RuntimeError, match="out must live on the GPU"):
        D.disc_losses(logits=x, out=torch.zeros(6, dtype=torch.float64))
    with pytest.raises(ValueError, match="out must be a torch.float64"):
        D.disc_losses(logits=x, out=torch.zeros(6, device=DEV))
    torch.cuda.synchronize()
    assert float(f.abs().sum()) == 0 and int(nbt) == 7
    out = torch.full((6,), 3.0, device=DEV, dtype=torch.float64)
    assert D.disc_losses(logits=x + 1, out=out) is out and out.tolist()[:3] == [1.0, 0.0, 2.0] and float(out[5]) == 3.0
    st, slots = torch.zeros(2, 8, device=DEV), torch.zeros(16, device=DEV, dtype=torch.float64)
    rc = _lib.load().mebt_op_disc_bn_finish(slots.data_ptr(), 1, 8, 1, st.data_ptr(), None, None, None, 0, _lib.cur_stream())
    assert rc == 2 and b"more than 1 value per channel" in _lib.load().mebt_last_error()


# ---- loss values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("n", [1, 255, 2049, 2048 * 1024 + 77])
def test_disc_losses_vs_fp64_torch(n, dtype):
    g = torch.Generator().manual_seed(n)
    l = (torch.randn(n, generator=g) * 3).to(TDT[dtype])
    a, b = torch.randn(n, generator=g).to(TDT[dtype]), torch.randn(n, generator=g).to(TDT[dtype])
    l[0] = 25.0                                    # past softplus's threshold
    out = D.disc_losses(l.to(DEV), a.to(DEV), b.to(DEV)).cpu()
    ld = l.double()
    want = torch.stack([ld.mean(), F.relu(1 - ld).mean(), F.relu(1 + ld).mean(), F.softplus(-ld).mean(), F.softplus(ld).mean(),
                        (a.double() - b.double()).abs().mean()])
    assert torch.allclose(out, want, rtol=1e-12, atol=1e-13), (out, want)
    assert torch.equal(out, D.disc_losses(l.to(DEV), a.to(DEV), b.to(DEV)).cpu())
    only = D.disc_losses(feat_a=a.to(DEV), feat_b=b.to(DEV)).cpu()
    assert float(only[:5].abs().sum()) == 0 and only[5] == out[5]
    real, fake = l.to(DEV), a.to(DEV)
    assert float(D.hinge_d_loss(real, fake)) == pytest.approx(float(0.5 * (F.relu(1 - ld).mean() + F.relu(1 + a.double()).mean())), rel=1e-12)
    assert float(D.vanilla_d_loss(real, fake)) == pytest.approx(float(0.5 * (F.softplus(-ld).mean() + F.softplus(a.double()).mean())), rel=1e-12)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("gcase", list(GAN_CASES))
def test_loss_values_equal_the_references(gcase, mode, dtype):
    """the reference's thirteen logged values from the twin's stage outputs (float64, rounded to the storage dtype) through the HIP
    reductions, for hinge and vanilla, both feature weights and both sides of discriminator_iter_start"""
    cfg, g = GAN_CASES[gcase], gold()
    x, xr = structured_clip(cfg["shape"]), structured_clip(cfg["shape"], 1)
    B, Cc, T, H, W = x.shape
    sel = torch.from_numpy(g[f"{gcase}_frame_idx"]).reshape(-1, 1, 1, 1, 1).repeat(1, Cc, 1, H, W)
    fr, frr = torch.gather(x, 2, sel).squeeze(2), torch.gather(xr, 2, sel).squeeze(2)
    sds = closed_form_state_dict(cfg["ndf"], cfg["L"], False), closed_form_state_dict(cfg["ndf"], cfg["L"], True)
    storage = torch.float16 if dtype == "f16" else None
    calls = []
    for three_d, inp in ((False, fr), (False, frr), (True, x), (True, xr)):          # image real / fake, video real / fake
        _, feats, _ = D.disc_twin(sds[three_d], inp, cfg["L"], training=mode == "train", dtype=torch.float64, storage=storage)
        calls.append([cl(f).to(DEV, TDT[dtype]) for f in feats])
    ir, if_, vr, vf = calls
    for kind, gfw, step in GAN_CONFIGS:
        a = gan_args(kind, gfw)
        factor = D.adopt_weight(step, threshold=a["discriminator_iter_start"])
        d_loss = D.hinge_d_loss if kind == "hinge" else D.vanilla_d_loss
        got = {"g_image_loss": -D.disc_losses(logits=if_[-1])[0], "g_video_loss": -D.disc_losses(logits=vf[-1])[0],
               "image_gan_feat_loss": D.feature_matching(if_, ir), "video_gan_feat_loss": D.feature_matching(vf, vr),
               "logits_image_real": D.disc_losses(logits=ir[-1])[0], "logits_image_fake": D.disc_losses(logits=if_[-1])[0],
               "logits_video_real": D.disc_losses(logits=vr[-1])[0], "logits_video_fake": D.disc_losses(logits=vf[-1])[0],
               "d_image_loss": d_loss(ir[-1], if_[-1]), "d_video_loss": d_loss(vr[-1], vf[-1])}
        assert all(v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda for v in got.values())
        got["aeloss"] = factor * (got["g_image_loss"] + got["g_video_loss"])
        got["gan_feat_loss"] = factor * gfw * (got["image_gan_feat_loss"] + got["video_gan_feat_loss"])
        got["discloss"] = factor * (got["d_image_loss"] + got["d_video_loss"])
        want = g[f"{gcase}_{mode}_{kind}_{int(gfw)}_{step}_ref"]
        tol = scalar_tolerances(g[f"{gcase}_{mode}_callstats"], a, step, dtype == "f16")
        for i, k in enumerate(G_KEYS + D_KEYS):
            print(f"loss values {gcase} {mode} {dtype} {kind} {gfw} {step} {k}: {float(got[k]):.7f} vs {want[i]:.7f}, bound {tol[i]:.2e}")
            assert abs(float(got[k]) - want[i]) <= tol[i], (k, kind, gfw, step, float(got[k]), want[i], tol[i])


# ---- rejected arguments --------------------------------------------------------------------------------------------------------------------
def test_argument_checks_return_the_status_without_launching():
    lib = _lib.load()
    s = _lib.cur_stream()
    out = torch.full((9, 16), 7.0, device=DEV, dtype=torch.float16)
    slots = torch.zeros(16 * 2, device=DEV, dtype=torch.float64)
    st, f = torch.zeros(2, 16, device=DEV), torch.zeros(16, device=DEV)
    for rc, who, call in [
            (1, b"disc_bn_partials", lambda: lib.mebt_op_disc_bn_partials(_lib.F16, None, 9, 16, slots.data_ptr(), 256, s)),
            (1, b"disc_bn_partials", lambda: lib.mebt_op_disc_bn_partials(_lib.F16, out.data_ptr(), 9, 16, None, 256, s)),
            (1, b"disc_bn_partials", lambda: lib.mebt_op_disc_bn_partials(_lib.F16, out.data_ptr(), 9, 16, slots.data_ptr() + 4, 256, s)),
            (2, b"disc_bn_partials", lambda: lib.mebt_op_disc_bn_partials(_lib.F16, out.data_ptr(), 0, 16, slots.data_ptr(), 256, s)),
            (4, b"disc_bn_partials", lambda: lib.mebt_op_disc_bn_partials(_lib.F16, out.data_ptr(), 9, 16, slots.data_ptr(), 255, s)),
            (5, b"disc_bn_partials", lambda: lib.mebt_op_disc_bn_partials(_lib.BF16, out.data_ptr(), 9, 16, slots.data_ptr(), 256, s)),
            (1, b"disc_bn_finish", lambda: lib.mebt_op_disc_bn_finish(None, 1, 16, 9, st.data_ptr(), None, None, None, 0, s)),
            (1, b"disc_bn_finish", lambda: lib.mebt_op_disc_bn_finish(slots.data_ptr(), 1, 16, 9, None, None, None, None, 0, s)),
            (1, b"disc_bn_finish", lambda: lib.mebt_op_disc_bn_finish(slots.data_ptr(), 1, 16, 9, st.data_ptr(), f.data_ptr(), None, None, 1, s)),
            (2, b"disc_bn_finish", lambda: lib.mebt_op_disc_bn_finish(slots.data_ptr(), 0, 16, 9, st.data_ptr(), None, None, None, 0, s)),
            (2, b"disc_bn_finish", lambda: lib.mebt_op_disc_bn_finish(slots.data_ptr(), 1, 16, 1, st.data_ptr(), None, None, None, 0, s)),
            (1, b"disc_losses", lambda: lib.mebt_op_disc_losses(_lib.F16, None, 9, None, None, 0, slots.data_ptr(), slots.data_ptr(), 256, s)),
            (1, b"disc_losses", lambda: lib.mebt_op_disc_losses(_lib.F16, out.data_ptr(), 9, None, None, 0, None, slots.data_ptr(), 256, s)),
            (1, b"disc_losses", lambda: lib.mebt_op_disc_losses(_lib.F16, None, 0, out.data_ptr(), None, 9, slots.data_ptr(), slots.data_ptr(), 256, s)),
            (2, b"disc_losses", lambda: lib.mebt_op_disc_losses(_lib.F16, None, 0, None, None, 0, slots.data_ptr(), slots.data_ptr(), 256, s)),
            (4, b"disc_losses", lambda: lib.mebt_op_disc_losses(_lib.F16, out.data_ptr(), 9, None, None, 0, slots.data_ptr(), slots.data_ptr(), 39, s)),
            (1, b"disc_losses", lambda: lib.mebt_op_disc_losses(_lib.F16, out.data_ptr(), 9, None, None, 0, slots.data_ptr(), None, 256, s)),
            (5, b"disc_losses", lambda: lib.mebt_op_disc_losses(_lib.BF16, out.data_ptr(), 9, None, None, 0, slots.data_ptr(), slots.data_ptr(), 256, s))]:
        assert call() == rc, lib.mebt_last_error()
        assert lib.mebt_last_error().startswith(who + b": ")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and float(slots.abs().sum()) == 0 and float(st.abs().sum()) == 0
    assert lib.mebt_disc_losses_scratch_bytes(9, 0) == 40 and lib.mebt_disc_losses_scratch_bytes(2049, 5000) == 8 * (10 + 3)
    assert lib.mebt_disc_losses_scratch_bytes(0, 0) == 0 and lib.mebt_disc_losses_scratch_bytes(10 ** 9, 0) == 8 * 5 * 1024
