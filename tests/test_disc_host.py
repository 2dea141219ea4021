"""Host-side checks of the first-stage discriminators (mebt_amd/discriminator.py): geometry, state-dict schema, checkpoint access, the
plain-torch twins against the golden of the real reference classes (tests/golden/disc), the command's flags and the C ABI's symbols.
No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mebt_amd import _lib
from mebt_amd import discriminator as D
from tests.disc_common import (CASES, D_KEYS, G_KEYS, GAN_CASES, GAN_CONFIGS, ROOT, SD_CONFIGS, case_input, case_sd, check_against_golden,
                               closed_form_state_dict, gan_args, gold, scalar_tolerances, structured_clip)
from tests.helpers import tiny_vqgan

NEW_SYMBOLS = ["mebt_op_disc_bn_partials", "mebt_op_disc_bn_finish", "mebt_disc_losses_scratch_bytes", "mebt_op_disc_losses"]


def test_log_names_are_the_golden_ones():
    assert D.G_KEYS == G_KEYS and D.D_KEYS == D_KEYS


@pytest.mark.parametrize("three_d", [False, True])
@pytest.mark.parametrize("ndf,L", SD_CONFIGS)
def test_state_dict_schema_is_the_references(ndf, L, three_d):
    g = gold()
    tag = f"sd_{ndf}_{L}_{'3d' if three_d else '2d'}"
    keys = [str(k) for k in g[tag + "_keys"]]
    shapes = [tuple(int(v) for v in row if v >= 0) for row in g[tag + "_shapes"]]
    net = (D.NLayerDiscriminator3D if three_d else D.NLayerDiscriminator)(3, ndf, L)
    sd = net.state_dict()
    assert list(sd) == keys and [tuple(v.shape) for v in sd.values()] == shapes
    assert D.expected_keys(ndf, L, three_d) == dict(zip(keys, shapes))
    # the plan's channels are the weights' and reach the 512 cap
    plan = D.layer_plan(3, ndf, L, (4, 16, 16) if three_d else (1, 16, 16), three_d)
    assert [(e["cout"], e["cin"]) for e in plan] == [s[:2] for k, s in zip(keys, shapes) if k.endswith(".0.weight")]
    assert max(e["cout"] for e in plan) == min(ndf * 2 ** L, 512) and plan[-1]["cout"] == 1
    # strict round trip in both directions
    cf_sd = closed_form_state_dict(ndf, L, three_d)
    net.load_state_dict(cf_sd, strict=True)
    back = net.state_dict()
    assert list(back) == list(cf_sd) and all(torch.equal(back[k], cf_sd[k]) for k in cf_sd)


@pytest.mark.parametrize("c", list(CASES))
def test_layer_plan_gives_the_recorded_output_shapes(c):
    cfg, g = CASES[c], gold()
    shape = cfg["shape"]
    net = (D.NLayerDiscriminator3D if cfg["three_d"] else D.NLayerDiscriminator)(3, cfg["ndf"], cfg["L"])
    plan = net.plan(shape)
    assert len(plan) == cfg["L"] + 2
    for n, e in enumerate(plan):
        want = tuple(g[f"{c}_eval_shape{n}"])
        assert (shape[0], e["cout"]) + (e["out_dims"] if cfg["three_d"] else e["out_dims"][1:]) == want
        assert e["stride"] == (2 if n < cfg["L"] else 1) and e["bn"] == (1 <= n <= cfg["L"]) and e["act"] == (n <= cfg["L"])
        assert e["K"] == (64 if cfg["three_d"] else 16) * e["cin"]


def test_training_geometry_of_the_issue():
    plan = D.layer_plan(3, 64, 3, (16, 128, 128), True)
    assert [(e["cout"],) + e["out_dims"] for e in plan] == [(64, 9, 65, 65), (128, 5, 33, 33), (256, 3, 17, 17), (512, 4, 18, 18), (1, 5, 19, 19)]
    assert [e["K"] for e in plan] == [192, 4096, 8192, 16384, 32768]
    assert 30e9 < D.plan_flops(plan, 1) < 34e9
    assert 1.8e9 < D.plan_flops(D.layer_plan(3, 64, 3, (1, 128, 128), False), 1) < 2.3e9


def _full_checkpoint(ndf=8, L=3):
    vqm, args = tiny_vqgan(n_codes=64)
    args.disc_channels, args.disc_layers, args.image_channels = ndf, L, 3
    sd = dict(vqm.state_dict())
    sd.update(closed_form_state_dict(ndf, L, False, prefix=D.IMAGE_PREFIX))
    sd.update(closed_form_state_dict(ndf, L, True, prefix=D.VIDEO_PREFIX))
    return vqm, args, sd


def test_extract_and_read_file(tmp_path):
    vqm, args, sd = _full_checkpoint()
    img, vid = D.extract(sd)
    want_i, want_v = closed_form_state_dict(8, 3, False), closed_form_state_dict(8, 3, True)
    assert list(img) == list(want_i) and list(vid) == list(want_v)
    assert all(torch.equal(img[k], want_i[k]) for k in img) and all(torch.equal(vid[k], want_v[k]) for k in vid)
    path = str(tmp_path / "gan.ckpt")
    torch.save({"state_dict": sd, "hyper_parameters": {"args": args}, "global_step": 3}, path)
    img2, vid2 = D.read_file(path)
    assert all(torch.equal(img2[k], want_i[k]) for k in img2) and all(torch.equal(vid2[k], want_v[k]) for k in vid2)
    nets = D.load_discriminators(path, torch.device("cpu"), "f32")
    assert isinstance(nets[0], D.NLayerDiscriminator) and isinstance(nets[1], D.NLayerDiscriminator3D)
    assert (nets[1].ndf, nets[1].n_layers, nets[1].compute_dtype, nets[1].training) == (8, 3, "f32", False)
    assert D.load_discriminators(path, torch.device("cpu"))[0].compute_dtype == "f16"
    with pytest.raises(ValueError, match="dtype"):
        D.load_discriminators(path, torch.device("cpu"), "bf16")
    assert all(torch.equal(v, want_v[k]) for k, v in nets[1].state_dict().items())
    # a partial set raises and names the key; no tensors at all: None
    part = {k: v for k, v in sd.items() if k != D.VIDEO_PREFIX + "model2.1.running_var"}
    with pytest.raises(ValueError, match=re.escape(D.VIDEO_PREFIX + "model2.1.running_var")):
        D.extract(part)
    with pytest.raises(ValueError, match=re.escape(D.IMAGE_PREFIX + "model0.0.weight")):
        D.extract({k: v for k, v in sd.items() if not k.startswith(D.IMAGE_PREFIX)})
    assert D.extract(dict(vqm.state_dict())) is None
    plain = str(tmp_path / "plain.ckpt")
    torch.save({"state_dict": vqm.state_dict(), "hyper_parameters": {"args": args}}, plain)
    assert D.read_file(plain) is None
    with pytest.raises(ValueError, match="holds no image_discriminator"):
        D.load_discriminators(plain, torch.device("cpu"))


def test_vqgan_still_skips_the_discriminator_keys():
    vqm, args, sd = _full_checkpoint()
    before = {k: v.clone() for k, v in vqm.state_dict().items()}
    vqm.load_state_dict(sd, strict=True)
    after = vqm.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert not any(k.startswith((D.IMAGE_PREFIX, D.VIDEO_PREFIX)) for k in after)


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("c", list(CASES))
def test_twin_equals_the_reference(c, mode):
    cfg, g = CASES[c], gold()
    logits, feats, bufs = D.disc_twin(case_sd(c), case_input(c), cfg["L"], training=mode == "train", dtype=torch.float64)
    check_against_golden(c, mode, "f32", logits, feats, report=lambda s: None)
    if mode == "train":
        names = [k for k in bufs if not k.endswith("tracked")]
        assert len(names) == len(g[f"{c}_train_bufstats"]) == 2 * cfg["L"]
        for k in bufs:
            want = torch.from_numpy(np.asarray(g[f"{c}_train_buf_{k}"]))
            if k.endswith("tracked"):
                assert int(bufs[k]) == int(want) == 8
            else:
                d32, _, mx = g[f"{c}_train_bufstats"][names.index(k)]
                assert float((bufs[k] - want.double()).abs().max()) <= 4 * max(d32, 2.0 ** -24) * mx, k
    else:
        assert bufs == {}


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("gcase", list(GAN_CASES))
def test_gan_terms_twin_equals_the_reference(gcase, mode):
    cfg, g = GAN_CASES[gcase], gold()
    x, xr = structured_clip(cfg["shape"]), structured_clip(cfg["shape"], 1)
    sds = closed_form_state_dict(cfg["ndf"], cfg["L"], False), closed_form_state_dict(cfg["ndf"], cfg["L"], True)
    for kind, gfw, step in GAN_CONFIGS:
        a = gan_args(kind, gfw)
        got = {}
        for which in ("generator", "discriminator"):
            got.update(D.gan_terms_twin(a, sds[0], sds[1], cfg["L"], x, xr, g[f"{gcase}_frame_idx"], step, which, training=mode == "train"))
        assert list(got) == ["g_image_loss", "g_video_loss", "aeloss", "image_gan_feat_loss", "video_gan_feat_loss", "gan_feat_loss"] + list(D_KEYS)
        want = g[f"{gcase}_{mode}_{kind}_{int(gfw)}_{step}_ref"]
        tol = scalar_tolerances(g[f"{gcase}_{mode}_callstats"], a, step, False)
        for i, k in enumerate(G_KEYS + D_KEYS):
            assert abs(float(got[k]) - want[i]) <= tol[i], (k, kind, gfw, step, float(got[k]), want[i])
        if step < 10:
            assert float(got["aeloss"]) == 0 and float(got["discloss"]) == 0 and float(got["gan_feat_loss"]) == 0
        else:
            assert float(got["discloss"]) > 0 and (float(got["gan_feat_loss"]) > 0) == (gfw > 0)
    # a GAN weight of 0 leaves its real side out
    a = gan_args("hinge", 1.0, image_gan_weight=0.0)
    got = D.gan_terms_twin(a, sds[0], sds[1], cfg["L"], x, xr, g[f"{gcase}_frame_idx"], 10, "generator")
    assert float(got["image_gan_feat_loss"]) == 0 and float(got["video_gan_feat_loss"]) > 0


def test_one_value_per_channel_in_training_mode_is_refused():
    net = D.NLayerDiscriminator(3, 8, 2).train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        net.check_batch((1, 3, 1, 1))
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        D.disc_twin(closed_form_state_dict(8, 2, False), torch.zeros(1, 3, 1, 1), 2, training=True)
    assert len(net.check_batch((2, 3, 1, 1))) == 4 and len(net.eval().check_batch((1, 3, 1, 1))) == 4
    for bad in [(2, 3, 4, 8, 8), (2, 4, 8, 8), (2, 3, 0, 8)]:
        with pytest.raises(ValueError):
            net.plan(bad)
    with pytest.raises(ValueError):
        D.NLayerDiscriminator3D(3, 12, 3).plan((1, 3, 4, 8, 8))


def test_forward_is_not_built_and_host_tensors_are_refused_before_any_launch():
    with pytest.raises(NotImplementedError, match="forward is not built"):
        D.NLayerDiscriminator(3, 8, 2)(torch.zeros(2, 3, 8, 8))
    z = torch.zeros(4, 8)
    for call in (lambda: D.disc_losses(logits=z), lambda: D.hinge_d_loss(z, z), lambda: D.feature_matching([z, z], [z, z]),
                 lambda: D.batch_stats(z), lambda: D.disc_losses(logits=z.to(torch.int32))):
        with pytest.raises(RuntimeError, match="on the GPU"):
            call()
    with pytest.raises(ValueError):
        D.disc_losses()
    with pytest.raises(NotImplementedError, match="forward is not built"):
        D.NLayerDiscriminator3D(3, 8, 2)(torch.zeros(2, 3, 2, 8, 8), update_running=False)


def test_buffers_a_kernel_writes_are_checked_before_any_launch(tmp_path):
    """running_mean, running_var, num_batches and a caller's `out` go to the kernels as raw pointers: dtype, size, contiguity and
    device are refused first, whatever the input is"""
    x, f = torch.zeros(4, 8), torch.zeros(8)
    nbt = torch.tensor(7)
    for kw, exc, what in [(dict(running_mean=f, running_var=f, update=True), RuntimeError, "running_mean must live on the GPU"),
                          (dict(running_mean=f.double(), running_var=f, update=True), ValueError, "running_mean must be a torch.float32"),
                          (dict(running_mean=f, running_var=f.half(), update=True), ValueError, "running_var must be a torch.float32"),
                          (dict(running_mean=f, running_var=torch.zeros(7), update=True), ValueError, "running_var must be contiguous with 8"),
                          (dict(running_mean=torch.zeros(8, 2)[:, 0], running_var=f, update=True), ValueError, "not contiguous"),
                          (dict(running_mean=f, running_var=f, num_batches=nbt.to(torch.int32), update=True), ValueError, "num_batches must be a torch.int64"),
                          (dict(running_mean=f, running_var=f, num_batches=torch.zeros(2, dtype=torch.int64), update=True), ValueError, "1 element"),
                          (dict(running_mean=[0.0] * 8, running_var=f, update=True), ValueError, "running_mean must be"),
                          (dict(update=True), ValueError, "needs running_mean"),
                          (dict(num_batches=nbt), RuntimeError, "num_batches must live on the GPU")]:
        with pytest.raises(exc, match=re.escape(what)):
            D.batch_stats(x, **kw)
    # the buffers of a CPU-resident holder, as load_discriminators(path, 'cpu') builds it
    vqm, args, sd = _full_checkpoint()
    path = str(tmp_path / "gan.ckpt")
    torch.save({"state_dict": sd, "hyper_parameters": {"args": args}}, path)
    bn = D.load_discriminators(path, "cpu")[0].model1[1]
    with pytest.raises(RuntimeError, match="running_mean must live on the GPU"):
        D.batch_stats(torch.zeros(4, bn.num_features), bn.running_mean, bn.running_var, bn.num_batches_tracked, True)
    for out, exc, what in [(torch.zeros(6), ValueError, "out must be a torch.float64"), (torch.zeros(5, dtype=torch.float64), ValueError, "6 element"),
                           (torch.zeros(6, 2, dtype=torch.float64)[:, 0], ValueError, "not contiguous"),
                           (torch.zeros(6, dtype=torch.float64), RuntimeError, "out must live on the GPU")]:
        with pytest.raises(exc, match=re.escape(what)):
            D.disc_losses(logits=x, out=out)


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mebt_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
    assert re.search(r"#define MEBT_DISC_BN_ROWS %d\b" % D.BN_ROWS, header)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
