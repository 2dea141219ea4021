"""Host-side checks of the discriminators' forward (mebt_amd/discriminator.py: arrange_weight, DiscRunner, gan_terms): the weight
arrangement against torch's convolutions, the C ABI's new symbols, every refusal that comes before a launch, and the flags of
`python -m mebt_amd.measure_recon --disc`.  No GPU."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from mebt_amd import _lib
from mebt_amd import discriminator as D
from tests.disc_common import ROOT, gan_args

NEW_SYMBOLS = ["mebt_op_disc_ingest", "mebt_op_disc_conv", "mebt_op_disc_bn_act", "mebt_op_disc_head"]


def _patches(x, three_d, stride):
    """every output voxel's receptive field as a row in the kernels' K order (tap, ci): [B * voxels, taps * Cin]"""
    pad = (2, 2, 2, 2, 2, 2) if three_d else (2, 2, 2, 2)
    p = F.pad(x, pad)
    if three_d:
        p = p.unfold(2, 4, stride).unfold(3, 4, stride).unfold(4, 4, stride)            # [B, C, To, Ho, Wo, 4, 4, 4]
        return p.permute(0, 2, 3, 4, 5, 6, 7, 1).reshape(-1, 64 * x.shape[1])
    p = p.unfold(2, 4, stride).unfold(3, 4, stride)                                     # [B, C, Ho, Wo, 4, 4]
    return p.permute(0, 2, 3, 4, 5, 1).reshape(-1, 16 * x.shape[1])


@pytest.mark.parametrize("three_d", [False, True])
@pytest.mark.parametrize("cin,cout,stride", [(3, 8, 2), (8, 72, 1), (64, 5, 2)])
def test_arrange_weight_is_the_convolution(cin, cout, stride, three_d):
    g = torch.Generator().manual_seed(cin * 100 + cout)
    shape = (2, cin, 3, 5, 6) if three_d else (2, cin, 5, 6)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    w = torch.randn((cout, cin) + ((4, 4, 4) if three_d else (4, 4)), generator=g, dtype=torch.float64)
    want = (F.conv3d if three_d else F.conv2d)(x, w, stride=stride, padding=2)
    cs = 4 if cin == 3 else cin
    a = D.arrange_weight(w.float(), "f32", cin_store=cs if cin == 3 else None)
    taps = 64 if three_d else 16
    K = taps * cs
    assert a.dtype == torch.float32 and tuple(a.shape) == (-(-cout // 64) * 64, -(-K // 32) * 32) and a.is_contiguous()
    assert float(a[cout:].abs().sum()) == 0 and float(a[:, K:].abs().sum()) == 0
    xs = torch.cat([x, torch.zeros(shape[0], cs - cin, *shape[2:], dtype=torch.float64)], 1)
    if cs != cin:                                                                       # the stored extra channel's columns are zero
        assert float(a[:cout, :K].view(cout, taps, cs)[:, :, cin:].abs().sum()) == 0
    got = _patches(xs, three_d, stride) @ a[:cout, :K].double().T                      # [M, cout]
    want_rows = want.permute(0, *range(2, want.dim()), 1).reshape(-1, cout)
    assert got.shape == want_rows.shape
    assert float((got - want_rows).abs().max()) <= 2.0 ** -20 * float(want.abs().max())  # the weight's rounding to fp32
    assert D.arrange_weight(w.float(), torch.float16).dtype == torch.float16
    with pytest.raises(ValueError, match="cin_store"):
        D.arrange_weight(w.float(), "f32", cin_store=cin + 2)
    with pytest.raises(ValueError, match="arrange_weight expects"):
        D.arrange_weight(torch.zeros(8, 3, 3, 3), "f32")


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mebt_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert D.TILE_ROWS == {"f16": 128, "f32": 64}
    tile = open(os.path.join(ROOT, "mebt_amd", "csrc", "mfma_tile.h")).read()
    assert re.search(r"TileCfg<f16_t>.*BM = 128", tile) and re.search(r"TileCfg<float>.*BM = 64", tile)


def test_runner_refuses_before_any_launch():
    img, vid = D.NLayerDiscriminator(3, 8, 2), D.NLayerDiscriminator3D(3, 8, 2)
    ri, rv = D.DiscRunner(img, "f32"), D.DiscRunner(vid)
    assert ri.dtype == "f32" and rv.dtype == "f16"
    assert [tuple(s["w"].shape) for s in ri.stages] == [(64, 64), (64, 128), (64, 256), (64, 512)]
    with pytest.raises(TypeError, match="DiscRunner expects"):
        D.DiscRunner(torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match="dtype must be"):
        D.DiscRunner(img, "bf16")
    # ranks and channels
    with pytest.raises(ValueError, match="expects a 4-D input"):
        ri(torch.zeros(2, 3, 4, 8, 8))
    with pytest.raises(ValueError, match="expects a 5-D input"):
        rv(torch.zeros(2, 3, 8, 8))
    with pytest.raises(ValueError, match="3 input channels"):
        ri(torch.zeros(2, 4, 8, 8))
    with pytest.raises(ValueError, match="frame_idx picks one frame"):
        rv(torch.zeros(2, 3, 4, 8, 8), frame_idx=[0, 1])
    with pytest.raises(ValueError, match="frame_idx picks one frame"):
        ri(torch.zeros(2, 3, 8, 8), frame_idx=[0, 1])
    # the frame index: range, count, kind
    for bad in ([0, 4], [-1, 0], [0], [0.5, 1.0]):
        with pytest.raises(ValueError, match="frame_idx must"):
            ri(torch.zeros(2, 3, 4, 8, 8), frame_idx=bad)
    # torch's refusal of a training-mode BatchNorm over one value per channel
    img.train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ri(torch.zeros(1, 3, 1, 1))
    img.eval()
    with pytest.raises(ValueError, match="fp32 input"):
        ri(torch.zeros(2, 3, 8, 8, dtype=torch.float16))
    # host tensors and host-resident holders
    with pytest.raises(RuntimeError, match="x must live on the GPU"):
        ri(torch.zeros(2, 3, 8, 8))
    with pytest.raises(RuntimeError, match="x must live on the GPU"):
        ri(torch.zeros(2, 3, 4, 8, 8), frame_idx=[3, 0])
    with pytest.raises(RuntimeError, match="x must live on the GPU"):
        rv(torch.zeros(2, 3, 4, 8, 8))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        D.ingest(torch.zeros(2, 3, 8, 8), "f16")
    with pytest.raises(RuntimeError, match="on the GPU"):
        D.conv_stage(torch.zeros(2, 1, 8, 8, 8), torch.zeros(64, 128), torch.zeros(8), 1, 2, 8)
    with pytest.raises(RuntimeError, match="on the GPU"):
        D.bn_act(torch.zeros(2, 1, 8, 8, 8), torch.zeros(2, 8), torch.zeros(8), torch.zeros(8))


def test_runner_notices_a_parameter_that_moved():
    net = D.NLayerDiscriminator(3, 8, 2)
    r = D.DiscRunner(net, "f32")
    assert not r._stale()
    with torch.no_grad():
        net.model1[0].weight.mul_(2.0)
    assert r._stale()
    before = r.stages[1]["w"].clone()
    r.refresh()
    assert not r._stale() and torch.equal(r.stages[1]["w"], 2.0 * before)


def test_gan_terms_refuses_before_any_launch():
    ri, rv = D.DiscRunner(D.NLayerDiscriminator(3, 8, 2)), D.DiscRunner(D.NLayerDiscriminator3D(3, 8, 2))
    a = gan_args("hinge", 1.0)
    x = torch.zeros(2, 3, 4, 8, 8)
    with pytest.raises(ValueError, match="which must be"):
        D.gan_terms(a, ri, rv, x, x, [0, 1], 0, "both")
    with pytest.raises(ValueError, match=r"must be \[B, 3, T, H, W\]"):
        D.gan_terms(a, ri, rv, x[:, :, 0], x[:, :, 0], [0, 1], 0, "generator")
    with pytest.raises(ValueError, match="differ in shape"):
        D.gan_terms(a, ri, rv, x, x[:, :, :2], [0, 1], 0, "generator")
    with pytest.raises(ValueError, match="in this order"):
        D.gan_terms(a, rv, ri, x, x, [0, 1], 0, "generator")
    with pytest.raises(ValueError, match="3 input channels"):
        D.gan_terms(a, ri, rv, torch.zeros(2, 1, 4, 8, 8), torch.zeros(2, 1, 4, 8, 8), [0, 1], 0, "generator")
    with pytest.raises(ValueError, match="frame_idx must lie in"):
        D.gan_terms(a, ri, rv, x, x, [0, 4], 0, "discriminator")
    ri.net.train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        D.gan_terms(a, ri, rv, torch.zeros(1, 3, 4, 1, 1), torch.zeros(1, 3, 4, 1, 1), [0], 0, "generator")
    ri.net.eval()
    for which in ("generator", "discriminator"):
        with pytest.raises(RuntimeError, match="x must live on the GPU"):
            D.gan_terms(a, ri, rv, x, x, [0, 1], 0, which)


def test_measure_recon_has_the_disc_flags_and_keeps_its_defaults():
    from mebt_amd import measure_recon as mr
    p = mr.build_parser()
    a = p.parse_args(["--vqgan_ckpt", "x.ckpt"])
    assert a.disc is False and a.disc_dtype == "f16" and a.disc_stats == "batch"
    assert (a.vqgan_dtype, a.seed, a.out, a.n_sample, a.lpips, a.lpips_every, a.lpips_dtype) == ("f16", 0, "recon.csv", 2048, False, 1, "f16")
    b = p.parse_args(["--disc", "--disc_dtype", "f32", "--disc_stats", "running"])
    assert b.disc is True and b.disc_dtype == "f32" and b.disc_stats == "running"
    with pytest.raises(SystemExit):
        p.parse_args(["--disc_stats", "both"])
    assert mr.DISC_COLUMNS == list(D.G_KEYS + D.D_KEYS) and len(mr.DISC_COLUMNS) == 13
