"""LPIPS backward, host side (no GPU): the data-gradient weight arrangement, the float64 twin at given decisions against plain autograd,
the closed formulas the operator tests use against autograd, the fixture (tests/golden/lpips_grad) and its regeneration, the flags of
`python -m mebt_amd.train_vqgan` for the perceptual term, the checkpoint's `perceptual_model.*` round trip and the exported symbols."""
import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lpips")
REF = os.environ.get("MEBT_REFERENCE", "/root/reference")
sys.path.insert(0, GOLD)

from make_golden_lpips import CASES, closed_form_state_dict, to_input  # noqa: E402
from mebt_amd import lpips as LP  # noqa: E402
from tests import lpips_grad_common as lg  # noqa: E402


@pytest.fixture(scope="module")
def sd():
    return closed_form_state_dict()


@pytest.fixture(scope="module")
def fx():
    return lg.load_fixture()


def images(tag):
    g = np.load(os.path.join(GOLD, "lpips_golden.npz"))
    return to_input(g[f"a_{tag}"]), to_input(g[f"b_{tag}"])


@pytest.mark.parametrize("cin,cout", [(3, 64), (64, 64), (128, 256)])
def test_arrange_weight_dgrad_in_the_forward_layout_is_conv_transpose2d(cin, cout):
    g = torch.Generator().manual_seed(cin + cout)
    w = torch.randn(cout, cin, 3, 3, generator=g).double()             # fp32 values: the arrangement passes through float32
    dy = torch.randn(2, 5, 7, cout, generator=g, dtype=torch.float64)
    wl = LP.arrange_weight_dgrad(w, torch.float64)
    assert tuple(wl.shape) == (-(-cin // 64) * 64, -(-9 * cout // 32) * 32)
    assert float(wl[cin:].abs().max() if wl.shape[0] > cin else 0.0) == 0.0 and float(wl[:, 9 * cout:].abs().sum()) == 0.0
    got = lg.conv_as_forward_layout(dy, wl, cout, cin)
    want = F.conv_transpose2d(dy.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert LP.arrange_weight_dgrad(w, torch.float16).dtype == torch.float16


@pytest.mark.parametrize("tag", ["s16", "odd"])
def test_twin_at_its_own_decisions_is_autograd(sd, tag):
    a, b = images(tag)
    bq = b.double().clone().requires_grad_(True)
    val, _ = LP.lpips_twin(sd, a, bq)
    val.sum().backward()
    v2, g2, d_feats, acts = lg.twin_at(sd, a, b)
    assert torch.equal(v2, val.detach())
    assert float((g2 - bq.grad).abs().max()) <= 1e-12 * float(bq.grad.abs().max())
    # fed back as decisions, its own activations change nothing
    v3, g3, d3, _ = lg.twin_at(sd, a, b, decisions=acts)
    assert torch.equal(v3, v2) and torch.equal(g3, g2) and all(torch.equal(p, q) for p, q in zip(d3, d_feats))
    assert [tuple(t.shape[1:]) for t in acts] == [(c, h, w) for (_s, h, w, _ci, c, _f) in LP.plan_flops(*CASES[tag][1:])[1]]


def test_twin_at_foreign_decisions_differs_only_through_them(sd):
    """one ReLU decision of the deepest slice switched off: the gradient moves, the value does not follow the mask's own sign rule"""
    a, b = images("s16")
    _, g0, _, acts = lg.twin_at(sd, a, b)
    dec = [t.clone() for t in acts]
    pos = dec[12].flatten().argmax()
    dec[12].view(-1)[pos] = 0.0
    _, g1, _, _ = lg.twin_at(sd, a, b, decisions=dec)
    assert float((g1 - g0).abs().max()) > 0.0


def test_head_formula_and_pool_rule_are_autograd(sd):
    g = torch.Generator().manual_seed(5)
    n, P, C = 2, 6, 64
    f0, f1 = torch.randn(n, P, C, generator=g, dtype=torch.float64).relu(), torch.randn(n, P, C, generator=g, dtype=torch.float64).relu()
    w = torch.rand(C, generator=g, dtype=torch.float64)
    q = f1.clone().requires_grad_(True)
    to4 = lambda t: t.permute(0, 2, 1).reshape(n, C, 2, 3)
    (LP.head_twin(to4(f0), to4(q), w).sum() * 0.75).backward()
    want = torch.where(f1 > 0, q.grad, torch.zeros_like(f1))
    got = lg.head_bwd_formula(f0, f1, w, 0.75)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    x = torch.randn(2, 5, 7, 3, generator=g, dtype=torch.float64).relu() + 0.01
    xq = x.clone().requires_grad_(True)
    dy = torch.randn(2, 2, 3, 3, generator=g, dtype=torch.float64)
    F.max_pool2d(xq.permute(0, 3, 1, 2), 2, 2).backward(dy.permute(0, 3, 1, 2))
    assert torch.equal(lg.pool_bwd_rule(x, dy), xq.grad)


def test_fixture_loads_and_the_references_own_rounding_is_inside_the_gate(fx):
    for tag, (N, H, W) in CASES.items():
        g = fx[f"grad_{tag}"]
        assert g.dtype == np.float32 and g.shape == (N, 3, H, W) and np.isfinite(g).all() and np.abs(g).max() > 0
        assert float(fx[f"dev_{tag}"]) <= lg.REF_GATE, (tag, float(fx[f"dev_{tag}"]))
    names = [k[len("vqmax/"):] for k in fx if k.startswith("vqmax/")]
    assert len(names) == 68 and all("vqdot/" + k in fx and "twin_dev/" + k in fx for k in names)
    full = [k for k in names if "vqgrad/" + k in fx]
    assert full and all(fx["vqgrad/" + k].nbytes < 64 * 1024 for k in full)
    for k in full:
        g = fx["vqgrad/" + k].astype(np.float64)
        assert abs(np.abs(g).max() - float(fx["vqmax/" + k])) <= 1e-6 * float(fx["vqmax/" + k])
        assert abs((g * lg.probe(k, g.shape)).sum() - float(fx["vqdot/" + k])) <= 1e-5 * np.abs(g).sum()
    assert fx["vq_frame_idx"].shape == (2,) and fx["vq_losses"].shape == (3,) and fx["vq_losses"][2] > 0
    assert fx["layer_max_full"].shape == (14,)
    table = np.array((LP.GRAD_MAX_INPUT,) + LP.GRAD_MAX_TABLE)
    assert np.abs(table / fx["layer_max_full"] - 1).max() <= 5e-3, "mebt_amd.lpips.GRAD_MAX_TABLE is the fixture's measurement"
    for path in os.listdir(lg.GOLDEN_DIR):
        assert os.path.getsize(os.path.join(lg.GOLDEN_DIR, path)) < 1024 * 1024, path


def test_the_float64_twin_matches_the_reference_fixture(sd, fx):
    for tag in ("s16", "mid"):
        a, b = images(tag)
        _, g, _, _ = lg.twin_at(sd, a, b)
        ref = fx[f"grad_{tag}"].astype(np.float64)
        err = np.abs(g.numpy() / CASES[tag][0] - ref).max() / np.abs(ref).max()
        assert err <= lg.REF_GATE, (tag, err)


def test_default_branch_scale_is_a_power_of_two_with_headroom():
    import math
    for coef, H, W in ((64.0, 16, 16), (1.0, 128, 128), (8192.0 / 16, 128, 128), (1e-9, 64, 64)):
        s = LP.default_branch_scale(coef, H, W)
        assert math.frexp(s)[0] == 0.5
        top = coef * s * LP.GRAD_MAX_INPUT * LP.GRAD_TABLE_PIXELS / (H * W)
        assert LP.GRAD_TARGET / 2 < top <= LP.GRAD_TARGET
    assert LP.default_branch_scale(0.0, 16, 16) == 1.0


def test_golden_lpips_grad_fixture_regenerates_identically(tmp_path, fx):
    if not os.path.isdir(REF):
        pytest.skip("reference tree not available")
    env = dict(os.environ, MEBT_GOLDEN_OUT=str(tmp_path))
    out = subprocess.run([sys.executable, os.path.join(lg.GOLDEN_DIR, "make_golden_lpips_grad.py")], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    again = {}
    for name in sorted(os.listdir(tmp_path)):
        with np.load(os.path.join(tmp_path, name)) as z:
            again.update({k: z[k] for k in z.files})
    assert sorted(again) == sorted(fx)
    for k in fx:
        assert again[k].dtype == fx[k].dtype and again[k].shape == fx[k].shape and np.array_equal(again[k], fx[k]), k


# ---- the command and its checkpoints -------------------------------------------------------------------------------------------------------
def test_train_vqgan_check_args_accepts_the_perceptual_term_only_with_weights(tmp_path, sd):
    from mebt_amd import train_vqgan as T
    (tmp_path / "frames").mkdir()
    base = ["--data_path", str(tmp_path / "frames"), "--image_folder", "--max_steps", "4"]
    ck = str(tmp_path / "lpips.pt")
    torch.save(sd, ck)
    parse = lambda extra: T.build_parser().parse_args(base + extra)
    T.check_args(parse([]))
    T.check_args(parse(["--perceptual_weight", "1.0", "--lpips_ckpt", ck]))
    T.check_args(parse(["--perceptual_weight", "1.0", "--lpips_ckpt", ck]), lpips_available=True)
    T.check_args(parse(["--perceptual_weight", "1.0", "--vqgan_ckpt", "resumed.ckpt"]))            # judged once the checkpoint is read
    with pytest.raises(SystemExit, match="perceptual weights"):
        T.check_args(parse(["--perceptual_weight", "1.0"]))
    with pytest.raises(SystemExit, match="perceptual weights"):
        T.check_args(parse(["--perceptual_weight", "1.0", "--vqgan_ckpt", "resumed.ckpt"]), lpips_available=False)
    with pytest.raises(SystemExit, match="no such file"):
        T.check_args(parse(["--perceptual_weight", "1.0", "--lpips_ckpt", str(tmp_path / "missing.pt")]))
    with pytest.raises(SystemExit, match="GAN phase"):
        T.check_args(parse(["--perceptual_weight", "1.0", "--lpips_ckpt", ck, "--max_steps", "11", "--discriminator_iter_start", "10"]))
    T.check_args(parse(["--lpips_ckpt", str(tmp_path / "missing.pt")]))                            # unused at weight 0


def test_checkpoints_carry_the_perceptual_weights_and_a_resume_finds_them(tmp_path, sd):
    from mebt_amd.train_vqgan import checkpoint_dict
    from mebt_amd.vqgan import VQGAN
    from tests.golden import make_golden as mg
    c = mg.VQGAN_CONFIGS["vq_micro"]
    args = argparse.Namespace(n_hiddens=c["n_hiddens"], downsample=c["downsample"], image_channels=3, embedding_dim=c["embedding_dim"],
                              n_codes=c["n_codes"], sequence_length=4, sample_every_n_frames=1, resolution=16, perceptual_weight=1.0)
    m = VQGAN(args)
    bare = checkpoint_dict(m, 1)["state_dict"]
    assert not any(k.startswith(LP.PREFIX) for k in bare)
    m.lpips_weights = LP.extract(sd)
    ck = checkpoint_dict(m, 3)
    carried = {k for k in ck["state_dict"] if k.startswith(LP.PREFIX)}
    assert carried == {LP.PREFIX + k for k in sd}
    assert tuple(ck["state_dict"][LP.PREFIX + "scaling_layer.scale"].shape) == (1, 3, 1, 1)         # the reference's shapes
    assert set(bare) == set(ck["state_dict"]) - carried
    path = str(tmp_path / "last.ckpt")
    torch.save(ck, path)
    back = VQGAN.load_from_checkpoint(path)
    assert back.lpips_weights is not None
    assert all(torch.equal(back.lpips_weights[k], v) for k, v in LP.extract(sd).items())
    torch.save(ck["state_dict"], str(tmp_path / "sd.pt"))                                          # and the same file serves --lpips_ckpt
    assert LP.read_file(str(tmp_path / "sd.pt")).keys() == back.lpips_weights.keys()


def test_recon_backward_without_perceptual_weights_is_a_runtime_error():
    from mebt_amd.vqgan import VQGAN
    from tests.golden import make_golden as mg
    import inspect
    c = mg.VQGAN_CONFIGS["vq_micro"]
    m = VQGAN(argparse.Namespace(n_hiddens=c["n_hiddens"], downsample=c["downsample"], image_channels=3, embedding_dim=c["embedding_dim"],
                                 n_codes=c["n_codes"], sequence_length=4, sample_every_n_frames=1, resolution=16, perceptual_weight=0.5))
    with pytest.raises(RuntimeError, match="perceptual weights"):
        m.recon_backward(torch.zeros(1, 3, 4, 16, 16))
    assert inspect.signature(VQGAN.recon_backward).parameters["frame_idx"].default is None


def test_library_exports_the_backward_operators_and_checks_the_frame_pairs_on_the_host():
    from mebt_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = ("mebt_op_lpips_head_bwd", "mebt_op_maxpool_2x2_bwd", "mebt_op_conv2d_3x3_dgrad", "mebt_op_lpips_input_bwd")
    for name in names:
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    header = open(os.path.join(ROOT, "include", "mebt_hip.h")).read()
    assert all(f"int {n}(" in header for n in names)
    # the pairs are judged before anything is launched: no device is touched by a refused call (the device pointers are never read)
    bound = _lib.load()
    scale = (ctypes.c_float * 3)(.458, .448, .450)
    fake = ctypes.c_void_p(4096)

    def call(pairs, B=2, T=3, factor=1.0):
        host = torch.tensor(pairs, dtype=torch.int32)
        return bound.mebt_op_lpips_input_bwd(_lib.F32, fake, fake, ctypes.c_void_p(host.data_ptr()), fake, B, T, 16, 16, len(pairs), scale, factor, None)
    assert call([(1, 2), (1, 2)]) == 1 and b"distinct" in bound.mebt_last_error()
    assert call([(0, 0), (1, 2), (0, 0)]) == 1
    assert call([(2, 0)]) == 1 and b"outside" in bound.mebt_last_error()
    assert call([(0, 3)]) == 1 and call([(0, -1)]) == 1
    assert call([(0, 0)], factor=3.0) == 1 and b"power of two" in bound.mebt_last_error()
    assert call([(0, 0)], factor=0.0) == 1 and call([(0, 0)], factor=-2.0) == 1
    assert bound.mebt_op_lpips_input_bwd(_lib.F32, None, fake, fake, fake, 2, 3, 16, 16, 1, scale, 1.0, None) == 1
    assert bound.mebt_op_lpips_input_bwd(_lib.BF16, fake, fake, fake, fake, 2, 3, 16, 16, 1, scale, 1.0, None) == 5
