"""LPIPS, host side (no GPU): the float32 twin against the real reference's golden figures (tests/golden/lpips/lpips_golden.npz), the
fixture's regeneration, the key schema (prefix, partial sets, `lin`-only files, `VQGAN.load_state_dict`), the host weight arrangement,
the frame lists, `ReconAccumulator` with an `lpips` entry and the `measure_recon` flags."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lpips")
REF = os.environ.get("MEBT_REFERENCE", "/root/reference")
sys.path.insert(0, GOLD)

from make_golden_lpips import CASES, closed_form_state_dict, to_input  # noqa: E402
from mebt_amd import lpips as LP  # noqa: E402
from mebt_amd import measure_recon as MR  # noqa: E402
from mebt_amd import recon  # noqa: E402

TWIN_REL = 1e-5              # the float32 twin against the reference itself (measured <= 3e-7)


def golden():
    return np.load(os.path.join(GOLD, "lpips_golden.npz"))


@pytest.fixture(scope="module")
def sd():
    return closed_form_state_dict()


def test_golden_schema_is_the_reference_state_dict(sd):
    g = golden()
    shapes = {str(k): tuple(int(x) for x in s if x >= 0) for k, s in zip(g["sd_keys"], g["sd_shapes"])}
    assert len(shapes) == 33
    want = dict(LP.expected_shapes())
    want["scaling_layer.shift"] = want["scaling_layer.scale"] = (1, 3, 1, 1)
    assert shapes == want
    assert {k: tuple(v.shape) for k, v in sd.items()} == shapes
    assert [k for k, _, _ in LP.conv_keys()] == [f"net.slice{s}.{i}" for s, idx in ((1, (0, 2)), (2, (5, 7)), (3, (10, 12, 14)),
                                                                                 (4, (17, 19, 21)), (5, (24, 26, 28))) for i in idx]
    assert all(float(sd[f"lin{k}.model.1.weight"].min()) >= 0 for k in range(5))


@pytest.mark.parametrize("tag", list(CASES))
def test_float32_twin_equals_the_reference(sd, tag):
    g = golden()
    torch.set_num_threads(4)
    val, lay = LP.lpips_twin(sd, to_input(g[f"a_{tag}"]), to_input(g[f"b_{tag}"]), dtype=torch.float32)
    ev = (np.abs(val.numpy() - g[f"val_{tag}"]) / g[f"val_{tag}"]).max()
    el = (np.abs(lay.numpy() - g[f"layers_{tag}"]) / g[f"layers_{tag}"]).max()
    print(f"[twin f32 {tag}] value rel {ev:.2e}, per-layer rel {el:.2e}")
    assert ev <= TWIN_REL and el <= TWIN_REL, (ev, el)
    assert val.shape == (CASES[tag][0],) and lay.shape == (CASES[tag][0], 5)
    # the slice outputs behind them: per-channel means of pair 0
    for side, key in ((0, "a"), (1, "b")):
        feats = LP.twin_features(sd, to_input(g[f"{key}_{tag}"][:1]), dtype=torch.float32)
        means = np.concatenate([f[0].mean(dim=(1, 2)).numpy() for f in feats])
        want = g[f"means_{tag}"][side]
        assert means.shape == want.shape == (1472,)
        assert np.abs(means - want).max() <= TWIN_REL * np.abs(want).max()


def test_float64_twin_is_close_to_the_float32_reference(sd):
    g = golden()
    val, _ = LP.lpips_twin(sd, to_input(g["a_odd"]), to_input(g["b_odd"]))
    assert val.dtype == torch.float64
    assert (np.abs(val.numpy() - g["val_odd"]) / g["val_odd"]).max() <= TWIN_REL


def test_golden_lpips_fixture_regenerates_bit_identically(tmp_path):
    if not os.path.isdir(REF):
        pytest.skip("reference tree not available")
    env = dict(os.environ, MEBT_GOLDEN_OUT=str(tmp_path))
    out = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_lpips.py")], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    a, b = np.load(os.path.join(tmp_path, "lpips_golden.npz")), golden()
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    assert os.path.getsize(os.path.join(GOLD, "lpips_golden.npz")) < 200 * 1024


# ---- key schema -------------------------------------------------------------------------------------------------------------------------
def test_extract_strips_the_prefix_and_fills_the_scaling_constants(sd):
    pref = {LP.PREFIX + k: v for k, v in sd.items()}
    pref["encoder.conv_first.conv.weight"] = torch.zeros(2)
    pref["lin_unrelated"] = torch.zeros(1)
    a, b = LP.extract(sd), LP.extract(pref)
    assert set(a) == set(b) == set(LP.expected_shapes()) | {"scaling_layer.shift", "scaling_layer.scale"}
    assert all(torch.equal(a[k], b[k]) and a[k].dtype == torch.float32 and a[k].device.type == "cpu" for k in a)
    assert a["scaling_layer.shift"].shape == (3,)
    bare = {k: v for k, v in sd.items() if not k.startswith("scaling_layer.")}
    c = LP.extract(bare)
    assert c["scaling_layer.shift"].tolist() == pytest.approx([-.030, -.088, -.188]) and c["scaling_layer.scale"].tolist() == pytest.approx(
        [.458, .448, .450])
    assert LP.extract({"encoder.w": torch.zeros(1)}) is None


def test_partial_sets_raise_and_name_what_is_missing(sd):
    part = {k: v for k, v in sd.items() if k not in ("net.slice3.12.bias", "lin4.model.1.weight")}
    with pytest.raises(ValueError, match=r"missing 2 of 31.*net\.slice3\.12\.bias.*lin4\.model\.1\.weight"):
        LP.extract(part)
    wrong = dict(sd)
    wrong["net.slice1.0.weight"] = torch.zeros(64, 3, 1, 1)
    with pytest.raises(ValueError, match="wrong shape"):
        LP.extract(wrong)


def test_a_lin_only_file_is_refused(sd, tmp_path):
    path = str(tmp_path / "vgg.pth")
    torch.save({k: v for k, v in sd.items() if k.startswith("lin")}, path)
    with pytest.raises(ValueError, match="VGG-16 convolutions"):
        LP.read_file(path)
    with pytest.raises(ValueError, match="VGG-16 convolutions"):
        LP.LPIPS.load(path)
    full = str(tmp_path / "full.pt")
    torch.save({"state_dict": {LP.PREFIX + k: v for k, v in sd.items()}}, full)
    own = LP.read_file(full)
    assert torch.equal(own["net.slice5.28.weight"], sd["net.slice5.28.weight"])
    src = open(os.path.join(ROOT, "mebt_amd", "lpips.py")).read()
    assert "http" not in src and "download(" not in src


def test_vqgan_load_state_dict_keeps_the_perceptual_tensors(sd):
    from tests.helpers import tiny_vqgan
    vqm, _ = tiny_vqgan(n_codes=512)
    keys = list(vqm.state_dict())
    assert vqm.lpips_weights is None and vqm.lpips is None
    full = dict(vqm.state_dict())
    full.update({LP.PREFIX + k: v for k, v in sd.items()})
    full["image_discriminator.main.0.weight"] = torch.zeros(3)
    res = vqm.load_state_dict(full, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert list(vqm.state_dict()) == keys and not any("lpips" in n or "perceptual" in n for n, _ in vqm.named_buffers())
    own = vqm.lpips_weights
    assert own is not None and torch.equal(own["net.slice1.0.weight"], sd["net.slice1.0.weight"]) and own["lin2.model.1.weight"].device.type == "cpu"
    # a later load without them leaves the set in place; a partial set raises
    vqm.load_state_dict(vqm.state_dict(), strict=True)
    assert vqm.lpips_weights is own
    del full[LP.PREFIX + "net.slice2.5.weight"]
    with pytest.raises(ValueError, match=r"net\.slice2\.5\.weight"):
        vqm.load_state_dict(full, strict=True)


# ---- host weight arrangement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout,cin", [(64, 3), (128, 64), (40, 32)])
def test_arranged_weight_follows_the_index_formula(cout, cin):
    w = torch.arange(cout * cin * 9, dtype=torch.float32).reshape(cout, cin, 3, 3) * 0.25 - 7.0
    a = LP.arrange_weight(w, torch.float32)
    K = 9 * cin
    assert tuple(a.shape) == (-(-cout // 64) * 64, -(-K // 32) * 32) and a.is_contiguous()
    n, dh, dw, ci = np.meshgrid(np.arange(cout), np.arange(3), np.arange(3), np.arange(cin), indexing="ij")
    got = a.numpy()[n, (dh * 3 + dw) * cin + ci]
    assert np.array_equal(got, w.numpy()[n, ci, dh, dw])
    pad = a.clone()
    pad[:cout, :K] = 0
    assert float(pad.abs().max()) == 0.0
    assert LP.arrange_weight(w, torch.float16).dtype == torch.float16


def test_plan_flops_is_ten_gflop_per_128_image():
    total, per = LP.plan_flops(128, 128)
    assert len(per) == 13 and abs(total / 1e9 - 10.0) < 0.06
    assert per[0][1:5] == (128, 128, 3, 64) and per[-1][1:5] == (8, 8, 512, 512)


def test_frame_lists():
    net = LP.LPIPS.__new__(LP.LPIPS)
    assert net._pairs(None, 2, 3).tolist() == [[0, 0], [0, 1], [0, 2], [1, 0], [1, 1], [1, 2]]
    assert net._pairs(torch.tensor([2, 0]), 2, 3).tolist() == [[0, 2], [1, 0]]
    assert net._pairs([(1, 1), (0, 2), (1, 1)], 2, 3).tolist() == [[1, 1], [0, 2], [1, 1]]
    assert net._pairs(None, 2, 3).dtype == torch.int32
    for bad in (torch.tensor([0, 3]), [(2, 0)], [(0, -1)], torch.tensor([0, 1, 2]), torch.tensor([0.0, 1.0])):
        with pytest.raises(ValueError):
            net._pairs(bad, 2, 3)


# ---- ReconAccumulator / measure_recon ---------------------------------------------------------------------------------------------------------
def fake_stats(B, T, seed, with_lpips):
    g = torch.Generator().manual_seed(seed)
    st = {"abs_sum": torch.rand(B, generator=g, dtype=torch.float64), "commit_sq_sum": torch.rand(1, generator=g, dtype=torch.float64),
          "hist": torch.randint(0, 5, (32,), generator=g), "sq_err": torch.randint(1, 1000, (B, T), generator=g),
          "ssim": torch.rand(B, T, generator=g, dtype=torch.float64), "frame_bytes": 768, "z_values": 64 * B,
          "recon": torch.zeros(B, 3, T, 16, 16)}
    if with_lpips:
        st["lpips"] = torch.rand(B, -(-T // 2), generator=g, dtype=torch.float64)
    return st


def test_accumulator_carries_lpips_after_the_fields():
    acc = recon.ReconAccumulator(32, device="cpu")
    stats = [fake_stats(2, 4, 1, True), fake_stats(3, 4, 2, True)]
    for st in stats:
        acc.add(st)
    res = acc.result()
    assert list(res) == recon.FIELDS + ["LPIPS"]
    allv = torch.cat([s["lpips"].reshape(-1) for s in stats])
    assert allv.numel() == 10 and abs(res["LPIPS"] - float(allv.mean())) <= 1e-15
    plain = recon.ReconAccumulator(32, device="cpu")
    for st in stats:
        plain.add({k: v for k, v in st.items() if k != "lpips"})
    res0 = plain.result()
    assert list(res0) == recon.FIELDS and all(res0[k] == res[k] for k in recon.FIELDS)


def test_measure_recon_parser_flags():
    p = MR.build_parser()
    a = p.parse_args([])
    assert a.lpips is False and a.lpips_ckpt == "" and a.lpips_every == 1 and a.lpips_dtype == MR.LPIPS_DTYPE_DEFAULT
    a = p.parse_args(["--lpips", "--lpips_ckpt", "w.pt", "--lpips_dtype", "f32", "--lpips_every", "4"])
    assert a.lpips and a.lpips_ckpt == "w.pt" and a.lpips_dtype == "f32" and a.lpips_every == 4
    with pytest.raises(SystemExit):
        p.parse_args(["--lpips_dtype", "bf16"])
    assert isinstance(a, argparse.Namespace)
