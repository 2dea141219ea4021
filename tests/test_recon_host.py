"""First-stage validation figures on the CPU (mebt_amd/recon.py): the float64 twins of the metric operators against the values the real
reference logs (tests/golden/recon/recon_golden.npz, made by make_golden_recon.py), closed forms of SSIM / PSNR / perplexity, and the
command line's parser.  No GPU: the kernels themselves are held to the same twins in tests/test_gpu_recon.py."""
import math
import os

import numpy as np
import pytest
import torch

from mebt_amd import recon
from oracle import vqgan_oracle as vq
from tests.golden import make_golden as mg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recon", "recon_golden.npz")


@pytest.mark.parametrize("name", ["vq_micro", "vq_c5"])
def test_twins_on_the_oracle_reproduce_the_reference_validation_figures(name):
    """recon_loss, commitment_loss, perplexity of the reference's own modules to fp32 rounding (rel 1e-4); the oracle reproduces every
    golden id (tests/test_oracle_golden.py), so no tie allowance"""
    g = np.load(GOLDEN)
    cfg = mg.vqgan_cfg(name)
    P = vq.closed_form_params(cfg)
    x = mg.vqgan_video(name)
    with torch.no_grad():
        ids, z, _ = vq.encode(P, cfg, x, return_all=True)
        rec = vq.decode(P, cfg, ids)
    assert np.array_equal(ids.numpy(), g[f"{name}_ids"])
    zf = z.permute(0, 2, 3, 4, 1).reshape(-1, cfg.embedding_dim)
    hist, sq = recon.code_stats_twin(ids, zf, P["codebook.embeddings"])
    got = {"recon_loss": float(recon.abs_diff_sum_twin(x, rec).sum()) / x.numel() * float(g[f"{name}_l1_weight"]),
           "commitment_loss": 0.25 * float(sq) / zf.numel(), "perplexity": float(recon.perplexity_of(hist))}
    for k, v in got.items():
        ref = float(g[f"{name}_{k}"])
        print(f"[{name}] {k}: twin {v!r} reference {ref!r}")
        assert abs(v - ref) <= 1e-4 * abs(ref), (k, v, ref)


def _frames(seed, n=2, h=19, w=23):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8))


def test_ssim_twin_of_a_frame_with_itself_is_exactly_one():
    a = _frames(1)
    sq, s = recon.clip_quality_u8_twin(a, a.clone())
    assert sq.dtype == torch.int64 and (sq == 0).all()
    assert (s == 1.0).all()


@pytest.mark.parametrize("p,q", [(0, 0), (0, 255), (17, 200), (250, 253), (128, 127)])
def test_ssim_twin_of_two_constant_frames(p, q):
    a = torch.full((1, 11, 14, 3), p, dtype=torch.uint8)
    b = torch.full((1, 11, 14, 3), q, dtype=torch.uint8)
    _, s = recon.clip_quality_u8_twin(a, b)
    want = (2.0 * p * q + recon.C1) / (p * p + q * q + recon.C1)
    assert abs(float(s) - want) <= 1e-12, (float(s), want)


def test_ssim_window_and_twin_shapes():
    g = recon.ssim_window()
    assert g.dtype == np.float64 and len(g) == 11 and abs(g.sum() - 1.0) < 1e-15 and np.allclose(g, g[::-1], rtol=0, atol=0)
    assert abs(g[4] / g[5] - math.exp(-1 / 4.5)) < 1e-15
    a, b = _frames(2, n=6).view(2, 3, 19, 23, 3), _frames(3, n=6).view(2, 3, 19, 23, 3)
    sq, s = recon.clip_quality_u8_twin(a, b)
    assert tuple(sq.shape) == tuple(s.shape) == (2, 3) and s.dtype == torch.float64
    assert tuple(recon.ssim_map_twin(a[0], b[0]).shape) == (3, 3, 9, 13)
    with pytest.raises(ValueError, match="window"):
        recon.clip_quality_u8_twin(a[..., :10, :, :], b[..., :10, :, :])


def test_psnr_of_frames_one_level_apart():
    a = _frames(4).clamp(max=254)
    sq, _ = recon.clip_quality_u8_twin(a, a + 1)
    pixels = 19 * 23 * 3
    assert (sq == pixels).all()
    psnr = recon.psnr_of(sq, pixels)
    assert (psnr - 10 * math.log10(255.0 ** 2)).abs().max().item() <= 1e-12
    assert (recon.psnr_of(torch.zeros(3, dtype=torch.int64), pixels) == 0).all()        # identical frames: counted apart, no inf


@pytest.mark.parametrize("n_codes", [512, 2048])
def test_perplexity_of_a_uniform_histogram_is_the_code_count(n_codes):
    """the reference's 1e-10 inside the logarithm (codebook.py:94) lowers the figure by a factor exp(-n_codes * 1e-10): 2e-7 at the
    reference's default of 2048 codes, inside the 1e-6 asked for here (at 16384 codes the definition itself is 1.6e-6 below n_codes)"""
    p = float(recon.perplexity_of(torch.full((n_codes,), 3, dtype=torch.int64)))
    assert abs(p - n_codes) <= 1e-6 * n_codes
    one = torch.zeros(n_codes, dtype=torch.int64)
    one[7] = 5
    assert abs(float(recon.perplexity_of(one)) - 1.0) <= 1e-9


def test_code_stats_twin_skips_ids_out_of_range_and_accumulates():
    g = torch.Generator().manual_seed(0)
    e, z = torch.randn(8, 4, generator=g), torch.randn(6, 4, generator=g)
    ids = torch.tensor([3, -1, 7, 8, 3, 0])
    hist, sq = recon.code_stats_twin(ids, z, e)
    assert hist.tolist() == [1, 0, 0, 2, 0, 0, 0, 1]
    keep = [0, 2, 4, 5]
    want = sum(float(((z[m].double() - e[ids[m]].double()) ** 2).sum()) for m in keep)
    assert abs(float(sq) - want) <= 1e-12 * want
    hist2, _ = recon.code_stats_twin(ids, z, e, hist=hist)
    assert hist2.tolist() == [2, 0, 0, 4, 0, 0, 0, 2]


def test_measure_recon_parser_takes_the_data_flags_of_measure_fvd():
    from mebt_amd import measure_fvd, measure_recon
    argv = ["--data_path", "/d", "--image_folder", "--train", "--sequence_length", "4", "--resolution", "16", "--batch_size", "8",
            "--num_workers", "0", "--sample_every_n_frames", "2", "--packed_path", "/p", "--n_sample", "4"]
    a = measure_recon.build_parser().parse_args(argv + ["--vqgan_ckpt", "v.ckpt", "--vqgan_dtype", "f32", "--out", "o.csv", "--save_np", "r.npy",
                                                        "--compute_fvd", "--i3d_ckpt", "w.pt", "--i3d_dtype", "f32", "--i3d_batch", "8"])
    b = measure_fvd.build_parser().parse_args(argv)
    data_flags = ["data_path", "image_folder", "train", "sequence_length", "resolution", "batch_size", "num_workers", "sample_every_n_frames",
                  "packed_path", "n_sample", "vtokens", "image_channels"]
    assert all(getattr(a, k) == getattr(b, k) for k in data_flags)
    assert (a.vqgan_ckpt, a.vqgan_dtype, a.out, a.save_np, a.compute_fvd, a.i3d_ckpt, a.i3d_dtype, a.i3d_batch) == \
        ("v.ckpt", "f32", "o.csv", "r.npy", True, "w.pt", "f32", 8)
    d = measure_recon.build_parser().parse_args([])
    assert (d.n_sample, d.vqgan_dtype, d.compute_fvd, d.save_np, d.train) == (2048, "f16", False, "", False)


def test_accumulator_result_fields_are_the_documented_columns():
    assert recon.FIELDS == ["recon_loss", "commitment_loss", "perplexity", "perplexity_set", "codes_used", "PSNR", "SSIM", "identical_frames",
                            "n_clips"]


def test_golden_recon_fixture_regenerates_identically(tmp_path):
    """where the reference tree is at hand, make_golden_recon.py writes the committed file again, value for value"""
    import subprocess
    import sys
    from tests.golden.make_golden import REF
    if not os.path.isdir(REF):
        pytest.skip("reference tree not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(GOLDEN), "make_golden_recon.py")], cwd=root,
                         env=dict(os.environ, MEBT_GOLDEN_OUT=str(tmp_path)), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    a, b = np.load(os.path.join(tmp_path, "recon_golden.npz")), np.load(GOLDEN)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
