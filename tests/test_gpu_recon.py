"""First-stage validation on MI355X: the three metric operators of csrc/recon/recon.hip against their float64 twins
(mebt_amd/recon.py), `VQGAN.validation_step` against the twins and the reference's golden figures, `ReconAccumulator`, and the
`python -m mebt_amd.measure_recon` command on a generated frame folder.  GPU only.

Tolerances.  abs_diff_sum / code_stats: rel 1e-5 — a lane adds at most 64 fp32 terms before fp64 takes over, 64 * 2^-24 = 4e-6.
clip_quality_u8: the squared error is exact; SSIM within 5e-4 of the float64 twin per frame — centred moments are at most 2^14, so one
fp32 rounding is about 1e-3 absolute, a few of them against denominators of at least C2 = 58.5 give at most 2e-4 (measured maxima:
profiles/recon_parity_measured.txt).  Every operator is run twice and must return the same bits."""
import argparse
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mebt_amd import _lib, recon
from mebt_amd import measure_recon as MR
from mebt_amd.frames import video_to_clip_u8
from oracle import vqgan_oracle as vq
from tests.golden import make_golden as mg
from tests.helpers import record_measured, tiny_vqgan, write_tree
from tests.test_fvd_frames_host import write_png_tree
from tests.test_gpu_fvd import closed_form_sd

DEV = "cuda"
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def record(name, value, gate):
    """measured maxima next to their gates, through the suite's own log of measured parity figures (the figures of one MI355X run are
    kept as profiles/recon_parity_measured.txt); never fails a test"""
    record_measured("recon " + name, value, gate)


# ---- abs_diff_sum -------------------------------------------------------------------------------------------------------------------
# the last case: 258 workgroups per clip, so the finishing kernel's threads 0 and 1 add a second slot (more than 256 slots, no multiple of it)
@pytest.mark.parametrize("B,n", [(1, 1), (3, 3 * 4 * 16 * 16), (2, 3 * 5 * 24 * 40 + 0), (5, 100003), (1, 257 * recon.ABS_CHUNK + 5)])
def test_abs_diff_sum_vs_twin(B, n):
    g = torch.Generator().manual_seed(n)
    x, y = torch.rand(B, n, generator=g) - 0.5, torch.rand(B, n, generator=g) - 0.5
    xd, yd = x.to(DEV), y.to(DEV)
    out = recon.abs_diff_sum(xd, yd)
    assert out.dtype == torch.float64 and tuple(out.shape) == (B,)
    ref = recon.abs_diff_sum_twin(x, y)
    err = ((out.cpu() - ref).abs() / ref).max().item()
    print(f"[abs_diff_sum {B}x{n}] max rel err {err:.2e}")
    record(f"abs_diff_sum[{B}x{n}] rel", err, 1e-5)
    assert err <= 1e-5
    assert torch.equal(recon.abs_diff_sum(xd, yd), out)                         # bit-identical run to run
    if B > 1:                                                                   # clips do not leak into each other
        assert torch.equal(recon.abs_diff_sum(xd[1:].contiguous(), yd[1:].contiguous()), out[1:])


# ---- clip_quality_u8 ------------------------------------------------------------------------------------------------------------------
def quality_inputs(kind, N, H, W, rs):
    if kind == "noise20":
        a = rs.randint(0, 256, (N, H, W, 3)).astype(np.float64)
        b = a + rs.normal(0, 20, a.shape)
    elif kind == "ramp8":
        a = np.broadcast_to(np.linspace(0, 255, W)[None, None, :, None], (N, H, W, 3)).copy()
        b = a + rs.normal(0, 8, a.shape)
    elif kind == "bright2":
        a = rs.randint(250, 254, (N, H, W, 3)).astype(np.float64)
        b = a + rs.normal(0, 2, a.shape)
    elif kind == "flat8":                        # beyond the four asked for: low SSIM (noise against a nearly flat frame)
        a = np.full((N, H, W, 3), 100.0) + rs.normal(0, 1, (N, H, W, 3))
        b = a + rs.normal(0, 8, a.shape)
    elif kind == "independent":                  # ... and SSIM near 0
        a = rs.randint(0, 256, (N, H, W, 3)).astype(np.float64)
        b = rs.randint(0, 256, (N, H, W, 3)).astype(np.float64)
    else:
        a = rs.randint(0, 256, (N, H, W, 3)).astype(np.float64)
        b = a.copy()
    to_u8 = lambda t: torch.from_numpy(np.clip(np.rint(t), 0, 255).astype(np.uint8))
    return to_u8(a), to_u8(b)


@pytest.mark.parametrize("N,H,W", [(1, 11, 11), (3, 11, 37), (4, 24, 40), (2, 16, 16), (6, 33, 47)])
def test_clip_quality_u8_vs_twin(N, H, W):
    rs = np.random.RandomState(H * 100 + W)
    for kind in ("noise20", "ramp8", "bright2", "identical", "flat8", "independent"):
        a, b = quality_inputs(kind, N, H, W, rs)
        ad, bd = a.to(DEV), b.to(DEV)
        sq, ssim = recon.clip_quality_u8(ad, bd)
        assert sq.dtype == torch.int64 and ssim.dtype == torch.float64 and tuple(sq.shape) == tuple(ssim.shape) == (N,)
        sq_ref, ssim_ref = recon.clip_quality_u8_twin(a, b)
        err = (ssim.cpu() - ssim_ref).abs().max().item()
        print(f"[clip_quality {N}x{H}x{W} {kind}] SSIM {ssim_ref.min().item():.3f}..{ssim_ref.max().item():.3f}, max |kernel - twin| {err:.2e}")
        record(f"clip_quality_u8[{N}x{H}x{W} {kind}] ssim abs", err, 5e-4)
        assert torch.equal(sq.cpu(), sq_ref), kind
        assert err <= 5e-4, (kind, err)
        if kind == "identical":
            assert (sq == 0).all() and (ssim.cpu() - 1.0).abs().max().item() <= 5e-4
        sq2, ssim2 = recon.clip_quality_u8(ad, bd)
        assert torch.equal(sq2, sq) and torch.equal(ssim2, ssim), kind           # bit-identical run to run


def test_clip_quality_u8_takes_clips():
    rs = np.random.RandomState(3)
    a, b = quality_inputs("noise20", 6, 16, 16, rs)
    sq, ssim = recon.clip_quality_u8(a.view(2, 3, 16, 16, 3).to(DEV), b.view(2, 3, 16, 16, 3).to(DEV))
    sq1, ssim1 = recon.clip_quality_u8(a.to(DEV), b.to(DEV))
    assert tuple(sq.shape) == tuple(ssim.shape) == (2, 3)
    assert torch.equal(sq.view(-1), sq1) and torch.equal(ssim.view(-1), ssim1)


# ---- code_stats -----------------------------------------------------------------------------------------------------------------------
# the last case: 258 workgroups, more slots than the finishing kernel has threads and no multiple of them
@pytest.mark.parametrize("M,n_codes,d,skewed", [(64, 512, 64, False), (1000, 16384, 256, True), (257 * recon.CODE_ROWS + 1, 1, 1, False)])
def test_code_stats_vs_twin(M, n_codes, d, skewed):
    g = torch.Generator().manual_seed(M)
    z, e = torch.randn(M, d, generator=g), torch.randn(n_codes, d, generator=g)
    if skewed:          # most rows on a handful of codes: many adders on few bins
        ids = torch.where(torch.rand(M, generator=g) < 0.9, torch.randint(0, 4, (M,), generator=g), torch.randint(0, n_codes, (M,), generator=g))
    else:
        ids = torch.randint(0, n_codes, (M,), generator=g)
    zd, ed, idd = z.to(DEV), e.to(DEV), ids.to(DEV)
    hist, sq = recon.code_stats(idd, zd, ed)
    hist_ref, sq_ref = recon.code_stats_twin(ids, z, e)
    assert hist.dtype == torch.int64 and torch.equal(hist.cpu(), torch.bincount(ids, minlength=n_codes)) and torch.equal(hist.cpu(), hist_ref)
    err = abs(float(sq) - float(sq_ref)) / float(sq_ref)
    print(f"[code_stats {M}x{n_codes}x{d}] sq_sum rel err {err:.2e}")
    record(f"code_stats[{M}x{n_codes}x{d}] sq_sum rel", err, 1e-5)
    assert err <= 1e-5
    # a second call adds to the first call's histogram; the sum is this call's, bit for bit
    hist2, sq2 = recon.code_stats(idd, zd, ed, hist=hist)
    assert hist2 is hist and torch.equal(hist.cpu(), 2 * hist_ref) and torch.equal(sq2, sq)
    # two ids out of range change nothing: legitimate input to the skip rule
    ids_bad = torch.cat([ids, torch.tensor([-1, n_codes])])
    z_bad = torch.cat([z, torch.randn(2, d, generator=g)])
    hist3, sq3 = recon.code_stats(ids_bad.to(DEV), z_bad.to(DEV), ed)
    assert torch.equal(hist3.cpu(), hist_ref) and abs(float(sq3) - float(sq_ref)) <= 1e-5 * float(sq_ref)
    if M % recon.CODE_ROWS == 0:                 # the two extra rows sit in a workgroup of their own: the very same partials
        assert torch.equal(sq3, sq)


# ---- argument checks: a status and a message, nothing launched ---------------------------------------------------------------------------
def test_argument_checks():
    lib = _lib.load()
    a = torch.zeros(2, 10, 16, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.MebtError, match="window"):
        recon.clip_quality_u8(a, a)                                              # H = 10
    sentinel = -7.0
    x = torch.ones(2, 40000, device=DEV)
    out = torch.full((2,), sentinel, device=DEV, dtype=torch.float64)
    scratch = torch.full((64,), sentinel, device=DEV, dtype=torch.float64)
    need = 8 * 2 * 3                                                             # 3 chunks of 16384 per clip
    calls = {
        "null pointer": lambda: lib.mebt_op_abs_diff_sum(_lib.ptr(x), None, _lib.ptr(out), 2, 40000, _lib.ptr(scratch), need, _lib.cur_stream()),
        "scratch too small": lambda: lib.mebt_op_abs_diff_sum(_lib.ptr(x), _lib.ptr(x), _lib.ptr(out), 2, 40000, _lib.ptr(scratch), need - 8,
                                                              _lib.cur_stream()),
        "null pointer ": lambda: lib.mebt_op_abs_diff_sum(_lib.ptr(x), _lib.ptr(x), _lib.ptr(out), 2, 40000, None, need, _lib.cur_stream()),
    }
    f = torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device=DEV)
    sq, ss = torch.full((1,), -7, device=DEV, dtype=torch.int64), torch.full((1,), sentinel, device=DEV, dtype=torch.float64)
    calls["window"] = lambda: lib.mebt_op_clip_quality_u8(_lib.ptr(f), _lib.ptr(f), _lib.ptr(sq), _lib.ptr(ss), 1, 10, 16, _lib.ptr(scratch), 512,
                                                          _lib.cur_stream())
    calls["scratch too small "] = lambda: lib.mebt_op_clip_quality_u8(_lib.ptr(f), _lib.ptr(f), _lib.ptr(sq), _lib.ptr(ss), 1, 16, 16,
                                                                      _lib.ptr(scratch), 8, _lib.cur_stream())
    ids = torch.zeros(20, dtype=torch.int64, device=DEV)
    z = torch.zeros(20, 8, device=DEV)
    hist = torch.zeros(4, dtype=torch.int64, device=DEV)
    calls["scratch too small  "] = lambda: lib.mebt_op_code_stats(_lib.ptr(ids), _lib.ptr(z), _lib.ptr(z), _lib.ptr(hist), _lib.ptr(out), 20, 4, 8,
                                                                  _lib.ptr(scratch), 8, _lib.cur_stream())
    calls["null pointer  "] = lambda: lib.mebt_op_code_stats(_lib.ptr(ids), _lib.ptr(z), _lib.ptr(z), None, _lib.ptr(out), 20, 4, 8,
                                                             _lib.ptr(scratch), 16, _lib.cur_stream())
    for what, call in calls.items():
        status = call()
        assert status != 0, what
        assert what.strip() in lib.mebt_last_error().decode(), (what, lib.mebt_last_error())
    torch.cuda.synchronize()
    assert (out == sentinel).all() and (scratch == sentinel).all() and (sq == -7).all() and (ss == sentinel).all() and (hist == 0).all()


# ---- VQGAN.validation_step ------------------------------------------------------------------------------------------------------------
def build(name, dtype):
    from mebt_amd.vqgan import VQGAN
    c = mg.VQGAN_CONFIGS[name]
    args = argparse.Namespace(n_hiddens=c["n_hiddens"], downsample=c["downsample"], image_channels=3, embedding_dim=c["embedding_dim"],
                              n_codes=c["n_codes"], sequence_length=c["video"][2], sample_every_n_frames=1, resolution=c["video"][3])
    m = VQGAN(args)
    m.load_state_dict(vq.closed_form_params(mg.vqgan_cfg(name)), strict=False)
    m.compute_dtype = dtype
    return m.to(DEV).eval()


def twin_figures(st, x, model, l1_weight=4.0):
    """the three figures from the float64 twins on the GPU run's own z, ids and decode"""
    emb = model._prepared["emb"].cpu()
    z = model._last_z.reshape(-1, emb.shape[1]).cpu()
    hist, sq = recon.code_stats_twin(st["ids"].cpu(), z, emb)
    return {"val/recon_loss": float(recon.abs_diff_sum_twin(x, st["recon"].cpu()).sum()) / x.numel() * l1_weight,
            "val/commitment_loss": 0.25 * float(sq) / z.numel(), "val/perplexity": float(recon.perplexity_of(hist))}


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_validation_step_on_vq_micro(dtype):
    name = "vq_micro"
    model = build(name, dtype)
    x = mg.vqgan_video(name)
    kept, inner = {}, model.reconstruct_stats
    model.reconstruct_stats = lambda *a, **k: kept.setdefault("st", inner(*a, **k))       # keep the step's own tensors
    out = model.validation_step({"video": x.to(DEV)}, 0)
    assert set(out) == {"val/recon_loss", "val/commitment_loss", "val/perplexity", "val/perceptual_loss"}
    assert model.logged.keys() == out.keys() and all(model.logged[k] is out[k] for k in out)
    assert float(out["val/perceptual_loss"]) == 0.0
    # the twins on this step's own z, ids and decode: only the operators' rounding differs
    st = kept["st"]
    ref = twin_figures(st, x, model)
    got = {"val/recon_loss": float(st["abs_sum"].sum()) / x.numel() * 4.0, "val/commitment_loss": 0.25 * float(st["commit_sq_sum"]) / st["z_values"],
           "val/perplexity": float(recon.perplexity_of(st["hist"]))}
    for k in ref:
        err = abs(got[k] - ref[k]) / abs(ref[k])
        print(f"[validation_step {dtype}] {k}: kernels {got[k]!r} twin {ref[k]!r} logged {float(out[k])!r}")
        record(f"validation_step[{dtype}] {k} rel vs twin", err, 1e-5)
        assert err <= 1e-5, (k, got[k], ref[k])
        assert abs(float(out[k]) - ref[k]) <= 1e-5 * abs(ref[k]), (k, float(out[k]), ref[k])
    if dtype != "f32":
        return
    # the real reference's figures, provided the ids are its ids; they may differ only at the golden file's own near ties
    g = np.load(os.path.join(G, "recon", "recon_golden.npz"))
    gv = np.load(os.path.join(G, name + ".npz"))
    mism = st["ids"].cpu().numpy() != g[f"{name}_ids"]
    gap = (gv["best2"][:, 1] - gv["best2"][:, 0]).reshape(mism.shape)
    assert (gap[mism] < 1e-3).all() and mism.sum() <= 2, (int(mism.sum()), gap[mism])
    for k in ("recon_loss", "commitment_loss", "perplexity"):
        want = float(g[f"{name}_{k}"])
        if k == "perplexity" and mism.any():
            print(f"[validation_step] {int(mism.sum())} ids differ at reference near ties: the golden perplexity is not compared")
            continue
        err = abs(got["val/" + k] - want) / abs(want)
        record(f"validation_step[f32] {k} rel vs reference", err, 1e-4)
        assert err <= 1e-4, (k, got["val/" + k], want)


def test_validation_step_without_the_default_perceptual_weight(capsys):
    vqm, args = tiny_vqgan(n_codes=512)
    args.perceptual_weight, args.l1_weight = 0.1, 2.0
    vqm = vqm.to(DEV).eval()
    vqm.compute_dtype = "f32"
    x = torch.rand(1, 3, 4, 16, 16, generator=torch.Generator().manual_seed(1)) - 0.5
    out = vqm.validation_step({"video": x}, 0)
    assert "val/perceptual_loss" not in out and "LPIPS" in capsys.readouterr().out
    st = vqm.reconstruct_stats(x.to(DEV))
    assert abs(float(out["val/recon_loss"]) - float(st["abs_sum"].sum()) / x.numel() * 2.0) <= 1e-4 * float(out["val/recon_loss"])


# ---- ReconAccumulator -------------------------------------------------------------------------------------------------------------------
def test_accumulator_over_three_batches():
    vqm, _ = tiny_vqgan(n_codes=512)
    vqm = vqm.to(DEV).eval()
    vqm.compute_dtype = "f32"
    g = torch.Generator().manual_seed(2)
    acc = recon.ReconAccumulator(512, l1_weight=4.0, device=DEV)
    stats = []
    for B in (2, 2, 1):
        x = (torch.rand(B, 3, 4, 16, 16, generator=g) - 0.5).to(DEV)
        stats.append(vqm.reconstruct_stats(x))
        acc.add(stats[-1])
    res = acc.result()
    assert list(res) == recon.FIELDS and res["n_clips"] == 5
    ids = [s["ids"].cpu().reshape(-1) for s in stats]
    per_batch = [float(recon.perplexity_of(torch.bincount(i, minlength=512))) for i in ids]
    want = (2 * per_batch[0] + 2 * per_batch[1] + per_batch[2]) / 5
    assert abs(res["perplexity"] - want) <= 1e-12 * want
    whole = torch.bincount(torch.cat(ids), minlength=512)
    assert abs(res["perplexity_set"] - float(recon.perplexity_of(whole))) <= 1e-12 * res["perplexity_set"]
    assert res["codes_used"] == float((whole > 0).sum()) / 512
    n = sum(s["recon"].numel() for s in stats)
    assert abs(res["recon_loss"] - 4.0 * sum(float(s["abs_sum"].sum()) for s in stats) / n) <= 1e-12 * res["recon_loss"]
    nz = sum(s["z_values"] for s in stats)
    assert abs(res["commitment_loss"] - 0.25 * sum(float(s["commit_sq_sum"]) for s in stats) / nz) <= 1e-12 * res["commitment_loss"]
    sq = torch.cat([s["sq_err"].reshape(-1) for s in stats]).cpu()
    ssim = torch.cat([s["ssim"].reshape(-1) for s in stats]).cpu()
    assert sq.numel() == 5 * 4 and res["identical_frames"] == int((sq == 0).sum())
    psnr = 10 * torch.log10(255.0 ** 2 / (sq[sq > 0].double() / (16 * 16 * 3)))
    assert abs(res["PSNR"] - float(psnr.mean())) <= 1e-12 * res["PSNR"] and abs(res["SSIM"] - float(ssim.mean())) <= 1e-12


# ---- the command ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("recon")
    root = str(tmp_path_factory.mktemp("recon_frames"))
    write_tree(root)
    vqm, args = tiny_vqgan(n_codes=512)
    ck = str(tmp / "vqgan.ckpt")
    torch.save({"state_dict": vqm.state_dict(), "hyper_parameters": {"args": args}}, ck)
    common = ["--vqgan_ckpt", ck, "--vqgan_dtype", "f32", "--num_workers", "0", "--image_folder", "--train", "--seed", "11"]
    small = ["--data_path", root, "--sequence_length", "4", "--resolution", "16", "--n_sample", "4", "--batch_size", "3"]
    return dict(tmp=tmp, root=root, ck=ck, common=common, small=small)


def close_rows(a, b):
    """two runs of the command on the same clips: the first stage's GroupNorm statistics are float atomic sums, so its output differs in
    the last bits from run to run (tests/test_gpu_vqgan.py) and a byte next to a truncation edge may move by one level: the integer
    columns are equal, the losses agree to 1e-5 relative, PSNR to 1e-2 dB, SSIM to 1e-4, the perplexities to one token of 512"""
    assert list(a) == list(b)
    for k in a:
        if k in ("identical_frames", "n_clips"):
            assert a[k] == b[k], k
        else:
            tol = {"PSNR": 1e-2, "SSIM": 1e-4, "perplexity": 1e-2 * abs(b[k]), "perplexity_set": 1e-2 * abs(b[k]),
                   "codes_used": 1.0 / 512}.get(k, 1e-5 * abs(b[k]))
            assert abs(a[k] - b[k]) <= tol, (k, a[k], b[k])


def test_measure_recon_on_a_folder(setup, capsys):
    from mebt_amd.vqgan import load_vqgan
    tmp = setup["tmp"]
    out, saved = str(tmp / "row.csv"), str(tmp / "rec.npy")
    row = MR.main(setup["small"] + setup["common"] + ["--out", out, "--save_np", saved])
    text = capsys.readouterr().out
    lines = open(out).read().splitlines()
    assert lines[0] == "," + ",".join(recon.FIELDS) and len(lines) == 2 and lines[1].startswith("0,")
    cells = lines[1].split(",")[1:]
    assert [float(c) for c in cells] == [float(row[k]) for k in recon.FIELDS] and lines[1].split(",", 1)[1] in text
    assert row["n_clips"] == 4 and 0 < row["SSIM"] < 1 and 0 < row["PSNR"] < 100 and row["recon_loss"] > 0

    # the same batches, straight through reconstruct_stats
    args = MR.build_parser().parse_args(setup["small"] + setup["common"])
    vqm = load_vqgan(setup["ck"], torch.device(DEV))
    vqm.compute_dtype = "f32"
    MR.seed_everything(args.seed)
    stats, clips, left = [], [], 4
    for x, u8 in MR.real_batches(args, torch.device(DEV)):
        x, u8 = x[:left].contiguous(), u8[:left].contiguous()
        assert torch.equal(video_to_clip_u8(x), u8)                              # both routes to the real side's bytes agree
        stats.append(vqm.reconstruct_stats(x, clip_u8=u8))
        clips.append(x)
        left -= len(x)
        if left == 0:
            break
    assert [len(c) for c in clips] == [3, 1]
    n = sum(s["recon"].numel() for s in stats)
    sq = torch.cat([s["sq_err"].reshape(-1) for s in stats]).cpu()
    hists = [s["hist"].cpu() for s in stats]
    want = {"recon_loss": 4.0 * sum(float(s["abs_sum"].sum()) for s in stats) / n,
            "commitment_loss": 0.25 * sum(float(s["commit_sq_sum"]) for s in stats) / sum(s["z_values"] for s in stats),
            "perplexity": (3 * float(recon.perplexity_of(hists[0])) + float(recon.perplexity_of(hists[1]))) / 4,
            "perplexity_set": float(recon.perplexity_of(hists[0] + hists[1])),
            "codes_used": float(((hists[0] + hists[1]) > 0).sum()) / 512,
            "PSNR": float((10 * torch.log10(255.0 ** 2 / (sq[sq > 0].double() / 768))).mean()),
            "SSIM": float(torch.cat([s["ssim"].reshape(-1) for s in stats]).mean()),
            "identical_frames": int((sq == 0).sum()), "n_clips": 4}
    close_rows(row, want)

    # --save_np: the bytes of decode(encode(x)) as the sampling scripts would save them
    rec = np.load(saved)
    assert rec.dtype == np.uint8 and rec.shape == (4, 4, 16, 16, 3)
    x = torch.cat(clips)
    direct = video_to_clip_u8(vqm.decode(vqm.encode(x))).cpu().numpy().astype(np.int16)
    diff = np.abs(rec.astype(np.int16) - direct)
    assert diff.max() <= 1 and (diff != 0).mean() <= 1e-3                        # another decode run: see close_rows

    # a split shorter than --n_sample ends the run there and says so
    capsys.readouterr()
    row_all = MR.main(setup["small"][:-4] + ["--n_sample", "1000", "--batch_size", "3"] + setup["common"] + ["--out", out])
    assert 4 < row_all["n_clips"] < 1000 and f"the split ended after {row_all['n_clips']} clips" in capsys.readouterr().out


def test_measure_recon_from_a_pack_gives_the_folder_row(setup):
    from mebt_amd import packed as P
    tmp = setup["tmp"]
    pack = str(tmp / "pack")
    P.build_pack(setup["root"], pack, 16, splits=["train"], resize=P.gpu_resize)
    a = MR.main(setup["small"] + setup["common"] + ["--out", str(tmp / "a.csv")])
    b = MR.main(setup["small"] + setup["common"] + ["--out", str(tmp / "b.csv"), "--packed_path", pack])
    close_rows(a, b)


def test_measure_recon_with_fvd(setup, tmp_path_factory):
    """rFVD / rKVD through the HIP I3D with closed-form weights.  The I3D's head needs clips of at least 9 frames, so this case runs the
    same checkpoint (the first stage is convolutional) on 16-frame clips of a folder of four 18-frame videos, and from an .npy of them."""
    tmp = setup["tmp"]
    root = write_png_tree(str(tmp_path_factory.mktemp("recon_png")), 4, 18, seed=4)
    ck = str(tmp / "i3d.pt")
    torch.save(closed_form_sd(), ck)
    argv = ["--data_path", root, "--sequence_length", "16", "--resolution", "16", "--n_sample", "4", "--batch_size", "4", "--compute_fvd",
            "--i3d_ckpt", ck, "--i3d_dtype", "f32"] + setup["common"]
    out = str(tmp / "fvd.csv")
    row = MR.main(argv + ["--out", out, "--save_np", str(tmp / "rec16.npy")])
    assert list(row) == recon.FIELDS + ["rFVD", "rKVD"] and row["n_clips"] == 4
    assert math.isfinite(row["rFVD"]) and math.isfinite(row["rKVD"])
    assert open(out).read().splitlines()[0] == "," + ",".join(recon.FIELDS + ["rFVD", "rKVD"])
    rec = np.load(str(tmp / "rec16.npy"))
    assert rec.dtype == np.uint8 and rec.shape == (4, 16, 16, 16, 3)
    # the .npy route of the real side, fed with reconstructions as "real" clips: same columns, finite figures
    row2 = MR.main(["--data_path", str(tmp / "rec16.npy"), "--sequence_length", "16", "--n_sample", "4", "--batch_size", "2",
                    "--vqgan_ckpt", setup["ck"], "--vqgan_dtype", "f32", "--out", out])
    assert list(row2) == recon.FIELDS and row2["n_clips"] == 4 and 0 < row2["SSIM"] <= 1
