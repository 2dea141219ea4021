"""EMA codebook of first-stage training on MI355X: the operators of csrc/codebook/codebook_train.hip against the float64 statements of
tests/codebook_common.py, `VQGAN.recon_backward(update_codebook=True)` against the run of the real reference recorded in
tests/golden/codebook_train, the f16 mode, `train_step` and the `python -m mebt_amd.train_vqgan` command.  GPU only.

Gates.  codebook_sums: n_total exact; |encode_sum - float64| <= K 2^-23 sum |z| over the code's rows, K the code's count (the summation
bound of DESIGN.md §9d; the operator adds the rows one after the other in fp32 and has no quantisation of its own), which is an exact
zero for a code without rows; two runs bitwise equal.  codebook_ema: against the reference's statements in torch fp32 on the CPU, within
8 times the largest deviation of that fp32 run from the float64 one, per tensor (the GroupNorm precedent of tests/test_gpu_vqgrad.py; the
factor covers another summation order for n = sum N); the restart mask exactly, the inputs keeping every N 1e-4 away from the threshold;
the restart rows bit for bit fl(z + fl(noise * std)).  Whole model, f32: ids, restart mask and count exactly, losses to 1e-4 (the SGD gate
of tests/test_gpu_vqgrad.py), N / z_avg / embeddings within 8 times the deviation of the reference's fp32 buffers from the float64 twin of the
whole run recorded in the fixture (`twin_dev/*`, which accumulates over the steps as the buffers do), of the buffer's maximum."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import vqgan_oracle as vq
from tests import codebook_common as cc
from tests import vqgrad_common as vc
from tests.golden import make_golden as mg

DEV = "cuda"
U32 = 2.0 ** -23
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measured(line):
    """print a measured figure and, when MEBT_PARITY_OUT names a file, append it there (profiles/codebook_train_parity_measured.txt is
    one such file); never fails a test"""
    path = os.environ.get("MEBT_PARITY_OUT")
    if path:
        try:
            with open(path, "a") as f:
                f.write(line + "\n")
        except OSError:
            pass
    print(line)


# ---- operators -------------------------------------------------------------------------------------------------------------------------
def _case(name):
    """-> (ids int64 [M], z fp32 [M, d], n_codes) on the CPU"""
    M, n_codes, d = {"sparse": (64, 512, 64), "ragged": (1000, 37, 20), "one_code": (2048, 8, 64), "c5_width": (4096, 256, 256),
                     "skipped": (1000, 37, 20), "wide": (70, 5, 516), "odd_d": (333, 11, 19)}[name]
    g = torch.Generator().manual_seed(M + d)
    z = torch.randn(M, d, generator=g) * 1.3 + 0.2
    ids = torch.randint(0, n_codes, (M,), generator=g)
    if name == "one_code":
        ids[:] = 5                                                  # the longest list: every row on one code
    if name == "ragged":
        ids[torch.rand(M, generator=g) < 0.5] = 3                   # one long list (> 64 rows) among short ones
    if name == "skipped":
        ids[::97] = -1
        ids[5::131] = n_codes
        ids[7::211] = 1 << 40
    return ids, z, n_codes


CASES = ["sparse", "ragged", "one_code", "c5_width", "skipped", "wide", "odd_d"]


@pytest.mark.parametrize("name", CASES)
def test_codebook_sums_operator(name):
    """(64, 512, 64): most codes empty; (1000, 37, 20): ragged M, lists on both sides of the 64-row threshold between the in-register sort
    and the walk over the ids, and the same sums from a z that is not 16-byte aligned; (2048, 8, 64) with every row on one code;
    (4096, 256, 256): the config-5 width; ids out of range skipped; (70, 5, 516): more than one 256-column pass of a wave;
    (333, 11, 19): d % 4 != 0, the scalar path"""
    from mebt_amd.vqgan import Codebook
    ids, z, n_codes = _case(name)
    n_ref, s_ref, abs_ref = cc.sums_twin(ids, z, n_codes)
    idd, zd = ids.to(DEV), z.to(DEV)
    n1, s1 = Codebook.code_sums(idd, zd, n_codes)
    n2, s2 = Codebook.code_sums(idd, zd, n_codes)
    assert torch.equal(n1, n2) and torch.equal(s1, s2), "two runs differ"
    assert torch.equal(n1.cpu().double(), n_ref)
    bound = n_ref[:, None] * U32 * abs_ref
    err = (s1.cpu().double() - s_ref).abs()
    assert bool((err <= bound).all()), (name, float((err / (bound + 1e-300)).max()))
    measured(f"codebook_sums[{name}] worst err / (K 2^-23 sum|z|) {float((err / (bound + 1e-300))[bound > 0].max()):.3f}; longest list {int(n_ref.max())}")
    if name == "skipped":
        assert int(n_ref.sum()) < ids.numel()
    if name == "ragged":                                            # a misaligned z takes the scalar path and gives the same sums
        pad = torch.empty(z.numel() + 1, device=DEV)
        zo = pad[1:].view_as(z).copy_(zd)
        assert zo.data_ptr() % 16 != 0
        n3, s3 = Codebook.code_sums(idd, zo, n_codes)
        assert torch.equal(n3, n1) and torch.equal(s3, s1)


def _ema_inputs(name, thres):
    ids, z, n_codes = _case(name)
    M, d = z.shape
    g = torch.Generator().manual_seed(n_codes + d)
    n_total, encode_sum, _ = cc.sums_twin(ids, z, n_codes)
    n_total, encode_sum = n_total.float(), encode_sum.float()
    N = torch.rand(n_codes, generator=g) + 0.5
    # keep every updated N 1e-4 away from the threshold in float64: the restart mask then cannot hang on fp32 rounding
    new = N.double() * 0.99 + 0.01 * n_total.double()
    N[(new - thres).abs() < 2e-4] += 0.01
    assert float(((N.double() * 0.99 + 0.01 * n_total.double()) - thres).abs().min()) >= 1e-4
    z_avg = torch.randn(n_codes, d, generator=g)
    tiled = M < n_codes
    src = torch.randperm((-(-n_codes // M) if tiled else 1) * M, generator=g)[:n_codes]
    noise = torch.randn(n_codes, d, generator=g) if tiled else None
    return z, N, z_avg, n_total, encode_sum, src, noise


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("no_restart", [False, True])
def test_codebook_ema_and_restart_rows_operators(name, no_restart):
    from mebt_amd.vqgan import Codebook
    thres = 1.0
    z, N, z_avg, n_total, encode_sum, src, noise = _ema_inputs(name, thres)
    n_codes, d = z_avg.shape
    cb = Codebook(n_codes, d, no_random_restart=no_restart, restart_thres=thres).to(DEV)
    # the restart rows: the reference's two roundings, bit for bit (with and, where M >= n_codes, without the noise term)
    k_want = cc.restart_rows_twin(z, src, noise)
    k_got = cb.restart_rows(z.to(DEV), src.to(DEV), None if noise is None else noise.to(DEV))
    assert torch.equal(k_got.cpu(), k_want), name
    ref = cc.ema_reference(N, z_avg, n_total, encode_sum, k_want, thres, no_restart)
    gate = cc.gate_of(ref)
    outs = []
    from mebt_amd import _lib
    lib = _lib.load()
    for _ in range(2):
        Nd, ad, ed = N.to(DEV), z_avg.to(DEV), torch.zeros(n_codes, d, device=DEV)
        restarted = torch.full((1,), -1, device=DEV, dtype=torch.int32)
        nbytes = int(lib.mebt_codebook_ema_scratch_bytes(n_codes))
        scratch = torch.empty(nbytes // 8 + 1, device=DEV, dtype=torch.float64)
        nt, es = n_total.to(DEV), encode_sum.to(DEV)
        _lib.check(lib.mebt_op_codebook_ema(_lib.ptr(Nd), _lib.ptr(ad), _lib.ptr(ed), _lib.ptr(nt), _lib.ptr(es),
                                            None if no_restart else _lib.ptr(k_got), _lib.ptr(restarted), n_codes, d, thres, _lib.ptr(scratch), nbytes,
                                            _lib.cur_stream()))
        outs.append((Nd.cpu(), ad.cpu(), ed.cpu(), int(restarted.item())))
    assert all(torch.equal(a, b) for a, b in zip(outs[0][:3], outs[1][:3])) and outs[0][3] == outs[1][3], "two runs differ"
    f32 = ref[torch.float32]
    usage = f32[3]
    assert torch.equal(outs[0][0] >= thres, usage), "the restart mask differs"
    assert torch.equal(usage, ref[torch.float64][3])
    assert outs[0][3] == (0 if no_restart else int((~usage).sum()))
    if not no_restart:
        assert torch.equal(outs[0][2][~usage], k_want[~usage])      # a restarted code is its restart row, to the bit
    for i, tname in enumerate(("N", "z_avg", "embeddings")):
        err = float((outs[0][i].double() - f32[i].double()).abs().max())
        measured(f"codebook_ema[{name}, no_random_restart={no_restart}] {tname}: |op - torch fp32| {err:.2e}, gate 8 x |torch fp32 - float64| {gate[i]:.2e}, "
                 f"ratio {err / gate[i]:.3f}")
        assert err <= gate[i], (name, tname, err, gate[i])


def test_codebook_operators_check_their_arguments():
    from mebt_amd import _lib
    lib = _lib.load()
    t = torch.zeros(64, device=DEV)
    ids = torch.zeros(4, device=DEV, dtype=torch.int64)
    s = _lib.cur_stream()
    assert lib.mebt_op_codebook_sums(_lib.ptr(ids), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), 0, 4, 4, _lib.ptr(t), 256, s) == 2          # M = 0
    assert lib.mebt_op_codebook_sums(_lib.ptr(ids), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), 4, 4, 4, _lib.ptr(t), 8, s) == 4            # scratch
    assert b"scratch" in lib.mebt_last_error()
    assert lib.mebt_op_codebook_sums(_lib.ptr(ids), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), 1 << 31, 4, 4, _lib.ptr(t), 1 << 40, s) == 2
    assert lib.mebt_op_codebook_ema(_lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), None, _lib.ptr(t), 4, 0, 1.0, _lib.ptr(t), 256, s) == 2
    assert lib.mebt_op_codebook_ema(_lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), None, _lib.ptr(t), 4, 4, 1.0, None, 0, s) == 1
    assert lib.mebt_op_codebook_restart_rows(_lib.ptr(t), None, None, _lib.ptr(t), 4, 4, 4, s) == 1
    torch.cuda.synchronize()


# ---- whole model -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return cc.load_fixture()


def build(fx, dtype):
    """vq_micro on the fixture's weights: the closed-form ones with pre_vq_conv times the recorded power of two"""
    from mebt_amd.vqgan import VQGAN
    c = mg.VQGAN_CONFIGS["vq_micro"]
    args = argparse.Namespace(n_hiddens=c["n_hiddens"], downsample=c["downsample"], image_channels=3, embedding_dim=c["embedding_dim"],
                              n_codes=c["n_codes"], sequence_length=c["video"][2], sample_every_n_frames=1, resolution=c["video"][3],
                              l1_weight=float(fx["l1_weight"]), perceptual_weight=0.0, lr=3e-4, restart_thres=float(fx["restart_thres"]))
    m = VQGAN(args)
    assert m.codebook._need_init is True
    P = vq.closed_form_params(mg.vqgan_cfg("vq_micro"))
    scale = float(fx["pre_vq_scale"])
    m.load_state_dict({k: (v * scale if k.startswith("pre_vq_conv.") else v) for k, v in P.items() if not k.startswith("codebook.")}, strict=False)
    assert m.codebook._need_init is True                                        # no codes were loaded
    m.compute_dtype = dtype
    return m.to(DEV).train()


def draws(fx, k):
    kw = dict(restart_src=torch.from_numpy(fx[f"src_{k}"]).to(DEV), restart_noise=torch.from_numpy(fx[f"noise_{k}"]).to(DEV))
    if k == 0:
        kw.update(init_src=torch.from_numpy(fx["src_init"]).to(DEV), init_noise=torch.from_numpy(fx["noise_init"]).to(DEV))
    return kw


def test_recon_backward_with_the_codebook_update_follows_the_reference_run(fx):
    """initialisation and three SGD steps with the fixture's draws injected: ids, restart mask and count at every step, the losses to 1e-4,
    the three buffers within 8 x the recorded deviation of the reference from its float64 twin.  After every update the NEXT encode
    must use the new codes: its ids are the fixture's next-step ids (with stale prepared codes they would be the old ones)."""
    m = build(fx, "f32")
    x = torch.from_numpy(fx["x"]).to(DEV)
    thres = float(fx["restart_thres"])
    opt = torch.optim.SGD([p for n, p in m.named_parameters() if n.startswith(vc.TRAINED)], lr=float(fx["sgd_lr"]))
    worst, moved = 0.0, 0
    for k in range(cc.STEPS - 1):
        opt.zero_grad()
        out = m.recon_backward(x, update_codebook=True, **draws(fx, k))
        assert m.codebook._need_init is False
        assert sorted(out) == ["codes_restarted", "commitment_loss", "encodings", "finite", "grad_scale", "perplexity", "recon_loss", "x_recon"]
        assert out["finite"] is True
        assert np.array_equal(out["encodings"].cpu().numpy(), fx[f"ids_{k}"]), f"step {k}: the ids differ from the reference's"
        for key, want in (("recon_loss", fx["step_losses"][k, 0]), ("commitment_loss", fx["step_losses"][k, 1])):
            print(f"[codebook model f32] step {k} {key}: {float(out[key]):.8e} (reference {want:.8e})")
            assert abs(float(out[key]) - want) <= 1e-4 * want, (k, key, float(out[key]), want)
        cb = m.codebook
        mask = fx[f"N_{k}"] >= thres
        assert np.array_equal(cb.N.cpu().numpy() >= thres, mask), f"step {k}: the restart mask differs"
        assert int(out["codes_restarted"]) == int((~mask).sum())
        for name in ("N", "z_avg", "embeddings"):
            ref = fx[f"{name}_{k}"].astype(np.float64)
            err = np.abs(getattr(cb, name).cpu().double().numpy() - ref).max() / np.abs(ref).max()
            gate = 8 * float(fx[f"twin_dev/{name}_{k}"])
            worst = max(worst, err / gate)
            measured(f"codebook model f32 step {k} {name}: {err:.2e} of the maximum, gate {gate:.2e}, ratio {err / gate:.3f}")
            assert err <= gate, (k, name, err, gate)
        opt.step()
        nxt = m.encode(x)
        assert np.array_equal(nxt.cpu().numpy(), fx[f"ids_{k + 1}"]), f"after step {k}: the next encode does not use the updated codes"
        moved += int((fx[f"ids_{k + 1}"] != fx[f"ids_{k}"]).sum())
    assert moved > 0, "the fixture's ids never move: the check above would pass on stale codes"
    measured(f"codebook model f32: worst buffer deviation / gate over three steps {worst:.3f}")


def test_update_codebook_leaves_this_steps_losses_and_gradients_on_the_old_codes(fx):
    """the update runs after the last reader of the codes: losses and every gradient of a step with update_codebook=True are those of the
    same step with the codebook frozen at the codes the search used (the GroupNorm sums of the forward are float atomics: the f32 gate
    of tests/test_gpu_vqgrad.py, 2e-5 of the tensor's maximum, not bits)"""
    a, b = build(fx, "f32"), build(fx, "f32")
    x = torch.from_numpy(fx["x"]).to(DEV)
    b.codebook.init_from(torch.from_numpy(fx["z_0"]).to(DEV), torch.from_numpy(fx["src_init"]).to(DEV), torch.from_numpy(fx["noise_init"]).to(DEV))
    codes = b.codebook.embeddings.clone()
    out_a = a.recon_backward(x, update_codebook=True, **draws(fx, 0))
    out_b = b.recon_backward(x)
    assert torch.equal(b.codebook.embeddings, codes) and "codes_restarted" not in out_b
    assert not torch.equal(a.codebook.embeddings, codes)
    assert torch.equal(out_a["encodings"], out_b["encodings"])
    for key in ("recon_loss", "commitment_loss"):
        assert abs(float(out_a[key]) - float(out_b[key])) <= 1e-4 * float(out_b[key]), key
    ga = {k: p.grad.cpu().double().numpy() for k, p in a.named_parameters() if k.startswith(vc.TRAINED)}
    gb = {k: p.grad.cpu().double().numpy() for k, p in b.named_parameters() if k.startswith(vc.TRAINED)}
    for k in gb:                                # the three exactly-zero bias gradients are judged against their layer's weight gradient
        assert np.abs(ga[k] - gb[k]).max() <= 2e-5 * vc.scale_of(k, gb), k


def test_three_f16_steps_with_the_codebook_update(fx):
    m = build(fx, "f16")
    x = torch.from_numpy(fx["x"]).to(DEV)
    thres = float(fx["restart_thres"])
    opt = torch.optim.SGD([p for n, p in m.named_parameters() if n.startswith(vc.TRAINED)], lr=float(fx["sgd_lr"]))
    totals = []
    for k in range(cc.STEPS - 1):
        opt.zero_grad()
        out = m.recon_backward(x, update_codebook=True, **draws(fx, k))
        assert out["finite"] is True and float(out["perplexity"]) > 1.0
        assert int(out["codes_restarted"]) == int((m.codebook.N < thres).sum())
        totals.append(float(out["recon_loss"]) + float(out["commitment_loss"]))
        opt.step()
    opt.zero_grad()
    out = m.recon_backward(x)
    totals.append(float(out["recon_loss"]) + float(out["commitment_loss"]))
    print(f"[codebook model f16] loss over the steps: {' '.join(f'{v:.5f}' for v in totals)}")
    assert totals[3] < totals[0]


def test_train_step_on_a_fresh_model_initialises_updates_and_steps():
    """no injected draws: the device generator gives them"""
    from tests.helpers import tiny_vqgan
    m, _ = tiny_vqgan(n_codes=512)
    m = m.to(DEV).train()
    m.compute_dtype = "f32"
    opt = m.configure_optimizers()
    x = (torch.rand(2, 3, 4, 16, 16, generator=torch.Generator().manual_seed(3)) - 0.5).to(DEV)
    assert m.codebook._need_init is True and float(m.codebook.N.abs().max()) == 0.0
    w0 = m.decoder.conv_last.conv.weight.detach().clone()
    gen = torch.Generator(device=DEV).manual_seed(9)
    out = m.train_step(x, opt, generator=gen)
    assert m.codebook._need_init is False and out["finite"] is True
    N, rows = m.codebook.N, out["encodings"].numel()
    assert float(N.min()) >= 0.99 - 1e-6 and abs(float(N.sum()) - (0.99 * 512 + 0.01 * rows)) <= 1e-3      # N was 1 after the initialisation
    assert int(out["codes_restarted"]) == int((N < 1.0).sum())
    assert bool(torch.isfinite(m.codebook.embeddings).all())
    assert not torch.equal(m.decoder.conv_last.conv.weight, w0), "the optimizer step was not taken"
    out = m.train_step(x, opt, generator=gen)
    assert 0 <= int(out["encodings"].min()) and int(out["encodings"].max()) < 512


def test_train_vqgan_command_writes_a_checkpoint_that_load_vqgan_reads(tmp_path):
    from tests.test_fvd_frames_host import write_png_tree
    from mebt_amd.vqgan import load_vqgan
    os.makedirs(str(tmp_path / "frames"))
    root = write_png_tree(str(tmp_path / "frames"), 3, 6, seed=2)
    run = str(tmp_path / "run")
    cmd = [sys.executable, "-m", "mebt_amd.train_vqgan", "--data_path", root, "--image_folder", "--sequence_length", "4", "--resolution", "16",
           "--batch_size", "2", "--num_workers", "0", "--n_hiddens", "16", "--downsample", "2", "4", "4", "--embedding_dim", "64", "--n_codes", "512",
           "--max_steps", "4", "--log_every", "1", "--ckpt_every", "2", "--default_root_dir", run, "--dtype", "f32", "--seed", "1",
           "--restart_thres", "0.995"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("step ")]
    assert len(lines) == 4 and all(w in lines[-1] for w in ("recon_loss", "commitment_loss", "perplexity", "codes_restarted", "grad_scale")), res.stdout
    assert os.path.exists(os.path.join(run, "checkpoints", "step=2.ckpt"))
    path = os.path.join(run, "checkpoints", "last.ckpt")
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["global_step"] == 4 and {"codebook.embeddings", "codebook.N", "codebook.z_avg"} <= set(ck["state_dict"])
    assert float(ck["state_dict"]["codebook.N"].abs().max()) > 0.0
    assert ck["hyper_parameters"]["args"].n_codes == 512 and ck["hyper_parameters"]["args"].restart_thres == 0.995
    m = load_vqgan(path, torch.device(DEV))
    assert m.codebook._need_init is False
    m.compute_dtype = "f32"
    x = (torch.rand(1, 3, 4, 16, 16, generator=torch.Generator().manual_seed(5)) - 0.5).to(DEV)
    ids = m.encode(x)
    assert tuple(ids.shape) == (1, 2, 4, 4) and 0 <= int(ids.min()) and int(ids.max()) < 512
