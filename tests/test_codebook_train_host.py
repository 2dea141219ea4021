"""EMA codebook of first-stage training, the parts that need no GPU: the fixture of the real reference (tests/golden/codebook_train)
against the float64 statements of tests/codebook_common.py given the recorded draws, the fixture's own safety margins, the C ABI's
symbols, the argument errors of `python -m mebt_amd.train_vqgan`, and a training checkpoint's round trip on the CPU."""
import argparse

import numpy as np
import pytest
import torch

from tests import codebook_common as cc
from tests.golden import make_golden as mg


@pytest.fixture(scope="module")
def fx():
    return cc.load_fixture()


def test_float64_statements_reproduce_the_fixture_from_its_recorded_draws(fx):
    """initialisation and four updates from the recorded z, ids, src and noise alone: n_total and the restart mask equal exactly, the
    restart rows bit for bit in fp32, N / z_avg / embeddings within 1e-5 of the buffer's maximum of the reference's fp32 buffers (the
    chain below feeds every step the float64 state of the step before; measured 1.6e-6)"""
    c = mg.VQGAN_CONFIGS["vq_micro"]
    n_codes, d, thres = c["n_codes"], c["embedding_dim"], float(fx["restart_thres"])
    z0 = torch.from_numpy(fx["z_0"])
    M = z0.shape[0]
    assert M == 64 and M < n_codes and z0.shape[1] == d
    src, noise = torch.from_numpy(fx["src_init"]), torch.from_numpy(fx["noise_init"])
    assert src.min() >= 0 and src.max() < -(-n_codes // M) * M
    k32 = cc.restart_rows_twin(z0, src, noise)
    N, zavg = torch.ones(n_codes, dtype=torch.float64), k32.double()
    restarts, keeps, worst = 0, 0, 0.0
    for k in range(cc.STEPS):
        z, ids = torch.from_numpy(fx[f"z_{k}"]), torch.from_numpy(fx[f"ids_{k}"]).reshape(-1)
        n_total, encode_sum, _ = cc.sums_twin(ids, z, n_codes)
        assert np.array_equal(n_total.numpy(), fx[f"n_total_{k}"].astype(np.float64)) and int(n_total.sum()) == M
        k_rand = cc.restart_rows_twin(z, torch.from_numpy(fx[f"src_{k}"]), torch.from_numpy(fx[f"noise_{k}"]))
        emb, usage = cc.ema_statements(N, zavg, n_total, encode_sum, k_rand.double(), thres, False)
        Nf = fx[f"N_{k}"]
        assert np.abs(Nf - thres).min() >= 1e-4, "a code sits on the restart edge"
        assert np.array_equal(usage.numpy(), Nf >= thres)
        restarts, keeps = restarts + int((~usage).sum()), keeps + int(usage.sum())
        # a restarted code IS its restart row, to the bit
        assert np.array_equal(fx[f"embeddings_{k}"][~usage.numpy()], k_rand.numpy()[~usage.numpy()])
        for name, t in (("N", N), ("z_avg", zavg), ("embeddings", emb)):
            err = float((torch.from_numpy(fx[f"{name}_{k}"]).double() - t).abs().max() / t.abs().max())
            worst = max(worst, err)
            assert err <= 1e-5, (k, name, err)
            assert float(fx[f"twin_dev/{name}_{k}"]) <= 1e-5
    assert restarts > 0 and keeps > 0
    print(f"[codebook fixture] worst deviation of the reference's fp32 buffers from the float64 statements {worst:.2e} of the buffer's maximum")
    assert fx["step_losses"].shape == (cc.STEPS, 2) and fx["step_losses"][3].sum() < fx["step_losses"][0].sum()


def test_fixture_ids_are_clear_of_rounding(fx):
    """in every recorded forward the best code beats the second best by 2e-3 of its distance, and by 8 times the largest deviation of
    the fp32 distances from float64 ones: after the initialisation the codes are z's own rows plus noise, the best distance comes out
    of a cancellation and a relative gap alone would not keep the ids off rounding"""
    for k in range(cc.STEPS):
        flat = torch.from_numpy(fx[f"z_{k}"])
        e = torch.from_numpy(fx["embeddings_%d" % (k - 1)]) if k else cc.restart_rows_twin(flat, torch.from_numpy(fx["src_init"]),
                                                                                           torch.from_numpy(fx["noise_init"]))
        d32 = (flat ** 2).sum(1, keepdim=True) - 2 * flat @ e.t() + (e.t() ** 2).sum(0, keepdim=True)
        f64, e64 = flat.double(), e.double()
        d64 = (f64 ** 2).sum(1, keepdim=True) - 2 * f64 @ e64.t() + (e64.t() ** 2).sum(0, keepdim=True)
        assert np.array_equal(d64.argmin(1).numpy(), fx[f"ids_{k}"].reshape(-1))
        b2 = torch.topk(d64, 2, dim=1, largest=False).values
        assert float(((b2[:, 1] - b2[:, 0]) / b2[:, 0].abs()).min()) >= 2e-3
        assert float((b2[:, 1] - b2[:, 0]).min()) >= 8 * float((d32.double() - d64).abs().max())


def test_library_exports_the_codebook_operators():
    import ctypes
    from mebt_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mebt_op_codebook_sums", "mebt_op_codebook_ema", "mebt_op_codebook_restart_rows", "mebt_codebook_sums_scratch_bytes",
                 "mebt_codebook_ema_scratch_bytes"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    bound = _lib.load()
    assert bound.mebt_codebook_sums_scratch_bytes(64, 512) == 4 * (3 * 512 + 1 + 64)
    assert bound.mebt_codebook_ema_scratch_bytes(16384) == 4 * 64 and bound.mebt_codebook_ema_scratch_bytes(37) == 4
    # argument checks come before any launch: null operands and empty shapes are refused on a machine without a GPU too
    assert bound.mebt_op_codebook_sums(None, None, None, None, 4, 4, 4, None, 0, None) == 1
    assert b"null" in bound.mebt_last_error()
    assert bound.mebt_op_codebook_restart_rows(None, None, None, None, 4, 4, 4, None) == 1
    assert bound.mebt_op_codebook_ema(None, None, None, None, None, None, None, 4, 4, 1.0, None, 0, None) == 1


def _model(**kw):
    from mebt_amd.vqgan import VQGAN
    c = mg.VQGAN_CONFIGS["vq_micro"]
    return VQGAN(argparse.Namespace(n_hiddens=c["n_hiddens"], downsample=c["downsample"], image_channels=3, embedding_dim=c["embedding_dim"],
                                    n_codes=c["n_codes"], sequence_length=4, sample_every_n_frames=1, resolution=16, **kw))


def test_codebook_keeps_the_restart_arguments_and_needs_init_when_fresh():
    m = _model()
    assert m.codebook._need_init is True and m.codebook.no_random_restart is False and m.codebook.restart_thres == 1.0
    m = _model(no_random_restart=True, restart_thres=0.5)
    assert m.codebook.no_random_restart is True and m.codebook.restart_thres == 0.5
    from mebt.modules.codebook import Codebook
    assert Codebook(8, 4, True, 2.0).restart_thres == 2.0


def test_training_checkpoint_round_trips_on_the_cpu(tmp_path):
    from mebt_amd.train_vqgan import checkpoint_dict
    from mebt_amd.vqgan import VQGAN, load_vqgan
    m = _model(restart_thres=0.995, l1_weight=4.0, perceptual_weight=0.0)
    with torch.no_grad():
        m.codebook.N.fill_(0.75)
        m.codebook.z_avg.mul_(2.0)
    ck = checkpoint_dict(m, 7)
    assert sorted(ck) == ["global_step", "hyper_parameters", "state_dict"] and ck["global_step"] == 7
    assert {"codebook.embeddings", "codebook.N", "codebook.z_avg"} <= set(ck["state_dict"])
    path = str(tmp_path / "last.ckpt")
    torch.save(ck, path)
    back = VQGAN.load_from_checkpoint(path)
    assert back.codebook._need_init is False, "a trained codebook must not be re-initialised on resume"
    assert back.codebook.restart_thres == 0.995
    for k, v in m.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k
    assert load_vqgan(path).codebook._need_init is False
    # a state dict without codes leaves a fresh model waiting for its initialisation
    fresh = _model()
    fresh.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("codebook.")}, strict=False)
    assert fresh.codebook._need_init is True


def test_train_vqgan_refuses_the_phases_that_are_not_built(tmp_path):
    from mebt_amd import train_vqgan as T
    base = ["--data_path", str(tmp_path), "--image_folder"]
    with pytest.raises(SystemExit, match="LPIPS backward"):
        T.main(base + ["--perceptual_weight", "0.1", "--max_steps", "4"])
    with pytest.raises(SystemExit, match="GAN phase"):
        T.main(base + ["--max_steps", "50001"])
    with pytest.raises(SystemExit, match="GAN phase"):
        T.main(base + ["--max_steps", "11", "--discriminator_iter_start", "10"])
    with pytest.raises(SystemExit, match="frame folder"):
        T.main(["--data_path", str(tmp_path / "missing"), "--image_folder", "--max_steps", "4"])
    args = T.build_parser().parse_args(base)
    assert args.max_steps == 50000 and args.discriminator_iter_start == 50000 and args.restart_thres == 1.0 and args.no_random_restart is False
    assert args.n_codes == 2048 and args.embedding_dim == 256 and args.n_hiddens == 240 and tuple(args.downsample) == (4, 4, 4)


def test_update_codebook_refuses_a_cpu_model_and_recon_backward_keeps_its_default():
    import inspect
    from mebt_amd.vqgan import VQGAN
    sig = inspect.signature(VQGAN.recon_backward)
    assert sig.parameters["update_codebook"].default is False
    m = _model()
    with pytest.raises(ValueError, match="GPU"):
        m.codebook.update(torch.zeros(4, 64), torch.zeros(4, dtype=torch.int64))


def test_update_codebook_on_several_ranks_names_what_is_missing(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    m = _model()
    with pytest.raises(NotImplementedError, match="all-reduces.*broadcast"):
        m.recon_backward(torch.zeros(1, 3, 4, 16, 16), update_codebook=True)
    with pytest.raises(NotImplementedError, match="codebook.py:70-72,84-85"):
        m.codebook.update(torch.zeros(4, 64), torch.zeros(4, dtype=torch.int64))
