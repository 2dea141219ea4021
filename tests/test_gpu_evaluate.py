"""One-command evaluation on MI355X: the decoded-video -> uint8-clip kernel (csrc/frames/frames.hip, `mebt_op_video_to_clip_u8`)
against its numpy twin bit for bit, the `samples_u8` log of the sampling drivers, `--device_u8` of the two sampling command lines
against the float route's files, and `python -m mebt_amd.evaluate` end to end against `measure_fvd` on the files it keeps."""
import argparse
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mebt_amd import _lib
from mebt_amd import frames as F
from mebt_amd import scripts_common as SC
from tests.helpers import closed_form_hook, product_config
from tests.test_host_evaluate import edge_values, edge_video

DEV = "cuda"
SENTINEL = 0xA5


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------
def random_video(B, Td, H, W, seed):
    """both sides of the clamp, and the edge values where they fit"""
    rs = np.random.RandomState(seed)
    x = ((rs.rand(B, 3, Td, H, W) - 0.5) * 1.3).astype(np.float32)
    e = edge_values()
    n = min(x.size, len(e))
    x.reshape(-1)[:n] = e[:n]
    return torch.from_numpy(x)


@pytest.mark.parametrize("B,Td,T,H,W", [(2, 4, 4, 16, 16),
                                        (1, 5, 3, 7, 9),           # rows of 27 bytes, frames off dword alignment, T < Td
                                        (3, 2, 2, 128, 128),       # 8 chunks per frame
                                        (1, 1, 1, 1, 1),
                                        (2, 3, 3, 5, 1),
                                        (2, 2, 1, 45, 47)])        # 6345 bytes per frame: two chunks, the second frame off alignment
def test_kernel_equals_the_twin(B, Td, T, H, W):
    x = random_video(B, Td, H, W, seed=B * 100 + H)
    out = F.video_to_clip_u8(x.to(DEV), T)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B, T, H, W, 3) and out.is_contiguous()
    assert torch.equal(out.cpu(), torch.from_numpy(F.video_u8_twin(x, T)))


def test_kernel_equals_the_twin_on_the_edge_values():
    x = edge_video()
    for T in (3, 2):
        assert torch.equal(F.video_to_clip_u8(x.to(DEV), T).cpu(), torch.from_numpy(F.video_u8_twin(x, T)))
    assert torch.equal(F.video_to_clip_u8(x.to(DEV)).cpu(), torch.from_numpy(F.video_u8_twin(x, 3)))       # T=None: every frame
    v = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0]).reshape(1, 1, 1, 1, 4).repeat(1, 3, 1, 1, 1)
    assert F.video_to_clip_u8(v.to(DEV))[0, 0, 0, :, 1].tolist() == [0, 255, 0, 127]                        # NaN writes 0


def test_out_rows_of_a_larger_store():
    """rows 2..3 of a 6-row store of odd-sized clips (567 bytes each): exactly those rows are written"""
    B, Td, T, H, W = 2, 5, 3, 7, 9
    x = random_video(B, Td, H, W, seed=4)
    store = torch.full((6, T, H, W, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    got = F.video_to_clip_u8(x.to(DEV), T, out=store[2:4])
    assert got.data_ptr() == store[2:4].data_ptr()
    host = store.cpu().numpy()
    assert np.array_equal(host[2:4], F.video_u8_twin(x, T))
    assert (host[:2] == SENTINEL).all() and (host[4:] == SENTINEL).all()


def test_argument_checks_raise_without_a_launch(monkeypatch):
    x = torch.zeros(2, 3, 4, 6, 6, device=DEV)
    lib = _lib.load()
    px, st = _lib.ptr(x), _lib.cur_stream()
    for argv, what in (((px, None, 2, 4, 4, 6, 6, st), "null pointer"), ((px, px, 2, 4, 5, 6, 6, st), "bad shape"),
                       ((px, px, 2, 4, 0, 6, 6, st), "bad shape"), ((px, px, 1, 1, 1, 1 << 15, 1 << 15, st), "frame too large")):
        with pytest.raises(_lib.MebtError, match="video_to_clip_u8: " + what):
            _lib.check(lib.mebt_op_video_to_clip_u8(*argv))
    torch.cuda.synchronize()
    assert not x.any()                                              # nothing ran on the tensor both pointers named

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(F._lib, "load", no_launch)
    with pytest.raises(ValueError, match="float32"):
        F.video_to_clip_u8(x.half())
    with pytest.raises(ValueError, match="float32"):
        F.video_to_clip_u8(x[:, :2])
    with pytest.raises(ValueError, match="contiguous"):
        F.video_to_clip_u8(x.transpose(3, 4))
    with pytest.raises(ValueError, match="GPU"):
        F.video_to_clip_u8(x.cpu())
    with pytest.raises(ValueError, match="T = 5"):
        F.video_to_clip_u8(x, 5)
    with pytest.raises(ValueError, match="T = 0"):
        F.video_to_clip_u8(x, 0)
    for bad in (torch.zeros(2, 4, 6, 6, 3, device=DEV),                                  # float
                torch.zeros(2, 3, 6, 6, 3, dtype=torch.uint8, device=DEV),               # another T
                torch.zeros(2, 4, 6, 6, 3, dtype=torch.uint8),                           # on the host
                torch.zeros(2, 4, 6, 6, 6, dtype=torch.uint8, device=DEV)[..., ::2]):    # not contiguous
        with pytest.raises(ValueError, match="out"):
            F.video_to_clip_u8(x, out=bad)


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------
def pixel_model(latent_frames, downsample):
    """the micro transformer (6 layers, 64 wide, closed-form weights) over a latent grid [latent_frames, 4, 4] of 512 codes with a
    closed-form 3D-VQGAN of 16 hidden channels attached: the micro pair of test_gpu_vqgan.py at the temporal ratio of 4 the sampling
    drivers assume, so that `total_length` frames come out of the decode"""
    from mebt.transformer import Net2NetTransformer
    from mebt_amd.vqgan import VQGAN
    from oracle import closed_form as cf
    from oracle import mebt_oracle as orc
    from oracle import vqgan_oracle as vq
    from tests.golden import make_golden as mg
    n_tok = latent_frames * 16
    tcfg, fscfg, mcfg = product_config("micro", vtokens=False)
    tcfg["first_stage_vocab_size"] = tcfg["vocab_size"] = 512
    tcfg["block_size"] = n_tok
    mcfg["params"]["shape"], mcfg["params"]["max_token"], mcfg["params"]["budget"] = [latent_frames, 4, 4], n_tok, n_tok
    model = Net2NetTransformer(tcfg, fscfg, mcfg, cond_stage_key="label")
    model.compute_dtype = "f32"
    ocfg = orc.OracleConfig(6, 2, 64, n_tok, 8, mg.CONFIGS["micro"]["mode"], vocab_size=512, shape=[latent_frames, 4, 4], budget=n_tok,
                            avg_loss=1.0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in cf.state_dict_numpy(orc.param_shapes(ocfg)).items()}, strict=False)
    vcfg = vq.VQGANConfig(16, downsample, 3, 64, 512)
    R = 4 * downsample[1]
    fs = VQGAN(argparse.Namespace(n_hiddens=16, downsample=downsample, image_channels=3, embedding_dim=64, n_codes=512,
                                  sequence_length=latent_frames * downsample[0], sample_every_n_frames=1, resolution=R))
    fs.load_state_dict(vq.closed_form_params(vcfg), strict=False)
    fs.compute_dtype = "f32"
    model.first_stage_model = fs.eval()
    return model.to(DEV).eval()


@pytest.fixture(scope="module")
def micro8():
    """8 frames of 16 x 16 from the latent grid [2, 4, 4] of the micro model"""
    return pixel_model(2, (4, 4, 4))


def scripts_bytes(samples):
    """`write_outputs`' own statement on a driver's float samples"""
    return np.transpose((samples.cpu().numpy() * 255).astype(np.uint8), (0, 2, 3, 4, 1))


def test_drivers_log_samples_u8(micro8):
    """log['samples_u8'] is made from the decoded tensor log['samples'] holds, so it is compared with the same call's floats (a second
    decode is not bitwise equal: GroupNorm sums with float atomics).  `samples` = clamp(x) + 0.5 is a multiple of 2^-25 in [0, 1], so
    samples - 0.5 is exact and the twin adds the same 0.5 back: the twin of (samples - 0.5) is the twin of the decode."""
    from mebt_amd.sampling import bidirect_sample, draft_and_revise_sample, extrapolate
    kw = dict(n_draft=2, draft_t=1.0, draft_k=None, draft_p=None, n_revise=2, revise_t=0.3, revise_k=None, revise_p=None, M=2)
    log = draft_and_revise_sample(micro8, 3, 8, 8, 8, samples_u8=True, **kw)
    assert log["samples_u8"].dtype == torch.uint8 and tuple(log["samples_u8"].shape) == (3, 8, 16, 16, 3) and log["samples_u8"].is_cuda
    assert tuple(log["samples"].shape) == (3, 3, 8, 16, 16)
    assert np.array_equal(log["samples_u8"].cpu().numpy(), F.video_u8_twin(log["samples"].cpu() - 0.5, 8))
    assert np.array_equal(log["samples_u8"].cpu().numpy(), scripts_bytes(log["samples"]))
    assert len(np.unique(log["samples_u8"].cpu().numpy())) > 2                     # not only the two clamped levels
    assert "samples_u8" not in draft_and_revise_sample(micro8, 3, 8, 8, 8, **kw)
    # into the rows of a caller's store, and the two draft drivers
    rows = torch.full((4, 8, 16, 16, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    log = bidirect_sample(micro8, 2, 8, 8, 4, vid_n_steps=2, vid_c_temp=2.0, samples_u8=rows[1:3])
    assert log["samples_u8"].data_ptr() == rows[1:3].data_ptr() and np.array_equal(rows[1:3].cpu().numpy(), scripts_bytes(log["samples"]))
    assert (rows[0] == SENTINEL).all() and (rows[3] == SENTINEL).all()
    assert "samples_u8" not in bidirect_sample(micro8, 2, 8, 8, 4, vid_n_steps=2, vid_c_temp=2.0)
    log = extrapolate(micro8, log["code_maps"], 16, 8, 4, vid_n_steps=2, vid_c_temp=2.0, samples_u8=True)
    assert tuple(log["samples_u8"].shape) == (2, 16, 16, 16, 3) and np.array_equal(log["samples_u8"].cpu().numpy(), scripts_bytes(log["samples"]))


# ---- the two command lines with --device_u8 -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_runs(micro8, tmp_path_factory):
    """`sample` then `draft_and_revise --np_draft <its code maps>` on the micro pair without the flag and with it for both store
    placements, every run under the same noise, the numpy generator seeded in front of the uint8 writer, recording each driver log's float samples"""
    from mebt_amd import draft_and_revise as dnr_cli, sample as sample_cli, sampling
    tmp = tmp_path_factory.mktemp("device_u8")
    mp = pytest.MonkeyPatch()
    mp.chdir(tmp)
    recorded = []

    def load_with_noise(args):
        micro8.noise_hook = micro8.mask_sampler.noise_hook = closed_form_hook()[0]
        return micro8

    def recording(fn):
        def wrapped(*a, **k):
            log = fn(*a, **k)
            recorded.append(log["samples"].cpu().numpy())
            return log
        return wrapped

    def seeded(fn, seeds):
        """the numpy generator set right in front of the writer, so the replay on the recorded floats starts from the same state"""
        def wrapped(args, *a, **k):
            np.random.seed(seeds["seed"])
            return fn(args, *a, **k)
        return wrapped

    seeds = {"seed": 0}
    for mod in (sample_cli, dnr_cli):
        mp.setattr(mod, "write_outputs_u8", seeded(mod.write_outputs_u8, seeds))
    mp.setattr(sample_cli, "load_model", load_with_noise)
    mp.setattr(dnr_cli, "load_model", load_with_noise)
    mp.setattr(sampling, "bidirect_sample", recording(sampling.bidirect_sample))
    mp.setattr(sampling, "draft_and_revise_sample", recording(sampling.draft_and_revise_sample))
    runs = {}
    try:
        for tag, flags in (("float", ""), ("device", " --device_u8 --u8_store device"), ("host", " --device_u8 --u8_store host")):
            common = f"--gpt_ckpt none.ckpt --exp_name {tag} --dtype f32 --batch_size 2 --n_sample 3 --resolution 16 --dataset stl --no_phase --save_codemap"
            del recorded[:]
            seeds["seed"] = 23
            draft = sample_cli.main((f"{common} --total_length 8 --step_size 8 --context_size 4 --vid_n_steps 3 --vid_c_temp 2.0{flags}").split())
            draft_floats = list(recorded)
            del recorded[:]
            seeds["seed"] = 29
            revise = dnr_cli.main((f"{common} --total_length 8 --step_size 8 --context_size 8 --n_revise 2 --M 2 --revise_t 0.5 "
                                   f"--np_draft {draft}_codemap.npy{flags}").split())
            runs[tag] = dict(draft=str(tmp / draft), revise=str(tmp / revise), draft_floats=draft_floats, revise_floats=list(recorded))
    finally:
        mp.undo()
        micro8.noise_hook = micro8.mask_sampler.noise_hook = None
    runs["tmp"] = tmp
    return runs


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("stage,seed,n_batches", [("draft", 23, 2), ("revise", 29, 2)])
def test_device_u8_writes_the_float_routes_files(cli_runs, where, stage, seed, n_batches):
    """the .npy of a --device_u8 run is `write_outputs` of the floats its drivers logged (4 draft clips of which 3 are kept, so the
    permutation matters; the revise run's last batch is a single clip); its code maps are those of the run without the flag"""
    run, floats = cli_runs[where], cli_runs[where][stage + "_floats"]
    assert len(floats) == n_batches and floats[0].shape[1:] == (3, 8, 16, 16)
    want = str(cli_runs["tmp"] / f"want_{where}_{stage}")
    args = argparse.Namespace(save_codemap=False, no_np=False, n_sample=3, total_length=8)
    np.random.seed(seed)
    SC.write_outputs(args, want, floats, [], 16)
    assert open(run[stage] + ".npy", "rb").read() == open(want + ".npy", "rb").read()
    assert np.load(run[stage] + ".npy").shape == (3, 8, 16, 16, 3)
    assert open(run[stage] + "_codemap.npy", "rb").read() == open(cli_runs["float"][stage] + "_codemap.npy", "rb").read()


def test_clip_store_auto_placement():
    """`auto`: in HBM up to a quarter of the free device memory, else pinned host memory"""
    free = torch.cuda.mem_get_info()[0]
    assert SC.ClipStore.placement(int(free * 0.2)) == "device" and SC.ClipStore.placement(int(free * 0.3)) == "host"
    store = SC.ClipStore(4, 2, 8, 8)
    assert store.where == "device" and store.buf.is_cuda and tuple(store.buf.shape) == (4, 2, 8, 8, 3)
    host = SC.ClipStore(4, 2, 8, 8, where="host")
    assert host.where == "host" and host.buf.is_pinned()


# ---- evaluate, end to end -------------------------------------------------------------------------------------------------------------------
def test_evaluate_end_to_end(tmp_path, monkeypatch, capsys):
    """two runs of draft + revise at the smallest geometry the I3D takes, 16 frames of 32 x 32.  `draft_and_revise_sample` asserts
    total_length == step_size and the drivers decode four frames per latent frame, so 16 frames need a latent grid of four frames:
    the micro transformer at block size 64 ([4, 4, 4]) with a (4, 8, 8) closed-form first stage.  Every kept .npy scored by
    `measure_fvd` with the cached real embeddings gives that stage's FVD / KVD (the same bytes through the same batches)."""
    from mebt_amd import evaluate, measure_fvd
    from tests.test_fvd_frames_host import write_png_tree
    from tests.test_gpu_fvd import closed_form_sd
    model = pixel_model(4, (4, 8, 8))
    os.makedirs(tmp_path / "png")
    root = write_png_tree(str(tmp_path / "png"), 40, 18, seed=40)
    ck = str(tmp_path / "w.pt")
    torch.save(closed_form_sd(), ck)
    emb = str(tmp_path / "real_emb.npy")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(evaluate, "load_model", lambda args: model)
    scoring = ["--n_sample", "32", "--resolution", "32", "--num_workers", "0", "--i3d_ckpt", ck, "--i3d_dtype", "f32", "--real_embeddings", emb]
    rows = evaluate.main(f"--gpt_ckpt none.ckpt --exp_name e2e --dtype f32 --batch_size 16 --total_length 16 --step_size 16 --context_size 16 "
                         f"--vid_n_steps 2 --vid_c_temp 2.0 --no_phase --dataset stl --n_revise 1 --M 2 --revise_t 0.5 --keep_np --runs 0-1 "
                         f"--data_path {root} --image_folder --train".split() + scoring)
    out = capsys.readouterr().out
    assert out.count("computing fvd embeddings for real videos") == 1 and out.count("computing fvd embeddings for fake videos") == 4
    assert [(r[0], r[1]) for r in rows] == [(0, "draft"), (0, "revise"), (1, "draft"), (1, "revise")]
    assert "draft: FVD" in out and "revise: FVD" in out and "(2 runs)" in out
    summary = open("results/e2e/evaluate_16_stl.csv").read().splitlines()
    assert summary[0] == "run,stage,FVD,KVD" and len(summary) == 5
    assert summary[1] == f"0,draft,{rows[0][2]!r},{rows[0][3]!r}"
    args, _ = evaluate.parse_args("--exp_name e2e --total_length 16 --vid_n_steps 2 --vid_c_temp 2.0 --no_phase --dataset stl --n_revise 1 --M 2 "
                                  "--revise_t 0.5".split())
    args.save = "results/e2e"
    for run, stage, fvd, kvd in rows:
        csv_path = evaluate.stage_csv_names(args, run)[stage]
        lines = open(csv_path).read().splitlines()
        assert lines[0] == ",FVD,KVD" and lines[1] == f"0,{fvd!r},{kvd!r}", csv_path
        np_file = csv_path.replace("_consq_set_5.csv", ".npy")
        clips = np.load(np_file)
        assert clips.shape == (32, 16, 32, 32, 3) and clips.dtype == np.uint8 and len(np.unique(clips)) > 2
        assert os.path.isfile(np_file.replace(".npy", "_codemap.npy"))
        os.unlink(csv_path)
        fvd2, kvd2 = measure_fvd.main(["--np_file", np_file, "--data_path", "not-a-dataset", "--sequence_length", "16"] + scoring)
        print(f"run {run} {stage}: evaluate FVD {fvd!r} KVD {kvd!r}; measure_fvd FVD {fvd2!r} KVD {kvd2!r}")
        assert abs(fvd - fvd2) <= 1e-9 * max(1.0, abs(fvd2)), (run, stage, fvd, fvd2)
        assert abs(kvd - kvd2) <= 1e-9 * max(1.0, abs(kvd2)), (run, stage, kvd, kvd2)
    assert "for real videos" not in capsys.readouterr().out            # every measure_fvd call read the cached real embeddings
    assert np.isfinite([r[2:] for r in rows]).all()


def test_evaluate_needs_a_first_stage(tmp_path, monkeypatch):
    from mebt_amd import evaluate
    from tests.helpers import build_product
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(evaluate, "load_model", lambda args: build_product("micro", "f32").eval())
    with pytest.raises(SystemExit, match="no first stage"):
        evaluate.main("--gpt_ckpt none.ckpt --exp_name none --no_phase --runs 0".split())
