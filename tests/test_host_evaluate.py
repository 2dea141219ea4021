"""One-command evaluation, host side (mebt_amd/evaluate.py, scripts_common.ClipStore / write_outputs_u8, frames.video_u8_twin): the
numpy twin of the decoded-video -> uint8-clip kernel against the two statements of the sampling scripts it replaces, the byte identity
of the files the uint8 writer makes, and the command line against the flag sets of the reference's six scripts/valid_dnr_*.sh."""
import argparse
import os

import numpy as np
import pytest
import torch

from mebt_amd import draft_and_revise, evaluate, frames as F, measure_fvd, sample
from mebt_amd import scripts_common as SC


def edge_values():
    """every k / 255 - 0.5 and its two float32 neighbours (where the truncation changes level), +-0.5 and their neighbours (where
    the clamp starts), +-3, -0.0, +-inf"""
    k = (np.arange(256, dtype=np.float32) / np.float32(255)) - np.float32(0.5)
    exact = (np.arange(256, dtype=np.float64) / 255.0 - 0.5).astype(np.float32)
    v = np.concatenate([k, exact])
    v = np.concatenate([v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))])
    half = np.array([-0.5, 0.5], dtype=np.float32)
    extra = np.concatenate([half, np.nextafter(half, np.float32(-np.inf)), np.nextafter(half, np.float32(np.inf)),
                            np.array([3.0, -3.0, -0.0, 0.0, np.inf, -np.inf], dtype=np.float32)])
    return np.concatenate([v, extra]).astype(np.float32)


def edge_video(B=2, Td=3, H=19, W=31, seed=0):
    """float32 [B, 3, Td, H, W]: the edge values first, then random values on both sides of the clamp"""
    n = B * 3 * Td * H * W
    e = edge_values()
    assert n > 2 * len(e)
    rs = np.random.RandomState(seed)
    x = (rs.rand(n).astype(np.float32) - np.float32(0.5)) * np.float32(1.3)
    x[:len(e)] = e
    x[-len(e):] = e[::-1]                       # in another channel and at other offsets of the output dwords
    return torch.from_numpy(x.reshape(B, 3, Td, H, W))


def scripts_bytes(x, T):
    """what the scripts make of a decode: sampling._decode's clamp + 0.5 on torch, then write_outputs' float32 `* 255`, astype"""
    s = (torch.clamp(x, -0.5, 0.5) + 0.5)[:, :, :T]
    return np.transpose((s.numpy() * 255).astype(np.uint8), (0, 2, 3, 4, 1))


@pytest.mark.parametrize("T", [3, 2, 1])
def test_twin_equals_the_scripts_two_statements(T):
    x = edge_video()
    got = F.video_u8_twin(x, T)
    assert got.dtype == np.uint8 and got.shape == (2, T, 19, 31, 3) and got.flags.c_contiguous
    assert np.array_equal(got, scripts_bytes(x, T))
    assert np.array_equal(F.video_u8_twin(x.numpy(), T), got)
    levels = F.video_u8_twin(torch.from_numpy(edge_values()[:256].copy()).reshape(1, 1, 1, 1, 256).expand(1, 3, 1, 1, 256), 1)
    assert len(np.unique(levels)) > 250 and levels.min() == 0 and levels.max() == 255     # the table spans the levels


def test_twin_special_values():
    v = torch.tensor([-0.5, 0.5, -3.0, 3.0, -0.0, float("inf"), float("-inf"), float("nan")]).reshape(1, 1, 1, 1, 8).repeat(1, 3, 1, 1, 1)
    assert F.video_u8_twin(v, 1)[0, 0, 0, :, 0].tolist() == [0, 255, 0, 255, 127, 255, 0, 0]     # NaN writes 0


def test_video_to_clip_u8_rejects_host_and_wrong_tensors():
    x = torch.zeros(1, 3, 2, 4, 4)
    with pytest.raises(ValueError, match="GPU"):
        F.video_to_clip_u8(x)
    with pytest.raises(ValueError, match="float32"):
        F.video_to_clip_u8(x.double())
    with pytest.raises(ValueError, match="float32"):
        F.video_to_clip_u8(torch.zeros(1, 4, 2, 4, 4))
    with pytest.raises(ValueError, match="float32"):
        F.video_to_clip_u8(np.zeros((1, 3, 2, 4, 4), np.float32))


def _args(**kw):
    d = dict(save_codemap=True, no_np=False, n_sample=5, total_length=4)
    d.update(kw)
    return argparse.Namespace(**d)


def test_write_outputs_u8_files_equal_write_outputs(tmp_path, capsys):
    """the same decoded floats through both writers under the same numpy seed: n_total 8 > n_sample 5, so the permutation matters"""
    R, T = 6, 4
    rs = np.random.RandomState(3)
    batches = [torch.from_numpy(((rs.rand(b, 3, T, R, R) - 0.5) * 1.2).astype(np.float32)) for b in (3, 3, 2)]
    batches[0].view(-1)[:len(edge_values())] = torch.from_numpy(edge_values())[:batches[0].numel()]
    codes = [rs.randint(0, 512, (len(b), 1, 2, 2)) for b in batches]
    a_np, b_np = str(tmp_path / "a" / "VID_run0"), str(tmp_path / "b" / "VID_run0")
    # the float route: what the drivers log (clamp + 0.5), moved to the host as the command lines do
    np.random.seed(11)
    SC.write_outputs(_args(), a_np, [(torch.clamp(v, -0.5, 0.5) + 0.5).numpy() for v in batches], codes, R, codemap_limit=5)
    store = SC.ClipStore(8, T, R, R, where="host")
    assert store.where == "host" and tuple(store.buf.shape) == (8, T, R, R, 3) and store.buf.dtype == torch.uint8
    for v in batches:
        assert store.target(len(v)) is True
        store.put(F.video_u8_twin(v, T))
    assert store.n == 8
    np.random.seed(11)
    sel = SC.write_outputs_u8(_args(), b_np, store, codes, codemap_limit=5)
    for suffix in (".npy", "_codemap.npy"):
        assert open(a_np + suffix, "rb").read() == open(b_np + suffix, "rb").read(), suffix
    out = np.load(b_np + ".npy")
    assert out.shape == (5, T, R, R, 3) and np.array_equal(sel.numpy(), out)
    np.random.seed(11)
    assert np.array_equal(out, store.buf.numpy()[np.random.permutation(8)[:5]])
    # keep_np=False: the same draw, the same clips, no video file; --no_np: no draw at all, as in write_outputs
    c_np = str(tmp_path / "c" / "VID_run0")
    np.random.seed(11)
    sel2 = SC.write_outputs_u8(_args(), c_np, store, codes, codemap_limit=5, keep_np=False)
    assert torch.equal(sel2, sel) and not os.path.exists(c_np + ".npy") and os.path.exists(c_np + "_codemap.npy")
    np.random.seed(11)
    assert SC.write_outputs_u8(_args(no_np=True), c_np, store, codes) is None
    assert np.random.randint(1 << 30) == np.random.RandomState(11).randint(1 << 30)
    # a store without clips (no first stage): the message of write_outputs, nothing drawn
    capsys.readouterr()
    assert SC.write_outputs_u8(_args(), c_np, SC.ClipStore(2, T, R, R, where="host"), codes) is None
    assert "no first stage attached" in capsys.readouterr().out


def test_clip_store_bounds_and_reset():
    store = SC.ClipStore(3, 2, 4, 4, where="host")
    store.put(np.zeros((2, 2, 4, 4, 3), np.uint8))
    with pytest.raises(ValueError, match="exceed"):
        store.put(np.zeros((2, 2, 4, 4, 3), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        store.put(np.zeros((1, 2, 4, 4, 3), np.float32))
    with pytest.raises(ValueError, match="uint8"):
        store.put(np.zeros((1, 2, 5, 4, 3), np.uint8))
    store.reset()
    assert store.n == 0
    store.put(np.full((3, 2, 4, 4, 3), 7, np.uint8))
    assert store.n == 3 and int(store.select(np.array([2, 0]))[1, 0, 0, 0, 0]) == 7
    with pytest.raises(ValueError, match="where"):
        SC.ClipStore(1, 1, 1, 1, where="disk")


# the six scripts/valid_dnr_config_ckpt_exp_*.sh of the reference: (dataset, LENGTH, runs, N_DRAFT, CTEMP, the sample line's own flags,
# M, STEPS, TEMP, the data flags of its two measure_fvd lines)
SCRIPTS = [
    ("ucf101", 128, 5, 32, "2.0", "--n_sample 512 --batch_size 4 --decoding_strategy maskgit --top_k 32 --save_codemap --bootstrap 64 --save_n 20",
     2, 32, "0.1", "--data_path datasets/vqgan_data/ucf_128 --image_folder --resolution 128 --train"),
    ("ucf101", 16, 10, 128, "6.0", "--n_sample 2048 --batch_size 16 --decoding_strategy maskgit --save_codemap --save_n 5",
     4, 4, "0.7", "--data_path datasets/vqgan_data/ucf_128 --train --image_folder --resolution 128"),
    ("stl", 128, 5, 32, "4.0", "--n_sample 512 --batch_size 2 --decoding_strategy maskgit --top_k 32 --save_codemap --bootstrap 64 --save_n 20",
     2, 2, "0.7", "--data_path datasets/vqgan_data/stl_128 --image_folder --resolution 128"),
    ("stl", 16, 10, 32, "8.0", "--n_sample 2048 --batch_size 16 --decoding_strategy maskgit --save_codemap --save_n 5",
     2, 2, "0.7", "--data_path datasets/vqgan_data/stl_128 --image_folder --resolution 128"),
    ("taichi", 128, 5, 32, "4.0", "--n_sample 512 --batch_size 4 --decoding_strategy maskgit --top_k 32 --save_codemap --bootstrap 64 --save_n 20",
     4, 2, "0.1", "--data_path datasets/vqgan_data/taichi_fvd --image_folder --resolution 128"),
    ("taichi", 16, 10, 64, "2.0", "--n_sample 2048 --batch_size 16 --decoding_strategy maskgit --save_codemap --save_n 5",
     8, 2, "0.3", "--data_path datasets/vqgan_data/taichi_fvd --image_folder --resolution 128 --sample_every_n_frames 4"),
]


@pytest.mark.parametrize("dataset,L,n_runs,n_draft,ctemp,sample_flags,M,steps,temp,data_flags", SCRIPTS,
                         ids=[f"{s[0]}_{s[1]}f" for s in SCRIPTS])
def test_evaluate_parses_the_shipped_scripts_flags(tmp_path, monkeypatch, dataset, L, n_runs, n_draft, ctemp, sample_flags, M, steps, temp,
                                                   data_flags):
    """one evaluate command line per script = its sample line without --run, the revise knobs of its draft_and_revise line and the
    data flags of its measure_fvd lines; the per-stage CSV names are those the script's own measure_fvd calls write"""
    monkeypatch.chdir(tmp_path)
    common = (f"--base cfg.yaml --gpt_ckpt g.ckpt --exp_name EXP --total_length {L} --context_size {L} --step_size {L} --verbose "
              f"--dataset {dataset} --no_phase --save_videos")
    draft_line = f"{common} --vid_c_temp {ctemp} --vid_n_steps {n_draft} {sample_flags}"
    revise_knobs = f"--n_revise {steps} --M {M} --revise_t {temp}"
    runs = f"0-{n_runs - 1}"
    line = f"{draft_line} {revise_knobs} --compute_fvd {data_flags} --sequence_length {L} --runs {runs}"
    args, unknown = evaluate.parse_args(line.split())
    assert not unknown and args.runs == list(range(n_runs)) and args.stages == ["draft", "revise"] and not args.keep_np
    assert args.sequence_length == L and args.image_folder and args.n_neighbor == 5 and args.i3d_dtype == "f16" and not args.device_u8
    assert args.train == ("--train" in data_flags) and args.n_revise == steps and args.M == M
    assert SC.resolve_checkpoint(args) == "g.ckpt"
    assert evaluate.summary_path(args) == f"results/EXP/evaluate_{L}_{dataset}.csv"
    # without --sequence_length the scorer's clip length is the sampler's
    assert evaluate.parse_args(line.replace(f"--sequence_length {L} ", "").split())[0].sequence_length == L
    n_sample = "512" if L == 128 else "2048"
    bs, save_n = sample_flags.split("--batch_size ")[1].split()[0], sample_flags.split("--save_n ")[1].split()[0]
    for run in (0, n_runs - 1):
        a, _ = sample.build_parser().parse_known_args(f"{draft_line} --run {run}".split())
        SC.resolve_checkpoint(a)
        _, draft_np = sample.output_names(a)
        os.makedirs(os.path.dirname(draft_np), exist_ok=True)
        np.save(draft_np + "_codemap.npy", np.zeros((1, 1, 2, 2), dtype=np.int64))
        b, _ = draft_and_revise.build_parser().parse_known_args(
            f"{common} {revise_knobs} --np_draft {draft_np}_codemap.npy --n_sample {n_sample} --run {run} --batch_size {bs} --save_n {save_n}".split())
        SC.resolve_checkpoint(b)
        _, postfix = draft_and_revise.apply_np_draft(b)
        _, revise_np = draft_and_revise.output_names(b, postfix)
        names = evaluate.stage_csv_names(args, run)
        assert names == {"draft": measure_fvd.consq_csv_name(draft_np + ".npy", 5), "revise": measure_fvd.consq_csv_name(revise_np + ".npy", 5)}
        # and the namespaces the two stages run with are the ones the two command lines parse
        ra = evaluate.revise_args(args, run)
        draft_and_revise.apply_np_draft(ra)
        for k, v in vars(b).items():
            assert getattr(ra, k) == v or k in ("save_codemap", "sequence_length", "resolution", "data_path", "image_folder",
                                                "sample_every_n_frames"), k
        da = evaluate.draft_args(args, run)
        for k, v in vars(a).items():
            assert getattr(da, k) == v or k in ("sequence_length", "resolution", "data_path", "image_folder", "sample_every_n_frames"), k
    assert names["revise"].endswith(f"VID_dnr_nd{n_draft}_dt0.0_nr{steps}_rt{temp}_M{M}_ctemp{ctemp}_run{n_runs - 1}_consq_set_5.csv")


def test_runs_and_stages_flags():
    assert evaluate.parse_runs("0-9") == list(range(10)) and evaluate.parse_runs("3") == [3]
    assert evaluate.parse_runs("0,2,5") == [0, 2, 5] and evaluate.parse_runs("0-2,7") == [0, 1, 2, 7]
    assert evaluate.parse_stages("revise") == ["revise"] and evaluate.parse_stages("revise,draft") == ["draft", "revise"]
    for bad in ("--runs 5-2", "--runs ,", "--stages score", "--stages draft,draft"):
        with pytest.raises(SystemExit):
            evaluate.build_parser().parse_args(bad.split())
    a = evaluate.build_parser().parse_args([])
    assert a.runs == list(range(10)) and a.stages == ["draft", "revise"]
    # the two sampling command lines know the flag, off by default
    for mod in (sample, draft_and_revise):
        p = mod.build_parser()
        assert not p.parse_args([]).device_u8 and p.parse_args(["--device_u8"]).device_u8 and p.parse_args([]).u8_store == "auto"


def test_fake_embeddings_takes_a_tensor_like_an_array(monkeypatch):
    """the same batches of 32, the same cycling and the same random window for a torch tensor as for the numpy array"""
    import random
    from mebt_amd import fvd
    seen = []

    def fake_logits(videos, i3d, device, batch=None):
        v = videos if torch.is_tensor(videos) else torch.from_numpy(videos)
        assert v.is_contiguous()
        seen.append(v.clone())
        return v.reshape(len(v), -1)[:, :4].float()

    monkeypatch.setattr(fvd, "get_fvd_logits", fake_logits)
    data = np.random.RandomState(0).randint(0, 256, (70, 9, 2, 2, 3)).astype(np.uint8)
    args = argparse.Namespace(batch_size=32, n_sample=100, sequence_length=3, sample_fake_n_frames=2, i3d_batch=None, np_file="x.npy")
    random.seed(5)
    a = measure_fvd.fake_embeddings(args, data, None, "cpu")
    first, seen[:] = list(seen), []
    random.seed(5)
    b = measure_fvd.fake_embeddings(args, torch.from_numpy(data), None, "cpu")
    assert len(first) == len(seen) == 4 and all(torch.equal(x, y) for x, y in zip(first, seen))
    assert torch.equal(a, b) and tuple(a.shape) == (100, 4) and tuple(first[0].shape) == (32, 3, 2, 2, 3)
