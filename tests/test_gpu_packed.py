"""Packed frame datasets on MI355X (mebt_amd/packed.py, csrc/frames/frames.hip: `mebt_op_pack_to_video`, `mebt_op_pack_to_clip_u8`):
the gather kernel against numpy with no tolerance (odd resolutions, a pack off its allocation's alignment, rows past 2**32 bytes), a
pack built by `python -m mebt_amd.pack_frames` against the twin-built one, loader batches in both residency modes against the
reference's FrameListDataset items, and the train and FVD command lines from a pack against the same runs from the folder."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mebt_amd import frames as F
from mebt_amd import packed as P
from mebt_amd.config import AttrDict
from tests.helpers import tiny_vqgan, write_tree
from tests.test_packed_host import CASES, RESOLUTIONS, _seed, twin_resize

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FRAMES = 40


# ---- kernel vs numpy ----------------------------------------------------------------------------------------------------------
def id_sets(B, T, n_frames):
    """descending with stride 2 from the last row (wrapping), and rows 0 / F - 1 repeated"""
    n = B * T
    down = (np.arange(n_frames - 1, n_frames - 1 - 2 * n, -2) % n_frames).reshape(B, T)
    ends = np.resize(np.array([0, n_frames - 1, n_frames - 1, 0, 0]), n).reshape(B, T)
    return [down, ends]


def check_gather(pack, pack_np, ids_np):
    R = pack_np.shape[1]
    ids = torch.from_numpy(ids_np.astype(np.int64)).to(DEV)
    rows = pack_np[ids_np]                                                        # [B, T, R, R, 3]
    video = P.pack_to_video(pack, ids, R)
    clip = P.pack_to_clip_u8(pack, ids, R)
    torch.cuda.synchronize()
    assert video.dtype == torch.float32 and tuple(video.shape) == (ids_np.shape[0], 3, ids_np.shape[1], R, R)
    assert clip.dtype == torch.uint8 and tuple(clip.shape) == rows.shape
    assert np.array_equal(video.cpu().numpy(), F.norm_table()[rows].transpose(0, 4, 1, 2, 3))
    assert np.array_equal(clip.cpu().numpy(), F.byte_table()[rows])


@pytest.mark.parametrize("B,T,R", [(3, 5, 16), (2, 3, 17), (4, 2, 31), (1, 1, 1), (2, 4, 128), (2, 3, 47)])
def test_gather_matches_numpy(B, T, R):
    """R = 17 and 31: frames of 867 / 2883 bytes, so source frames start off every alignment and the uint8 runs off a dword
    boundary; R = 1: a 3-byte frame; R = 128: eight chunks per frame; R = 47: frames of 6627 bytes, two chunks each and an odd
    length, so the chunked uint8 runs start at every offset from a dword boundary"""
    pack_np = np.random.RandomState(R).randint(0, 256, (N_FRAMES, R, R, 3)).astype(np.uint8)
    pack = torch.from_numpy(pack_np).to(DEV)
    for ids in id_sets(B, T, N_FRAMES):
        assert ids.min() == 0 or ids.max() == N_FRAMES - 1
        check_gather(pack, pack_np, ids)


@pytest.mark.parametrize("B,T,R", [(3, 5, 16), (2, 3, 17)])
def test_gather_from_a_pack_off_its_allocation(B, T, R):
    """the pack as a slice of a larger byte buffer, one byte past its start: no row is 16-byte aligned when R = 16"""
    pack_np = np.random.RandomState(100 + R).randint(0, 256, (N_FRAMES, R, R, 3)).astype(np.uint8)
    buf = torch.zeros(pack_np.size + 64, dtype=torch.uint8, device=DEV)
    pack = buf[1:1 + pack_np.size].view(N_FRAMES, R, R, 3)
    pack.copy_(torch.from_numpy(pack_np))
    assert pack.data_ptr() % 16 == 1 and pack.is_contiguous()
    for ids in id_sets(B, T, N_FRAMES):
        check_gather(pack, pack_np, ids)


def test_gather_rows_past_4_gib():
    """byte offsets of the gathered rows exceed 2**32: 87 384 frames of 128 x 128 x 3, only the last two written and read"""
    R = 128
    n_frames = (1 << 32) // (R * R * 3) + 3
    assert (n_frames - 2) * R * R * 3 > 1 << 32
    pack = torch.empty(n_frames, R, R, 3, dtype=torch.uint8, device=DEV)
    try:
        last = np.random.RandomState(7).randint(0, 256, (2, R, R, 3)).astype(np.uint8)
        pack[-2:] = torch.from_numpy(last).to(DEV)
        ids = torch.tensor([[n_frames - 1, n_frames - 2]], device=DEV)
        video, clip = P.pack_to_video(pack, ids, R), P.pack_to_clip_u8(pack, ids, R)
        torch.cuda.synchronize()
        rows = last[::-1][None]
        assert np.array_equal(video.cpu().numpy(), F.norm_table()[rows].transpose(0, 4, 1, 2, 3))
        assert np.array_equal(clip.cpu().numpy(), F.byte_table()[rows])
    finally:
        del pack
        torch.cuda.empty_cache()


def test_gather_argument_checks():
    pack = torch.zeros(5, 4, 4, 3, dtype=torch.uint8, device=DEV)
    ids = torch.zeros(2, 3, dtype=torch.int64, device=DEV)
    for fn in (P.pack_to_video, P.pack_to_clip_u8):
        assert tuple(fn(pack, ids, 4).shape) in ((2, 3, 3, 4, 4), (2, 3, 4, 4, 3))
        with pytest.raises(ValueError, match="uint8"):
            fn(pack.float(), ids, 4)
        with pytest.raises(ValueError, match="GPU"):
            fn(pack.cpu(), ids.cpu(), 4)
        with pytest.raises(ValueError, match="ids"):
            fn(pack, ids.int(), 4)
        with pytest.raises(ValueError, match="ids"):
            fn(pack, ids.cpu(), 4)
        with pytest.raises(ValueError, match="ids"):
            fn(pack, ids.view(-1), 4)
        with pytest.raises(ValueError, match="resolution 8"):
            fn(pack, ids, 8)
        with pytest.raises(ValueError, match="uint8 pack"):
            fn(pack.view(5, 2, 8, 3), ids, 2)


# ---- packs of the fixture tree ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("frames"))
    return root, write_tree(root)


@pytest.fixture(scope="module")
def twin_packs(tree, tmp_path_factory):
    root, _ = tree
    out = {}
    for R in RESOLUTIONS:
        out[R] = str(tmp_path_factory.mktemp(f"twin{R}"))
        P.build_pack(root, out[R], R, resize=twin_resize)
    return out


def same_pack(a, b):
    for split in ("train", "test"):
        pa, pb = P.Pack(a, split), P.Pack(b, split)
        assert pa.paths == pb.paths and pa.list_sha1 == pb.list_sha1 and np.array_equal(pa.sizes, pb.sizes)
        assert pa.rows.shape == pb.rows.shape and np.array_equal(pa.rows, pb.rows), split


def test_pack_frames_cli_builds_the_twin_pack(tree, twin_packs, tmp_path):
    root, _ = tree
    out = str(tmp_path / "pack16")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "mebt_amd.pack_frames", "--data_path", root, "--out", out,
                        "--resolution", "16", "--num_workers", "2", "--frames_per_launch", "5"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    n = len(P.Pack(out, "train").paths)
    assert re.search(rf"^train: {n} frames, \d+ bytes, [\d.]+ frames/s", r.stdout, re.M), r.stdout
    assert re.search(r"^test: \d+ frames, ", r.stdout, re.M), r.stdout
    same_pack(out, twin_packs[16])


@pytest.mark.parametrize("R", [12, 10])
def test_gpu_built_pack_equals_the_twin_pack(tree, twin_packs, tmp_path, R):
    root, _ = tree
    out = str(tmp_path / "pack")
    P.build_pack(root, out, R, resize=P.gpu_resize, frames_per_launch=3)
    same_pack(out, twin_packs[R])


# ---- loader batches vs the reference's items ------------------------------------------------------------------------------------
CLIP_CASES = [c for c in CASES if c[1]["sequence_length"] > 0]


@pytest.mark.parametrize("resident", [False, True], ids=["host", "resident"])
@pytest.mark.parametrize("tag,kw,train,seed", CLIP_CASES, ids=[c[0] for c in CLIP_CASES])
def test_loader_batches_equal_the_reference_items(tree, twin_packs, capsys, tag, kw, train, seed, resident):
    from mebt_amd.data import VideoData
    root, d = tree
    R, T = kw["resolution"], kw["sequence_length"]
    n = len(d[f"{tag}__video_lens"])
    a = AttrDict(data_path=root, image_folder=True, batch_size=n, num_workers=0, packed_path=twin_packs[R], packed_resident=resident, **kw)
    data = VideoData(a, shuffle=False, raw=True)
    loader = data.train_dataloader() if train else data.val_dataloader()
    assert ("resident in device memory" if resident else "host memmap") in capsys.readouterr().out
    it = iter(loader)                                # the iterator draws its base seed from torch's generator: seed after it
    _seed(seed)
    batch = next(it)
    v = batch["video"]
    assert isinstance(v, P.PackedVideoBatch) and len(v) == n and v.shape == (n, 3, T, R, R)
    assert v.pack.is_cuda == resident and (resident or torch.equal(v.ids, torch.arange(n * T).view(n, T)))
    ref = torch.from_numpy(d[f"{tag}__video"].reshape(n, 3, T, R, R))
    assert torch.equal(F.to_device_video(v, DEV).cpu(), ref)
    assert torch.equal(batch["indices"], torch.from_numpy(d[f"{tag}__indices"]))
    # the uint8 clip: byte_table of the rows the same draws select
    _seed(seed)
    rows = np.stack([loader.dataset.pack.rows[loader.dataset[i]["video"].numpy()] for i in range(n)])
    clip = v.to(DEV, non_blocking=True).to_clip_u8()
    assert clip.dtype == torch.uint8 and np.array_equal(clip.cpu().numpy(), F.byte_table()[rows])
    assert torch.equal(clip.cpu(), ((ref + 0.5) * 255).movedim(1, -1).byte())     # the reference's own expression on its items


# ---- python -m mebt_amd.train -------------------------------------------------------------------------------------------------
def _plain(x):
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    return [_plain(v) for v in x] if isinstance(x, (list, tuple)) else x


STEP = re.compile(r"^step (\d+): train/loss ([\d.]+) acc1 ([\d.]+) acc5 ([\d.]+) lr (\S+)\s+[\d.]+ ms/step$", re.M)


def test_train_cli_from_a_pack_equals_the_folder_run(tree, twin_packs, tmp_path):
    """3 steps from the folder (in-process loader) and 3 from its pack, same seed: the same clips in the same order, so step 1
    prints the same line (up to the wall-clock figure at its end).  Afterwards the weights differ in the last bit (atomically
    accumulated gradients), which tests/test_gpu_frames.py bounds for two runs on the same clips: rtol 1e-6 on the loss
    statistics, 5e-5 on every parameter (6e-3 on attn.key.bias) at a learning rate ten times this one.  The parameters of the
    step-3 checkpoints are held to those bounds at full precision; the printed loss has only four decimals, so there a
    difference within rtol 1e-6 may still round across one unit of the last digit: |a - b| <= 1e-6 |b| + 1e-4."""
    import yaml
    from mebt_amd import presets
    root, _ = tree
    vq, args = tiny_vqgan()
    ck = str(tmp_path / "vqgan.ckpt")
    torch.save({"state_dict": vq.state_dict(), "hyper_parameters": {"args": args}}, ck)
    cfg = _plain(presets.tiny(vtokens=False))
    cfg["model"]["params"]["vis_epoch"] = 1000
    cfg["model"]["vqvae"]["params"]["ckpt_path"] = ck
    cfg["data"] = dict(data_path=root, image_folder=True, vtokens=False, sequence_length=4, resolution=16, sample_every_n_frames=1,
                       batch_size=2, num_workers=0)
    cfg["exp"] = dict(exact_lr=1e-4)
    yml = tmp_path / "frames.yaml"
    yml.write_text(yaml.safe_dump(cfg))
    base = ["timeout", "-k", "10", "600", sys.executable, "-m", "mebt_amd.train", "--base", str(yml), "--log_every", "1", "--max_steps", "3",
            "--dtype", "f32", "--ckpt_every", "3"]
    outs = []
    for name, extra in (("folder", []), ("pack", [f"data.packed_path={twin_packs[16]}"])):
        r = subprocess.run(base + ["--default_root_dir", str(tmp_path / name)] + extra, cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
        outs.append(r.stdout)
    assert "clips come from the pack" not in outs[0] and "clips come from the pack" in outs[1]
    assert "num_workers=0 is ignored" in outs[1] and "resident in device memory (auto" in outs[1], outs[1]
    folder, pack = STEP.findall(outs[0]), STEP.findall(outs[1])
    print("folder:", folder, "\npack:  ", pack)
    assert [s[0] for s in folder] == ["1", "2", "3"] == [s[0] for s in pack]
    assert folder[0] == pack[0]                                    # step 1: identical as text
    for a, b in zip(folder[1:], pack[1:]):
        assert a[4] == b[4]                                        # the schedule
        assert abs(float(a[1]) - float(b[1])) <= 1e-6 * abs(float(b[1])) + 1e-4, (a, b)
    sd = [torch.load(str(tmp_path / name / "step=3.ckpt"), map_location="cpu", weights_only=False)["state_dict"] for name in ("folder", "pack")]
    assert sd[0].keys() == sd[1].keys()
    worst = ("", 0.0)
    for k in sd[0]:
        if k.startswith("first_stage") or not sd[0][k].is_floating_point():
            continue
        dlt = (sd[0][k].float() - sd[1][k].float()).abs().max().item()
        worst = max(worst, (k, dlt), key=lambda kv: kv[1])
        assert dlt <= (6e-3 if k.endswith("attn.key.bias") else 5e-5), (k, dlt)
    print("largest parameter difference after 3 steps:", worst)


# ---- python -m mebt_amd.measure_fvd ---------------------------------------------------------------------------------------------
SEED, T, R, N_SAMPLE = 31, 16, 32, 40


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """the 40-video tree, the closed-form I3D checkpoint and a fake set"""
    from tests.test_fvd_frames_host import write_png_tree
    from tests.test_gpu_fvd import closed_form_sd
    tmp = tmp_path_factory.mktemp("fvd_packed")
    root = write_png_tree(str(tmp_path_factory.mktemp("png40")), 40, T + 2, seed=40)
    ck = str(tmp / "w.pt")
    torch.save(closed_form_sd(), ck)
    rng = np.random.default_rng(2)
    fake = str(tmp / "fake.npy")
    np.save(fake, rng.integers(0, 256, (64, T, R, R, 3), dtype=np.uint8))
    common = ["--n_sample", str(N_SAMPLE), "--sequence_length", str(T), "--resolution", str(R), "--num_workers", "0", "--i3d_ckpt", ck,
              "--i3d_dtype", "f32"]
    return dict(tmp=tmp, root=root, ck=ck, fake=fake, common=common, folder_args=["--data_path", root, "--image_folder", "--train"])


def test_measure_fvd_from_a_pack_prints_the_folder_routes_numbers(folder, capsys):
    """same bytes, same batch order, and the I3D has no split-K: FVD and KVD character for character"""
    from mebt_amd import measure_fvd as M
    pack = str(folder["tmp"] / "pack")
    assert P.build_pack(folder["root"], pack, R, splits=["train"], resize=P.gpu_resize)["train"] == 40 * (T + 2)
    argv = ["--np_file", folder["fake"]] + folder["folder_args"] + folder["common"]
    capsys.readouterr()
    _seed(SEED)
    a = M.main(argv)
    out_a = capsys.readouterr().out
    _seed(SEED)
    b = M.main(argv + ["--packed_path", pack])
    out_b = capsys.readouterr().out
    assert "resident in device memory (auto" in out_b and "host memmap" not in out_a
    pick = lambda s: [ln for ln in s.splitlines() if ln.startswith(("FVD = ", "KVD = "))]
    assert len(pick(out_a)) == 2 and pick(out_a) == pick(out_b), (pick(out_a), pick(out_b))
    assert a == b and "warning" not in out_b
