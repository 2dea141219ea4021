"""Frame ingest (csrc/frames/frames.hip) and pixel-space training on MI355X: the kernel against PIL's outputs and the reference's
FrameListDataset items (tests/golden/frames/), a TrainLoop step on raw frames against the token step on the same clips, and
`python -m mebt_amd.train` on a frame folder with a saved first stage."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mebt_amd import frames as F
from tests.helpers import tiny_vqgan, write_tree
from tests.test_frames_host import CASES

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "frames")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("frames"))
    return root, write_tree(root)


def test_kernel_matches_pil_on_the_fixture_table():
    d = np.load(os.path.join(GOLD, "frames_resize.npz"))
    lut = torch.from_numpy(F.norm_table())
    for i, (h, w, R) in enumerate(d["table"].tolist()):
        a = np.random.RandomState(1000 + i).randint(0, 256, (h, w, 3)).astype(np.uint8)
        out = F.frames_to_video(torch.from_numpy(a).view(1, 1, h, w, 3).to(DEV), R)
        torch.cuda.synchronize()
        ref = lut[torch.from_numpy(d[f"out_{i}"]).long()].permute(2, 0, 1).reshape(1, 3, 1, R, R)
        assert torch.equal(out.cpu(), ref), (h, w, R)


@pytest.mark.parametrize("B,T,h,w,R", [(3, 5, 240, 320, 128), (2, 7, 33, 47, 17), (1, 3, 128, 96, 128), (4, 2, 9, 9, 31),
                                       (2, 3, 200, 150, 64)])
def test_kernel_matches_the_twin_on_batches(B, T, h, w, R):
    """several clips and frames per launch, partial row tiles (R not a multiple of the tile), up- and downscales"""
    rs = np.random.RandomState(B * 1000 + R)
    a = rs.randint(0, 256, (B, T, h, w, 3)).astype(np.uint8)
    out = F.frames_to_video(torch.from_numpy(a).to(DEV), R).cpu()
    ref = np.stack([F.clip_twin(a[b], R) for b in range(B)])
    assert torch.equal(out, torch.from_numpy(ref))


@pytest.mark.parametrize("tag,kw,train,seed", [c for c in CASES if c[1]["sequence_length"] > 0], ids=[c[0] for c in CASES
                                                                                                     if c[1]["sequence_length"] > 0])
def test_raw_batches_equal_the_reference_items(tree, tag, kw, train, seed):
    """the reference's own items (PIL in its DataLoader workers) against raw mode + collate + the kernel: mixed source sizes
    in one batch, crop-only frames (crop side == R) and resized ones"""
    from mebt_amd.data import FrameListDataset
    root, d = tree
    ds = FrameListDataset(root, train=train, raw=True, **kw)
    random.seed(seed)
    torch.manual_seed(seed)
    items = [ds[i] for i in range(len(ds))]
    batch = F.collate_raw(items, kw["resolution"])
    assert len(batch["video"].groups) == len({tuple(it["video"].shape) for it in items}) > 1
    out = F.to_device_video(batch["video"].pin_memory(), DEV).cpu()
    R, T = kw["resolution"], kw["sequence_length"]
    ref = d[f"{tag}__video"].reshape(len(items), 3, T, R, R)
    assert torch.equal(out, torch.from_numpy(ref))
    assert torch.equal(batch["indices"], torch.from_numpy(d[f"{tag}__indices"]))


def _tiny_model(vq):
    from mebt_amd import presets
    torch.manual_seed(3)
    cfg = presets.tiny(vtokens=False)
    cfg.exp.exact_lr = 1e-3
    model = presets.build_model(cfg, compute_dtype="f32")
    model.first_stage_model = vq
    return model


def test_train_step_on_raw_frames_equals_the_token_step(tree):
    """TrainLoop.step on a raw uint8 batch (mixed source sizes) = the token step on VQGAN.encode of the reference's float
    clips: same token ids, same loss statistics, same parameters after two steps"""
    from mebt_amd.data import FrameListDataset
    from mebt_amd.trainer import TrainLoop
    root, d = tree
    tag, kw, train, seed = CASES[0]                              # 5 clips of T 4 at R 16 -> tokens [2, 8, 8]
    ds = FrameListDataset(root, train=train, raw=True, **kw)
    random.seed(seed)
    torch.manual_seed(seed)
    items = [ds[i] for i in range(len(ds))]
    batch = F.collate_raw(items, kw["resolution"])
    ref_video = torch.from_numpy(d[f"{tag}__video"].reshape(len(items), 3, 4, 16, 16)).to(DEV)
    vq, _ = tiny_vqgan()
    vq = vq.to(DEV).eval()
    vq.compute_dtype = "f32"
    ids_ref = vq.encode(ref_video)
    ids_raw = vq.encode(batch["video"].to(DEV).to_video())
    assert torch.equal(ids_ref, ids_raw)
    perms = torch.stack([torch.randperm(128, generator=torch.Generator().manual_seed(i)) for i in range(len(items))]).to(DEV)

    stats, params = [], []
    for kind in ("raw", "tokens"):
        model = _tiny_model(vq).to(DEV).train()
        loop = TrainLoop(model, max_steps=10, fused_optimizer=False)
        random.seed(77)
        st = []
        for _ in range(2):
            x = batch["video"].to(DEV, non_blocking=True) if kind == "raw" else ids_ref
            st.append(loop.step(x, perms).cpu())
        torch.cuda.synchronize()
        stats.append(torch.stack(st))
        params.append({k: v.detach().float().cpu().clone() for k, v in model.state_dict().items() if not k.startswith("first_stage")})
    assert torch.equal(stats[0][0], stats[1][0])                 # same ids, same weights: the first forward is the same
    assert torch.allclose(stats[0], stats[1], rtol=1e-6, atol=0)
    for k in params[0]:
        # atomically accumulated gradients (embedding rows, bias column sums) may differ in the last bit between two runs
        # (tests/test_gpu_product.py): bounded well below one AdamW step of lr 1e-3
        dlt = (params[0][k] - params[1][k]).abs().max().item()
        assert dlt <= (6e-3 if k.endswith("attn.key.bias") else 5e-5), (k, dlt)


def test_pixel_video_step_takes_the_float_contract(tree):
    """a float pixel video [B, 3, T, H, W] (the reference's batch) goes through encode_to_z in TrainLoop.step"""
    from mebt_amd.trainer import TrainLoop
    _, d = tree
    vq, _ = tiny_vqgan()
    vq = vq.to(DEV).eval()
    video = torch.from_numpy(d["s4r16__video"].reshape(5, 3, 4, 16, 16)).to(DEV)
    model = _tiny_model(vq).to(DEV).train()
    loop = TrainLoop(model, max_steps=10, fused_optimizer=False)
    random.seed(1)
    st = loop.step(video, torch.stack([torch.randperm(128) for _ in range(5)]).to(DEV)).cpu()
    assert loop.step_count == 1 and torch.isfinite(st).all() and float(st[3]) > 0


def test_train_cli_on_a_frame_folder_and_resume(tree, tmp_path):
    import yaml
    from mebt_amd import presets
    root, _ = tree
    vq, args = tiny_vqgan()
    ck = str(tmp_path / "vqgan.ckpt")
    torch.save({"state_dict": vq.state_dict(), "hyper_parameters": {"args": args}}, ck)

    def plain(x):
        if isinstance(x, dict):
            return {k: plain(v) for k, v in x.items()}
        return [plain(v) for v in x] if isinstance(x, (list, tuple)) else x
    cfg = plain(presets.tiny(vtokens=False))
    cfg["model"]["params"]["vis_epoch"] = 1000
    cfg["model"]["vqvae"]["params"]["ckpt_path"] = ck
    cfg["data"] = dict(data_path=root, image_folder=True, vtokens=False, sequence_length=4, resolution=16, sample_every_n_frames=1,
                       batch_size=2, num_workers=2)
    cfg["exp"] = dict(exact_lr=1e-4)
    yml = tmp_path / "frames.yaml"
    yml.write_text(yaml.safe_dump(cfg))
    runs = str(tmp_path / "runs")
    base = [sys.executable, "-m", "mebt_amd.train", "--base", str(yml), "--log_every", "1", "--ckpt_every", "2",
            "--default_root_dir", runs]
    r = subprocess.run(["timeout", "-k", "10", "600"] + base + ["--max_steps", "4"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "Total num of videos: 5" in r.stdout                  # the train list; 5 clips at batch 2 = 3 steps per epoch
    assert "step 4: train/loss" in r.stdout and "epoch 1: val/loss" in r.stdout, r.stdout[-3000:]
    assert os.path.exists(os.path.join(runs, "step=2.ckpt")) and os.path.exists(os.path.join(runs, "step=4.ckpt"))
    r2 = subprocess.run(["timeout", "-k", "10", "600"] + base + ["--max_steps", "5", "--ckpt_path", os.path.join(runs, "step=4.ckpt")],
                        cwd=ROOT, capture_output=True, text=True)
    assert r2.returncode == 0, (r2.stdout[-3000:], r2.stderr[-3000:])
    assert "step 5: train/loss" in r2.stdout and "step 4:" not in r2.stdout, r2.stdout[-3000:]
