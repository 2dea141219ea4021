"""Frame-folder data and the frame-ingest definition, on the CPU: the dataset mirror against the reference's own
FrameListDataset items (tests/golden/frames/frames_data.npz), Pillow's fixed-point resampler as mebt_amd.frames builds it
against PIL (frames_resize.npz and, with Pillow installed, a live sweep), the VideoData dispatcher and the train CLI's choice
of data source."""
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "frames")
sys.path.insert(0, ROOT)

from mebt_amd import frames as F  # noqa: E402
from mebt_amd.config import AttrDict  # noqa: E402
from tests.helpers import write_tree  # noqa: E402

# tests/golden/frames/make_golden_frames.py:CASES
CASES = [("s4r16", dict(sequence_length=4, resolution=16, sample_every_n_frames=1, latent_shape=[1, 4, 4]), True, 11),
         ("s3e2r16", dict(sequence_length=3, resolution=16, sample_every_n_frames=2, latent_shape=[1, 2, 2]), True, 12),
         ("whole", dict(sequence_length=-1, resolution=12, sample_every_n_frames=1, latent_shape=[2, 3]), True, 13),
         ("test_s4r10", dict(sequence_length=4, resolution=10, sample_every_n_frames=1, latent_shape=[4]), False, 14)]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL")
    root = str(tmp_path_factory.mktemp("frames"))
    return root, write_tree(root)


def _items(ds, seed):
    random.seed(seed)
    torch.manual_seed(seed)
    return [ds[i] for i in range(len(ds))]


@pytest.mark.parametrize("tag,kw,train,seed", CASES, ids=[c[0] for c in CASES])
def test_dataset_matches_reference_items(tree, tag, kw, train, seed, capsys):
    from mebt_amd.data import FrameListDataset
    root, d = tree
    ds = FrameListDataset(root, train=train, **kw)
    assert capsys.readouterr().out.splitlines()[-1] == f"Total num of discontinuous videos: {int(d[f'{tag}__discontinuous'])}"
    assert ds.discontinuities == int(d[f"{tag}__discontinuous"])
    assert [os.path.relpath(v[0], root) for v in ds.data_all] == [str(x) for x in d[f"{tag}__first_frames"]]
    assert [len(v) for v in ds.data_all] == d[f"{tag}__video_lens"].tolist()
    items = _items(ds, seed)
    R, off = kw["resolution"], 0
    for it, T, perm in zip(items, d[f"{tag}__T"], d[f"{tag}__indices"]):
        n = 3 * int(T) * R * R
        ref = d[f"{tag}__video"][off:off + n].reshape(3, int(T), R, R)
        off += n
        assert it["video"].dtype == torch.float32 and tuple(it["video"].shape) == ref.shape
        assert np.array_equal(it["video"].numpy(), ref), tag
        assert torch.equal(it["indices"], torch.from_numpy(perm))
    assert off == d[f"{tag}__video"].size


@pytest.mark.parametrize("tag,kw,train,seed", CASES, ids=[c[0] for c in CASES])
def test_raw_mode_plus_twin_is_the_float_item(tree, tag, kw, train, seed):
    """raw=True draws the same random numbers and returns the decoded source frames; the numpy twin of the ingest turns
    them into the reference's float clip exactly"""
    from mebt_amd.data import FrameListDataset
    root, d = tree
    raw = _items(FrameListDataset(root, train=train, raw=True, **kw), seed)
    ref = _items(FrameListDataset(root, train=train, **kw), seed)
    for a, b in zip(raw, ref):
        v = a["video"]
        assert v.dtype == torch.uint8 and v.dim() == 4 and v.shape[-1] == 3
        assert torch.equal(a["indices"], b["indices"])
        assert np.array_equal(F.clip_twin(v.numpy(), kw["resolution"]), b["video"].numpy())


def test_twin_matches_pil_fixture_table():
    d = np.load(os.path.join(GOLD, "frames_resize.npz"))
    for i, (h, w, R) in enumerate(d["table"].tolist()):
        a = np.random.RandomState(1000 + i).randint(0, 256, (h, w, 3)).astype(np.uint8)
        y0, x0, S = F.crop_box(h, w)
        got = F.resize_twin(np.ascontiguousarray(a[y0:y0 + S, x0:x0 + S]), R)
        assert np.array_equal(got, d[f"out_{i}"]), (h, w, R)


def test_twin_matches_pil_random_sweep():
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(3)
    for _ in range(40):
        S, R = int(rs.randint(1, 90)), int(rs.randint(1, 90))
        a = rs.randint(0, 256, (S, S, 3)).astype(np.uint8)
        ref = np.asarray(Image.fromarray(a).resize((R, R), Image.BILINEAR))
        assert np.array_equal(F.resize_twin(a, R), ref), (S, R)


def test_coefficient_tables():
    """Pillow's windows: clipped to the input, weights summing to 2**22 up to rounding, one unit weight on a same-size axis"""
    for n_in, n_out in [(240, 128), (64, 128), (7, 5), (1, 3), (128, 128), (1920, 128)]:
        xmin, cnt, k = F.axis_coeffs(n_in, n_out)
        assert k.dtype == np.int32 and k.shape == (n_out, cnt.max())
        assert (xmin >= 0).all() and (xmin + cnt <= n_in).all() and (cnt >= 1).all()
        assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + cnt) >= 0).all()       # the kernel's row span relies on it
        assert (np.abs(k.sum(1) - (1 << 22)) <= cnt).all()
        assert all((k[i, cnt[i]:] == 0).all() for i in range(n_out))
    xmin, cnt, k = F.axis_coeffs(128, 128)
    assert (xmin == np.arange(128)).all() and (k[:, 0] == 1 << 22).all()


def test_norm_table_is_the_reference_expression():
    for u in range(256):
        img = np.full((1, 1, 3), u, np.uint8)
        x = np.asarray(img, dtype=np.float32)
        x /= 255.
        assert F.norm_table()[u] == (x - 0.5)[0, 0, 0]


def test_plan_tiles_fit_the_lds():
    for Hs, Ws, R in [(240, 320, 128), (1080, 1920, 128), (2160, 3840, 128), (64, 64, 256), (7, 9, 5)]:
        y0, x0, S = F.crop_box(Hs, Ws)
        xmin, cnt, k = F.axis_coeffs(S, R)
        p = F._Plan.__new__(F._Plan)
        try:
            F._Plan.__init__(p, Hs, Ws, R, "cpu")
        except ValueError:
            assert (cnt.max() + 1) * R * 3 > F.MAX_LDS_BYTES
            continue
        assert p.span * R * 3 <= F.MAX_LDS_BYTES and 1 <= p.rows <= F.MAX_TILE_ROWS
        for r in range(0, R, p.rows):
            last = min(r + p.rows, R) - 1
            assert xmin[last] + cnt[last] - xmin[r] <= p.span


def test_rejects_non_rgb_frames(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from mebt_amd.data import FrameListDataset
    for mode in ("L", "P", "RGBA"):
        d = tmp_path / mode
        d.mkdir()
        paths = []
        for k in range(1, 6):
            p = str(d / f"v_{k}.png")
            Image.new(mode, (8, 8)).save(p)
            paths.append(p)
        paths.append(str(d / "z_1.png"))                  # the last video is never flushed
        (d / "train.txt").write_text("\n".join(paths) + "\n")
        for raw in (False, True):
            ds = FrameListDataset(str(d), 4, resolution=8, latent_shape=[4], raw=raw)
            with pytest.raises(ValueError, match="RGB"):
                ds[0]


def test_collate_raw_groups_sizes():
    items = [{"video": torch.full((2, h, w, 3), i, dtype=torch.uint8), "indices": torch.arange(4) + i}
             for i, (h, w) in enumerate([(6, 8), (5, 5), (6, 8), (5, 5), (9, 9)])]
    b = F.collate_raw(items, resolution=4)
    raw = b["video"]
    assert isinstance(raw, F.RawVideoBatch) and len(raw) == 5 and raw.shape == (5, 3, 2, 4, 4)
    assert [g[1].tolist() for g in raw.groups] == [[0, 2], [1, 3], [4]]
    for f, s in raw.groups:
        assert f.dtype == torch.uint8 and s.dtype == torch.int32
        assert [int(f[j, 0, 0, 0, 0]) for j in range(len(s))] == s.tolist()
    assert torch.equal(b["indices"], torch.stack([it["indices"] for it in items]))


def test_ingest_needs_the_gpu():
    with pytest.raises(ValueError, match="GPU"):
        F.frames_to_video(torch.zeros(1, 1, 4, 4, 3, dtype=torch.uint8), 4)
    with pytest.raises(ValueError, match="uint8"):
        F.frames_to_video(torch.zeros(1, 1, 4, 4, 3), 4)


def test_video_data_dispatch(tree, tmp_path):
    from mebt_amd.data import FrameListDataset, TokenClipDataset, VideoData
    root, _ = tree
    tok = tmp_path / "tok.npz"
    np.savez(tok, train_data=np.zeros((10, 4, 4), np.int64), train_idx=np.array([0, 10]),
             test_data=np.zeros((10, 4, 4), np.int64), test_idx=np.array([0, 10]))
    a = AttrDict(data_path=str(tok), vtokens=True, image_folder=True, sequence_length=2, resolution=4, spatial_length=4,
                 latent_shape=[2, 4, 4], batch_size=1, num_workers=0)
    assert isinstance(VideoData(a)._dataset(True), TokenClipDataset)
    a = AttrDict(data_path=root, image_folder=True, sequence_length=4, resolution=16, latent_shape=[1, 4, 4], batch_size=2,
                 num_workers=0)
    ds = VideoData(a)._dataset(True)
    assert isinstance(ds, FrameListDataset) and not ds.raw and len(ds) == 5
    loader = VideoData(a, raw=True, shuffle=False).train_dataloader()
    batch = next(iter(loader))
    assert isinstance(batch["video"], F.RawVideoBatch) and batch["indices"].shape == (2, 16)
    float_batch = next(iter(VideoData(a, shuffle=False).train_dataloader()))
    assert float_batch["video"].shape == (2, 3, 4, 16, 16)
    with pytest.raises(NotImplementedError, match="h5py"):
        VideoData(AttrDict(data_path=root, preprocessed_hdf5=True))._dataset(True)
    with pytest.raises(NotImplementedError, match="torchvision"):
        VideoData(AttrDict(data_path=root))._dataset(True)
    with pytest.raises(NotImplementedError, match="torchvision"):
        VideoData(AttrDict(data_path=root, sample_every_n_frames=2))._dataset(True)


def test_sharded_frame_loader(tree):
    from mebt_amd.data import VideoData
    root, _ = tree
    a = AttrDict(data_path=root, image_folder=True, sequence_length=4, resolution=16, latent_shape=[1, 4, 4], batch_size=1,
                 num_workers=0)
    seen = []
    for r in range(2):
        loader = VideoData(a, world_size=2, rank=r, raw=True).train_dataloader()
        assert len(loader) == 3                               # 5 videos, padded to 6
        seen += [int(s) for b in loader for _, s in b["video"].groups for s in s]
    assert all(s == 0 for s in seen)                          # batch size 1: every clip lands in slot 0


def test_train_cli_data_source(tree, tmp_path):
    from mebt_amd.train import check_first_stage, frame_folder_data
    from mebt_amd import presets
    root, _ = tree
    d = AttrDict(data_path=root, image_folder=True, vtokens=False)
    assert frame_folder_data(d)
    assert not frame_folder_data(d, tokens="t.npz")                            # --tokens wins
    assert not frame_folder_data(AttrDict(d, vtokens=True))
    assert not frame_folder_data(AttrDict(d, image_folder=False))
    assert not frame_folder_data(AttrDict(d, data_path=str(tmp_path)))       # a directory without train.txt
    assert not frame_folder_data(AttrDict(d, data_path=os.path.join(root, "train.txt")))
    assert not frame_folder_data(AttrDict())
    cfg = presets.tiny(vtokens=False)
    with pytest.raises(SystemExit, match="ckpt_path"):
        check_first_stage(cfg)
    cfg.model.vqvae.params.ckpt_path = str(tmp_path / "missing.ckpt")
    with pytest.raises(SystemExit, match="no such file"):
        check_first_stage(cfg)
    (tmp_path / "vq.ckpt").write_bytes(b"")
    cfg.model.vqvae.params.ckpt_path = str(tmp_path / "vq.ckpt")
    check_first_stage(cfg)
    with pytest.raises(SystemExit, match="vtokens"):
        check_first_stage(presets.tiny(vtokens=True))

