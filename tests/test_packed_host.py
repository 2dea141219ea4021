"""Packed frame datasets on the CPU (mebt_amd/packed.py): the builder's bookkeeping with the numpy twin as the resize, the packed
dataset against the reference's own FrameListDataset items (tests/golden/frames/frames_data.npz), the host-mode collate, stale
and interrupted packs, the data-source choice and the id checks that come before any launch."""
import os
import random
import shutil
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mebt_amd import frames as F  # noqa: E402
from mebt_amd import packed as P  # noqa: E402
from mebt_amd.config import AttrDict  # noqa: E402
from tests.helpers import write_tree  # noqa: E402

# tests/golden/frames/make_golden_frames.py:CASES
CASES = [("s4r16", dict(sequence_length=4, resolution=16, sample_every_n_frames=1, latent_shape=[1, 4, 4]), True, 11),
         ("s3e2r16", dict(sequence_length=3, resolution=16, sample_every_n_frames=2, latent_shape=[1, 2, 2]), True, 12),
         ("whole", dict(sequence_length=-1, resolution=12, sample_every_n_frames=1, latent_shape=[2, 3]), True, 13),
         ("test_s4r10", dict(sequence_length=4, resolution=10, sample_every_n_frames=1, latent_shape=[4]), False, 14)]
RESOLUTIONS = (16, 12, 10)


def twin_resize(frames, R):
    """build_pack's `resize` on the CPU: center crop + frames.resize_twin; h == w == R is a copy"""
    n, h, w, _ = frames.shape
    if h == R and w == R:
        return frames.copy()
    y0, x0, S = F.crop_box(h, w)
    return np.stack([F.resize_twin(np.ascontiguousarray(f[y0:y0 + S, x0:x0 + S]), R) for f in frames])


def fixture_frames(d):
    """relative name -> decoded uint8 [h, w, 3]"""
    out, off = {}, 0
    for name, shp in zip(d["names"], d["shapes"]):
        n = int(np.prod(shp))
        out[str(name)] = d["pixels"][off:off + n].reshape(shp)
        off += n
    return out


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("frames"))
    return root, write_tree(root)


@pytest.fixture(scope="module")
def packs(tree, tmp_path_factory):
    """the twin-built packs of the fixture tree: resolution -> directory (both splits)"""
    root, _ = tree
    out = {}
    for R in RESOLUTIONS:
        out[R] = str(tmp_path_factory.mktemp(f"pack{R}"))
        n = P.build_pack(root, out[R], R, splits=("train", "test"), resize=twin_resize, frames_per_launch=7)
        assert set(n) == {"train", "test"} and all(v > 0 for v in n.values())
    return out


def _seed(s):
    random.seed(s)
    torch.manual_seed(s)


# ---- builder vs twin ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", RESOLUTIONS)
@pytest.mark.parametrize("split", ["train", "test"])
def test_builder_rows_are_the_twin_of_every_frame(tree, packs, R, split):
    from mebt_amd.data import FrameListDataset, is_image_file
    root, d = tree
    px = fixture_frames(d)
    pack = P.Pack(packs[R], split)
    assert pack.version == P.VERSION and pack.resolution == R
    assert pack.rows.dtype == np.uint8 and pack.rows.shape == (len(pack.paths), R, R, 3)
    assert sorted(os.listdir(packs[R])) == ["test_frames.npy", "test_index.npz", "train_frames.npy", "train_index.npz"]

    # paths: the sorted image list without the placeholder entries and without the never-flushed last video
    lines = sorted(os.path.join(root, str(n)) for n in d[f"{split}_list"])
    images = [p for p in lines if is_image_file(p)]
    if split == "train":
        assert len(images) < len(lines)                                   # the train list holds placeholder entries
    assert pack.paths == images[:len(pack.paths)] and len(pack.paths) < len(images)
    videos = FrameListDataset(root, 0, resolution=R, train=split == "train", latent_shape=[1]).data_all
    assert [p for v in videos for p in v] == pack.paths
    last = images[len(pack.paths):]                                       # one video: one id, consecutive frame numbers
    assert len({os.path.basename(p).rsplit("_", 1)[0] for p in last}) == 1
    assert pack.list_sha1 == P.list_sha1(root, split) and len(pack.list_sha1) == 40

    row = 0
    for v in videos:
        h, w = px[os.path.relpath(v[0], root)].shape[:2]                  # the first frame decides the crop of the whole video
        y0, x0, S = F.crop_box(h, w)
        for p in v:
            f = px[os.path.relpath(p, root)]
            assert f.shape[:2] == (h, w)
            ref = f if (h == R and w == R) else F.resize_twin(np.ascontiguousarray(f[y0:y0 + S, x0:x0 + S]), R)
            assert np.array_equal(pack.rows[row], ref), p
            assert tuple(pack.sizes[row]) == (h, w)
            row += 1
    assert row == len(pack.paths)


def test_builder_rejects_a_frame_of_another_size(tmp_path):
    from PIL import Image
    paths = []
    for k in range(1, 5):
        p = str(tmp_path / f"v_{k}.png")
        Image.new("RGB", (8, 6) if k != 3 else (6, 8)).save(p)
        paths.append(p)
    paths.append(str(tmp_path / "z_1.png"))
    (tmp_path / "train.txt").write_text("\n".join(paths) + "\n")
    with pytest.raises(ValueError, match="8x6 frame in a video of 6x8"):
        P.build_pack(str(tmp_path), str(tmp_path / "pack"), 4, splits=["train"], resize=twin_resize)
    assert os.listdir(tmp_path / "pack") == []


# ---- dataset vs the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,kw,train,seed", CASES, ids=[c[0] for c in CASES])
def test_packed_dataset_matches_reference_items(tree, packs, tmp_path, monkeypatch, tag, kw, train, seed):
    """the golden float items of the reference's FrameListDataset from pack rows + the float table, with only the list files of
    the folder at hand and no image opened"""
    root, d = tree
    lists = tmp_path / "lists"
    lists.mkdir()
    for lst in ("train.txt", "test.txt"):
        shutil.copy(os.path.join(root, lst), lists / lst)
    import mebt_amd.data as D
    monkeypatch.setattr(D, "_open_rgb", lambda path: pytest.fail(f"the packed dataset opened {path}"))
    R = kw["resolution"]
    ds = P.PackedFrameDataset(str(lists), packs[R], train=train, **kw)
    assert [len(v) for v in ds.data_all] == d[f"{tag}__video_lens"].tolist() and len(ds) == len(d[f"{tag}__video_lens"])
    assert [os.path.relpath(v[0], root) for v in ds.data_all] == [str(x) for x in d[f"{tag}__first_frames"]]
    _seed(seed)
    items = [ds[i] for i in range(len(ds))]
    lut, off = F.norm_table(), 0
    for it, T, perm in zip(items, d[f"{tag}__T"], d[f"{tag}__indices"]):
        n = 3 * int(T) * R * R
        ref = d[f"{tag}__video"][off:off + n].reshape(3, int(T), R, R)
        off += n
        rows = it["video"]
        assert rows.dtype == torch.int64 and tuple(rows.shape) == (int(T),)
        got = lut[ds.pack.rows[rows.numpy()]].transpose(3, 0, 1, 2)
        assert got.dtype == np.float32 and np.array_equal(got, ref), tag
        assert torch.equal(it["indices"], torch.from_numpy(perm))
    assert off == d[f"{tag}__video"].size


# ---- host-mode collate --------------------------------------------------------------------------------------------------------
def test_host_mode_collate_gathers_the_rows(tree, packs):
    root, _ = tree
    tag, kw, train, seed = CASES[0]
    ds = P.PackedFrameDataset(root, packs[16], train=train, **kw)
    _seed(seed)
    items = [ds[i] for i in range(3)]
    batch = P.collate_packed(items, ds.pack, resident=False)
    v = batch["video"]
    assert isinstance(v, P.PackedVideoBatch) and isinstance(v, F.RawVideoBatch)
    assert len(v) == 3 and v.shape == (3, 3, 4, 16, 16)
    assert torch.equal(v.ids, torch.arange(12).view(3, 4)) and v.ids.dtype == torch.int64
    assert v.pack.dtype == torch.uint8 and tuple(v.pack.shape) == (12, 16, 16, 3)
    want = np.stack([ds.pack.rows[int(r)] for it in items for r in it["video"]])
    assert np.array_equal(v.pack.numpy(), want)
    assert torch.equal(batch["indices"], torch.stack([it["indices"] for it in items]))
    moved = v.to("cpu")
    assert torch.equal(moved.pack, v.pack) and torch.equal(moved.ids, v.ids) and moved.shape == v.shape


# ---- stale and interrupted packs ------------------------------------------------------------------------------------------------
def _copy_lists(root, dst):
    os.makedirs(dst, exist_ok=True)
    for lst in ("train.txt", "test.txt"):
        shutil.copy(os.path.join(root, lst), os.path.join(dst, lst))
    return str(dst)


def test_stale_packs_name_the_rebuild_command(tree, packs, tmp_path):
    root, _ = tree
    kw = dict(sequence_length=4, sample_every_n_frames=1, latent_shape=[1, 4, 4])
    P.PackedFrameDataset(root, packs[16], resolution=16, **kw)                       # the pack as built loads

    def command(folder, pack_dir, R):
        return f"python -m mebt_amd.pack_frames --data_path {folder} --out {pack_dir} --resolution {R} --split train"

    # another resolution
    with pytest.raises(ValueError) as e:
        P.PackedFrameDataset(root, packs[16], resolution=12, **kw)
    assert "resolution 16" in str(e.value) and command(root, packs[16], 12) in str(e.value)
    # an edited list
    edited = _copy_lists(root, tmp_path / "edited")
    lines = open(os.path.join(edited, "train.txt")).read().splitlines()
    open(os.path.join(edited, "train.txt"), "w").write("\n".join(lines[1:]) + "\n")
    with pytest.raises(ValueError) as e:
        P.PackedFrameDataset(edited, packs[16], resolution=16, **kw)
    assert "train.txt changed" in str(e.value) and command(edited, packs[16], 16) in str(e.value)
    # a path missing from `paths`
    broken = str(tmp_path / "broken")
    shutil.copytree(packs[16], broken)
    z = dict(np.load(os.path.join(broken, "train_index.npz")))
    gone = str(z["paths"][2])
    z["paths"] = np.array([p if i != 2 else p + ".moved" for i, p in enumerate(z["paths"])])
    with open(os.path.join(broken, "train_index.npz"), "wb") as f:
        np.savez(f, **z)
    with pytest.raises(ValueError) as e:
        P.PackedFrameDataset(root, broken, resolution=16, **kw)
    assert f"{gone} is not in the pack" in str(e.value) and command(root, broken, 16) in str(e.value)
    # another format version
    z["paths"] = np.load(os.path.join(packs[16], "train_index.npz"))["paths"]
    z["version"] = np.int64(P.VERSION + 1)
    with open(os.path.join(broken, "train_index.npz"), "wb") as f:
        np.savez(f, **z)
    with pytest.raises(ValueError, match="version") as e:
        P.PackedFrameDataset(root, broken, resolution=16, **kw)
    assert command(root, broken, 16) in str(e.value)
    # no pack at all
    with pytest.raises(ValueError) as e:
        P.PackedFrameDataset(root, str(tmp_path), resolution=16, **kw)
    assert command(root, str(tmp_path), 16) in str(e.value)


def test_an_interrupted_build_leaves_nothing_that_loads(tree, tmp_path):
    root, _ = tree
    calls = []

    def dies_midway(frames, R):
        calls.append(len(frames))
        if len(calls) == 3:
            raise KeyboardInterrupt
        return twin_resize(frames, R)

    out = str(tmp_path / "pack")
    with pytest.raises(KeyboardInterrupt):
        P.build_pack(root, out, 16, splits=["train"], resize=dies_midway, frames_per_launch=4)
    assert len(calls) == 3 and os.listdir(out) == []
    with pytest.raises(ValueError, match="pack_frames"):
        P.PackedFrameDataset(root, out, 4, resolution=16, latent_shape=[4])
    with pytest.raises(ValueError, match="frames_per_launch"):
        P.build_pack(root, out, 16, splits=["train"], resize=twin_resize, frames_per_launch=65536)


# ---- data source choice ---------------------------------------------------------------------------------------------------------
def test_video_data_takes_the_pack(tree, packs, capsys):
    from mebt_amd.data import FrameListDataset, VideoData
    root, d = tree
    a = AttrDict(data_path=root, image_folder=True, sequence_length=4, resolution=16, latent_shape=[1, 4, 4], batch_size=2, num_workers=8,
                 packed_path=packs[16], packed_resident=False)
    ds = VideoData(a)._dataset(True)
    assert isinstance(ds, P.PackedFrameDataset) and len(ds) == 5
    assert isinstance(VideoData(a)._dataset(False), P.PackedFrameDataset)
    plain = VideoData(AttrDict({k: v for k, v in a.items() if not k.startswith("packed")}))._dataset(True)
    assert isinstance(plain, FrameListDataset) and not isinstance(plain, P.PackedFrameDataset)
    capsys.readouterr()
    data = VideoData(a, raw=True, shuffle=False)
    loader = data.train_dataloader()
    out = capsys.readouterr().out
    assert "host memmap (data.packed_resident: False)" in out and "num_workers=8 is ignored" in out
    assert loader.num_workers == 0 and len(loader) == 3
    batch = next(iter(loader))
    assert isinstance(batch["video"], P.PackedVideoBatch) and batch["video"].shape == (2, 3, 4, 16, 16)
    assert batch["indices"].shape == (2, 16)
    data.train_dataloader()
    assert "packed_resident" not in capsys.readouterr().out           # the split's pack is opened once
    for r in range(2):                                                # data parallel: the frame loader's sharding
        sharded = VideoData(a, world_size=2, rank=r).train_dataloader()
        assert len(sharded) == 2 and type(sharded.sampler).__name__ == "ShardedSampler"
    with pytest.raises(ValueError, match="packed_resident"):
        P.choose_resident(ds.pack, "sometimes")
    assert P.choose_resident(ds.pack, True)[0] is True and P.choose_resident(ds.pack, "False")[0] is False


def test_train_cli_data_source_with_a_pack(tree, packs, tmp_path):
    from mebt_amd.train import frame_folder_data, packed_frame_data
    root, _ = tree
    d = AttrDict(data_path=root, image_folder=True, vtokens=False, packed_path=packs[16])
    assert frame_folder_data(d) and packed_frame_data(d)
    assert not packed_frame_data(AttrDict(d, packed_path=None)) and frame_folder_data(AttrDict(d, packed_path=None))
    assert not packed_frame_data(AttrDict({k: v for k, v in d.items() if k != "packed_path"}))
    assert not packed_frame_data(d, tokens="t.npz")                             # --tokens wins
    assert not packed_frame_data(AttrDict(d, vtokens=True))
    assert not packed_frame_data(AttrDict(d, image_folder=False))
    assert not packed_frame_data(AttrDict(d, data_path=str(tmp_path)))        # the list files still come from data_path
    assert not packed_frame_data(AttrDict())


def test_fvd_parser_takes_packed_path(tree, packs):
    from mebt_amd import measure_fvd as M
    root, _ = tree
    for sliding in (False, True):
        assert M.build_parser(sliding).parse_args([]).packed_path == ""
        args = M.build_parser(sliding).parse_args(["--data_path", root, "--image_folder", "--packed_path", packs[16]])
        assert args.packed_path == packs[16] and M.frame_folder(args)


# ---- id checks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [5, -1])
def test_out_of_range_ids_raise_before_any_library_call(monkeypatch, bad):
    from mebt_amd import _lib
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was called"))
    pack = torch.zeros(5, 4, 4, 3, dtype=torch.uint8)
    ids = torch.tensor([[0, 4], [bad, 1]])
    batch = P.PackedVideoBatch(pack, ids, 4)
    for call in (batch.to_video, batch.to_clip_u8, batch.to("cpu").to_video):
        with pytest.raises(IndexError, match=r"outside the pack's \[0, 5\)"):
            call()


def test_gather_needs_the_gpu():
    pack = torch.zeros(5, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        P.pack_to_video(pack, torch.zeros(1, 2, dtype=torch.int64), 4)
    with pytest.raises(ValueError, match="uint8"):
        P.pack_to_clip_u8(pack.float(), torch.zeros(1, 2, dtype=torch.int64), 4)


def test_packed_path_without_a_frame_folder_is_refused(tree, packs, tmp_path):
    from mebt_amd.data import VideoData
    root, _ = tree
    tok = tmp_path / "tok.npz"
    np.savez(tok, train_data=np.zeros((10, 4, 4), np.int64), train_idx=np.array([0, 10]),
             test_data=np.zeros((10, 4, 4), np.int64), test_idx=np.array([0, 10]))
    a = AttrDict(data_path=str(tok), vtokens=True, image_folder=True, sequence_length=2, resolution=4, spatial_length=4,
                 latent_shape=[2, 4, 4], batch_size=1, num_workers=0, packed_path=packs[16])
    with pytest.raises(ValueError, match="image_folder"):
        VideoData(a).train_dataloader()
