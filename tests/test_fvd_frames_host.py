"""The real side of FVD / KVD from a frame folder, on the CPU: the byte table of the reference's `((video + 0.5) * 255).byte()`, the
numpy twin of the uint8 ingest against the reference's own FrameListDataset items (tests/golden/frames/frames_data.npz), and which
batches `measure_fvd.real_batches` takes (reference measure_fvd_with_numpy.py:55-67) on generated PNG trees."""
import os
import random

import numpy as np
import pytest
import torch

from mebt_amd import frames as F
from mebt_amd import measure_fvd as M
from tests.helpers import write_tree
from tests.test_frames_host import CASES

CLIP_CASES = [c for c in CASES if c[1]["sequence_length"] > 0]
SIZES = [(12, 16), (15, 10)]          # source sizes (h, w) of the generated trees: landscape and portrait, mixed in every batch


def ref_bytes(video):
    """the reference's real clip (measure_fvd_with_numpy.py:63): float [..., 3, T, R, R] -> uint8 [..., T, R, R, 3]"""
    return ((video + 0.5) * 255).movedim(-4, -1).byte()


def write_png_tree(root, videos, frames, seed=0):
    """`videos` videos of `frames` random tiny frames each, sizes alternating over SIZES, listed in train.txt and test.txt; one
    more video is written because the loader never flushes the last one of a list"""
    from PIL import Image
    rs = np.random.RandomState(seed)
    paths = []
    for v in range(videos + 1):
        h, w = SIZES[v % len(SIZES)]
        for k in range(frames):
            p = os.path.join(root, f"v{v:03d}_{k + 1:04d}.png")          # zero-padded: the list is sorted as strings
            Image.fromarray(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(p)
            paths.append(p)
    for lst in ("train.txt", "test.txt"):
        with open(os.path.join(root, lst), "w") as f:
            f.write("\n".join(paths) + "\n")
    return root


def fvd_args(root, n_sample, sequence_length, resolution, extra=()):
    """the namespace `measure_fvd.main` hands to `real_embeddings` for a folder run"""
    args = M.build_parser().parse_args(["--data_path", str(root), "--image_folder", "--train", "--n_sample", str(n_sample),
                                        "--sequence_length", str(sequence_length), "--resolution", str(resolution),
                                        "--num_workers", "0", *extra])
    args.batch_size = 32
    return args


def reference_real_clips(args):
    """the reference's real loop on this project's float loader (PIL in the dataset, as the reference): the uint8 clips
    [N, T, R, R, 3] it would embed, batch by batch, before the cut to n_sample"""
    from mebt_amd.config import AttrDict
    from mebt_amd.data import VideoData
    data = VideoData(AttrDict(vars(args)), True, raw=False)
    loader = data.train_dataloader() if args.train else data.val_dataloader()
    out = []
    while True:
        for batch in loader:
            if batch["video"].shape[0] % 16 == 0:
                out.append(ref_bytes(batch["video"]).numpy())
            if len(out) * args.batch_size >= args.n_sample:
                return out


def twin_batch(raw, R):
    """clip_u8_twin of every clip of a RawVideoBatch, in batch order"""
    out = [None] * len(raw)
    for f, s in raw.groups:
        for clip, slot in zip(f.numpy(), s.tolist()):
            out[slot] = F.clip_u8_twin(clip, R)
    return np.stack(out)


def seed(s):
    random.seed(s)
    torch.manual_seed(s)


# ---- 1. byte table ----------------------------------------------------------------------------------------------------------
def test_byte_table_is_the_reference_expression():
    t = F.byte_table()
    assert t.dtype == np.uint8 and t.shape == (256,)
    for u in range(256):
        img = np.full((1, 1, 3), u, np.uint8)
        x = np.asarray(img, dtype=np.float32)            # FrameListDataset.getTensor
        x /= 255.
        video = torch.from_numpy(x - 0.5)
        assert t[u] == int(((video + 0.5) * 255).byte()[0, 0, 0]), u
    ident = np.arange(256)
    moved = int((t != ident).sum())
    print(f"byte table: {moved} of 256 levels differ from the identity")
    assert moved > 0
    assert np.abs(t.astype(np.int64) - ident).max() == 1
    assert moved == 63                                    # IEEE float32 arithmetic and a truncation: the same on every host


# ---- 2. twin against the reference's items --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL")
    root = str(tmp_path_factory.mktemp("frames"))
    return root, write_tree(root)


@pytest.mark.parametrize("tag,kw,train,s", CLIP_CASES, ids=[c[0] for c in CLIP_CASES])
def test_twin_equals_the_reference_bytes(tree, tag, kw, train, s):
    from mebt_amd.data import FrameListDataset
    root, d = tree
    ds = FrameListDataset(root, train=train, raw=True, **kw)
    seed(s)
    items = [ds[i] for i in range(len(ds))]
    R, T = kw["resolution"], kw["sequence_length"]
    ref = ref_bytes(torch.from_numpy(d[f"{tag}__video"].reshape(len(items), 3, T, R, R))).numpy()
    assert ref.shape == (len(items), T, R, R, 3)
    got = np.stack([F.clip_u8_twin(it["video"].numpy(), R) for it in items])
    assert got.dtype == np.uint8 and np.array_equal(got, ref)
    floats = np.stack([F.clip_twin(it["video"].numpy(), R) for it in items])
    assert not np.array_equal(got, np.rint((floats + 0.5) * 255).transpose(0, 2, 3, 4, 1))     # the table is not PIL's bytes


# ---- 3. batch selection -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    pytest.importorskip("PIL")
    return {n: write_png_tree(str(tmp_path_factory.mktemp(f"png{n}")), n, 6, seed=n) for n in (40, 48, 10)}


def test_real_batches_two_passes(trees, capsys):
    """40 videos, n_sample 40: 32 (+ a skipped 8) in the first pass, 32 in the second, and 2 x 32 >= 40 stops the walk"""
    args = fvd_args(trees[40], 40, 4, 8)
    seed(21)
    raw = list(M.real_batches(args))
    assert [len(b) for b in raw] == [32, 32]
    assert all(isinstance(b, F.RawVideoBatch) and len(b.groups) == 2 for b in raw)
    assert "warning" not in capsys.readouterr().out
    seed(21)
    ref = reference_real_clips(args)
    assert [len(b) for b in ref] == [32, 32]
    for a, b in zip(raw, ref):
        assert np.array_equal(twin_batch(a, 8), b)
    assert not np.array_equal(ref[0], ref[1])                # the second pass is a new shuffle with new start frames


def test_real_batches_count_a_batch_of_16_as_32(trees, capsys):
    """48 videos, n_sample 64: batches of 32 and 16 are used, 2 x 32 >= 64 stops after one pass with 48 clips"""
    args = fvd_args(trees[48], 64, 4, 8)
    seed(22)
    raw = list(M.real_batches(args))
    assert [len(b) for b in raw] == [32, 16]
    out = capsys.readouterr().out
    assert "warning" in out and "48" in out and "64" in out
    seed(22)
    ref = reference_real_clips(args)
    assert sum(len(b) for b in ref) == 48
    for a, b in zip(raw, ref):
        assert np.array_equal(twin_batch(a, 8), b)


def test_real_batches_test_list_and_exits(trees, tmp_path):
    args = fvd_args(trees[10], 40, 4, 8)
    with pytest.raises(SystemExit, match="16"):              # 10 videos: no batch is ever a multiple of 16
        list(M.real_batches(args))
    args = fvd_args(trees[40], 40, -1, 8)
    with pytest.raises(SystemExit, match="sequence_length"):
        list(M.real_batches(args))
    args = fvd_args(trees[40], 32, 4, 8)
    args.train = False                                       # the test list, through val_dataloader
    seed(23)
    assert [len(b) for b in M.real_batches(args)] == [32]


def test_real_side_choice(trees, tmp_path):
    """a frame folder needs --image_folder and the list file of the chosen split; anything else falls through to the .npy route or
    the message that names all three options"""
    args = fvd_args(trees[40], 40, 4, 8)
    assert M.frame_folder(args)
    args.image_folder = False
    assert not M.frame_folder(args)
    os.remove(os.path.join(str(write_png_tree(str(tmp_path), 1, 1)), "test.txt"))
    args = fvd_args(tmp_path, 40, 4, 8)
    assert M.frame_folder(args)
    args.train = False
    assert not M.frame_folder(args)
    with pytest.raises(SystemExit) as e:
        M.real_embeddings(args, None, "cpu")
    assert all(w in str(e.value) for w in ("--real_embeddings", "--image_folder", ".npy"))
