#!/usr/bin/env python3
"""Generate the frame-ingest fixtures (tests/golden/frames/*.npz) by running the reference's own FrameListDataset.

Needs the reference tree (REF below) and Pillow; it is never run by the tests.  The reference's mebt/data.py imports
h5py, torchvision and pytorch_lightning at module level: only those third-party modules are stubbed (empty stand-ins,
as tests/golden/make_golden.py:gen_data_contract does), the dataset logic and PIL are the real ones.

frames_data.npz     the synthetic PNG tree (names, shapes, pixels, list files) and the reference items (`video`, `indices`)
                    for several dataset settings under fixed `random` / `torch` seeds
frames_resize.npz   PIL crop + Image.resize(BILINEAR) outputs for a table of (Hs, Ws, R); the inputs are
                    np.random.RandomState(seed).randint(0, 256, (Hs, Ws, 3)) and are rebuilt by the tests

Usage:  python tests/golden/frames/make_golden_frames.py
"""
import contextlib
import io
import os
import random
import shutil
import sys
import tempfile
import types

sys.dont_write_bytecode = True
REF = os.environ.get("MEBT_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np
import torch
from PIL import Image

# the synthetic tree: (list name, frame numbers, (h, w)); list entries are written unsorted on purpose
VIDEOS = [
    ("walk", list(range(1, 13)), (12, 20)),          # 1, 10, 11, 12, 2 .. 9 in string order: two breaks
    ("pan_cam", list(range(1, 6)) + list(range(7, 12)), (20, 12)),   # a missing frame 6; '_' inside the video id
    ("d1/jump", list(range(1, 8)), (16, 16)),        # a sub-directory; crop side == R
    ("tall", list(range(1, 8)), (24, 16)),           # crop side == R, but h != R: the reference still calls resize
    ("tiny", [1, 2], (10, 14)),                      # too short: dropped
    ("skip", list(range(1, 9)), (30, 30)),           # a listed non-image entry is spliced in (skip_4.json)
    ("zz_last", list(range(1, 8)), (14, 18)),        # the last video of the list: never flushed
]
TEST_VIDEOS = [("t_a", list(range(1, 7)), (18, 24)), ("t_b", list(range(1, 9)), (16, 16)), ("t_c", [1, 2, 3], (8, 8))]
EXTRA = {"skip": "skip_4.json"}

CASES = [  # tag, kwargs, train, seed
    ("s4r16", dict(sequence_length=4, resolution=16, sample_every_n_frames=1, latent_shape=[1, 4, 4]), True, 11),
    ("s3e2r16", dict(sequence_length=3, resolution=16, sample_every_n_frames=2, latent_shape=[1, 2, 2]), True, 12),
    ("whole", dict(sequence_length=-1, resolution=12, sample_every_n_frames=1, latent_shape=[2, 3]), True, 13),
    ("test_s4r10", dict(sequence_length=4, resolution=10, sample_every_n_frames=1, latent_shape=[4]), False, 14),
]

RESIZE = [(240, 320, 128), (128, 128, 128), (128, 256, 128), (256, 128, 128), (7, 9, 5), (9, 7, 5), (64, 64, 128), (100, 60, 33),
          (31, 17, 16), (5, 5, 17), (480, 640, 128), (720, 1280, 128), (1080, 1920, 128), (256, 200, 256), (3, 2, 64)]


def import_reference_data():
    for name, path in (("mebt", [f"{REF}/mebt"]),):
        m = types.ModuleType(name)
        m.__path__ = path
        sys.modules[name] = m
    h5 = types.ModuleType("h5py")
    h5.File = None
    sys.modules["h5py"] = h5
    for name in ("torchvision", "torchvision.datasets", "torchvision.datasets.video_utils"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision.datasets.video_utils"].VideoClips = object
    pl = types.ModuleType("pytorch_lightning")
    pl.LightningDataModule = object
    sys.modules["pytorch_lightning"] = pl
    import importlib
    return importlib.import_module("mebt.data")


def frame_names(videos, extra=True):
    names = []
    for vid, nums, _ in videos:
        for k in nums:
            names.append(f"{vid}_{k}.png")
        if extra and vid in EXTRA:
            names.append(os.path.join(os.path.dirname(vid), EXTRA[vid]))
    return names


def write_tree(root, rs):
    """PNG files plus the list files; returns (names, shapes, pixels) of every PNG"""
    names, shapes, pix = [], [], []
    for videos in (VIDEOS, TEST_VIDEOS):
        for vid, nums, (h, w) in videos:
            for k in nums:
                a = rs.randint(0, 256, (h, w, 3), dtype=np.uint8)
                n = f"{vid}_{k}.png"
                os.makedirs(os.path.dirname(os.path.join(root, n)), exist_ok=True)
                Image.fromarray(a).save(os.path.join(root, n))
                names.append(n); shapes.append((h, w, 3)); pix.append(a.reshape(-1))
    for n in EXTRA.values():
        open(os.path.join(root, n), "w").write("{}")
    train = frame_names(VIDEOS)
    test = frame_names(TEST_VIDEOS)
    rs.shuffle(train)
    rs.shuffle(test)
    for fn, lst in (("train.txt", train), ("test.txt", test)):
        with open(os.path.join(root, fn), "w") as f:
            f.write("\n".join(os.path.join(root, n) for n in lst) + "\n")
    return names, np.array(shapes, np.int32), np.concatenate(pix), train, test


def gen_data(data_mod):
    root = tempfile.mkdtemp(prefix="frames_golden_")
    try:
        names, shapes, pix, train, test = write_tree(root, np.random.RandomState(5))
        out = dict(names=np.array(names), shapes=shapes, pixels=pix, train_list=np.array(train), test_list=np.array(test))
        for tag, kw, is_train, seed in CASES:
            log = io.StringIO()
            with contextlib.redirect_stdout(log):
                ds = data_mod.FrameListDataset(root, train=is_train, **kw)
            out[f"{tag}__discontinuous"] = np.array(int(log.getvalue().split("discontinuous videos:")[1].split()[0]))
            random.seed(seed)
            torch.manual_seed(seed)
            vids, perms, lens = [], [], []
            for i in range(len(ds)):
                it = ds[i]
                v = it["video"].numpy()
                vids.append(np.ascontiguousarray(v).reshape(-1)); lens.append(v.shape[1]); perms.append(it["indices"].numpy())
            out[f"{tag}__first_frames"] = np.array([os.path.relpath(v[0], root) for v in ds.data_all])
            out[f"{tag}__video_lens"] = np.array([len(v) for v in ds.data_all], np.int32)
            out[f"{tag}__T"] = np.array(lens, np.int32)
            out[f"{tag}__video"] = np.concatenate(vids).astype(np.float32)
            out[f"{tag}__indices"] = np.stack(perms).astype(np.int64)
        np.savez_compressed(os.path.join(HERE, "frames_data.npz"), **out)
    finally:
        shutil.rmtree(root)


def gen_resize():
    out = {"table": np.array(RESIZE, np.int32)}
    for i, (h, w, R) in enumerate(RESIZE):
        a = np.random.RandomState(1000 + i).randint(0, 256, (h, w, 3)).astype(np.uint8)
        img = Image.fromarray(a)
        if h > w:
            half = (h - w) // 2
            img = img.crop((0, half, w, half + w))
        elif w > h:
            half = (w - h) // 2
            img = img.crop((half, 0, half + h, h))
        if h != R or w != R:
            img = img.resize((R, R), Image.BILINEAR)
        out[f"out_{i}"] = np.asarray(img, dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "frames_resize.npz"), **out)


if __name__ == "__main__":
    gen_data(import_reference_data())
    gen_resize()
    for f in ("frames_data.npz", "frames_resize.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)))
