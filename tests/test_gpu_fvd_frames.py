"""The real side of FVD / KVD from a frame folder on MI355X: the uint8 output of the frame-ingest kernel (csrc/frames/frames.hip,
`mebt_op_frames_to_clip_u8`) against its numpy twin and the reference's FrameListDataset items, and both measure-FVD command lines
on a generated frame folder against the .npy route fed with the bytes the reference would embed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mebt_amd import frames as F
from mebt_amd import measure_fvd as M
from mebt_amd import measure_sliding_fvd as MS
from tests.helpers import write_tree
from tests.test_fvd_frames_host import CLIP_CASES, fvd_args, ref_bytes, reference_real_clips, seed, write_png_tree
from tests.test_gpu_fvd import closed_form_sd

DEV = "cuda"
SENTINEL = 0xA5


# ---- 4. kernel == twin ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,h,w,R", [(3, 5, 240, 320, 128),      # a real downscale, full tiles
                                       (2, 7, 33, 47, 17),         # partial tiles, odd R: rows of 51 bytes, frames off dword alignment
                                       (1, 3, 128, 96, 128),       # upscale
                                       (4, 2, 9, 9, 31),           # square source, upscale
                                       (2, 3, 200, 150, 64),       # portrait
                                       (2, 3, 16, 24, 16),         # crop side == R: the copy kernel
                                       (2, 3, 60, 80, 47),         # rows of 141 bytes: a tile's run of 2256 bytes starts off a dword
                                                                   # boundary in every other frame and takes three passes of the lanes
                                       (2, 3, 47, 47, 47)])        # the same odd frames of 6627 bytes through the copy kernel
def test_u8_kernel_matches_the_twin(B, T, h, w, R):
    rs = np.random.RandomState(B * 1000 + R)
    a = rs.randint(0, 256, (B, T, h, w, 3)).astype(np.uint8)
    out = F.frames_to_clip_u8(torch.from_numpy(a).to(DEV), R)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B, T, R, R, 3)
    ref = np.stack([F.clip_u8_twin(a[b], R) for b in range(B)])
    assert torch.equal(out.cpu(), torch.from_numpy(ref))


def test_u8_copy_kernel_off_dword_alignment():
    """crop side == R with odd R: every second frame of the output starts off a dword boundary"""
    a = np.random.RandomState(5).randint(0, 256, (2, 3, 13, 19, 3)).astype(np.uint8)
    out = F.frames_to_clip_u8(torch.from_numpy(a).to(DEV), 13)
    assert torch.equal(out.cpu(), torch.from_numpy(np.stack([F.clip_u8_twin(c, 13) for c in a])))


def test_u8_mixed_sizes_through_slots():
    """a mixed-size batch through collate_raw -> to_clip_u8(), then the same groups into a larger `out`: rows that no slot names, and
    the clip of a slot outside [0, Bout), are not written"""
    rs = np.random.RandomState(9)
    R, T = 17, 3
    sizes = [(20, 31), (17, 17), (20, 31), (40, 25), (17, 17)]
    items = [{"video": torch.from_numpy(rs.randint(0, 256, (T, h, w, 3)).astype(np.uint8)), "indices": torch.arange(2)} for h, w in sizes]
    ref = np.stack([F.clip_u8_twin(it["video"].numpy(), R) for it in items])
    raw = F.collate_raw(items, R)["video"]
    assert len(raw.groups) == 3
    got = raw.to(DEV).to_clip_u8()
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(ref))

    out = torch.full((8, T, R, R, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    where = {0: 6, 1: 1, 2: -1, 3: 4, 4: 9}                  # batch position -> row of `out`; -1 and 9 are outside [0, 8)
    for f, s in raw.groups:
        slots = torch.tensor([where[int(i)] for i in s], dtype=torch.int32, device=DEV)
        F.frames_to_clip_u8(f.to(DEV), R, out=out, slots=slots)
    out = out.cpu().numpy()
    for i, row in where.items():
        if 0 <= row < 8:
            assert np.array_equal(out[row], ref[i]), i
    for row in set(range(8)) - set(where.values()):
        assert (out[row] == SENTINEL).all(), row


def test_u8_argument_checks():
    x = torch.zeros(1, 2, 4, 4, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="uint8"):
        F.frames_to_clip_u8(x.float(), 4)
    with pytest.raises(ValueError, match="GPU"):
        F.frames_to_clip_u8(x.cpu(), 4)
    with pytest.raises(ValueError, match="out"):
        F.frames_to_clip_u8(x, 4, out=torch.zeros(1, 3, 2, 4, 4, device=DEV))          # the float clip is not the uint8 clip
    with pytest.raises(ValueError, match="slots"):
        F.frames_to_clip_u8(x, 4, slots=torch.zeros(1, dtype=torch.int32, device=DEV))


# ---- 5. kernel == the reference's items ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("frames"))
    return root, write_tree(root)


@pytest.mark.parametrize("tag,kw,train,s", CLIP_CASES, ids=[c[0] for c in CLIP_CASES])
def test_u8_raw_batches_equal_the_reference_bytes(tree, tag, kw, train, s):
    from mebt_amd.data import FrameListDataset
    root, d = tree
    ds = FrameListDataset(root, train=train, raw=True, **kw)
    seed(s)
    items = [ds[i] for i in range(len(ds))]
    batch = F.collate_raw(items, kw["resolution"])
    assert len(batch["video"].groups) > 1
    out = batch["video"].pin_memory().to(DEV, non_blocking=True).to_clip_u8().cpu()
    R, T = kw["resolution"], kw["sequence_length"]
    ref = ref_bytes(torch.from_numpy(d[f"{tag}__video"].reshape(len(items), 3, T, R, R)))
    assert torch.equal(out, ref)


# ---- 6 / 7. the command lines on a folder ---------------------------------------------------------------------------------------
SEED, T, R, N_SAMPLE = 31, 16, 32, 40


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """the 40-video tree, the closed-form I3D checkpoint, and measure_fvd's results on the folder"""
    tmp = tmp_path_factory.mktemp("fvd_frames")
    root = write_png_tree(str(tmp_path_factory.mktemp("png40")), 40, T + 2, seed=40)
    ck = str(tmp / "w.pt")
    torch.save(closed_form_sd(), ck)
    rng = np.random.default_rng(2)
    fake = str(tmp / "fake.npy")
    np.save(fake, rng.integers(0, 256, (64, T, R, R, 3), dtype=np.uint8))
    common = ["--n_sample", str(N_SAMPLE), "--sequence_length", str(T), "--resolution", str(R), "--num_workers", "0", "--i3d_ckpt", ck,
              "--i3d_dtype", "f32"]
    return dict(tmp=tmp, root=root, ck=ck, fake=fake, common=common, folder_args=["--data_path", root, "--image_folder", "--train"])


def test_measure_fvd_on_a_folder_equals_the_npy_route(folder, capsys):
    tmp, common = folder["tmp"], folder["common"]
    emb = str(tmp / "real_emb.npy")
    csv_path = tmp / "fake_consq_set_5.csv"
    seed(SEED)
    fvd, kvd = M.main(["--np_file", folder["fake"], "--real_embeddings", emb] + folder["folder_args"] + common)
    out = capsys.readouterr().out
    assert "Total num of videos: 40" in out and "computing fvd embeddings for real videos" in out and "warning" not in out
    lines = csv_path.read_text().splitlines()
    assert lines[0] == ",FVD,KVD" and lines[1] == f"0,{float(fvd)!r},{float(kvd)!r}"
    assert np.load(emb).shape == (N_SAMPLE, 400)

    # the .npy route on the bytes the reference would embed: main() draws from the generators in the order load_model (the I3D's
    # constructor initialises its weights from torch's generator), then the loader, so the replay does the same
    args = fvd_args(folder["root"], N_SAMPLE, T, R)
    seed(SEED)
    M.load_model(M.build_parser().parse_args(["--i3d_ckpt", folder["ck"], "--i3d_dtype", "f32"]), torch.device(DEV))
    clips = reference_real_clips(args)
    assert [len(c) for c in clips] == [32, 32]
    real = str(tmp / "real.npy")
    np.save(real, np.concatenate(clips)[:N_SAMPLE])
    csv_path.unlink()
    capsys.readouterr()
    fvd2, kvd2 = M.main(["--np_file", folder["fake"], "--data_path", real] + common)
    print(f"folder route FVD {fvd!r} KVD {kvd!r}; .npy route FVD {fvd2!r} KVD {kvd2!r}")
    assert abs(fvd - fvd2) <= 1e-9 * max(1.0, abs(fvd2)), (fvd, fvd2)
    assert abs(kvd - kvd2) <= 1e-9 * max(1.0, abs(kvd2)), (kvd, kvd2)
    assert csv_path.exists()

    # with the embeddings of the first call the folder is not opened
    csv_path.unlink()
    capsys.readouterr()
    fvd3, kvd3 = M.main(["--np_file", folder["fake"], "--real_embeddings", emb] + folder["folder_args"] + common)
    out = capsys.readouterr().out
    assert "loaded real embeddings" in out and "Total num of videos" not in out and "for real videos" not in out
    assert (fvd3, kvd3) == (fvd, kvd) and csv_path.exists()


def test_measure_sliding_fvd_on_a_folder(folder, capsys):
    tmp, common = folder["tmp"], folder["common"]
    first = tmp / "real_emb.npy"
    if not first.exists():                                    # run alone: the folder route of measure_fvd makes the file
        seed(SEED)
        M.main(["--np_file", folder["fake"], "--real_embeddings", str(first)] + folder["folder_args"] + common)
    long_fake = str(tmp / "long.npy")
    np.save(long_fake, np.random.default_rng(3).integers(0, 256, (32, 128, R, R, 3), dtype=np.uint8))
    emb = str(tmp / "real_emb_sliding.npy")
    capsys.readouterr()
    seed(SEED)
    rows = MS.main(["--np_file", long_fake, "--slide", "56", "--real_embeddings", emb] + folder["folder_args"] + common)
    assert "Total num of videos: 40" in capsys.readouterr().out
    assert [r[0] for r in rows] == [0, 56] and all(np.isfinite(r[1]) and np.isfinite(r[2]) for r in rows)
    lines = (tmp / f"long_slide56_clip{T}_5.csv").read_text().splitlines()
    assert lines[0] == ",t,fvd,kvd" and len(lines) == 3
    assert [ln.split(",")[:2] for ln in lines[1:]] == [["0", "0"], ["1", "56"]]
    assert np.array_equal(np.load(emb), np.load(str(first)))
