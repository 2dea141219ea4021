"""FVD / KVD, host side (no GPU): the I3D parameter tree against the reference's state dict, the float64 statistics against the
reference's scalars (tests/golden/fvd/fvd_golden.npz), the launch plan's TF-"same" geometry against the reference's endpoint
shapes, the measure-FVD command lines of the reference's driver scripts, their CSV output, and the profiled-sources fingerprint."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "fvd")
REF = os.environ.get("MEBT_REFERENCE", "/root/reference")
sys.path.insert(0, GOLD)

from mebt_amd import fvd as FV  # noqa: E402
from mebt_amd import i3d as I  # noqa: E402
from mebt_amd import measure_fvd as MF  # noqa: E402

FVD_REL_TOL = 1e-9           # vs the reference's functions on float64 tensors (measured ~1e-13)
FVD_F32_REL_TOL = 1e-3       # vs the reference as its scripts call it, on float32 tensors (measured 5.3e-4: its float32 SVD)


def golden():
    return np.load(os.path.join(GOLD, "i3d_golden.npz"))


def golden_shapes():
    g = golden()
    return {str(k): tuple(int(x) for x in s if x >= 0) for k, s in zip(g["sd_keys"], g["sd_shapes"])}


def test_state_dict_keys_and_shapes_match_the_reference():
    sd = I.InceptionI3d(400, in_channels=3).state_dict()
    assert len(sd) == 344
    assert {k: tuple(v.shape) for k, v in sd.items()} == golden_shapes()


def test_closed_form_state_dict_loads_strict():
    from make_golden_fvd import closed_form_state_dict
    m = I.InceptionI3d(400, in_channels=3)
    res = m.load_state_dict(closed_form_state_dict(golden_shapes()), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert m._prepared is None
    assert abs(float(m.Mixed_3b.b1a.bn.running_var.min()) - 0.75) < 0.05


def test_frechet_distance_and_polynomial_mmd_match_the_reference():
    g = np.load(os.path.join(GOLD, "fvd_golden.npz"))
    fd = FV.frechet_distance(g["emb1"], g["emb2"])
    kd = FV.polynomial_mmd(g["emb1"], g["emb2"])
    assert abs(fd - float(g["fvd"])) <= FVD_REL_TOL * abs(float(g["fvd"])), (fd, float(g["fvd"]))
    assert abs(fd - float(g["fvd_f32"])) <= FVD_F32_REL_TOL * abs(float(g["fvd_f32"])), (fd, float(g["fvd_f32"]))
    assert abs(kd - float(g["kvd"])) <= FVD_REL_TOL * abs(float(g["kvd"])), (kd, float(g["kvd"]))
    assert FV.frechet_distance(torch.from_numpy(g["emb1"]), torch.from_numpy(g["emb1"])) < 1e-6 * float(g["fvd"])


def test_matrix_square_root_keeps_tiny_singular_values():
    """the reference's where(s < eps, s, sqrt(s)): singular values below 1e-10 pass through unrooted"""
    m = np.diag([4.0, 1e-12])
    assert np.allclose(FV._symmetric_matrix_square_root(m), np.diag([2.0, 1e-12]), rtol=0, atol=1e-15)


@pytest.mark.parametrize("tag,T", [("a", 16), ("b", 12)])
def test_launch_plan_matches_reference_endpoint_shapes(tag, T):
    g = golden()
    plan = I.launch_plan(T)
    names = [str(n) for n in g[f"endpoints_{tag}"]]
    assert [e["endpoint"] for e in plan[:-1]] == names
    for e, shp in zip(plan, g[f"endpoint_shapes_{tag}"]):
        assert (e["cout"],) + tuple(e["out_dims"]) == tuple(int(x) for x in shp), e["endpoint"]
    assert plan[-1]["out_dims"] == (1, 1, 1)


def test_same_padding_is_asymmetric():
    assert I.same_pad(6, 3, 2) == (0, 1, 3)           # even size, stride 2: pad 1 at the back
    assert I.same_pad(3, 3, 2) == (1, 1, 2)           # odd size: pad 2
    assert I.same_pad(224, 7, 2) == (2, 3, 112)       # Conv3d_1a
    assert I.same_pad(3, 2, 2) == (0, 1, 2)           # MaxPool3d_5a at T = 12 (3 -> 2)


def test_plan_flops_match_the_shape_table():
    assert abs(I.plan_flops(16) / 1e9 - 55.6) < 0.05


def _script_command_lines():
    lines = []
    for f in sorted(os.listdir(os.path.join(REF, "scripts"))):
        if f.startswith("valid_dnr_"):
            txt = open(os.path.join(REF, "scripts", f)).read().replace("\\\n", " ")
            lines += [ln.split("measure_fvd_with_numpy.py", 1)[1] for ln in txt.splitlines() if "measure_fvd_with_numpy.py" in ln]
    return lines


def test_reference_script_command_lines_parse():
    if not os.path.isdir(REF):
        pytest.skip("reference tree not available")
    lines = _script_command_lines()
    assert len(lines) >= 12
    for ln in lines:
        argv = re.sub(r"\$\{?\w+\}?", "X", re.sub(r"\$\{?LENGTH\}?", "16", ln)).split()
        a = MF.build_parser().parse_args(argv)
        assert a.compute_fvd and a.image_folder and a.np_file.endswith(".npy")
        assert a.i3d_dtype == "f16" and a.real_embeddings == ""
    a = MF.build_parser(sliding=True).parse_args(["--np_file", "x.npy", "--slide", "4", "--sequence_length", "16"])
    assert a.slide == 4 and a.n_sample == 512


def test_csv_names_match_the_reference():
    assert MF.consq_csv_name("results/e/VID_run0.npy", 5) == "results/e/VID_run0_consq_set_5.csv"
    assert MF.sliding_csv_name("results/e/VID.npy", 8, 16, 5) == "results/e/VID_slide8_clip16_5.csv"


def test_csv_text_equals_pandas_to_csv(tmp_path):
    pd = pytest.importorskip("pandas")
    rows = [[0, 123.45678901234, 0.0012345678], [8, 1e-05, 3.0]]
    MF.write_csv(tmp_path / "a.csv", ["t", "fvd", "kvd"], rows)
    df = pd.DataFrame({"t": [r[0] for r in rows], "fvd": [r[1] for r in rows], "kvd": [r[2] for r in rows]})
    assert (tmp_path / "a.csv").read_text() == df.to_csv()
    MF.write_csv(tmp_path / "b.csv", ["FVD", "KVD"], [[np.float64(812.5), 0.25]])
    assert (tmp_path / "b.csv").read_text() == pd.DataFrame({"FVD": [812.5], "KVD": [0.25]}).to_csv()


def test_missing_checkpoint_names_all_three_places(tmp_path, monkeypatch):
    monkeypatch.setenv("MEBT_I3D_CKPT", str(tmp_path / "nope.pt"))
    monkeypatch.setattr(FV, "DEFAULT_CKPT", str(tmp_path / "default.pt"))
    with pytest.raises(FileNotFoundError) as e:
        FV.load_fvd_model("cpu", path=str(tmp_path / "given.pt"))
    msg = str(e.value)
    assert "given.pt" in msg and "nope.pt" in msg and "default.pt" in msg


def test_network_has_no_cpu_path():
    m = I.InceptionI3d(400)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(torch.zeros(1, 3, 16, 224, 224))


def test_real_side_rejects_a_dataset_directory(tmp_path):
    a = MF.build_parser().parse_args(["--np_file", "f.npy", "--data_path", str(tmp_path)])
    with pytest.raises(SystemExit, match=r"\.npy of real clips"):
        MF.real_embeddings(a, None, "cpu")


def test_csrc_fingerprint_unchanged():
    from mebt_amd.launch import csrc_fingerprint
    with open(os.path.join(ROOT, "profiles", "r06_pmc_traffic.json")) as f:
        assert csrc_fingerprint() == json.load(f)["_csrc_sha256"]


def test_golden_fvd_fixtures_regenerate_bit_identically(tmp_path):
    if not os.path.isdir(REF):
        pytest.skip("reference tree not available")
    env = dict(os.environ, MEBT_GOLDEN_OUT=str(tmp_path))
    out = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_fvd.py")], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    for f in ("i3d_golden.npz", "fvd_golden.npz"):
        a, b = np.load(os.path.join(tmp_path, f)), np.load(os.path.join(GOLD, f))
        assert sorted(a.files) == sorted(b.files), f
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (f, k)
