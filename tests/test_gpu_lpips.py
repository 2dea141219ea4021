"""LPIPS on MI355X: the four operators of csrc/lpips/lpips.hip against their float64 twins, the whole network against the real reference's
golden figures (tests/golden/lpips), frame selection, `VQGAN.validation_step` / `reconstruct_stats` with perceptual weights and the
`python -m mebt_amd.measure_recon --lpips` command.  GPU only.

Bounds.  conv2d_3x3: with S = sum |a| |w| + |bias| taken by the float64 twin on the operands as the kernel sees them (rounded to fp16
first in fp16 mode), every output lies within K * 2^-23 * S of the twin, K = 9 Cin: the standard bound (K + 1) u S of a K-term fp32 sum
plus the bias add, u = 2^-24, with K + 1 <= 2 K; ReLU does not increase a difference.  fp16 mode adds the store's rounding, 2^-11 |y|, and
2^-25 for results in fp16's subnormal range.  The same prepared weights through mebt_op_i3d_conv, an independent kernel, meet the same
bound.  maxpool_2x2 and lpips_input are exact.  lpips_head: a lane adds at most 8 fp32 terms between butterflies of 6 levels, twice, so
about 30 roundings of 6e-8 sit on a value: gate 2 x the measured deviation and never above 1e-4 (the gate of the sibling recon sums).
Whole network, fp32: 1e-4 relative against the reference's own numbers (recon_golden's gate; measured figures in
profiles/lpips_parity_measured.txt); fp16: 2 x the measured worst relative deviation over the four golden cases."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lpips")
sys.path.insert(0, GOLD)

from make_golden_lpips import CASES, closed_form_state_dict, to_input  # noqa: E402
from mebt_amd import _lib, recon  # noqa: E402
from mebt_amd import lpips as LP  # noqa: E402
from mebt_amd import measure_recon as MR  # noqa: E402
from oracle import vqgan_oracle as vq  # noqa: E402
from tests.golden import make_golden as mg  # noqa: E402
from tests.helpers import record_measured, tiny_vqgan  # noqa: E402

DEV = "cuda"
REF_GATE = 1e-4              # fp32 network against the reference's golden numbers
HEAD_MEASURED = {"f32": 6.6e-8, "f16": 1.3e-7}          # worst relative deviation of lpips_head from its twin on one MI355X run
F16_MEASURED = 2.44e-4       # worst relative deviation of the fp16 network from the golden values over the four cases, same run


def record(name, value, gate):
    record_measured("lpips " + name, value, gate)


def tdt(dtype):
    return torch.float16 if dtype == "f16" else torch.float32


@pytest.fixture(scope="module")
def sd():
    return closed_form_state_dict()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "lpips_golden.npz"))


# ---- conv2d_3x3 -------------------------------------------------------------------------------------------------------------------------
CONV_CASES = [(32, 64, 1, 1, 1), (32, 64, 2, 5, 7), (32, 64, 1, 17, 33), (32, 64, 3, 16, 16), (3, 64, 2, 16, 16), (3, 64, 1, 17, 33),
              (64, 128, 2, 9, 9), (512, 512, 2, 4, 4)]
_conv_cache = {}


def conv_case(cin, cout, N, H, W, dtype):
    """operands as the kernel sees them and the float64 twin with its bound, computed once per case"""
    key = (cin, cout, N, H, W, dtype)
    if key not in _conv_cache:
        g = torch.Generator().manual_seed(cin * 1000 + H * 10 + W)
        x = torch.randn(N, H, W, cin, generator=g).to(tdt(dtype))
        w = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(tdt(dtype))
        b = torch.randn(cout, generator=g) * 0.1
        xd, wd, bd = x.double().permute(0, 3, 1, 2), w.double(), b.double()
        pre = F.conv2d(xd, wd, bd, padding=1)
        S = F.conv2d(xd.abs(), wd.abs(), bd.abs(), padding=1)
        y = F.relu(pre).permute(0, 2, 3, 1).contiguous()
        bound = 9 * cin * 2.0 ** -23 * S.permute(0, 2, 3, 1)
        if dtype == "f16":
            bound = bound + 2.0 ** -11 * y.abs() + 2.0 ** -25
        _conv_cache[key] = (x, w, b, y, bound.contiguous())
    return _conv_cache[key]


def run_conv(x, w, b, dtype, fn=LP.conv2d_3x3):
    cout, cin = int(w.shape[0]), int(w.shape[1])
    xd = x.to(DEV).contiguous()
    wa = LP.arrange_weight(w.to(DEV), tdt(dtype))
    out = torch.full((*x.shape[:3], cout), float("nan"), device=DEV, dtype=tdt(dtype))
    fn(xd, wa, b.to(DEV), out, cin, cout, dtype)
    return out


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("cin,cout,N,H,W", CONV_CASES)
def test_conv2d_3x3_vs_twin(cin, cout, N, H, W, dtype):
    x, w, b, y, bound = conv_case(cin, cout, N, H, W, dtype)
    out = run_conv(x, w, b, dtype)
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    ratio = ((got - y).abs() / bound).max().item()
    print(f"[conv2d_3x3 {dtype} {cin}->{cout} {N}x{H}x{W}] max |kernel - twin| / bound {ratio:.3f}, max abs {(got - y).abs().max().item():.2e}")
    record(f"conv2d_3x3[{dtype} {cin}->{cout} {N}x{H}x{W}] err / bound", ratio, 1.0)
    assert ratio <= 1.0
    assert torch.equal(run_conv(x, w, b, dtype), out)                            # bit-identical run to run
    if N > 1:                                                                   # image 0 alone: the same bits as inside the batch
        assert torch.equal(run_conv(x[:1], w, b, dtype)[0], out[0])


@pytest.mark.parametrize("cin,cout,N,H,W", CONV_CASES)
def test_i3d_conv_on_the_same_weights_meets_the_same_bound(cin, cout, N, H, W):
    x, w, b, y, bound = conv_case(cin, cout, N, H, W, "f32")
    got = run_conv(x, w, b, "f32", fn=LP.conv2d_3x3_i3d).cpu().double()
    ratio = ((got - y).abs() / bound).max().item()
    record(f"i3d_conv as 3x3[f32 {cin}->{cout} {N}x{H}x{W}] err / bound", ratio, 1.0)
    assert ratio <= 1.0
    own = run_conv(x, w, b, "f32").cpu().double()
    assert ((own - got).abs() <= 2 * bound).all()


def test_conv2d_3x3_argument_checks():
    lib = _lib.load()
    x = torch.zeros(1, 4, 4, 32, device=DEV)
    w = torch.zeros(64, 288, device=DEV)
    out = torch.full((1, 4, 4, 64), -7.0, device=DEV)
    s = _lib.cur_stream()
    calls = {
        "Cin": lambda: lib.mebt_op_conv2d_3x3(_lib.F32, _lib.ptr(x), _lib.ptr(w), None, _lib.ptr(out), 1, 4, 4, 5, 64, 1, s),
        "Cin ": lambda: lib.mebt_op_conv2d_3x3(_lib.F32, _lib.ptr(x), _lib.ptr(w), None, _lib.ptr(out), 1, 4, 4, 544, 64, 1, s),
        "null pointer": lambda: lib.mebt_op_conv2d_3x3(_lib.F32, None, _lib.ptr(w), None, _lib.ptr(out), 1, 4, 4, 32, 64, 1, s),
        "null pointer ": lambda: lib.mebt_op_conv2d_3x3(_lib.F32, _lib.ptr(x), None, None, _lib.ptr(out), 1, 4, 4, 32, 64, 1, s),
        "null pointer  ": lambda: lib.mebt_op_conv2d_3x3(_lib.F32, _lib.ptr(x), _lib.ptr(w), None, None, 1, 4, 4, 32, 64, 1, s),
        "dtype": lambda: lib.mebt_op_conv2d_3x3(_lib.BF16, _lib.ptr(x), _lib.ptr(w), None, _lib.ptr(out), 1, 4, 4, 32, 64, 1, s),
        "need N": lambda: lib.mebt_op_conv2d_3x3(_lib.F32, _lib.ptr(x), _lib.ptr(w), None, _lib.ptr(out), 0, 4, 4, 32, 64, 1, s),
        "aligned": lambda: lib.mebt_op_conv2d_3x3(_lib.F32, _lib.ptr(x) + 4, _lib.ptr(w), None, _lib.ptr(out), 1, 4, 4, 32, 64, 1, s),
    }
    for what, call in calls.items():
        assert call() != 0, what
        assert what.strip() in lib.mebt_last_error().decode(), (what, lib.mebt_last_error())
    torch.cuda.synchronize()
    assert (out == -7.0).all()


# ---- maxpool_2x2 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("H,W", [(9, 9), (5, 2), (16, 16), (2, 3)])
def test_maxpool_2x2_is_exact(H, W, dtype):
    g = torch.Generator().manual_seed(H * 17 + W)
    for Cc in (16, 3):                                                          # the 16-byte path and the element path
        x = (torch.randn(2, H, W, Cc, generator=g) - 0.5).to(tdt(dtype))
        out = torch.full((2, H // 2, W // 2, Cc), float("nan"), device=DEV, dtype=tdt(dtype))
        LP.maxpool_2x2(x.to(DEV), out, dtype)
        ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).to(tdt(dtype))
        assert (x < 0).any() and torch.equal(out.cpu(), ref), (H, W, Cc)


def test_maxpool_2x2_needs_two_rows():
    x = torch.zeros(1, 1, 4, 8, device=DEV)
    out = torch.full((1, 1, 2, 8), -7.0, device=DEV)
    with pytest.raises(_lib.MebtError, match="H >= 2"):
        LP.maxpool_2x2(x, out, "f32")
    with pytest.raises(_lib.MebtError, match="W >= 2"):
        LP.maxpool_2x2(x.view(1, 4, 1, 8), out, "f32")
    torch.cuda.synchronize()
    assert (out == -7.0).all()


# ---- lpips_head -----------------------------------------------------------------------------------------------------------------------------
def run_head(f, w, n, P, Cc, dtype, out=None, layer=False):
    out = torch.zeros(n, device=DEV, dtype=torch.float64) if out is None else out
    scratch = torch.empty(max(1, LP.head_scratch_bytes(n, P) // 8), device=DEV, dtype=torch.float64)
    lay = torch.full((n, 5), -1.0, device=DEV, dtype=torch.float64) if layer else None
    LP.lpips_head(f, w, out, n, P, Cc, scratch, None if lay is None else lay[:, 3], 5, dtype)
    return out, lay


@pytest.mark.parametrize("dtype", ["f32", "f16"])
# (1, 4113): 258 workgroups per pair, more slots than the finishing kernel has threads and no multiple of them
@pytest.mark.parametrize("Cc,P", [(64, 1), (64, 7), (64, 300), (512, 1), (512, 7), (512, 300), (1, 257 * LP.HEAD_ROWS + 1)])
def test_lpips_head_vs_twin(Cc, P, dtype):
    n = 3
    g = torch.Generator().manual_seed(Cc + P)
    f = torch.relu(torch.randn(2 * n, P, Cc, generator=g)).to(tdt(dtype))
    f[0, 0] = 0                                                                  # a zero vector on one side ...
    f[n + 1, P - 1] = 0
    f[2, P // 2] = 0                                                             # ... and on both
    f[n + 2, P // 2] = 0
    w = torch.rand(Cc, generator=g) * 4 / Cc
    fd = f.double().permute(0, 2, 1).unsqueeze(-1)                              # [2n, C, P, 1]
    ref = LP.head_twin(fd[:n], fd[n:], w.double())
    fg, wg = f.to(DEV), w.to(DEV)
    out, lay = run_head(fg, wg, n, P, Cc, dtype, layer=True)
    assert torch.isfinite(out).all() and out.dtype == torch.float64
    some = ref > 0                                                              # P = 1: pair 2 is zero against zero, exactly 0
    assert some[:2].all() and (out.cpu()[~some] == 0).all()
    err = ((out.cpu() - ref).abs()[some] / ref[some]).max().item()
    gate = min(2 * HEAD_MEASURED[dtype], 1e-4)
    print(f"[lpips_head {dtype} C={Cc} P={P}] max rel err {err:.2e} (gate {gate:.1e})")
    record(f"lpips_head[{dtype} C={Cc} P={P}] rel", err, gate)
    assert err <= gate
    assert torch.equal(lay[:, 3], out) and (lay[:, [0, 1, 2, 4]] == -1.0).all()
    assert torch.equal(run_head(fg, wg, n, P, Cc, dtype)[0], out)                # bit-identical run to run
    acc = torch.zeros(n, device=DEV, dtype=torch.float64)
    want = torch.zeros(n, dtype=torch.float64)
    for _ in range(5):                                                          # five calls accumulate
        run_head(fg, wg, n, P, Cc, dtype, out=acc)
        want = want + out.cpu()
    assert torch.equal(acc.cpu(), want)
    # an all-zero pair contributes exactly 0
    z, _ = run_head(torch.zeros_like(fg), wg, n, P, Cc, dtype)
    assert (z == 0).all()


def test_lpips_head_argument_checks():
    lib = _lib.load()
    f = torch.zeros(2, 40, 64, device=DEV)
    w = torch.zeros(64, device=DEV)
    out = torch.full((1,), -7.0, device=DEV, dtype=torch.float64)
    scratch = torch.full((8,), -7.0, device=DEV, dtype=torch.float64)
    s = _lib.cur_stream()
    need = LP.head_scratch_bytes(1, 40)
    assert need == 24
    calls = {
        "scratch too small": lambda: lib.mebt_op_lpips_head(_lib.F32, _lib.ptr(f), _lib.ptr(w), _lib.ptr(out), None, 1, 1, 40, 64, _lib.ptr(scratch),
                                                            need - 8, s),
        "null pointer": lambda: lib.mebt_op_lpips_head(_lib.F32, _lib.ptr(f), None, _lib.ptr(out), None, 1, 1, 40, 64, _lib.ptr(scratch), need, s),
        "null pointer ": lambda: lib.mebt_op_lpips_head(_lib.F32, _lib.ptr(f), _lib.ptr(w), _lib.ptr(out), None, 1, 1, 40, 64, None, need, s),
        "need N": lambda: lib.mebt_op_lpips_head(_lib.F32, _lib.ptr(f), _lib.ptr(w), _lib.ptr(out), None, 1, 1, 0, 64, _lib.ptr(scratch), need, s),
    }
    for what, call in calls.items():
        assert call() != 0, what
        assert what.strip() in lib.mebt_last_error().decode(), (what, lib.mebt_last_error())
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (scratch == -7.0).all()


# ---- frame selection ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_lpips_input_selects_and_scales_frames(dtype):
    g = torch.Generator().manual_seed(9)
    B, T, H, W = 3, 5, 7, 9
    x = torch.rand(B, 3, T, H, W, generator=g) - 0.5
    pairs = [(2, 4), (0, 0), (1, 3), (2, 4), (0, 2)]
    fr = torch.tensor(pairs, dtype=torch.int32, device=DEV)
    out = torch.full((len(pairs), H, W, 3), float("nan"), device=DEV, dtype=tdt(dtype))
    LP.lpips_input(x.to(DEV), fr, out, dtype=dtype)
    shift, scale = torch.tensor(LP.SHIFT).view(1, 1, 1, 3), torch.tensor(LP.SCALE).view(1, 1, 1, 3)
    ref = torch.stack([(x[b, :, t].permute(1, 2, 0) - shift[0]) / scale[0] for b, t in pairs])
    assert ref.dtype == torch.float32
    assert torch.equal(out.cpu(), ref.to(tdt(dtype)))                            # fp32 exact; fp16 the one rounding of the fp32 value
    # a pair outside the video is not read: zeros
    bad = torch.tensor([(0, 0), (3, 0), (0, 5), (-1, 0)], dtype=torch.int32, device=DEV)
    out = torch.full((4, H, W, 3), float("nan"), device=DEV, dtype=tdt(dtype))
    LP.lpips_input(x.to(DEV), bad, out, dtype=dtype)
    assert torch.equal(out[0].cpu(), ref[1].to(tdt(dtype))) and (out[1:] == 0).all()


# ---- the whole network ------------------------------------------------------------------------------------------------------------------------
def as_video(u8):
    """uint8 [N, H, W, 3] -> float32 [N, 3, 1, H, W] on the device: N clips of one frame"""
    return to_input(u8).unsqueeze(2).contiguous().to(DEV)


@pytest.fixture(scope="module")
def nets(sd):
    return {d: LP.LPIPS.from_state_dict(sd, dtype=d, device=DEV) for d in ("f32", "f16")}


@pytest.mark.parametrize("tag", list(CASES))
def test_lpips_fp32_equals_the_reference(nets, gold, tag):
    net = nets["f32"]
    a, b = as_video(gold[f"a_{tag}"]), as_video(gold[f"b_{tag}"])
    n = CASES[tag][0]
    means = {}

    def tap(s, feats):
        means[s] = torch.stack([feats[0].double().mean((0, 1)), feats[feats.shape[0] // 2].double().mean((0, 1))]).cpu()

    val, lay = net(a, b, layers=True, tap=tap)
    assert val.dtype == torch.float64 and tuple(val.shape) == (n,) and tuple(lay.shape) == (n, 5)
    ev = ((val.cpu().numpy() - gold[f"val_{tag}"]) / gold[f"val_{tag}"]).__abs__().max()
    el = ((lay.cpu().numpy() - gold[f"layers_{tag}"]) / gold[f"layers_{tag}"]).__abs__().max()
    print(f"[LPIPS f32 {tag}] value rel {ev:.2e}, per-layer rel {el:.2e} vs the reference")
    record(f"network[f32 {tag}] value rel vs reference", ev, REF_GATE)
    record(f"network[f32 {tag}] per-layer rel vs reference", el, REF_GATE)
    assert ev <= REF_GATE and el <= REF_GATE
    assert torch.equal(lay.sum(1), val) or ((lay.sum(1) - val).abs() <= 1e-15 * val).all()
    got = torch.cat([means[s] for s in range(5)], 1).numpy()                    # [2, 1472]: image a, image b of pair 0
    want = gold[f"means_{tag}"]
    off = 0
    for s, c in enumerate(LP.CHANNELS):
        d = np.abs(got[:, off:off + c] - want[:, off:off + c]).max() / np.abs(want[:, off:off + c]).max()
        record(f"network[f32 {tag}] slice {s + 1} channel means rel to the largest", d, REF_GATE)
        assert d <= REF_GATE, (tag, s, d)
        off += c
    assert torch.equal(net(a, b), val)                                          # bit-identical run to run
    if n > 1:                                                                   # chunks of one pair: not a bit moves
        keep = net.budget_bytes
        try:
            net.budget_bytes = 1
            assert net.pairs_per_chunk(16, 16) == 1
            v1, l1 = net(a, b, layers=True)
        finally:
            net.budget_bytes = keep
        assert torch.equal(v1, val) and torch.equal(l1, lay)
        assert torch.equal(net(a[1:], b[1:]), val[1:])                          # nor does the batch


def test_lpips_fp16_stays_within_twice_the_measured_deviation(nets, gold):
    worst = 0.0
    for tag in CASES:
        val = nets["f16"](as_video(gold[f"a_{tag}"]), as_video(gold[f"b_{tag}"]))
        dev = ((val.cpu().numpy() - gold[f"val_{tag}"]) / gold[f"val_{tag}"]).__abs__().max()
        print(f"[LPIPS f16 {tag}] value rel {dev:.2e} vs the reference")
        record(f"network[f16 {tag}] value rel vs reference", dev, 2 * F16_MEASURED)
        worst = max(worst, float(dev))
    assert worst <= 2 * F16_MEASURED, worst


def test_lpips_refuses_small_frames_and_other_devices(nets):
    x = torch.zeros(1, 3, 1, 15, 16, device=DEV)
    with pytest.raises(ValueError, match="H, W >= 16"):
        nets["f32"](x, x)
    y = torch.zeros(1, 3, 1, 16, 16)
    with pytest.raises(ValueError, match="is on cpu"):
        nets["f32"](y, y)


# ---- VQGAN.validation_step / reconstruct_stats ------------------------------------------------------------------------------------------------
def build_vq_micro(sd, weight, with_keys=True):
    from mebt_amd.vqgan import VQGAN
    c = mg.VQGAN_CONFIGS["vq_micro"]
    args = argparse.Namespace(n_hiddens=c["n_hiddens"], downsample=c["downsample"], image_channels=3, embedding_dim=c["embedding_dim"],
                              n_codes=c["n_codes"], sequence_length=c["video"][2], sample_every_n_frames=1, resolution=c["video"][3],
                              perceptual_weight=weight)
    m = VQGAN(args)
    full = dict(vq.closed_form_params(mg.vqgan_cfg("vq_micro")))
    if with_keys:
        full.update({LP.PREFIX + k: v for k, v in sd.items()})
    m.load_state_dict(full, strict=False)
    m.compute_dtype = "f32"
    return m.to(DEV).eval()


def twin_on_frames(sd, x, rec, pairs):
    a = torch.stack([x[b, :, t] for b, t in pairs]).cpu()
    r = torch.stack([rec[b, :, t] for b, t in pairs]).cpu()
    return LP.lpips_twin(sd, a, r)[0]


def test_validation_step_logs_the_perceptual_loss(sd):
    x = mg.vqgan_video("vq_micro")
    B, T = x.shape[0], x.shape[2]
    assert (B, T, x.shape[3]) == (2, 4, 16)
    model = build_vq_micro(sd, 0.1)
    kept, inner = {}, model.reconstruct_stats
    model.reconstruct_stats = lambda *a, **k: kept.setdefault("st", inner(*a, **k))
    seed = 123
    torch.manual_seed(seed)
    out = model.validation_step({"video": x.to(DEV)}, 0)
    after = torch.randint(0, 1000, [4])
    torch.manual_seed(seed)
    idx = torch.randint(0, T, [B])
    assert torch.equal(torch.randint(0, 1000, [4]), after)                       # exactly that one draw was consumed
    assert set(out) == {"val/recon_loss", "val/commitment_loss", "val/perplexity", "val/perceptual_loss"}
    pl = out["val/perceptual_loss"]
    assert pl.dtype == torch.float64 and pl.dim() == 0 and pl.is_cuda and model.logged["val/perceptual_loss"] is pl
    want = 0.1 * float(twin_on_frames(sd, x, kept["st"]["recon"], [(b, int(idx[b])) for b in range(B)]).mean())
    err = abs(float(pl) - want) / want
    print(f"[validation_step] val/perceptual_loss {float(pl)!r}, twin {want!r}, rel {err:.2e}, frames {idx.tolist()}")
    record("validation_step val/perceptual_loss rel vs twin", err, REF_GATE)
    assert err <= REF_GATE
    # the other three figures are those of a model without the keys (two decodes differ in the last bits: test_gpu_recon.close_rows)
    plain = build_vq_micro(sd, 0.1, with_keys=False)
    assert plain.lpips is None
    ref = plain.validation_step({"video": x.to(DEV)}, 0)
    assert "val/perceptual_loss" not in ref
    for k in ref:
        tol = 1e-2 if k == "val/perplexity" else 1e-5
        assert abs(float(out[k]) - float(ref[k])) <= tol * abs(float(ref[k])), k


def test_validation_step_with_weight_zero_draws_nothing(sd):
    x = mg.vqgan_video("vq_micro")
    model = build_vq_micro(sd, 0.0)
    assert model.lpips is not None
    torch.manual_seed(5)
    out = model.validation_step({"video": x.to(DEV)}, 0)
    after = torch.randint(0, 1000, [4])
    torch.manual_seed(5)
    assert torch.equal(torch.randint(0, 1000, [4]), after)
    assert float(out["val/perceptual_loss"]) == 0.0


def test_reconstruct_stats_scores_every_second_frame(sd):
    x = mg.vqgan_video("vq_micro").to(DEV)
    model = build_vq_micro(sd, 0.1)
    st = model.reconstruct_stats(x, lpips_every=2)
    lp = st["lpips"]
    assert lp.dtype == torch.float64 and tuple(lp.shape) == (2, 2)
    pairs = [(b, t) for b in range(2) for t in (0, 2)]
    assert torch.equal(model.lpips(x, st["recon"], frames=pairs).view(2, 2), lp)
    want = twin_on_frames(sd, x, st["recon"], pairs).view(2, 2)
    assert ((lp.cpu() - want).abs() <= REF_GATE * want).all()
    assert tuple(model.reconstruct_stats(x, lpips_every=3)["lpips"].shape) == (2, 2) and "lpips" not in model.reconstruct_stats(x)
    with pytest.raises(RuntimeError, match="perceptual weights"):
        build_vq_micro(sd, 0.1, with_keys=False).reconstruct_stats(x, lpips_every=1)


# ---- the command ----------------------------------------------------------------------------------------------------------------------------
def test_measure_recon_with_lpips(sd, tmp_path):
    from mebt_amd.vqgan import load_vqgan
    vqm, args = tiny_vqgan(n_codes=512)
    with_keys = dict(vqm.state_dict())
    with_keys.update({LP.PREFIX + k: v for k, v in sd.items()})
    ck, ck_plain, lp_file = str(tmp_path / "vq_lpips.ckpt"), str(tmp_path / "vq.ckpt"), str(tmp_path / "lpips.pt")
    torch.save({"state_dict": with_keys, "hyper_parameters": {"args": args}}, ck)
    torch.save({"state_dict": vqm.state_dict(), "hyper_parameters": {"args": args}}, ck_plain)
    torch.save(sd, lp_file)
    clips = np.random.RandomState(3).randint(0, 256, (4, 4, 16, 16, 3)).astype(np.uint8)
    clips[:, :, 4:12, 4:12] //= 2
    npy = str(tmp_path / "clips.npy")
    np.save(npy, clips)
    base = ["--data_path", npy, "--sequence_length", "4", "--n_sample", "4", "--batch_size", "3", "--vqgan_dtype", "f32", "--seed", "7"]
    flags = ["--lpips", "--lpips_dtype", "f32", "--lpips_every", "2"]
    out = str(tmp_path / "row.csv")
    row = MR.main(base + flags + ["--vqgan_ckpt", ck, "--out", out])
    assert list(row) == recon.FIELDS + ["LPIPS"]
    lines = open(out).read().splitlines()
    assert lines[0] == "," + ",".join(recon.FIELDS + ["LPIPS"]) and float(lines[1].split(",")[-1]) == row["LPIPS"]
    # the accumulator over the same batches
    a = MR.build_parser().parse_args(base + flags + ["--vqgan_ckpt", ck])
    model = load_vqgan(ck, torch.device(DEV))
    model.compute_dtype, model.lpips_dtype = "f32", "f32"
    MR.seed_everything(a.seed)
    acc = recon.ReconAccumulator(model.n_codes, device=DEV)
    sizes = []
    for x, u8 in MR.real_batches(a, torch.device(DEV)):
        st = model.reconstruct_stats(x, clip_u8=u8, lpips_every=2)
        assert tuple(st["lpips"].shape) == (len(x), 2)
        sizes.append(len(x))
        acc.add(st)
    assert sizes == [3, 1]
    want = acc.result()
    assert abs(row["LPIPS"] - want["LPIPS"]) <= 1e-4 * want["LPIPS"] and 1e-4 < row["LPIPS"] < 10
    # without --lpips the row is the old one; the tensors may come from a file of their own; neither source: a clear exit
    plain = MR.main(base + ["--vqgan_ckpt", ck, "--out", out])
    assert list(plain) == recon.FIELDS and open(out).read().splitlines()[0] == "," + ",".join(recon.FIELDS)
    for k in recon.FIELDS:
        if k in ("identical_frames", "n_clips"):
            assert plain[k] == row[k]
        else:
            tol = {"PSNR": 1e-2, "SSIM": 1e-4, "codes_used": 1.0 / 512}.get(k, (1e-2 if k.startswith("perplexity") else 1e-5) * abs(row[k]))
            assert abs(plain[k] - row[k]) <= tol, k
    ext = MR.main(base + flags + ["--vqgan_ckpt", ck_plain, "--lpips_ckpt", lp_file, "--out", out])
    assert abs(ext["LPIPS"] - row["LPIPS"]) <= 1e-4 * row["LPIPS"]
    with pytest.raises(SystemExit, match="perceptual_model"):
        MR.main(base + flags + ["--vqgan_ckpt", ck_plain, "--out", out])
