"""LPIPS backward on MI355X: the operators of csrc/lpips/lpips_bwd.hip and mebt_op_conv2d_3x3_dgrad against float64, `LPIPS.value_and_grad`
against the real reference's gradients (tests/golden/lpips_grad) and against the float64 twin at the kernels' own decisions, and
`VQGAN.recon_backward` / `train_step` with the perceptual term.  GPU only.

Gates.  head_bwd: a lane adds at most 8 fp32 terms between 6-level butterflies, three times, then a handful of fp32 operations per
element: 2 x the deviation measured on one MI355X run (profiles/lpips_grad_parity_measured.txt) and never above 1e-4 of the tensor's
maximum; f16 adds the store's 2^-11 |v|.  maxpool_2x2_bwd is a select: exact.  conv2d_3x3_dgrad: the summation bound of DESIGN.md §9d,
K 2^-23 sum |dy| |w| with K = 9 Cout products per element, plus 2^-11 |dx| where dx is stored as fp16.  lpips_input_bwd: one fp32
division, an exact multiply, one fp32 add: 1 ulp.  Whole network, f32: where no decision can flip (`s16`, `mid`) every element within
1e-4 of max |g| of the reference (its own float32 sits at 7e-7 of float64); where single decisions flip under a 1e-6 perturbation of the
weights (`odd`, `full`: each flip moves up to 5.8e-3 of max, ~1e-3 in relative L2) the relative L2 stays under 4e-3; on all four, against
the float64 twin AT THE KERNELS' OWN DECISIONS, 2 x the measured deviation and never above 1e-4 of max.  f16: 4 x the deviation of the
fp16-storage twin from float64 at the same decisions and the same scale (the margin of tests/test_gpu_vqgrad.py), and a cosine of at
least 0.999 against the reference (the storage twin alone gave 0.99962 on the CPU)."""
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
from mebt_amd import _lib  # noqa: E402
from mebt_amd import lpips as LP  # noqa: E402
from oracle import vqgan_oracle as vq  # noqa: E402
from tests import lpips_grad_common as lg  # noqa: E402
from tests import vqgrad_common as vc  # noqa: E402
from tests.golden import make_golden as mg  # noqa: E402
from tests.helpers import record_measured  # noqa: E402

DEV = "cuda"
U32, U16 = 2.0 ** -23, 2.0 ** -11
CAP = 1e-4                                   # of the tensor's maximum: no measured gate is ever wider
# worst deviations of one MI355X run, as a share of the tensor's maximum (f16: beyond the store's 2^-11 |v|)
HEAD_BWD_MEASURED = {"f32": 4.4e-7, "f16": 3.5e-8}
NET_F32_MEASURED = 2.2e-6                    # value_and_grad f32 against the float64 twin at its own decisions, worst of the four cases
F16_VALUE_MEASURED = 2.44e-4                 # the forward's fp16 figure (tests/test_gpu_lpips.py)


def record(name, value, gate):
    record_measured("lpips_grad " + name, value, gate)


def gate_of(measured):
    return min(2 * measured, CAP)


def tdt(dtype):
    return torch.float16 if dtype == "f16" else torch.float32


@pytest.fixture(scope="module")
def sd():
    return closed_form_state_dict()


@pytest.fixture(scope="module")
def fx():
    return lg.load_fixture()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "lpips_golden.npz"))


@pytest.fixture(scope="module")
def nets(sd):
    return {d: LP.LPIPS.from_state_dict(sd, dtype=d, device=DEV) for d in ("f32", "f16")}


# ---- lpips_head_bwd ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("Cc,P", [(64, 1), (64, 7), (512, 1), (512, 300)])
def test_lpips_head_bwd_vs_the_float64_formula(Cc, P, with_add, dtype):
    n = 2
    g = torch.Generator().manual_seed(Cc + P)
    f = torch.relu(torch.randn(2 * n, P, Cc, generator=g)).to(tdt(dtype))
    f[0, 0] = 0                                                                  # a zero vector on the real side ...
    f[n + 1, P - 1] = 0                                                          # ... and on the reconstruction's
    w = torch.rand(Cc, generator=g) * 4 / Cc
    coef = 4096.0 * P                                                            # results of order 1: clear of fp16's subnormals
    add = (torch.randn(n, P, Cc, generator=g) * 0.5).to(tdt(dtype)) if with_add else None
    fd = f.double()
    ref = lg.head_bwd_formula(fd[:n], fd[n:], w.double(), coef, None if add is None else add.double())
    fg, wg, ag = f.to(DEV), w.to(DEV), None if add is None else add.to(DEV)
    out = torch.full((n, P, Cc), float("nan"), device=DEV, dtype=tdt(dtype))
    LP.lpips_head_bwd(fg, wg, out, n, P, Cc, coef, ag, dtype)
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    assert (got[fd[n:] <= 0] == 0).all()                                         # the ReLU mask, the planted zero vector with it
    assert (got[1, P - 1] == 0).all() and torch.isfinite(got[0, 0]).all()
    store = U16 * ref.abs() if dtype == "f16" else torch.zeros_like(ref)
    dev = float(((got - ref).abs() - store).clamp_min(0).max() / ref.abs().max())
    gate = gate_of(HEAD_BWD_MEASURED[dtype])
    print(f"[lpips_head_bwd {dtype} C={Cc} P={P} add={with_add}] deviation {dev:.2e} of max (gate {gate:.1e})")
    record(f"head_bwd[{dtype} C={Cc} P={P} add={int(with_add)}] of max", dev, gate)
    assert dev <= gate
    again = torch.empty_like(out)
    LP.lpips_head_bwd(fg, wg, again, n, P, Cc, coef, ag, dtype)
    assert torch.equal(again, out)                                               # bit-identical run to run
    # the second pair alone: the same bits as inside the batch
    alone = torch.empty(1, P, Cc, device=DEV, dtype=tdt(dtype))
    LP.lpips_head_bwd(torch.stack([fg[1], fg[n + 1]]), wg, alone, 1, P, Cc, coef, None if ag is None else ag[1:], dtype)
    assert torch.equal(alone[0], out[1])


# ---- maxpool_2x2_bwd ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("Cc", [5, 64])
@pytest.mark.parametrize("H,W", [(2, 3), (5, 2), (9, 9), (16, 16)])
def test_maxpool_2x2_bwd_is_exact(H, W, Cc, dtype):
    g = torch.Generator().manual_seed(H * 100 + W + Cc)
    N = 2
    x = torch.relu(torch.randn(N, H, W, Cc, generator=g)).to(tdt(dtype))
    x[0, 0:2, 0:2, 0] = 0.75                                                     # four equal values: the first wins
    x[0, 0:2, 0:2, 1] = torch.tensor([[0.1, 0.9], [0.9, 0.2]]).to(tdt(dtype))     # two equal maxima: (0, 1) before (1, 0)
    x[0, 0:2, 0:2, 2] = torch.tensor([[0.1, 0.2], [0.9, 0.9]]).to(tdt(dtype))     # (1, 0) before (1, 1)
    x[0, 0:2, 0:2, 3] = torch.tensor([[0.9, 0.2], [0.1, 0.9]]).to(tdt(dtype))     # (0, 0) before (1, 1)
    x[1, 0:2, 0:2, :] = 0                                                        # windows of zeros pass nothing on
    x[1, 0:2, 0:2, 4] = torch.tensor([[-1.0, -0.5], [-2.0, -3.0]]).to(tdt(dtype))  # nor does a negative-only window
    dy = (torch.randn(N, H // 2, W // 2, Cc, generator=g) + 3.0).to(tdt(dtype))    # never zero: a dropped gradient shows
    ref = lg.pool_bwd_rule(x.double(), dy.double())
    assert (ref[1, 0:2, 0:2] == 0).all() and ref[0, 0, 0, 0] == dy[0, 0, 0, 0].double() and ref[0, 0, 1, 1] == dy[0, 0, 0, 1].double()
    assert ref[0, 1, 0, 2] == dy[0, 0, 0, 2].double() and ref[0, 0, 0, 3] == dy[0, 0, 0, 3].double()
    dx = torch.full((N, H, W, Cc), float("nan"), device=DEV, dtype=tdt(dtype))
    LP.maxpool_2x2_bwd(x.to(DEV), dy.to(DEV), dx, dtype)
    assert torch.equal(dx.cpu().double(), ref)                                    # every element written, trailing rows and columns 0
    # the narrow path of a wide shape: a view that is not 16-byte aligned
    if Cc == 64 and dtype == "f16":
        pad = torch.zeros(N * H * W * Cc + 1, device=DEV, dtype=torch.float16)
        pad[1:] = x.to(DEV).reshape(-1)
        out2 = torch.full((N, H, W, Cc), float("nan"), device=DEV, dtype=torch.float16)
        LP.maxpool_2x2_bwd(pad[1:].view(N, H, W, Cc), dy.to(DEV), out2, dtype)
        assert torch.equal(out2, dx)


# ---- conv2d_3x3_dgrad -------------------------------------------------------------------------------------------------------------------------
DGRAD_CASES = [(3, 64, 3, 5, 7), (64, 64, 3, 5, 7), (128, 256, 2, 4, 4), (512, 512, 2, 1, 1), (512, 512, 2, 2, 2)]     # the FORWARD's Cin, Cout


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("cin,cout,N,H,W", DGRAD_CASES)
def test_conv2d_3x3_dgrad_vs_conv_transpose2d(cin, cout, N, H, W, dtype):
    g = torch.Generator().manual_seed(cin * 1000 + cout + H)
    t = tdt(dtype)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(t)
    dy = torch.randn(N, H, W, cout, generator=g).to(t)
    y_prev = None if cin == 3 else torch.randn(N, H, W, cin, generator=g).to(t)   # the first layer's input is no ReLU output
    if y_prev is not None:
        y_prev[:, 0, 0, ::2] = 0                                                 # zeros mask like negatives
    dyd, wd = dy.double().permute(0, 3, 1, 2), w.double()
    ref = F.conv_transpose2d(dyd, wd, padding=1).permute(0, 2, 3, 1)
    S = F.conv_transpose2d(dyd.abs(), wd.abs(), padding=1).permute(0, 2, 3, 1)
    keep = torch.ones_like(ref, dtype=torch.bool) if y_prev is None else y_prev.double() > 0
    ref = torch.where(keep, ref, torch.zeros_like(ref))
    bound = 9 * cout * U32 * S + (U16 * ref.abs() + 2.0 ** -25 if dtype == "f16" else 0.0)
    wl = LP.arrange_weight_dgrad(w.to(DEV), t)
    dyg, yg = dy.to(DEV), None if y_prev is None else y_prev.to(DEV)
    # the forward on the same template, before and after: not a bit of it moves
    xf = torch.randn(N, H, W, cin, generator=g).to(t).to(DEV)
    wf, bf = LP.arrange_weight(w.to(DEV), t), torch.randn(cout, generator=g).to(DEV)
    fwd0 = LP.conv2d_3x3(xf, wf, bf, torch.empty(N, H, W, cout, device=DEV, dtype=t), cin, cout, dtype)
    dx = torch.full((N, H, W, cin), float("nan"), device=DEV, dtype=t)
    LP.conv2d_3x3_dgrad(dyg, wl, yg, dx, cout, cin, dtype)
    fwd1 = LP.conv2d_3x3(xf, wf, bf, torch.empty(N, H, W, cout, device=DEV, dtype=t), cin, cout, dtype)
    assert torch.equal(fwd0, fwd1)
    got = dx.cpu().double()
    assert torch.isfinite(got).all()
    assert (got[~keep] == 0).all()                                               # zeros exactly where y_prev <= 0
    ratio = float(((got - ref).abs() / (bound + 1e-300))[keep].max())
    print(f"[conv2d_3x3_dgrad {dtype} {cin}<-{cout} {N}x{H}x{W}] err / bound {ratio:.3f}")
    record(f"conv2d_3x3_dgrad[{dtype} {cin}<-{cout} {N}x{H}x{W}] err / bound", ratio, 1.0)
    assert ratio <= 1.0
    again = torch.empty_like(dx)
    LP.conv2d_3x3_dgrad(dyg, wl, yg, again, cout, cin, dtype)
    assert torch.equal(again, dx)
    alone = torch.empty(1, H, W, cin, device=DEV, dtype=t)                       # image 1 alone: the same bits as inside the batch
    LP.conv2d_3x3_dgrad(dyg[1:2].contiguous(), wl, None if yg is None else yg[1:2].contiguous(), alone, cout, cin, dtype)
    assert torch.equal(alone[0], dx[1])


# ---- lpips_input_bwd --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_lpips_input_bwd_adds_into_the_chosen_frames_only(dtype):
    g = torch.Generator().manual_seed(3)
    B, T, H, W = 2, 3, 5, 7
    pairs = [(1, 2), (0, 0)]
    seed0 = torch.randn(B, 3, T, H, W, generator=g)
    d = torch.randn(len(pairs), H, W, 3, generator=g).to(tdt(dtype))
    host = torch.tensor(pairs, dtype=torch.int32)
    for factor in (1.0, 0.125, 64.0):
        seed = seed0.clone().to(DEV)
        LP.lpips_input_bwd(d.to(DEV), host.to(DEV), host, seed, LP.SCALE, factor, dtype)
        got = seed.cpu()
        want = seed0.clone()
        scale = torch.tensor(LP.SCALE, dtype=torch.float32)
        for n, (b, t) in enumerate(pairs):
            want[b, :, t] += ((d[n].float() / scale) * factor).permute(2, 0, 1)        # fp32 division, exact multiply, fp32 add
        touched = torch.zeros(B, T, dtype=torch.bool)
        for b, t in pairs:
            touched[b, t] = True
        for b in range(B):
            for t in range(T):
                if not touched[b, t]:
                    assert torch.equal(got[b, :, t], seed0[b, :, t]), (b, t)
        ulp = (torch.nextafter(want.abs(), torch.tensor(float("inf"))) - want.abs())
        assert bool(((got - want).abs() <= ulp).all()), factor
        assert not torch.equal(got[1, :, 2], seed0[1, :, 2])
    seed = seed0.clone().to(DEV)
    dup = torch.tensor([(1, 2), (0, 0), (1, 2)], dtype=torch.int32)
    d3 = torch.zeros(3, H, W, 3, device=DEV, dtype=tdt(dtype))
    with pytest.raises(_lib.MebtError, match="distinct"):
        LP.lpips_input_bwd(d3, dup.to(DEV), dup, seed, LP.SCALE, 1.0, dtype)
    torch.cuda.synchronize()
    assert torch.equal(seed.cpu(), seed0)


def test_backward_operators_check_their_arguments():
    lib = _lib.load()
    s = _lib.cur_stream()
    f = torch.zeros(2, 4, 64, device=DEV)
    w = torch.zeros(64, device=DEV)
    out = torch.full((1, 4, 64), -7.0, device=DEV)
    p = _lib.ptr
    calls = [
        ("null pointer", lambda: lib.mebt_op_lpips_head_bwd(_lib.F32, p(f), None, None, p(out), 1, 4, 64, 1.0, s)),
        ("null pointer", lambda: lib.mebt_op_lpips_head_bwd(_lib.F32, p(f), p(w), None, None, 1, 4, 64, 1.0, s)),
        ("need N", lambda: lib.mebt_op_lpips_head_bwd(_lib.F32, p(f), p(w), None, p(out), 0, 4, 64, 1.0, s)),
        ("need N", lambda: lib.mebt_op_lpips_head_bwd(_lib.F32, p(f), p(w), None, p(out), 1, 0, 64, 1.0, s)),
        ("finite", lambda: lib.mebt_op_lpips_head_bwd(_lib.F32, p(f), p(w), None, p(out), 1, 4, 64, float("inf"), s)),
        ("dtype", lambda: lib.mebt_op_lpips_head_bwd(_lib.BF16, p(f), p(w), None, p(out), 1, 4, 64, 1.0, s)),
        ("null pointer", lambda: lib.mebt_op_maxpool_2x2_bwd(_lib.F32, p(f), None, p(out), 1, 2, 2, 64, s)),
        ("2 x 2 window", lambda: lib.mebt_op_maxpool_2x2_bwd(_lib.F32, p(f), p(f), p(out), 1, 1, 4, 64, s)),
        ("need N", lambda: lib.mebt_op_maxpool_2x2_bwd(_lib.F32, p(f), p(f), p(out), 0, 2, 2, 64, s)),
        ("dtype", lambda: lib.mebt_op_maxpool_2x2_bwd(_lib.BF16, p(f), p(f), p(out), 1, 2, 2, 64, s)),
        ("null pointer", lambda: lib.mebt_op_conv2d_3x3_dgrad(_lib.F32, p(f), None, None, p(out), 1, 2, 2, 64, 64, s)),
        ("multiple of 32", lambda: lib.mebt_op_conv2d_3x3_dgrad(_lib.F32, p(f), p(f), None, p(out), 1, 2, 2, 3, 64, s)),
        ("multiple of 32", lambda: lib.mebt_op_conv2d_3x3_dgrad(_lib.F32, p(f), p(f), None, p(out), 1, 2, 2, 48, 64, s)),
        ("multiple of 32", lambda: lib.mebt_op_conv2d_3x3_dgrad(_lib.F32, p(f), p(f), None, p(out), 1, 2, 2, 1024, 64, s)),
        ("need N", lambda: lib.mebt_op_conv2d_3x3_dgrad(_lib.F32, p(f), p(f), None, p(out), 1, 2, 2, 64, 0, s)),
        ("16-byte", lambda: lib.mebt_op_conv2d_3x3_dgrad(_lib.F32, p(f), p(f), p(f) + 4, p(out), 1, 2, 2, 64, 64, s)),
        ("dtype", lambda: lib.mebt_op_conv2d_3x3_dgrad(_lib.BF16, p(f), p(f), None, p(out), 1, 2, 2, 64, 64, s)),
    ]
    for what, call in calls:
        assert call() != 0, what
        assert what in lib.mebt_last_error().decode(), (what, lib.mebt_last_error())
    torch.cuda.synchronize()
    assert (out == -7.0).all()


# ---- the whole network ------------------------------------------------------------------------------------------------------------------------
def as_video(u8):
    """uint8 [N, H, W, 3] -> float32 [N, 3, 1, H, W] on the device: N clips of one frame"""
    return to_input(u8).unsqueeze(2).contiguous().to(DEV)


_runs = {}


def run_case(nets, gold, tag, dtype):
    """value_and_grad with the tape kept, and the float64 twin at the tape's decisions: computed once per (case, dtype)"""
    if (tag, dtype) not in _runs:
        net = nets[dtype]
        n = CASES[tag][0]
        a, b = as_video(gold[f"a_{tag}"]), as_video(gold[f"b_{tag}"])
        seed = torch.zeros_like(b)
        val, tape, d_feats = net.value_and_grad(a, b, torch.zeros(n, dtype=torch.int64), seed, 1.0, keep_tape=True)
        dec = lg.tape_decisions(tape, n)
        v64, g64, _, _ = lg.twin_at(closed_form_state_dict(), to_input(gold[f"a_{tag}"]), to_input(gold[f"b_{tag}"]), decisions=dec)
        _runs[(tag, dtype)] = dict(a=a, b=b, val=val, grad=seed[:, :, 0].cpu().double(), dec=dec, v64=v64, g64=g64,
                                   shapes=[tuple(t.shape) for t in tape], d_shapes=[tuple(t.shape) for t in d_feats])
    return _runs[(tag, dtype)]


@pytest.mark.parametrize("tag", list(CASES))
def test_value_and_grad_f32_against_the_reference_and_the_twin_at_its_decisions(nets, gold, fx, tag):
    r = run_case(nets, gold, tag, "f32")
    n, H, W = CASES[tag]
    assert torch.equal(r["val"], nets["f32"](r["a"], r["b"]))                     # the values are __call__'s, bit for bit
    assert r["shapes"] == [(2 * n, h, w, c) for (_s, h, w, _ci, c, _f) in LP.plan_flops(H, W)[1]]
    assert [s[0] for s in r["d_shapes"]] == [n] * 5 and [s[3] for s in r["d_shapes"]] == LP.CHANNELS
    ref = torch.from_numpy(fx[f"grad_{tag}"]).double() * n                        # the fixture differentiates the mean
    got = r["grad"]
    assert torch.isfinite(got).all()
    err = float((got - ref).abs().max() / ref.abs().max())
    l2 = float((got - ref).norm() / ref.norm())
    print(f"[value_and_grad f32 {tag}] vs the reference: {err:.2e} of max, relative L2 {l2:.2e}")
    if tag in ("s16", "mid"):
        record(f"network[f32 {tag}] of max vs reference", err, lg.REF_GATE)
        assert err <= lg.REF_GATE
    else:
        record(f"network[f32 {tag}] relative L2 vs reference", l2, lg.FLIP_L2)
        assert l2 <= lg.FLIP_L2
    dev = float((got - r["g64"]).abs().max() / r["g64"].abs().max())
    gate = gate_of(NET_F32_MEASURED)
    print(f"[value_and_grad f32 {tag}] vs the float64 twin at its own decisions: {dev:.2e} of max (gate {gate:.1e})")
    record(f"network[f32 {tag}] of max vs twin at decisions", dev, gate)
    assert dev <= gate
    assert float(((r["val"].cpu() - r["v64"]).abs() / r["v64"]).max()) <= lg.REF_GATE


@pytest.mark.parametrize("tag", list(CASES))
def test_value_and_grad_f16_within_four_times_the_storage_twin(nets, gold, fx, sd, tag):
    r = run_case(nets, gold, tag, "f16")
    n, H, W = CASES[tag]
    Sp = LP.default_branch_scale(1.0, H, W)
    _, g16, _, _ = lg.twin_at(sd, to_input(gold[f"a_{tag}"]), to_input(gold[f"b_{tag}"]), decisions=r["dec"], fp16_storage=True, scale=Sp)
    top = float(r["g64"].abs().max())
    twin_dev = float((g16 - r["g64"]).abs().max()) / top
    dev = float((r["grad"] - r["g64"]).abs().max()) / top
    ref = torch.from_numpy(fx[f"grad_{tag}"]).double() * n
    cos = float((r["grad"] * ref).sum() / (r["grad"].norm() * ref.norm()))
    print(f"[value_and_grad f16 {tag}] vs the float64 twin at its own decisions: {dev:.2e} of max; storage twin {twin_dev:.2e} (gate "
          f"{4 * twin_dev:.2e}); cosine vs the reference {cos:.6f}; branch scale {Sp:g}")
    record(f"network[f16 {tag}] of max vs twin at decisions", dev, 4 * twin_dev)
    record(f"network[f16 {tag}] 1 - cosine vs reference", 1 - cos, 1e-3)
    assert torch.isfinite(r["grad"]).all()
    assert dev <= 4 * twin_dev
    assert cos >= 0.999


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_value_and_grad_bits_do_not_depend_on_run_batch_or_chunk(nets, gold, dtype):
    net = nets[dtype]
    a, b = as_video(gold["a_odd"]), as_video(gold["b_odd"])
    fr = torch.zeros(3, dtype=torch.int64)

    def run(a_, b_, frames, coef=1.0, flags=None):
        seed = torch.zeros_like(b_)
        return net.value_and_grad(a_, b_, frames, seed, coef, flags=flags), seed
    flags = []
    v0, s0 = run(a, b, fr, flags=flags)
    assert len(flags) == 1 and bool(flags[0])
    v1, s1 = run(a, b, fr)
    assert torch.equal(v0, v1) and torch.equal(s0, s1)                            # two runs
    v2, s2 = run(a[1:2], b[1:2], fr[:1])
    assert torch.equal(v2, v0[1:2]) and torch.equal(s2[0], s0[1])                  # a pair alone and in the batch of three
    keep = net.budget_bytes
    try:
        net.budget_bytes = 1
        assert net.pairs_per_chunk_grad(36, 20) == 1
        flags = []
        v3, s3 = run(a, b, fr, flags=flags)
        assert len(flags) == 3
    finally:
        net.budget_bytes = keep
    assert torch.equal(v3, v0) and torch.equal(s3, s0)                            # chunks of one pair
    # it ADDS: a second call on the same seed doubles it, and coef scales it
    seed = s0.clone()
    net.value_and_grad(a, b, fr, seed, 1.0)
    assert torch.equal(seed, 2 * s0)
    _, sh = run(a, b, fr, coef=0.5)
    assert torch.equal(sh, 0.5 * s0)                                              # a power of two moves the branch scale only
    with pytest.raises(ValueError, match="distinct"):
        run(a, b, [(0, 0), (0, 0)])
    # overflow of the branch is reported, not hidden
    if dtype == "f16":
        flags = []
        seed = torch.zeros_like(b)
        net.value_and_grad(a, b, fr, seed, 1.0, grad_scale=2.0 ** 40, flags=flags)
        assert not bool(flags[0])


# ---- VQGAN.recon_backward / train_step with the perceptual term -------------------------------------------------------------------------------
def build(sd, dtype, weight=1.0, with_keys=True):
    from mebt_amd.vqgan import VQGAN
    c = mg.VQGAN_CONFIGS["vq_micro"]
    args = argparse.Namespace(n_hiddens=c["n_hiddens"], downsample=c["downsample"], image_channels=3, embedding_dim=c["embedding_dim"],
                              n_codes=c["n_codes"], sequence_length=c["video"][2], sample_every_n_frames=1, resolution=c["video"][3],
                              l1_weight=4.0, perceptual_weight=weight, lr=3e-4)
    m = VQGAN(args)
    full = dict(vq.closed_form_params(mg.vqgan_cfg("vq_micro")))
    if with_keys:
        full.update({LP.PREFIX + k: v for k, v in sd.items()})
    m.load_state_dict(full, strict=False)
    m.compute_dtype = dtype
    return m.to(DEV).eval()


def grads_of(m):
    return {k: p.grad.detach().cpu().double().numpy() for k, p in m.named_parameters() if k.startswith(vc.TRAINED)}


def test_recon_backward_f32_with_the_perceptual_term_matches_the_reference(sd, fx):
    """every stored gradient within 2e-5 of its tensor's maximum of the reference's (the gate of tests/test_gpu_vqgrad.py); every one of
    the 68 through its projection on a fixed direction p: an elementwise error of at most 2e-5 max |g| moves sum g p by at most
    2e-5 max |g| sum |p|"""
    m = build(sd, "f32")
    x = torch.from_numpy(vc.load_fixture()["x"]).to(DEV)
    out = m.recon_backward(x, frame_idx=torch.from_numpy(fx["vq_frame_idx"]))
    assert sorted(out) == ["commitment_loss", "encodings", "finite", "frame_idx", "grad_scale", "perceptual_loss", "perplexity", "recon_loss",
                           "x_recon"]
    assert out["finite"] is True and out["frame_idx"].tolist() == fx["vq_frame_idx"].tolist()
    assert np.array_equal(out["encodings"].cpu().numpy(), fx["vq_ids"]), "the ids differ from the reference's"
    assert out["perceptual_loss"].dtype == torch.float64 and out["perceptual_loss"].dim() == 0
    for key, want, tol in (("recon_loss", fx["vq_losses"][0], 1e-5), ("commitment_loss", fx["vq_losses"][1], 1e-5),
                           ("perceptual_loss", fx["vq_losses"][2], lg.REF_GATE)):
        assert abs(float(out[key]) - want) <= tol * want, (key, float(out[key]), want)
    got = grads_of(m)
    names = [k[len("vqmax/"):] for k in fx if k.startswith("vqmax/")]
    assert sorted(got) == sorted(names)
    scale = {k: float(fx["vqmax/" + (k[:-len("bias")] + "weight" if k in vc.ZERO_BIAS else k)]) for k in names}
    worst = worst_dot = 0.0
    for k in names:
        p = lg.probe(k, got[k].shape)
        e = abs((got[k] * p).sum() - float(fx["vqdot/" + k])) / (scale[k] * np.abs(p).sum())
        worst_dot = max(worst_dot, e)
        assert e <= 2e-5, (k, "dot", e)
        if "vqgrad/" + k in fx:
            err = np.abs(got[k] - fx["vqgrad/" + k].astype(np.float64)).max() / scale[k]
            worst = max(worst, err)
            assert err <= 2e-5, (k, err)
    print(f"[recon_backward f32 + LPIPS] worst deviation from the reference {worst:.2e} of the tensor's maximum, projections {worst_dot:.2e}")
    record("recon_backward[f32] of max vs reference", worst, 2e-5)
    record("recon_backward[f32] projections vs reference", worst_dot, 2e-5)


def test_recon_backward_f16_with_the_perceptual_term_within_four_times_the_storage_twin(sd, fx):
    m = build(sd, "f16")
    m.__dict__["_lpips_keep_tape"] = True
    x = torch.from_numpy(vc.load_fixture()["x"])
    out = m.recon_backward(x.to(DEV), frame_idx=torch.from_numpy(fx["vq_frame_idx"]))
    assert np.array_equal(out["encodings"].cpu().numpy(), fx["vq_ids"]), "the f16 ids differ from the fixture's"
    assert out["finite"] is True and out["grad_scale"] == float(fx["vq_twin_scale"])
    B = x.shape[0]
    assert LP.default_branch_scale(out["grad_scale"] * 1.0 / B, 16, 16) == float(fx["vq_twin_branch_scale"])
    rec = out["x_recon"].cpu()
    signs = torch.sign(rec.double() - x)
    dec = lg.tape_decisions(out["lpips_tape"], B)
    cfg = mg.vqgan_cfg("vq_micro")
    P = vq.closed_form_params(cfg)
    ref, _, _, _ = lg.vq_objective_grads(P, cfg, sd, x, torch.from_numpy(fx["vq_ids"]), fx["vq_frame_idx"], l1_signs=signs, decisions=dec)
    got = grads_of(m)
    worst = 0.0
    for k in ref:
        err, gate = np.abs(got[k] - ref[k]).max() / vc.scale_of(k, ref), 4 * float(fx["twin_dev/" + k])
        worst = max(worst, err / gate)
        assert err <= gate, (k, err, gate)
    print(f"[recon_backward f16 + LPIPS] worst err / gate {worst:.3f}")
    record("recon_backward[f16] worst err / gate", worst, 1.0)
    fi = fx["vq_frame_idx"]
    twin = LP.lpips_twin(sd, torch.stack([x[b, :, fi[b]] for b in range(B)]), torch.stack([rec[b, :, fi[b]] for b in range(B)]))[0].mean()
    assert abs(float(out["perceptual_loss"]) - float(twin)) <= 2 * F16_VALUE_MEASURED * float(twin)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_weight_zero_is_bit_identical_to_a_model_without_perceptual_weights(sd, dtype):
    """on the 2 x 8 x 8 corner, where the forward's GroupNorm sums are order-free (tests/test_gpu_vqgrad.py) and two runs give the same bits"""
    x = torch.from_numpy(vc.load_fixture()["x"][:, :, :2, :8, :8].copy()).to(DEV)
    a, b = build(sd, dtype, 0.0, True), build(sd, dtype, 0.0, False)
    assert a.lpips is not None and b.lpips is None
    oa, ob = a.recon_backward(x), b.recon_backward(x)
    assert sorted(oa) == sorted(ob) == ["commitment_loss", "encodings", "finite", "grad_scale", "perplexity", "recon_loss", "x_recon"]
    for k in oa:
        assert torch.equal(oa[k], ob[k]) if torch.is_tensor(oa[k]) else oa[k] == ob[k], k
    ga, gb = grads_of(a), grads_of(b)
    assert all(np.array_equal(ga[k], gb[k]) for k in ga)


def test_recon_backward_without_perceptual_weights_raises(sd):
    m = build(sd, "f32", 1.0, False)
    x = torch.from_numpy(vc.load_fixture()["x"]).to(DEV)
    with pytest.raises(RuntimeError, match="perceptual weights"):
        m.recon_backward(x)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_train_step_with_the_perceptual_term_lowers_the_loss(sd, fx, dtype):
    m = build(sd, dtype).train()
    x = torch.from_numpy(vc.load_fixture()["x"]).to(DEV)
    opt = m.configure_optimizers()
    gen = torch.Generator(device=DEV).manual_seed(0)
    losses = []
    for _ in range(3):
        out = m.train_step(x, opt, generator=gen, frame_idx=torch.from_numpy(fx["vq_frame_idx"]))
        assert out["finite"] is True and all(torch.isfinite(p.grad).all() for n, p in m.named_parameters() if n.startswith(vc.TRAINED))
        losses.append(float(out["recon_loss"]) + float(out["commitment_loss"]) + float(out["perceptual_loss"]))
    print(f"[train_step {dtype} + LPIPS] loss over the steps: {' '.join(f'{v:.4f}' for v in losses)}")
    assert losses[2] < losses[0]
    # drawn when not given: one frame per clip, inside the clip
    out = m.train_step(x, opt, generator=gen)
    assert out["frame_idx"].shape == (2,) and int(out["frame_idx"].min()) >= 0 and int(out["frame_idx"].max()) < 4


def test_train_vqgan_command_trains_with_the_perceptual_term_and_resumes_without_lpips_ckpt(sd, tmp_path):
    import subprocess
    from tests.test_fvd_frames_host import write_png_tree
    os.makedirs(str(tmp_path / "frames"))
    root = write_png_tree(str(tmp_path / "frames"), 3, 6, seed=2)
    run, weights = str(tmp_path / "run"), str(tmp_path / "lpips.pt")
    torch.save(sd, weights)
    base = [sys.executable, "-m", "mebt_amd.train_vqgan", "--data_path", root, "--image_folder", "--sequence_length", "4", "--resolution", "16",
            "--batch_size", "2", "--num_workers", "0", "--log_every", "1", "--ckpt_every", "2", "--default_root_dir", run, "--dtype", "f16", "--seed", "1"]
    model = ["--n_hiddens", "16", "--downsample", "2", "4", "4", "--embedding_dim", "64", "--n_codes", "512", "--perceptual_weight", "1.0"]
    res = subprocess.run(base + model + ["--max_steps", "2", "--lpips_ckpt", weights], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("step ")]
    assert len(lines) == 2 and all("train/perceptual_loss" in l for l in lines), res.stdout
    assert float(lines[-1].split("train/perceptual_loss")[1].split()[0]) > 0.0
    last = os.path.join(run, "checkpoints", "last.ckpt")
    ck = torch.load(last, map_location="cpu", weights_only=False)
    assert ck["global_step"] == 2 and sum(k.startswith(LP.PREFIX) for k in ck["state_dict"]) == 33
    assert not hasattr(ck["hyper_parameters"]["args"], "lpips_ckpt") and ck["hyper_parameters"]["args"].perceptual_weight == 1.0
    res = subprocess.run(base + ["--max_steps", "3", "--vqgan_ckpt", last], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("step ")]
    assert len(lines) == 1 and lines[0].startswith("step 3:") and "train/perceptual_loss" in lines[0], res.stdout
