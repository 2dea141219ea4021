"""Operator tests of the row kernels of csrc/elementwise.hip, through the plain C entry points: LayerNorm in every form the engine
launches (row map, three jobs per launch, dy2 / dx_add / dx_accumulate, fp32 dx of a bf16 job, the dropout-masked dx2, grouped column
sums riding on the backward), the masked-token loss in both of its kernels and its backward, AdamW with bf16 gradient pieces, the
column sums, the embedding backward and the row movers.

Every input is rounded to its storage type before either side sees it, every reference is float64, every output lives in a Guard
buffer (sentinel before and behind the body, NaN inside; inputs are surrounded by POISON), and every gate is derived from the
reference's own fp32 error or from the number formats (see each test) and printed as `err / gate`.

Worst `err / gate` per family, as printed on an MI355X (164 cases, 12 s):
  LayerNorm forward    f32: y 0.15, mean 0.22, rstd 0.18; bf16: y 0.99 (the store's rounding: UB |y| is met where |y| is just
                       above a power of two), mean 0.11, rstd 0.19
  LayerNorm backward   f32: dx 0.19, dgamma 0.16, dbeta 0.07; bf16: dx 1.00 (0.996, the store again; 0.24 where dx is fp32),
                       dgamma 0.21, dbeta 0.02
  column sums          f32 0.02, bf16 0.21 (stand-alone), 0.02 / 0.006 riding on the LayerNorm backward
  loss                 lse 0.07, loss 0.07 (fused kernel: 0.03 / 0.02); dlogits f32 0.44 (ce_bwd) / 0.41 (fused), bf16 0.99 (the
                       store).  The fp32 emulation on the CPU: lse 0.08, loss 0.07, dlogits 0.41
  AdamW                m 0.24, v 0.44, p 0.31
  embedding backward   tok 0.26, pos 0.25, mask 0.10, sos 0.27
  row movers, dx2, row_rank, the top-1 / top-5 counts, the loss sum, the bf16 mirror: bit for bit

Two gates moved from their first derivation, each by a term named where it is used: the fp32 floor of the LayerNorm gates is never
below 2^-24 max|ref| (`floor`: on a one-row launch the measured deviation is a single sample), and AdamW's gate for p carries m's
own absolute error (`test_adamw`).
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from mebt_amd import _lib
from mebt_amd._lib import check, cur_stream, LnJob, ColsumItem, F32, BF16

DEV = "cuda"
SENTINEL = -77.0     # exact in bf16 and fp32
POISON = 5.0
U32 = 2.0 ** -23
UB = 2.0 ** -8       # bf16's unit roundoff
PAD = 64             # guard elements on either side of a body (a multiple of 16 bytes in every type)
NAMES = {F32: "f32", BF16: "bf16"}


def lib():
    return _lib.load()


def tdt(dtype):
    return torch.bfloat16 if dtype == BF16 else torch.float32


def q(x, dtype):
    """round to the storage type: both sides start from the same stored values"""
    return x.to(tdt(dtype)).float()


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


class Guard:
    """a device tensor of `shape` inside a flat buffer: PAD elements of `fill` before and behind it.  Outputs: fill = SENTINEL and the
    body starts as NaN (floating types) or as `init`; get() asserts that the guards survived.  Inputs: fill = POISON."""

    def __init__(self, shape, t, init=None, fill=SENTINEL):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        self.n = int(np.prod(shape)) if len(shape) else 1
        self.fill = fill
        self.flat = torch.full((self.n + 2 * PAD,), fill, device=DEV, dtype=t)
        self.body = self.flat[PAD:PAD + self.n].view(shape)
        if init is not None:
            self.body[:] = init.to(DEV, t) if torch.is_tensor(init) else init
        elif t.is_floating_point:
            self.body[:] = float("nan")
        self.ptr = self.flat.data_ptr() + PAD * self.flat.element_size()

    def get(self):
        """the body on the CPU (float64 for floating types), after asserting that nothing around it was written"""
        assert bool((self.flat[:PAD] == self.fill).all()) and bool((self.flat[PAD + self.n:] == self.fill).all()), "the kernel wrote outside its output"
        b = self.body.cpu()
        return b.double() if b.dtype.is_floating_point else b


def inp(x, t):
    """an input tensor surrounded by POISON"""
    return Guard(x.shape, t, init=x, fill=POISON)


def bits(x):
    """the stored bits of a CPU tensor, for bit-for-bit comparisons"""
    return x.contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32 if x.dtype == torch.float32 else torch.int64)


RATIOS = {}


def gate_check(what, got, ref, gate, family=None):
    """assert |got - ref| <= gate element by element and print the worst err / gate (a zero gate asks for equality)"""
    got, ref = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(ref, dtype=torch.float64)
    gate = torch.as_tensor(gate, dtype=torch.float64).expand_as(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: the kernel left elements unwritten or wrote non-finite values"
    err = (got - ref).abs()
    ratio = torch.where(gate > 0, err / gate.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{what}: err / gate = {worst:.3f}  (max err {float(err.max()) if err.numel() else 0.0:.3e})")
    if family:
        RATIOS[family] = max(RATIOS.get(family, 0.0), worst)
        print(f"  worst so far [{family}]: {RATIOS[family]:.3f}")
    assert worst <= 1.0, (what, worst)
    return worst


def map_rows(rows, seg):
    """row r -> (r / s) * stride + off + r % s for seg = (s, stride, off); None: identity.  Returns (index tensor, rows of the mapped buffer)"""
    r = torch.arange(rows)
    if seg is None:
        return r, rows
    s, stride, off = seg
    m = (r // s) * stride + off + r % s
    return m, (int(m.max()) + 3 if rows else 0)


def seg3(seg):
    return seg if seg is not None else (0, 0, 0)


# ------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------
FIXED = {BF16: [512, 1024, 2048], F32: [256, 1024]}              # the fixed-chunk widths of LN_WIDTHS
GENERIC = {BF16: [64, 320], F32: [4, 320, 2048]}                 # d = 4: 63 dead lanes; fp32 2048: all 8 chunks live
WIDTHS = [(dt, d) for dt in (F32, BF16) for d in FIXED[dt] + GENERIC[dt]]
WIDTH_IDS = [f"{NAMES[dt]}-{d}" for dt, d in WIDTHS]


def ln_ref64(x, g, b):
    """float64 LayerNorm (eps 1e-5) of rows x: y, mean, rstd, xhat"""
    x, g, b = x.double(), g.double(), b.double()
    mean = x.mean(-1)
    rstd = 1.0 / torch.sqrt(x.var(-1, unbiased=False) + 1e-5)
    xhat = (x - mean[:, None]) * rstd[:, None]
    return xhat * g + b, mean, rstd, xhat


def floor(got32, ref64):
    """max deviation of an fp32 CPU evaluation from float64, but never below what storing the float64 result in fp32 costs at the
    largest element (2^-24 max|ref|): on a launch of one row the measured deviation is a single sample and can fall below the
    format's own resolution, even to zero"""
    if ref64.numel() == 0:
        return 0.0
    return max(float((got32.double() - ref64).abs().max()), 2.0 ** -24 * float(ref64.abs().max()))


def ln_fwd_floor(x, g, b):
    """how far an fp32 CPU evaluation is from float64 at these inputs: (y of torch's F.layer_norm, mean, rstd), each as a max"""
    y64, m64, r64, _ = ln_ref64(x, g, b)
    y32 = F.layer_norm(x, (x.shape[-1],), g, b, 1e-5)
    m32 = x.mean(-1)
    r32 = 1.0 / torch.sqrt(x.var(-1, unbiased=False) + 1e-5)
    return floor(y32, y64), floor(m32, m64), floor(r32, r64)


def ln_case(dtype, d, rows, seed):
    x = q(rnd(rows, d, seed=seed, scale=1.5) + 0.3, dtype)
    g = 1.0 + 0.3 * rnd(d, seed=seed + 1)
    b = 0.2 * rnd(d, seed=seed + 2)
    return x, g, b


class FwdJob:
    """one forward job on the device: x rows, outputs in the mapped layout (the rows between the segments hold SENTINEL)"""

    def __init__(self, dtype, x, g, b, seg=None, stats=True):
        t = tdt(dtype)
        self.rows, self.d = x.shape
        self.x, self.g, self.b, self.seg = x, g, b, seg
        self.map, self.total = map_rows(self.rows, seg)
        self.xd, self.gd, self.bd = inp(x, t), inp(g, torch.float32), inp(b, torch.float32)
        yinit = torch.full((self.total, self.d), SENTINEL)
        yinit[self.map] = float("nan")
        self.y = Guard((self.total, self.d), t, init=yinit)
        sinit = torch.full((self.total,), SENTINEL)
        sinit[self.map] = float("nan")
        self.mean = Guard((self.total,), torch.float32, init=sinit) if stats else None
        self.rstd = Guard((self.total,), torch.float32, init=sinit) if stats else None

    def job(self):
        s = seg3(self.seg)
        return LnJob(x=self.xd.ptr, y=self.y.ptr, gamma=self.gd.ptr, beta=self.bd.ptr, mean=self.mean.ptr if self.mean else None,
                     rstd=self.rstd.ptr if self.rstd else None, rows=self.rows, d=self.d, seg=s[0], seg_stride=s[1], seg_off=s[2])

    def verify(self, dtype, what):
        if self.rows == 0:
            return
        y64, m64, r64, _ = ln_ref64(self.x, self.g, self.b)
        fy, fm, fr = ln_fwd_floor(self.x, self.g, self.b)
        other = torch.ones(self.total, dtype=torch.bool)
        other[self.map] = False
        y = self.y.get()
        assert bool((y[other] == SENTINEL).all()), f"{what}: rows between the segments were written"
        gate_check(f"{what} y", y[self.map], y64, 8 * fy + (UB * y64.abs() if dtype == BF16 else 0.0), "layernorm forward")
        if self.mean:
            mean, rstd = self.mean.get(), self.rstd.get()
            assert bool((mean[other] == SENTINEL).all()) and bool((rstd[other] == SENTINEL).all())
            gate_check(f"{what} mean", mean[self.map], m64, 8 * fm, "layernorm forward")
            gate_check(f"{what} rstd", rstd[self.map], r64, 8 * fr, "layernorm forward")


def run_fwd(dtype, jobs):
    arr = (LnJob * len(jobs))(*[j.job() for j in jobs])
    check(lib().mebt_op_layernorm_fwd_jobs(dtype, arr, len(jobs), cur_stream()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype,d", WIDTHS, ids=WIDTH_IDS)
def test_layernorm_forward_mapped_rows_and_inference_form(dtype, d):
    """rows = 10 through the map seg 5 / stride 9 / offset 3: y, mean and rstd land on rows 3..7 and 12..16, the rest keeps its
    sentinel; and the inference form (mean = rstd = NULL) at rows from {1, 5, 37}.
    Gates: 8 x the deviation of an fp32 CPU evaluation (torch's F.layer_norm; mean and rstd by the same formulas in fp32) from
    float64 at the same inputs, + UB |y| where y is stored as bf16."""
    j = FwdJob(dtype, *ln_case(dtype, d, 10, seed=d), seg=(5, 9, 3))
    run_fwd(dtype, [j])
    j.verify(dtype, f"ln_fwd mapped {NAMES[dtype]} d={d}")
    rows = {4: 37, 64: 1, 256: 1, 320: 5, 512: 5, 1024: 37, 2048: 1}[d]
    k = FwdJob(dtype, *ln_case(dtype, d, rows, seed=d + 7), stats=False)
    run_fwd(dtype, [k])
    k.verify(dtype, f"ln_fwd inference {NAMES[dtype]} d={d} rows={rows}")


@pytest.mark.parametrize("dtype,d", WIDTHS, ids=WIDTH_IDS)
def test_layernorm_forward_three_jobs_in_one_launch(dtype, d):
    """jobs of 5, 0, 37 and 1 rows at one width (three live: the fixed-chunk kernel at its widths); the last workgroup of each job
    has idle waves"""
    jobs = [FwdJob(dtype, *ln_case(dtype, d, r, seed=d + 11 * i), seg=(5, 9, 3) if i == 2 else None) for i, r in enumerate((5, 0, 37, 1))]
    run_fwd(dtype, jobs)
    for i, j in enumerate(jobs):
        j.verify(dtype, f"ln_fwd multi {NAMES[dtype]} d={d} job {i}")


def test_layernorm_forward_jobs_of_two_widths_take_the_generic_kernel():
    """a bf16 launch with d = 512 (a fixed-chunk width) and d = 320: no single chunk count fits, so the generic kernel runs both"""
    jobs = [FwdJob(BF16, *ln_case(BF16, 512, 5, seed=1)), FwdJob(BF16, *ln_case(BF16, 320, 37, seed=2)), FwdJob(BF16, *ln_case(BF16, 512, 1, seed=3))]
    run_fwd(BF16, jobs)
    for i, j in enumerate(jobs):
        j.verify(BF16, f"ln_fwd two widths job {i} d={j.d}")


def ln_bwd_ref64(x, dy, g):
    """float64 LayerNorm backward: dx, dgamma, dbeta and the absolute sums behind dgamma / dbeta"""
    _, _, rstd, xhat = ln_ref64(x, g, torch.zeros_like(g))
    dy, g = dy.double(), g.double()
    dyg = dy * g
    dx = rstd[:, None] * (dyg - dyg.mean(-1, keepdim=True) - xhat * (dyg * xhat).mean(-1, keepdim=True))
    return dx, (dy * xhat).sum(0), dy.sum(0), (dy.abs() * xhat.abs()).sum(0), dy.abs().sum(0)


def ln_bwd_floor(x, dy, g):
    """how far torch's fp32 CPU LayerNorm backward is from float64 at these inputs: max deviation of dx, dgamma, dbeta"""
    dx64, dg64, db64, _, _ = ln_bwd_ref64(x, dy, g)
    xr, gr, br = x.clone().requires_grad_(True), g.clone().requires_grad_(True), torch.zeros_like(g).requires_grad_(True)
    F.layer_norm(xr, (x.shape[-1],), gr, br, 1e-5).backward(dy)
    return floor(xr.grad, dx64), floor(gr.grad, dg64), floor(br.grad, db64)


class BwdJob:
    """one backward job.  dy, mean, rstd sit in the mapped layout (POISON between the segments), x / dy2 / dx_add / dx / dx2 at the
    plain row.  The statistics come from the forward entry point."""

    def __init__(self, dtype, d, rows, seed, seg=None, dy2=False, dx_add=False, accumulate=False, dx_f32=False, drop=None, dg=None, db=None):
        t = tdt(dtype)
        self.dtype, self.d, self.rows, self.seg = dtype, d, rows, seg
        self.x, self.g, b = ln_case(dtype, d, rows, seed)
        self.dy = q(rnd(rows, d, seed=seed + 3), dtype)
        self.dy2 = q(rnd(rows, d, seed=seed + 4, scale=0.7), dtype) if dy2 else None
        self.add = q(rnd(rows, d, seed=seed + 5, scale=2.0), dtype) if dx_add else None
        self.f32out = dtype == F32 or dx_f32
        self.out_t = torch.float32 if self.f32out else t
        self.old = rnd(rows, d, seed=seed + 6, scale=2.0).to(self.out_t).float() if accumulate else None
        self.fwd = FwdJob(dtype, self.x, self.g, b, seg=seg)
        self.map, self.total = self.fwd.map, self.fwd.total
        dym = torch.full((self.total, d), POISON)
        dym[self.map] = self.dy
        self.dyd = inp(dym, t)
        self.dy2d = inp(self.dy2, t) if dy2 else None
        self.addd = inp(self.add, t) if dx_add else None
        self.dx = Guard((rows, d), self.out_t, init=self.old)
        self.drop = drop
        self.dx2 = Guard((rows, d), self.out_t) if drop else None
        self.own_params = dg is None
        self.dg = dg if dg is not None else Guard((d,), torch.float32, init=torch.zeros(d))
        self.db = db if db is not None else Guard((d,), torch.float32, init=torch.zeros(d))

    def job(self):
        s = seg3(self.seg)
        j = LnJob(x=self.fwd.xd.ptr, dy=self.dyd.ptr, dy2=self.dy2d.ptr if self.dy2d else None, dx_add=self.addd.ptr if self.addd else None,
                  gamma=self.fwd.gd.ptr, mean=self.fwd.mean.ptr, rstd=self.fwd.rstd.ptr, dx=self.dx.ptr, dx2=self.dx2.ptr if self.dx2 else None,
                  dgamma=self.dg.ptr, dbeta=self.db.ptr, rows=self.rows, d=self.d, seg=s[0], seg_stride=s[1], seg_off=s[2],
                  dx_f32=int(self.f32out and self.dtype == BF16), dx_accumulate=int(self.old is not None))
        if self.drop:
            j.drop_seed, j.drop_site, j.drop_p = self.drop
        return j

    def upstream(self):
        return self.dy + (self.dy2 if self.dy2 is not None else 0.0)

    def verify_dx(self, what):
        """dx = LN'(dy + dy2) + (dx_add + old dx).  Gate: 8 x floor(torch's fp32 CPU backward against float64) + U32 |dx_add + old dx|
        (the addends are summed, then added, in fp32) + UB |dx| where dx is stored as bf16."""
        up = self.upstream()
        dx64 = ln_bwd_ref64(self.x, up, self.g)[0]
        extra = (self.add.double() if self.add is not None else 0.0) + (self.old.double() if self.old is not None else 0.0)
        ref = dx64 + extra
        fdx = ln_bwd_floor(self.x, up, self.g)[0]
        gate = 8 * fdx + U32 * torch.as_tensor(extra, dtype=torch.float64).abs() + (0.0 if self.f32out else UB * ref.abs())
        got = self.dx.get()
        gate_check(f"{what} dx", got, ref, gate, "layernorm backward dx")
        return got

    def param_terms(self):
        """(dgamma, dbeta, |.| sums, floors) of this job in float64"""
        up = self.upstream()
        _, dg, db, ag, ab = ln_bwd_ref64(self.x, up, self.g)
        _, fg, fb = ln_bwd_floor(self.x, up, self.g)
        return dg, db, ag, ab, fg, fb


def verify_params(what, jobs, dg, db, dg0, db0):
    """dgamma / dbeta = start + sum over the jobs.  Gate (the summation bound of test_gpu_vqgrad.py; it holds for any order of the
    atomics): 8 x floor + R U32 (sum_rows |dy + dy2| |xhat| + |start|), R = all rows of all jobs; the same with sum_rows |dy + dy2|
    for dbeta.  The start value is one more addend of the same sum."""
    rg, rb, ag, ab, fg, fb, R = dg0.double(), db0.double(), dg0.double().abs(), db0.double().abs(), 0.0, 0.0, 0
    for j in jobs:
        a, b, sa, sb, f1, f2 = j.param_terms()
        rg, rb, ag, ab, fg, fb, R = rg + a, rb + b, ag + sa, ab + sb, fg + f1, fb + f2, R + j.rows
    gate_check(f"{what} dgamma", dg.get(), rg, 8 * fg + R * U32 * ag, "layernorm backward dgamma / dbeta")
    gate_check(f"{what} dbeta", db.get(), rb, 8 * fb + R * U32 * ab, "layernorm backward dgamma / dbeta")


def run_bwd(dtype, jobs, colsums=None):
    run_fwd(dtype, [j.fwd for j in jobs])          # the statistics, in the mapped layout
    arr = (LnJob * len(jobs))(*[j.job() for j in jobs])
    cs = (ColsumItem * len(colsums))(*colsums) if colsums else None
    check(lib().mebt_op_layernorm_bwd_jobs(dtype, arr, len(jobs), cs, len(colsums) if colsums else 0, cur_stream()))
    torch.cuda.synchronize()


def single(dtype, d, rows, seed, what, **kw):
    j = BwdJob(dtype, d, rows, seed, **kw)
    run_bwd(dtype, [j])
    got = j.verify_dx(what)
    verify_params(what, [j], j.dg, j.db, torch.zeros(d), torch.zeros(d))
    return j, got


@pytest.mark.parametrize("dtype,d", WIDTHS, ids=WIDTH_IDS)
def test_layernorm_backward_plain_and_deterministic(dtype, d):
    """form (a) at 130 rows (the parameter part splits into chunks of 64 rows, the last with 2 rows: fewer than the 16 row lanes) and
    at 1 row; a second run gives the same bits of dx"""
    _, a = single(dtype, d, 130, d + 1, f"ln_bwd (a) {NAMES[dtype]} d={d} rows=130")
    _, b = single(dtype, d, 130, d + 1, f"ln_bwd (a) again {NAMES[dtype]} d={d}")
    assert torch.equal(a, b), "two runs of the same LayerNorm backward differ in dx"
    single(dtype, d, 1, d + 2, f"ln_bwd (a) {NAMES[dtype]} d={d} rows=1")


@pytest.mark.parametrize("dtype,d", WIDTHS, ids=WIDTH_IDS)
def test_layernorm_backward_addends_and_row_map(dtype, d):
    """forms (b) dy2 and dx_add together, (c) dx_accumulate onto a non-zero dx, (d) a bf16 job accumulating into an fp32 dx,
    (e) dy, mean and rstd through the row map (seg 5, stride 9, offset 3; 37 rows: the last segment is short) while x, dy2 and dx use
    the plain row"""
    n = NAMES[dtype]
    single(dtype, d, 37, d + 3, f"ln_bwd (b) {n} d={d}", dy2=True, dx_add=True)
    single(dtype, d, 5, d + 4, f"ln_bwd (c) {n} d={d}", accumulate=True)
    if dtype == BF16:
        single(dtype, d, 37, d + 5, f"ln_bwd (d) {n} d={d}", accumulate=True, dx_f32=True, dx_add=True)
    single(dtype, d, 37, d + 6, f"ln_bwd (e) {n} d={d}", seg=(5, 9, 3), dy2=True)


@pytest.mark.parametrize("dtype,d,dx_f32", [(BF16, 1024, 0), (BF16, 1024, 1), (BF16, 320, 0), (F32, 1024, 0), (F32, 320, 0)],
                         ids=["bf16-1024", "bf16-1024-dx_f32", "bf16-320", "f32-1024", "f32-320"])
def test_layernorm_backward_masked_second_output(dtype, d, dx_f32):
    """form (f): dx2 = stored dx x keep-scale of dropout site (seed, site, p = 0.25) at element row * d + e, rounded to dx's type,
    bit for bit.  bf16 at d = 1024 holds 8 elements per lane: both halves (mask index oi and oi + 4) are compared."""
    seed, site, p, rows = 0x1234567890ABCDEF, 17, 0.25, 37
    j, dx = single(dtype, d, rows, d + 8, f"ln_bwd (f) {NAMES[dtype]} d={d}", drop=(seed, site, p), dx_add=True, dx_f32=bool(dx_f32))
    mask = torch.ones(rows * d, device=DEV)
    check(lib().mebt_debug_dropout_mask(seed, site, p, rows * d, mask.data_ptr(), cur_stream()))
    torch.cuda.synchronize()
    mask = mask.cpu().view(rows, d)
    kept = float((mask != 0).float().mean())
    assert set(mask.unique().tolist()) == {0.0, float(np.float32(65536.0 / (65536.0 - 16384.0)))} and 0.70 < kept < 0.80, kept
    stored = j.dx.body.cpu()                         # in dx's type
    want = (stored.float() * mask).to(j.out_t)
    j.dx2.get()
    got = j.dx2.body.cpu()
    assert torch.equal(bits(got), bits(want)), f"dx2 differs from stored dx x mask at {int((bits(got) != bits(want)).sum())} elements"


def colsum_case(dtype, M, N, ldx, seed):
    X = q(rnd(M, N, seed=seed), dtype)
    Xp = torch.full((M, ldx), POISON)
    Xp[:, :N] = X
    out0 = rnd(N, seed=seed + 1)
    return X, inp(Xp, tdt(dtype)), out0, Guard((N,), torch.float32, init=out0)


def verify_colsum(what, X, out0, out):
    """gate per column: (M + 1) U32 (sum_m |X| + |out0|): M + 1 addends in fp32, in any order"""
    M = X.shape[0]
    ref = X.double().sum(0) + out0.double()
    gate_check(what, out.get(), ref, (M + 1) * U32 * (X.double().abs().sum(0) + out0.double().abs()), "column sums")


@pytest.mark.parametrize("dtype,d", WIDTHS, ids=WIDTH_IDS)
@pytest.mark.parametrize("with_colsums", [0, 1], ids=["g", "h"])
def test_layernorm_backward_three_jobs_share_dgamma(dtype, d, with_colsums):
    """forms (g) / (h): jobs of 130, 5 and 1 rows (and one of 0 rows) add into one dgamma / dbeta that start non-zero; (h): two
    grouped column sums ride on the same launch (ln_bwd_colsum_kernel)"""
    dg0, db0 = rnd(d, seed=d + 20), rnd(d, seed=d + 21)
    dg, db = Guard((d,), torch.float32, init=dg0), Guard((d,), torch.float32, init=db0)
    jobs = [BwdJob(dtype, d, 130, d + 30, dg=dg, db=db, dy2=True), BwdJob(dtype, d, 0, d + 31, dg=dg, db=db),
            BwdJob(dtype, d, 5, d + 32, dg=dg, db=db, seg=(5, 9, 3)), BwdJob(dtype, d, 1, d + 33, dg=dg, db=db, dx_add=True)]
    cases = [colsum_case(dtype, 37, 68, 72, d + 40), colsum_case(dtype, 130, 64, 64, d + 41)] if with_colsums else []
    items = [ColsumItem(X=c[1].ptr, out=c[3].ptr, M=c[0].shape[0], N=c[0].shape[1], ldx=c[1].body.shape[1]) for c in cases]
    run_bwd(dtype, jobs, items)
    what = f"ln_bwd ({'h' if with_colsums else 'g'}) {NAMES[dtype]} d={d}"
    for i, j in enumerate(jobs):
        if j.rows:
            j.verify_dx(f"{what} job {i}")
    verify_params(what, [j for j in jobs if j.rows], dg, db, dg0, db0)
    for i, c in enumerate(cases):
        verify_colsum(f"{what} colsum {i}", c[0], c[2], c[3])


# ------------------------------------------------------------------------------------------------
# column sums
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,N,ldx", [(1, 4, 4), (37, 68, 72), (130, 64, 64), (8200, 1024, 1024)])
def test_colsum(dtype, M, N, ldx):
    """out starts non-zero.  (37, 68, 72): a ragged last column group, POISON in the padding; (8200, 1024): the only small shape
    that keeps 512 rows per workgroup (ceil(8200 / 256) = 33 > 32 adders, and 16 x 17 workgroups fill the chip)"""
    X, Xd, out0, out = colsum_case(dtype, M, N, ldx, seed=M + N)
    check(lib().mebt_op_colsum(dtype, Xd.ptr, M, N, ldx, out.ptr, cur_stream()))
    torch.cuda.synchronize()
    verify_colsum(f"colsum {NAMES[dtype]} {M}x{N} ld {ldx}", X, out0, out)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_colsum_grouped(dtype):
    shapes = [(37, 68, 72), (0, 8, 8), (130, 64, 64), (300, 132, 132)]
    cases = [colsum_case(dtype, M, N, ld, seed=50 + i) if M else None for i, (M, N, ld) in enumerate(shapes)]
    dead = Guard((8,), torch.float32, init=torch.ones(8))
    items = [ColsumItem(X=c[1].ptr, out=c[3].ptr, M=M, N=N, ldx=ld) if c else ColsumItem(X=None, out=dead.ptr, M=0, N=N, ldx=ld)
             for c, (M, N, ld) in zip(cases, shapes)]
    check(lib().mebt_op_colsum_grouped(dtype, (ColsumItem * len(items))(*items), len(items), cur_stream()))
    torch.cuda.synchronize()
    for i, c in enumerate(cases):
        if c:
            verify_colsum(f"colsum grouped {NAMES[dtype]} item {i}", c[0], c[2], c[3])
    assert bool((dead.get() == 1.0).all())


# ------------------------------------------------------------------------------------------------
# masked-token loss
# ------------------------------------------------------------------------------------------------
CE_B, CE_NT, CE_N = 2, 4, 7
CE_V = [20, 1028, 4096, 16384]
CE_SC = float(np.float32(1.0 / 3.0))     # the scale and the smoothing reach the kernels as C floats: both sides use the rounded values


def f32(v):
    return float(np.float32(v))


@functools.lru_cache(maxsize=None)
def ce_case(V):
    """logits [8, V] = round(8 * 3 randn) / 8 (exact ties are frequent), targets placed by hand:
    row 0 the unique maximum; row 1 exactly 4 logits above; row 2 exactly 5 above; row 3 tied with an equal logit at a lower and one
    at a higher index; row 4 target 0; row 5 target V - 1; rows 6, 7 as drawn.  ti: distinct positions per sample; every other
    position of x_ids holds another id."""
    g = torch.Generator().manual_seed(V)
    rows = CE_B * CE_NT
    l = torch.round(8 * 3 * torch.randn(rows, V, generator=g)) / 8
    tgt = torch.randint(1, V - 1, (rows,), generator=g)
    tgt[3], tgt[4], tgt[5] = V // 2, 0, V - 1
    top = l.max(1).values
    l[0, tgt[0]] = top[0] + 1
    for r, k in ((1, 4), (2, 5)):
        others = [i for i in torch.argsort(l[r], descending=True).tolist() if i != int(tgt[r])][:k]
        l[r, tgt[r]] = top[r] + 0.5
        for n, i in enumerate(others):
            l[r, i] = top[r] + 1 + n
    l[3, tgt[3]] = l[3, 1] = l[3, V - 2] = top[3] + 1
    ti = torch.stack([torch.randperm(CE_N, generator=g)[:CE_NT] for _ in range(CE_B)])
    x_ids = torch.randint(0, V, (CE_B, CE_N), generator=g)
    for b in range(CE_B):
        for j in range(CE_NT):
            x_ids[b, ti[b, j]] = tgt[b * CE_NT + j]
    above = (l > l[torch.arange(rows), tgt][:, None]).sum(1)
    assert above[0] == 0 and above[1] == 4 and above[2] == 5 and above[3] == 0
    return l, tgt, ti, x_ids


def ce_ref64(l, tgt, eps, sc):
    rows, V = l.shape
    l64 = l.double()
    lse = torch.logsumexp(l64, 1)
    lt = l64[torch.arange(rows), tgt]
    loss = (1 - eps) * (lse - lt) + eps * (lse - l64.sum(1) / V)
    rank = (l > lt.float()[:, None]).sum(1) + ((l == lt.float()[:, None]) & (torch.arange(V)[None, :] < tgt[:, None])).sum(1)
    onehot = torch.zeros(rows, V, dtype=torch.float64)
    onehot[torch.arange(rows), tgt] = 1.0
    p = torch.exp(l64 - lse[:, None])
    dl = (p - (1 - eps) * onehot - eps / V) * sc
    return lse, lt, loss, rank, onehot, p, dl


def ce_gates(l, tgt, eps, sc):
    """gate_lse = U32 (|lse| + 2 R + V / 256 + 16), R = the row's max - min: |lse| covers the final add and the log, 2 R the
    argument rounding of __expf, V / 256 + 16 the per-thread chain and the block tree.
    gate_loss = gate_lse + U32 (|lse| + |lt| + 2 |loss|) + eps U32 (V / 256 + 16) mean|v|.
    gate_dl = |sc| (p (gate_lse + U32 (|v - lse| + 2)) + 2 U32 (p + onehot + eps / V))      (+ UB |dlogits| when stored as bf16)"""
    V = l.shape[1]
    lse, lt, loss, _, onehot, p, _ = ce_ref64(l, tgt, eps, sc)
    l64 = l.double()
    R = l64.max(1).values - l64.min(1).values
    g_lse = U32 * (lse.abs() + 2 * R + V / 256 + 16)
    g_loss = g_lse + U32 * (lse.abs() + lt.abs() + 2 * loss.abs()) + eps * U32 * (V / 256 + 16) * l64.abs().mean(1)
    g_dl = abs(sc) * (p * (g_lse[:, None] + U32 * ((l64 - lse[:, None]).abs() + 2)) + 2 * U32 * (p + onehot + eps / V))
    return g_lse, g_loss, g_dl


def ce_emulate(l, tgt, eps, sc, sign):
    """The loss kernels' arithmetic in fp32 on the CPU, in their summation order: thread t of 256 walks elements 4 t + 1024 c + q
    (c outer, q inner) for its running max, plain sum and exp sum; a wave is reduced by the xor butterfly (32, 16, .. 1), the four
    waves as ((w0 + w1) + w2) + w3.  __expf is modelled as the correctly rounded exponential of an argument that is off by one
    relative fp32 rounding, always in the direction `sign` (the worst case: every term's error has the same sign)."""
    f = np.float32
    rows, V = l.shape
    C_ = (V + 1023) // 1024
    a = np.full((rows, C_ * 1024), -np.inf, dtype=f)
    a[:, :V] = l.numpy()
    live = np.zeros((rows, C_ * 1024), dtype=bool)
    live[:, :V] = True
    a, live = a.reshape(rows, C_, 256, 4), live.reshape(rows, C_, 256, 4)

    def expf(x):
        return np.exp(x.astype(np.float64) * (1.0 + sign * 2.0 ** -24)).astype(f)

    def block(v, op):
        v = v.copy().reshape(rows, 4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            v = op(v, v[:, :, np.arange(64) ^ o])
        w = v[:, :, 0]
        return op(op(op(w[:, 0], w[:, 1]), w[:, 2]), w[:, 3])

    mx, sm = np.full((rows, 256), -np.inf, dtype=f), np.zeros((rows, 256), dtype=f)
    for c in range(C_):
        for k in range(4):
            ok = live[:, c, :, k]
            mx = np.where(ok, np.maximum(mx, a[:, c, :, k]), mx)
            sm = np.where(ok, sm + np.where(ok, a[:, c, :, k], f(0)), sm).astype(f)
    mxb = block(mx, np.maximum)
    se = np.zeros((rows, 256), dtype=f)
    for c in range(C_):
        for k in range(4):
            ok = live[:, c, :, k]
            se = np.where(ok, se + expf(np.where(ok, a[:, c, :, k], f(0)) - mxb[:, None]), se).astype(f)
    add = lambda x, y: (x + y).astype(f)
    seb, smb = block(se, add), block(sm, add)
    lse = (mxb + np.log(seb).astype(f)).astype(f)
    lt = l.numpy()[np.arange(rows), tgt.numpy()].astype(f)
    e = f(eps)
    loss = (((f(1) - e) * (lse - lt)).astype(f) + (e * (lse - (smb / f(V)).astype(f)).astype(f)).astype(f)).astype(f)
    onehot = np.zeros((rows, V), dtype=f)
    onehot[np.arange(rows), tgt.numpy()] = f(1) - e
    u = (e / f(V)).astype(f)
    dl = (((expf(l.numpy().astype(f) - lse[:, None]) - onehot).astype(f) - u).astype(f) * f(sc)).astype(f)
    return torch.from_numpy(lse), torch.from_numpy(loss), torch.from_numpy(dl)


@functools.lru_cache(maxsize=None)
def ce_emulation_ratios(V, eps):
    """worst emulated error / gate of (lse, loss, dlogits) over both signs of the injected __expf argument error"""
    l, tgt, _, _ = ce_case(V)
    sc, eps = CE_SC, f32(eps)
    lse64, _, loss64, _, _, _, dl64 = ce_ref64(l, tgt, eps, sc)
    g_lse, g_loss, g_dl = ce_gates(l, tgt, eps, sc)
    worst = [0.0, 0.0, 0.0]
    for sign in (-1.0, 1.0):
        lse, loss, dl = ce_emulate(l, tgt, eps, sc, sign)
        for i, (got, ref, gate) in enumerate(((lse, lse64, g_lse), (loss, loss64, g_loss), (dl, dl64, g_dl))):
            worst[i] = max(worst[i], float(((got.double() - ref).abs() / gate).max()))
    return tuple(worst)


def assert_ce_emulation_within_half_of_the_gates(V, eps):
    r = ce_emulation_ratios(V, eps)
    print(f"loss emulation V={V} eps={eps}: err / gate lse {r[0]:.3f}, loss {r[1]:.3f}, dlogits {r[2]:.3f}")
    assert max(r) <= 0.5, (V, eps, r)


def run_ce(V, eps, dl_dtype, sc):
    """mebt_op_cross_entropy; dl_dtype None: no dlogits"""
    l, tgt, ti, x_ids = ce_case(V)
    rows, eps = l.shape[0], f32(eps)
    ld, xd, td = inp(l, torch.float32), inp(x_ids, torch.int64), inp(ti, torch.int64)
    lse, loss = Guard((rows,), torch.float32), Guard((rows,), torch.float32)
    rank = Guard((rows,), torch.int32, init=-1, fill=-77)
    out4 = Guard((4,), torch.float64)
    dl = Guard((rows, V), tdt(dl_dtype), init=torch.full((rows, V), SENTINEL if V != 16384 else float("nan"))) if dl_dtype is not None else None
    check(lib().mebt_op_cross_entropy(ld.ptr, xd.ptr, td.ptr, CE_B, CE_N, CE_NT, V, eps, lse.ptr, loss.ptr, rank.ptr, out4.ptr,
                                      dl.ptr if dl else None, int(dl_dtype == BF16), sc, cur_stream()))
    torch.cuda.synchronize()
    return ld, xd, td, lse, loss, rank, out4, dl


def verify_ce_stats(what, V, eps, lse, loss, rank, out4):
    l, tgt, _, _ = ce_case(V)
    eps = f32(eps)
    lse64, _, loss64, rank64, _, _, _ = ce_ref64(l, tgt, eps, 1.0)
    g_lse, g_loss, _ = ce_gates(l, tgt, eps, 1.0)
    got_rank = rank.get()
    assert got_rank.tolist() == rank64.tolist(), (what, got_rank.tolist(), rank64.tolist())
    assert got_rank[0] == 0 and got_rank[1] == 4 and got_rank[2] == 5 and got_rank[3] == 1     # row 3: the equal logit at the lower index ranks above
    gate_check(f"{what} lse", lse.get(), lse64, g_lse, "loss")
    stored = loss.get()
    gate_check(f"{what} loss", stored, loss64, g_loss, "loss")
    o = out4.get()
    assert float(o[1]) == int((rank64 < 1).sum()) and float(o[2]) == int((rank64 < 5).sum()) and float(o[3]) == l.shape[0], o
    assert float(o[0]) == float(stored.sum()), (float(o[0]), float(stored.sum()))     # the float64 sum of the stored fp32 row losses


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("V", CE_V)
def test_cross_entropy_generic_kernel_and_backward(V, eps):
    """ce_fwd_kernel at every V (at V = 16384: because no dlogits is asked for), and ce_bwd_kernel in f32 and bf16 with `upstream`
    NULL and a device scalar, reading the row_lse the forward stored.  At V != 16384 a dlogits buffer passed to the forward is
    left untouched (the documented behaviour)."""
    assert_ce_emulation_within_half_of_the_gates(V, eps)
    what = f"ce V={V} eps={eps}"
    sc, eps = CE_SC, f32(eps)
    ld, xd, td, lse, loss, rank, out4, dl = run_ce(V, eps, F32 if V != 16384 else None, sc)
    verify_ce_stats(what, V, eps, lse, loss, rank, out4)
    if dl is not None:
        assert bool((dl.get() == SENTINEL).all()), "the forward wrote dlogits at a V its fused kernel does not take"
    l, tgt, _, _ = ce_case(V)
    rows = l.shape[0]
    for dtype, up in ((F32, None), (BF16, 0.75), (F32, -1.5), (BF16, None)):
        upd = inp(torch.tensor([up]), torch.float32) if up is not None else None
        total = sc * (up if up is not None else 1.0)
        out = Guard((rows, V), tdt(dtype))
        check(lib().mebt_op_cross_entropy_bwd(dtype, ld.ptr, xd.ptr, td.ptr, lse.ptr, upd.ptr if upd else None, sc, eps, out.ptr,
                                              CE_B, CE_N, CE_NT, V, cur_stream()))
        torch.cuda.synchronize()
        ref = ce_ref64(l, tgt, eps, total)[6]
        gate = ce_gates(l, tgt, eps, total)[2] + (UB * ref.abs() if dtype == BF16 else 0.0)
        gate_check(f"{what} ce_bwd {NAMES[dtype]} upstream {up}", out.get(), ref, gate, "loss gradient")


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("dl_dtype", [F32, BF16], ids=["f32", "bf16"])
def test_cross_entropy_fused_kernel(dl_dtype, eps):
    """V = 16384 with dlogits: ce_fused_kernel; its statistics meet the same gates as the generic kernel's"""
    V, sc = 16384, CE_SC
    assert_ce_emulation_within_half_of_the_gates(V, eps)
    what = f"ce fused {NAMES[dl_dtype]} eps={eps}"
    eps = f32(eps)
    _, _, _, lse, loss, rank, out4, dl = run_ce(V, eps, dl_dtype, sc)
    verify_ce_stats(what, V, eps, lse, loss, rank, out4)
    l, tgt, _, _ = ce_case(V)
    ref = ce_ref64(l, tgt, eps, sc)[6]
    gate = ce_gates(l, tgt, eps, sc)[2] + (UB * ref.abs() if dl_dtype == BF16 else 0.0)
    gate_check(f"{what} dlogits", dl.get(), ref, gate, "loss gradient")


# ------------------------------------------------------------------------------------------------
# AdamW
# ------------------------------------------------------------------------------------------------
LR, B1, B2, EPS = (float(np.float32(v)) for v in (1e-3, 0.9, 0.95, 1e-8))      # as the C floats they are passed as


def adamw_ref64(p, g, m, v, step, wd, gs):
    """adamw_update4 in float64.  Returns p, m, v and the update term lr / bc1 * m / denom"""
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    gj = g * gs
    p = p * (1.0 - LR * wd)
    m = B1 * m + (1.0 - B1) * gj
    v = B2 * v + (1.0 - B2) * gj * gj
    upd = LR / bc1 * (m / (torch.sqrt(v) / math.sqrt(bc2) + EPS))
    return p - upd, m, v, upd


def check_adamw_reference_against_torch():
    """the float64 formula above against torch.optim.AdamW in float64, once, on the CPU"""
    g = torch.Generator().manual_seed(5)
    for step, wd in ((1, 0.0), (1000, float(np.float32(0.01)))):
        p, gr, m = (torch.randn(64, generator=g, dtype=torch.float64) for _ in range(3))
        v = torch.rand(64, generator=g, dtype=torch.float64) * 0.1
        w = p.clone().requires_grad_(True)
        opt = torch.optim.AdamW([w], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd)
        w.grad = gr.clone()
        opt.state[w]["step"] = torch.tensor(float(step - 1))
        opt.state[w]["exp_avg"], opt.state[w]["exp_avg_sq"] = m.clone(), v.clone()
        opt.step()
        rp, rm, rv, _ = adamw_ref64(p, gr, m, v, step, wd, 1.0)
        assert float((w.detach() - rp).abs().max()) < 1e-14 and float((opt.state[w]["exp_avg"] - rm).abs().max()) < 1e-15
        assert float((opt.state[w]["exp_avg_sq"] - rv).abs().max()) < 1e-15


def test_adamw_reference_matches_torch():
    check_adamw_reference_against_torch()


@pytest.mark.parametrize("step,wd", [(1, 0.0), (1, 0.01), (1000, 0.0), (1000, 0.01)])
@pytest.mark.parametrize("form", ["f32", "bf16x1", "bf16x3"])
@pytest.mark.parametrize("n", [4, 1028, 4096 * 1024 + 1028])
def test_adamw(n, form, step, wd):
    """n = 4096 * 1024 + 1028 exceeds the 4096-workgroup cap: the grid-stride loop runs twice, the second time with a ragged tail.
    bf16x3: three bf16 gradient pieces at g_stride = n + 8 with POISON between them.
    Gates: m: 4 U32 (|b1 m| + |(1 - b1) g'|); v: 4 U32 (|b2 v| + |(1 - b2) g'^2|); p: 2 U32 |p| + 2^-20 lr / bc1 |m / denom| (the
    update term carries about a dozen fp32 roundings and the 1-ulp rsqrtf) + lr / bc1 gate_m / denom.  The last term is m's own
    absolute error carried into the update: where b1 m and (1 - b1) g' cancel, that error is large against |m|, which the relative
    term cannot see (among 4 M elements a plain fp32 evaluation of the formula on the CPU reaches 1.97 x the gate without it, the
    same figure the kernel gave, and 0.25 x the gate with it).  The bf16 mirror is the stored p rounded to bf16."""
    wd = float(np.float32(wd))
    gs = float(np.float32(1.0 / 3.0))
    pieces = {"f32": 1, "bf16x1": 1, "bf16x3": 3}[form]
    gt = torch.float32 if form == "f32" else torch.bfloat16
    stride = n + 8 if pieces > 1 else n
    p0, m0 = rnd(n, seed=n + step), rnd(n, seed=n + step + 1, scale=0.1)
    v0 = torch.rand(n, generator=torch.Generator().manual_seed(n + step + 2)) * 0.01
    gp = rnd(pieces, n, seed=n + step + 3).to(gt)
    gbuf = torch.full((pieces, stride), POISON, dtype=gt)
    gbuf[:, :n] = gp
    gd = inp(gbuf, gt)
    pd, md, vd = Guard((n,), torch.float32, init=p0), Guard((n,), torch.float32, init=m0), Guard((n,), torch.float32, init=v0)
    mirror = Guard((n,), torch.bfloat16) if form != "f32" else None
    check(lib().mebt_op_adamw(pd.ptr, gd.ptr, md.ptr, vd.ptr, mirror.ptr if mirror else None, n, LR, B1, B2, EPS, wd, step, gs,
                              int(form != "f32"), pieces, stride, cur_stream()))
    torch.cuda.synchronize()
    g64 = gp.double().sum(0)
    rp, rm, rv, upd = adamw_ref64(p0.double(), g64, m0.double(), v0.double(), step, wd, gs)
    gj = g64 * gs
    what = f"adamw n={n} {form} step={step} wd={wd:g}"
    gate_m = 4 * U32 * ((B1 * m0.double()).abs() + ((1 - B1) * gj).abs())
    denom = torch.sqrt(rv) / math.sqrt(1.0 - B2 ** step) + EPS
    gate_check(f"{what} m", md.get(), rm, gate_m, "adamw")
    gate_check(f"{what} v", vd.get(), rv, 4 * U32 * ((B2 * v0.double()).abs() + (1 - B2) * gj * gj), "adamw")
    gate_check(f"{what} p", pd.get(), rp, 2 * U32 * rp.abs() + 2.0 ** -20 * upd.abs() + LR / (1.0 - B1 ** step) * gate_m / denom, "adamw")
    if mirror:
        mirror.get()
        assert torch.equal(bits(mirror.body.cpu()), bits(pd.body.cpu().to(torch.bfloat16))), "the bf16 mirror is not the stored p rounded to bf16"


# ------------------------------------------------------------------------------------------------
# embedding backward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [4, 64, 320])
@pytest.mark.parametrize("NC,NT", [(5, 4), (0, 4), (5, 0)])
def test_embed_bwd(dtype, d, NC, NT):
    """B = 2, N = 12, NS = 2; tokens from 6 ids, so several rows add into one g_tok_emb row; all four gradient buffers start
    non-zero.  Reference: float64 index_add and column sums.  Gate per element: (K + 1) U32 (sum |addends| + |start|), K the number
    of addends of that element."""
    B, N, NS, V = 2, 12, 2, 6
    t = tdt(dtype)
    g = torch.Generator().manual_seed(d + NC)
    x_ids = torch.randint(0, V, (B, N), generator=g)
    perm = torch.stack([torch.randperm(N, generator=g) for _ in range(B)])
    ci, ti = perm[:, :NC].contiguous(), perm[:, NC:NC + NT].contiguous()
    g_ctx = rnd(B, NC, d, seed=d + 1)
    g_tgt, g_sos = q(rnd(B, NT, d, seed=d + 2), dtype), q(rnd(B, NS, d, seed=d + 3), dtype)
    start = [rnd(V, d, seed=d + 4), rnd(N, d, seed=d + 5), rnd(d, seed=d + 6), rnd(NS, d, seed=d + 7)]
    bufs = [Guard(s.shape, torch.float32, init=s) for s in start]
    ins = [inp(x_ids, torch.int64), inp(ci, torch.int64), inp(ti, torch.int64), inp(g_ctx, torch.float32), inp(g_tgt, t), inp(g_sos, t)]
    check(lib().mebt_op_embed_bwd(dtype, *[i.ptr for i in ins], *[b.ptr for b in bufs], B, N, NC, NT, NS, d, cur_stream()))
    torch.cuda.synchronize()
    ref = [s.double().clone() for s in start]
    mag = [s.double().abs() for s in start]
    cnt = [torch.zeros(V, 1), torch.zeros(N, 1), torch.full((1,), float(B * NT)), torch.full((1, 1), float(B))]
    def add(k, i, v):
        ref[k][i] += v.double()
        mag[k][i] += v.double().abs()
        cnt[k][i] += 1

    for b in range(B):
        for r in range(NC):
            pos = int(ci[b, r])
            add(0, int(x_ids[b, pos]), g_ctx[b, r])
            add(1, pos, g_ctx[b, r])
        for j in range(NT):
            add(1, int(ti[b, j]), g_tgt[b, j])
    ref[2] += g_tgt.double().sum((0, 1))
    mag[2] += g_tgt.double().abs().sum((0, 1))
    ref[3] += g_sos.double().sum(0)
    mag[3] += g_sos.double().abs().sum(0)
    for k, name in enumerate(("g_tok_emb", "g_pos_emb", "g_mask_emb", "g_sos_emb")):
        gate_check(f"embed_bwd {NAMES[dtype]} d={d} NC={NC} NT={NT} {name}", bufs[k].get(), ref[k], (cnt[k].double() + 1) * U32 * mag[k], "embedding backward")


# ------------------------------------------------------------------------------------------------
# row movers (bit-exact)
# ------------------------------------------------------------------------------------------------
def run_copy_rows(src_t, dst_t, rows, d, s_seg, d_seg, seed):
    smap, stotal = map_rows(rows, s_seg)
    dmap, dtotal = map_rows(rows, d_seg)
    vals = rnd(rows, d, seed=seed, scale=3.0).to(src_t)
    src = torch.full((stotal, d), POISON, dtype=src_t)
    src[smap] = vals
    sd = inp(src, src_t)
    dst = Guard((dtotal, d), dst_t, init=torch.full((dtotal, d), SENTINEL))
    s, dd = seg3(s_seg), seg3(d_seg)
    check(lib().mebt_op_copy_rows(sd.ptr, dst.ptr, rows, d, int(src_t == torch.float32), int(dst_t == torch.float32), *s, *dd, cur_stream()))
    torch.cuda.synchronize()
    dst.get()
    got = dst.body.cpu()
    want = torch.full((dtotal, d), SENTINEL, dtype=dst_t)
    want[dmap] = vals.to(dst_t)                   # torch's conversion: round to nearest even
    assert torch.equal(bits(got), bits(want)), f"copy_rows: {int((bits(got) != bits(want)).sum())} elements differ"


@pytest.mark.parametrize("src_t,dst_t", [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32),
                                         (torch.bfloat16, torch.bfloat16)], ids=["f32-f32", "f32-bf16", "bf16-f32", "bf16-bf16"])
@pytest.mark.parametrize("s_seg,d_seg", [(None, None), ((5, 9, 3), None), (None, (4, 6, 1)), ((5, 9, 3), (4, 6, 1))], ids=["plain", "src-map", "dst-map", "both"])
def test_copy_rows(src_t, dst_t, s_seg, d_seg):
    """37 rows of 68 elements through a source map, a destination map and both; the rows between the destination's segments keep
    their sentinel; f32 -> bf16 is torch's round to nearest even"""
    run_copy_rows(src_t, dst_t, 37, 68, s_seg, d_seg, seed=3)


def test_copy_rows_past_the_grid_cap():
    """2100 rows x 4096: 2.15 M vectors, past the 8192 workgroups x 256 threads of one pass"""
    run_copy_rows(torch.float32, torch.bfloat16, 2100, 4096, None, (100, 101, 1), seed=4)


@pytest.mark.parametrize("row_bytes", [16, 1040])
@pytest.mark.parametrize("scatter", [0, 1], ids=["gather", "scatter"])
def test_index_rows(row_bytes, scatter):
    """B = 2, n = 5, npos = 9; row_bytes = 1040: a second pass with one live lane.  One position is -1 and one is npos: their
    destination rows keep the sentinel (and nothing is read for them)."""
    B, n, npos, w = 2, 5, 9, row_bytes // 4
    g = torch.Generator().manual_seed(row_bytes + scatter)
    idx = torch.stack([torch.randperm(npos, generator=g)[:n] for _ in range(B)])
    idx[0, 2], idx[1, 4] = -1, npos
    src_rows, dst_rows = (n, npos) if scatter else (npos, n)
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, src_rows, w), generator=g, dtype=torch.int64).to(torch.int32)
    sd = inp(src, torch.int32)
    dst = Guard((B, dst_rows, w), torch.int32, init=-77, fill=-77)
    idxd = inp(idx, torch.int64)
    check(lib().mebt_op_index_rows(sd.ptr, dst.ptr, idxd.ptr, B, n, npos, row_bytes, scatter, cur_stream()))
    torch.cuda.synchronize()
    want = torch.full((B, dst_rows, w), -77, dtype=torch.int32)
    for b in range(B):
        for j in range(n):
            pos = int(idx[b, j])
            if 0 <= pos < npos:
                if scatter:
                    want[b, pos] = src[b, j]
                else:
                    want[b, j] = src[b, pos]
    assert torch.equal(dst.get(), want)
