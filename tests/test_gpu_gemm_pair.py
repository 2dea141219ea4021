"""The pair launch of the bf16 GEMM family (two independent products in one grid: the q and k|v projections of a block, forward and
dgrad) through mebt_op_gemm_pair, every entry of its kernel table forced with mebt_debug_pair_config, and the kernel that really ran
read back with mebt_debug_gemm_last_launch.  GPU only.

Reference everywhere: the fp64 product of small-integer operands ([-3, 3], K <= 320: |sum| <= 2880, far below 2^24, so the fp32
accumulation, the integer bias and the integer residual are exact).  The bf16 output is therefore the bf16 rounding of the reference bit
for bit: torch.equal, no tolerance.  Outputs sit in buffers prefilled with a sentinel (padding columns, a guard row behind the last
row) that has to survive."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from mebt_amd import _lib
from mebt_amd._lib import cur_stream
from tests.test_gpu_ops import DEV, SENTINEL, MEBT_STATUS_EINVAL, OutBuf, assert_ran, bf16_round, last_launch, lib, rnd, strided

BF = torch.bfloat16

# the pair table (gemm_layout.inc), entry by entry: if the table and this list drift apart, a case here fails
PAIR_TABLE = [(192, 128, 2), (192, 128, 3), (128, 128, 2), (128, 128, 3), (128, 128, 4), (96, 128, 2), (96, 128, 3), (96, 128, 4),
              (128, 64, 2), (128, 64, 3), (128, 64, 4), (64, 128, 2), (64, 128, 3), (64, 128, 4), (96, 64, 2), (96, 64, 3),
              (96, 64, 4), (64, 64, 2), (64, 64, 3), (64, 64, 4)]


class Prod:
    """one product of a pair: operands on the device, the fp64 reference, and where the output goes.
    lda = 2 K: A is the second column half of a [M, 2 K] buffer whose first half holds other integers; out = (buffer, column): C is a
    column block of a shared OutBuf instead of a buffer of its own with ldc = N + 8."""

    def __init__(self, M, N, K, b_kc, seed, bias=False, epilogue=_lib.EPI_NONE, wide_a=False, c_f32=0, out=None):
        self.M, self.N, self.K, self.epilogue, self.c_f32 = M, N, K, epilogue, c_f32
        Am, Bm = rnd(M, K, seed=seed, ints=True), rnd(N, K, seed=seed + 1, ints=True)
        self.ref = Am.double() @ Bm.double().t()
        if wide_a:
            both = torch.cat([rnd(M, K, seed=seed + 2, ints=True), Am], dim=1)
            self.keepA, base = strided(both, 2 * K, BF)
            self.A, self.lda = base + K * 2, 2 * K
        else:
            self.keepA, self.A = strided(Am, K, BF)
            self.lda = K
        Bs = Bm if b_kc else Bm.t().contiguous()
        self.keepB, self.B = strided(Bs, Bs.shape[1], BF)
        self.ldb = Bs.shape[1]
        self.bias = None
        if bias:
            b = rnd(N, seed=seed + 3, ints=True)
            self.bias = b.to(DEV)
            self.ref = self.ref + b.double()
        self.aux, self.ld_aux = None, 0
        if epilogue == _lib.EPI_RESID:
            x = rnd(M, N, seed=seed + 4, ints=True)
            self.ld_aux = N + 8
            self.keepX, self.aux = strided(x, self.ld_aux, BF)
            self.ref = self.ref + x.double()
        self.shared = out is not None
        if self.shared:
            self.buf, col = out
            self.C, self.ldc = self.buf.ptr + col * 2, self.buf.ld
        else:
            self.buf = OutBuf(M, N, N + 8, 0, torch.float32 if c_f32 else BF)
            self.C, self.ldc = self.buf.ptr, N + 8

    def expected(self):
        return self.ref if self.c_f32 else bf16_round(self.ref)

    def check(self):
        got = self.buf.result().double()
        assert torch.equal(got, self.expected()), (got - self.expected()).abs().max()


def launch_pair(p0, p1, b_kc):
    vp = lambda *v: (ctypes.c_void_p * 2)(*v)
    i2 = lambda name: (ctypes.c_int32 * 2)(getattr(p0, name), getattr(p1, name))
    bias = vp(*(p.bias.data_ptr() if p.bias is not None else None for p in (p0, p1)))
    st = lib().mebt_op_gemm_pair(vp(p0.A, p1.A), vp(p0.B, p1.B), vp(p0.C, p1.C), bias, vp(p0.aux, p1.aux), i2("M"), i2("N"), i2("K"),
                                 i2("lda"), i2("ldb"), i2("ldc"), i2("ld_aux"), i2("epilogue"), i2("c_f32"), b_kc, cur_stream())
    torch.cuda.synchronize()
    return st


def tiles_of(p, tbm, tbn):
    return -(-p.M // tbm) * -(-p.N // tbn)


def run_forced(p0, p1, b_kc, cfg):
    """the pair under the forced table entry cfg = (tbm, tbn, ring): one launch of that kernel on a grid of both products' tiles"""
    tbm, tbn, ring = cfg
    lib().mebt_debug_pair_config(tbm, tbn, ring)
    last_launch()
    try:
        st = launch_pair(p0, p1, b_kc)
    finally:
        lib().mebt_debug_pair_config(0, 0, 0)
    _lib.check(st)
    k = assert_ran((tbm, tbn), ring, family=1)
    assert (k["threads"], k["gx"], k["gy"], k["gz"]) == (256, tiles_of(p0, tbm, tbn) + tiles_of(p1, tbm, tbn), 1, 1), k


@pytest.mark.parametrize("b_kc", [1, 0])
@pytest.mark.parametrize("cfg", PAIR_TABLE, ids=lambda c: "%dx%dr%d" % c)
def test_pair_every_table_entry(cfg, b_kc):
    """all 20 (tile, ring) entries x both B layouts: different M, N and K per product, ragged against every tile, product 1 smaller
    than the largest tile"""
    p0, p1 = Prod(328, 200, 192, b_kc, seed=101), Prod(72, 264, 320, b_kc, seed=111)
    run_forced(p0, p1, b_kc, cfg)
    p0.check()
    p1.check()


@pytest.mark.parametrize("cfg", [(96, 128, 3), (64, 64, 2)], ids=lambda c: "%dx%dr%d" % c)
def test_pair_forward_form_of_the_engine(cfg):
    """q and k|v projections: fp32 bias, no epilogue, B k-contiguous, the outputs column blocks of ONE wider buffer (ldc = N0 + N1);
    the rows of the block of the shorter product that it does not own stay untouched"""
    M0, M1, N0, N1 = 328, 72, 136, 264
    out = OutBuf(M0, N0 + N1, N0 + N1, 0, BF, init=torch.full((M0, N0 + N1), SENTINEL))
    p0 = Prod(M0, N0, 128, 1, seed=121, bias=True, out=(out, 0))
    p1 = Prod(M1, N1, 192, 1, seed=131, bias=True, out=(out, N0))
    run_forced(p0, p1, 1, cfg)
    want = torch.full((M0, N0 + N1), SENTINEL, dtype=torch.float64)
    want[:, :N0] = p0.expected()
    want[:M1, N0:] = p1.expected()
    assert torch.equal(out.result().double(), want)


@pytest.mark.parametrize("cfg", [(96, 128, 3), (64, 64, 2)], ids=lambda c: "%dx%dr%d" % c)
def test_pair_backward_form_of_the_engine(cfg):
    """the dgrads: B row-contiguous; product 0 reads A as a column half of a wider buffer (lda = 2 K), product 1 adds an integer
    residual read at ld_aux = N + 8"""
    p0 = Prod(328, 200, 192, 0, seed=141, wide_a=True)
    p1 = Prod(72, 264, 320, 0, seed=151, epilogue=_lib.EPI_RESID)
    run_forced(p0, p1, 0, cfg)
    p0.check()
    p1.check()


@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("b_kc", [1, 0])
@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("cfg,big,small", [((64, 64, 2), (512, 256), (192, 192)), ((128, 128, 2), (512, 512), (384, 128))], ids=["64x64", "128x128"])
def test_pair_tile_order(cfg, big, small, K, b_kc, swapped):
    """the XCD-aware tile order inside each product of the grid: a tile count of whole XCD sub-grids (32 / 16 tiles) next to one that
    is no multiple of 8 (9 / 3 tiles: the contiguous-run order), in both positions of the pair, at the prologue-only k-tile counts of the
    ring (K = 64, 128)"""
    pb, ps = Prod(*big, K, b_kc, seed=161), Prod(*small, K, b_kc, seed=171)
    p0, p1 = (ps, pb) if swapped else (pb, ps)
    run_forced(p0, p1, b_kc, cfg)
    p0.check()
    p1.check()


@pytest.mark.parametrize("b_kc", [1, 0])
@pytest.mark.parametrize("M1", [4, 36])
@pytest.mark.parametrize("cfg", [(192, 128, 2), (64, 64, 4)], ids=lambda c: "%dx%dr%d" % c)
def test_pair_few_rows(cfg, M1, b_kc):
    """row counts of the sampling loops: product 1 has far fewer rows than a tile (4) or a ragged handful (36)"""
    p0, p1 = Prod(328, 200, 192, b_kc, seed=181), Prod(M1, 264, 320, b_kc, seed=191)
    run_forced(p0, p1, b_kc, cfg)
    p0.check()
    p1.check()


def test_pair_forced_tile_without_kernel_is_rejected():
    """a forced 256 x 128 (no pair kernel has that tile) fails with MEBT_STATUS_EINVAL naming the tile, launches nothing and writes nothing"""
    p0, p1 = Prod(328, 200, 192, 1, seed=201), Prod(72, 264, 320, 1, seed=211)
    for p in (p0, p1):
        p.buf.body()[:] = SENTINEL
    lib().mebt_debug_pair_config(256, 128, 2)
    last_launch()
    try:
        st = launch_pair(p0, p1, 1)
    finally:
        lib().mebt_debug_pair_config(0, 0, 0)
    assert st == MEBT_STATUS_EINVAL and b"gemm pair" in lib().mebt_last_error() and b"256 x 128" in lib().mebt_last_error()
    assert last_launch()[0] == 0
    for p in (p0, p1):
        assert bool((p.buf.flat == SENTINEL).all())


@pytest.mark.parametrize("which", [0, 1])
def test_pair_products_that_do_not_qualify_launch_separately(which):
    """an fp32 output on one product: not a pair, even with a pair configuration forced; two single-product launches, both exact"""
    p0 = Prod(328, 200, 192, 1, seed=221, c_f32=int(which == 0))
    p1 = Prod(72, 264, 320, 1, seed=231, c_f32=int(which == 1))
    lib().mebt_debug_pair_config(64, 64, 2)
    last_launch()
    try:
        st = launch_pair(p0, p1, 1)
    finally:
        lib().mebt_debug_pair_config(0, 0, 0)
    _lib.check(st)
    n, k = last_launch()
    assert (n, k["family"]) == (2, 0), (n, k)
    p0.check()
    p1.check()


def test_pair_tune_table_lines_choose_the_launch():
    """the tune table -> pair path: the key holds the bucketed M of both products (row counts just above 128 and just below 256 share a
    line), a value is a packed GemmConfig of the pair table and 0 means "launch separately"; without a line the default is 96 x 128 ring 3.
    N0 = 136 / N1 = 264 is a signature the shipped table cannot hold (its widths are multiples of 128)."""
    N0, N1, K0, K1, M1 = 136, 264, 128, 192, 72
    key = f"7 {0x20000000 | 1} 256 {N0} 128 {M1} {N1} 256"          # kind | b_kc, then (bucketed M, N, bucketed K) of both products
    saved = _lib.tune_table_text()
    version = saved.splitlines()[0]                                 # "1 -1 <MEBT_TUNE_VERSION>": a text of another version is ignored as a whole
    assert f" {N0} 128 {M1} {N1} 256 " not in saved

    def run(M0):
        p0, p1 = Prod(M0, N0, K0, 1, seed=241), Prod(M1, N1, K1, 1, seed=251)
        last_launch()
        _lib.check(launch_pair(p0, p1, 1))
        got = last_launch()
        p0.check()
        p1.check()
        return got, tiles_of(p0, 64, 128) + tiles_of(p1, 64, 128), tiles_of(p0, 96, 128) + tiles_of(p1, 96, 128)

    try:
        for M0 in (136, 248):
            (n, k), _, t96 = run(M0)
            assert (n, k["family"], k["tbm"], k["tbn"], k["code"], k["gx"]) == (1, 1, 96, 128, 3, t96), (M0, n, k)
        assert _lib.tune_table_merge(f"{version}\n{key} {(64 << 20) | (128 << 8) | 4}\n", overwrite=True) == 1
        for M0 in (136, 248):
            (n, k), t64, _ = run(M0)
            assert (n, k["family"], k["tbm"], k["tbn"], k["code"], k["gx"]) == (1, 1, 64, 128, 4, t64), (M0, n, k)
        assert _lib.tune_table_merge(f"{version}\n{key} 0\n", overwrite=True) == 1
        for M0 in (136, 248):
            (n, k), _, _ = run(M0)
            assert (n, k["family"]) == (2, 0), (M0, n, k)
    finally:
        _lib.tune_table_merge(saved, replace=True)
    assert _lib.tune_table_text() == saved
