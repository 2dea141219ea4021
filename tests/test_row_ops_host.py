"""Host side of the row-kernel entry points (mebt_op_layernorm_*_jobs, mebt_op_colsum*, mebt_op_cross_entropy*, mebt_op_adamw,
mebt_op_embed_bwd, mebt_op_copy_rows, mebt_op_index_rows): exported symbols, the ctypes mirrors of their structs, and that every
refusal and every empty shape is decided before the first HIP call — none of this needs a device, and none of the dummy pointers
passed here is ever dereferenced."""
import ctypes as C
import os
import re

import pytest

from mebt_amd import _lib
from mebt_amd._lib import LnJob, ColsumItem, F32, BF16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ESHAPE, EDTYPE = 0, 1, 2, 5
DUMMY = 0x1000            # a non-null address that nothing reads: these calls return before any launch
NEW = ["mebt_op_layernorm_fwd_jobs", "mebt_op_layernorm_bwd_jobs", "mebt_op_colsum", "mebt_op_colsum_grouped", "mebt_op_cross_entropy",
       "mebt_op_cross_entropy_bwd", "mebt_op_adamw", "mebt_op_embed_bwd", "mebt_op_copy_rows", "mebt_op_index_rows"]


@pytest.fixture(scope="module")
def lib():
    """the library with the prototypes bound, without _lib.load() (which would merge the tune table: not needed here)"""
    assert os.path.exists(_lib.LIB_PATH), "build the library first: python -c 'import __graft_entry__ as g; g.build()'"
    l = C.CDLL(_lib.LIB_PATH)
    for name in NEW + ["mebt_last_error", "mebt_abi_version"]:
        fn = getattr(l, name)
        fn.restype, fn.argtypes = _lib.PROTOTYPES[name]
    return l


def refused(lib, status, want, word):
    msg = lib.mebt_last_error()
    assert status == want and msg and word.encode() in msg, (status, want, msg)


def test_library_exports_the_row_operators(lib):
    hdr = open(os.path.join(ROOT, "include", "mebt_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.PROTOTYPES and re.search(r"\b%s\s*\(" % name, hdr), name
    assert lib.mebt_abi_version() == 2
    assert "#define MEBT_LN_MAX_JOBS 3" in hdr and _lib.MEBT_LN_MAX_JOBS == 3


CTYPE = {"const void*": C.c_void_p, "void*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "int32_t": C.c_int32,
         "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "float": C.c_float}


def header_struct(name):
    """a ctypes.Structure built from the field list of `typedef struct <name> { ... } <name>;` in the header (one type per
    declaration, several names allowed), laid out by the same C rules the compiler applies"""
    hdr = open(os.path.join(ROOT, "include", "mebt_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (s.strip() for s in body.split(";"))):
        m = re.fullmatch(r"((?:const )?\w+\*?)\s+(.+)", decl)
        assert m and m.group(1) in CTYPE, decl
        fields += [(n.strip(), CTYPE[m.group(1)]) for n in m.group(2).split(",")]
    return type("H_" + name, (C.Structure,), {"_fields_": fields})


@pytest.mark.parametrize("name,mirror", [("mebt_ln_job", LnJob), ("mebt_colsum_item", ColsumItem)])
def test_ctypes_mirrors_have_the_headers_layout(name, mirror):
    H = header_struct(name)
    assert C.sizeof(mirror) == C.sizeof(H) and C.sizeof(H) % 8 == 0
    assert [(n, getattr(mirror, n).offset, getattr(mirror, n).size) for n, _ in mirror._fields_] == \
           [(n, getattr(H, n).offset, getattr(H, n).size) for n, _ in H._fields_]
    if mirror is LnJob:
        assert C.sizeof(LnJob) == 152 and LnJob.drop_seed.offset == 136 and LnJob.rows.offset == 104


def fwd_job(rows=4, d=64, **kw):
    j = LnJob(x=DUMMY, y=DUMMY, gamma=DUMMY, beta=DUMMY, mean=DUMMY, rstd=DUMMY, rows=rows, d=d)
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def bwd_job(rows=4, d=64, **kw):
    j = LnJob(x=DUMMY, dy=DUMMY, gamma=DUMMY, mean=DUMMY, rstd=DUMMY, dx=DUMMY, dgamma=DUMMY, dbeta=DUMMY, rows=rows, d=d)
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def jobs(*js):
    return (LnJob * len(js))(*js), len(js)


def test_layernorm_jobs_refusals_and_empty_launches(lib):
    fwd = lambda dt, *js: lib.mebt_op_layernorm_fwd_jobs(dt, *jobs(*js), None)
    bwd = lambda dt, *js: lib.mebt_op_layernorm_bwd_jobs(dt, *jobs(*js), None, 0, None)
    refused(lib, fwd(7, fwd_job()), EDTYPE, "dtype")
    refused(lib, bwd(-1, bwd_job()), EDTYPE, "dtype")
    refused(lib, lib.mebt_op_layernorm_fwd_jobs(F32, None, 1, None), EINVAL, "job list")
    refused(lib, lib.mebt_op_layernorm_bwd_jobs(F32, None, 2, None, 0, None), EINVAL, "job list")
    for f in ("x", "y", "gamma", "beta", "rstd"):        # rstd alone: mean and rstd go together
        refused(lib, fwd(BF16, fwd_job(**{f: None})), EINVAL, "null")
    for f in ("x", "dy", "gamma", "mean", "rstd", "dx", "dgamma", "dbeta"):
        refused(lib, bwd(F32, bwd_job(**{f: None})), EINVAL, "null")
    for d in (6, 2050, 2052, 0):
        refused(lib, fwd(F32, fwd_job(d=d)), ESHAPE, "multiple of 4")
        refused(lib, bwd(BF16, bwd_job(d=d)), ESHAPE, "multiple of 4")
    refused(lib, fwd(F32, fwd_job(seg=5, seg_stride=4)), ESHAPE, "row map")
    refused(lib, bwd(F32, bwd_job(drop_p=1.0, dx2=DUMMY)), EINVAL, "drop_p")
    # a fourth live job is refused; jobs without rows do not count
    refused(lib, fwd(F32, fwd_job(), fwd_job(), fwd_job(), fwd_job()), EINVAL, "too many")
    refused(lib, bwd(F32, bwd_job(), bwd_job(), bwd_job(), bwd_job(rows=1)), EINVAL, "too many")
    refused(lib, fwd(F32, fwd_job(), fwd_job(rows=0), fwd_job(), fwd_job(), fwd_job(d=6)), EINVAL, "too many")
    refused(lib, fwd(F32, fwd_job(), fwd_job(rows=0), fwd_job(), fwd_job(rows=0), fwd_job(d=6)), ESHAPE, "multiple of 4")   # three live: gets as far as the third's width
    # nothing live: 0, whatever the dead jobs hold
    assert fwd(F32, fwd_job(rows=0, d=7, x=None)) == OK and bwd(BF16, bwd_job(rows=0, d=7, dy=None), bwd_job(rows=-3)) == OK
    assert lib.mebt_op_layernorm_fwd_jobs(F32, None, 0, None) == OK and lib.mebt_op_layernorm_bwd_jobs(F32, None, 0, None, 0, None) == OK
    # the column sums that ride on the backward are checked too, before the launch
    cs = (ColsumItem * 1)(ColsumItem(X=DUMMY, out=DUMMY, M=3, N=6, ldx=8))
    refused(lib, lib.mebt_op_layernorm_bwd_jobs(F32, *jobs(bwd_job()), cs, 1, None), ESHAPE, "multiples of 4")
    refused(lib, lib.mebt_op_layernorm_bwd_jobs(F32, *jobs(bwd_job()), None, 1, None), EINVAL, "item list")
    refused(lib, lib.mebt_op_layernorm_bwd_jobs(F32, *jobs(bwd_job()), cs, 13, None), EINVAL, "item list")


def test_colsum_refusals_and_empty_shapes(lib):
    refused(lib, lib.mebt_op_colsum(3, DUMMY, 4, 4, 4, DUMMY, None), EDTYPE, "dtype")
    refused(lib, lib.mebt_op_colsum(F32, DUMMY, 4, 6, 8, DUMMY, None), ESHAPE, "multiples of 4")
    refused(lib, lib.mebt_op_colsum(BF16, DUMMY, 4, 8, 4, DUMMY, None), ESHAPE, "ldx >= N")
    refused(lib, lib.mebt_op_colsum(BF16, DUMMY, 4, 8, 10, DUMMY, None), ESHAPE, "multiples of 4")
    refused(lib, lib.mebt_op_colsum(F32, None, 4, 8, 8, DUMMY, None), EINVAL, "null")
    refused(lib, lib.mebt_op_colsum(F32, DUMMY, 4, 8, 8, None, None), EINVAL, "null")
    assert lib.mebt_op_colsum(F32, None, 0, 8, 8, None, None) == OK and lib.mebt_op_colsum(BF16, None, 5, 0, 0, None, None) == OK
    items = (ColsumItem * 3)(ColsumItem(X=DUMMY, out=DUMMY, M=0, N=6, ldx=0), ColsumItem(M=5, N=0), ColsumItem(X=DUMMY, out=DUMMY, M=2, N=6, ldx=8))
    assert lib.mebt_op_colsum_grouped(F32, items, 2, None) == OK          # the two empty items (an empty item is not looked at)
    assert lib.mebt_op_colsum_grouped(F32, None, 0, None) == OK
    refused(lib, lib.mebt_op_colsum_grouped(F32, items, 3, None), ESHAPE, "multiples of 4")
    refused(lib, lib.mebt_op_colsum_grouped(F32, None, 2, None), EINVAL, "item list")
    refused(lib, lib.mebt_op_colsum_grouped(F32, items, 13, None), EINVAL, "item list")
    refused(lib, lib.mebt_op_colsum_grouped(9, items, 2, None), EDTYPE, "dtype")


def test_cross_entropy_refusals_and_empty_shapes(lib):
    D = DUMMY
    ce = lambda B=2, N=7, NT=4, V=20, ptrs=(D,) * 7: lib.mebt_op_cross_entropy(ptrs[0], ptrs[1], ptrs[2], B, N, NT, V, 0.1, ptrs[3], ptrs[4], ptrs[5],
                                                                              ptrs[6], None, 0, 1.0, None)
    refused(lib, ce(V=18), ESHAPE, "multiple of 4")
    refused(lib, ce(V=0), ESHAPE, "multiple of 4")
    refused(lib, ce(NT=8), ESHAPE, "NT <= N")
    for i in range(7):
        refused(lib, ce(ptrs=tuple(None if k == i else D for k in range(7))), EINVAL, "null")
    assert ce(B=0, ptrs=(None,) * 7) == OK and ce(NT=0, ptrs=(None,) * 7) == OK
    bw = lambda dt=F32, B=2, N=7, NT=4, V=20, ptrs=(D,) * 5: lib.mebt_op_cross_entropy_bwd(dt, ptrs[0], ptrs[1], ptrs[2], ptrs[3], None, 1.0, 0.0, ptrs[4],
                                                                                          B, N, NT, V, None)
    refused(lib, bw(dt=2), EDTYPE, "dtype")
    refused(lib, bw(V=1030), ESHAPE, "multiple of 4")
    for i in range(5):
        refused(lib, bw(ptrs=tuple(None if k == i else D for k in range(5))), EINVAL, "null")
    assert bw(B=0, ptrs=(None,) * 5) == OK and bw(dt=BF16, NT=0, ptrs=(None,) * 5) == OK


def test_adamw_refusals_and_empty_shapes(lib):
    D = DUMMY
    ad = lambda p=D, g=D, m=D, v=D, n=8, step=1, g_bf16=0, pieces=1, stride=0: lib.mebt_op_adamw(p, g, m, v, None, n, 1e-3, 0.9, 0.95, 1e-8, 0.01, step, 1.0,
                                                                                               g_bf16, pieces, stride, None)
    refused(lib, ad(n=6), ESHAPE, "multiple of 4")
    refused(lib, ad(n=-4), EINVAL, "n >= 0")
    refused(lib, ad(step=0), EINVAL, "step >= 1")
    refused(lib, ad(pieces=0), EINVAL, "g_pieces")
    refused(lib, ad(pieces=3, g_bf16=0, stride=16), ESHAPE, "pieces")
    refused(lib, ad(pieces=3, g_bf16=1, stride=4), ESHAPE, "pieces")
    refused(lib, ad(pieces=3, g_bf16=1, stride=10), ESHAPE, "pieces")
    for k in ("p", "g", "m", "v"):
        refused(lib, ad(**{k: None}), EINVAL, "null")
    assert ad(n=0, p=None, g=None, m=None, v=None) == OK


def test_embed_bwd_and_row_mover_refusals_and_empty_shapes(lib):
    D = DUMMY
    eb = lambda dt=F32, B=2, N=12, NC=5, NT=4, NS=2, d=64, ptrs=(D,) * 10: lib.mebt_op_embed_bwd(dt, *ptrs, B, N, NC, NT, NS, d, None)
    refused(lib, eb(dt=4), EDTYPE, "dtype")
    refused(lib, eb(d=6), ESHAPE, "multiple of 4")
    refused(lib, eb(NC=9), ESHAPE, "extents")
    for i in range(10):
        refused(lib, eb(ptrs=tuple(None if k == i else D for k in range(10))), EINVAL, "null")
    assert eb(B=0, ptrs=(None,) * 10) == OK and eb(NC=0, NT=0, NS=0, ptrs=(None,) * 10) == OK

    cp = lambda src=D, dst=D, rows=3, d=8, s_seg=0: lib.mebt_op_copy_rows(src, dst, rows, d, 1, 0, s_seg, 0, 0, 0, 0, 0, None)
    refused(lib, cp(d=6), ESHAPE, "multiple of 4")
    refused(lib, cp(s_seg=-1), ESHAPE, "row map")
    refused(lib, cp(src=None), EINVAL, "null")
    refused(lib, cp(dst=None), EINVAL, "null")
    assert cp(rows=0, src=None, dst=None) == OK and cp(d=0, src=None, dst=None) == OK

    ix = lambda src=D, dst=D, idx=D, B=2, n=5, row_bytes=16: lib.mebt_op_index_rows(src, dst, idx, B, n, 9, row_bytes, 0, None)
    for rb in (8, 24, 1032, 0):
        refused(lib, ix(row_bytes=rb), ESHAPE, "16 bytes")
    for k in ("src", "dst", "idx"):
        refused(lib, ix(**{k: None}), EINVAL, "null")
    assert ix(B=0, src=None, dst=None, idx=None) == OK and ix(n=0, src=None, dst=None, idx=None) == OK


@pytest.mark.parametrize("V", [20, 1028, 4096, 16384])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_loss_emulation_stays_within_half_of_the_gates(V, eps):
    """the fp32 emulation of the loss kernels (their summation order, the worst-case __expf argument error injected) against the
    float64 reference, on the cases and gates of tests/test_gpu_row_ops.py: at most half of each gate before any GPU run"""
    from tests.test_gpu_row_ops import assert_ce_emulation_within_half_of_the_gates
    assert_ce_emulation_within_half_of_the_gates(V, eps)


def test_adamw_float64_reference_matches_torch():
    from tests.test_gpu_row_ops import check_adamw_reference_against_torch
    check_adamw_reference_against_torch()
