// Every global offset of the discriminators' forward kernels (csrc/disc/disc_conv.hip), and every decision that an access is skipped.
// Plain C++17 with no HIP in it: tests/disc_conv_walk.cpp walks these functions on the CPU for every workgroup, thread and K slice of
// the tested shapes and checks bounds, alignment, single writes and the convolution itself.  The kernels add what a function returns
// to a base pointer and form no address of their own.
//
// A stage is the 4^d convolution (d = 2: kt 1, d = 3: kt 4), stride 1 or 2, zero padding 2 per side, as an implicit GEMM:
// M = B To Ho Wo output voxels, N = Cout, K = (tap, ci) with ci fastest and tap = (dt 4 + dh) 4 + dw.  Maps are channels-last
// [B, T, H, W, C]; weights are [Npad][Kpad].  Offsets are in elements and 64-bit.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define DISC_FN __host__ __device__ __forceinline__
#else
#define DISC_FN inline
#endif

constexpr int DISC_BK = 32, DISC_BN = 64, DISC_THREADS = 256, DISC_PAD = 2;
constexpr int DISC_FLUSH_K = 1024;          // fp32: the accumulator is added into a second one every DISC_FLUSH_K of K

// one stage.  Cin is the channel count as stored (3 input channels are stored as 4, the fourth 0); VEC elements make a 16-byte chunk
// of K (8 fp16, 4 fp32); GV <= VEC is the width of one gather: VEC where Cin is a multiple of it, else 4 (Cin 4 in fp16: a chunk is
// two taps of 8 bytes each)
struct DiscGeom {
    int B, Ti, Hi, Wi, Cin;
    int kt, stride;
    int To, Ho, Wo, Cout;
    int Kpad, Npad;
    int BM, VEC, GV;
    int cin_shift;                          // log2 Cin where Cin is a power of two (every ndf that is one), else -1: k / Cin is a shift
};

DISC_FN int disc_out_extent(int n, int stride) { return stride == 2 ? n / 2 + 1 : n + 1; }
DISC_FN int disc_round_up(int v, int to) { return (v + to - 1) / to * to; }

// the geometry of a stage from its input; elem_bytes 2 (fp16: 128-row tiles) or 4 (fp32: 64-row tiles)
DISC_FN DiscGeom disc_geom(int B, int Ti, int Hi, int Wi, int Cin, int kt, int stride, int Cout, int elem_bytes) {
    DiscGeom g;
    g.B = B; g.Ti = Ti; g.Hi = Hi; g.Wi = Wi; g.Cin = Cin; g.kt = kt; g.stride = stride; g.Cout = Cout;
    g.To = kt == 4 ? disc_out_extent(Ti, stride) : 1;
    g.Ho = disc_out_extent(Hi, stride);
    g.Wo = disc_out_extent(Wi, stride);
    g.Kpad = disc_round_up(kt * 16 * Cin, DISC_BK);
    g.Npad = disc_round_up(Cout, DISC_BN);
    g.BM = elem_bytes == 2 ? 128 : 64;
    g.VEC = 16 / elem_bytes;
    g.GV = Cin % g.VEC == 0 ? g.VEC : 4;
    g.cin_shift = -1;
    for (int sft = 0; sft < 31; ++sft)
        if (Cin == 1 << sft) g.cin_shift = sft;
    return g;
}

DISC_FN int64_t disc_rows(const DiscGeom& g) { return (int64_t)g.B * g.To * g.Ho * g.Wo; }
DISC_FN int disc_K(const DiscGeom& g) { return g.kt * 16 * g.Cin; }
DISC_FN int64_t disc_row_tiles(const DiscGeom& g) { return (disc_rows(g) + g.BM - 1) / g.BM; }
DISC_FN int64_t disc_in_elems(const DiscGeom& g) { return (int64_t)g.B * g.Ti * g.Hi * g.Wi * g.Cin; }
DISC_FN int64_t disc_w_elems(const DiscGeom& g) { return (int64_t)g.Npad * g.Kpad; }
DISC_FN int64_t disc_out_elems(const DiscGeom& g) { return disc_rows(g) * g.Cout; }
DISC_FN int64_t disc_slot_count(const DiscGeom& g) { return (int64_t)g.Cout * 2 * disc_row_tiles(g); }

// staging: chunk i of thread tid is 16-byte chunk `ch` of tile row `row` (A: rows of the BM x 32 slice, i < BM * 32 / VEC / 256;
// B: rows of the 64 x 32 slice, i < 64 * 32 / VEC / 256)
struct DiscChunk { int row, ch; };
DISC_FN DiscChunk disc_stage_chunk(int tid, int i, int VEC) {
    const int id = tid + DISC_THREADS * i, cpr = DISC_BK / VEC;
    return {id / cpr, id % cpr};
}

// the fragment map of mfma_tile.h's result: value r of acc[i][j] of `lane` of `wave` is tile row disc_frag_row, tile column disc_frag_col
DISC_FN int disc_frag_row(int wave, int i, int lane, int WM) { return 16 * WM * wave + 16 * i + (lane & 15); }
DISC_FN int disc_frag_col(int j, int lane, int r) { return 16 * j + 4 * (lane >> 4) + r; }

// an output row's gather origin: the voxel index of its clip's first input voxel, and the input coordinate of tap (0, 0, 0), which
// may be negative (front padding).  A row at or past M is clamped to the last row and marked: it reads nothing and writes nothing.
struct DiscOrg { int64_t clip; int t, h, w; int ok; };
DISC_FN DiscOrg disc_row_origin(const DiscGeom& g, int64_t m) {
    DiscOrg o;
    const int64_t M = disc_rows(g);
    o.ok = m < M;
    if (m >= M) m = M - 1;
    const int wo = (int)(m % g.Wo); m /= g.Wo;
    const int ho = (int)(m % g.Ho); m /= g.Ho;
    const int to = (int)(m % g.To); m /= g.To;
    o.clip = m * g.Ti * g.Hi * g.Wi;
    o.t = g.kt == 4 ? to * g.stride - DISC_PAD : 0;
    o.h = ho * g.stride - DISC_PAD;
    o.w = wo * g.stride - DISC_PAD;
    return o;
}

// k (a multiple of GV) -> tap and channel; taps are 16 (kt 1) or 64 (kt 4): shifts and masks on k / Cin
struct DiscTap { int dt, dh, dw, ci; };
DISC_FN DiscTap disc_tap(const DiscGeom& g, int k) {
    const int tap = g.cin_shift >= 0 ? k >> g.cin_shift : k / g.Cin;
    return {tap >> 4, (tap >> 2) & 3, tap & 3, k - tap * g.Cin};
}

// the input offset of the GV elements of row `o` from k on; false: they read zero (k at or past K, a row past M, a tap in the padding)
DISC_FN bool disc_in_offset(const DiscGeom& g, const DiscOrg& o, int k, int64_t& off) {
    if (!o.ok || k >= disc_K(g)) return false;
    const DiscTap t = disc_tap(g, k);
    const int ti = o.t + t.dt, hi = o.h + t.dh, wi = o.w + t.dw;
    if ((unsigned)ti >= (unsigned)g.Ti || (unsigned)hi >= (unsigned)g.Hi || (unsigned)wi >= (unsigned)g.Wi) return false;
    off = (o.clip + ((int64_t)ti * g.Hi + hi) * g.Wi + wi) * g.Cin + t.ci;
    return true;
}

// the weight offset of the VEC elements of output channel n (< Npad) from k (< Kpad) on
DISC_FN int64_t disc_w_offset(const DiscGeom& g, int n, int k) { return (int64_t)n * g.Kpad + k; }

// the output offset of (m, n); false: not stored (a row at or past M, a column at or past Cout)
DISC_FN bool disc_out_offset(const DiscGeom& g, int64_t m, int n, int64_t& off) {
    if (m >= disc_rows(g) || n >= g.Cout) return false;
    off = m * g.Cout + n;
    return true;
}

// the BatchNorm slot of (channel, moment q, row tile), the layout mebt_op_disc_bn_finish reads; false: no such channel
DISC_FN bool disc_slot_offset(const DiscGeom& g, int c, int q, int64_t tile, int64_t& off) {
    if (c >= g.Cout) return false;
    off = ((int64_t)c * 2 + q) * disc_row_tiles(g) + tile;
    return true;
}

// the one-channel stage: wave `m` (one output voxel) reads chunk `it` of `lane` at k = (it 64 + lane) VEC, for it < disc_head_iters;
// its input offset is disc_in_offset's (GV = VEC there), its weight offset k itself (row 0 of the arranged weight)
DISC_FN int disc_head_iters(const DiscGeom& g) { return (disc_K(g) / g.VEC + 63) / 64; }
DISC_FN int disc_head_k(const DiscGeom& g, int it, int lane) { return (it * 64 + lane) * g.VEC; }
// iterations between two flushes of a lane's accumulator: DISC_FLUSH_K of K
DISC_FN int disc_head_flush_iters(const DiscGeom& g) { return DISC_FLUSH_K / (64 * g.VEC); }

// ingest: the source offset in fp32 [B, 3, T, H, W] of channel c of destination voxel (b, t, h, w), where a frame index picks frame f
// of the clip for t = 0; the destination offset of that voxel's 4 stored channels in [B, To, H, W, 4]
DISC_FN int64_t disc_ingest_src(int T, int H, int W, int64_t b, int c, int f, int h, int w) {
    return (((b * 3 + c) * T + f) * H + h) * W + w;
}
DISC_FN int64_t disc_ingest_dst(int To, int H, int W, int64_t b, int t, int h, int w) { return ((((b * To + t) * H + h) * W + w)) * 4; }
