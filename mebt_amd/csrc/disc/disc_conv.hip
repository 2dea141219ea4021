// First-stage discriminators (reference mebt/vqgan.py:416-520), the forward: ingest, the 4^d strided convolution with its BatchNorm
// partials, the normalise + LeakyReLU pass and the one-channel last stage.  DESIGN.md §9i.  The reductions are in disc.hip.
//
// Maps are channels-last [B, T, H, W, C] (T = 1 for the image network) of fp16 or fp32.  Every global offset comes from disc_addr.h,
// which tests/disc_conv_walk.cpp walks on the CPU; the kernels here only add such an offset to a base pointer.  The tile and its step
// are mfma_tile.h's, the fixed-order sums block_reduce.h's.  No float atomics: an output row's K order is fixed (slices of 32 in index
// order) and does not depend on M, the batch or the tile the row sits in; the BatchNorm partials of a tile are added lanes by
// butterfly, then row blocks and waves in index order through LDS, one fp64 slot per (channel, moment, row tile).
//
// fp32: the tile accumulator is added into a second fp32 accumulator every DISC_FLUSH_K = 1024 of K (32 slices) and cleared, so a
// long K (16384, 32768 at ndf 64) is a short sum of short sums; the interval is fixed, so the order is the same on every run.  The
// one-channel kernel does the same per lane, every 1024 of K of the wave.
#include "../block_reduce.h"
#include "../host_util.h"
#include "../mfma_tile.h"
#include "disc_addr.h"

namespace {

constexpr float DISC_SLOPE = 0.2f;
static_assert(DISC_BK == TILE_BK && DISC_BN == TILE_BN && DISC_THREADS == TILE_THREADS, "disc_addr.h states mfma_tile.h's tile");

// fp32 [B, 3, T, H, W] -> channels-last [B, To, H, W, 4] of T_ with a zero fourth channel; frame_idx (int64 [B], or null) picks one
// frame of every clip (To = 1): the gather of vqgan.py:104-108
template <typename T_>
__global__ __launch_bounds__(256) void disc_ingest_kernel(const float* x, const int64_t* frame_idx, T_* out, int B, int T, int H, int W, int To) {
    const int64_t total = (int64_t)B * To * H * W;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
        int64_t r = v;
        const int w = (int)(r % W); r /= W;
        const int h = (int)(r % H); r /= H;
        const int t = (int)(r % To);
        const int64_t b = r / To;
        int f = t;
        if (frame_idx) {
            const int64_t fi = frame_idx[b];
            f = fi < 0 ? 0 : (fi >= T ? T - 1 : (int)fi);            // the host has refused an index outside [0, T)
        }
        f32x4 px;
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = x[disc_ingest_src(T, H, W, b, c, f, h, w)];
        px[3] = 0.f;
        store4<T_>(out + disc_ingest_dst(To, H, W, b, t, h, w), px);
    }
}

// SUB = VEC / GV gathers per 16-byte chunk of K (2 only for Cin 4 in fp16)
template <typename T, int SUB>
__global__ __launch_bounds__(256) void disc_conv_kernel(const T* in, const T* w, const float* bias, T* out, double* slots, const DiscGeom g, int act) {
    using Cfg = TileCfg<T>;
    constexpr int VEC = Cfg::VEC, BM = Cfg::BM, LD = Cfg::LD, WM = Cfg::WM;
    constexpr int ACH = BM * DISC_BK / VEC / 256, BCH = DISC_BN * DISC_BK / VEC / 256;
    __shared__ __attribute__((aligned(16))) T sA[2][BM * LD];
    __shared__ __attribute__((aligned(16))) T sB[2][DISC_BN * LD];
    __shared__ double sred[2][4 * WM][DISC_BN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int n0 = blockIdx.y * DISC_BN;

    DiscOrg org[ACH];
    DiscChunk ac[ACH], bc[BCH];
#pragma unroll
    for (int i = 0; i < ACH; ++i) { ac[i] = disc_stage_chunk(tid, i, VEC); org[i] = disc_row_origin(g, m0 + ac[i].row); }
#pragma unroll
    for (int i = 0; i < BCH; ++i) bc[i] = disc_stage_chunk(tid, i, VEC);

    u32x4 ra[ACH], rb[BCH];
    auto gload = [&](int kk) {
        const int kb = kk * DISC_BK;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const int k = kb + ac[i].ch * VEC;
            int64_t off;
            if constexpr (SUB == 1) {
                if (disc_in_offset(g, org[i], k, off)) ra[i] = *reinterpret_cast<const u32x4*>(in + off);
                else ra[i] = u32x4{0u, 0u, 0u, 0u};
            } else {
                u32x2 lo = {0u, 0u}, hi = {0u, 0u};
                if (disc_in_offset(g, org[i], k, off)) lo = *reinterpret_cast<const u32x2*>(in + off);
                if (disc_in_offset(g, org[i], k + VEC / 2, off)) hi = *reinterpret_cast<const u32x2*>(in + off);
                ra[i] = u32x4{lo[0], lo[1], hi[0], hi[1]};
            }
        }
#pragma unroll
        for (int i = 0; i < BCH; ++i) rb[i] = *reinterpret_cast<const u32x4*>(w + disc_w_offset(g, n0 + bc[i].row, kb + bc[i].ch * VEC));
    };
    auto lstore = [&](int s) {
#pragma unroll
        for (int i = 0; i < ACH; ++i) *reinterpret_cast<u32x4*>(&sA[s][ac[i].row * LD + ac[i].ch * VEC]) = ra[i];
#pragma unroll
        for (int i = 0; i < BCH; ++i) *reinterpret_cast<u32x4*>(&sB[s][bc[i].row * LD + bc[i].ch * VEC]) = rb[i];
    };

    f32x4 acc[WM][4];
    tile_zero(acc);
    f32x4 tot[sizeof(T) == 4 ? WM : 1][4];
    if constexpr (sizeof(T) == 4) tile_zero(tot);
    auto flush = [&]() {
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) { tot[i][j] += acc[i][j]; acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        }
    };

    const int nk = g.Kpad / DISC_BK;
    const int fr = lane & 15, fq = lane >> 4;
    int ar[WM], br[4];
#pragma unroll
    for (int i = 0; i < WM; ++i) ar[i] = (16 * WM * wave + 16 * i + fr) * LD;
#pragma unroll
    for (int j = 0; j < 4; ++j) br[j] = (16 * j + fr) * LD;
    gload(0);
    lstore(0);
    __syncthreads();
    for (int kk = 0; kk < nk; ++kk) {
        const int s = kk & 1;
        if (kk + 1 < nk) gload(kk + 1);
        tile_mma<T, WM>(acc, sA[s], ar, sB[s], br, fq);
        if ((kk + 1) % (DISC_FLUSH_K / DISC_BK) == 0) flush();
        if (kk + 1 < nk) lstore(s ^ 1);
        __syncthreads();
    }
    flush();

    // bias, and the value the statistics are taken from: fp32, before the store rounds it
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + disc_frag_col(j, lane, r);
                const float v = sizeof(T) == 4 ? tot[sizeof(T) == 4 ? i : 0][j][r] : acc[i][j][r];
                acc[i][j][r] = v + (n < g.Cout ? bias[n] : 0.f);
            }

    if (slots) {
        const int64_t M = disc_rows(g);
#pragma unroll
        for (int i = 0; i < WM; ++i) {
            const bool live = m0 + disc_frag_row(wave, i, lane, WM) < M;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double d1 = live ? (double)acc[i][j][r] : 0.0;
                    double d2 = d1 * d1;
#pragma unroll
                    for (int o = 8; o > 0; o >>= 1) { d1 += __shfl_xor(d1, o, 64); d2 += __shfl_xor(d2, o, 64); }
                    if (fr == 0) {
                        sred[0][wave * WM + i][disc_frag_col(j, lane, r)] = d1;
                        sred[1][wave * WM + i][disc_frag_col(j, lane, r)] = d2;
                    }
                }
        }
        __syncthreads();
        if (tid < 2 * DISC_BN) {
            const int q = tid >> 6, col = tid & 63;
            double s = 0.0;
#pragma unroll
            for (int rbk = 0; rbk < 4 * WM; ++rbk) s += sred[q][rbk][col];
            int64_t off;
            if (disc_slot_offset(g, n0 + col, q, blockIdx.x, off)) slots[off] = s;
        }
    }

#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const int64_t m = m0 + disc_frag_row(wave, i, lane, WM);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int64_t off;
                if (!disc_out_offset(g, m, n0 + disc_frag_col(j, lane, r), off)) continue;
                float v = acc[i][j][r];
                if (act) v = v > 0.f ? v : DISC_SLOPE * v;
                out[off] = (T)v;
            }
    }
}

// in place on a map [M, C]: (x - mean) rstd gamma + beta, then LeakyReLU(0.2); stats fp32 [2][C] = mean, rstd.  The arithmetic is
// fp64 (the pass is bound by memory), one rounding to T at the store.  C is a multiple of 4.
template <typename T>
__global__ __launch_bounds__(256) void disc_bn_act_kernel(T* x, int64_t n4, int C, const float* stats, const float* gamma, const float* beta) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int c0 = (int)((i * 4) % C);
        f32x4 v = load4<T>(x + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = c0 + e;
            const double y = ((double)v[e] - (double)stats[c]) * (double)stats[C + c] * (double)gamma[c] + (double)beta[c];
            v[e] = (float)(y > 0.0 ? y : 0.2 * y);
        }
        store4<T>(x + i * 4, v);
    }
}

// the last stage, Cout = 1: one wave per output voxel, lanes stride over K in 16-byte chunks, taps in the padding are skipped
template <typename T>
__global__ __launch_bounds__(256) void disc_head_kernel(const T* in, const T* w, const float* bias, T* out, const DiscGeom g) {
    constexpr int VEC = TileCfg<T>::VEC;
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= disc_rows(g)) return;                       // wave uniform; no barrier follows
    const DiscOrg org = disc_row_origin(g, m);
    const int iters = disc_head_iters(g), every = disc_head_flush_iters(g), K = disc_K(g);
    float acc = 0.f, tot = 0.f;
    for (int it = 0; it < iters; ++it) {
        const int k = disc_head_k(g, it, lane);
        int64_t off;
        if (k < K && disc_in_offset(g, org, k, off)) {
            T xv[VEC], wv[VEC];
            *reinterpret_cast<u32x4*>(xv) = *reinterpret_cast<const u32x4*>(in + off);
            *reinterpret_cast<u32x4*>(wv) = *reinterpret_cast<const u32x4*>(w + disc_w_offset(g, 0, k));
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc = fmaf((float)xv[e], (float)wv[e], acc);
        }
        if ((it + 1) % every == 0) { tot += acc; acc = 0.f; }
    }
    tot += acc;
    tot = wave_sum(tot);
    int64_t off;
    if (lane == 0 && disc_out_offset(g, m, 0, off)) out[off] = (T)(tot + bias[0]);
}

// the checks the convolution and the one-channel stage share, in this order: shape, extents, channel width, alignment, buffer sizes
int check_stage(const char* who, int32_t dtype, const void* in, int64_t in_bytes, const void* w, int64_t w_bytes, const float* bias, const void* out,
                int64_t out_bytes, int32_t B, int32_t Ti, int32_t Hi, int32_t Wi, int32_t Cin, int32_t kt, int32_t stride, int32_t To, int32_t Ho,
                int32_t Wo, int32_t Cout, DiscGeom* geom) {
    if (!in || !w || !bias || !out) return fail(MEBT_EINVAL, who, "null pointer");
    if (int rc = check_dtype(who, dtype)) return rc;
    if (B < 1 || Ti < 1 || Hi < 1 || Wi < 1 || Cin < 1 || Cout < 1) return fail(MEBT_ESHAPE, who, "bad shape");
    if ((kt != 1 && kt != 4) || (stride != 1 && stride != 2) || (kt == 1 && Ti != 1)) return fail(MEBT_ESHAPE, who, "kt must be 1 (T = 1) or 4, stride 1 or 2");
    if (To != (kt == 4 ? disc_out_extent(Ti, stride) : 1) || Ho != disc_out_extent(Hi, stride) || Wo != disc_out_extent(Wi, stride))
        return fail(MEBT_ESHAPE, who, "output size does not follow from the input: n // 2 + 1 at stride 2, n + 1 at stride 1");
    const int eb = dtype == MEBT_DTYPE_F16 ? 2 : 4, vec = 16 / eb;
    if (Cin % 4 || (Cin % vec && Cin != 4)) return fail(MEBT_ESHAPE, who, "Cin as stored must be 4 or a multiple of the 16-byte vector");
    if ((int64_t)kt * 16 * Cin > 0x3FFFFFFFll || (int64_t)Cout > 0x3FFFFFFFll) return fail(MEBT_ESHAPE, who, "K or Cout too large");
    const DiscGeom g = disc_geom(B, Ti, Hi, Wi, Cin, kt, stride, Cout, eb);
    if ((int64_t)B * Ti * Hi * Wi > 0x7FFFFFFFll * 64) return fail(MEBT_ESHAPE, who, "input too large");
    if (disc_row_tiles(g) > 0x7FFFFFFFll) return fail(MEBT_ESHAPE, who, "too many output voxels for one launch");
    if (!aligned16(in) || !aligned16(w) || !aligned16(out)) return fail(MEBT_EINVAL, who, "in, w and out must be 16-byte aligned");
    if (in_bytes < disc_in_elems(g) * eb) return fail(MEBT_EWORKSPACE, who, "input buffer too small");
    if (w_bytes != disc_w_elems(g) * eb) return fail(MEBT_EWORKSPACE, who, "weight buffer is not Npad x Kpad");
    if (out_bytes < disc_out_elems(g) * eb) return fail(MEBT_EWORKSPACE, who, "output buffer too small");
    *geom = g;
    return MEBT_OK;
}

}  // namespace

extern "C" int mebt_op_disc_ingest(int32_t dtype, const float* x, const int64_t* frame_idx, void* out, int64_t out_bytes, int32_t B, int32_t T,
                                   int32_t H, int32_t W, mebt_stream_t stream) {
    const char* who = "disc_ingest";
    if (!x || !out) return fail(MEBT_EINVAL, who, "null pointer");
    if (int rc = check_dtype(who, dtype)) return rc;
    if (B < 1 || T < 1 || H < 1 || W < 1) return fail(MEBT_ESHAPE, who, "bad shape");
    if (!aligned16(out) || (reinterpret_cast<uintptr_t>(x) & 3) || (reinterpret_cast<uintptr_t>(frame_idx) & 7))
        return fail(MEBT_EINVAL, who, "out must be 16-byte aligned, x 4-byte, frame_idx 8-byte");
    const int To = frame_idx ? 1 : T;
    const int64_t voxels = (int64_t)B * To * H * W;
    if (out_bytes < voxels * 4 * (dtype == MEBT_DTYPE_F16 ? 2 : 4)) return fail(MEBT_EWORKSPACE, who, "output buffer too small");
    with_dtype(dtype, [&](auto tag) {
        using T_ = decltype(tag);
        hipLaunchKernelGGL(disc_ingest_kernel<T_>, dim3(grid_of(voxels)), dim3(256), 0, S(stream), x, frame_idx, reinterpret_cast<T_*>(out), B, T, H, W, To);
    });
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int mebt_op_disc_conv(int32_t dtype, const void* in, int64_t in_bytes, const void* w, int64_t w_bytes, const float* bias, void* out,
                                 int64_t out_bytes, void* slots, int64_t slots_bytes, int32_t B, int32_t Ti, int32_t Hi, int32_t Wi, int32_t Cin,
                                 int32_t kt, int32_t stride, int32_t To, int32_t Ho, int32_t Wo, int32_t Cout, int32_t act, mebt_stream_t stream) {
    const char* who = "disc_conv";
    DiscGeom g;
    if (int rc = check_stage(who, dtype, in, in_bytes, w, w_bytes, bias, out, out_bytes, B, Ti, Hi, Wi, Cin, kt, stride, To, Ho, Wo, Cout, &g)) return rc;
    if (slots_bytes != 0 && !slots) return fail(MEBT_EINVAL, who, "null pointer");
    if (slots)
        if (int rc = check_scratch(who, slots, slots_bytes, 8 * disc_slot_count(g), disc_row_tiles(g))) return rc;
    const dim3 grid((unsigned)disc_row_tiles(g), (unsigned)(g.Npad / DISC_BN));
    with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, S(stream), reinterpret_cast<const T*>(in), reinterpret_cast<const T*>(w), bias,
                               reinterpret_cast<T*>(out), reinterpret_cast<double*>(slots), g, (int)(act != 0));
        };
        if (g.GV == g.VEC) launch(disc_conv_kernel<T, 1>);
        else launch(disc_conv_kernel<T, 2>);
    });
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int mebt_op_disc_bn_act(int32_t dtype, void* x, int64_t M, int32_t C, const float* stats, const float* gamma, const float* beta,
                                   mebt_stream_t stream) {
    const char* who = "disc_bn_act";
    if (!x || !stats || !gamma || !beta) return fail(MEBT_EINVAL, who, "null pointer");
    if (int rc = check_dtype(who, dtype)) return rc;
    if (M < 1 || C < 1 || C % 4) return fail(MEBT_ESHAPE, who, "bad shape: C must be a positive multiple of 4");
    if (!aligned16(x)) return fail(MEBT_EINVAL, who, "x must be 16-byte aligned");
    const int64_t n4 = M * C / 4;
    with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(disc_bn_act_kernel<T>, dim3(grid_of(n4)), dim3(256), 0, S(stream), reinterpret_cast<T*>(x), n4, C, stats, gamma, beta);
    });
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int mebt_op_disc_head(int32_t dtype, const void* in, int64_t in_bytes, const void* w, int64_t w_bytes, const float* bias, void* out,
                                 int64_t out_bytes, int32_t B, int32_t Ti, int32_t Hi, int32_t Wi, int32_t Cin, int32_t kt, int32_t To, int32_t Ho,
                                 int32_t Wo, mebt_stream_t stream) {
    const char* who = "disc_head";
    DiscGeom g;
    if (int rc = check_stage(who, dtype, in, in_bytes, w, w_bytes, bias, out, out_bytes, B, Ti, Hi, Wi, Cin, kt, 1, To, Ho, Wo, 1, &g)) return rc;
    if (g.GV != g.VEC) return fail(MEBT_ESHAPE, who, "Cin must be a multiple of the 16-byte vector");
    const int64_t blocks = (disc_rows(g) + 3) / 4;
    if (blocks > 0x7FFFFFFFll) return fail(MEBT_ESHAPE, who, "too many output voxels for one launch");
    with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(disc_head_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, S(stream), reinterpret_cast<const T*>(in),
                           reinterpret_cast<const T*>(w), bias, reinterpret_cast<T*>(out), g);
    });
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}
