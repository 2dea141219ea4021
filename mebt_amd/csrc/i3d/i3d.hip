// Inception-I3D forward for FVD / KVD on gfx950 (reference mebt/fvd/pytorch_i3d.py, mebt/fvd/fvd.py:preprocess).
//
// Layout: activations are channels-last [B, T, H, W, C] (fp16 in the fast mode, fp32 in the parity mode).  Every convolution
// (Unit3D: conv + folded eval-mode BatchNorm + ReLU) is an implicit GEMM: M = output voxels, N = Cout, K = taps x Cin as one
// flat (tap, ci) index, ci fastest, padded to a multiple of 32.  Weights are pre-arranged on the host as [Npad][Kpad] (Npad a
// multiple of 64, zero rows / columns in the padding).  Padding is TF "same" ZERO padding with an asymmetric front / back
// (pytorch_i3d.py Unit3D.compute_pad): a tap that falls outside the input reads 0.  The epilogue writes each column range to its
// own destination with an explicit channel stride and offset, so an Inception branch lands directly in its slice of the
// concatenated output and the three 1x1 convolutions that read a module's input run as one GEMM.
//
// K-slice addressing: a block builds, once, a table in LDS of (dt, dh, dw, ci) for every 16-byte chunk of K (Cin a multiple of
// the chunk width) or for every element (Conv3d_1a, Cin = 3, K = 1029: no padding of Cin to 4); the k-loop then gathers without
// integer division.  The row of an output voxel is fixed for the whole k-loop and its accumulation order never depends on M or
// on the tile it sits in, so a clip's result does not depend on the batch it is part of.
#include "../host_util.h"
#include "../kernels.h"
#include "../mfma_tile.h"
#include <math.h>

namespace {

constexpr int I3D_BK = TILE_BK, I3D_BN = TILE_BN;
constexpr int I3D_MAX_TAB = 2048;      // LDS entries of the K table (8 KiB)

__device__ __forceinline__ uint32_t tab_entry(const mebt_i3d_conv_desc& p, int k, int K) {
    if (k >= K) return 0u;
    const int tap = k / p.Cin, ci = k - tap * p.Cin;
    const int khw = p.k[1] * p.k[2];
    const int dt = tap / khw, r = tap - dt * khw, dh = r / p.k[2], dw = r - dh * p.k[2];
    return 0x80000000u | ((uint32_t)dw << 24) | ((uint32_t)dh << 20) | ((uint32_t)dt << 16) | (uint32_t)ci;
}

// one output row's gather origin: batch, and the input coordinate of tap (0, 0, 0) (may be negative: front padding)
struct RowOrg { int b, t, h, w; bool ok; };

template <typename T>
__device__ __forceinline__ bool tap_offset(const mebt_i3d_conv_desc& p, const RowOrg& o, uint32_t e, size_t& off) {
    if (!o.ok || !(e & 0x80000000u)) return false;
    const int ti = o.t + (int)((e >> 16) & 15), hi = o.h + (int)((e >> 20) & 15), wi = o.w + (int)((e >> 24) & 15);
    if ((unsigned)ti >= (unsigned)p.Ti || (unsigned)hi >= (unsigned)p.Hi || (unsigned)wi >= (unsigned)p.Wi) return false;
    off = ((((size_t)o.b * p.Ti + ti) * p.Hi + hi) * p.Wi + wi) * p.Cin + (e & 0xFFFFu);
    return true;
}

template <typename T>
__global__ __launch_bounds__(256) void i3d_conv_kernel(const mebt_i3d_conv_desc p, int vec_mode, int Kpad) {
    using Cfg = TileCfg<T>;
    constexpr int VEC = Cfg::VEC, BM = Cfg::BM, LD = Cfg::LD, WM = Cfg::WM;
    constexpr int ACH = BM * I3D_BK / VEC / 256;       // A chunks per thread (2)
    constexpr int BCH = I3D_BN * I3D_BK / VEC / 256;   // B chunks per thread (1 fp16, 2 fp32)
    constexpr int CPR = I3D_BK / VEC;                  // chunks per row
    __shared__ __attribute__((aligned(16))) T sA[2][BM * LD];
    __shared__ __attribute__((aligned(16))) T sB[2][I3D_BN * LD];
    __shared__ uint32_t tab[I3D_MAX_TAB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = p.k[0] * p.k[1] * p.k[2] * p.Cin;
    const long M = (long)p.B * p.To * p.Ho * p.Wo;
    const long m0 = (long)blockIdx.x * BM;
    const int n0 = blockIdx.y * I3D_BN;
    const T* in = reinterpret_cast<const T*>(p.in);
    const T* w = reinterpret_cast<const T*>(p.w);

    const int nent = vec_mode ? Kpad / VEC : Kpad;
    for (int i = tid; i < nent; i += 256) tab[i] = tab_entry(p, vec_mode ? i * VEC : i, K);

    RowOrg org[ACH];
    int arow[ACH], ach[ACH];
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
        const int id = tid + 256 * i;
        arow[i] = id / CPR; ach[i] = id % CPR;
        long m = m0 + arow[i];
        org[i].ok = m < M;
        if (m >= M) m = M - 1;
        const int wo = (int)(m % p.Wo); m /= p.Wo;
        const int ho = (int)(m % p.Ho); m /= p.Ho;
        const int to = (int)(m % p.To);
        org[i].b = (int)(m / p.To);
        org[i].t = to * p.s[0] - p.pad_front[0];
        org[i].h = ho * p.s[1] - p.pad_front[1];
        org[i].w = wo * p.s[2] - p.pad_front[2];
    }
    int brow[BCH], bch[BCH];
#pragma unroll
    for (int i = 0; i < BCH; ++i) { const int id = tid + 256 * i; brow[i] = id / CPR; bch[i] = id % CPR; }
    __syncthreads();                                   // the K table

    f32x4 acc[WM][4];
    tile_zero(acc);

    u32x4 ra[ACH], rb[BCH];
    auto gload = [&](int kk) {
        const int kb = kk * I3D_BK;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const int k = kb + ach[i] * VEC;
            if (vec_mode) {
                size_t off;
                if (tap_offset<T>(p, org[i], tab[k / VEC], off)) ra[i] = *reinterpret_cast<const u32x4*>(in + off);
                else ra[i] = u32x4{0u, 0u, 0u, 0u};
            } else {
                T v[VEC];
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    size_t off;
                    v[e] = tap_offset<T>(p, org[i], tab[k + e], off) ? in[off] : (T)0;
                }
                __builtin_memcpy(&ra[i], v, sizeof(ra[i]));
            }
        }
#pragma unroll
        for (int i = 0; i < BCH; ++i)
            rb[i] = *reinterpret_cast<const u32x4*>(w + (size_t)(n0 + brow[i]) * Kpad + kb + bch[i] * VEC);
    };
    auto lstore = [&](int s) {
#pragma unroll
        for (int i = 0; i < ACH; ++i) *reinterpret_cast<u32x4*>(&sA[s][arow[i] * LD + ach[i] * VEC]) = ra[i];
#pragma unroll
        for (int i = 0; i < BCH; ++i) *reinterpret_cast<u32x4*>(&sB[s][brow[i] * LD + bch[i] * VEC]) = rb[i];
    };

    const int nk = Kpad / I3D_BK;
    gload(0);
    lstore(0);
    __syncthreads();
    const int fr = lane & 15, fq = lane >> 4;
    for (int kk = 0; kk < nk; ++kk) {
        const int s = kk & 1;
        if (kk + 1 < nk) gload(kk + 1);
        int ar[WM], br[4];
#pragma unroll
        for (int i = 0; i < WM; ++i) ar[i] = (16 * WM * wave + 16 * i + fr) * LD;
#pragma unroll
        for (int j = 0; j < 4; ++j) br[j] = (16 * j + fr) * LD;
        tile_mma<T, WM>(acc, sA[s], ar, sB[s], br, fq);
        if (kk + 1 < nk) lstore(s ^ 1);
        __syncthreads();
    }
    // tile_mma's fragment map: the lane holds output row (lane & 15) of row block i, columns 16 j + 4 (lane >> 4) .. + 3
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const long m = m0 + 16 * WM * wave + 16 * i + fr;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + 16 * j + 4 * fq + r;
                if (n >= p.Cout) continue;
                float v = acc[i][j][r] + (p.bias ? p.bias[n] : 0.f);
                if (p.relu) v = fmaxf(v, 0.f);
                int g = 0;
                while (g + 1 < p.nseg && n >= p.seg[g].n1) ++g;
                const mebt_i3d_seg& sg = p.seg[g];
                reinterpret_cast<T*>(sg.out)[(size_t)m * sg.cstride + sg.coff + (n - sg.n0)] = (T)v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// MaxPool3dSamePadding: F.pad with zeros, then the max (pytorch_i3d.py:13-46).  One thread per output element.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void i3d_maxpool_kernel(const T* in, T* out, int B, int Ti, int Hi, int Wi, int C, int To, int Ho, int Wo,
                                                          int kt, int kh, int kw, int st, int sh, int sw, int pt, int ph, int pw) {
    const long total = (long)B * To * Ho * Wo * C;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        long r = idx;
        const int c = (int)(r % C); r /= C;
        const int wo = (int)(r % Wo); r /= Wo;
        const int ho = (int)(r % Ho); r /= Ho;
        const int to = (int)(r % To);
        const int b = (int)(r / To);
        float v = -INFINITY;
        for (int dt = 0; dt < kt; ++dt) {
            const int ti = to * st - pt + dt;
            for (int dh = 0; dh < kh; ++dh) {
                const int hi = ho * sh - ph + dh;
                for (int dw = 0; dw < kw; ++dw) {
                    const int wi = wo * sw - pw + dw;
                    float x = 0.f;                      // a padded position holds 0
                    if ((unsigned)ti < (unsigned)Ti && (unsigned)hi < (unsigned)Hi && (unsigned)wi < (unsigned)Wi)
                        x = (float)in[((((size_t)b * Ti + ti) * Hi + hi) * Wi + wi) * C + c];
                    v = fmaxf(v, x);
                }
            }
        }
        out[idx] = (T)v;
    }
}

// ------------------------------------------------------------------------------------------------
// preprocess (fvd.py:17-28): uint8 frames [N, H, W, 3] -> bilinear (align_corners=False, source coordinate clamped at 0) to
// [N, Ho, Wo, 3] -> 2 x / 255 - 1, in ATen's upsample_bilinear2d order (height weights outside, width weights inside).
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void i3d_preprocess_kernel(const uint8_t* in, T* out, int N, int H, int W, int Ho, int Wo, float sy, float sx) {
    const long total = (long)N * Ho * Wo;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int x = (int)(idx % Wo);
        const int y = (int)((idx / Wo) % Ho);
        const long n = idx / ((long)Wo * Ho);
        float fy = sy * ((float)y + 0.5f) - 0.5f;
        fy = fy < 0.f ? 0.f : fy;
        float fx = sx * ((float)x + 0.5f) - 0.5f;
        fx = fx < 0.f ? 0.f : fx;
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 < H - 1 ? y0 + 1 : y0, x1 = x0 < W - 1 ? x0 + 1 : x0;
        const float ly1 = fy - (float)y0, ly0 = 1.f - ly1, lx1 = fx - (float)x0, lx0 = 1.f - lx1;
        const uint8_t* f = in + (size_t)n * H * W * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v00 = f[((size_t)y0 * W + x0) * 3 + c], v01 = f[((size_t)y0 * W + x1) * 3 + c];
            const float v10 = f[((size_t)y1 * W + x0) * 3 + c], v11 = f[((size_t)y1 * W + x1) * 3 + c];
            const float v = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
            out[idx * 3 + c] = (T)(2.0f * v / 255.0f - 1.0f);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// head (pytorch_i3d.py:324-331): AvgPool3d([2, 7, 7], stride 1) -> logits 1x1x1 conv with bias -> mean over time, in fp32
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void i3d_avgpool_kernel(const T* x, float* pooled, int B, int T_, int H, int W, int C) {
    const int Tp = T_ - 1;
    const long total = (long)B * Tp * C;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const int t = (int)((idx / C) % Tp);
    const int b = (int)(idx / ((long)C * Tp));
    float s = 0.f;
    for (int dt = 0; dt < 2; ++dt)
        for (int h = 0; h < H; ++h)
            for (int w = 0; w < W; ++w) s += (float)x[((((size_t)b * T_ + t + dt) * H + h) * W + w) * C + c];
    pooled[idx] = s / (float)(2 * H * W);
}

__global__ __launch_bounds__(256) void i3d_logits_kernel(const float* pooled, const float* w, const float* bias, float* logits, int B, int Tp, int C,
                                                         int ncls) {
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);          // one wave per (clip, class)
    const int lane = threadIdx.x & 63;
    if (item >= (long)B * ncls) return;
    const int n = (int)(item % ncls), b = (int)(item / ncls);
    float tot = 0.f;
    for (int t = 0; t < Tp; ++t) {
        const float* x = pooled + ((size_t)b * Tp + t) * C;
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += x[c] * w[(size_t)n * C + c];
        s = wave_sum(s);
        tot += s + (bias ? bias[n] : 0.f);
    }
    if (lane == 0) logits[item] = tot / (float)Tp;
}

int same_out(int size, int s) { return (size + s - 1) / s; }

}  // namespace

extern "C" int mebt_op_i3d_conv(int32_t dtype, const mebt_i3d_conv_desc* d, mebt_stream_t stream) {
    if (!d || !d->in || !d->w) { mebt_set_error("i3d_conv: null pointer"); return MEBT_EINVAL; }
    if (int rc = check_dtype("i3d_conv", dtype)) return rc;
    const mebt_i3d_conv_desc& p = *d;
    if (p.B < 1 || p.Ti < 1 || p.Hi < 1 || p.Wi < 1 || p.Cin < 1 || p.Cin > 0xFFFF || p.Cout < 1) {
        mebt_set_error("i3d_conv: bad shape"); return MEBT_EINVAL;
    }
    const int in_sz[3] = {p.Ti, p.Hi, p.Wi}, out_sz[3] = {p.To, p.Ho, p.Wo};
    for (int a = 0; a < 3; ++a) {
        if (p.k[a] < 1 || p.k[a] > 15 || p.s[a] < 1 || p.pad_front[a] < 0 || p.pad_back[a] < 0 || p.pad_front[a] >= p.k[a]) {
            mebt_set_error("i3d_conv: kernel / stride / padding out of range"); return MEBT_EINVAL;
        }
        if (out_sz[a] != (in_sz[a] + p.pad_front[a] + p.pad_back[a] - p.k[a]) / p.s[a] + 1 || out_sz[a] < 1) {
            mebt_set_error("i3d_conv: output size does not follow from input, kernel, stride and padding"); return MEBT_EINVAL;
        }
    }
    if (p.nseg < 1 || p.nseg > MEBT_I3D_MAX_SEGS || p.seg[0].n0 != 0 || p.seg[p.nseg - 1].n1 != p.Cout) {
        mebt_set_error("i3d_conv: the output segments must cover [0, Cout)"); return MEBT_EINVAL;
    }
    for (int g = 0; g < p.nseg; ++g) {
        const mebt_i3d_seg& s = p.seg[g];
        if (!s.out || s.n1 <= s.n0 || (g > 0 && s.n0 != p.seg[g - 1].n1) || s.coff < 0 || s.coff + (s.n1 - s.n0) > s.cstride) {
            mebt_set_error("i3d_conv: bad output segment (null, empty, not contiguous, or past its channel stride)"); return MEBT_EINVAL;
        }
    }
    const bool f16 = dtype == MEBT_DTYPE_F16;
    const int vec = f16 ? 8 : 4;
    const int K = p.k[0] * p.k[1] * p.k[2] * p.Cin;
    const int Kpad = (K + I3D_BK - 1) / I3D_BK * I3D_BK;
    const int vec_mode = p.Cin % vec == 0;
    if ((vec_mode ? Kpad / vec : Kpad) > I3D_MAX_TAB) { mebt_set_error("i3d_conv: K too long for the LDS tap table"); return MEBT_EINVAL; }
    if ((size_t)p.B * p.Ti * p.Hi * p.Wi > 0x7FFFFFFFull) { mebt_set_error("i3d_conv: input has more than 2^31 voxels"); return MEBT_EINVAL; }
    const long M = (long)p.B * p.To * p.Ho * p.Wo;
    const int bm = f16 ? TileCfg<f16_t>::BM : TileCfg<float>::BM;
    const long gx = (M + bm - 1) / bm;
    if (gx > 0x7FFFFFFFL) { mebt_set_error("i3d_conv: too many output voxels"); return MEBT_EINVAL; }
    const dim3 grid((unsigned)gx, (unsigned)((p.Cout + I3D_BN - 1) / I3D_BN));
    with_dtype(dtype, [&](auto tag) { hipLaunchKernelGGL(i3d_conv_kernel<decltype(tag)>, grid, dim3(256), 0, S(stream), p, vec_mode, Kpad); });
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int mebt_op_i3d_maxpool(int32_t dtype, const void* in, void* out, int32_t B, int32_t Ti, int32_t Hi, int32_t Wi, int32_t C,
                                   int32_t kt, int32_t kh, int32_t kw, int32_t st, int32_t sh, int32_t sw, mebt_stream_t stream) {
    if (!in || !out) { mebt_set_error("i3d_maxpool: null pointer"); return MEBT_EINVAL; }
    if (int rc = check_dtype("i3d_maxpool", dtype)) return rc;
    if (B < 1 || Ti < 1 || Hi < 1 || Wi < 1 || C < 1 || kt < 1 || kh < 1 || kw < 1 || st < 1 || sh < 1 || sw < 1) {
        mebt_set_error("i3d_maxpool: bad shape"); return MEBT_EINVAL;
    }
    // "same" padding (pytorch_i3d.py:15-19): only the front pad moves the window; the output size is ceil(size / stride)
    auto pad = [](int size, int k, int s) { const int t = size % s == 0 ? k - s : k - size % s; return t > 0 ? t : 0; };
    const int pt = pad(Ti, kt, st) / 2, ph = pad(Hi, kh, sh) / 2, pw = pad(Wi, kw, sw) / 2;
    const int To = same_out(Ti, st), Ho = same_out(Hi, sh), Wo = same_out(Wi, sw);
    const long total = (long)B * To * Ho * Wo * C;
    with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(i3d_maxpool_kernel<T>, dim3(grid_of(total)), dim3(256), 0, S(stream), reinterpret_cast<const T*>(in),
                           reinterpret_cast<T*>(out), B, Ti, Hi, Wi, C, To, Ho, Wo, kt, kh, kw, st, sh, sw, pt, ph, pw);
    });
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int mebt_op_i3d_preprocess(int32_t dtype, const uint8_t* in, void* out, int32_t N, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                                      mebt_stream_t stream) {
    if (!in || !out) { mebt_set_error("i3d_preprocess: null pointer"); return MEBT_EINVAL; }
    if (int rc = check_dtype("i3d_preprocess", dtype)) return rc;
    if (N < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1) { mebt_set_error("i3d_preprocess: bad shape"); return MEBT_EINVAL; }
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const long total = (long)N * Ho * Wo;
    const dim3 grid(grid_of(total));
    with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(i3d_preprocess_kernel<T>, grid, dim3(256), 0, S(stream), in, reinterpret_cast<T*>(out), N, H, W, Ho, Wo, sy, sx);
    });
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int mebt_op_i3d_head(int32_t dtype, const void* x, const float* w, const float* bias, float* pooled, float* logits, int32_t B, int32_t T,
                                int32_t H, int32_t W, int32_t C, int32_t ncls, mebt_stream_t stream) {
    if (!x || !w || !pooled || !logits) { mebt_set_error("i3d_head: null pointer"); return MEBT_EINVAL; }
    if (int rc = check_dtype("i3d_head", dtype)) return rc;
    if (B < 1 || T < 2 || H != 7 || W != 7 || C < 1 || ncls < 1) {
        mebt_set_error("i3d_head: expects [B, T >= 2, 7, 7, C] (AvgPool3d [2, 7, 7] to one spatial position)"); return MEBT_EINVAL;
    }
    const long np = (long)B * (T - 1) * C;
    const long nl = (long)B * ncls;
    const dim3 pool_grid((unsigned)((np + 255) / 256));
    with_dtype(dtype, [&](auto tag) {
        using E = decltype(tag);
        hipLaunchKernelGGL(i3d_avgpool_kernel<E>, pool_grid, dim3(256), 0, S(stream), reinterpret_cast<const E*>(x), pooled, B, T, H, W, C);
    });
    hipLaunchKernelGGL(i3d_logits_kernel, dim3((unsigned)((nl + 3) / 4)), dim3(256), 0, S(stream), pooled, w, bias, logits, B, T - 1, C, ncls);
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}
