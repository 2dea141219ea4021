// LPIPS (VGG-16 perceptual distance) for the first-stage validation (include/mebt_hip.h "LPIPS"; mebt_amd/lpips.py; reference
// mebt/modules/lpips.py): the input scaling, a 3x3 convolution with bias and ReLU, the 2x2 max pool and the normalise / difference /
// 1x1 `lin` / spatial-mean head.  Activations are channels-last [N, H, W, C], fp16 (fast) or fp32 (parity); every offset is 64-bit.
//
// Convolution.  A workgroup owns BM output pixels (128 fp16, 64 fp32) and 64 output channels.  The BM pixels are G rectangular patches
// of PH x PW pixels (powers of two, PH * PW * G = BM; G = 1 with an 8 x 16 patch on the large maps, several small patches, of several
// images if need be, on the 8 x 8 ... 1 x 1 maps).  Per 32-channel slice of the input the workgroup stages every patch with its one-pixel
// halo into LDS once, positions outside the image as zeros, and serves the nine taps from shifted windows of that image: a lane's A
// fragment of tap (dh, dw) is the 32 channels at LDS position `own + (dh - 1) * (PW + 2) + (dw - 1)`, no branch in the tap loop.  The
// weights [Cout_pad64][Kpad32], K = (tap, ci) with ci fastest (the layout mebt_op_i3d_conv reads), are staged one kernel row (three
// taps) of the slice at a time; the next stage's operands are fetched into registers while the current one is multiplied.  An
// output's accumulation order is (slice, dh, dw, channel) whatever the batch, the patch shape or the tile it falls in: no split-K.
// The first layer (Cin = 3, K = 27 padded to 32) is a kernel of its own: one im2col tile, one K step.
// The data gradient of training (mebt_op_conv2d_3x3_dgrad; the rest of the backward is lpips_bwd.hip) is the same kernel on flipped,
// transposed weights, instantiated with MASK: its epilogue keeps a result only where the forward activation below was positive.
//
// Head.  One wave per pixel: channel norms and the weighted squared difference in fp32 (at most C / 64 terms per lane between
// fixed-order butterflies), fp64 from there; one fp64 partial per workgroup in the caller's scratch, added in index order by a
// second kernel (csrc/block_reduce.h: no float atomics, the same bits on every run).
#include "../block_reduce.h"
#include "../host_util.h"
#include "../mfma_tile.h"

namespace {

constexpr int CV_BK = TILE_BK, CV_BN = TILE_BN, CV_THREADS = TILE_THREADS;

struct ConvArgs {
    const void* in; const void* w; const float* bias; void* out;
    const void* mask;               // MASK kernels only: the output is kept where mask (the output's shape) is positive, else 0
    int N, H, W, Cin, Cout, Kpad, relu;
    int PH, PW, G, PY, PX;          // patch rows / columns, patches per tile, patches per image down / across
    long long NP;                   // patches of the whole batch
};

// lane's four consecutive output channels n0 + 16 j + 4 fq + (0..3) of one pixel, for j = 0..3
// MASK (the data gradient, mebt_op_conv2d_3x3_dgrad): m is the pixel of the forward activation below, the ReLU's backward is fused
template <typename T, bool MASK = false>
__device__ __forceinline__ void store_pixel(T* o, const f32x4* acc, int n0, int fq, const ConvArgs& p, const T* m = nullptr) {
    const bool vec = (p.Cout & 3) == 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int nb = n0 + 16 * j + 4 * fq;
        if (nb >= p.Cout) continue;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = nb + r;
            v[r] = acc[j][r] + ((p.bias && n < p.Cout) ? p.bias[n] : 0.f);
            if (p.relu) v[r] = fmaxf(v[r], 0.f);
            if constexpr (MASK) {
                if (n < p.Cout && !((float)m[n] > 0.f)) v[r] = 0.f;
            }
        }
        if (vec) {
            if constexpr (sizeof(T) == 2) *reinterpret_cast<f16x4*>(o + nb) = f16x4{(f16_t)v[0], (f16_t)v[1], (f16_t)v[2], (f16_t)v[3]};
            else *reinterpret_cast<f32x4*>(o + nb) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (nb + r < p.Cout) o[nb + r] = (T)v[r];
        }
    }
}

// staged positions (patches with their halos) of the small-patch instantiation; the large-patch one holds 4 BM
template <typename T> constexpr int NPOS_SMALL = sizeof(T) == 2 ? 208 : 128;

template <typename T, int NPOS, bool MASK = false>
__global__ __launch_bounds__(CV_THREADS) void conv3x3_kernel(const ConvArgs p) {
    using Cfg = TileCfg<T>;
    constexpr int VEC = Cfg::VEC, LD = Cfg::LD, WM = Cfg::WM;
    constexpr int CPR = CV_BK / VEC;                                 // 16-byte chunks per 32-channel row
    constexpr int ACH = (NPOS * CPR + CV_THREADS - 1) / CV_THREADS;  // patch chunks per thread
    constexpr int BCH = CV_BN * 3 * CPR / CV_THREADS;                // weight chunks per thread (3 fp16, 6 fp32)
    static_assert(CV_BN * 3 * CPR % CV_THREADS == 0, "weight chunks divide evenly");
    __shared__ __attribute__((aligned(16))) T sA[NPOS * LD];         // [position][32 channels]
    __shared__ __attribute__((aligned(16))) T sB[CV_BN * 3 * LD];    // [output channel][dw][32 channels]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int LW = p.PW + 2, ppos = (p.PH + 2) * LW, npos = p.G * ppos;
    const int ppatch = p.PH * p.PW, ppi = p.PY * p.PX;
    const long long q0 = (long long)blockIdx.x * p.G;
    const int n0 = blockIdx.y * CV_BN;
    const T* in = reinterpret_cast<const T*>(p.in);
    const T* w = reinterpret_cast<const T*>(p.w);

    // where each of this thread's patch chunks comes from: element offset at slice 0, -1 = zeros (outside the image or past the
    // last patch), -2 = past the staged positions (nothing is written)
    long long aoff[ACH];
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
        const int id = tid + CV_THREADS * i;
        const int pos = id / CPR, ch = id % CPR;
        aoff[i] = -2;
        if (pos < npos) {
            const int g = pos / ppos, rem = pos - g * ppos;
            const int pr = rem / LW, pc = rem - pr * LW;
            const long long q = q0 + g;
            aoff[i] = -1;
            if (q < p.NP) {
                const long long n = q / ppi;
                const int r2 = (int)(q - n * ppi), py = r2 / p.PX, px = r2 - py * p.PX;
                const int y = py * p.PH + pr - 1, x = px * p.PW + pc - 1;
                if ((unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W)
                    aoff[i] = ((n * p.H + y) * p.W + x) * p.Cin + ch * VEC;
            }
        }
    }
    int apos[WM];                                                    // LDS position of the lane's own pixel in each of its blocks
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const int row = 16 * WM * wave + 16 * i + fr;
        const int g = row / ppatch, rr = row - g * ppatch;
        const int r = rr / p.PW, c = rr - r * p.PW;
        apos[i] = g * ppos + (r + 1) * LW + c + 1;
    }

    u32x4 ra[ACH], rb[BCH];
    auto gloadA = [&](int slice) {
#pragma unroll
        for (int i = 0; i < ACH; ++i)
            ra[i] = aoff[i] >= 0 ? *reinterpret_cast<const u32x4*>(in + aoff[i] + slice * CV_BK) : u32x4{0u, 0u, 0u, 0u};
    };
    auto lstoreA = [&]() {
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const int id = tid + CV_THREADS * i;
            if (aoff[i] != -2) *reinterpret_cast<u32x4*>(&sA[(id / CPR) * LD + (id % CPR) * VEC]) = ra[i];
        }
    };
    auto gloadB = [&](int st) {
        const int slice = st / 3, dh = st - 3 * slice;
#pragma unroll
        for (int i = 0; i < BCH; ++i) {
            const int id = tid + CV_THREADS * i;
            const int n = id / (3 * CPR), rem = id - n * 3 * CPR, dw = rem / CPR, ch = rem - dw * CPR;
            rb[i] = *reinterpret_cast<const u32x4*>(w + (size_t)(n0 + n) * p.Kpad + (size_t)(dh * 3 + dw) * p.Cin + slice * CV_BK + ch * VEC);
        }
    };
    auto lstoreB = [&]() {
#pragma unroll
        for (int i = 0; i < BCH; ++i) {
            const int id = tid + CV_THREADS * i;
            const int n = id / (3 * CPR), rem = id - n * 3 * CPR, dw = rem / CPR, ch = rem - dw * CPR;
            *reinterpret_cast<u32x4*>(&sB[(n * 3 + dw) * LD + ch * VEC]) = rb[i];
        }
    };

    f32x4 acc[WM][4];
    tile_zero(acc);

    const int nst = (p.Cin / CV_BK) * 3;                             // stages: (slice, dh)
    gloadA(0);
    gloadB(0);
    lstoreA();
    lstoreB();
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int nxt = st + 1;
        const bool more = nxt < nst, new_slice = more && nxt % 3 == 0;
        if (more) gloadB(nxt);
        if (new_slice) gloadA(nxt / 3);
        const int shift = (st % 3 - 1) * LW - 1;                      // window of tap (dh, 0)
#pragma unroll
        for (int dw = 0; dw < 3; ++dw) {
            int ar[WM], br[4];
#pragma unroll
            for (int i = 0; i < WM; ++i) ar[i] = (apos[i] + shift + dw) * LD;
#pragma unroll
            for (int j = 0; j < 4; ++j) br[j] = ((16 * j + fr) * 3 + dw) * LD;
            tile_mma<T, WM>(acc, sA, ar, sB, br, fq);
        }
        __syncthreads();
        if (more) lstoreB();
        if (new_slice) lstoreA();
        __syncthreads();
    }

    // tile_mma's fragment map: the lane holds pixel (lane & 15) of block i, channels 16 j + 4 (lane >> 4) .. + 3
    T* out = reinterpret_cast<T*>(p.out);
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const int row = 16 * WM * wave + 16 * i + fr;
        const int g = row / ppatch, rr = row - g * ppatch;
        const int r = rr / p.PW, c = rr - r * p.PW;
        const long long q = q0 + g;
        if (q >= p.NP) continue;
        const long long n = q / ppi;
        const int r2 = (int)(q - n * ppi), py = r2 / p.PX, px = r2 - py * p.PX;
        const int y = py * p.PH + r, x = px * p.PW + c;
        if (y >= p.H || x >= p.W) continue;
        const size_t o = (size_t)((n * p.H + y) * p.W + x) * (size_t)p.Cout;
        if constexpr (MASK) store_pixel<T, true>(out + o, acc[i], n0, fq, p, reinterpret_cast<const T*>(p.mask) + o);
        else store_pixel<T>(out + o, acc[i], n0, fq, p);
    }
}

// Cin = 3: rows are the flat (image, pixel) index; the 27 taps x channels of a row are gathered into one K step
template <typename T>
__global__ __launch_bounds__(CV_THREADS) void conv3x3_c3_kernel(const ConvArgs p, long long M) {
    using Cfg = TileCfg<T>;
    constexpr int VEC = Cfg::VEC, BM = Cfg::BM, LD = Cfg::LD, WM = Cfg::WM;
    constexpr int CPR = CV_BK / VEC;
    __shared__ __attribute__((aligned(16))) T sA[BM * LD];
    __shared__ __attribute__((aligned(16))) T sB[CV_BN * LD];
    __shared__ long long s_pix[BM];                                  // pixel index (n * H + y) * W + x of the row, -1 past M
    __shared__ int s_y[BM], s_x[BM];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const long long m0 = (long long)blockIdx.x * BM;
    const int n0 = blockIdx.y * CV_BN;
    const T* in = reinterpret_cast<const T*>(p.in);
    const T* w = reinterpret_cast<const T*>(p.w);

    if (tid < BM) {
        const long long m = m0 + tid;
        s_pix[tid] = m < M ? m : -1;
        const long long t = m / p.W;
        s_x[tid] = (int)(m - t * p.W);
        s_y[tid] = (int)(t % p.H);
    }
    for (int e = tid; e < CV_BN * CPR; e += CV_THREADS) {
        const int n = e / CPR, ch = e - n * CPR;
        *reinterpret_cast<u32x4*>(&sB[n * LD + ch * VEC]) = *reinterpret_cast<const u32x4*>(w + (size_t)(n0 + n) * CV_BK + ch * VEC);
    }
    __syncthreads();
    {
        const int k = tid & 31, tap = k / 3, ci = k - 3 * tap, dh = tap / 3 - 1, dw = tap % 3 - 1;
        for (int row = tid >> 5; row < BM; row += CV_THREADS / 32) {
            T v = (T)0.f;
            const long long pix = s_pix[row];
            if (k < 27 && pix >= 0) {
                const int y = s_y[row] + dh, x = s_x[row] + dw;
                if ((unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W) v = in[(size_t)(pix + (long long)dh * p.W + dw) * 3 + ci];
            }
            sA[row * LD + k] = v;
        }
    }
    __syncthreads();

    f32x4 acc[WM][4];
    tile_zero(acc);
    int ar[WM], br[4];
#pragma unroll
    for (int i = 0; i < WM; ++i) ar[i] = (16 * WM * wave + 16 * i + fr) * LD;
#pragma unroll
    for (int j = 0; j < 4; ++j) br[j] = (16 * j + fr) * LD;
    tile_mma<T, WM>(acc, sA, ar, sB, br, fq);
    T* out = reinterpret_cast<T*>(p.out);                           // tile_mma's fragment map: the lane holds row (lane & 15) of block i
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const long long pix = s_pix[16 * WM * wave + 16 * i + fr];
        if (pix < 0) continue;
        store_pixel<T>(out + (size_t)pix * (size_t)p.Cout, acc[i], n0, fq, p);
    }
}

// ---- (x - shift) / scale of chosen frames of a video, channels-last ----------------------------------------------------------------
struct Scaling { float shift[3], scale[3]; };

template <typename T>
__global__ __launch_bounds__(256) void lpips_input_kernel(const float* __restrict__ video, const int32_t* __restrict__ frames,
                                                          T* __restrict__ out, int B, int Tn, int H, int W, long long total, Scaling sc) {
    const long long hw = (long long)H * W;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long n = idx / hw, r = idx - n * hw;
        const int b = frames[2 * n], t = frames[2 * n + 1];
        const bool ok = (unsigned)b < (unsigned)B && (unsigned)t < (unsigned)Tn;          // a pair outside the video reads nothing
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = 0.f;
            if (ok) v = __fdiv_rn(__fsub_rn(video[(((size_t)b * 3 + c) * (size_t)Tn + t) * (size_t)hw + r], sc.shift[c]), sc.scale[c]);
            out[idx * 3 + c] = (T)v;
        }
    }
}

// ---- nn.MaxPool2d(2, 2): VEC channels of one output pixel per thread ------------------------------------------------------------------
template <typename T, int VEC>
__global__ __launch_bounds__(256) void maxpool2x2_kernel(const T* __restrict__ in, T* __restrict__ out, int H, int W, int C, int Ho, int Wo,
                                                         long long total) {
    struct alignas(sizeof(T) * VEC) V { T v[VEC]; };
    const int cv = C / VEC;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        long long r = idx;
        const int c = (int)(r % cv); r /= cv;
        const int xo = (int)(r % Wo); r /= Wo;
        const int yo = (int)(r % Ho);
        const long long n = r / Ho;
        const T* src = in + (((size_t)n * H + 2 * yo) * (size_t)W + 2 * xo) * (size_t)C + (size_t)c * VEC;
        const V a = *reinterpret_cast<const V*>(src), b = *reinterpret_cast<const V*>(src + C);
        const V d = *reinterpret_cast<const V*>(src + (size_t)W * C), e = *reinterpret_cast<const V*>(src + (size_t)W * C + C);
        V o;
#pragma unroll
        for (int k = 0; k < VEC; ++k) o.v[k] = (T)fmaxf(fmaxf((float)a.v[k], (float)b.v[k]), fmaxf((float)d.v[k], (float)e.v[k]));
        *reinterpret_cast<V*>(out + idx * VEC) = o;
    }
}

// ---- head ----------------------------------------------------------------------------------------------------------------------------
constexpr int HD_THREADS = 256, HD_WAVES = HD_THREADS / MEBT_WAVE, HD_ROWS = MEBT_LPIPS_HEAD_ROWS;

// workgroup (n, k) takes pixels [k * HD_ROWS, (k + 1) * HD_ROWS) of pair n, wave w pixels w, w + 4, ... in turn
template <typename T>
__global__ __launch_bounds__(HD_THREADS) void lpips_head_kernel(const T* __restrict__ f, const float* __restrict__ w, double* __restrict__ part,
                                                                long long N, long long P, int C, long long blocks) {
    __shared__ double sh[HD_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long n = blockIdx.x / blocks, k = blockIdx.x - n * blocks;
    double acc = 0.0;
    for (int j = wave; j < HD_ROWS; j += HD_WAVES) {
        const long long px = k * HD_ROWS + j;
        if (px >= P) break;                                          // wave uniform
        const T* a = f + ((size_t)n * (size_t)P + (size_t)px) * (size_t)C;
        const T* b = f + ((size_t)(N + n) * (size_t)P + (size_t)px) * (size_t)C;
        float s0 = 0.f, s1 = 0.f;
        for (int c = lane; c < C; c += MEBT_WAVE) {
            const float u = (float)a[c], v = (float)b[c];
            s0 += u * u;
            s1 += v * v;
        }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        const float d0 = sqrtf(s0) + 1e-10f, d1 = sqrtf(s1) + 1e-10f;  // the eps outside the root: a zero vector gives 0 / 1e-10 = 0
        float t = 0.f;
        for (int c = lane; c < C; c += MEBT_WAVE) {
            const float d = (float)a[c] / d0 - (float)b[c] / d1;
            t += w[c] * (d * d);
        }
        acc += wave_sum((double)t);
    }
    const double s = waves_sum<HD_WAVES>(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// out[n] += v, layer_out[n * layer_stride] = v, v = inv_p * (part[n * blocks + 0] + part[n * blocks + 1] + ...), the slots in
// slot_sum's order
__global__ __launch_bounds__(HD_THREADS) void lpips_head_finish_kernel(const double* __restrict__ part, long long blocks, double* __restrict__ out,
                                                                       double* __restrict__ layer_out, long long layer_stride, double inv_p) {
    __shared__ double sh[HD_WAVES];
    const double v = slot_sum<HD_THREADS>(part + (size_t)blockIdx.x * (size_t)blocks, blocks, sh);
    if (threadIdx.x == 0) {
        // the product is rounded before it is added (no fused multiply-add): out accumulates exactly the values layer_out receives
#pragma clang fp contract(off)
        const double s = v * inv_p;
        out[blockIdx.x] = out[blockIdx.x] + s;
        if (layer_out) layer_out[(size_t)blockIdx.x * (size_t)layer_stride] = s;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
template <typename T, bool MASK = false>
int launch_conv(ConvArgs a, hipStream_t stream) {
    using Cfg = TileCfg<T>;
    const unsigned gy = (unsigned)((a.Cout + CV_BN - 1) / CV_BN);
    if (!MASK && a.Cin == 3) {
        const long long M = (long long)a.N * a.H * a.W, gx = (M + Cfg::BM - 1) / Cfg::BM;
        if (gx > 0x7FFFFFFFll) return fail(MEBT_ESHAPE, "conv2d_3x3", "too many output pixels for one launch");
        hipLaunchKernelGGL(conv3x3_c3_kernel<T>, dim3((unsigned)gx, gy), dim3(CV_THREADS), 0, stream, a, M);
        MEBT_HIP_CHECK(hipGetLastError());
        return MEBT_OK;
    }
    // the patch: as wide as the map up to 16 columns, then as tall as the map up to BM pixels; the rest of the tile is more patches
    int pw = 2, ph = 2;
    while (pw < 16 && pw < a.W) pw *= 2;
    while (ph * pw < Cfg::BM && ph < a.H) ph *= 2;
    a.PW = pw; a.PH = ph; a.G = Cfg::BM / (ph * pw);
    a.PY = (a.H + ph - 1) / ph; a.PX = (a.W + pw - 1) / pw;
    a.NP = (long long)a.N * a.PY * a.PX;
    const long long gx = (a.NP + a.G - 1) / a.G;
    if (gx > 0x7FFFFFFFll) return fail(MEBT_ESHAPE, "conv2d_3x3", "too many output pixels for one launch");
    const int npos = a.G * (ph + 2) * (pw + 2);                     // <= 4 BM
    const dim3 grid((unsigned)gx, gy);
    if (npos <= NPOS_SMALL<T>) hipLaunchKernelGGL((conv3x3_kernel<T, NPOS_SMALL<T>, MASK>), grid, dim3(CV_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((conv3x3_kernel<T, 4 * Cfg::BM, MASK>), grid, dim3(CV_THREADS), 0, stream, a);
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

}  // namespace

extern "C" int mebt_op_lpips_input(int32_t dtype, const float* video, const int32_t* frames, void* out, int32_t B, int32_t T, int32_t H, int32_t W,
                                   int64_t n_frames, const float* shift, const float* scale, mebt_stream_t stream) {
    const char* who = "lpips_input";
    if (!video || !frames || !out || !shift || !scale) return fail(MEBT_EINVAL, who, "null pointer");
    if (int rc = check_dtype(who, dtype)) return rc;
    if (B < 1 || T < 1 || H < 1 || W < 1 || n_frames < 1) return fail(MEBT_ESHAPE, who, "need B, T, H, W, n_frames >= 1");
    if (n_frames > (1ll << 40) / ((int64_t)H * W)) return fail(MEBT_ESHAPE, who, "too many pixels");
    Scaling sc;
    for (int c = 0; c < 3; ++c) {
        sc.shift[c] = shift[c];
        sc.scale[c] = scale[c];
        if (!(scale[c] != 0.f)) return fail(MEBT_EINVAL, who, "scale must be non-zero");
    }
    const long long total = (long long)n_frames * H * W;
    with_dtype(dtype, [&](auto tag) {
        using E = decltype(tag);
        hipLaunchKernelGGL(lpips_input_kernel<E>, dim3(grid_of(total)), dim3(256), 0, S(stream), video, frames, reinterpret_cast<E*>(out), B, T, H, W,
                           total, sc);
    });
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int mebt_op_conv2d_3x3(int32_t dtype, const void* in, const void* w, const float* bias, void* out, int32_t N, int32_t H, int32_t W,
                                  int32_t Cin, int32_t Cout, int32_t relu, mebt_stream_t stream) {
    const char* who = "conv2d_3x3";
    if (!in || !w || !out) return fail(MEBT_EINVAL, who, "null pointer");
    if (int rc = check_dtype(who, dtype)) return rc;
    if (N < 1 || H < 1 || W < 1 || Cout < 1) return fail(MEBT_ESHAPE, who, "need N, H, W, Cout >= 1");
    if (H > (1 << 20) || W > (1 << 20)) return fail(MEBT_ESHAPE, who, "map too large");
    if (!(Cin == 3 || (Cin >= 32 && Cin % 32 == 0 && Cin <= 512))) return fail(MEBT_ESHAPE, who, "need Cin == 3, or Cin a multiple of 32 up to 512");
    if (!aligned16(in) || !aligned16(w) || !aligned16(out)) return fail(MEBT_EINVAL, who, "in, w and out must be 16-byte aligned");
    ConvArgs a{};
    a.in = in; a.w = w; a.bias = bias; a.out = out;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.relu = relu != 0;
    a.Kpad = (9 * Cin + CV_BK - 1) / CV_BK * CV_BK;
    return with_dtype(dtype, [&](auto tag) { return launch_conv<decltype(tag)>(a, S(stream)); });
}

// The data gradient of the convolution above: the same kernel on `arrange_weight_dgrad`'s weights (taps flipped, channels swapped),
// no bias, no ReLU; with y_prev the epilogue keeps the result only where the forward activation below was positive.
extern "C" int mebt_op_conv2d_3x3_dgrad(int32_t dtype, const void* dy, const void* w_dgrad, const void* y_prev, void* dx, int32_t N, int32_t H,
                                        int32_t W, int32_t Cin, int32_t Cout, mebt_stream_t stream) {
    const char* who = "conv2d_3x3_dgrad";
    if (!dy || !w_dgrad || !dx) return fail(MEBT_EINVAL, who, "null pointer");
    if (int rc = check_dtype(who, dtype)) return rc;
    if (N < 1 || H < 1 || W < 1 || Cout < 1) return fail(MEBT_ESHAPE, who, "need N, H, W, Cout >= 1");
    if (H > (1 << 20) || W > (1 << 20)) return fail(MEBT_ESHAPE, who, "map too large");
    if (!(Cin >= 32 && Cin % 32 == 0 && Cin <= 512)) return fail(MEBT_ESHAPE, who, "need Cin (the forward's Cout) a multiple of 32 up to 512");
    if (!aligned16(dy) || !aligned16(w_dgrad) || !aligned16(dx) || !aligned16(y_prev))
        return fail(MEBT_EINVAL, who, "dy, w_dgrad, y_prev and dx must be 16-byte aligned");
    ConvArgs a{};
    a.in = dy; a.w = w_dgrad; a.bias = nullptr; a.out = dx; a.mask = y_prev;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.relu = 0;
    a.Kpad = (9 * Cin + CV_BK - 1) / CV_BK * CV_BK;
    return with_dtype(dtype, [&](auto tag) {
        return y_prev ? launch_conv<decltype(tag), true>(a, S(stream)) : launch_conv<decltype(tag)>(a, S(stream));
    });
}

extern "C" int mebt_op_maxpool_2x2(int32_t dtype, const void* in, void* out, int32_t N, int32_t H, int32_t W, int32_t C, mebt_stream_t stream) {
    const char* who = "maxpool_2x2";
    if (!in || !out) return fail(MEBT_EINVAL, who, "null pointer");
    if (int rc = check_dtype(who, dtype)) return rc;
    if (N < 1 || C < 1) return fail(MEBT_ESHAPE, who, "need N, C >= 1");
    if (H < 2 || W < 2) return fail(MEBT_ESHAPE, who, "a 2 x 2 window needs H >= 2 and W >= 2");
    const int Ho = H / 2, Wo = W / 2;
    const int vec = dtype == MEBT_DTYPE_F16 ? 8 : 4;
    const bool wide = C % vec == 0 && aligned16(in) && aligned16(out);
    const long long total = (long long)N * Ho * Wo * (wide ? C / vec : C);
    const dim3 grid(grid_of(total)), block(256);
    with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        const T* i = reinterpret_cast<const T*>(in);
        T* o = reinterpret_cast<T*>(out);
        if (wide) hipLaunchKernelGGL((maxpool2x2_kernel<T, 16 / sizeof(T)>), grid, block, 0, S(stream), i, o, H, W, C, Ho, Wo, total);
        else hipLaunchKernelGGL((maxpool2x2_kernel<T, 1>), grid, block, 0, S(stream), i, o, H, W, C, Ho, Wo, total);
    });
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int mebt_op_lpips_head(int32_t dtype, const void* feats, const float* w, double* out, double* layer_out, int64_t layer_stride,
                                  int64_t N, int64_t P, int32_t C, void* scratch, int64_t scratch_bytes, mebt_stream_t stream) {
    const char* who = "lpips_head";
    if (!feats || !w || !out) return fail(MEBT_EINVAL, who, "null pointer");
    if (int rc = check_dtype(who, dtype)) return rc;
    if (N < 1 || P < 1 || C < 1 || P > (1ll << 40)) return fail(MEBT_ESHAPE, who, "need N, C >= 1 and 1 <= P <= 2^40");
    if (layer_out && layer_stride < 1) return fail(MEBT_EINVAL, who, "layer_stride must be >= 1");
    const long long blocks = (P + HD_ROWS - 1) / HD_ROWS;
    if (N > 0x7FFFFFFFll / blocks) return fail(MEBT_ESHAPE, who, "too large for one launch");           // before N * blocks can overflow
    if (int rc = check_scratch(who, scratch, scratch_bytes, 8 * N * blocks, N * blocks)) return rc;
    double* part = reinterpret_cast<double*>(scratch);
    const dim3 grid((unsigned)(N * blocks));
    with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(lpips_head_kernel<T>, grid, dim3(HD_THREADS), 0, S(stream), reinterpret_cast<const T*>(feats), w, part, (long long)N,
                           (long long)P, C, blocks);
    });
    MEBT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lpips_head_finish_kernel, dim3((unsigned)N), dim3(HD_THREADS), 0, S(stream), part, blocks, out, layer_out,
                       (long long)layer_stride, 1.0 / (double)P);
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}
