// LPIPS backward for first-stage training (include/mebt_hip.h "LPIPS backward"; mebt_amd/lpips.py `LPIPS.value_and_grad`).
// The network's weights are frozen, so the backward is the data gradient alone: the head's backward at each slice output, the
// convolutions' data gradients (mebt_op_conv2d_3x3_dgrad, next to the forward template in lpips.hip), the 2x2 max pool's backward and
// the input scaling's backward into the fp32 seed video.  Activations and their gradients are channels-last [N, H, W, C], fp16 or fp32;
// every offset is 64-bit.  Nothing here adds into memory another thread writes and no reduction crosses a wave, so every run gives the
// same bits and an image's gradient does not depend on the batch it ran in.
#include <algorithm>
#include <vector>

#include "../host_util.h"

namespace {

// ---- head: one wave per pixel, as the forward ------------------------------------------------------------------------------------------
constexpr int HB_THREADS = 256, HB_WAVES = HB_THREADS / MEBT_WAVE;

// f [2 N, P, C]; pixel q of pair n: f0 = f[n, q, :], f1 = f[N + n, q, :].  k = -2 coef / P.
//   g_c = k w_c (f0_c / d0 - f1_c / d1),  df1_c = g_c / d1 - f1_c (sum_k g_k f1_k) / (|f1| d1^2),  d = |f| + 1e-10
// out[n, q, c] = f1_c > 0 ? df1_c + add[n, q, c] : 0.  Norms and the dot product: at most ceil(C / 64) fp32 terms per lane, then a
// fixed-order butterfly.
template <typename T>
__global__ __launch_bounds__(HB_THREADS) void lpips_head_bwd_kernel(const T* __restrict__ f, const float* __restrict__ w, const T* __restrict__ add,
                                                                    T* __restrict__ out, long long N, long long P, int C, float k, long long rows) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long long row = (long long)blockIdx.x * HB_WAVES + wave; row < rows; row += (long long)gridDim.x * HB_WAVES) {   // wave uniform
        const T* a = f + (size_t)row * (size_t)C;
        const T* b = f + ((size_t)N * (size_t)P + (size_t)row) * (size_t)C;
        float s0 = 0.f, s1 = 0.f;
        for (int c = lane; c < C; c += MEBT_WAVE) {
            const float u = (float)a[c], v = (float)b[c];
            s0 += u * u;
            s1 += v * v;
        }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        const float n1 = sqrtf(s1), d0 = sqrtf(s0) + 1e-10f, d1 = n1 + 1e-10f;
        float dot = 0.f;
        for (int c = lane; c < C; c += MEBT_WAVE) {
            const float v = (float)b[c];
            const float g = k * w[c] * ((float)a[c] / d0 - v / d1);
            dot += g * v;
        }
        dot = wave_sum(dot);
        const float back = n1 > 0.f ? dot / (n1 * d1 * d1) : 0.f;  // a zero vector: u = 0 / 1e-10 whatever the direction
        const size_t o = (size_t)row * (size_t)C;
        for (int c = lane; c < C; c += MEBT_WAVE) {
            const float v = (float)b[c];
            const float g = k * w[c] * ((float)a[c] / d0 - v / d1);
            float r = g / d1 - v * back;
            if (add) r += (float)add[o + c];
            out[o + c] = (T)(v > 0.f ? r : 0.f);
        }
    }
}

// ---- nn.MaxPool2d(2, 2) backward: VEC channels of one window per thread ----------------------------------------------------------------
// Windows are counted over ceil(H / 2) x ceil(W / 2) so that the trailing odd row and column, which no window of the forward covers,
// are written too (zeros).  The winner is the first maximum in the order (0, 0), (0, 1), (1, 0), (1, 1); it receives dy where its own
// value is positive (the pool reads a ReLU output: a window of zeros passes nothing on).
template <typename T, int VEC>
__global__ __launch_bounds__(256) void maxpool2x2_bwd_kernel(const T* __restrict__ in, const T* __restrict__ dy, T* __restrict__ dx, int H, int W,
                                                             int C, int Ho, int Wo, int Hc, int Wc, long long total) {
    struct alignas(sizeof(T) * VEC) V { T v[VEC]; };
    const int cv = C / VEC;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        long long r = idx;
        const int c = (int)(r % cv); r /= cv;
        const int xo = (int)(r % Wc); r /= Wc;
        const int yo = (int)(r % Hc);
        const long long n = r / Hc;
        const size_t base = (((size_t)n * H + 2 * yo) * (size_t)W + 2 * xo) * (size_t)C + (size_t)c * VEC;
        const size_t right = C, down = (size_t)W * C;
        const bool has_r = 2 * xo + 1 < W, has_d = 2 * yo + 1 < H;
        V z;
#pragma unroll
        for (int k = 0; k < VEC; ++k) z.v[k] = (T)0.f;
        if (yo >= Ho || xo >= Wo) {                                  // no window of the forward here
            *reinterpret_cast<V*>(dx + base) = z;
            if (has_r) *reinterpret_cast<V*>(dx + base + right) = z;
            if (has_d) *reinterpret_cast<V*>(dx + base + down) = z;
            continue;                                                // has_r && has_d would be a whole window
        }
        const V a = *reinterpret_cast<const V*>(in + base), b = *reinterpret_cast<const V*>(in + base + right);
        const V d = *reinterpret_cast<const V*>(in + base + down), e = *reinterpret_cast<const V*>(in + base + down + right);
        const V g = *reinterpret_cast<const V*>(dy + (((size_t)n * Ho + yo) * (size_t)Wo + xo) * (size_t)C + (size_t)c * VEC);
        V oa = z, ob = z, od = z, oe = z;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float va = (float)a.v[k], vb = (float)b.v[k], vd = (float)d.v[k], ve = (float)e.v[k];
            int win = 0;
            float m = va;
            if (vb > m) { m = vb; win = 1; }
            if (vd > m) { m = vd; win = 2; }
            if (ve > m) { m = ve; win = 3; }
            if (m > 0.f) {
                if (win == 0) oa.v[k] = g.v[k];
                else if (win == 1) ob.v[k] = g.v[k];
                else if (win == 2) od.v[k] = g.v[k];
                else oe.v[k] = g.v[k];
            }
        }
        *reinterpret_cast<V*>(dx + base) = oa;
        *reinterpret_cast<V*>(dx + base + right) = ob;
        *reinterpret_cast<V*>(dx + base + down) = od;
        *reinterpret_cast<V*>(dx + base + down + right) = oe;
    }
}

// ---- ScalingLayer backward into the fp32 seed video -------------------------------------------------------------------------------------
struct InvScale { float scale[3]; };

// seed[b, c, t, y, x] += factor * (d_in[n, y, x, c] / scale[c]) for (b, t) = frames[n]; the host has checked that the pairs are
// distinct and inside the video, so every seed element has one writer
template <typename T>
__global__ __launch_bounds__(256) void lpips_input_bwd_kernel(const T* __restrict__ d_in, const int32_t* __restrict__ frames,
                                                              float* __restrict__ seed, int Tn, int H, int W, long long total, float factor,
                                                              InvScale sc) {
    const long long hw = (long long)H * W;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long n = idx / hw, r = idx - n * hw;
        const int b = frames[2 * n], t = frames[2 * n + 1];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* s = seed + (((size_t)b * 3 + c) * (size_t)Tn + t) * (size_t)hw + r;
            *s = __fadd_rn(*s, __fmul_rn(factor, __fdiv_rn((float)d_in[idx * 3 + c], sc.scale[c])));
        }
    }
}

}  // namespace

extern "C" int mebt_op_lpips_head_bwd(int32_t dtype, const void* feats, const float* w, const void* add, void* d_feats, int64_t N, int64_t P,
                                      int32_t C, double coef, mebt_stream_t stream) {
    const char* who = "lpips_head_bwd";
    if (!feats || !w || !d_feats) return fail(MEBT_EINVAL, who, "null pointer");
    if (int rc = check_dtype(who, dtype)) return rc;
    if (N < 1 || P < 1 || C < 1 || P > (1ll << 40)) return fail(MEBT_ESHAPE, who, "need N, C >= 1 and 1 <= P <= 2^40");
    if (N > (1ll << 40) / P) return fail(MEBT_ESHAPE, who, "too many pixels");
    const float k = (float)(-2.0 * coef / (double)P);
    if (!(k == k) || k - k != 0.f) return fail(MEBT_EINVAL, who, "coef / P must be finite in fp32");
    const long long rows = (long long)N * P, g = (rows + HB_WAVES - 1) / HB_WAVES;
    const dim3 grid((unsigned)(g < 65536 ? g : 65536));
    with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(lpips_head_bwd_kernel<T>, grid, dim3(HB_THREADS), 0, S(stream), reinterpret_cast<const T*>(feats), w,
                           reinterpret_cast<const T*>(add), reinterpret_cast<T*>(d_feats), (long long)N, (long long)P, C, k, rows);
    });
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int mebt_op_maxpool_2x2_bwd(int32_t dtype, const void* in, const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C,
                                       mebt_stream_t stream) {
    const char* who = "maxpool_2x2_bwd";
    if (!in || !dy || !dx) return fail(MEBT_EINVAL, who, "null pointer");
    if (int rc = check_dtype(who, dtype)) return rc;
    if (N < 1 || C < 1) return fail(MEBT_ESHAPE, who, "need N, C >= 1");
    if (H < 2 || W < 2) return fail(MEBT_ESHAPE, who, "a 2 x 2 window needs H >= 2 and W >= 2");
    const int Ho = H / 2, Wo = W / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2;
    const int vec = dtype == MEBT_DTYPE_F16 ? 8 : 4;
    const bool wide = C % vec == 0 && aligned16(in) && aligned16(dy) && aligned16(dx);
    const long long total = (long long)N * Hc * Wc * (wide ? C / vec : C);
    const dim3 grid(grid_of(total)), block(256);
    with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        const T* i = reinterpret_cast<const T*>(in);
        const T* g = reinterpret_cast<const T*>(dy);
        T* o = reinterpret_cast<T*>(dx);
        if (wide) hipLaunchKernelGGL((maxpool2x2_bwd_kernel<T, 16 / sizeof(T)>), grid, block, 0, S(stream), i, g, o, H, W, C, Ho, Wo, Hc, Wc, total);
        else hipLaunchKernelGGL((maxpool2x2_bwd_kernel<T, 1>), grid, block, 0, S(stream), i, g, o, H, W, C, Ho, Wo, Hc, Wc, total);
    });
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int mebt_op_lpips_input_bwd(int32_t dtype, const void* d_in, const int32_t* frames, const int32_t* frames_host, float* seed, int32_t B,
                                       int32_t T, int32_t H, int32_t W, int64_t n_frames, const float* scale, float factor,
                                       mebt_stream_t stream) {
    const char* who = "lpips_input_bwd";
    if (!d_in || !frames || !frames_host || !seed || !scale) return fail(MEBT_EINVAL, who, "null pointer");
    if (int rc = check_dtype(who, dtype)) return rc;
    if (B < 1 || T < 1 || H < 1 || W < 1 || n_frames < 1) return fail(MEBT_ESHAPE, who, "need B, T, H, W, n_frames >= 1");
    if (n_frames > (int64_t)B * T) return fail(MEBT_EINVAL, who, "more frames than the video holds: the (b, t) pairs must be distinct");
    if (n_frames > (1ll << 40) / ((int64_t)H * W)) return fail(MEBT_ESHAPE, who, "too many pixels");
    int e = 0;
    const float m = frexpf(factor, &e);
    if (!(factor > 0.f) || factor - factor != 0.f || m != 0.5f) return fail(MEBT_EINVAL, who, "factor must be a positive power of two");
    InvScale sc;
    for (int c = 0; c < 3; ++c) {
        sc.scale[c] = scale[c];
        if (!(scale[c] != 0.f)) return fail(MEBT_EINVAL, who, "scale must be non-zero");
    }
    std::vector<int64_t> keys((size_t)n_frames);
    for (int64_t n = 0; n < n_frames; ++n) {
        const int32_t b = frames_host[2 * n], t = frames_host[2 * n + 1];
        if (b < 0 || b >= B || t < 0 || t >= T) return fail(MEBT_EINVAL, who, "a (b, t) pair lies outside the video");
        keys[(size_t)n] = (int64_t)b * T + t;
    }
    std::sort(keys.begin(), keys.end());
    if (std::adjacent_find(keys.begin(), keys.end()) != keys.end())
        return fail(MEBT_EINVAL, who, "the (b, t) pairs must be distinct: each seed element has one writer");
    const long long total = (long long)n_frames * H * W;
    with_dtype(dtype, [&](auto tag) {
        using E = decltype(tag);
        hipLaunchKernelGGL(lpips_input_bwd_kernel<E>, dim3(grid_of(total)), dim3(256), 0, S(stream), reinterpret_cast<const E*>(d_in), frames, seed,
                           T, H, W, total, factor, sc);
    });
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}
