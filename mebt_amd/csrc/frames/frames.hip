// Frame ingest for pixel-space training (reference mebt/data.py FrameListDataset.getTensor): uint8 RGB frames [N, Hs, Ws, 3]
// -> center crop to the shorter side -> PIL `Image.resize((R, R), BILINEAR)` -> float32(u) / 255 - 0.5, written as the
// reference's clip layout [B, 3, T, R, R] (N = B * T, frame n = clip n / T, time n % T).
//
// Pillow's 8-bit resampler is integer arithmetic once its coefficients are fixed; the host builds them exactly as Pillow does
// (mebt_amd/frames.py:axis_coeffs) and passes one table for both axes (the crop is square): xmin[R], n[R], k[R][K] int32.
// Each pass computes acc = 1 << 21 + sum(k * px) in int32 and keeps clamp(acc >> 22, 0, 255); the horizontal pass runs first and
// its result is uint8, as in Pillow.  There is no floating point before the final table lookup, so the output equals PIL's.
//
// One workgroup per (frame, tile of `rows` output rows): the horizontal pass resamples the source rows the tile needs
// [xmin[r0], xmin[r1] + n[r1]) into LDS as uint8, the vertical pass reads them back and stores one fp32 plane per channel, lanes
// along W.  Same-size frames (crop side == R) take a second kernel: crop + normalise + HWC -> CHW transpose.
#include "../common.h"
#include "../../../include/mebt_hip.h"

namespace {

constexpr int FR_THREADS = 256;
constexpr int FR_MAX_LDS = 60 * 1024;        // mebt_amd/frames.py:MAX_LDS_BYTES

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(FR_THREADS) void frames_resize_kernel(const uint8_t* __restrict__ frames, float* __restrict__ out, int T,
                                                                   int Hs, int Ws, int y0, int x0, int R, const int32_t* __restrict__ tab,
                                                                   int K, int rows, int span, const float* __restrict__ lut,
                                                                   const int32_t* __restrict__ slots, int Bout) {
    extern __shared__ uint8_t tmp[];          // [span][R][3] uint8: the horizontally resampled source rows
    __shared__ float lut_s[256];
    const int n = blockIdx.y, bl = n / T, t = n - bl * T;
    const int b = slots ? slots[bl] : bl;
    if (b < 0 || b >= Bout) return;           // uniform over the block
    lut_s[threadIdx.x] = lut[threadIdx.x];
    const int32_t* xmin = tab;
    const int32_t* cnt = tab + R;
    const int32_t* kk = tab + 2 * R;
    const int r0 = blockIdx.x * rows;
    const int r1 = min(r0 + rows, R) - 1;
    const int ybase = xmin[r0];
    const int nrow = min(xmin[r1] + cnt[r1] - ybase, span);
    const uint8_t* src = frames + (size_t)n * Hs * Ws * 3;
    const int R3 = R * 3;

    // horizontal pass: source rows [ybase, ybase + nrow) of the crop -> tmp
    for (int i = threadIdx.x; i < nrow * R; i += FR_THREADS) {
        const int row = i / R, x = i - row * R;
        const uint8_t* p = src + ((size_t)(y0 + ybase + row) * Ws + x0 + xmin[x]) * 3;
        const int32_t* w = kk + (size_t)x * K;
        const int m = cnt[x];
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int k = 0; k < m; ++k) {
            const int wk = w[k];
            a0 += wk * (int)p[3 * k];
            a1 += wk * (int)p[3 * k + 1];
            a2 += wk * (int)p[3 * k + 2];
        }
        uint8_t* d = tmp + row * R3 + x * 3;
        d[0] = (uint8_t)clip8(a0);
        d[1] = (uint8_t)clip8(a1);
        d[2] = (uint8_t)clip8(a2);
    }
    __syncthreads();

    // vertical pass: output rows [r0, r1] from tmp, then the normalisation table; lanes along W -> coalesced plane stores
    const size_t plane = (size_t)R * R;
    float* o = out + ((size_t)b * 3 * T + t) * plane;            // channel c at o + c * T * plane
    const int nout = (r1 - r0 + 1) * R;
    for (int i = threadIdx.x; i < nout; i += FR_THREADS) {
        const int rr = i / R, x = i - rr * R, r = r0 + rr;
        const int ym = xmin[r] - ybase;
        const int m = min(cnt[r], nrow - ym);
        const int32_t* w = kk + (size_t)r * K;
        const uint8_t* s = tmp + ym * R3 + x * 3;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int k = 0; k < m; ++k) {
            const int wk = w[k];
            a0 += wk * (int)s[k * R3];
            a1 += wk * (int)s[k * R3 + 1];
            a2 += wk * (int)s[k * R3 + 2];
        }
        const size_t off = (size_t)r * R + x;
        o[off] = lut_s[clip8(a0)];
        o[(size_t)T * plane + off] = lut_s[clip8(a1)];
        o[2 * (size_t)T * plane + off] = lut_s[clip8(a2)];
    }
}

// crop side == R: no resampling (PIL's same-size resize is a copy)
__global__ __launch_bounds__(FR_THREADS) void frames_copy_kernel(const uint8_t* __restrict__ frames, float* __restrict__ out, int T, int Hs,
                                                                 int Ws, int y0, int x0, int R, const float* __restrict__ lut,
                                                                 const int32_t* __restrict__ slots, int Bout) {
    __shared__ float lut_s[256];
    const int n = blockIdx.y, bl = n / T, t = n - bl * T;
    const int b = slots ? slots[bl] : bl;
    if (b < 0 || b >= Bout) return;
    lut_s[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const size_t plane = (size_t)R * R;
    const uint8_t* src = frames + (size_t)n * Hs * Ws * 3;
    float* o = out + ((size_t)b * 3 * T + t) * plane;
    for (int i = blockIdx.x * FR_THREADS + threadIdx.x; i < R * R; i += gridDim.x * FR_THREADS) {
        const int y = i / R, x = i - y * R;
        const uint8_t* p = src + ((size_t)(y0 + y) * Ws + x0 + x) * 3;
        o[i] = lut_s[p[0]];
        o[(size_t)T * plane + i] = lut_s[p[1]];
        o[2 * (size_t)T * plane + i] = lut_s[p[2]];
    }
}

hipStream_t S(mebt_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

}  // namespace

extern "C" int mebt_op_frames_to_video(const uint8_t* frames, float* out, int32_t N, int32_t T, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0,
                                       int32_t S_, int32_t R, const int32_t* tab, int32_t K, int32_t rows, int32_t span, const float* lut,
                                       const int32_t* slots, int32_t Bout, mebt_stream_t stream) {
    if (!frames || !out || !lut) { mebt_set_error("frames_to_video: null pointer"); return MEBT_EINVAL; }
    if (N < 1 || T < 1 || N % T || Hs < 1 || Ws < 1 || R < 1 || Bout < 1) { mebt_set_error("frames_to_video: bad shape"); return MEBT_EINVAL; }
    if (S_ < 1 || y0 < 0 || x0 < 0 || y0 + S_ > Hs || x0 + S_ > Ws) { mebt_set_error("frames_to_video: crop box outside the frame"); return MEBT_EINVAL; }
    if (!slots && N / T > Bout) { mebt_set_error("frames_to_video: more clips than output slots"); return MEBT_EINVAL; }
    if ((long)Hs * Ws * 3 > (1l << 40) || (long)R * R > (1l << 30)) { mebt_set_error("frames_to_video: frame too large"); return MEBT_EINVAL; }
    if (N > 65535) { mebt_set_error("frames_to_video: at most 65535 frames per launch"); return MEBT_EINVAL; }
    if (S_ == R) {
        const int g = (int)((R * R + FR_THREADS - 1) / FR_THREADS);
        hipLaunchKernelGGL(frames_copy_kernel, dim3(g < 64 ? g : 64, N), dim3(FR_THREADS), 0, S(stream), frames, out, T, Hs, Ws, y0, x0, R, lut,
                           slots, Bout);
    } else {
        if (!tab || K < 1 || rows < 1 || span < 1 || span > S_) { mebt_set_error("frames_to_video: bad coefficient table"); return MEBT_EINVAL; }
        const long lds = (long)span * R * 3;
        if (lds > FR_MAX_LDS) { mebt_set_error("frames_to_video: the source rows of one tile exceed the LDS"); return MEBT_EINVAL; }
        hipLaunchKernelGGL(frames_resize_kernel, dim3((R + rows - 1) / rows, N), dim3(FR_THREADS), (size_t)lds, S(stream), frames, out, T, Hs, Ws,
                           y0, x0, R, tab, K, rows, span, lut, slots, Bout);
    }
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}
