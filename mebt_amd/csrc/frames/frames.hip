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
//
// Both kernels are templates on the output element.  float: the clip above.  uint8_t (`mebt_op_frames_to_clip_u8`, the real side of
// FVD): the resampled byte goes through a 256-entry uint8 table instead (the reference's `((video + 0.5) * 255).byte()`, built on the
// host: mebt_amd/frames.py:byte_table) and is stored as the I3D path's clip [B, T, R, R, 3].  There a frame is R rows of R * 3 bytes
// and a channel is just a column, so the vertical pass writes the tile's contiguous run of output bytes a dword per lane (byte_run.h).
#include "../host_util.h"
#include "byte_run.h"

namespace {

constexpr int FR_THREADS = 256;
constexpr int FR_MAX_LDS = 60 * 1024;        // mebt_amd/frames.py:MAX_LDS_BYTES

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// one pass of Pillow's resampler for N adjacent bytes: a[c] = clip8(1 << 21 + sum over the m taps of w[k] * s[k * stride + c])
template <int N>
__device__ __forceinline__ void taps(const int32_t* w, int m, const uint8_t* s, int stride, int (&a)[N]) {
    for (int c = 0; c < N; ++c) a[c] = 1 << 21;
    for (int k = 0; k < m; ++k)
        for (int c = 0; c < N; ++c) a[c] += w[k] * (int)s[k * stride + c];
    for (int c = 0; c < N; ++c) a[c] = clip8(a[c]);
}

// the launch's 256-entry table staged in LDS, one entry per lane (FR_THREADS of them); the caller's barrier publishes it
template <typename Out>
__device__ __forceinline__ const Out* stage_table(const Out* __restrict__ lut) {
    __shared__ Out lut_s[256];
    lut_s[threadIdx.x] = lut[threadIdx.x];
    return lut_s;
}

// pixel i of one frame of the float clip [B, 3, T, R, R]: channel c is the plane at o + c * cstride (cstride = T * R * R)
template <typename Out>
__device__ __forceinline__ void store_planes(Out* o, size_t cstride, size_t i, Out c0, Out c1, Out c2) {
    o[i] = c0;
    o[cstride + i] = c1;
    o[2 * cstride + i] = c2;
}

template <typename Out>
__global__ __launch_bounds__(FR_THREADS) void frames_resize_kernel(const uint8_t* __restrict__ frames, Out* __restrict__ out, int T,
                                                                   int Hs, int Ws, int y0, int x0, int R, const int32_t* __restrict__ tab,
                                                                   int K, int rows, int span, const Out* __restrict__ lut,
                                                                   const int32_t* __restrict__ slots, int Bout) {
    extern __shared__ uint8_t tmp[];          // [span][R][3] uint8: the horizontally resampled source rows
    const int n = blockIdx.y, bl = n / T, t = n - bl * T;
    const int b = slots ? slots[bl] : bl;
    if (b < 0 || b >= Bout) return;           // uniform over the block
    const Out* lut_s = stage_table(lut);
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
        int a[3];
        taps(kk + (size_t)x * K, cnt[x], src + ((size_t)(y0 + ybase + row) * Ws + x0 + xmin[x]) * 3, 3, a);
        uint8_t* d = tmp + row * R3 + x * 3;
        d[0] = (uint8_t)a[0];
        d[1] = (uint8_t)a[1];
        d[2] = (uint8_t)a[2];
    }
    __syncthreads();

    // vertical pass: the bytes a[0, N) of output row r from byte `col` of its R3, one walk over the row's taps in tmp
    auto vpass = [&](int r, int col, auto& a) {
        const int ym = xmin[r] - ybase;
        taps(kk + (size_t)r * K, min(cnt[r], nrow - ym), tmp + ym * R3 + col, R3, a);
    };
    const size_t plane = (size_t)R * R;
    if constexpr (sizeof(Out) == 1) {
        // the tile's run of (r1 - r0 + 1) * R3 output bytes through the byte table
        uint8_t* run = out + (((size_t)b * T + t) * R + r0) * R3;
        const int nrun = (r1 - r0 + 1) * R3;
        auto byte = [&](int jj) {
            int a[1];
            vpass(r0 + jj / R3, jj % R3, a);
            return lut_s[a[0]];
        };
        // four columns of one output row in one walk; a dword across a row boundary goes byte by byte
        auto quad = [&](int j, uint32_t& v) {
            const int rr = j / R3, col = j - rr * R3;
            if (col + 4 > R3) return false;
            int a[4];
            vpass(r0 + rr, col, a);
            v = (uint32_t)lut_s[a[0]] | (uint32_t)lut_s[a[1]] << 8 | (uint32_t)lut_s[a[2]] << 16 | (uint32_t)lut_s[a[3]] << 24;
            return true;
        };
        write_run(run, nrun, 0, nrun, 4 * (int)threadIdx.x - run_mis(run), 4 * FR_THREADS, quad, byte);
        return;
    }
    // output rows [r0, r1] through the normalisation table; lanes along W -> coalesced plane stores
    Out* o = out + ((size_t)b * 3 * T + t) * plane;              // channel c at o + c * T * plane
    const int nout = (r1 - r0 + 1) * R;
    for (int i = threadIdx.x; i < nout; i += FR_THREADS) {
        const int rr = i / R, x = i - rr * R, r = r0 + rr;
        int a[3];
        vpass(r, x * 3, a);
        store_planes(o, (size_t)T * plane, (size_t)r * R + x, lut_s[a[0]], lut_s[a[1]], lut_s[a[2]]);
    }
}

// crop side == R: no resampling (PIL's same-size resize is a copy)
template <typename Out>
__global__ __launch_bounds__(FR_THREADS) void frames_copy_kernel(const uint8_t* __restrict__ frames, Out* __restrict__ out, int T, int Hs,
                                                                 int Ws, int y0, int x0, int R, const Out* __restrict__ lut,
                                                                 const int32_t* __restrict__ slots, int Bout) {
    const int n = blockIdx.y, bl = n / T, t = n - bl * T;
    const int b = slots ? slots[bl] : bl;
    if (b < 0 || b >= Bout) return;
    const Out* lut_s = stage_table(lut);
    __syncthreads();
    const size_t plane = (size_t)R * R;
    const uint8_t* src = frames + (size_t)n * Hs * Ws * 3;
    if constexpr (sizeof(Out) == 1) {
        // the frame is one run of R rows of R3 bytes; source row y is the R3 bytes at src + ((y0 + y) * Ws + x0) * 3
        const int R3 = R * 3, nrun = R * R3;
        uint8_t* run = out + ((size_t)b * T + t) * nrun;
        auto byte = [&](int jj) {
            const int y = jj / R3, col = jj - y * R3;
            return lut_s[src[((size_t)(y0 + y) * Ws + x0) * 3 + col]];
        };
        // the source bytes of a dword share no alignment with it: every dword is put together from its bytes
        write_run(run, nrun, 0, nrun, 4 * (int)(blockIdx.x * FR_THREADS + threadIdx.x) - run_mis(run), 4 * (int)gridDim.x * FR_THREADS,
                  [](int, uint32_t&) { return false; }, byte);
        return;
    }
    Out* o = out + ((size_t)b * 3 * T + t) * plane;
    for (int i = blockIdx.x * FR_THREADS + threadIdx.x; i < R * R; i += gridDim.x * FR_THREADS) {
        const int y = i / R, x = i - y * R;
        const uint8_t* p = src + ((size_t)(y0 + y) * Ws + x0 + x) * 3;
        store_planes(o, (size_t)T * plane, (size_t)i, lut_s[p[0]], lut_s[p[1]], lut_s[p[2]]);
    }
}

// ---- packed frame datasets (mebt_amd/packed.py): gather rows of a pack [F, R, R, 3] uint8 by id --------------------------------------
// The pack holds every frame after crop + resize, so a training clip is T rows of it and the only work left is the table lookup and the
// layout: the same outputs as the copy kernel above, with the source frame chosen by ids[n] instead of n.  One workgroup per (frame,
// chunk of PK_CHUNK bytes of it): the chunk is staged in LDS with 16-byte loads over its 16-byte-aligned body (single bytes for the at
// most 15 bytes before and after it; the LDS copy keeps the global address' offset mod 16, so any pack pointer and any R work), then
// read back a pixel (float: three planes, lanes along W) or a dword of the output run (uint8) per lane.  Every offset into the pack
// is 64-bit; an id outside [0, F) writes nothing.
template <typename Out>
__global__ __launch_bounds__(FR_THREADS) void pack_gather_kernel(const uint8_t* __restrict__ pack, int64_t F, const int64_t* __restrict__ ids,
                                                                 Out* __restrict__ out, int T, int R, int nchunk, const Out* __restrict__ lut) {
    __shared__ __attribute__((aligned(16))) uint8_t buf[PK_CHUNK + 16];
    const int64_t n = blockIdx.x / nchunk;
    const int k = (int)(blockIdx.x - n * nchunk);
    const int64_t id = ids[n];
    if (id < 0 || id >= F) return;            // uniform over the block
    const int tid = threadIdx.x;
    const int nrun = R * R * 3;
    const uint8_t* src = pack + (size_t)id * (size_t)nrun;
    uint8_t* run = sizeof(Out) == 1 ? reinterpret_cast<uint8_t*>(out) + (size_t)n * (size_t)nrun : nullptr;
    // this block's bytes of the frame: [c0, c1); the uint8 chunks are counted in dwords of the output run, which starts run_mis early
    const RunChunk ch = run_chunk(k, run ? run_mis(run) : 0, nrun);
    const int c0 = ch.c0, c1 = ch.c1;
    if (c0 >= c1) return;
    const Out* lut_s = stage_table(lut);
    const uint8_t* a = src + c0;
    const int len = c1 - c0;
    const int sh = (int)(reinterpret_cast<uintptr_t>(a) & 15);           // buf[sh + j] = a[j]: a + j and buf + sh + j agree mod 16
    const int head = min((16 - sh) & 15, len);
    const int nvec = (len - head) >> 4;
    const int tail = head + nvec * 16;
    for (int i = tid; i < nvec; i += FR_THREADS)
        *reinterpret_cast<uint4*>(buf + sh + head + 16 * i) = *reinterpret_cast<const uint4*>(a + head + 16 * i);
    if (tid < head) buf[sh + tid] = a[tid];
    if (tid < len - tail) buf[sh + tail + tid] = a[tail + tid];
    __syncthreads();
    const int s0 = sh - c0;                   // buf[s0 + j] = byte j of the frame, c0 <= j < c1

    if constexpr (sizeof(Out) == 1) {
        write_run(run, nrun, c0, c1, ch.j0 + 4 * tid, 4 * FR_THREADS, [&](int j) { return lut_s[buf[s0 + j]]; });
        return;
    }
    const size_t plane = (size_t)R * R;
    const int64_t b = n / T;
    const int t = (int)(n - b * T);
    Out* o = out + ((size_t)b * 3 * T + t) * plane;                      // channel c at o + c * T * plane
    for (int p = c0 / 3 + tid; p < c1 / 3; p += FR_THREADS) {
        const uint8_t* s = buf + s0 + 3 * p;
        store_planes(o, (size_t)T * plane, (size_t)p, lut_s[s[0]], lut_s[s[1]], lut_s[s[2]]);
    }
}

// ---- decoded video -> uint8 clip (mebt_amd/frames.py:video_to_clip_u8): what the sampling scripts keep of a decode ---------------------
// in fp32 [B, 3, Td, H, W] (VQGAN.decode) -> out uint8 [B, T, H, W, 3], the first T frames, u = (uint8) trunc((clamp(x, -0.5, 0.5) + 0.5)
// * 255): the scripts' `torch.clamp(img, -0.5, 0.5) + 0.5`, then numpy's float32 `* 255` and `.astype(np.uint8)`.  Two separately rounded
// float32 operations (__fadd_rn, __fmul_rn: never contracted into x * 255 + 127.5, which rounds differently); NaN writes 0.  One
// workgroup per (frame, chunk of PK_CHUNK bytes of its run of H * W * 3 output bytes): the pixels the chunk touches are read from the
// three planes, lanes along W, converted and interleaved in LDS, then read back a dword of the run per lane as in the gather above.
__device__ __forceinline__ uint8_t video_byte(float x) {
    const float c = fminf(fmaxf(x, -0.5f), 0.5f);           // fmaxf drops a NaN operand: NaN -> -0.5 -> 0
    return (uint8_t)(int)__fmul_rn(__fadd_rn(c, 0.5f), 255.0f);
}

__global__ __launch_bounds__(FR_THREADS) void video_to_clip_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, int Td, int T,
                                                                   int HW, int nchunk) {
    __shared__ __attribute__((aligned(16))) uint8_t buf[PK_CHUNK + 16];
    const int64_t n = blockIdx.x / nchunk;                   // output frame b * T + t
    const int k = (int)(blockIdx.x - n * nchunk);
    const int64_t b = n / T;
    const int t = (int)(n - b * T);
    const int tid = threadIdx.x;
    const int nrun = HW * 3;
    uint8_t* run = out + (size_t)n * (size_t)nrun;
    // this block's bytes of the frame: [c0, c1), counted in dwords of the output run, which starts run_mis(run) early
    const RunChunk ch = run_chunk(k, run_mis(run), nrun);
    const int c0 = ch.c0, c1 = ch.c1;
    if (c0 >= c1) return;                                    // uniform over the block
    const int p0 = c0 / 3, p1 = (c1 + 2) / 3;                // the pixels those bytes belong to: at most PK_CHUNK / 3 + 2
    const size_t plane = (size_t)Td * (size_t)HW;            // channel c of frame t at in + ((b * 3 + c) * Td + t) * HW
    const float* src = in + ((size_t)b * 3 * Td + t) * (size_t)HW;
    for (int p = p0 + tid; p < p1; p += FR_THREADS) {
        uint8_t* d = buf + 3 * (p - p0);
        d[0] = video_byte(src[p]);
        d[1] = video_byte(src[plane + p]);
        d[2] = video_byte(src[2 * plane + p]);
    }
    __syncthreads();
    const int s0 = -3 * p0;                                  // buf[s0 + j] = byte j of the frame, c0 <= j < c1
    write_run(run, nrun, c0, c1, ch.j0 + 4 * tid, 4 * FR_THREADS, [&](int j) { return buf[s0 + j]; });
}

int fail(const char* who, const char* what) { return fail(MEBT_EINVAL, who, what); }     // every refusal of this file is MEBT_EINVAL

// grid of the two chunked kernels over `nframes` runs of nrun bytes: one block per (run, chunk); `out` as in run_chunks
int chunk_grid(const char* who, long nrun, const void* out, long nframes, int* nchunk, unsigned* blocks) {
    if (nrun > (1l << 30)) return fail(who, "frame too large");                            // a run's bytes are indexed in int
    const long n = run_chunks(nrun, out);
    if (nframes * n > (1l << 24)) return fail(who, "too many frames for one launch");      // grid.x * 256 threads stays below 2^32
    *nchunk = (int)n;
    *blocks = (unsigned)(nframes * n);
    return MEBT_OK;
}

// argument checks and launch of both entries
template <typename Out>
int frames_launch(const char* who, const uint8_t* frames, Out* out, int32_t N, int32_t T, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0,
                  int32_t S_, int32_t R, const int32_t* tab, int32_t K, int32_t rows, int32_t span, const Out* lut, const int32_t* slots,
                  int32_t Bout, mebt_stream_t stream) {
    if (!frames || !out || !lut) return fail(who, "null pointer");
    if (N < 1 || T < 1 || N % T || Hs < 1 || Ws < 1 || R < 1 || Bout < 1) return fail(who, "bad shape");
    if (S_ < 1 || y0 < 0 || x0 < 0 || y0 + S_ > Hs || x0 + S_ > Ws) return fail(who, "crop box outside the frame");
    if (!slots && N / T > Bout) return fail(who, "more clips than output slots");
    // uint8 output: the frame's R * R * 3 bytes are indexed in int
    if ((long)Hs * Ws * 3 > (1l << 40) || (long)R * R * (sizeof(Out) == 1 ? 3 : 1) > (1l << 30)) return fail(who, "frame too large");
    if (N > 65535) return fail(who, "at most 65535 frames per launch");
    if (S_ == R) {
        const long work = sizeof(Out) == 1 ? ((long)R * R * 3 + 3) / 4 + 1 : (long)R * R;      // lanes per frame: dwords of the run, or pixels
        const int g = (int)((work + FR_THREADS - 1) / FR_THREADS);
        hipLaunchKernelGGL(frames_copy_kernel<Out>, dim3(g < 64 ? g : 64, N), dim3(FR_THREADS), 0, S(stream), frames, out, T, Hs, Ws, y0, x0, R,
                           lut, slots, Bout);
    } else {
        if (!tab || K < 1 || rows < 1 || span < 1 || span > S_) return fail(who, "bad coefficient table");
        const long lds = (long)span * R * 3;
        if (lds > FR_MAX_LDS) return fail(who, "the source rows of one tile exceed the LDS");
        hipLaunchKernelGGL(frames_resize_kernel<Out>, dim3((R + rows - 1) / rows, N), dim3(FR_THREADS), (size_t)lds, S(stream), frames, out, T,
                           Hs, Ws, y0, x0, R, tab, K, rows, span, lut, slots, Bout);
    }
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

template <typename Out>
int pack_launch(const char* who, const uint8_t* pack, int64_t F, const int64_t* ids, Out* out, int32_t B, int32_t T, int32_t R, const Out* lut,
                mebt_stream_t stream) {
    if (!pack || !ids || !out || !lut) return fail(who, "null pointer");
    if (F < 1 || B < 1 || T < 1 || R < 1) return fail(who, "bad shape");
    int nchunk;
    unsigned blocks;
    if (int e = chunk_grid(who, (long)R * R * 3, sizeof(Out) == 1 ? out : nullptr, (long)B * T, &nchunk, &blocks)) return e;
    hipLaunchKernelGGL(pack_gather_kernel<Out>, dim3(blocks), dim3(FR_THREADS), 0, S(stream), pack, F, ids, out, T, R, nchunk, lut);
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

}  // namespace

extern "C" int mebt_op_frames_to_video(const uint8_t* frames, float* out, int32_t N, int32_t T, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0,
                                       int32_t S_, int32_t R, const int32_t* tab, int32_t K, int32_t rows, int32_t span, const float* lut,
                                       const int32_t* slots, int32_t Bout, mebt_stream_t stream) {
    return frames_launch<float>("frames_to_video", frames, out, N, T, Hs, Ws, y0, x0, S_, R, tab, K, rows, span, lut, slots, Bout, stream);
}

extern "C" int mebt_op_frames_to_clip_u8(const uint8_t* frames, uint8_t* out, int32_t N, int32_t T, int32_t Hs, int32_t Ws, int32_t y0,
                                         int32_t x0, int32_t S_, int32_t R, const int32_t* tab, int32_t K, int32_t rows, int32_t span,
                                         const uint8_t* lut, const int32_t* slots, int32_t Bout, mebt_stream_t stream) {
    return frames_launch<uint8_t>("frames_to_clip_u8", frames, out, N, T, Hs, Ws, y0, x0, S_, R, tab, K, rows, span, lut, slots, Bout, stream);
}

extern "C" int mebt_op_pack_to_video(const uint8_t* pack, int64_t F, const int64_t* ids, float* out, int32_t B, int32_t T, int32_t R,
                                     const float* lut, mebt_stream_t stream) {
    return pack_launch<float>("pack_to_video", pack, F, ids, out, B, T, R, lut, stream);
}

extern "C" int mebt_op_pack_to_clip_u8(const uint8_t* pack, int64_t F, const int64_t* ids, uint8_t* out, int32_t B, int32_t T, int32_t R,
                                       const uint8_t* lut, mebt_stream_t stream) {
    return pack_launch<uint8_t>("pack_to_clip_u8", pack, F, ids, out, B, T, R, lut, stream);
}

extern "C" int mebt_op_video_to_clip_u8(const float* in, uint8_t* out, int32_t B, int32_t Td, int32_t T, int32_t H, int32_t W,
                                        mebt_stream_t stream) {
    const char* who = "video_to_clip_u8";
    if (!in || !out) return fail(who, "null pointer");
    if (B < 1 || Td < 1 || T < 1 || T > Td || H < 1 || W < 1) return fail(who, "bad shape");
    int nchunk;
    unsigned blocks;
    if (int e = chunk_grid(who, (long)H * W * 3, out, (long)B * T, &nchunk, &blocks)) return e;
    hipLaunchKernelGGL(video_to_clip_kernel, dim3(blocks), dim3(FR_THREADS), 0, S(stream), in, out, Td, T, H * W, nchunk);
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}
