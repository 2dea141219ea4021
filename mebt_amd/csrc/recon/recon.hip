// First-stage validation metrics (include/mebt_hip.h "reconstruction metrics"; mebt_amd/recon.py): the sums behind the reference's
// val/recon_loss, val/commitment_loss and val/perplexity (mebt/vqgan.py:190-196, modules/codebook.py:64,93-94) and the per-frame
// squared error and SSIM of a reconstruction.
//
// Reproducibility: a floating-point sum never meets an atomic.  Every workgroup reduces its share in a fixed order (lanes by xor
// butterfly, waves 0..3 in turn) and stores ONE fp64 partial at its own slot of the caller's scratch slab; a second kernel adds the
// slots of each output in index order.  The same input therefore gives the same bits on every run.  The only atomics are the 64-bit
// integer adds of the code histogram, which are exact in any order.  Every offset into an operand is 64-bit.
#include <cmath>

#include "../block_reduce.h"
#include "../host_util.h"

namespace {

struct SsimWindow { float g[11]; };                  // the normalised 11-tap Gaussian, rounded from fp64

constexpr int RC_THREADS = 256;
constexpr int RC_WAVES = RC_THREADS / MEBT_WAVE;

// out[o] = scale * (part[o * count + 0] + part[o * count + 1] + ...), the slots in slot_sum's order
__global__ __launch_bounds__(RC_THREADS) void sum_partials_kernel(const double* __restrict__ part, int64_t count, double* __restrict__ out,
                                                                  double scale) {
    __shared__ double sh[RC_WAVES];
    const double s = slot_sum<RC_THREADS>(part + (size_t)blockIdx.x * (size_t)count, count, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = s * scale;
}

// ---- sum |x - y| per clip ------------------------------------------------------------------------------------------------------
// workgroup (b, k) takes elements [k * CHUNK, (k + 1) * CHUNK) of clip b: 64 terms per lane in fp32 (the bound the tolerance of the
// tests rests on), then fp64.  VEC: n % 4 == 0 and 16-byte aligned operands, so every clip and every chunk starts on a float4.
constexpr int64_t ABS_CHUNK = MEBT_RECON_ABS_CHUNK;
static_assert(ABS_CHUNK == 64 * RC_THREADS, "a lane adds at most 64 fp32 terms");

template <bool VEC>
__global__ __launch_bounds__(RC_THREADS) void abs_diff_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                              double* __restrict__ part, int64_t n, int64_t blocks) {
    __shared__ double sh[RC_WAVES];
    const int64_t b = blockIdx.x / blocks;
    const int64_t k = blockIdx.x - b * blocks;
    const int64_t c0 = k * ABS_CHUNK;
    const int64_t c1 = c0 + ABS_CHUNK < n ? c0 + ABS_CHUNK : n;
    const float* xb = x + (size_t)b * (size_t)n;
    const float* yb = y + (size_t)b * (size_t)n;
    float acc = 0.f;
    if (VEC) {
        for (int64_t i = c0 + 4 * (int64_t)threadIdx.x; i < c1; i += 4 * RC_THREADS) {
            const f32x4 u = *reinterpret_cast<const f32x4*>(xb + i), v = *reinterpret_cast<const f32x4*>(yb + i);
            acc += fabsf(u[0] - v[0]);
            acc += fabsf(u[1] - v[1]);
            acc += fabsf(u[2] - v[2]);
            acc += fabsf(u[3] - v[3]);
        }
    } else {
        for (int64_t i = c0 + threadIdx.x; i < c1; i += RC_THREADS) acc += fabsf(xb[i] - yb[i]);
    }
    const double s = block_sum<RC_WAVES>((double)acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ---- squared error and SSIM per frame ----------------------------------------------------------------------------------------
// One workgroup per (frame, tile of TH x TW window positions).  The tile's (TH + 10) x (TW + 10) pixels of both images go to LDS as
// bytes, one plane per channel (pixels past the frame: 128, the centre, which no valid position reads).  Per channel: the horizontal
// pass writes the five windowed row sums (u, v, u u, v v, u v of the centred bytes) of every tile row, the vertical pass finishes the
// window, forms the SSIM map in fp32 and adds it to the lane's fp64 sum.  Squared error: every pixel is counted by the one tile that
// owns it (rows [y0, y0 + TH) and columns [x0, x0 + TW); the last tile of a row / column of tiles also owns its halo).
constexpr int TH = MEBT_RECON_TILE_H, TW = MEBT_RECON_TILE_W, WIN = 11, HALO = WIN - 1;
constexpr int IH = TH + HALO, IW = TW + HALO, IWP = IW + 2;     // plane row padded to a multiple of 4 bytes
static_assert(TW == 32 && (TH * TW) % RC_THREADS == 0, "lane -> position mapping of the two passes");

__global__ __launch_bounds__(RC_THREADS) void clip_quality_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                  double* __restrict__ part_ssim, long long* __restrict__ part_sq, int H,
                                                                  int W, int tx_n, int tiles, SsimWindow win) {
    __shared__ uint8_t sa[3][IH][IWP], sb[3][IH][IWP];
    __shared__ float tmp[5][IH][TW];
    __shared__ double sh_d[RC_WAVES];
    __shared__ long long sh_q[RC_WAVES];
    const int tid = threadIdx.x;
    const int64_t n = blockIdx.x / tiles;
    const int t = (int)(blockIdx.x - n * tiles);
    const int ty = t / tx_n, tx = t - ty * tx_n;
    const int y0 = ty * TH, x0 = tx * TW;
    const bool last_y = ty == tiles / tx_n - 1, last_x = tx == tx_n - 1;
    const size_t frame = (size_t)n * (size_t)H * (size_t)W * 3;
    const uint8_t* fa = a + frame;
    const uint8_t* fb = b + frame;

    int sq = 0;                                                  // at most 13 bytes per lane: 13 * 255^2 fits
    for (int i = tid; i < IH * IW * 3; i += RC_THREADS) {
        const int r = i / (IW * 3);
        const int j = i - r * (IW * 3);
        const int px = j / 3, c = j - 3 * px;
        const int y = y0 + r, xx = x0 + px;
        uint8_t va = 128, vb = 128;
        if (y < H && xx < W) {
            const size_t off = ((size_t)y * (size_t)W + (size_t)xx) * 3 + c;
            va = fa[off];
            vb = fb[off];
            if ((r < TH || last_y) && (px < TW || last_x)) {
                const int d = (int)va - (int)vb;
                sq += d * d;
            }
        }
        sa[c][r][px] = va;
        sb[c][r][px] = vb;
    }
    __syncthreads();

    const int vh = H - HALO - y0 < TH ? H - HALO - y0 : TH;       // window positions of this tile inside the frame
    const int vw = W - HALO - x0 < TW ? W - HALO - x0 : TW;
    const float C1 = 6.5025f, C2 = 58.5225f;                     // (0.01 * 255)^2, (0.03 * 255)^2
    double acc = 0.0;
    for (int c = 0; c < 3; ++c) {
        for (int i = tid; i < IH * TW; i += RC_THREADS) {
            const int r = i >> 5, cx = i & 31;
            float mu = 0.f, mv = 0.f, uu = 0.f, vv = 0.f, uv = 0.f;
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const float u = (float)((int)sa[c][r][cx + k] - 128), v = (float)((int)sb[c][r][cx + k] - 128);
                const float wu = win.g[k] * u, wv = win.g[k] * v;
                mu += wu;
                mv += wv;
                uu += wu * u;
                vv += wv * v;
                uv += wu * v;
            }
            tmp[0][r][cx] = mu;
            tmp[1][r][cx] = mv;
            tmp[2][r][cx] = uu;
            tmp[3][r][cx] = vv;
            tmp[4][r][cx] = uv;
        }
        __syncthreads();
        for (int i = tid; i < TH * TW; i += RC_THREADS) {
            const int r = i >> 5, cx = i & 31;
            if (r < vh && cx < vw) {
                float mu = 0.f, mv = 0.f, uu = 0.f, vv = 0.f, uv = 0.f;
#pragma unroll
                for (int k = 0; k < WIN; ++k) {
                    const float w = win.g[k];
                    mu += w * tmp[0][r + k][cx];
                    mv += w * tmp[1][r + k][cx];
                    uu += w * tmp[2][r + k][cx];
                    vv += w * tmp[3][r + k][cx];
                    uv += w * tmp[4][r + k][cx];
                }
                const float var_a = uu - mu * mu, var_b = vv - mv * mv, cov = uv - mu * mv;      // shift invariant
                const float ma = mu + 128.f, mb = mv + 128.f;
                const float num = (2.f * ma * mb + C1) * (2.f * cov + C2);
                const float den = (ma * ma + mb * mb + C1) * (var_a + var_b + C2);
                acc += (double)(num / den);
            }
        }
        __syncthreads();
    }
    const double s = block_sum<RC_WAVES>(acc, sh_d);
    const long long q = block_sum<RC_WAVES>((long long)sq, sh_q);
    if (tid == 0) {
        part_ssim[blockIdx.x] = s;
        part_sq[blockIdx.x] = q;
    }
}

__global__ __launch_bounds__(RC_THREADS) void clip_quality_finish_kernel(const double* __restrict__ part_ssim,
                                                                         const long long* __restrict__ part_sq, int tiles,
                                                                         double* __restrict__ ssim, int64_t* __restrict__ sq_err,
                                                                         double inv_count) {
    __shared__ double sh_d[RC_WAVES];
    __shared__ long long sh_q[RC_WAVES];
    const size_t base = (size_t)blockIdx.x * (size_t)tiles;
    double acc = 0.0;
    long long q = 0;
    for (int j = threadIdx.x; j < tiles; j += RC_THREADS) {
        acc += part_ssim[base + j];
        q += part_sq[base + j];
    }
    const double s = block_sum<RC_WAVES>(acc, sh_d);
    q = block_sum<RC_WAVES>(q, sh_q);
    if (threadIdx.x == 0) {
        ssim[blockIdx.x] = s * inv_count;
        sq_err[blockIdx.x] = (int64_t)q;
    }
}

// ---- code histogram and sum |z - e|^2 -----------------------------------------------------------------------------------------
// One wave per row, CODE_ROWS rows per workgroup (wave w takes rows w, w + 4, ...).  A lane squares at most 4 differences in fp32
// before fp64 takes over.  An id outside [0, n_codes) is skipped before the embedding row is addressed (the pack kernels' rule).
constexpr int CODE_ROWS = MEBT_RECON_CODE_ROWS;

template <bool VEC>
__global__ __launch_bounds__(RC_THREADS) void code_stats_kernel(const int64_t* __restrict__ ids, const float* __restrict__ z,
                                                                const float* __restrict__ emb, unsigned long long* __restrict__ hist,
                                                                double* __restrict__ part, int64_t M, int n_codes, int d) {
    __shared__ double sh[RC_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int j = wave; j < CODE_ROWS; j += RC_WAVES) {
        const int64_t m = (int64_t)blockIdx.x * CODE_ROWS + j;
        if (m >= M) break;                                       // wave uniform
        const int64_t id = ids[m];
        if (id < 0 || id >= n_codes) continue;                   // wave uniform
        const float* zr = z + (size_t)m * (size_t)d;
        const float* er = emb + (size_t)id * (size_t)d;
        double rs = 0.0;
        if (VEC) {
            for (int i = 4 * lane; i < d; i += 4 * MEBT_WAVE) {
                const f32x4 u = *reinterpret_cast<const f32x4*>(zr + i), v = *reinterpret_cast<const f32x4*>(er + i);
                const float t0 = u[0] - v[0], t1 = u[1] - v[1], t2 = u[2] - v[2], t3 = u[3] - v[3];
                rs += (double)(t0 * t0 + t1 * t1 + t2 * t2 + t3 * t3);
            }
        } else {
            for (int i = lane; i < d; i += MEBT_WAVE) {
                const float t0 = zr[i] - er[i];
                rs += (double)(t0 * t0);
            }
        }
        acc += wave_sum(rs);
        if (lane == 0) atomicAdd(hist + id, 1ull);
    }
    const double s = waves_sum<RC_WAVES>(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ---- workgroup counts (the scratch formulas of the header) and launchers, which trust their arguments: the entry points check them ------
int64_t recon_abs_diff_blocks(int64_t n) { return (n + ABS_CHUNK - 1) / ABS_CHUNK; }
int64_t recon_quality_tiles(int H, int W) { return (int64_t)((H - HALO + TH - 1) / TH) * ((W - HALO + TW - 1) / TW); }
int64_t recon_code_blocks(int64_t M) { return (M + CODE_ROWS - 1) / CODE_ROWS; }

int launch_abs_diff_sum(const float* x, const float* y, double* out, int B, int64_t n, double* scratch, hipStream_t stream) {
    const int64_t blocks = recon_abs_diff_blocks(n);
    const dim3 grid((unsigned)(blocks * B));
    if (n % 4 == 0 && aligned16(x) && aligned16(y))
        hipLaunchKernelGGL(abs_diff_kernel<true>, grid, dim3(RC_THREADS), 0, stream, x, y, scratch, n, blocks);
    else
        hipLaunchKernelGGL(abs_diff_kernel<false>, grid, dim3(RC_THREADS), 0, stream, x, y, scratch, n, blocks);
    MEBT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sum_partials_kernel, dim3(B), dim3(RC_THREADS), 0, stream, scratch, blocks, out, 1.0);
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

int launch_clip_quality_u8(const uint8_t* a, const uint8_t* b, int64_t* sq_err, double* ssim, int N, int H, int W, const SsimWindow& win,
                           void* scratch, hipStream_t stream) {
    const int tx_n = (W - HALO + TW - 1) / TW;
    const int tiles = (int)recon_quality_tiles(H, W);
    double* part_ssim = reinterpret_cast<double*>(scratch);
    long long* part_sq = reinterpret_cast<long long*>(part_ssim + (size_t)N * tiles);
    hipLaunchKernelGGL(clip_quality_kernel, dim3((unsigned)((int64_t)N * tiles)), dim3(RC_THREADS), 0, stream, a, b, part_ssim, part_sq, H, W,
                       tx_n, tiles, win);
    MEBT_HIP_CHECK(hipGetLastError());
    const double inv_count = 1.0 / (3.0 * (double)(H - HALO) * (double)(W - HALO));
    hipLaunchKernelGGL(clip_quality_finish_kernel, dim3(N), dim3(RC_THREADS), 0, stream, part_ssim, part_sq, tiles, ssim, sq_err, inv_count);
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

int launch_code_stats(const int64_t* ids, const float* z, const float* emb, int64_t* hist, double* sq_sum, int64_t M, int n_codes, int d,
                      double* scratch, hipStream_t stream) {
    const int64_t blocks = recon_code_blocks(M);
    unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
    if (d % 4 == 0 && aligned16(z) && aligned16(emb))
        hipLaunchKernelGGL(code_stats_kernel<true>, dim3((unsigned)blocks), dim3(RC_THREADS), 0, stream, ids, z, emb, h, scratch, M, n_codes, d);
    else
        hipLaunchKernelGGL(code_stats_kernel<false>, dim3((unsigned)blocks), dim3(RC_THREADS), 0, stream, ids, z, emb, h, scratch, M, n_codes, d);
    MEBT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(RC_THREADS), 0, stream, scratch, blocks, sq_sum, 1.0);
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

}  // namespace

extern "C" int mebt_op_abs_diff_sum(const float* x, const float* y, double* out, int32_t B, int64_t n, void* scratch, int64_t scratch_bytes,
                                    mebt_stream_t stream) {
    const char* who = "abs_diff_sum";
    if (!x || !y || !out) return fail(MEBT_EINVAL, who, "null pointer");
    if (B < 1 || n < 1 || n > (1ll << 40)) return fail(MEBT_ESHAPE, who, "need B >= 1 and 1 <= n <= 2^40");
    const int64_t blocks = recon_abs_diff_blocks(n) * B;
    if (int rc = check_scratch(who, scratch, scratch_bytes, 8 * blocks, blocks)) return rc;
    return launch_abs_diff_sum(x, y, out, B, n, reinterpret_cast<double*>(scratch), S(stream));
}

extern "C" int mebt_op_clip_quality_u8(const uint8_t* a, const uint8_t* b, int64_t* sq_err, double* ssim, int32_t N, int32_t H, int32_t W,
                                       void* scratch, int64_t scratch_bytes, mebt_stream_t stream) {
    const char* who = "clip_quality_u8";
    if (!a || !b || !sq_err || !ssim) return fail(MEBT_EINVAL, who, "null pointer");
    if (N < 1) return fail(MEBT_ESHAPE, who, "need N >= 1");
    if (H < WIN || W < WIN) return fail(MEBT_ESHAPE, who, "the 11 x 11 SSIM window needs H >= 11 and W >= 11");
    if (H > (1 << 20) || W > (1 << 20)) return fail(MEBT_ESHAPE, who, "frame too large");
    const int64_t blocks = recon_quality_tiles(H, W) * N;
    if (int rc = check_scratch(who, scratch, scratch_bytes, 16 * blocks, blocks)) return rc;
    SsimWindow win;
    double g[WIN], tot = 0.0;
    for (int i = 0; i < WIN; ++i) tot += g[i] = exp(-(double)((i - WIN / 2) * (i - WIN / 2)) / 4.5);          // sigma 1.5
    for (int i = 0; i < WIN; ++i) win.g[i] = (float)(g[i] / tot);
    return launch_clip_quality_u8(a, b, sq_err, ssim, N, H, W, win, scratch, S(stream));
}

extern "C" int mebt_op_code_stats(const int64_t* ids, const float* z, const float* embeddings, int64_t* hist, double* sq_sum, int64_t M,
                                  int32_t n_codes, int32_t d, void* scratch, int64_t scratch_bytes, mebt_stream_t stream) {
    const char* who = "code_stats";
    if (!ids || !z || !embeddings || !hist || !sq_sum) return fail(MEBT_EINVAL, who, "null pointer");
    if (M < 1 || n_codes < 1 || d < 1) return fail(MEBT_ESHAPE, who, "need M, n_codes, d >= 1");
    const int64_t blocks = recon_code_blocks(M);
    if (int rc = check_scratch(who, scratch, scratch_bytes, 8 * blocks, blocks)) return rc;
    return launch_code_stats(ids, z, embeddings, hist, sq_sum, M, n_codes, d, reinterpret_cast<double*>(scratch), S(stream));
}
