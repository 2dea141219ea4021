// 3D-VQGAN first stage, backward (reference mebt/vqgan.py:98-102,183-184: the autoencoder objective before discriminator_iter_start,
// recon_loss + commitment_loss): the gradient of every operator of csrc/vqgan.hip.
//
//   data gradient of a convolution   the gradient on the PADDED input lattice is itself a convolution of dy (a stride-s convolution's
//                                    is a transposed one, issued per parity class; a transposed one's is a strided one), so it runs on
//                                    mebt_op_conv3d's kernels.  "Zero outside" is a physical zero border: mebt_op_pad_zero copies dy into a
//                                    buffer wide enough that no tap leaves it (the forward's clamp never acts).  mebt_op_halo_fold then
//                                    adds the halo of the fp32 lattice onto the border voxels the forward's clamp folded it onto, adds
//                                    the residual branch's gradient and stores once.
//   weight and bias gradient         conv3d_wgrad_kernel: implicit GEMM, M = Cout, N = ntaps x Cin, K = voxels, 64 x 64 tiles of one tap,
//                                    v_mfma_f32_16x16x32_f16 (fp16) or fp32 FMAs (parity mode).  K is split over workgroups; every
//                                    workgroup stores one fp32 slab, a finishing kernel adds the slabs in index order and removes the
//                                    gradient scale.  No float atomics, no hand-off inside a launch: the same inputs give the same bits.
//   GroupNorm + SiLU                 h and sigmoid(h) recomputed from x and the forward's statistics; per-channel slabs, fixed-order
//                                    fp64 finish, then dx.
//   seeds                            L1 sign seed, quantiser seed (commitment + straight-through).
#include "../conv3d.h"
#include <string.h>

namespace {

// ------------------------------------------------------------------------------------------------
// zero-padded copy: dst [B, pT, pH, pW, C] of T <- src at offset `front`, zero elsewhere
// src_mode 0: channels-last T; 1: channels-last fp32; 2: fp32 [B, C, T, H, W]
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pad_zero_kernel(const void* src, T* dst, int Tn, int Hn, int Wn, int fT, int fH, int fW, int pT, int pH,
                                                       int pW, int C, int src_mode, long total) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        long r = i;
        const int c = (int)(r % C); r /= C;
        const int w = (int)(r % pW) - fW; r /= pW;
        const int h = (int)(r % pH) - fH; r /= pH;
        const int t = (int)(r % pT) - fT;
        const long b = r / pT;
        float v = 0.f;
        if (t >= 0 && t < Tn && h >= 0 && h < Hn && w >= 0 && w < Wn) {
            const size_t sp = ((size_t)t * Hn + h) * Wn + w, plane = (size_t)Tn * Hn * Wn;
            if (src_mode == 0) v = (float)reinterpret_cast<const T*>(src)[((size_t)b * plane + sp) * C + c];
            else if (src_mode == 1) v = reinterpret_cast<const float*>(src)[((size_t)b * plane + sp) * C + c];
            else v = reinterpret_cast<const float*>(src)[((size_t)b * C + c) * plane + sp];
        }
        dst[i] = (T)v;
    }
}

// ------------------------------------------------------------------------------------------------
// halo fold: dx[b, i, c] = add[b, i, c] + sum over the lattice positions q whose clamped coordinate is i, per dimension
// q = i + f inside; the first voxel also takes q = 0 .. f - 1, the last one q = D + f .. pD - 1 (a one-voxel axis takes all).
// ------------------------------------------------------------------------------------------------
template <typename T, typename TO>
__global__ __launch_bounds__(256) void halo_fold_kernel(const float* dxp, const T* add, TO* dx, int Tn, int Hn, int Wn, int pT, int pH, int pW,
                                                        int fT, int fH, int fW, int C, long total) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        long r = i;
        const int c = (int)(r % C); r /= C;
        const int w = (int)(r % Wn); r /= Wn;
        const int h = (int)(r % Hn); r /= Hn;
        const int t = (int)(r % Tn);
        const long b = r / Tn;
        const int t0 = t == 0 ? 0 : t + fT, t1 = t == Tn - 1 ? pT - 1 : t + fT;
        const int h0 = h == 0 ? 0 : h + fH, h1 = h == Hn - 1 ? pH - 1 : h + fH;
        const int w0 = w == 0 ? 0 : w + fW, w1 = w == Wn - 1 ? pW - 1 : w + fW;
        float s = 0.f;
        for (int qt = t0; qt <= t1; ++qt)
            for (int qh = h0; qh <= h1; ++qh)
                for (int qw = w0; qw <= w1; ++qw) s += dxp[((((size_t)b * pT + qt) * pH + qh) * pW + qw) * C + c];
        if (add) s += (float)add[i];
        dx[i] = (TO)s;
    }
}

// ------------------------------------------------------------------------------------------------
// weight + bias gradient.  Workgroup (ks, tap j, tile): dw[co0 .. +63][j][ci0 .. +63] over the voxels [ks * chunk, (ks + 1) * chunk) of
// the class, in k-steps of 32 voxels.  Both operands arrive voxel-major (a voxel's channels are contiguous) and are written to LDS
// transposed, [channel][voxel], so that a lane's 8 k-values are one 16-byte LDS read.  Rows beyond the channel count and voxels beyond
// the chunk are zeros.
// ------------------------------------------------------------------------------------------------
constexpr int WT = 64, WK = 32, WLD = 40;

// channels c0 .. c0 + 7 of one channels-last voxel (C channels at s): 16-byte loads where C % 8 == 0, else scalars; channels >= C keep a's value
template <typename T>
__device__ __forceinline__ void load8_cl(const T* s, int c0, int C, T (&a)[8]) {
    if ((C & 7) == 0) {
        if (c0 < C) {
            *reinterpret_cast<u32x4*>(a) = *reinterpret_cast<const u32x4*>(s + c0);
            if (sizeof(T) == 4) *reinterpret_cast<u32x4*>(a + 4) = *reinterpret_cast<const u32x4*>(s + c0 + 4);
        }
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) if (c0 + q < C) a[q] = s[c0 + q];
    }
}

template <typename T>
__device__ __forceinline__ void load8_dy(const mebt_conv3d_desc& p, size_t ov, int c0, T (&a)[8]) {
    if (p.out_mode == 0) {
        const T* s = reinterpret_cast<const T*>(p.out) + out_cl(p, ov, 0);
        load8_cl(s, c0, p.Cout, a);
    } else if (p.out_mode == 1) {
        const float* s = reinterpret_cast<const float*>(p.out) + out_cl(p, ov, 0);
#pragma unroll
        for (int q = 0; q < 8; ++q) if (c0 + q < p.Cout) a[q] = (T)s[c0 + q];
    } else {
        const size_t plane = out_plane(p);            // out_ncdhw(p, ov, c0 + q, plane) with the sample's base taken once
        const float* s = reinterpret_cast<const float*>(p.out) + (ov / plane) * p.Cout * plane + ov % plane;
#pragma unroll
        for (int q = 0; q < 8; ++q) if (c0 + q < p.Cout) a[q] = (T)s[(size_t)(c0 + q) * plane];
    }
}

template <typename T>
__device__ __forceinline__ void load8_x(const mebt_conv3d_desc& p, const Vox& v, int j, int c0, T (&b)[8]) {
    const Coord c = tap_coord(p, v, j);
    const size_t plane = (size_t)p.Ti * p.Hi * p.Wi, sp = ((size_t)c.t * p.Hi + c.h) * p.Wi + c.w;
    if (p.in_mode == 0) {
        const T* s = reinterpret_cast<const T*>(p.in) + ((size_t)v.b * plane + sp) * p.Cin;
        load8_cl(s, c0, p.Cin, b);
    } else {
        const float* s = reinterpret_cast<const float*>(p.in) + (size_t)v.b * p.Cin * plane + sp;
#pragma unroll
        for (int q = 0; q < 8; ++q) if (c0 + q < p.Cin) b[q] = (T)s[(size_t)(c0 + q) * plane];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void conv3d_wgrad_kernel(const mebt_conv3d_desc p, float* part, long chunk, int ci_tiles, size_t stride) {
    __shared__ __attribute__((aligned(16))) T sA[WT * WLD];       // dy^T  [co][voxel]
    __shared__ __attribute__((aligned(16))) T sB[WT * WLD];       // x^T   [ci][voxel] of tap j
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ks = blockIdx.x, j = blockIdx.y;
    const int co0 = ((int)blockIdx.z / ci_tiles) * WT, ci0 = ((int)blockIdx.z % ci_tiles) * WT;
    const long Mcls = (long)p.B * p.cT * p.cH * p.cW;
    const long k0 = (long)ks * chunk, k1 = k0 + chunk < Mcls ? k0 + chunk : Mcls;
    const int lv = tid >> 3, lc = (tid & 7) * 8;                  // loader: voxel of the k-step, first of 8 channels of the tile
    const bool want_bias = j == 0 && ci0 == 0;
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    float bsum = 0.f;
    for (long kb = k0; kb < k1; kb += WK) {
        __attribute__((aligned(16))) T a[8];
        __attribute__((aligned(16))) T b[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) { a[q] = (T)0.f; b[q] = (T)0.f; }
        const long m = kb + lv;
        if (m < k1) {
            const Vox v = decode_vox(p, m);
            load8_dy<T>(p, out_voxel(p, v), co0 + lc, a);
            load8_x<T>(p, v, j, ci0 + lc, b);
        }
        __syncthreads();                                          // the previous k-step's reads are done
#pragma unroll
        for (int q = 0; q < 8; ++q) { sA[(lc + q) * WLD + lv] = a[q]; sB[(lc + q) * WLD + lv] = b[q]; }
        __syncthreads();
        if constexpr (sizeof(T) == 2) {
            // wave: rows co0 + 16 wave .. + 15; acc[4 n + r] = dw[16 wave + 4 (lane >> 4) + r][16 n + (lane & 15)]
            const int fr = lane & 15, fc = (lane >> 4) * 8;
            const f16x8 af = *reinterpret_cast<const f16x8*>(&sA[(16 * wave + fr) * WLD + fc]);
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const f16x8 bf = *reinterpret_cast<const f16x8*>(&sB[(16 * n + fr) * WLD + fc]);
                f32x4 c = {acc[4 * n], acc[4 * n + 1], acc[4 * n + 2], acc[4 * n + 3]};
                c = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, c, 0, 0, 0);
                acc[4 * n] = c[0]; acc[4 * n + 1] = c[1]; acc[4 * n + 2] = c[2]; acc[4 * n + 3] = c[3];
            }
        } else {
            // thread: co 4 (tid >> 4) + q, ci 4 (tid & 15) + r; acc[4 q + r]
            const int tc = (tid >> 4) * 4, ti = (tid & 15) * 4;
            for (int v = 0; v < WK; ++v) {
                float av[4], bv[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) { av[q] = (float)sA[(tc + q) * WLD + v]; bv[q] = (float)sB[(ti + q) * WLD + v]; }
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[4 * q + r] += av[q] * bv[r];
            }
        }
        if (want_bias && tid < WT)
            for (int v = 0; v < WK; ++v) bsum += (float)sA[tid * WLD + v];
    }
    float* slab = part + (size_t)ks * stride;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + 16 * wave + 4 * (lane >> 4) + r, ci = ci0 + 16 * n + (lane & 15);
                if (co < p.Cout && ci < p.Cin) slab[((size_t)co * p.ntaps + j) * p.Cin + ci] = acc[4 * n + r];
            }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + (tid >> 4) * 4 + q, ci = ci0 + (tid & 15) * 4 + r;
                if (co < p.Cout && ci < p.Cin) slab[((size_t)co * p.ntaps + j) * p.Cin + ci] = acc[4 * q + r];
            }
    }
    if (want_bias && tid < WT && co0 + tid < p.Cout) slab[(size_t)p.Cout * p.ntaps * p.Cin + co0 + tid] = bsum;
}

// out[i] = scale * (slab 0 + slab 1 + ...)[i] in index order; the first `nw` go to dw, the rest (bias sums) to db when given
__global__ __launch_bounds__(256) void wgrad_finish_kernel(const float* part, float* dw, float* db, size_t nw, size_t stride, int nsplit, float scale) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= stride) return;
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s += part[(size_t)k * stride + i];
    if (i < nw) dw[i] = s * scale;
    else if (db) db[i - nw] = s * scale;
}

// ------------------------------------------------------------------------------------------------
// GroupNorm + SiLU backward
// ------------------------------------------------------------------------------------------------
// xhat and dh = dy * s * (1 + h (1 - s)) of one element; mean / rstd from the forward's {sum, sum of squares} by the forward's own gn_mean_rstd
__device__ __forceinline__ void gn_point(float x, float dy, float sum, float sq, float inv_n, float gamma, float beta, float& xhat, float& dh,
                                         float& rstd) {
    float mean;
    gn_mean_rstd(sum, sq, inv_n, mean, rstd);
    xhat = (x - mean) * rstd;
    const float h = xhat * gamma + beta;
    const float s = 1.0f / (1.0f + expf(-h));
    dh = dy * s * (1.0f + h * (1.0f - s));
}

// pass 1: part[b][slab][0][c] = sum dh, part[b][slab][1][c] = sum dh * xhat over the slab's voxels (thread layout of gn_stats_kernel)
template <typename T>
__global__ __launch_bounds__(256) void gn_bwd_partial_kernel(const T* x, const T* dy, const float* stats, const float* gamma, const float* beta,
                                                             float* part, long vox, int C, int rpb) {
    __shared__ float red[2][256 * 4];
    const int b = blockIdx.y, cpg = C / 32;
    const int lpr = C / 4, rows_par = 256 / lpr;
    const int cl = threadIdx.x % lpr, rl = threadIdx.x / lpr;
    const long r0 = (long)blockIdx.x * rpb, r1 = r0 + rpb < vox ? r0 + rpb : vox;
    const float inv_n = 1.0f / ((float)vox * cpg);
    f32x4 s1 = {0, 0, 0, 0}, s2 = {0, 0, 0, 0};
    if (rl < rows_par) {
        const int c = cl * 4;
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + c), b4 = *reinterpret_cast<const f32x4*>(beta + c);
        float sm[4], sq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int g = (c + j) / cpg;
            sm[j] = stats[((size_t)b * 32 + g) * 2]; sq[j] = stats[((size_t)b * 32 + g) * 2 + 1];
        }
        for (long r = r0 + rl; r < r1; r += rows_par) {
            const size_t e = ((size_t)b * vox + r) * C + c;
            const f32x4 xv = load4<T>(x + e), dv = load4<T>(dy + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float xhat, dh, rstd;
                gn_point(xv[j], dv[j], sm[j], sq[j], inv_n, g4[j], b4[j], xhat, dh, rstd);
                s1[j] += dh; s2[j] += dh * xhat;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { red[0][threadIdx.x * 4 + j] = s1[j]; red[1][threadIdx.x * 4 + j] = s2[j]; }
    __syncthreads();
    float* out = part + ((size_t)b * gridDim.x + blockIdx.x) * 2 * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        float a = 0.f, q = 0.f;
        for (int r = 0; r < rows_par; ++r) {
            a += red[0][(r * lpr + c / 4) * 4 + (c & 3)];
            q += red[1][(r * lpr + c / 4) * 4 + (c & 3)];
        }
        out[c] = a; out[C + c] = q;
    }
}
// finish, groups: gs[b][g] = {sum_c gamma_c sum dh, sum_c gamma_c sum dh xhat}, slabs then channels in index order, fp64
__global__ __launch_bounds__(64) void gn_bwd_group_kernel(const float* part, const float* gamma, double* gs, int B, int nslab, int C) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= B * 32) return;
    const int b = i / 32, g = i % 32, cpg = C / 32;
    double a = 0.0, q = 0.0;
    for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
        double ca = 0.0, cq = 0.0;
        for (int s = 0; s < nslab; ++s) {
            const float* src = part + ((size_t)b * nslab + s) * 2 * C;
            ca += (double)src[c]; cq += (double)src[C + c];
        }
        a += (double)gamma[c] * ca; q += (double)gamma[c] * cq;
    }
    gs[(size_t)i * 2] = a; gs[(size_t)i * 2 + 1] = q;
}
// finish, parameters: dbeta_c = scale * sum dh, dgamma_c = scale * sum dh xhat over samples and slabs in index order, fp64
__global__ __launch_bounds__(256) void gn_bwd_param_kernel(const float* part, float* dgamma, float* dbeta, int B, int nslab, int C, float scale) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, q = 0.0;
    for (long s = 0; s < (long)B * nslab; ++s) { a += (double)part[(size_t)s * 2 * C + c]; q += (double)part[(size_t)s * 2 * C + C + c]; }
    dbeta[c] = (float)(a * (double)scale); dgamma[c] = (float)(q * (double)scale);
}
// pass 2: dx = rstd (gamma dh - mean_g(gamma dh) - xhat mean_g(gamma dh xhat)) (+ add)
template <typename T>
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const T* x, const T* dy, const T* add, T* dx, const float* stats, const double* gs,
                                                           const float* gamma, const float* beta, long vox, int C, long total4) {
    const int cpg = C / 32;
    const float inv_n = 1.0f / ((float)vox * cpg);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
        const long e = i * 4;
        const int c = (int)(e % C);
        const long b = e / (vox * C);
        const f32x4 xv = load4<T>(x + e), dv = load4<T>(dy + e);
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + c), b4 = *reinterpret_cast<const f32x4*>(beta + c);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int g = (c + j) / cpg;
            const size_t si = ((size_t)b * 32 + g) * 2;
            float xhat, dh, rstd;
            gn_point(xv[j], dv[j], stats[si], stats[si + 1], inv_n, g4[j], b4[j], xhat, dh, rstd);
            const float m1 = (float)(gs[si] * (double)inv_n), m2 = (float)(gs[si + 1] * (double)inv_n);
            o[j] = rstd * (g4[j] * dh - m1 - xhat * m2);
        }
        if (add) o += load4<T>(add + e);
        store4<T>(dx + e, o);
    }
}

// ------------------------------------------------------------------------------------------------
// seeds
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void l1_seed_kernel(const float* xr, const float* x, float* out, size_t n, float c) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float d = xr[i] - x[i];
        out[i] = d > 0.f ? c : (d < 0.f ? -c : 0.f);
    }
}
__global__ __launch_bounds__(256) void vq_seed_kernel(const float* z, const float* e, const int64_t* ids, const float* gst, float* dz, size_t n, int d,
                                                      int n_codes, float c) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        long id = ids[i / d];
        id = id < 0 ? 0 : (id >= n_codes ? n_codes - 1 : id);
        const float v = c * (z[i] - e[(size_t)id * d + i % d]);
        dz[i] = gst ? v + gst[i] : v;
    }
}

}  // namespace

extern "C" int mebt_op_pad_zero(int32_t dtype, const void* src, void* dst, int32_t B, int32_t T, int32_t H, int32_t W, int32_t fT, int32_t fH,
                                int32_t fW, int32_t pT, int32_t pH, int32_t pW, int32_t C, int32_t src_mode, mebt_stream_t stream) {
    if (!dtype_ok(dtype)) { mebt_set_error("pad_zero: dtype must be f32 or f16"); return MEBT_EDTYPE; }
    if (B < 0 || T < 0 || H < 0 || W < 0 || C < 0 || fT < 0 || fH < 0 || fW < 0 || pT < T + fT || pH < H + fH || pW < W + fW || src_mode < 0 || src_mode > 2) {
        mebt_set_error("pad_zero: the padded box must hold the source at its offset (p >= n + front, front >= 0); src_mode 0..2");
        return MEBT_ESHAPE;
    }
    const size_t total = (size_t)B * pT * pH * pW * C;
    if (!total) return MEBT_OK;
    if (!dst || (!src && (size_t)B * T * H * W * C)) { mebt_set_error("pad_zero: null pointer"); return MEBT_EINVAL; }
    const unsigned blocks = blocks_for(total, 65536);
    with_dtype(dtype, [&](auto tag) {
        hipLaunchKernelGGL(pad_zero_kernel<decltype(tag)>, dim3(blocks), dim3(256), 0, S(stream), src, (decltype(tag)*)dst, T, H, W, fT, fH, fW, pT, pH, pW, C, src_mode, (long)total);
    });
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int mebt_op_halo_fold(int32_t dtype, const float* dxp, const void* add, void* dx, int32_t B, int32_t T, int32_t H, int32_t W, int32_t pT,
                                 int32_t pH, int32_t pW, int32_t fT, int32_t fH, int32_t fW, int32_t C, int32_t out_mode, mebt_stream_t stream) {
    if (!dtype_ok(dtype)) { mebt_set_error("halo_fold: dtype must be f32 or f16"); return MEBT_EDTYPE; }
    if (B < 0 || T < 0 || H < 0 || W < 0 || C < 0 || fT < 0 || fH < 0 || fW < 0 || pT < T + fT || pH < H + fH || pW < W + fW || out_mode < 0 || out_mode > 1) {
        mebt_set_error("halo_fold: the lattice must hold the tensor at its offset (p >= n + front, front >= 0); out_mode 0..1");
        return MEBT_ESHAPE;
    }
    const size_t total = (size_t)B * T * H * W * C;
    if (!total) return MEBT_OK;
    if (!dxp || !dx) { mebt_set_error("halo_fold: null pointer"); return MEBT_EINVAL; }
    const unsigned blocks = blocks_for(total, 65536);
#define FOLD(T_, TO_) hipLaunchKernelGGL((halo_fold_kernel<T_, TO_>), dim3(blocks), dim3(256), 0, S(stream), dxp, (const T_*)add, (TO_*)dx, T, H, W, pT, pH, pW, fT, fH, fW, C, (long)total)
    if (is_f16(dtype)) { if (out_mode == 0) FOLD(f16_t, f16_t); else FOLD(f16_t, float); }
    else FOLD(float, float);
#undef FOLD
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int64_t mebt_conv3d_wgrad_scratch_bytes(const mebt_conv3d_desc* d, int32_t nsplit) {
    if (!d || nsplit < 1) return 0;
    return (int64_t)nsplit * ((int64_t)d->Cout * d->ntaps * d->Cin + d->Cout) * 4;
}

extern "C" int mebt_op_conv3d_wgrad(int32_t dtype, const mebt_conv3d_desc* d, float* dw, float* db, float inv_scale, int32_t nsplit, void* scratch,
                                    int64_t scratch_bytes, mebt_stream_t stream) {
    if (!d || !dw) { mebt_set_error("conv3d_wgrad: null pointer"); return MEBT_EINVAL; }
    if (!dtype_ok(dtype)) { mebt_set_error("conv3d_wgrad: dtype must be f32 or f16"); return MEBT_EDTYPE; }
    const mebt_conv3d_desc& p = *d;
    if (p.ntaps < 1 || p.ntaps > MEBT_CONV_MAX_TAPS || p.Cin < 1 || p.Cout < 1 || nsplit < 1 || p.in_mode < 0 || p.in_mode > 1 || p.out_mode < 0 || p.out_mode > 2) {
        mebt_set_error("conv3d_wgrad: bad tap / channel / split count or layout mode");
        return MEBT_ESHAPE;
    }
    const size_t nw = (size_t)p.Cout * p.ntaps * p.Cin, stride = nw + p.Cout;
    const long mcls = (long)p.B * p.cT * p.cH * p.cW;
    if (mcls <= 0) {           // an empty class: the gradient of nothing
        MEBT_HIP_CHECK(hipMemsetAsync(dw, 0, nw * 4, S(stream)));
        if (db) MEBT_HIP_CHECK(hipMemsetAsync(db, 0, (size_t)p.Cout * 4, S(stream)));
        return MEBT_OK;
    }
    if (!p.in || !p.out || !scratch) { mebt_set_error("conv3d_wgrad: null pointer"); return MEBT_EINVAL; }
    if (scratch_bytes < mebt_conv3d_wgrad_scratch_bytes(d, nsplit)) { mebt_set_error("conv3d_wgrad: scratch too small (mebt_conv3d_wgrad_scratch_bytes)"); return MEBT_EINVAL; }
    long chunk = (mcls + nsplit - 1) / nsplit;
    chunk = (chunk + WK - 1) / WK * WK;
    const int ns = (int)((mcls + chunk - 1) / chunk);               // <= nsplit: every workgroup has voxels
    const int co_tiles = (p.Cout + WT - 1) / WT, ci_tiles = (p.Cin + WT - 1) / WT;
    if ((long)co_tiles * ci_tiles > 65535) { mebt_set_error("conv3d_wgrad: too many channel tiles"); return MEBT_ESHAPE; }
    const dim3 grid(ns, p.ntaps, co_tiles * ci_tiles);
    float* part = reinterpret_cast<float*>(scratch);
    with_dtype(dtype, [&](auto tag) { hipLaunchKernelGGL(conv3d_wgrad_kernel<decltype(tag)>, grid, dim3(256), 0, S(stream), p, part, chunk, ci_tiles, stride); });
    hipLaunchKernelGGL(wgrad_finish_kernel, dim3((unsigned)((stride + 255) / 256)), dim3(256), 0, S(stream), part, dw, db, nw, stride, ns, inv_scale);
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int64_t mebt_groupnorm_silu_bwd_scratch_bytes(int32_t B, int64_t vox_per_sample, int32_t C) {
    if (B <= 0 || vox_per_sample <= 0 || C <= 0) return 0;
    const int rpb = gn_rows_per_block(vox_per_sample);
    const int64_t nslab = (vox_per_sample + rpb - 1) / rpb;
    return (int64_t)B * 32 * 2 * 8 + (int64_t)B * nslab * 2 * C * 4;
}

extern "C" int mebt_op_groupnorm_silu_bwd(int32_t dtype, const void* x, const float* stats, const float* gamma, const float* beta, const void* dy,
                                          const void* add, void* dx, float* dgamma, float* dbeta, float inv_scale, int32_t B,
                                          int64_t vox_per_sample, int32_t C, void* scratch, int64_t scratch_bytes, mebt_stream_t stream) {
    if (C % 32 || C > 1024 || C < 32) { mebt_set_error("groupnorm_bwd: channels must be a multiple of 32 (32 groups) and <= 1024"); return MEBT_ESHAPE; }
    if (!dtype_ok(dtype)) { mebt_set_error("groupnorm_bwd: dtype must be f32 or f16"); return MEBT_EDTYPE; }
    if (!dgamma || !dbeta) { mebt_set_error("groupnorm_bwd: null pointer"); return MEBT_EINVAL; }
    if (B <= 0 || vox_per_sample <= 0) {
        MEBT_HIP_CHECK(hipMemsetAsync(dgamma, 0, (size_t)C * 4, S(stream)));
        MEBT_HIP_CHECK(hipMemsetAsync(dbeta, 0, (size_t)C * 4, S(stream)));
        return MEBT_OK;
    }
    if (!x || !stats || !gamma || !beta || !dy || !dx || !scratch) { mebt_set_error("groupnorm_bwd: null pointer"); return MEBT_EINVAL; }
    if (scratch_bytes < mebt_groupnorm_silu_bwd_scratch_bytes(B, vox_per_sample, C)) { mebt_set_error("groupnorm_bwd: scratch too small (mebt_groupnorm_silu_bwd_scratch_bytes)"); return MEBT_EINVAL; }
    const int rpb = gn_rows_per_block(vox_per_sample);
    const int nslab = (int)((vox_per_sample + rpb - 1) / rpb);
    double* gs = reinterpret_cast<double*>(scratch);
    float* part = reinterpret_cast<float*>(gs + (size_t)B * 64);
    const dim3 grid(nslab, B);
    const long total4 = (long)B * vox_per_sample * C / 4;
    const unsigned ablocks = blocks_for((size_t)total4, 8192);
    auto run = [&](auto* xt, auto* dyt, auto* addt, auto* dxt) {
        hipLaunchKernelGGL(gn_bwd_partial_kernel, grid, dim3(256), 0, S(stream), xt, dyt, stats, gamma, beta, part, (long)vox_per_sample, C, rpb);
        hipLaunchKernelGGL(gn_bwd_group_kernel, dim3((B * 32 + 63) / 64), dim3(64), 0, S(stream), part, gamma, gs, B, nslab, C);
        hipLaunchKernelGGL(gn_bwd_param_kernel, dim3((C + 255) / 256), dim3(256), 0, S(stream), part, dgamma, dbeta, B, nslab, C, inv_scale);
        hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3(ablocks), dim3(256), 0, S(stream), xt, dyt, addt, dxt, stats, gs, gamma, beta, (long)vox_per_sample, C, total4);
    };
    with_dtype(dtype, [&](auto tag) { using E = decltype(tag); run((const E*)x, (const E*)dy, (const E*)add, (E*)dx); });
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int mebt_op_l1_seed(const float* x_recon, const float* x, float* out, int64_t n, float c, mebt_stream_t stream) {
    if (n <= 0) return MEBT_OK;
    if (!x_recon || !x || !out) { mebt_set_error("l1_seed: null pointer"); return MEBT_EINVAL; }
    hipLaunchKernelGGL(l1_seed_kernel, dim3(blocks_for((size_t)n, 8192)), dim3(256), 0, S(stream), x_recon, x, out, (size_t)n, c);
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int mebt_op_vq_seed(const float* z, const float* embeddings, const int64_t* ids, const float* g_st, float* dz, int64_t M, int32_t d,
                               int32_t n_codes, float c, mebt_stream_t stream) {
    if (M <= 0 || d <= 0) return MEBT_OK;
    if (n_codes < 1) { mebt_set_error("vq_seed: empty codebook"); return MEBT_ESHAPE; }
    if (!z || !embeddings || !ids || !dz) { mebt_set_error("vq_seed: null pointer"); return MEBT_EINVAL; }
    hipLaunchKernelGGL(vq_seed_kernel, dim3(blocks_for((size_t)M * d, 8192)), dim3(256), 0, S(stream), z, embeddings, ids, g_st, dz, (size_t)M * d, d, n_codes, c);
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}
