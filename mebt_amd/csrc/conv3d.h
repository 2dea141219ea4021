// Voxel addressing of the 3D-VQGAN convolutions, shared by the forward (vqgan.hip) and the backward (vqgan_bwd/vqgan_bwd.hip): voxel index ->
// coordinates, the input voxel a tap reads (replicate padding IS the clamp in tap_coord: the one definition of SamePadConv3d's border), an output
// voxel's place in the three output layouts, GroupNorm's {sum, sum of squares} -> mean and rstd, and the launchers' small host helpers.
#pragma once
#include "host_util.h"

namespace {

// class-local voxel index -> (b, t', h', w')
struct Vox { int b, t, h, w; };
__device__ __forceinline__ Vox decode_vox(const mebt_conv3d_desc& p, long m) {
    Vox v;
    v.w = (int)(m % p.cW); m /= p.cW;
    v.h = (int)(m % p.cH); m /= p.cH;
    v.t = (int)(m % p.cT); v.b = (int)(m / p.cT);
    return v;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// input coordinates: callers index with their own width (size_t; 32 bits in the two thin MFMA kernels, whose launcher vouches for < 2^31 elements)
struct Coord { int t, h, w; };
// the input voxel tap `j` of output voxel v reads.  Replicate padding: a position outside the input box reads the nearest voxel inside
__device__ __forceinline__ Coord tap_coord(const mebt_conv3d_desc& p, const Vox& v, int j) {
    Coord c;
    c.t = clampi(v.t * p.sm[0] + p.tap[j][0], p.Ti - 1);
    c.h = clampi(v.h * p.sm[1] + p.tap[j][1], p.Hi - 1);
    c.w = clampi(v.w * p.sm[2] + p.tap[j][2], p.Wi - 1);
    return c;
}
// its voxel number in the channels-last input
__device__ __forceinline__ size_t in_voxel(const mebt_conv3d_desc& p, const Vox& v, int j) {
    const Coord c = tap_coord(p, v, j);
    return (((size_t)v.b * p.Ti + c.t) * p.Hi + c.h) * p.Wi + c.w;
}
__device__ __forceinline__ size_t out_voxel(const mebt_conv3d_desc& p, const Vox& v) {
    const int t = v.t * p.os[0] + p.pi[0], h = v.h * p.os[1] + p.pi[1], w = v.w * p.os[2] + p.pi[2];
    return (((size_t)v.b * p.To + t) * p.Ho + h) * p.Wo + w;
}

// element offset of channel c of output voxel ov: channels-last (out_mode 0, 1 and the residual) / fp32 [B, C, T, H, W] (out_mode 2; plane = out_plane(p))
__device__ __forceinline__ size_t out_plane(const mebt_conv3d_desc& p) { return (size_t)p.To * p.Ho * p.Wo; }
__device__ __forceinline__ size_t out_cl(const mebt_conv3d_desc& p, size_t ov, int c) { return ov * p.Cout + c; }
__device__ __forceinline__ size_t out_ncdhw(const mebt_conv3d_desc& p, size_t ov, int c, size_t plane) {
    return ((ov / plane) * p.Cout + c) * plane + ov % plane;
}
// the scalar epilogue of the direct, voxel and last-layer kernels: (+ residual) and one store in the descriptor's output layout
template <typename T>
__device__ __forceinline__ void store_out(const mebt_conv3d_desc& p, size_t ov, int c, float a, size_t plane) {
    if (p.resid) a += (float)reinterpret_cast<const T*>(p.resid)[out_cl(p, ov, c)];
    if (p.out_mode == 0) reinterpret_cast<T*>(p.out)[out_cl(p, ov, c)] = (T)a;
    else if (p.out_mode == 1) reinterpret_cast<float*>(p.out)[out_cl(p, ov, c)] = a;
    else reinterpret_cast<float*>(p.out)[out_ncdhw(p, ov, c, plane)] = a;
}

// GroupNorm (eps 1e-6): {sum, sum of squares} of a group of 1 / inv_n elements -> mean, rstd; the forward and the backward both decode them here
__device__ __forceinline__ void gn_mean_rstd(float sum, float sq, float inv_n, float& mean, float& rstd) {
    mean = sum * inv_n;
    const float var = fmaxf(sq * inv_n - mean * mean, 0.f);
    rstd = rsqrtf(var + 1e-6f);
}

// ---- host (S and the other entry-point helpers: host_util.h) ---------------------------------------------------------------
inline bool dtype_ok(int dtype) { return dtype == MEBT_DTYPE_F32 || dtype == MEBT_DTYPE_F16; }
inline bool is_f16(int dtype) { return dtype == MEBT_DTYPE_F16; }
// 256-thread blocks for n items, at least 1 and at most `cap` (grid-stride kernels)
inline unsigned blocks_for(size_t n, unsigned cap) {
    const size_t b = (n + 255) / 256;
    return (unsigned)(b < cap ? (b ? b : 1) : cap);
}
// voxels per workgroup of the GroupNorm statistics passes: <= 512 slabs (adders) per sample
inline int gn_rows_per_block(int64_t vox) {
    int rpb = 64;
    while ((vox + rpb - 1) / rpb > 512) rpb *= 2;
    return rpb;
}

}  // namespace
