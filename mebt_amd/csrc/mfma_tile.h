// The 64-column MFMA tile step of the implicit-GEMM convolutions outside the VQGAN (i3d/i3d.hip, lpips/lpips.hip).  Device only.
// A workgroup of 256 threads owns BM rows (output pixels / voxels) x BN = 64 columns (output channels) and walks K in slices of
// BK = 32; wave w owns the WM 16-row blocks 16 WM w + 16 i.  Both operands sit in LDS as rows of LD elements, K contiguous.
// The kernels keep their own staging, addressing and epilogues: only the tile's shape and the step are shared.
#pragma once
#include "common.h"

constexpr int TILE_BK = 32, TILE_BN = 64, TILE_THREADS = 256;

template <typename T> struct TileCfg;
// fp16: 128 x 64 tiles, each wave 32 rows (two 16-row blocks) x 64 columns, v_mfma_f32_16x16x32_f16
template <> struct TileCfg<f16_t> { static constexpr int VEC = 8, WM = 2, BM = 128, LD = 40; };
// fp32: 64 x 64 tiles, each wave 16 rows x 64 columns, v_mfma_f32_16x16x4_f32 (an exact fp32 FMA chain)
template <> struct TileCfg<float> { static constexpr int VEC = 4, WM = 1, BM = 64, LD = 36; };

template <int WM>
__device__ __forceinline__ void tile_zero(f32x4 (&acc)[WM][4]) {
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// One BK slice: acc[i][j] += A_i B_j^T, computed as D^T = B A^T.  a_rows[i] is the element offset in sA of the LDS row (its 32 K
// values) of the lane's row (lane & 15) of row block i, b_rows[j] the one in sB of column 16 j + (lane & 15); fq = lane >> 4 picks the
// lane's part of K.
// Fragment map of the result, which every epilogue relies on: acc[i][j][r] of a lane is row (lane & 15) of row block i, column
// 16 j + 4 (lane >> 4) + r.
template <typename T, int WM>
__device__ __forceinline__ void tile_mma(f32x4 (&acc)[WM][4], const T* sA, const int (&a_rows)[WM], const T* sB, const int (&b_rows)[4], int fq) {
    if constexpr (sizeof(T) == 2) {
        f16x8 af[WM], bf[4];
#pragma unroll
        for (int i = 0; i < WM; ++i) af[i] = *reinterpret_cast<const f16x8*>(&sA[a_rows[i] + fq * 8]);
#pragma unroll
        for (int j = 0; j < 4; ++j) bf[j] = *reinterpret_cast<const f16x8*>(&sB[b_rows[j] + fq * 8]);
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[j], af[i], acc[i][j], 0, 0, 0);
    } else {
#pragma unroll
        for (int q = 0; q < TILE_BK / 4; ++q) {
            float af[WM], bf[4];
#pragma unroll
            for (int i = 0; i < WM; ++i) af[i] = sA[a_rows[i] + 4 * q + fq];
#pragma unroll
            for (int j = 0; j < 4; ++j) bf[j] = sB[b_rows[j] + 4 * q + fq];
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j], af[i], acc[i][j], 0, 0, 0);
        }
    }
}
