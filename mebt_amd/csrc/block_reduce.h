// Fixed-order sums of a workgroup (device only): no float atomics, so the same input gives the same bits on every run.  The order is
// always lanes by xor butterfly 32..1 (wave_sum, common.h), then waves 0, 1, 2, ... left to right.  A launch that needs one sum over
// many workgroups has each store ONE partial at its own slot of a scratch slab; a second kernel adds the slots with slot_sum.
#pragma once
#include "common.h"

// the sum of one value per wave (`v` is wave uniform), returned to every thread; `sh` [WAVES] may be reused afterwards
template <int WAVES, typename T>
__device__ __forceinline__ T waves_sum(T v, T* sh) {
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = sh[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += sh[w];
    __syncthreads();
    return s;
}

// the workgroup's sum of one value per thread
template <int WAVES, typename T>
__device__ __forceinline__ T block_sum(T v, T* sh) { return waves_sum<WAVES>(wave_sum(v), sh); }

// the index-order sum of `count` fp64 slots by a workgroup of THREADS: thread t adds slots t, t + THREADS, ... in order, then block_sum
template <int THREADS>
__device__ __forceinline__ double slot_sum(const double* __restrict__ p, int64_t count, double* sh) {
    double acc = 0.0;
    for (int64_t j = threadIdx.x; j < count; j += THREADS) acc += p[j];
    return block_sum<THREADS / MEBT_WAVE>(acc, sh);
}
