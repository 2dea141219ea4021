// First-stage training, the codebook's side (include/mebt_hip.h "EMA codebook"; mebt_amd/vqgan.py Codebook.update / init_from): the code
// statistics, the EMA update with random restarts and the restart rows of reference mebt/modules/codebook.py:25-46,66-89.
//
// Reproducibility: no floating-point sum meets an atomic.  codebook_sums builds an inverted index (rows per code) with INTEGER atomics:
// a histogram, an exclusive scan, and a row list per code filled through an atomic slot counter.  Such a list comes back in arrival
// order, so the wave that sums a code first brings its rows into ascending order: a list of at most 64 rows is rank-sorted in
// registers (one row per lane, the rank counted with shuffles); a longer one is not read at all, the wave walks `ids` in row order
// 64 at a time and takes the matches of each ballot from the lowest bit up.  Either way the rows of a code are added one after the
// other in ascending row order in fp32, so the same input gives the same bits on every run.  codebook_ema needs one sum over the codes,
// n = sum N: every workgroup of the first kernel stores the xor-butterfly sum of its 256 codes, and every wave of the second adds those
// partials in the same fixed order.  Every product and sum of the update is a separately rounded fp32 operation (__fmul_rn /
// __fadd_rn / __fdiv_rn): nothing contracts into an FMA.  Every offset into an operand is 64-bit.
#include <cmath>

#include "../host_util.h"

// hipcc contracts a * b + c into an FMA by default, and HIP's __fmul_rn / __fadd_rn are inline functions around the plain operators that
// carry the translation unit's contraction setting: the Makefile compiles this file with -ffp-contract=off, which is what keeps every
// product and sum separately rounded (a quotient's own expansion uses FMAs and is IEEE-correct either way).  The pragma covers the
// operators written in this file, not the ones inside the header's functions.
#pragma clang fp contract(off)

namespace {

constexpr int CT_THREADS = 256;
constexpr int CT_WAVES = CT_THREADS / MEBT_WAVE;
constexpr int CT_COLS = 4 * MEBT_WAVE;               // columns of one pass of a wave on the 16-byte path

// ---- inverted index -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CT_THREADS) void code_count_kernel(const int64_t* __restrict__ ids, int* __restrict__ count, int64_t M, int n_codes) {
    const int64_t m = (int64_t)blockIdx.x * CT_THREADS + threadIdx.x;
    if (m >= M) return;
    const int64_t id = ids[m];
    if (id < 0 || id >= n_codes) return;
    atomicAdd(count + id, 1);
}

// one workgroup: offset[c] = count[0] + ... + count[c - 1], offset[n_codes] = the number of rows with an id in range; cursor[] = 0.
// Thread t owns the codes [t * per, (t + 1) * per).
__global__ __launch_bounds__(CT_THREADS) void code_scan_kernel(const int* __restrict__ count, int* __restrict__ offset, int* __restrict__ cursor,
                                                               int n_codes) {
    __shared__ int sh[CT_THREADS];
    const int per = (n_codes + CT_THREADS - 1) / CT_THREADS;
    const int c0 = threadIdx.x * per;
    const int c1 = c0 + per < n_codes ? c0 + per : n_codes;
    int s = 0;
    for (int c = c0; c < c1; ++c) s += count[c];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < CT_THREADS; ++t) {
            const int v = sh[t];
            sh[t] = run;
            run += v;
        }
        offset[n_codes] = run;
    }
    __syncthreads();
    int run = sh[threadIdx.x];
    for (int c = c0; c < c1; ++c) {
        offset[c] = run;
        run += count[c];
        cursor[c] = 0;
    }
}

__global__ __launch_bounds__(CT_THREADS) void code_fill_kernel(const int64_t* __restrict__ ids, const int* __restrict__ offset,
                                                               int* __restrict__ cursor, int* __restrict__ rows, int64_t M, int n_codes) {
    const int64_t m = (int64_t)blockIdx.x * CT_THREADS + threadIdx.x;
    if (m >= M) return;
    const int64_t id = ids[m];
    if (id < 0 || id >= n_codes) return;
    const int slot = atomicAdd(cursor + id, 1);          // arrival order: code_sum_kernel sorts
    rows[offset[id] + slot] = (int)m;
}

// the columns one lane holds of one pass: a float4 at c0 + 4 * lane (VEC) or one float at c0 + lane
template <bool VEC>
__device__ __forceinline__ f32x4 load_cols(const float* __restrict__ z, int64_t row, int d, int col) {
    const float* p = z + (size_t)row * (size_t)d + col;
    if (VEC) return *reinterpret_cast<const f32x4*>(p);
    return f32x4{*p, 0.f, 0.f, 0.f};
}

template <bool VEC>
__device__ __forceinline__ void add_cols(f32x4& acc, const f32x4& v) {
    acc[0] = __fadd_rn(acc[0], v[0]);
    if (VEC) {
        acc[1] = __fadd_rn(acc[1], v[1]);
        acc[2] = __fadd_rn(acc[2], v[2]);
        acc[3] = __fadd_rn(acc[3], v[3]);
    }
}

template <bool VEC>
__device__ __forceinline__ void add_row(f32x4& acc, const float* __restrict__ z, int64_t row, int d, int col) {
    add_cols<VEC>(acc, load_cols<VEC>(z, row, d, col));
}

// one wave per code.  Its rows in ascending order, each added to the running fp32 sum of its column.
template <bool VEC>
__global__ __launch_bounds__(CT_THREADS) void code_sum_kernel(const int64_t* __restrict__ ids, const float* __restrict__ z,
                                                              const int* __restrict__ count, const int* __restrict__ offset,
                                                              const int* __restrict__ rows, float* __restrict__ n_total,
                                                              float* __restrict__ encode_sum, int64_t M, int n_codes, int d) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int code = blockIdx.x * CT_WAVES + wave;
    if (code >= n_codes) return;                                   // wave uniform
    const int cnt = count[code];
    if (lane == 0) n_total[code] = (float)cnt;
    float* out = encode_sum + (size_t)code * (size_t)d;
    const int width = VEC ? CT_COLS : MEBT_WAVE;
    const int mine = VEC ? 4 * lane : lane;

    int my_row = 0x7FFFFFFF, my_rank = -1;
    if (cnt <= MEBT_WAVE) {                                        // short list: rank sort in registers
        if (lane < cnt) my_row = rows[offset[code] + lane];
        int rank = 0;
        for (int j = 0; j < MEBT_WAVE; ++j) rank += __shfl(my_row, j, MEBT_WAVE) < my_row ? 1 : 0;      // the rows of a list are distinct
        my_rank = lane < cnt ? rank : -1;
    }
    for (int c0 = 0; c0 < d; c0 += width) {
        const int col = c0 + mine;
        const bool live = col < d;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (cnt <= MEBT_WAVE) {
            for (int p = 0; p < cnt; ++p) {
                const unsigned long long who = __ballot(my_rank == p);
                const int row = __shfl(my_row, __ffsll((long long)who) - 1, MEBT_WAVE);
                if (live && who) add_row<VEC>(acc, z, row, d, col);        // `who` is never empty: the rows of a list are distinct
            }
        } else {                                                   // long list: the ids themselves, in row order
            for (int64_t m0 = 0; m0 < M; m0 += MEBT_WAVE) {
                const int64_t m = m0 + lane;
                const int64_t id = m < M ? ids[m] : -1;
                unsigned long long hit = __ballot(id == (int64_t)code);
                while (hit) {                                      // wave uniform: four rows' loads in flight, added in row order
                    int b[4], n = 0;
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (hit) {
                            b[u] = __ffsll((long long)hit) - 1;
                            hit &= hit - 1;
                            n = u + 1;
                        }
                    if (live) {
                        f32x4 v[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (u < n) v[u] = load_cols<VEC>(z, m0 + b[u], d, col);
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (u < n) add_cols<VEC>(acc, v[u]);
                    }
                }
            }
        }
        if (live) {
            if (VEC) *reinterpret_cast<f32x4*>(out + col) = acc;
            else out[col] = acc[0];
        }
    }
}

// ---- EMA update --------------------------------------------------------------------------------------------------------------------
// N = 0.99 N + 0.01 n_total (codebook.py:74) and the workgroup's sum of the new N, lanes by xor butterfly, waves 0..3 in turn
__global__ __launch_bounds__(CT_THREADS) void ema_count_kernel(float* __restrict__ N, const float* __restrict__ n_total, float* __restrict__ part,
                                                               int n_codes) {
    __shared__ float sh[CT_WAVES];
    const int c = blockIdx.x * CT_THREADS + threadIdx.x;
    float v = 0.f;
    if (c < n_codes) {
        v = __fadd_rn(__fmul_rn(N[c], 0.99f), __fmul_rn(0.01f, n_total[c]));
        N[c] = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, MEBT_WAVE));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = __fadd_rn(__fadd_rn(__fadd_rn(sh[0], sh[1]), sh[2]), sh[3]);
}

// one wave per code: codebook.py:75-80,87-89.  `k_rand` NULL: no random restart.
template <bool VEC>
__global__ __launch_bounds__(CT_THREADS) void ema_rows_kernel(const float* __restrict__ N, float* __restrict__ z_avg, float* __restrict__ emb,
                                                              const float* __restrict__ encode_sum, const float* __restrict__ k_rand,
                                                              const float* __restrict__ part, int parts, int* __restrict__ restarted,
                                                              int n_codes, int d, float eps_total, float thres) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int code = blockIdx.x * CT_WAVES + wave;
    if (code >= n_codes) return;                                   // wave uniform
    // n = sum N: lane l adds the partials l, l + 64, ... in order, then the butterfly; the same order in every wave
    float n = 0.f;
    for (int j = lane; j < parts; j += MEBT_WAVE) n = __fadd_rn(n, part[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n = __fadd_rn(n, __shfl_xor(n, o, MEBT_WAVE));
    const float Nc = N[code];
    const float w = __fmul_rn(__fdiv_rn(__fadd_rn(Nc, 1e-7f), __fadd_rn(n, eps_total)), n);
    const bool restart = k_rand != nullptr;
    const float usage = Nc >= thres ? 1.f : 0.f;
    const float unused = __fadd_rn(1.f, -usage);
    if (restart && lane == 0 && usage == 0.f) atomicAdd(restarted, 1);
    const size_t base = (size_t)code * (size_t)d;
    const int step = VEC ? CT_COLS : MEBT_WAVE;
    for (int col = VEC ? 4 * lane : lane; col < d; col += step) {
        f32x4 a, s, k = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {
            a = *reinterpret_cast<const f32x4*>(z_avg + base + col);
            s = *reinterpret_cast<const f32x4*>(encode_sum + base + col);
            if (restart) k = *reinterpret_cast<const f32x4*>(k_rand + base + col);
        } else {
            a[0] = z_avg[base + col];
            s[0] = encode_sum[base + col];
            if (restart) k[0] = k_rand[base + col];
        }
        f32x4 e;
#pragma unroll
        for (int i = 0; i < (VEC ? 4 : 1); ++i) {
            a[i] = __fadd_rn(__fmul_rn(a[i], 0.99f), __fmul_rn(0.01f, s[i]));
            e[i] = __fdiv_rn(a[i], w);
            if (restart) e[i] = __fadd_rn(__fmul_rn(e[i], usage), __fmul_rn(k[i], unused));
        }
        if (VEC) {
            *reinterpret_cast<f32x4*>(z_avg + base + col) = a;
            *reinterpret_cast<f32x4*>(emb + base + col) = e;
        } else {
            z_avg[base + col] = a[0];
            emb[base + col] = e[0];
        }
    }
}

// ---- restart rows (codebook.py:25-32,82-83): out[j] = z[src[j] mod M] + noise[j] * std, the product rounded before the sum ---------------
__global__ __launch_bounds__(CT_THREADS) void restart_rows_kernel(const float* __restrict__ z, const int64_t* __restrict__ src,
                                                                  const float* __restrict__ noise, float* __restrict__ out, int64_t M,
                                                                  int n_codes, int d, float sd) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int code = blockIdx.x * CT_WAVES + wave;
    if (code >= n_codes) return;
    int64_t r = src[code] % M;
    if (r < 0) r += M;
    const float* zr = z + (size_t)r * (size_t)d;
    const size_t base = (size_t)code * (size_t)d;
    for (int col = lane; col < d; col += MEBT_WAVE) {
        float v = zr[col];
        if (noise) v = __fadd_rn(v, __fmul_rn(noise[base + col], sd));
        out[base + col] = v;
    }
}

// this file's slabs start on 16 bytes and carry no workgroup bound: an overload of host_util.h's check, not a copy
int check_scratch(const char* who, const void* scratch, int64_t scratch_bytes, int64_t need) {
    if (!scratch) return fail(MEBT_EINVAL, who, "null pointer");
    if (reinterpret_cast<uintptr_t>(scratch) & 15) return fail(MEBT_EINVAL, who, "scratch must be 16-byte aligned");
    if (scratch_bytes < need) return fail(MEBT_EWORKSPACE, who, "scratch too small");
    return MEBT_OK;
}

int64_t wave_blocks(int n_codes) { return ((int64_t)n_codes + CT_WAVES - 1) / CT_WAVES; }

}  // namespace

extern "C" int64_t mebt_codebook_sums_scratch_bytes(int64_t M, int32_t n_codes) {
    if (M < 1 || n_codes < 1) return 0;
    return 4 * (3 * (int64_t)n_codes + 1 + M);
}

extern "C" int mebt_op_codebook_sums(const int64_t* ids, const float* z, float* n_total, float* encode_sum, int64_t M, int32_t n_codes,
                                     int32_t d, void* scratch, int64_t scratch_bytes, mebt_stream_t stream) {
    const char* who = "codebook_sums";
    if (!ids || !z || !n_total || !encode_sum) return fail(MEBT_EINVAL, who, "null pointer");
    if (M < 1 || n_codes < 1 || d < 1) return fail(MEBT_ESHAPE, who, "need M, n_codes, d >= 1");
    if (M > 0x7FFFFFFFll - CT_THREADS || n_codes > (1 << 28)) return fail(MEBT_ESHAPE, who, "need M < 2^31 - 256 and n_codes <= 2^28");
    if (int rc = check_scratch(who, scratch, scratch_bytes, mebt_codebook_sums_scratch_bytes(M, n_codes))) return rc;
    int* count = reinterpret_cast<int*>(scratch);
    int* offset = count + n_codes;
    int* cursor = offset + n_codes + 1;
    int* rows = cursor + n_codes;
    hipStream_t st = S(stream);
    MEBT_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int) * (size_t)n_codes, st));
    const dim3 row_grid((unsigned)((M + CT_THREADS - 1) / CT_THREADS));
    hipLaunchKernelGGL(code_count_kernel, row_grid, dim3(CT_THREADS), 0, st, ids, count, M, n_codes);
    MEBT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(code_scan_kernel, dim3(1), dim3(CT_THREADS), 0, st, count, offset, cursor, n_codes);
    MEBT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(code_fill_kernel, row_grid, dim3(CT_THREADS), 0, st, ids, offset, cursor, rows, M, n_codes);
    MEBT_HIP_CHECK(hipGetLastError());
    const dim3 code_grid((unsigned)wave_blocks(n_codes));
    if (d % 4 == 0 && aligned16(z) && aligned16(encode_sum))
        hipLaunchKernelGGL(code_sum_kernel<true>, code_grid, dim3(CT_THREADS), 0, st, ids, z, count, offset, rows, n_total, encode_sum, M, n_codes, d);
    else
        hipLaunchKernelGGL(code_sum_kernel<false>, code_grid, dim3(CT_THREADS), 0, st, ids, z, count, offset, rows, n_total, encode_sum, M, n_codes, d);
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int64_t mebt_codebook_ema_scratch_bytes(int32_t n_codes) {
    if (n_codes < 1) return 0;
    return 4 * (((int64_t)n_codes + CT_THREADS - 1) / CT_THREADS);
}

extern "C" int mebt_op_codebook_ema(float* N, float* z_avg, float* embeddings, const float* n_total, const float* encode_sum,
                                    const float* k_rand, int32_t* restarted, int32_t n_codes, int32_t d, float restart_thres, void* scratch,
                                    int64_t scratch_bytes, mebt_stream_t stream) {
    const char* who = "codebook_ema";
    if (!N || !z_avg || !embeddings || !n_total || !encode_sum || !restarted) return fail(MEBT_EINVAL, who, "null pointer");
    if (n_codes < 1 || d < 1) return fail(MEBT_ESHAPE, who, "need n_codes, d >= 1");
    if (n_codes > (1 << 28)) return fail(MEBT_ESHAPE, who, "need n_codes <= 2^28");
    if (int rc = check_scratch(who, scratch, scratch_bytes, mebt_codebook_ema_scratch_bytes(n_codes))) return rc;
    float* part = reinterpret_cast<float*>(scratch);
    const int parts = (n_codes + CT_THREADS - 1) / CT_THREADS;
    hipStream_t st = S(stream);
    MEBT_HIP_CHECK(hipMemsetAsync(restarted, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(ema_count_kernel, dim3((unsigned)parts), dim3(CT_THREADS), 0, st, N, n_total, part, n_codes);
    MEBT_HIP_CHECK(hipGetLastError());
    const float eps_total = (float)((double)n_codes * 1e-7);          // `n + self.n_codes * 1e-7`: the product in double, rounded once
    const dim3 code_grid((unsigned)wave_blocks(n_codes));
    const bool vec = d % 4 == 0 && aligned16(z_avg) && aligned16(embeddings) && aligned16(encode_sum) && (!k_rand || aligned16(k_rand));
    if (vec)
        hipLaunchKernelGGL(ema_rows_kernel<true>, code_grid, dim3(CT_THREADS), 0, st, N, z_avg, embeddings, encode_sum, k_rand, part, parts, restarted,
                           n_codes, d, eps_total, restart_thres);
    else
        hipLaunchKernelGGL(ema_rows_kernel<false>, code_grid, dim3(CT_THREADS), 0, st, N, z_avg, embeddings, encode_sum, k_rand, part, parts, restarted,
                           n_codes, d, eps_total, restart_thres);
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int mebt_op_codebook_restart_rows(const float* z, const int64_t* src, const float* noise, float* out, int64_t M, int32_t n_codes,
                                             int32_t d, mebt_stream_t stream) {
    const char* who = "codebook_restart_rows";
    if (!z || !src || !out) return fail(MEBT_EINVAL, who, "null pointer");
    if (M < 1 || n_codes < 1 || d < 1) return fail(MEBT_ESHAPE, who, "need M, n_codes, d >= 1");
    if (n_codes > (1 << 28)) return fail(MEBT_ESHAPE, who, "need n_codes <= 2^28");
    const float sd = (float)(0.01 / sqrt((double)d));                // codebook.py:29, rounded to fp32 where it meets the fp32 noise
    hipLaunchKernelGGL(restart_rows_kernel, dim3((unsigned)wave_blocks(n_codes)), dim3(CT_THREADS), 0, S(stream), z, src, noise, out, M, n_codes, d,
                       sd);
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}
