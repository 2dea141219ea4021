// First-stage discriminators (reference mebt/vqgan.py:27-37,416-520), the reductions: BatchNorm batch statistics and the values of the
// GAN losses.  DESIGN.md §9i.  The convolutions and the normalisation pass are in disc_conv.hip.
//
// Layout: a map is channels-last [M, C] (M = batch x voxels) of `dtype`: fp16 or fp32.  Sums are fp64 from the element on and every
// offset is 64-bit.  No float atomics and no reduction whose order depends on the launch: a workgroup adds its rows (or elements) in
// order and stores ONE partial at its own slot, a second kernel adds the slots in index order (block_reduce.h slot_sum), so the same
// input gives the same bits on every run.
//
// BatchNorm: slot [channel][moment][g] holds {sum, sum of squares} of rows [g R, (g + 1) R), R = MEBT_DISC_BN_ROWS; bn_finish turns
// a channel's slots into mean and 1 / sqrt(var + eps) (biased variance, clamped at 0) and, when asked, moves the running buffers
// (momentum 0.1, unbiased variance) as nn.BatchNorm does in training mode.
#include "../block_reduce.h"
#include "../host_util.h"
#include <math.h>

namespace {

constexpr double DISC_BN_EPS = 1e-5, DISC_BN_MOMENTUM = 0.1;
constexpr int DISC_LOSS_ITEMS = 2048;       // elements per workgroup of the loss partials (at most DISC_LOSS_MAX_BLOCKS workgroups)
constexpr int DISC_LOSS_MAX_BLOCKS = 1024;

// workgroup g adds rows [g R, (g + 1) R) in order, one thread per channel
template <typename T>
__global__ __launch_bounds__(256) void disc_bn_partials_kernel(const T* x, long M, int C, double* slots, long n_slots) {
    const long r0 = (long)blockIdx.x * MEBT_DISC_BN_ROWS;
    const long r1 = r0 + MEBT_DISC_BN_ROWS < M ? r0 + MEBT_DISC_BN_ROWS : M;
    for (int c = threadIdx.x; c < C; c += 256) {
        double s1 = 0.0, s2 = 0.0;
        for (long r = r0; r < r1; ++r) { const double v = (double)(float)x[(size_t)r * C + c]; s1 += v; s2 += v * v; }
        slots[((size_t)c * 2 + 0) * n_slots + blockIdx.x] = s1;
        slots[((size_t)c * 2 + 1) * n_slots + blockIdx.x] = s2;
    }
}

// one workgroup per channel: the slots in index order -> mean, rstd (fp32 [2][C]); `update`: the running buffers and num_batches_tracked
__global__ __launch_bounds__(256) void disc_bn_finish_kernel(const double* slots, long n_slots, int C, double count, float* stats, float* running_mean,
                                                             float* running_var, int64_t* num_batches, int update) {
    __shared__ double sh[4];
    const int c = blockIdx.x;
    const double s1 = slot_sum<256>(slots + ((size_t)c * 2 + 0) * n_slots, n_slots, sh);
    const double s2 = slot_sum<256>(slots + ((size_t)c * 2 + 1) * n_slots, n_slots, sh);
    if (threadIdx.x != 0) return;
    const double mean = s1 / count;
    double var = s2 / count - mean * mean;
    var = var > 0.0 ? var : 0.0;
    stats[c] = (float)mean;
    stats[C + c] = (float)(1.0 / sqrt(var + DISC_BN_EPS));
    if (update) {
        running_mean[c] = (float)((1.0 - DISC_BN_MOMENTUM) * (double)running_mean[c] + DISC_BN_MOMENTUM * mean);
        running_var[c] = (float)((1.0 - DISC_BN_MOMENTUM) * (double)running_var[c] + DISC_BN_MOMENTUM * var * (count / (count - 1.0)));
        if (c == 0 && num_batches) *num_batches += 1;
    }
}

__device__ __forceinline__ double softplus64(double x) { return x > 20.0 ? x : log1p(exp(x)); }

// workgroup g takes elements [g per, (g + 1) per): slot [k][g] = the sum of term k
template <typename T>
__global__ __launch_bounds__(256) void disc_logit_partials_kernel(const T* l, int64_t n, int64_t per, double* slots, int nb) {
    __shared__ double sh[4];
    const int64_t e0 = (int64_t)blockIdx.x * per, e1 = e0 + per < n ? e0 + per : n;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = e0 + threadIdx.x; i < e1; i += 256) {
        const double v = (double)(float)l[i];
        s[0] += v;
        s[1] += 1.0 - v > 0.0 ? 1.0 - v : 0.0;
        s[2] += 1.0 + v > 0.0 ? 1.0 + v : 0.0;
        s[3] += softplus64(-v);
        s[4] += softplus64(v);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double t = block_sum<4>(s[k], sh);
        if (threadIdx.x == 0) slots[(size_t)k * nb + blockIdx.x] = t;
    }
}
template <typename T>
__global__ __launch_bounds__(256) void disc_absdiff_partials_kernel(const T* a, const T* b, int64_t n, int64_t per, double* slots) {
    __shared__ double sh[4];
    const int64_t e0 = (int64_t)blockIdx.x * per, e1 = e0 + per < n ? e0 + per : n;
    double s = 0.0;
    for (int64_t i = e0 + threadIdx.x; i < e1; i += 256) s += fabs((double)(float)a[i] - (double)(float)b[i]);
    s = block_sum<4>(s, sh);
    if (threadIdx.x == 0) slots[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void disc_loss_finish_kernel(const double* slots, int nbl, double nl, int nbf, double nf, double* out) {
    __shared__ double sh[4];
    for (int k = 0; k < 5 && nbl > 0; ++k) {
        const double t = slot_sum<256>(slots + (size_t)k * nbl, nbl, sh);
        if (threadIdx.x == 0) out[k] = t / nl;
    }
    if (nbf > 0) {
        const double t = slot_sum<256>(slots + (size_t)5 * nbl, nbf, sh);
        if (threadIdx.x == 0) out[5] = t / nf;
    }
}

inline int64_t loss_blocks(int64_t n, int64_t* per) {
    if (n <= 0) { *per = 0; return 0; }
    int64_t nb = (n + DISC_LOSS_ITEMS - 1) / DISC_LOSS_ITEMS;
    if (nb > DISC_LOSS_MAX_BLOCKS) nb = DISC_LOSS_MAX_BLOCKS;
    *per = (n + nb - 1) / nb;
    return (n + *per - 1) / *per;
}

}  // namespace

extern "C" int mebt_op_disc_bn_partials(int32_t dtype, const void* x, int64_t M, int32_t C, void* slots, int64_t slots_bytes, mebt_stream_t stream) {
    const char* who = "disc_bn_partials";
    if (!x) return fail(MEBT_EINVAL, who, "null pointer");
    if (int rc = check_dtype(who, dtype)) return rc;
    if (M < 1 || C < 1) return fail(MEBT_ESHAPE, who, "bad shape");
    const int64_t n_slots = (M + MEBT_DISC_BN_ROWS - 1) / MEBT_DISC_BN_ROWS;
    if (int rc = check_scratch(who, slots, slots_bytes, (int64_t)16 * C * n_slots, n_slots)) return rc;
    with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(disc_bn_partials_kernel<T>, dim3((unsigned)n_slots), dim3(256), 0, S(stream), reinterpret_cast<const T*>(x), (long)M, C,
                           reinterpret_cast<double*>(slots), (long)n_slots);
    });
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int mebt_op_disc_bn_finish(const void* slots, int64_t n_slots, int32_t C, int64_t count, float* stats, float* running_mean,
                                      float* running_var, int64_t* num_batches_tracked, int32_t update, mebt_stream_t stream) {
    const char* who = "disc_bn_finish";
    if (!slots || !stats || (update && (!running_mean || !running_var))) return fail(MEBT_EINVAL, who, "null pointer");
    if (reinterpret_cast<uintptr_t>(slots) & 7) return fail(MEBT_EINVAL, who, "slots must be 8-byte aligned");
    if (n_slots < 1 || n_slots > 0x7FFFFFFFll || C < 1 || count < 1) return fail(MEBT_ESHAPE, who, "bad shape");
    if (count < 2) return fail(MEBT_ESHAPE, who, "expected more than 1 value per channel when training");
    hipLaunchKernelGGL(disc_bn_finish_kernel, dim3((unsigned)C), dim3(256), 0, S(stream), reinterpret_cast<const double*>(slots), (long)n_slots, C,
                       (double)count, stats, running_mean, running_var, num_batches_tracked, (int)update);
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}

extern "C" int64_t mebt_disc_losses_scratch_bytes(int64_t n_logits, int64_t n_feat) {
    int64_t per;
    return 8 * (5 * loss_blocks(n_logits, &per) + loss_blocks(n_feat, &per));
}

extern "C" int mebt_op_disc_losses(int32_t dtype, const void* logits, int64_t n_logits, const void* feat_a, const void* feat_b, int64_t n_feat,
                                   double* out, void* scratch, int64_t scratch_bytes, mebt_stream_t stream) {
    const char* who = "disc_losses";
    if (int rc = check_dtype(who, dtype)) return rc;
    if (!out || (n_logits > 0 && !logits) || (n_feat > 0 && (!feat_a || !feat_b))) return fail(MEBT_EINVAL, who, "null pointer");
    if (n_logits < 0 || n_feat < 0 || (n_logits == 0 && n_feat == 0)) return fail(MEBT_ESHAPE, who, "nothing to reduce");
    int64_t perl, perf;
    const int64_t nbl = loss_blocks(n_logits, &perl), nbf = loss_blocks(n_feat, &perf);
    if (int rc = check_scratch(who, scratch, scratch_bytes, 8 * (5 * nbl + nbf), nbl + nbf)) return rc;
    double* slots = reinterpret_cast<double*>(scratch);
    with_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        if (nbl) hipLaunchKernelGGL(disc_logit_partials_kernel<T>, dim3((unsigned)nbl), dim3(256), 0, S(stream), reinterpret_cast<const T*>(logits),
                                    n_logits, perl, slots, (int)nbl);
        if (nbf) hipLaunchKernelGGL(disc_absdiff_partials_kernel<T>, dim3((unsigned)nbf), dim3(256), 0, S(stream), reinterpret_cast<const T*>(feat_a),
                                    reinterpret_cast<const T*>(feat_b), n_feat, perf, slots + 5 * nbl);
    });
    hipLaunchKernelGGL(disc_loss_finish_kernel, dim3(1), dim3(256), 0, S(stream), slots, (int)nbl, (double)n_logits, (int)nbf, (double)n_feat, out);
    MEBT_HIP_CHECK(hipGetLastError());
    return MEBT_OK;
}
