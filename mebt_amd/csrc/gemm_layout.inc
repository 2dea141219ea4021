// One operand layout of the bf16 GEMM family: the kernel tables of that layout, each instantiation listed once (dispatch, tuning and
// the LDS attributes are in gemm.hip).  Included by gemm_kk.hip / gemm_kr.hip / gemm_rr.hip / gemm_rk.hip with MEBT_GEMM_AK /
// MEBT_GEMM_BK / MEBT_GEMM_TAG set; MEBT_GEMM_PAIR adds the pair kernels, MEBT_GEMM_GROUPED the grouped weight gradients.
#include "gemm_kernels.h"
#define MEBT_CAT2(a, b) a##b
#define MEBT_CAT(a, b) MEBT_CAT2(a, b)

namespace {
constexpr bool AK = MEBT_GEMM_AK, BKC = MEBT_GEMM_BK;
#define RING_LDS(TM, TN, R) ((R) * ((TM) + (TN)) * BK * 2)
#define REG(TM, TN) {GemmVariant::reg, TM, TN, 0, 256, RING_LDS(TM, TN, 2), (const void*)&gemm_bf16_kernel<AK, BKC, TM, TN>}
#define DMA(TM, TN, R) {GemmVariant::dma, TM, TN, R, 256, RING_LDS(TM, TN, R), (const void*)&gemm_bf16_dma_kernel<AK, BKC, TM, TN, R>}
#define PIPE(TM, TN, R) {GemmVariant::pipe, TM, TN, R, 256, RING_LDS(TM, TN, R), (const void*)&gemm_bf16_pipe_kernel<AK, BKC, TM, TN, R>}
#define KS2(TM, TN, R) {GemmVariant::ks2, TM, TN, R, 512, ks2_lds(TM, TN, R), (const void*)&gemm_bf16_dma_ks2_kernel<AK, BKC, TM, TN, R>}
#define PAIR(TM, TN, R) {GemmVariant::dma, TM, TN, R, 256, RING_LDS(TM, TN, R), (const void*)&gemm_pair_kernel<AK, BKC, TM, TN, R>}

// Tiles in the order the tuner times them (the first of equal times wins).  Rings: LDS-DMA 2-4 within 128 KiB, plus 5 (160 KiB) and the
// register-staged reference for the four square-ish tiles; pipelined 2-4 within 160 KiB; two pipelines 2-3 (96 x 128 ring 3 does not fit).
const GemmKernel single[] = {
    DMA(192, 128, 2), DMA(192, 128, 3), PIPE(192, 128, 2), PIPE(192, 128, 3), PIPE(192, 128, 4),
    REG(128, 128), DMA(128, 128, 2), DMA(128, 128, 3), DMA(128, 128, 4), DMA(128, 128, 5), PIPE(128, 128, 2), PIPE(128, 128, 3), PIPE(128, 128, 4),
    DMA(96, 128, 2), DMA(96, 128, 3), DMA(96, 128, 4), PIPE(96, 128, 2), PIPE(96, 128, 3), PIPE(96, 128, 4), KS2(96, 128, 2), KS2(96, 128, 3),
    REG(128, 64), DMA(128, 64, 2), DMA(128, 64, 3), DMA(128, 64, 4), DMA(128, 64, 5), PIPE(128, 64, 2), PIPE(128, 64, 3), PIPE(128, 64, 4),
    KS2(128, 64, 2), KS2(128, 64, 3),
    REG(64, 128), DMA(64, 128, 2), DMA(64, 128, 3), DMA(64, 128, 4), DMA(64, 128, 5), PIPE(64, 128, 2), PIPE(64, 128, 3), PIPE(64, 128, 4),
    KS2(64, 128, 2), KS2(64, 128, 3),
    DMA(96, 64, 2), DMA(96, 64, 3), DMA(96, 64, 4), PIPE(96, 64, 2), PIPE(96, 64, 3), PIPE(96, 64, 4), KS2(96, 64, 2), KS2(96, 64, 3),
    REG(64, 64), DMA(64, 64, 2), DMA(64, 64, 3), DMA(64, 64, 4), DMA(64, 64, 5), PIPE(64, 64, 2), PIPE(64, 64, 3), PIPE(64, 64, 4),
    KS2(64, 64, 2), KS2(64, 64, 3),
    {GemmVariant::w8, 256, 256, 2, 512, RING_LDS(256, 256, 2), (const void*)&gemm_bf16_w8_kernel<AK, BKC, 2>},
#if MEBT_GEMM_AK    // the staggered groups read A KC only
    {GemmVariant::pp, 256, 256, 0, 512, 8 * 128 * BK * 2 + 8 * 4096, (const void*)&gemm_bf16_pp_kernel<BKC>},
#endif
};
#ifdef MEBT_GEMM_PAIR
// tile-major, rings ascending: the pair tuner's candidate order (LDS-DMA rings within 128 KiB)
const GemmKernel pair[] = {
    PAIR(192, 128, 2), PAIR(192, 128, 3), PAIR(128, 128, 2), PAIR(128, 128, 3), PAIR(128, 128, 4), PAIR(96, 128, 2), PAIR(96, 128, 3), PAIR(96, 128, 4),
    PAIR(128, 64, 2), PAIR(128, 64, 3), PAIR(128, 64, 4), PAIR(64, 128, 2), PAIR(64, 128, 3), PAIR(64, 128, 4), PAIR(96, 64, 2), PAIR(96, 64, 3),
    PAIR(96, 64, 4), PAIR(64, 64, 2), PAIR(64, 64, 3), PAIR(64, 64, 4),
};
#endif
#ifdef MEBT_GEMM_GROUPED
#define GROUPED(TM, TN, R) {GemmVariant::dma, TM, TN, R, 256, RING_LDS(TM, TN, R), (const void*)&wgrad_grouped_kernel<TM, TN, R>}
// tile-major, rings ascending: the grouped tuner's candidate order.  256 x 128 is eight waves, ring 2 or 3 (4 x 48 KiB does not fit).
const GemmKernel grouped[] = {
    {GemmVariant::dma, 256, 128, 2, 512, RING_LDS(256, 128, 2), (const void*)&wgrad_grouped_kernel<256, 128, 2, 8>},
    {GemmVariant::dma, 256, 128, 3, 512, RING_LDS(256, 128, 3), (const void*)&wgrad_grouped_kernel<256, 128, 3, 8>},
    GROUPED(128, 128, 2), GROUPED(128, 128, 3), GROUPED(128, 128, 4), GROUPED(128, 64, 2), GROUPED(128, 64, 3), GROUPED(128, 64, 4),
    GROUPED(64, 128, 2), GROUPED(64, 128, 3), GROUPED(64, 128, 4), GROUPED(64, 64, 2), GROUPED(64, 64, 3), GROUPED(64, 64, 4),
};
#endif
template <int N> constexpr GemmTable table_of(const GemmKernel (&k)[N]) { return {k, N}; }
}  // namespace

GemmTables MEBT_CAT(mebt_gemm_tables_, MEBT_GEMM_TAG)() {
    GemmTables t = {table_of(single), {nullptr, 0}, {nullptr, 0}};
#ifdef MEBT_GEMM_PAIR
    t.pair = table_of(pair);
#endif
#ifdef MEBT_GEMM_GROUPED
    t.grouped = table_of(grouped);
#endif
    return t;
}
