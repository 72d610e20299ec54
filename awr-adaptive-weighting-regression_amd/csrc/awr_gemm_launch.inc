// Run-time flags -> compile-time variants of the LDS-DMA GEMM (conv_gemm_dma_kernel), one workgroup-tile shape per translation unit:
// csrc/awr_gemm_t<TM><TN>.hip includes this file and explicitly instantiates launch_dma_tile<TM, TN>; csrc/awr_conv.hip only declares it.
#pragma once
#include "awr_conv_kernels.inc"
#include "awr_conv_modes.h"

namespace awr {
// ---- dispatch of the LDS-DMA GEMM instantiations (run-time flags -> compile-time variants) ----
template <int TM, int TN, int KB, int NBUF, int AFF>
void launch_dma_em(const awr_conv_args* a, dim3 grid, hipStream_t st, bool epre, int em) {
    // Accumulator orientation (round 5 study, profiles/r05_epilogue_orientation.txt): 0 = mfma(activation fragment, weight fragment), a lane owns 16 PIXELS
    // of one channel -- the shipped form.  Builds with -DAWR_EPI_STUDY also carry 1 = operand roles swapped (a lane owns 16 CHANNELS of one pixel: the bounce
    // tile written as four 16-byte rows instead of sixteen 4-byte columns) and 2 = 1 with the reduction-free epilogue stored straight from the accumulators
    // (no LDS): bit-identical results, 1 is not faster anywhere, 2 is 6-9 % SLOWER on the store-heavy 1x1 launches (32-byte runs per pixel per store
    // instruction instead of whole 128-byte lines).  $AWR_EPI selects.
#ifdef AWR_EPI_STUDY
    static const int sw = env_int("AWR_EPI", 0);
#define AWR_DMA_SW(EPRE, EM, DUAL, ACCB)                                                                                                                   \
    do {                                                                                                                                                   \
        if (sw == 0) hipLaunchKernelGGL((conv_gemm_dma_kernel<TM, TN, KB, NBUF, AFF, EPRE, EM, DUAL, ACCB, 0>), grid, dim3(256), 0, st, *a);               \
        else if (sw == 1 || EM != 1) hipLaunchKernelGGL((conv_gemm_dma_kernel<TM, TN, KB, NBUF, AFF, EPRE, EM, DUAL, ACCB, 1>), grid, dim3(256), 0, st, *a); \
        else hipLaunchKernelGGL((conv_gemm_dma_kernel<TM, TN, KB, NBUF, AFF, EPRE, EM, DUAL, ACCB, (EM == 1 ? 2 : 1)>), grid, dim3(256), 0, st, *a);      \
    } while (0)
#else
#define AWR_DMA_SW(EPRE, EM, DUAL, ACCB) hipLaunchKernelGGL((conv_gemm_dma_kernel<TM, TN, KB, NBUF, AFF, EPRE, EM, DUAL, ACCB, 0>), grid, dim3(256), 0, st, *a)
#endif
#define AWR_DMA_K(EPRE, EM, DUAL) AWR_DMA_SW(EPRE, EM, DUAL, false)
#define AWR_DMA_KB(EM) AWR_DMA_SW(false, EM, false, (KB == 16 && NBUF >= 2))
    const bool blocked = KB == 16 && NBUF >= 2 && a->accum == 1 && a->Cin * a->ph[0].ntaps > 256;      // (shorter K extents are one block anyway)
    // statistics from the accumulators (EM 5) where the stored value is accumulator + bias and every tile lies inside M: bit-identical outputs,
    // statistics 1.5x CLOSER to float64 than the row-layout form, isolated 1x1 launches with statistics +4-8 % (16x16 maps +20 %), Hourglass-1 step
    // -0.5 % (profiles/r05_fast_stats.txt).  The default since round 6 (AWR_FAST_STATS=0 / awr_debug_set_knob("fast_stats", 0): the row-layout form);
    // round 5 had parked it because the chaotic two-image ResNet18 fixture happened to land worse with the MORE accurate sums
    {
        const int64_t M = (int64_t)a->B * a->Hq * a->Wq;
#ifndef AWR_EPI_STUDY      // (the swapped-operand study forms keep the row-layout statistics)
        // (not the 128x128 tile with the masked input affine: 128 -> 131 registers would cost it its fourth wave)
        if (em == 2 && !a->res && !a->out_scale && !epre && M % (64 * TM) == 0 && !(TM == 2 && TN == 2 && AFF == 1) && g_knob_fast_stats) em = 5;
#endif
    }
    if constexpr (AFF == 2) {          // data gradients only: no statistics epilogue, no second tensor, no operand prefetch
        if (blocked) {
            if (em == 4) AWR_DMA_KB(4);
            else if (em == 3) AWR_DMA_KB(3);
            else AWR_DMA_KB(1);
        } else {
            if (em == 4) AWR_DMA_K(false, 4, false);
            else if (em == 3) AWR_DMA_K(false, 3, false);
            else AWR_DMA_K(false, 1, false);
        }
    } else if (a->in2) {               // conv3 + skip_layer: K = [in | in2]; no operand prefetch (the launcher excludes it), no BNR epilogue
        if (blocked) {                 // (Hourglass conv3 + skip: K = 128 + 256)
            if (em == 5) AWR_DMA_SW(false, 5, true, (KB == 16 && NBUF >= 2));
            else if (em == 2) AWR_DMA_SW(false, 2, true, (KB == 16 && NBUF >= 2));
            else AWR_DMA_SW(false, 1, true, (KB == 16 && NBUF >= 2));
        } else {
            if (em == 5) AWR_DMA_K(false, 5, true);
            else if (em == 2) AWR_DMA_K(false, 2, true);
            else AWR_DMA_K(false, 1, true);
        }
    } else if (epre) {                 // short K loops (<= 256 terms: one accumulation block in either mode) whose epilogue reads exactly one operand tensor
        if (em == 3) AWR_DMA_K(true, 3, false);
        else if (em == 2) AWR_DMA_K(true, 2, false);
        else AWR_DMA_K(true, 1, false);
    } else if (blocked) {
        if (em == 4) AWR_DMA_KB(4);
        else if (em == 3) AWR_DMA_KB(3);
        else if (em == 5) AWR_DMA_KB(5);
        else if (em == 2) AWR_DMA_KB(2);
        else AWR_DMA_KB(1);
    } else {
        if (em == 4) AWR_DMA_K(false, 4, false);
        else if (em == 3) AWR_DMA_K(false, 3, false);
        else if (em == 5) AWR_DMA_K(false, 5, false);
        else if (em == 2) AWR_DMA_K(false, 2, false);
        else AWR_DMA_K(false, 1, false);
    }
#undef AWR_DMA_KB
#undef AWR_DMA_K
#undef AWR_DMA_SW
}
template <int TM, int TN>
void launch_dma_tile(const awr_conv_args* a, dim3 grid, hipStream_t st, int mode, int aff, bool epre, int em) {
#ifdef AWR_DMA_STUDY
    if (mode == 1 && aff < 2) { aff ? launch_dma_em<TM, TN, 32, 2, 1>(a, grid, st, epre, em) : launch_dma_em<TM, TN, 32, 2, 0>(a, grid, st, epre, em); return; }
    if (mode == 3 && aff < 2) { aff ? launch_dma_em<TM, TN, 32, 1, 1>(a, grid, st, epre, em) : launch_dma_em<TM, TN, 32, 1, 0>(a, grid, st, epre, em); return; }
#endif
    // (round-5 study, -DAWR_AFF_LDS_STUDY + AWR_AFF_LDS=1: the fused input affine as an in-LDS pass, AFF == 4 -- fewer registers, bit-identical, NOT faster:
    // profiles/r05_affine_lds_pass.txt)
#ifdef AWR_AFF_LDS_STUDY
    static const int aff_lds = env_int("AWR_AFF_LDS", 0);
    if (aff && aff != 2 && aff_lds) { launch_dma_em<TM, TN, 16, 2, 4>(a, grid, st, epre, em); return; }
#endif
    // deep pipeline (four stage buffers, three in flight) for launches of at most 384 workgroups (1.5 per CU) whose K loop is long enough to matter;
    // (ordered or, since round 6, blocked accumulation), no 128x128 tile (it never wins at that size), no un-materialised BatchNorm backward.  Measured (profiles/r05_deep_pipeline.txt):
    // isolated launches do not move, steps whose launches are ALL small do -- ResNet18 train batch 4 3.59 -> 3.01 ms, batch 16 5.04 -> 4.59 ms (a launch
    // that shares the CUs with the weight gradients of two side streams sees load latencies two buffers do not cover); with 512 the batch-64 steps
    // lose 1 % (layer4, the Hourglass 8x8 levels), with 384 they are unchanged.  AWR_DEEP=0: never (A/B hook), AWR_DEEP_MAX_WGS: the bound
    if constexpr (!(TM == 2 && TN == 2)) {
        const int deep_on = g_knob_deep;
        int minsteps = 1 << 30;
        for (int p = 0; p < a->nphase; ++p) minsteps = a->ph[p].ntaps * (a->Cin / 16) < minsteps ? a->ph[p].ntaps * (a->Cin / 16) : minsteps;
        static const int deep_wgs = env_int("AWR_DEEP_MAX_WGS", 384);
        // AWR_DEEP_1X1 (study hook, results unchanged): single-tap launches of ANY size take the deep form -- a 1x1 conv at 64x64 x 64 images streams
        // its whole A operand from HBM once (2-3.5 TB/s needed at MFMA speed) with one 4 KB stage per resident workgroup in flight
        bool single_tap = g_knob_deep_1x1 != 0;
        for (int p = 0; p < a->nphase && single_tap; ++p) single_tap = a->ph[p].ntaps == 1;
        if (deep_on && aff != 2 && ((int64_t)grid.x * grid.y <= deep_wgs || single_tap) && minsteps >= 8) {
            if (aff == 3) launch_dma_em<TM, TN, 16, 4, 3>(a, grid, st, epre, em);
            else if (aff == 1) launch_dma_em<TM, TN, 16, 4, 1>(a, grid, st, epre, em);
            else launch_dma_em<TM, TN, 16, 4, 0>(a, grid, st, epre, em);
            return;
        }
    }
    if (aff == 2) launch_dma_em<TM, TN, 16, 2, 2>(a, grid, st, epre, em);
    else if (aff == 3) launch_dma_em<TM, TN, 16, 2, 3>(a, grid, st, epre, em);
    else if (aff == 1) launch_dma_em<TM, TN, 16, 2, 1>(a, grid, st, epre, em);
    else launch_dma_em<TM, TN, 16, 2, 0>(a, grid, st, epre, em);
}
// A plain (or, with in2, two-tensor) 1x1 launch that also writes the 2x2 max-pool of its output (awr_conv_args.pool_out): the shipped stage shape only.
// The launcher has checked every condition of the form (conv_gemm_one).
template <int TM, int TN>
void launch_dma_pool_tile(const awr_conv_args* a, dim3 grid, hipStream_t st) {
    if (a->in2) hipLaunchKernelGGL((conv_gemm_dma_pool_kernel<TM, TN, true>), grid, dim3(256), 0, st, *a);
    else hipLaunchKernelGGL((conv_gemm_dma_pool_kernel<TM, TN, false>), grid, dim3(256), 0, st, *a);
}
}  // namespace awr
