// mpx_fire.h -- SqueezeNet 1.1: the head's global average pool, written as the fp32 logits K4b reads.
//
// (The Fire module itself needs no kernel of its own: squeeze, expand1x1 and expand3x3 are MFMA convs, and the channel concatenation of the
// two expand outputs is the SLICE form of conv_f16x3_kernel, mpx_conv.h -- each conv writes its half of the pixel rows of one buffer.)
#pragma once
#include "mpx_conv.h"

namespace mpx {

// ------------------------------------------------------------------------------------------
// Global average pool [B][hw][c] split planes -> fp32 [B][out_pitch]: torchvision's squeezenet ends in Conv2d(512, 1000, 1) + ReLU +
// AdaptiveAvgPool2d((1, 1)), so the pooled values ARE the logits and go straight to the softmax (K4b) without a re-split.
// One thread = 8 channels of one image, as global_avgpool_kernel.  The hw values hi + lo are summed in fp64: every value is a multiple of
// 2^-24 (fp16's subnormal step) below 2^16, so the sum is EXACT in any order, and the logit is the exact mean rounded twice (the fp64
// division, then the conversion to fp32).  A single fp32 accumulator was not good enough here: with logits near 18 the partial sums reach
// 3000, where an fp32 step is 2.4e-4, and 169 such roundings put the mean 1e-5 off -- more than four times what the fp32 CPU loop, whose
// sum is a tree, is from fp64.  The loads of four pixels are issued before their four adds: the map is 169 pixels deep and a thread has
// nothing else to hide the latency with.
// A kernel of its own, not an instantiation of global_avgpool_kernel<LOAD> (mpx_kernels.h): its sums are fp64 and its output is fp32.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void global_avgpool_logits_kernel(const half_t* __restrict__ in_hi,
                                                                     const half_t* __restrict__ in_lo,
                                                                     float* __restrict__ out, int B, int hw, int c,
                                                                     int out_pitch) {
    const int cg = c / 8;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= B * cg) return;
    const int g = t % cg, n = t / cg;
    const half_t* ph = in_hi + (size_t)n * hw * c + g * 8;
    const half_t* pl = in_lo + (size_t)n * hw * c + g * 8;
    double sum[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sum[j] = 0.0;
    int i = 0;
    for (; i + 4 <= hw; i += 4) {
        h8 vh[4], vl[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            vh[u] = *(const h8*)(ph + (size_t)(i + u) * c);
            vl[u] = *(const h8*)(pl + (size_t)(i + u) * c);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 8; ++j) sum[j] += (double)((float)vh[u][j] + (float)vl[u][j]);
    }
    for (; i < hw; ++i) {
        const h8 vh = *(const h8*)(ph + (size_t)i * c);
        const h8 vl = *(const h8*)(pl + (size_t)i * c);
#pragma unroll
        for (int j = 0; j < 8; ++j) sum[j] += (double)((float)vh[j] + (float)vl[j]);
    }
    const double denom = (double)hw;
    float* po = out + (size_t)n * out_pitch + g * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) po[j] = (float)(sum[j] / denom);
}

}  // namespace mpx
