// mpx_dw.h -- MobileNetV2's element-wise kernels on split-fp16 NHWC planes, gfx950: the depthwise 3x3 conv + BatchNorm + ReLU6 and the
// global average pool that clamps at 6 as it loads.
//
// ReLU6 and the MFMA convs.  The conv kernels' epilogues know ReLU only.  relu6(x) = min(relu(x), 6), so an MFMA conv that torchvision
// follows with ReLU6 runs with its ReLU epilogue and its CONSUMER takes min(x, 6) as it loads: every such conv of MobileNetV2 is read
// either by a depthwise layer (the stem, every expand conv) or by the global average pool (features.18).  Same arithmetic: the value
// the producer stored is relu(.) rounded to hi + lo, min(., 6) of it is exact, and 6 itself is a split-fp16 number.
#pragma once
#include "mpx_conv.h"

namespace mpx {

// ------------------------------------------------------------------------------------------
// Depthwise 3x3 conv (pad 1, stride 1 or 2) + BatchNorm + ReLU6 on planes [B][hin][hin][pitch] -> [B][ho][ho][pitch],
// ho = (hin - 1) / stride + 1.  One thread = 8 channels of one output pixel: per tap one 16-byte load per plane, hi + lo merged exactly
// in fp32 (and, with clamp_in, min(x, 6): the ReLU6 of the producing MFMA conv), then
//     acc = 0;  for ky in 0..2, kx in 0..2 (row-major):  acc = fma(w[ky * 3 + kx][c], x[iy][ix][c], acc)      one rounding per tap
// with the taps outside the map left out (they would add w * 0, which changes nothing), then fl(fl(s * acc) + t), min(max(., 0), 6),
// the re-split and one 16-byte store per plane.  w: fp32 tap-major [9][pitch]; s, t: fp32 [pitch] (BatchNorm scale and shift, computed
// in double and rounded once on the host).  Channels of the pitch beyond the layer's own carry zero weights, scale and shift, so they
// are written as exact zeros.  Consecutive lanes take consecutive 16-byte units of a pixel; the grid is capped (host: 8 blocks per CU)
// and strides over the rest, advancing (pixel, unit) by a fixed step without a division per round; offsets are 64-bit.  No atomics, no
// scratch, no LDS.
// ------------------------------------------------------------------------------------------
struct DwParams {
    const half_t* x_hi;
    const half_t* x_lo;
    half_t* y_hi;
    half_t* y_lo;
    const float* w;          // [9][pitch]
    const float* scale;      // [pitch]
    const float* shift;
    long long npix;          // B * ho * ho output pixels
    int hin, ho, pitch, stride, clamp_in;
};

__global__ __launch_bounds__(256) void dwconv3x3_bn_relu6_kernel(const DwParams p) {
    const unsigned cg = (unsigned)p.pitch >> 3;                     // units per pixel
    const unsigned step = gridDim.x * 256u;                         // <= 2^20 units: 32-bit divisions, once
    const unsigned u0 = blockIdx.x * 256u + threadIdx.x;
    const unsigned dpix = step / cg, dk = step % cg;
    long long pix = u0 / cg;
    unsigned k = u0 % cg;
    const long long howo = (long long)p.ho * p.ho;
    while (pix < p.npix) {
        const int c = (int)(k << 3);
        const long long n = pix / howo;
        const int rem = (int)(pix - n * howo);
        const int oy = rem / p.ho, ox = rem - oy * p.ho;
        const int iy0 = oy * p.stride - 1, ix0 = ox * p.stride - 1;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = iy0 + ky;
            if ((unsigned)iy >= (unsigned)p.hin) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ix0 + kx;
                if ((unsigned)ix >= (unsigned)p.hin) continue;
                const size_t at = (((size_t)n * p.hin + iy) * p.hin + ix) * p.pitch + c;
                const h8 vh = *(const h8*)(p.x_hi + at);
                const h8 vl = *(const h8*)(p.x_lo + at);
                const float* wt = p.w + (size_t)(ky * 3 + kx) * p.pitch + c;
                const f4 w0 = *(const f4*)wt, w1 = *(const f4*)(wt + 4);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float x = (float)vh[j] + (float)vl[j];
                    if (p.clamp_in) x = fminf(x, 6.f);
                    acc[j] = __fmaf_rn(j < 4 ? w0[j & 3] : w1[j & 3], x, acc[j]);
                }
            }
        }
        const f4 s0 = *(const f4*)(p.scale + c), s1 = *(const f4*)(p.scale + c + 4);
        const f4 t0 = *(const f4*)(p.shift + c), t1 = *(const f4*)(p.shift + c + 4);
        h8 oh, ol;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float s = j < 4 ? s0[j & 3] : s1[j & 3], t = j < 4 ? t0[j & 3] : t1[j & 3];
            const float v = fminf(fmaxf(__fadd_rn(__fmul_rn(s, acc[j]), t), 0.f), 6.f);
            half_t hi, lo;
            split_f32(v, hi, lo);
            oh[j] = hi;
            ol[j] = lo;
        }
        const size_t at_y = (size_t)pix * p.pitch + c;
        *(h8*)(p.y_hi + at_y) = oh;
        *(h8*)(p.y_lo + at_y) = ol;
        pix += dpix;
        k += dk;
        if (k >= cg) { k -= cg; ++pix; }
    }
}

// ------------------------------------------------------------------------------------------
// Global average pool [B][hw][c] -> [B][c] of min(x, 6): global_avgpool_kernel with the ReLU6 clamp of the producing MFMA conv
// (features.18) taken on load.  One thread = 8 channels of one image; the hw values are summed in pixel order in fp32 and divided by hw.
// A kernel of its own: global_avgpool_kernel stays as it is.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void global_avgpool_clamp6_kernel(const half_t* __restrict__ in_hi,
                                                                     const half_t* __restrict__ in_lo,
                                                                     half_t* __restrict__ out_hi,
                                                                     half_t* __restrict__ out_lo, int B, int hw,
                                                                     int c) {
    const int cg = c / 8;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= B * cg) return;
    const int g = t % cg, n = t / cg;
    float sum[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sum[j] = 0.f;
    for (int i = 0; i < hw; ++i) {
        const size_t o = ((size_t)n * hw + i) * c + g * 8;
        const h8 vh = *(const h8*)(in_hi + o);
        const h8 vl = *(const h8*)(in_lo + o);
#pragma unroll
        for (int j = 0; j < 8; ++j) sum[j] += fminf((float)vh[j] + (float)vl[j], 6.f);
    }
    h8 oh, ol;
    const float denom = (float)hw;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        half_t hi, lo;
        split_f32(__fdiv_rn(sum[j], denom), hi, lo);
        oh[j] = hi;
        ol[j] = lo;
    }
    const size_t o = (size_t)n * c + g * 8;
    *(h8*)(out_hi + o) = oh;
    *(h8*)(out_lo + o) = ol;
}

}  // namespace mpx
