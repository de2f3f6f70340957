// mpx_dw.h -- the depthwise conv + BatchNorm kernels on split-fp16 NHWC planes, gfx950: MobileNetV2's 3x3 + ReLU6, one thread per output
// pixel, and the run form, one thread per run of output pixels: k x k with an optional SiLU on either side, which serves ShuffleNetV2 (3x3,
// linear) and EfficientNet-B0 (3x3 / 5x5, SiLU).  (ConvNeXt's depthwise 7x7 + LayerNorm is mpx_cnext.h's.)
//
// ReLU6 and the MFMA convs.  The conv kernels' epilogues know ReLU only.  relu6(x) = min(relu(x), 6), so an MFMA conv that torchvision
// follows with ReLU6 runs with its ReLU epilogue and its CONSUMER takes min(x, 6) as it loads: every such conv of MobileNetV2 is read
// either by a depthwise layer (the stem, every expand conv) or by the global average pool (features.18).  Same arithmetic: the value
// the producer stored is relu(.) rounded to hi + lo, min(., 6) of it is exact, and 6 itself is a split-fp16 number.
//
// SiLU and the MFMA convs.  silu(x) = x * sigmoid(x) cannot be had from ReLU by a clamp on load.  So an MFMA conv that torchvision follows
// with SiLU (EfficientNet's stem, every expand conv, features.8) runs WITHOUT an activation and stores bn(conv(x)); its one CONSUMER takes
// silu(x) as it loads: a depthwise layer (act_in) or the SiLU global pool (mpx_kernels.h).  The depthwise layer applies its own SiLU in its
// epilogue (act_out), once per element.  No MFMA kernel, epilogue or tile changes.
#pragma once
#include "mpx_conv.h"

namespace mpx {

// ------------------------------------------------------------------------------------------
// Depthwise 3x3 conv (pad 1, stride 1 or 2) + BatchNorm + ReLU6 on planes [B][hin][hin][pitch] -> [B][ho][ho][pitch],
// ho = (hin - 1) / stride + 1.  One thread = 8 channels of one output pixel: per tap one 16-byte load per plane, hi + lo merged exactly
// in fp32 (and, with clamp_in, min(x, 6): the ReLU6 of the producing MFMA conv), then
//     acc = 0;  for ky in 0..2, kx in 0..2 (row-major):  acc = fma(w[ky * 3 + kx][c], x[iy][ix][c], acc)      one rounding per tap
// with the taps outside the map left out (they would add w * 0, which changes nothing), then fma(s, acc, t) -- ONE rounding: the
// __fmul_rn / __fadd_rn below are a plain * and + in this toolchain's headers and this kernel compiles under the default contract(fast),
// so the BatchNorm is eight v_fma_f32 that feed v_med3_f32 (the run form below rounds twice, under contract(off); the depthwise bound of
// tests/test_gpu_mobilenet.py covers both forms) --, min(max(., 0), 6),
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
    const float* w;          // [k * k][pitch]
    const float* scale;      // [pitch]
    const float* shift;
    long long npix;          // B * ho * ho output pixels
    int hin, ho, pitch, stride, clamp_in;
    long long rows;          // B * ho output rows               (the three fields the run form reads, behind the one-pixel form's)
    int act_in, act_out;     // SiLU on load / in the epilogue   (dwconv_bn_act_kernel<K, STRIDE, true> only)
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
// THE RUN FORM.  Depthwise K x K conv (K = 3 or 5, pad (K - 1) / 2, stride 1 or 2) + BatchNorm, with SiLU on the input (act_in) and on the
// output (act_out) when SILU: planes [B][hin][hin][pitch] -> [B][ho][ho][pitch], ho = (hin - 1) / STRIDE + 1.  Per output element, in fp32:
//     x = hi + lo (exact);  a = act_in ? silu(x) : x, once per LOADED element, not once per tap;
//     acc = 0;  for ky in 0..K-1, kx in 0..K-1 (row-major):  acc = fma(w[ky * K + kx][c], a[iy][ix][c], acc)   over the taps inside the map;
//     v = fl(fl(s * acc) + t) -- two roundings: the product and the sum are plain operators under `#pragma clang fp contract(off)` (the
//         __fmul_rn / __fadd_rn of this toolchain's headers are a plain * and + compiled under the default contract(fast), and were fused
//         into one fma when ShuffleNetV2's kernel used them);
//     act_out ? silu(v) : v;  the re-split;  one 16-byte store per plane.
// SILU = false is ShuffleNetV2's LINEAR layer (branch1.0 / branch2.3 with their BatchNorms; K = 3): it ignores act_in / act_out and
// carries no SiLU code -- negative results and results above 6 pass through unchanged.  SILU = true is EfficientNet-B0's layer, the two
// flags run-time values.
// w: fp32 tap-major [K * K][pitch]; s, t: fp32 [pitch].  Channels of the pitch beyond the layer's own -- the gaps of a two-half map
// (mpx_shuffle.h) included -- carry zero weights, scale and shift and come out as exact zeros (silu(0) = 0; their inputs are exact zeros
// wherever the engine produces them).
// One thread = 8 channels of a run of W output pixels along x (W = 4 at stride 1, 2 at stride 2), as maxpool3x3_clip_kernel (mpx_pool3c.h).
// Row by row it loads the run's NC = STRIDE * (W - 1) + K input columns once -- 18 loads per plane for four 3x3 stride-1 outputs where one
// thread per output pixel issues 36, 8 columns a row for four 5x5 outputs where it would load 20 -- and feeds every output its K taps of
// that row, kx ascending: each output still sees its taps in row-major order, one fma each, so the result has the bits of the one-pixel
// form.  A column outside the map is loaded at a clamped index (inside the planes) and its fma is not taken; a row outside the map is
// skipped.  Only one input row (NC x 8 values) is live at a time.  (DESIGN.md 16 has the times of both forms.)
// Units (n, oy, run, 8-channel group) are 64-bit, consecutive lanes take consecutive 16-byte groups of a pixel; the grid is capped by the
// host and strides over the rest.  Offsets are 64-bit.  No atomics, no scratch (every array is indexed by unrolled constants), no LDS.
// ------------------------------------------------------------------------------------------
template <int K, int STRIDE>
struct DwRun {
    static constexpr int W = STRIDE == 1 ? 4 : 2;       // output pixels per thread
    static constexpr int NC = STRIDE * (W - 1) + K;     // input columns under them
};

template <int K, int STRIDE, bool SILU>
__global__ __launch_bounds__(256) void dwconv_bn_act_kernel(const DwParams p) {
#pragma clang fp contract(off)
    constexpr int W = DwRun<K, STRIDE>::W, NC = DwRun<K, STRIDE>::NC, PAD = (K - 1) / 2;
    const long long cg = p.pitch >> 3;
    const int runs = (p.ho + W - 1) / W;
    const long long units = p.rows * runs * cg;
    const int last = p.hin - 1;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < units; t += (long long)gridDim.x * 256) {
        const long long g = t % cg;
        long long r = t / cg;
        const int run = (int)(r % runs);
        r /= runs;
        const int oy = (int)(r % p.ho);
        const long long n = r / p.ho;
        const int c = (int)g << 3;
        const int ox0 = run * W;
        const int iy0 = oy * STRIDE - PAD, ix0 = ox0 * STRIDE - PAD;
        float acc[W][8];
#pragma unroll
        for (int k = 0; k < W; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int iy = iy0 + ky;
            if ((unsigned)iy >= (unsigned)p.hin) continue;
            const size_t row = ((size_t)n * p.hin + iy) * p.hin * p.pitch + c;
            float xm[NC][8];
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                const size_t at = row + (size_t)min(max(ix0 + q, 0), last) * p.pitch;
                const h8 vh = *(const h8*)(p.x_hi + at);
                const h8 vl = *(const h8*)(p.x_lo + at);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float x = (float)vh[j] + (float)vl[j];
                    if constexpr (SILU) xm[q][j] = p.act_in ? silu_f32(x) : x;
                    else xm[q][j] = x;
                }
            }
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const float* wt = p.w + (size_t)(ky * K + kx) * p.pitch + c;
                const f4 w0 = *(const f4*)wt, w1 = *(const f4*)(wt + 4);
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    const bool in_map = (unsigned)(ix0 + STRIDE * k + kx) < (unsigned)p.hin;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float f = __fmaf_rn(j < 4 ? w0[j & 3] : w1[j & 3], xm[STRIDE * k + kx][j], acc[k][j]);
                        acc[k][j] = in_map ? f : acc[k][j];
                    }
                }
            }
        }
        const f4 s0 = *(const f4*)(p.scale + c), s1 = *(const f4*)(p.scale + c + 4);
        const f4 t0 = *(const f4*)(p.shift + c), t1 = *(const f4*)(p.shift + c + 4);
        const size_t out0 = (((size_t)n * p.ho + oy) * p.ho + ox0) * p.pitch + c;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            if (ox0 + k >= p.ho) break;         // the last run of a row may be short
            h8 oh, ol;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float s = j < 4 ? s0[j & 3] : s1[j & 3], sh = j < 4 ? t0[j & 3] : t1[j & 3];
                const float m = s * acc[k][j];          // plain operators, inside this block's contract(off): two roundings
                float v = m + sh;
                if constexpr (SILU) {
                    if (p.act_out) v = silu_f32(v);
                }
                half_t hi, lo;
                split_f32(v, hi, lo);
                oh[j] = hi;
                ol[j] = lo;
            }
            *(h8*)(p.y_hi + out0 + (size_t)k * p.pitch) = oh;
            *(h8*)(p.y_lo + out0 + (size_t)k * p.pitch) = ol;
        }
    }
}

}  // namespace mpx
