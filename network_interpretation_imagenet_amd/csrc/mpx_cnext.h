// mpx_cnext.h -- the kernels of a ConvNeXt block (torchvision's convnext_tiny / convnext_small) on split-fp16 NHWC planes, gfx950: the
// depthwise 7x7 conv + bias + LayerNorm over the channels of each pixel in one launch, the stand-alone LayerNorm over the channels of a
// pixel, and the global average pool with the LayerNorm of the head behind it.
//
// LayerNorm is the first normalisation here whose constants are statistics of the activations themselves: a pixel's C channels are spread
// over C / 8 threads, so the two sums (mean, centred squares) cross threads -- through the LDS, in ONE fixed order, so that a pixel's result
// depends on nothing but the pixel: not on the batch, not on where the image sits in it, not on the grid.
//
// THE ARITHMETIC, per pixel, in fp32, plain operators under contract(off) (one rounding per operator, fma only where it says fma):
//     part_g = ((((((v[8g] + v[8g+1]) + v[8g+2]) + ...) + v[8g+7])                       per 8-channel group g = 0 .. C/8 - 1
//     mean   = (((part_0 + part_1) + part_2) + ... + part_{C/8-1}) / (float)C            groups ascending, one IEEE division
//     d_c    = v_c - mean
//     sq_g   = (((d[8g] * d[8g]) + d[8g+1] * d[8g+1]) + ...) + d[8g+7] * d[8g+7]         products rounded, then added, channels ascending
//     var    = (((sq_0 + sq_1) + sq_2) + ... ) / (float)C                                two-pass: centred and biased, never E[v^2] - mean^2
//     rstd   = 1.0f / sqrtf(var + eps)                                                   IEEE square root and division
//     y_c    = ((d_c * rstd) * gamma_c) + beta_c
// then the split and one 16-byte store per plane.  v is never rounded to split-fp16 and never goes to HBM.
#pragma once
#include <cmath>

#include "mpx_conv.h"

namespace mpx {

// (The fourth kernel of the family, GELU in the epilogue of the generic MFMA conv kernel, lives with that kernel: mpx_conv.h, ConvGelu.)

constexpr int CN_NT = 256;              // threads of a workgroup of every kernel below

// Workgroup shape.  G = C / 8 threads hold a pixel (or a run of pixels): 12, 24, 48, 96 for C = 96, 192, 384, 768.  A workgroup of 256
// threads holds R = 256 / G whole SLOTS of G consecutive threads (thread t: slot t / G, group t % G), so a pixel's threads always sit in
// one workgroup; the 256 - R * G threads behind the last slot are idle (they reach every barrier and do nothing else):
//     C =  96: R = 21, 4 idle     C = 192: R = 10, 16 idle     C = 384: R = 5, 16 idle     C = 768: R = 2, 64 idle
// Any C that is a multiple of 8 up to 2048 works (G <= 256).
__host__ __device__ inline int cn_slots(int C) { return CN_NT / (C >> 3); }

// The LayerNorm statistics of the W pixels a slot holds.  v[k][j]: channel 8 g + j of pixel k, replaced by d = v - mean.  psum / psq:
// LDS, W * 256 floats each.  EVERY thread of the workgroup calls this (two barriers inside); `active` = the thread belongs to a slot that
// has work.  The two arrays alternate, so a barrier always lies between a slot's reads of one and the next iteration's writes to it.
template <int W>
__device__ __forceinline__ void cn_ln_stats(float (&v)[W][8], float (&rstd)[W], int slot, int g, int G, bool active, float fC, float eps,
                                            float* psum, float* psq) {
#pragma clang fp contract(off)
    if (active) {
#pragma unroll
        for (int k = 0; k < W; ++k) {
            float s = v[k][0];
#pragma unroll
            for (int j = 1; j < 8; ++j) s = s + v[k][j];
            psum[(slot * W + k) * G + g] = s;
        }
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const float* q = psum + (slot * W + k) * G;
            float s = q[0];
            for (int i = 1; i < G; ++i) s = s + q[i];
            const float mean = s / fC;
            float s2 = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = v[k][j] - mean;
                const float dd = d * d;
                v[k][j] = d;
                s2 = j == 0 ? dd : s2 + dd;
            }
            psq[(slot * W + k) * G + g] = s2;
        }
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const float* q = psq + (slot * W + k) * G;
            float s = q[0];
            for (int i = 1; i < G; ++i) s = s + q[i];
            const float var = s / fC;
            rstd[k] = 1.0f / sqrtf(var + eps);
        }
    }
}

// y = ((d * rstd) * gamma) + beta of 8 channels, split and stored at `at` of both planes
__device__ __forceinline__ void cn_ln_store(const float (&d)[8], float rstd, const f4& g0, const f4& g1, const f4& b0, const f4& b1, half_t* y_hi,
                                            half_t* y_lo, size_t at) {
#pragma clang fp contract(off)
    h8 oh, ol;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float n = d[j] * rstd;
        const float m = n * (j < 4 ? g0[j & 3] : g1[j & 3]);
        const float y = m + (j < 4 ? b0[j & 3] : b1[j & 3]);
        half_t hi, lo;
        split_f32(y, hi, lo);
        oh[j] = hi;
        ol[j] = lo;
    }
    *(h8*)(y_hi + at) = oh;
    *(h8*)(y_lo + at) = ol;
}

// ------------------------------------------------------------------------------------------
// 1. Depthwise 7x7 conv (pad 3, stride 1) + bias + LayerNorm over C: planes [B][H][H][C] -> [B][H][H][C], one launch.
//     acc_c = 0;  acc_c = fma(w[ky * 7 + kx][c], x[iy][ix][c], acc_c) over the taps inside the map, row-major;  v_c = acc_c + bias_c;
//     then the LayerNorm above.  x = hi + lo (exact).  w: fp32 tap-major [49][C]; bias, gamma, beta: fp32 [C].
// The depthwise part is the run form of dwconv_bn_act_kernel (mpx_dw.h): one thread = 8 channels of a run of W = 4 output pixels along
// x; row by row it loads the run's 10 input columns once and feeds every output its 7 taps of that row, kx ascending.  A column outside
// the map is loaded at a clamped index and its fma is not taken; a row outside the map is skipped.  A unit is (image, output row, run);
// the G threads of a slot hold one unit, a workgroup R units at a time.  The grid is capped by the host; a workgroup strides over the
// units with a trip count that is the same for all of its threads, so every thread reaches every barrier, the threads of a slot without a
// unit and the idle ones included.  The pixels of a short last run (H % 4 != 0) are computed from clamped loads and not stored.
// Offsets are 64-bit.  No atomics, no scratch; 8 KB of static LDS.
// ------------------------------------------------------------------------------------------
struct CnDwLnParams {
    const half_t* x_hi;
    const half_t* x_lo;
    half_t* y_hi;
    half_t* y_lo;
    const float* w;          // [49][C]
    const float* bias;       // [C]
    const float* gamma;      // [C]
    const float* beta;       // [C]
    long long units;         // B * H * runs
    int H, C;
    float eps;
};

constexpr int CN_DW_K = 7, CN_DW_W = 4, CN_DW_NC = CN_DW_W - 1 + CN_DW_K;

__global__ __launch_bounds__(CN_NT, 2) void dwconv7x7_ln_kernel(const CnDwLnParams p) {
#pragma clang fp contract(off)
    constexpr int K = CN_DW_K, W = CN_DW_W, NC = CN_DW_NC, PAD = 3;
    __shared__ float psum[W * CN_NT], psq[W * CN_NT];
    const int G = p.C >> 3, R = CN_NT / G;
    const int slot = threadIdx.x / G, g = threadIdx.x - slot * G, c = g << 3;
    const int runs = (p.H + W - 1) / W, last = p.H - 1;
    const float fC = (float)p.C;
    for (long long base = (long long)blockIdx.x * R; base < p.units; base += (long long)gridDim.x * R) {
        const long long u = base + slot;
        const bool active = slot < R && u < p.units;
        float v[W][8], rstd[W];
        int oy = 0, ox0 = 0;
        long long n = 0;
        if (active) {
            const int run = (int)(u % runs);
            const long long r = u / runs;
            oy = (int)(r % p.H);
            n = r / p.H;
            ox0 = run * W;
            const int iy0 = oy - PAD, ix0 = ox0 - PAD;
#pragma unroll
            for (int k = 0; k < W; ++k)
#pragma unroll
                for (int j = 0; j < 8; ++j) v[k][j] = 0.f;
            // (not unrolled: unrolled, hipcc hoists the loads of all seven rows -- 140 x 16 bytes -- and the kernel needs 346 registers, one
            // wave per SIMD; as a loop it needs 231, two waves per SIMD, without scratch.  A bound of three waves per SIMD -- 168
            // registers -- spills 148 bytes per lane and was not kept.)
#pragma unroll 1
            for (int ky = 0; ky < K; ++ky) {
                const int iy = iy0 + ky;
                if ((unsigned)iy >= (unsigned)p.H) continue;
                const size_t row = ((size_t)n * p.H + iy) * p.H * p.C + c;
                float xm[NC][8];
#pragma unroll
                for (int q = 0; q < NC; ++q) {
                    const size_t at = row + (size_t)min(max(ix0 + q, 0), last) * p.C;
                    const h8 vh = *(const h8*)(p.x_hi + at);
                    const h8 vl = *(const h8*)(p.x_lo + at);
#pragma unroll
                    for (int j = 0; j < 8; ++j) xm[q][j] = (float)vh[j] + (float)vl[j];
                }
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const float* wt = p.w + (size_t)(ky * K + kx) * p.C + c;
                    const f4 w0 = *(const f4*)wt, w1 = *(const f4*)(wt + 4);
#pragma unroll
                    for (int k = 0; k < W; ++k) {
                        const bool in_map = (unsigned)(ix0 + k + kx) < (unsigned)p.H;
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float f = __fmaf_rn(j < 4 ? w0[j & 3] : w1[j & 3], xm[k + kx][j], v[k][j]);
                            v[k][j] = in_map ? f : v[k][j];
                        }
                    }
                }
            }
            const f4 c0 = *(const f4*)(p.bias + c), c1 = *(const f4*)(p.bias + c + 4);
#pragma unroll
            for (int k = 0; k < W; ++k)
#pragma unroll
                for (int j = 0; j < 8; ++j) v[k][j] = v[k][j] + (j < 4 ? c0[j & 3] : c1[j & 3]);
        }
        cn_ln_stats<W>(v, rstd, slot, g, G, active, fC, p.eps, psum, psq);
        if (active) {
            const f4 g0 = *(const f4*)(p.gamma + c), g1 = *(const f4*)(p.gamma + c + 4);
            const f4 b0 = *(const f4*)(p.beta + c), b1 = *(const f4*)(p.beta + c + 4);
            const size_t out0 = (((size_t)n * p.H + oy) * p.H + ox0) * p.C + c;
#pragma unroll
            for (int k = 0; k < W; ++k) {
                if (ox0 + k >= p.H) break;          // the last run of a row may be short
                cn_ln_store(v[k], rstd[k], g0, g1, b0, b1, p.y_hi, p.y_lo, out0 + (size_t)k * p.C);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// 2. Stand-alone LayerNorm over the C channels of each pixel: planes [rows * in_stride][C] -> [rows][C], v = hi + lo (exact), the arithmetic
// above.  Output row r is the LayerNorm of input row r * in_stride: 1 for a map or a token sequence (mpx_layernorm_c), T for a ViT's
// encoder.ln on the class-token row of each image (mpx_layernorm_rows).
// One thread = 8 channels of one pixel, a slot = one pixel, a workgroup R pixels at a time; grid capped by the host, uniform trip count,
// every thread at every barrier.  Offsets are 64-bit.  No atomics, no scratch; 2 KB of static LDS.
// ------------------------------------------------------------------------------------------
struct CnLnParams {
    const half_t* x_hi;
    const half_t* x_lo;
    half_t* y_hi;
    half_t* y_lo;
    const float* gamma;      // [C]
    const float* beta;       // [C]
    long long rows;
    long long in_stride;     // rows of the input planes between two rows that are normalised
    int C;
    float eps;
};

__global__ __launch_bounds__(CN_NT) void layernorm_c_kernel(const CnLnParams p) {
    __shared__ float psum[CN_NT], psq[CN_NT];
    const int G = p.C >> 3, R = CN_NT / G;
    const int slot = threadIdx.x / G, g = threadIdx.x - slot * G, c = g << 3;
    const float fC = (float)p.C;
    for (long long base = (long long)blockIdx.x * R; base < p.rows; base += (long long)gridDim.x * R) {
        const long long u = base + slot;
        const bool active = slot < R && u < p.rows;
        float v[1][8], rstd[1];
        if (active) {
            const size_t at = (size_t)u * p.in_stride * p.C + c;
            const h8 vh = *(const h8*)(p.x_hi + at);
            const h8 vl = *(const h8*)(p.x_lo + at);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[0][j] = (float)vh[j] + (float)vl[j];
        }
        cn_ln_stats<1>(v, rstd, slot, g, G, active, fC, p.eps, psum, psq);
        if (active) {
            const f4 g0 = *(const f4*)(p.gamma + c), g1 = *(const f4*)(p.gamma + c + 4);
            const f4 b0 = *(const f4*)(p.beta + c), b1 = *(const f4*)(p.beta + c + 4);
            cn_ln_store(v[0], rstd[0], g0, g1, b0, b1, p.y_hi, p.y_lo, (size_t)u * p.C + c);
        }
    }
}

// ------------------------------------------------------------------------------------------
// 3. The head: global average pool [B][hw][C] -> the LayerNorm over C of the pooled row -> split planes [B][C].  v_c = (the hw values
// hi + lo of channel c summed in pixel order in fp32) / (float)hw, global_avgpool_kernel's order, NOT re-split in between; then the
// arithmetic above.  A slot = one image: one thread walks the hw pixels of its 8 channels.  Same workgroup shape, barriers and grid rule.
// ------------------------------------------------------------------------------------------
struct CnPoolLnParams {
    const half_t* x_hi;
    const half_t* x_lo;
    half_t* y_hi;
    half_t* y_lo;
    const float* gamma;
    const float* beta;
    int B, hw, C;
    float eps;
};

__global__ __launch_bounds__(CN_NT) void global_avgpool_ln_kernel(const CnPoolLnParams p) {
    __shared__ float psum[CN_NT], psq[CN_NT];
    const int G = p.C >> 3, R = CN_NT / G;
    const int slot = threadIdx.x / G, g = threadIdx.x - slot * G, c = g << 3;
    const float fC = (float)p.C, denom = (float)p.hw;
    for (long long base = (long long)blockIdx.x * R; base < p.B; base += (long long)gridDim.x * R) {
        const long long n = base + slot;
        const bool active = slot < R && n < p.B;
        float v[1][8], rstd[1];
        if (active) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[0][j] = 0.f;
            for (int i = 0; i < p.hw; ++i) {
                const size_t o = ((size_t)n * p.hw + i) * p.C + c;
                const h8 vh = *(const h8*)(p.x_hi + o);
                const h8 vl = *(const h8*)(p.x_lo + o);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[0][j] += (float)vh[j] + (float)vl[j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) v[0][j] = v[0][j] / denom;
        }
        cn_ln_stats<1>(v, rstd, slot, g, G, active, fC, p.eps, psum, psq);
        if (active) {
            const f4 g0 = *(const f4*)(p.gamma + c), g1 = *(const f4*)(p.gamma + c + 4);
            const f4 b0 = *(const f4*)(p.beta + c), b1 = *(const f4*)(p.beta + c + 4);
            cn_ln_store(v[0], rstd[0], g0, g1, b0, b1, p.y_hi, p.y_lo, (size_t)n * p.C + c);
        }
    }
}

}  // namespace mpx
