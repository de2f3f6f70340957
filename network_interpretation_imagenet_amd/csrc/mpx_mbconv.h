// mpx_mbconv.h -- the element-wise kernels of an MBConv block with Squeeze-and-Excitation (torchvision's EfficientNet-B0) on split-fp16 NHWC
// planes, gfx950: the depthwise k x k conv + BatchNorm with SiLU on either side, the SE gate (global pool + two FCs per image), the SE
// scale, and the global average pool that takes SiLU as it loads.
//
// SiLU and the MFMA convs.  The conv kernels' epilogues know ReLU only, and silu(x) = x * sigmoid(x) cannot be had from ReLU by a clamp on
// load.  So an MFMA conv that torchvision follows with SiLU (the stem, every expand conv, features.8) runs WITHOUT an activation and stores
// bn(conv(x)); its one CONSUMER takes silu(x) as it loads: a depthwise layer (act_in) or the SiLU global pool.  The depthwise layer applies
// its own SiLU in its epilogue (act_out), once per element.  No MFMA kernel, epilogue or tile changes.
#pragma once
#include <cmath>

#include "mpx_conv.h"

namespace mpx {

// silu(x) = x / (1 + e^-x): the accurate expf and an IEEE division.  For large negative x expf overflows to +inf and the quotient is -0,
// the correct limit; silu(0) = 0, so pad channels stay exact zeros.  The one definition every kernel below uses.
__device__ __forceinline__ float silu_f32(float x) { return x / (1.0f + expf(-x)); }

// ------------------------------------------------------------------------------------------
// Depthwise K x K conv (K = 3 or 5, pad (K - 1) / 2, stride 1 or 2) + BatchNorm, with SiLU on the input (act_in) and on the output (act_out):
// planes [B][hin][hin][pitch] -> [B][ho][ho][pitch], ho = (hin - 1) / STRIDE + 1.  Per output element, in fp32:
//     x = hi + lo (exact);  a = act_in ? silu(x) : x, once per LOADED element, not once per tap;
//     acc = 0;  for ky in 0..K-1, kx in 0..K-1 (row-major):  acc = fma(w[ky * K + kx][c], a[iy][ix][c], acc)   over the taps inside the map;
//     v = fl(fl(s * acc) + t) -- two roundings: plain operators under contract(off), as dwconv3x3_bn_kernel (mpx_shuffle.h has the reason);
//     act_out ? silu(v) : v;  the re-split;  one 16-byte store per plane.
// w: fp32 tap-major [K * K][pitch]; s, t: fp32 [pitch].  Channels of the pitch beyond the layer's own carry zero weights, scale and shift and
// come out as exact zeros (silu(0) = 0).
// THE RUN FORM of dwconv3x3_bn_kernel: one thread = 8 channels of a run of W output pixels along x (W = 4 at stride 1, 2 at stride 2).  Row
// by row it loads the run's NC = STRIDE * (W - 1) + K input columns once (8 columns for four 5x5 stride-1 outputs where one thread per
// output pixel would load 20) and feeds every output its K taps of that row, kx ascending: each output sees its taps in row-major order.  A
// column outside the map is loaded at a clamped index (inside the planes) and its fma is not taken; a row outside the map is skipped.  Only
// one input row (NC x 8 values) is live at a time.
// Units (n, oy, run, 8-channel group) are 64-bit, consecutive lanes take consecutive 16-byte groups of a pixel; the grid is capped by the
// host and strides over the rest.  Offsets are 64-bit.  No atomics, no scratch (every array is indexed by unrolled constants), no LDS.
// ------------------------------------------------------------------------------------------
struct MbDwParams {
    const half_t* x_hi;
    const half_t* x_lo;
    half_t* y_hi;
    half_t* y_lo;
    const float* w;          // [K * K][pitch]
    const float* scale;      // [pitch]
    const float* shift;
    long long rows;          // B * ho output rows
    int hin, ho, pitch, act_in, act_out;
};

template <int K, int STRIDE>
struct MbDwRun {
    static constexpr int W = STRIDE == 1 ? 4 : 2;       // output pixels per thread
    static constexpr int NC = STRIDE * (W - 1) + K;     // input columns under them
};

template <int K, int STRIDE>
__global__ __launch_bounds__(256) void dwconv_bn_act_kernel(const MbDwParams p) {
#pragma clang fp contract(off)
    constexpr int W = MbDwRun<K, STRIDE>::W, NC = MbDwRun<K, STRIDE>::NC, PAD = (K - 1) / 2;
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
                    xm[q][j] = p.act_in ? silu_f32(x) : x;
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
                if (p.act_out) v = silu_f32(v);
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

// ------------------------------------------------------------------------------------------
// The SE gate of one image per workgroup: gate = sigmoid(fc2(act(fc1(mean over the hw pixels of x)))), act = SiLU (EfficientNet) or ReLU (RegNetY:
// the template parameter below), planes [B][hw][pitch] -> f32
// [B][pitch].  256 threads, three phases with a barrier between them; every summation order is a fixed function of (hw, pitch, q), never of
// B, the grid or timing, so an image's gate has the same bits alone and anywhere in any batch.  No atomics.
//   POOL.  G = pitch / 8 groups of 8 channels.  S = max(1, 256 / G) slices: thread t < S * G takes group t % G and the pixels s, s + S,
//       s + 2 S, ... (s = t / G) in ascending order, fp32 adds of hi + lo (exact), into part[s][c] (LDS); with G > 256 a thread takes the
//       groups t, t + 256, ...  Then pooled[c] = (part[0][c] + part[1][c] + ... + part[S - 1][c]) / hw, slices ascending, one division.
//       Consecutive threads read consecutive 16-byte units: a wave reads whole pixels.
//   FC1.  One wave per output j = wave, wave + 4, ... < q: lane l sums fma(w1[j][c], pooled[c], .) over c = l, l + 64, ... ascending, the 64
//       lane sums are folded by the xor butterfly 32, 16, 8, 4, 2, 1 (the same tree in every lane), and s1[j] = act(b1[j] + sum): silu, or ReLU as `v <= 0 ? 0 : v`.
//   FC2.  Thread t takes the channels c = t, t + 256, ...: z = fma(w2[j][c], s1[j], z) over j ascending from z = 0, gate[c] = 1 / (1 +
//       expf(-(b2[c] + z))).
// w1: f32 [q][pitch] (fc1.weight, zero columns on the pad channels); b1: f32 [q]; w2: f32 [q][pitch], j-major (w2[j][c] = fc2.weight[c][j]:
// consecutive threads read consecutive floats), zero on the pad channels; b2: f32 [pitch] with -inf ON THE PAD CHANNELS: 1 / (1 + expf(+inf)) = 0
// exactly, so the pad channels' gates are exact zeros (sigmoid's limit, as silu's above) and the kernel needs no channel count.
// (From pitch 1032 on S is 1 and only G of the 256 threads pool: at pitch 1152 on a 7x7 map 144 threads walk 49 pixels each.  Cutting the
// pixels of a group over the idle threads as well would still be a fixed function of (hw, pitch, q); not done here)
// hw from 1 upward, q from 1 upward (no multiple of anything), pitch a multiple of 8.  Dynamic LDS: (S * pitch + pitch + q) floats --
// S * pitch <= 2048 below pitch 2048; 9.4 KB for the widest layer here (pitch 1152, q 48).
// ------------------------------------------------------------------------------------------
struct SeGateParams {
    const half_t* x_hi;
    const half_t* x_lo;
    const float* w1;
    const float* b1;
    const float* w2;
    const float* b2;
    float* gate;             // [B][pitch]
    int hw, pitch, q;
};

__host__ __device__ inline int se_gate_slices(int pitch) { return (pitch >> 3) >= 256 ? 1 : 256 / (pitch >> 3); }

// RELU = false: the gate above (EfficientNet).  RELU = true: fc1 ends in ReLU instead of SiLU -- s1[j] = (v <= 0 ? 0 : v) with v = b1[j] + sum, the
// project's ReLU form -- which is torchvision's default SqueezeExcitation and the gate of a RegNetY block; POOL and FC2 are the same code.
template <bool RELU>
__global__ __launch_bounds__(256) void se_gate_kernel(const SeGateParams p) {
    extern __shared__ __attribute__((aligned(16))) float se_lds[];
    const int G = p.pitch >> 3, S = se_gate_slices(p.pitch);
    float* part = se_lds;                       // [S][pitch]
    float* pooled = part + (size_t)S * p.pitch; // [pitch]
    float* s1 = pooled + p.pitch;               // [q]
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * p.hw * p.pitch;
    // ---- pool
    const int s = tid / G;
    if (s < S) {
        for (int g = tid - s * G; g < G; g += 256) {        // G <= 256: one group per thread
            float sum[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) sum[j] = 0.f;
#pragma unroll 4
            for (int i = s; i < p.hw; i += S) {
                const size_t at = base + (size_t)i * p.pitch + (g << 3);
                const h8 vh = *(const h8*)(p.x_hi + at);
                const h8 vl = *(const h8*)(p.x_lo + at);
#pragma unroll
                for (int j = 0; j < 8; ++j) sum[j] += (float)vh[j] + (float)vl[j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) part[(size_t)s * p.pitch + (g << 3) + j] = sum[j];
        }
    }
    __syncthreads();
    const float denom = (float)p.hw;
    for (int c = tid; c < p.pitch; c += 256) {
        float sum = part[c];
        for (int s = 1; s < S; ++s) sum += part[(size_t)s * p.pitch + c];
        pooled[c] = sum / denom;
    }
    __syncthreads();
    // ---- fc1
    const int lane = tid & 63, wave = tid >> 6;
    for (int j = wave; j < p.q; j += 4) {
        const float* wr = p.w1 + (size_t)j * p.pitch;
        float sum = 0.f;
        for (int c = lane; c < p.pitch; c += 64) sum = __fmaf_rn(wr[c], pooled[c], sum);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
        if (lane == 0) {
            const float v = p.b1[j] + sum;
            s1[j] = RELU ? (v <= 0.f ? 0.f : v) : silu_f32(v);
        }
    }
    __syncthreads();
    // ---- fc2
    float* out = p.gate + (size_t)blockIdx.x * p.pitch;
    for (int c = tid; c < p.pitch; c += 256) {
        float z = 0.f;
        for (int j = 0; j < p.q; ++j) z = __fmaf_rn(p.w2[(size_t)j * p.pitch + c], s1[j], z);
        out[c] = 1.0f / (1.0f + expf(-(p.b2[c] + z)));
    }
}

// ------------------------------------------------------------------------------------------
// The SE scale: out = split(fl((hi + lo) * gate[n][c])) on planes [B][hw][pitch], gate f32 [B][pitch].  Element-wise: one thread = 8 channels
// of one pixel, one 16-byte load and store per plane and two 16-byte loads of the gate; a unit is read and written by the same thread, so
// out may alias in.  Units are 64-bit, the grid is capped by the host and strides over the rest.  No LDS, no atomics, no scratch.
// ------------------------------------------------------------------------------------------
struct SeScaleParams {
    const half_t* x_hi;
    const half_t* x_lo;
    const float* gate;
    half_t* y_hi;
    half_t* y_lo;
    long long units;         // B * hw * pitch / 8
    long long per_image;     // hw * pitch / 8
    int pitch;
};

__global__ __launch_bounds__(256) void se_scale_kernel(const SeScaleParams p) {
#pragma clang fp contract(off)
    const long long cg = p.pitch >> 3;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < p.units; t += (long long)gridDim.x * 256) {
        const long long n = t / p.per_image;
        const int c = (int)(t % cg) << 3;
        const size_t at = (size_t)t << 3;
        const h8 vh = *(const h8*)(p.x_hi + at);
        const h8 vl = *(const h8*)(p.x_lo + at);
        const float* gp = p.gate + (size_t)n * p.pitch + c;
        const f4 g0 = *(const f4*)gp, g1 = *(const f4*)(gp + 4);
        h8 oh, ol;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = ((float)vh[j] + (float)vl[j]) * (j < 4 ? g0[j & 3] : g1[j & 3]);
            half_t hi, lo;
            split_f32(v, hi, lo);
            oh[j] = hi;
            ol[j] = lo;
        }
        *(h8*)(p.y_hi + at) = oh;
        *(h8*)(p.y_lo + at) = ol;
    }
}

// ------------------------------------------------------------------------------------------
// Global average pool [B][hw][c] -> [B][c] of silu(x): global_avgpool_clamp6_kernel (mpx_dw.h) with the SiLU of the producing MFMA conv
// (features.8) in place of the clamp.  One thread = 8 channels of one image; the hw values are summed in pixel order in fp32 and divided by
// hw once.  A kernel of its own: the other pools stay as they are.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void global_avgpool_silu_kernel(const half_t* __restrict__ in_hi, const half_t* __restrict__ in_lo,
                                                                   half_t* __restrict__ out_hi, half_t* __restrict__ out_lo, int B, int hw,
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
        for (int j = 0; j < 8; ++j) sum[j] += silu_f32((float)vh[j] + (float)vl[j]);
    }
    h8 oh, ol;
    const float denom = (float)hw;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        half_t hi, lo;
        split_f32(sum[j] / denom, hi, lo);
        oh[j] = hi;
        ol[j] = lo;
    }
    const size_t o = (size_t)n * c + g * 8;
    *(h8*)(out_hi + o) = oh;
    *(h8*)(out_lo + o) = ol;
}

}  // namespace mpx
