// mpx_mbconv.h -- the Squeeze-and-Excitation kernels of an MBConv block (torchvision's EfficientNet-B0) and of a RegNetY block on split-fp16
// NHWC planes, gfx950: the SE gate (global pool + two FCs per image) and the SE scale.  (The block's depthwise k x k conv + BatchNorm with
// SiLU on either side is the run form of mpx_dw.h, which also says how SiLU meets the MFMA convs; the global average pool that takes SiLU as
// it loads is mpx_kernels.h's global_avgpool_kernel<POOL_SILU>; silu_f32 itself is mpx_conv.h's.)
#pragma once
#include "mpx_conv.h"

namespace mpx {

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
// exactly, so the pad channels' gates are exact zeros (sigmoid's limit, as silu_f32's) and the kernel needs no channel count.
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

}  // namespace mpx
