// mpx_gconv.h -- grouped 3x3 conv (pad 1, stride 1 or 2) + BatchNorm + ReLU, gfx950: the conv2 of a ResNeXt bottleneck (tile id 16).
//
// The layer is width -> width with 32 groups of cg = width / 32 channels.  Its channels are cut into CHANNEL BLOCKS of CB = max(cg, 16):
// block b reads input channels [b * CB, (b + 1) * CB) and writes the same output channels.  For cg >= 16 a block is one group; for cg = 4 /
// 8 a block holds 4 / 2 groups, and the host packer (pack_gconv_weights, mpx_api.hip) writes their weights block-diagonally with exact zeros
// (0 * x adds nothing: activations are finite).  Per block the conv is the small GEMM
//   D[co][pixel] = sum_k W[co][k] * X[pixel][k],   k = (ky, kx, ci), ci fastest over the block's CB channels, K = 9 * CB padded to KP(CB)
// on v_mfma_f32_16x16x32_f16 as mpx_conv.h's three products per 32-wide K step, W_hi*X_lo, W_lo*X_hi, W_hi*X_hi in that order, into one fp32
// accumulator.  A = weights (MFMA rows = cout), B = pixels (MFMA cols): an accumulator quad is 4 consecutive channels of one pixel.
//
// One wave owns 16 consecutive output pixels (of the flat index m = (n * ho + oy) * wo + ox: a 7-pixel row simply continues in the next row
// or image) x one channel block; the 4 waves of a workgroup take 4 neighbouring blocks of the same pixels, so the 128-byte lines they touch
// are shared in L1.  Operands come 16 bytes per lane straight from global memory, no LDS: lane l holds K elements (l >> 4) * 8 .. + 8 of
// MFMA row / column l & 15.  CB is a multiple of 8, so a lane's 8 elements are 8 consecutive channels of ONE tap.
// A TAP OUTSIDE THE MAP (and the K padding behind tap 8, and a pixel m >= M) IS AN OPERAND OF EXACT ZEROS: the load address is clamped to the
// plane's first element and the loaded bits are ANDed with 0 -- the weight of that tap is not zero and an MFMA cannot skip a term.  The mask
// is bit arithmetic on purpose (mpx_conv.h, stage_x: a per-lane branch around a load would put MFMAs under a partial EXEC).
// Packed weight planes: [block][CB / 16 row fragments][KP / 32 steps][64 lanes][8], i.e. a wave's fragment of one step is one contiguous KiB
// already in lane order (gconv_w_index).
// Epilogue: conv_f16x3_kernel's phase 1 + 2 on registers -- acc * scale + shift, ReLU as `v <= 0 ? 0 : v`, split_f32 -- and 8-byte stores of
// the quad into both planes.  No residual operand (conv2 never has one), no atomics, no split-K; offsets are 64-bit.  Every output element
// is computed from its own pixel's column of the MFMA alone, so its bits do not depend on the batch around it.
#pragma once
#include "mpx_conv.h"

namespace mpx {

constexpr int GCONV_WAVES = 4;      // channel blocks per workgroup

__host__ __device__ constexpr int gconv_cb(int cg) { return cg > 16 ? cg : 16; }
__host__ __device__ constexpr int gconv_kp(int cb) { return (9 * cb + 31) / 32 * 32; }      // 160, 288, 576 for CB = 16, 32, 64

// Element index of weight (row r of block b, k) within a packed plane
__host__ __device__ inline size_t gconv_w_index(int b, int r, int k, int cb) {
    const int nks = gconv_kp(cb) >> 5;
    const int lane = (((k >> 3) & 3) << 4) | (r & 15);
    return ((((size_t)b * (cb >> 4) + (r >> 4)) * nks + (k >> 5)) * 64 + lane) * 8 + (k & 7);
}

typedef unsigned int u4 __attribute__((ext_vector_type(4)));

// ConvParams as conv_f16x3_kernel takes them: pix_stride = cout = the layer's width, n_tiles_c = its channel blocks (a multiple of
// GCONV_WAVES), kh = kw = 3, pad = 1.  Grid (ceil(M / 16), n_tiles_c / GCONV_WAVES), 64 * GCONV_WAVES threads.
template <int CB>
__global__ __launch_bounds__(64 * GCONV_WAVES) void gconv3x3_f16x3_kernel(const ConvParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int CF = CB / 16, NKS = gconv_kp(CB) / 32;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int blk = blockIdx.y * GCONV_WAVES + wave;
    if (blk >= p.n_tiles_c) return;                 // wave-uniform
    const int q = lane >> 4, col = lane & 15;
    const long long m = (long long)blockIdx.x * 16 + col;
    const bool m_ok = m < p.M;
    const int howo = p.ho * p.wo;
    const int mm = m_ok ? (int)m : 0;
    const int n = mm / howo;
    const int rem = mm - n * howo;
    const int oy = rem / p.wo, ox = rem - oy * p.wo;
    const int iy0 = oy * p.stride - 1, ix0 = ox * p.stride - 1;
    const int C = p.pix_stride;
    // element offset of (n, iy0, ix0, first channel of the block); negative on the border, used only under a tap that is inside
    const long long xbase = (((long long)n * p.hin + iy0) * p.win + ix0) * C + (long long)blk * CB;
    const size_t wbase = (size_t)blk * CF * NKS * 512 + (size_t)lane * 8;

    struct Frags {
        h8 a_hi[CF], a_lo[CF], b_hi, b_lo;
    };
    auto load = [&](int ks, Frags& f) {
#pragma unroll
        for (int a = 0; a < CF; ++a) {
            const size_t wo_ = wbase + (size_t)(a * NKS + ks) * 512;
            f.a_hi[a] = *(const h8*)(p.w_hi + wo_);
            f.a_lo[a] = *(const h8*)(p.w_lo + wo_);
        }
        const int k8 = ks * 32 + q * 8;
        const int tap = k8 / CB, ci0 = k8 - tap * CB;
        const int ky = (tap * 11) >> 5, kx = tap - 3 * ky;          // tap / 3 for tap <= 10
        const int iy = iy0 + ky, ix = ix0 + kx;
        const bool ok = m_ok && tap < 9 && (unsigned)iy < (unsigned)p.hin && (unsigned)ix < (unsigned)p.win;
        const long long off = ok ? xbase + ((long long)ky * p.win + kx) * C + ci0 : 0;
        const unsigned keep = ok ? 0xffffffffu : 0u;
        const u4 vh = *(const u4*)(p.x_hi + off) & keep;
        const u4 vl = *(const u4*)(p.x_lo + off) & keep;
        f.b_hi = __builtin_bit_cast(h8, vh);
        f.b_lo = __builtin_bit_cast(h8, vl);
    };
    f4 acc[CF];
#pragma unroll
    for (int a = 0; a < CF; ++a) acc[a] = (f4){0.f, 0.f, 0.f, 0.f};
    Frags f[2];
    load(0, f[0]);
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        if (ks + 1 < NKS) load(ks + 1, f[(ks + 1) & 1]);
        const Frags& c = f[ks & 1];
#pragma unroll
        for (int a = 0; a < CF; ++a) {
            acc[a] = __builtin_amdgcn_mfma_f32_16x16x32_f16(c.a_hi[a], c.b_lo, acc[a], 0, 0, 0);
            acc[a] = __builtin_amdgcn_mfma_f32_16x16x32_f16(c.a_lo[a], c.b_hi, acc[a], 0, 0, 0);
            acc[a] = __builtin_amdgcn_mfma_f32_16x16x32_f16(c.a_hi[a], c.b_hi, acc[a], 0, 0, 0);
        }
    }
    // epilogue: D row = channel (lane >> 4) * 4 + reg of the fragment, col = pixel
    if (!m_ok) return;
#pragma unroll
    for (int a = 0; a < CF; ++a) {
        const int ch = blk * CB + a * 16 + q * 4;
        const f4 sc = *(const f4*)(p.scale + ch);
        const f4 sh = *(const f4*)(p.shift + ch);
        const f4 v = acc[a] * sc + sh;
        h4 oh, ol;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float r = p.relu ? (v[j] <= 0.f ? 0.f : v[j]) : v[j];
            half_t hi, lo;
            split_f32(r, hi, lo);
            oh[j] = hi;
            ol[j] = lo;
        }
        const size_t o = (size_t)m * p.cout + ch;
        __builtin_nontemporal_store(oh, (h4*)(p.y_hi + o));
        __builtin_nontemporal_store(ol, (h4*)(p.y_lo + o));
    }
#endif
}

}  // namespace mpx
