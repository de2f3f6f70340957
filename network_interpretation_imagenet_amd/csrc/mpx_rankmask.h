// mpx_rankmask.h -- a second pixel source for the input staging: select between the image and a fill image on a per-pixel rank, and the
// blurred image RISE's insertion curve starts from.
//
// Holds rank_apply_kernel and blur_fill_kernel; the normalised pixel and the slot layout are mpx_stage.h's, as in every staging kernel.
//
// Every other staging entry writes the normalised pixel times a weight (mpx_softmask.h): a removed pixel is zero.  The causal metrics of a
// saliency map (Petsiuk, Das, Saenko, "RISE: Randomized Input Sampling for Explanation of Black-box Models", BMVC 2018, section 4.1) need
// more: DELETION replaces the most salient pixels, `step` more per row, by a substrate; INSERTION starts from a substrate (the blurred image)
// and reveals them.  Row m of either curve is the image with the pixels of rank below thresh[m] taken from one source and the rest from
// the other, so a curve is a rank map (one i32 per pixel), a threshold per row and at most one fill image.
//
// rank_apply_kernel, per row m, pixel p, channel c:
//   V_c = the normalised pixel, K0's op sequence bit for bit (u8 -> /255 -> -mean -> /std, each rounded; or the f32 as given)
//   F_c = fill[c][p]          if a fill image is given
//       = fl(V_c * 0.0f)      otherwise: K0's removed pixel, the -0.0 of a negative pixel included (pinned with fp32_value)
//   top = rank[p] < thresh[m]                     signed integer compare; nothing else is asked of rank or thresh
//   o_c = keep_top ? (top ? V_c : F_c) : (top ? F_c : V_c)
//   hi, lo = split_f32(o_c); channel 3 = +0.0; the 3-pixel border is not touched; out_f32[m][c][p] = o_c when given.
// No multiply touches a kept pixel (V * 1.0f == V, so it equals K0's kept pixel bit for bit).  V, F and the two splits of each are computed
// ONCE per pixel, outside the row loop; the loop body is a compare, a select and two 8-byte h4 stores in K0's coalesced wave rows.  rank[p]
// and the image are read once per tile of STAGE_MT rows.
//
// blur_fill_kernel: the separable correlation of the normalised image with klen taps and zero padding (RISE applies
// Conv2d(3, 3, klen, padding = klen / 2) with a Gaussian to the normalised tensor).  With r = klen / 2, klen odd in [1, 31]:
//   h[c][y][x]   = sum over k = 0 .. klen-1 with 0 <= x + k - r < 224, k ascending, from +0.0:  acc = fl(acc + fl(t[k] * V[c][y][x + k - r]))
//   out[c][y][x] = the same along y over h
// all in fp32, a product and a sum rounded on their own (no FMA); h is never rounded to fp16 and never leaves the LDS.
// Tile: one block = BF_TH x BF_TW = 16 x 32 output pixels of one channel, 7 x 14 x 3 = 294 blocks.  LDS, sized for klen = 31 (r = 15):
//   s_in  f32[16 + 30][32 + 30] = 11,408 B   the tile of V with its halo (zero outside the image; those cells are never summed)
//   s_h   f32[16 + 30][32]      =  5,888 B   the row pass over every tile row, halo rows included
//   s_t   f32[32]               =    128 B   the taps
// = 17,424 B per block.  Stage, barrier, row pass, barrier, column pass; no global scratch.
//
// Both: #pragma clang fp contract(off), 64-bit offsets, no atomics, no scratch.
#pragma once
#include "mpx_stage.h"

namespace mpx {

constexpr int BF_TW = 32;           // blur: output tile width
constexpr int BF_TH = 16;           // blur: output tile height
constexpr int BF_KMAX = 31;         // blur: most taps
constexpr int BF_RMAX = BF_KMAX / 2;

struct RankParams {
    const uint8_t* img_u8;   // [H][W][3] or null
    const float* img_f32;    // [3][H][W] or null
    const int32_t* rank;     // [H][W]
    const int32_t* thresh;   // [M]
    const float* fill;       // [3][H][W] or null
    half_t* out_hi;          // engine staging, slot 0 (padded NHWC4)
    half_t* out_lo;
    float* out_f32;          // [M][3][H][W] or null
    float mean[3], std[3];
    int M, slot0, keep_top;
    int size, pad_size, border;   // 224, 230, 3
};

struct BlurParams {
    const uint8_t* img_u8;   // [H][W][3] or null
    const float* img_f32;    // [3][H][W] or null
    float* out;              // [3][H][W]
    float taps[BF_KMAX + 1];
    float mean[3], std[3];
    int klen, size;
};

__global__ __launch_bounds__(256) void rank_apply_kernel(const RankParams p) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const int m_base = blockIdx.y * STAGE_MT;
    const int mt = min(STAGE_MT, p.M - m_base);
    const int hw = p.size * p.size;
    const int pix = blockIdx.x * 256 + tid;
    if (pix >= hw) return;
    const int y = pix / p.size, x = pix - y * p.size;
    float v[3], f[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        v[c] = p.img_u8 ? normalize_u8(p.img_u8[(size_t)pix * 3 + c], p.mean[c], p.std[c]) : p.img_f32[(size_t)c * hw + pix];
        f[c] = p.fill ? p.fill[(size_t)c * hw + pix] : fp32_value(v[c] * 0.0f);
    }
    // the two sources as the rows see them: `a` where rank < thresh, `b` elsewhere
    float a[3], b[3];
    h4 a_hi, a_lo, b_hi, b_lo;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a[c] = p.keep_top ? v[c] : f[c];
        b[c] = p.keep_top ? f[c] : v[c];
        half_t hi, lo;
        split_f32(a[c], hi, lo);
        a_hi[c] = hi;
        a_lo[c] = lo;
        split_f32(b[c], hi, lo);
        b_hi[c] = hi;
        b_lo[c] = lo;
    }
    a_hi[3] = a_lo[3] = b_hi[3] = b_lo[3] = (half_t)0.f;
    const int rk = p.rank[pix];
    // The loop keeps its own spelling of the slot store (mpx_stage.h's layout): through store_staged_pixel the four rank rows of
    // tools/causal_bench.py measured 0.15 to 0.27 % slower than the parent's kernel, with this text the instructions are the parent's
    const size_t plane = (size_t)p.pad_size * p.pad_size * 4;
    const size_t pad_off = staged_pixel_offset(p, y, x);
    for (int mi = 0; mi < mt; ++mi) {
        const int m = m_base + mi;
        const bool top = rk < p.thresh[m];
        const size_t so = (size_t)(p.slot0 + m) * plane + pad_off;
        *(h4*)(p.out_hi + so) = top ? a_hi : b_hi;
        *(h4*)(p.out_lo + so) = top ? a_lo : b_lo;
        if (p.out_f32) {
#pragma unroll
            for (int c = 0; c < 3; ++c) p.out_f32[((size_t)m * 3 + c) * hw + pix] = top ? a[c] : b[c];
        }
    }
}

__global__ __launch_bounds__(256) void blur_fill_kernel(const BlurParams p) {
#pragma clang fp contract(off)
    __shared__ float s_in[BF_TH + 2 * BF_RMAX][BF_TW + 2 * BF_RMAX];
    __shared__ float s_h[BF_TH + 2 * BF_RMAX][BF_TW];
    __shared__ float s_t[BF_KMAX + 1];
    const int tid = threadIdx.x;
    const int n = p.size, hw = n * n;
    const int klen = p.klen, r = klen >> 1;
    const int c = blockIdx.z;
    const int x0 = blockIdx.x * BF_TW, y0 = blockIdx.y * BF_TH;
    const int in_w = BF_TW + 2 * r, in_h = BF_TH + 2 * r;
    if (tid <= BF_KMAX) s_t[tid] = p.taps[tid];
    const float mean = c == 0 ? p.mean[0] : c == 1 ? p.mean[1] : p.mean[2];
    const float std = c == 0 ? p.std[0] : c == 1 ? p.std[1] : p.std[2];
    // the tile of V with its halo: tile cell (ty, tx) is pixel (y0 - r + ty, x0 - r + tx); zero outside the image
    for (int i = tid; i < in_h * in_w; i += 256) {
        const int ty = i / in_w, tx = i - ty * in_w;
        const int y = y0 - r + ty, x = x0 - r + tx;
        float v = 0.0f;
        if (y >= 0 && y < n && x >= 0 && x < n) {
            const size_t pix = (size_t)y * n + x;
            v = p.img_u8 ? normalize_u8(p.img_u8[pix * 3 + c], mean, std) : p.img_f32[(size_t)c * hw + pix];
        }
        s_in[ty][tx] = v;
    }
    __syncthreads();
    // row pass: h of tile row ty at output column x0 + ox, over the taps whose pixel lies inside the image, k ascending
    for (int i = tid; i < in_h * BF_TW; i += 256) {
        const int ty = i / BF_TW, ox = i - ty * BF_TW;
        const int x = x0 + ox;
        const int k_lo = max(0, r - x), k_hi = min(klen, n + r - x);
        float acc = 0.0f;
        for (int k = k_lo; k < k_hi; ++k) {
            const float t = s_t[k] * s_in[ty][ox + k];      // rounded product ...
            acc = acc + t;                                  // ... rounded sum: not an FMA
        }
        s_h[ty][ox] = acc;
    }
    __syncthreads();
    // column pass: the same along y over h (h row ty is image row y0 - r + ty)
    for (int i = tid; i < BF_TH * BF_TW; i += 256) {
        const int oy = i / BF_TW, ox = i - oy * BF_TW;
        const int y = y0 + oy, x = x0 + ox;
        if (y >= n || x >= n) continue;
        const int k_lo = max(0, r - y), k_hi = min(klen, n + r - y);
        float acc = 0.0f;
        for (int k = k_lo; k < k_hi; ++k) {
            const float t = s_t[k] * s_h[oy + k][ox];
            acc = acc + t;
        }
        p.out[(size_t)c * hw + (size_t)y * n + x] = acc;
    }
}

}  // namespace mpx
