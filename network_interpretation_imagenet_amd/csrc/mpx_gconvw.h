// mpx_gconvw.h -- grouped 3x3 conv (pad 1, stride 1 or 2) + BatchNorm + ReLU for ANY group count and any group width that is a multiple
// of 8, on planes whose pixel pitch may exceed the layer's width, gfx950: the f.b of a RegNetX / RegNetY block (tile id 18).
//
// The layer is width -> width in G = width / CG groups of CG channels (16, 24, 48 or 120 in torchvision's RegNetX up to 8GF, 16, 24 or 56 in its
// RegNetY from 800MF to 8GF; G is whatever the stage width gives: 2 .. 63, 7, 17, 25, 37 and 49 among them; the stand-alone entry also runs G = 1).  Input pixels are x_pitch = p.pix_stride channels apart, output pixels p.cout
// channels, both >= width and multiples of 8.  Per group g the conv is mpx_gconv.h's small GEMM
//   D[co][pixel] = sum_k W[co][k] * X[pixel][k],   k = (ky, kx, ci), ci fastest over the group's CG channels, K = 9 * CG padded to a multiple of 32
// on v_mfma_f32_16x16x32_f16, the K steps ascending, each step the three products W_hi*X_lo, W_lo*X_hi, W_hi*X_hi in that order into one fp32
// accumulator.  For CG = 16 every index, operand and product is tile 16's (gconv3x3_f16x3_kernel<16>): the two kernels give the same bits, and
// the packed planes of such a layer are the same planes.
//
// Against mpx_gconv.h:
//   - a group has RF = ceil(CG / 16) row fragments; the rows >= CG of the last one (CG = 24, 56, 120) are exact-zero weights in the packed planes and
//     their accumulator quads are never stored (CG % 8 == 0: a lane's quad of 4 channels lies wholly inside or outside the group);
//   - K is the flattened (tap, ci) index, so a 32-wide K step may straddle taps (CG = 24, 48, 56, 120); a lane's 8 elements are still 8 consecutive
//     channels of ONE tap (CG % 8 == 0), and the padding behind tap 8 is an operand of exact zeros by the same clamp-and-AND as a tap outside
//     the map -- bit arithmetic, no branch around a load;
//   - the unit of work of a wave is (NT = 2 tiles of 16 consecutive output pixels) x (one group) x (a CHUNK of at most 4 row fragments): CG = 120
//     is 8 fragments = 2 chunks, so that a wave's double-buffered A fragments stay at 64 VGPRs (164 VGPRs in all, no scratch); CG = 56 is 4 fragments = one whole
//     chunk with the same 64 (142 VGPRs in all, no scratch; K = 504 padded to 512: its last K step holds 8 padding elements behind tap 8).  Unit u = group * NCH + chunk; the 4 waves of a workgroup take 4
//     consecutive units of the same pixels -- the chunks of one group, then the neighbouring groups -- so the pixel lines they read are shared
//     in L1.  The last workgroup in y is ragged for any G: a wave whose unit does not exist exits, wave-uniformly;
//   - the wave of unit 0 also writes the output's pad channels [width, p.cout) of its pixels as +0 in both planes: the arena's buffers are
//     reused at other pitches, the 1x1 consumer multiplies those channels by zero weights, and 0 * NaN from a stale buffer would poison a pixel.
// Packed weight planes: [group][RF][K / 32 steps][64 lanes][8] (gconvw_w_index), a wave's fragment of one step one contiguous KiB in lane order.
// Epilogue: mpx_gconv.h's -- acc * scale + shift, ReLU as `v <= 0 ? 0 : v`, split_f32, 8-byte stores of the quad into both planes.  No residual
// operand, no atomics, no split-K, no LDS, no scratch; offsets are 64-bit; global loads are 16 bytes.  Every output element is computed from its
// own pixel's column of the MFMA and its own row fragment alone: its bits depend neither on the batch, nor on the image's index, nor on the grid.
#pragma once
#include "mpx_gconv.h"

namespace mpx {

constexpr int GCONVW_WAVES = 4;     // units per workgroup
constexpr int GCONVW_CHUNK = 4;     // row fragments per unit, at most

__host__ __device__ constexpr int gconvw_rf(int cg) { return (cg + 15) / 16; }
__host__ __device__ constexpr int gconvw_kp(int cg) { return (9 * cg + 31) / 32 * 32; }     // 160, 224, 448, 512, 1088 for CG = 16, 24, 48, 56, 120
__host__ __device__ constexpr int gconvw_nch(int cg) { return (gconvw_rf(cg) + GCONVW_CHUNK - 1) / GCONVW_CHUNK; }

// Element index of weight (row r of group g, k) within a packed plane
__host__ __device__ inline size_t gconvw_w_index(int g, int r, int k, int cg) {
    const int nks = gconvw_kp(cg) >> 5;
    const int lane = (((k >> 3) & 3) << 4) | (r & 15);
    return ((((size_t)g * gconvw_rf(cg) + (r >> 4)) * nks + (k >> 5)) * 64 + lane) * 8 + (k & 7);
}

// Pixel tiles of 16 per wave: 2 -- a wave owns 32 consecutive pixels and uses every weight fragment twice, which halves the weight fetches and
// puts twice the MFMAs behind each of them.  In the network at batch 512, one tile -> two, both builds alternating twice in one call, ms of
// the grouped launches per batch: 400MF 2.61 -> 2.34, 800MF 4.32 -> 3.81, 1.6GF 9.98 -> 9.16, 3.2GF 14.76 -> 12.20, 8GF 29.44 -> 23.77; every
// one of the 36 shapes gains (x 0.78 .. 0.96).  -DMPX_GCONVW_NT=1 builds the one-tile form (A/B builds only).  An output element's bits do
// not depend on the choice: its K order and operands are the same.
#ifndef MPX_GCONVW_NT
#define MPX_GCONVW_NT 2
#endif
constexpr int GCONVW_NT = MPX_GCONVW_NT;

// ConvParams: pix_stride = the input's pixel pitch, cout = the output's, n_tiles_c = G, k_per_tap = width, kh = kw = 3, pad = 1.
// Grid (ceil(M / (16 NT)), ceil(G * NCH / GCONVW_WAVES)), 64 * GCONVW_WAVES threads.
template <int CG, int NT>
__global__ __launch_bounds__(64 * GCONVW_WAVES) void gconvw3x3_f16x3_kernel(const ConvParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(CG % 8 == 0 && CG >= 16, "a lane's 8 K elements are 8 consecutive channels of one tap");
    constexpr int RF = gconvw_rf(CG), NKS = gconvw_kp(CG) / 32, NCH = gconvw_nch(CG);
    constexpr int CF = RF < GCONVW_CHUNK ? RF : GCONVW_CHUNK;       // fragments of a whole chunk
    static_assert(RF % CF == 0, "every chunk of a group has the same number of row fragments");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int unit = blockIdx.y * GCONVW_WAVES + wave;
    if (unit >= p.n_tiles_c * NCH) return;          // wave-uniform
    const int g = unit / NCH, chunk = unit - g * NCH;
    const int q = lane >> 4, col = lane & 15;
    const int howo = p.ho * p.wo;
    const int P = p.pix_stride;
    long long m[NT], xbase[NT];
    bool m_ok[NT];
    int iy0[NT], ix0[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        m[t] = ((long long)blockIdx.x * NT + t) * 16 + col;
        m_ok[t] = m[t] < p.M;
        const int mm = m_ok[t] ? (int)m[t] : 0;
        const int n = mm / howo;
        const int rem = mm - n * howo;
        const int oy = rem / p.wo, ox = rem - oy * p.wo;
        iy0[t] = oy * p.stride - 1;
        ix0[t] = ox * p.stride - 1;
        // element offset of (n, iy0, ix0, first channel of the group); negative on the border, used only under a tap that is inside
        xbase[t] = (((long long)n * p.hin + iy0[t]) * p.win + ix0[t]) * P + (long long)g * CG;
    }
    const size_t wbase = ((size_t)g * RF + (size_t)chunk * CF) * NKS * 512 + (size_t)lane * 8;

    struct Frags {
        h8 a_hi[CF], a_lo[CF], b_hi[NT], b_lo[NT];
    };
    auto load = [&](int ks, Frags& f) {
#pragma unroll
        for (int a = 0; a < CF; ++a) {
            const size_t wo_ = wbase + (size_t)(a * NKS + ks) * 512;
            f.a_hi[a] = *(const h8*)(p.w_hi + wo_);
            f.a_lo[a] = *(const h8*)(p.w_lo + wo_);
        }
        const int k8 = ks * 32 + q * 8;
        const int tap = k8 / CG, ci0 = k8 - tap * CG;
        const int ky = (tap * 11) >> 5, kx = tap - 3 * ky;          // tap / 3 for tap <= 10
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int iy = iy0[t] + ky, ix = ix0[t] + kx;
            const bool ok = m_ok[t] && tap < 9 && (unsigned)iy < (unsigned)p.hin && (unsigned)ix < (unsigned)p.win;
            const long long off = ok ? xbase[t] + ((long long)ky * p.win + kx) * P + ci0 : 0;
            const unsigned keep = ok ? 0xffffffffu : 0u;
            const u4 vh = *(const u4*)(p.x_hi + off) & keep;
            const u4 vl = *(const u4*)(p.x_lo + off) & keep;
            f.b_hi[t] = __builtin_bit_cast(h8, vh);
            f.b_lo[t] = __builtin_bit_cast(h8, vl);
        }
    };
    f4 acc[NT][CF];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int a = 0; a < CF; ++a) acc[t][a] = (f4){0.f, 0.f, 0.f, 0.f};
    Frags f[2];
    load(0, f[0]);
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        if (ks + 1 < NKS) load(ks + 1, f[(ks + 1) & 1]);
        const Frags& c = f[ks & 1];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int a = 0; a < CF; ++a) {
                acc[t][a] = __builtin_amdgcn_mfma_f32_16x16x32_f16(c.a_hi[a], c.b_lo[t], acc[t][a], 0, 0, 0);
                acc[t][a] = __builtin_amdgcn_mfma_f32_16x16x32_f16(c.a_lo[a], c.b_hi[t], acc[t][a], 0, 0, 0);
                acc[t][a] = __builtin_amdgcn_mfma_f32_16x16x32_f16(c.a_hi[a], c.b_hi[t], acc[t][a], 0, 0, 0);
            }
    }
    // epilogue: D row = channel (lane >> 4) * 4 + reg of the fragment, col = pixel
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (!m_ok[t]) continue;
        const size_t obase = (size_t)m[t] * p.cout;
#pragma unroll
        for (int a = 0; a < CF; ++a) {
            const int r = (chunk * CF + a) * 16 + q * 4;        // the quad's first channel within the group
            if (r >= CG) continue;                              // a zero-weight row of the last fragment: not stored
            const int ch = g * CG + r;
            const f4 sc = *(const f4*)(p.scale + ch);
            const f4 sh = *(const f4*)(p.shift + ch);
            const f4 v = acc[t][a] * sc + sh;
            h4 oh, ol;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float rr = p.relu ? (v[j] <= 0.f ? 0.f : v[j]) : v[j];
                half_t hi, lo;
                split_f32(rr, hi, lo);
                oh[j] = hi;
                ol[j] = lo;
            }
            __builtin_nontemporal_store(oh, (h4*)(p.y_hi + obase + ch));
            __builtin_nontemporal_store(ol, (h4*)(p.y_lo + obase + ch));
        }
        // the pad channels [width, pitch) of this wave's pixels: +0 in both planes (unit 0 alone; width and pitch are multiples of 8)
        if (unit == 0) {
            const h4 z = (h4){(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f};
            for (int ch = p.k_per_tap + q * 4; ch < p.cout; ch += 16) {
                __builtin_nontemporal_store(z, (h4*)(p.y_hi + obase + ch));
                __builtin_nontemporal_store(z, (h4*)(p.y_lo + obase + ch));
            }
        }
    }
#endif
}

}  // namespace mpx
