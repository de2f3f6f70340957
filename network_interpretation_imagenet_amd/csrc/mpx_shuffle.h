// mpx_shuffle.h -- ShuffleNetV2's two element-wise kernels on split-fp16 NHWC planes, gfx950: the channel shuffle of a two-way concatenation
// and the depthwise 3x3 conv + BatchNorm with NO activation behind it.
//
// The two-half layout.  A ShuffleNetV2 stage map has 2 * bf logical channels (bf = oup / 2) and every block splits it into its first and
// second half.  It is stored with a pitch of 2 * hp, hp = bf rounded up to 32: logical channel l < bf at physical l, l >= bf at
// hp + (l - bf); physical channels [bf, hp) and [hp + bf, 2 hp) are exact zeros, written by every forward.  Both halves are then contiguous,
// 16-byte aligned and a whole number of 32-wide K steps: a stride-1 block's branch2.0 reads the second half in place (pointer + hp,
// pix_stride 2 hp, K = hp) and the shuffle reads the first half in place.
#pragma once
#include "mpx_dw.h"      // DwParams

namespace mpx {

// ------------------------------------------------------------------------------------------
// channel_shuffle(cat(a, b), 2) into the two-half layout: a [npix][a_pitch] and b [npix][b_pitch] carry bf real channels each, y is
// [npix][2 hp].  For physical output channel q, h = q / hp and j = q % hp: j >= bf is a pad channel (zero bits in both planes), else
// l = h * bf + j is the logical output channel and its (hi, lo) pair is copied verbatim from (l & 1 ? b : a)[l >> 1].  Pure data movement.
// One thread = 8 output channels of one pixel: one 16-byte store per plane.  hp is a multiple of 32, so a unit lies in one half; bf is even
// and j0 = the unit's first j a multiple of 8, so l0 = h * bf + j0 is even: the unit's even channels are a[s0 .. s0 + 3], its odd ones
// b[s0 .. s0 + 3], s0 = l0 / 2 = h * bf / 2 + j0 / 2.
// LOAD WIDTH FOLLOWS THE ALIGNMENT, selected at launch: s0 is a multiple of 4 elements (8 bytes) for both halves only when bf % 8 == 0
// (pitches are multiples of 8).  VEC = true (bf % 8 == 0): one 8-byte load per source plane.  VEC = false (bf / 2 = 29, 58, 61, 122 of
// ShuffleNetV2's twelve shapes): four 2-byte loads per source plane.  (The alternative -- aligned 16-byte loads around s0 and a funnel
// pick in registers -- reads elements left and right of the four it needs, pad channels and the neighbouring half among them, and at the
// last pixel of a plane past its end; a form whose every load is an element it copies needs no argument about what it may touch.)
// A unit that straddles bf (bf % 8 != 0 only) copies its nv = bf - j0 real channels through predicated 2-byte loads and writes zeros
// behind them; no pad channel of a or b is ever read.
// Units are 64-bit, consecutive lanes take consecutive 16-byte groups of a pixel; the grid is capped by the host and strides over the
// rest.  Offsets are 64-bit.  No LDS, no atomics, no scratch (every array below is indexed by unrolled constants).
// ------------------------------------------------------------------------------------------
struct ShuffleParams {
    const half_t* a_hi;
    const half_t* a_lo;
    const half_t* b_hi;
    const half_t* b_lo;
    half_t* y_hi;
    half_t* y_lo;
    long long npix;
    int a_pitch, b_pitch, bf, hp;
};

template <bool VEC>
__global__ __launch_bounds__(256) void shuffle2_concat_kernel(const ShuffleParams p) {
    const long long cg = (long long)(2 * p.hp) >> 3;                // units per pixel
    const long long units = p.npix * cg;
    const int ug = p.hp >> 3;                                       // units per half
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < units; t += (long long)gridDim.x * 256) {
        const long long pix = t / cg;
        const int g = (int)(t - pix * cg);
        const int h = g >= ug ? 1 : 0;
        const int j0 = (g - h * ug) << 3;
        const int nv = min(8, p.bf - j0);                           // real channels of this unit (even; <= 0: a pad unit)
        h8 oh, ol;
#pragma unroll
        for (int e = 0; e < 8; ++e) { oh[e] = (half_t)0.f; ol[e] = (half_t)0.f; }
        if (nv > 0) {
            const int s0 = (h * p.bf + j0) >> 1;
            const size_t at_a = (size_t)pix * p.a_pitch + s0, at_b = (size_t)pix * p.b_pitch + s0;
            if (VEC) {              // bf % 8 == 0: nv == 8 and both sources are 8-byte aligned
                const h4 ah = *(const h4*)(p.a_hi + at_a), al = *(const h4*)(p.a_lo + at_a);
                const h4 bh = *(const h4*)(p.b_hi + at_b), bl = *(const h4*)(p.b_lo + at_b);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    oh[2 * i] = ah[i]; ol[2 * i] = al[i];
                    oh[2 * i + 1] = bh[i]; ol[2 * i + 1] = bl[i];
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (2 * i < nv) {
                        oh[2 * i] = p.a_hi[at_a + i]; ol[2 * i] = p.a_lo[at_a + i];
                        oh[2 * i + 1] = p.b_hi[at_b + i]; ol[2 * i + 1] = p.b_lo[at_b + i];
                    }
                }
            }
        }
        const size_t at_y = (size_t)pix * (2 * p.hp) + ((size_t)g << 3);
        *(h8*)(p.y_hi + at_y) = oh;
        *(h8*)(p.y_lo + at_y) = ol;
    }
}

// ------------------------------------------------------------------------------------------
// Depthwise 3x3 conv (pad 1, stride 1 or 2) + BatchNorm, LINEAR: no activation behind it and no clamp on load (ShuffleNetV2's branch1.0 /
// branch2.3 with their BatchNorms branch1.1 / branch2.4).  Operand layout and arithmetic are dwconv3x3_bn_relu6_kernel's (mpx_dw.h) minus
// its two clamps: planes [B][hin][hin][pitch] -> [B][ho][ho][pitch], ho = (hin - 1) / stride + 1; x = hi + lo exact in fp32; per output
//     acc = 0;  for ky in 0..2, kx in 0..2 (row-major):  acc = fma(w[ky * 3 + kx][c], x[iy][ix][c], acc)
// over the taps inside the map, then fl(fl(s * acc) + t) -- two roundings: the product and the sum are written with plain operators under
// `#pragma clang fp contract(off)` (the __fmul_rn / __fadd_rn of this toolchain's headers are a plain * and + compiled under the default
// contract(fast), and were fused into one fma when this kernel used them) --, the re-split and one 16-byte store per plane.
// Negative results and results above 6 pass through unchanged.  Channels of the pitch beyond the layer's own -- the gaps of a two-half map included -- carry zero weights, scale and
// shift and are written as exact zeros (their inputs are exact zeros wherever the engine produces them).
// THE RUN FORM (DESIGN.md 16 has both times): one thread = 8 channels of a run of W output pixels along x (W = 4 at stride 1, 2 at stride 2),
// as maxpool3x3_clip_kernel (mpx_pool3c.h).  Row by row it loads the run's NC = STRIDE * (W - 1) + 3 input columns once -- 18 loads per plane
// for four stride-1 outputs where one thread per output pixel issues 36 -- and feeds every output its three taps of that row, kx ascending:
// each output still sees its taps in row-major order, one fma each, so the result has the bits of the one-pixel form.  A column outside the
// map is loaded at a clamped index (inside the planes) and its fma is not taken; a row outside the map is skipped.  Only one input row (NC x 8
// values) is live at a time.
// Units (n, oy, run, 8-channel group) are 64-bit, consecutive lanes take consecutive 16-byte groups of a pixel; the grid is capped by the
// host and strides over the rest.  Offsets are 64-bit.  No atomics, no scratch (every array below is indexed by unrolled constants), no LDS.
// A kernel of its own: dwconv3x3_bn_relu6_kernel stays as it is.
// ------------------------------------------------------------------------------------------
template <int STRIDE>
struct DwRun {
    static constexpr int W = STRIDE == 1 ? 4 : 2;       // output pixels per thread
    static constexpr int NC = STRIDE * (W - 1) + 3;     // input columns under them
};

template <int STRIDE>
__global__ __launch_bounds__(256) void dwconv3x3_bn_kernel(const DwParams p) {
#pragma clang fp contract(off)
    constexpr int W = DwRun<STRIDE>::W, NC = DwRun<STRIDE>::NC;
    const long long cg = p.pitch >> 3;
    const int runs = (p.ho + W - 1) / W;
    const long long units = p.npix / p.ho * runs * cg;              // B * ho rows of `runs` runs
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
        const int iy0 = oy * STRIDE - 1, ix0 = ox0 * STRIDE - 1;
        float acc[W][8];
#pragma unroll
        for (int k = 0; k < W; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
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
                for (int j = 0; j < 8; ++j) xm[q][j] = (float)vh[j] + (float)vl[j];
            }
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float* wt = p.w + (size_t)(ky * 3 + kx) * p.pitch + c;
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
                const float v = m + sh;
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
