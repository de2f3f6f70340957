// mpx_shuffle.h -- ShuffleNetV2's channel shuffle of a two-way concatenation on split-fp16 NHWC planes, gfx950.  (Its depthwise 3x3 conv +
// BatchNorm with NO activation behind it is the run form of mpx_dw.h, dwconv_bn_act_kernel<3, STRIDE, false>.)
//
// The two-half layout.  A ShuffleNetV2 stage map has 2 * bf logical channels (bf = oup / 2) and every block splits it into its first and
// second half.  It is stored with a pitch of 2 * hp, hp = bf rounded up to 32: logical channel l < bf at physical l, l >= bf at
// hp + (l - bf); physical channels [bf, hp) and [hp + bf, 2 hp) are exact zeros, written by every forward.  Both halves are then contiguous,
// 16-byte aligned and a whole number of 32-wide K steps: a stride-1 block's branch2.0 reads the second half in place (pointer + hp,
// pix_stride 2 hp, K = hp) and the shuffle reads the first half in place.
#pragma once
#include "mpx_conv.h"

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

}  // namespace mpx
