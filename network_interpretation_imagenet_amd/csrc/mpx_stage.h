// mpx_stage.h -- what every kernel that fills the engine's input slots shares: the normalised pixel, and one pixel of one slot.
//
// The normalised pixel is written ONCE, here: u8 -> /255 -> -mean -> /std, each op rounded in fp32 (torchvision's ToTensor .div(255) and
// Normalize .sub_(mean).div_(std)), or the f32 as given.  load_normalized_pixel serves softmask_apply_kernel<WS> (mpx_softmask.h) and
// stemtab_fill_kernel (mpx_stemtab.h); rank_apply_kernel and blur_fill_kernel (mpx_rankmask.h) call normalize_u8 per channel.
//
// A slot is [pad_size][pad_size][4] fp16 per plane (padded NHWC4, the 7x7 stem's operand): pixel (y, x) lies at
// ((y + border) * pad_size + (x + border)) * 4, channel 3 is +0.0 (staged_h4), the border is never written.  store_staged_pixel is the
// two 8-byte h4 stores of one pixel of slot slot0 + m and, where asked for, out_f32[m][c][pix] (rank_apply_kernel spells the same stores
// out in its own loop: mpx_rankmask.h says why).
//
// split_f32 (mpx_conv.h) holds a conversion, a subtraction and a conversion -- no multiply --, so there is nothing in it to contract: it
// is the same arithmetic inside and outside `#pragma clang fp contract(off)`.  What a kernel has to keep apart is its OWN product in front
// of the split (fp32_value, mpx_conv.h).
#pragma once
#include "mpx_conv.h"

namespace mpx {

constexpr int STAGE_MT = 32;        // rows per block tile of every apply kernel: a block reads its pixels once per 32 rows

// ToTensor: u8 -> f32, .div(255); Normalize: .sub_(mean).div_(std); each op rounds in fp32
__device__ __forceinline__ float normalize_u8(uint8_t b, float mean, float std) {
    const float t = __fdiv_rn((float)b, 255.0f);
    return __fdiv_rn(__fsub_rn(t, mean), std);
}

// v[c] = the normalised pixel `pix` of an image given as u8 [H][W][3] or as f32 [3][H][W] (hw = H * W); exactly one pointer is non-null
__device__ __forceinline__ void load_normalized_pixel(const uint8_t* img_u8, const float* img_f32, const float mean[3], const float std[3],
                                                      size_t pix, int hw, float v[3]) {
    if (img_u8) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = normalize_u8(img_u8[pix * 3 + c], mean[c], std[c]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = img_f32[(size_t)c * hw + pix];
    }
}

// where pixel (y, x) lies inside a slot, in fp16 elements
template <class P>
__device__ __forceinline__ size_t staged_pixel_offset(const P& p, int y, int x) {
    return ((size_t)(y + p.border) * p.pad_size + (x + p.border)) * 4;
}

// one plane's 8 bytes of a staged pixel: the three channels of a split triple and +0.0 in channel 3
__device__ __forceinline__ h4 staged_h4(const half_t c[3]) { return h4{c[0], c[1], c[2], (half_t)0.f}; }

// One pixel of slot p.slot0 + m from an already split triple packed by staged_h4: hi, then lo (plain stores: the stem reads these planes
// next, out of L2 / Infinity Cache), then o into out_f32 when given.  P: any params struct with out_hi / out_lo / out_f32 / slot0 / pad_size.
template <class P>
__device__ __forceinline__ void store_staged_pixel(const P& p, int m, size_t pad_off, int pix, int hw, h4 oh, h4 ol, const float o[3]) {
    const size_t plane = (size_t)p.pad_size * p.pad_size * 4;
    const size_t so = (size_t)(p.slot0 + m) * plane + pad_off;
    *(h4*)(p.out_hi + so) = oh;
    *(h4*)(p.out_lo + so) = ol;
    if (p.out_f32) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p.out_f32[((size_t)m * 3 + c) * hw + pix] = o[c];
    }
}

}  // namespace mpx
