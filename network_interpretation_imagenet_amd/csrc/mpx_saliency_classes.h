// mpx_saliency_classes.h -- RISE's estimator for many classes from the same forwards: a head that gathers K classes of every row, and the
// score-weighted sum of the masks (mpx_softmask.h) with a tile of classes per thread.
//
// mpx_softmask.h sums one class: sal[p] <- sal[p] + score[m] * w_m(p).  A second class through that kernel synthesises every weight w_m(p)
// again (two integer axes, two fp32 divisions, four LDS bytes) for one multiply and one add.  RISE's estimator is sal[k] = sum_m
// p_k(I * M_m) * M_m for EVERY class k of the same forwards, so the two kernels here
//   softmax_gather_classes_kernel   scores[b][k] = softmax(logits[b])[classes[k]]: the single-label head's arithmetic, K outputs per row;
//   saliency_classes_kernel<WS>     sal[k][p] <- fl(sal[k][p] + fl(scores[m][k] * w_m(p))), m ascending: w_m(p) is computed (or read) ONCE
//                                   per mask and pixel and spent on SC_KT classes whose accumulators stay in registers.
//
// Bit rules.  Both are restatements of kernels that exist, and are held to them bit for bit:
//   head       one wave per row, lane l takes columns l, l + 64, ..; the max and the sum are reduced in head_softmax_gather_kernel's order
//              (sequential per lane, then xor-shuffles 32, 16, .., 1); the terms are expf(row[i] - mx), the output is
//              __fdiv_rn(expf(row[c] - mx), sum).  After the xor reduction every lane holds mx and sum, so the lanes write the K outputs in
//              parallel.  scores[b][k] IS mpx_head_softmax_gather's score[b] for label[b] = classes[k]; a class outside [0, ncls) gives 0.0f.
//   sum        a multiply and an add per (class, mask, pixel), each rounded to fp32 on its own (contraction off), m ascending from the value
//              already in sal; w_m(p) comes from mpx_softmask.h's weight sources unchanged.  Map k IS mpx_rise_saliency /
//              mpx_softmask_saliency run with weight[m] = scores[m][k].  One thread owns a pixel and its class tile for the whole launch: no
//              atomics, no reduction tree, and the bits depend neither on the grid nor on how the rows are cut into consecutive calls.
#pragma once
#include "mpx_softmask.h"

namespace mpx {

// The class tile.  32 accumulators beside the RISE weight's registers: the kernel's resource line (profiles/rise_classes_kernel_resources.txt)
// stays under the 128 VGPRs at which a SIMD still holds four waves, and the weight is amortised over 32 classes.  A tile is walked in
// groups of SC_KG classes behind a block-uniform branch, so that K = 1 or 5 pays one group's multiply-adds and not the tile's.
constexpr int SC_KT = 32;
constexpr int SC_KG = 8;
constexpr int SC_THREADS = 256;     // four waves stage the RISE cells of a mask tile (up to 32 KB at s = 32) instead of one

// K4b's arithmetic with K gathers per row in place of one (and no argmax output: mpx_forward's head writes it).  The argmax is still carried
// through the max reduction exactly as K4b carries it, so that mx is the same value down to the sign of a zero.
__global__ __launch_bounds__(256) void softmax_gather_classes_kernel(const float* __restrict__ logits, const int32_t* __restrict__ classes,
                                                                     int K, float* __restrict__ scores, int score_pitch, int B, int ncls,
                                                                     int pitch) {
    const int lane = threadIdx.x & 63;
    const int img = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (img >= B) return;
    const float* row = logits + (size_t)img * pitch;
    float mx = -INFINITY;
    int arg = 0;
    for (int i = lane; i < ncls; i += 64) {
        const float v = row[i];
        if (v > mx) { mx = v; arg = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float omx = __shfl_xor(mx, off);
        const int oarg = __shfl_xor(arg, off);
        if (omx > mx || (omx == mx && oarg < arg)) { mx = omx; arg = oarg; }
    }
    float sum = 0.f;
    for (int i = lane; i < ncls; i += 64) sum += expf(row[i] - mx);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    float* out = scores + (size_t)img * score_pitch;
    for (int k = lane; k < K; k += 64) {            // the padding [K, score_pitch) is not written
        const int c = classes ? classes[k] : k;
        const bool ok = (unsigned)c < (unsigned)ncls;
        out[k] = ok ? __fdiv_rn(expf(row[c] - mx), sum) : 0.f;
    }
}

// One weight spent on the tile: acc[j] <- fl(acc[j] + fl(srow[j] * w)).  srow is the same for every thread of the block.  FULL: the tile
// holds SC_KT classes and its scores are SC_KT consecutive floats, read without a branch.  Otherwise groups at or beyond the tile's
// count kt are skipped by a block-uniform branch and the index is clamped to the tile's last class.
template <bool FULL>
__device__ __forceinline__ void spend_weight(float (&acc)[SC_KT], const float* srow, const float w, const int kt) {
#pragma clang fp contract(off)
#pragma unroll
    for (int g = 0; g < SC_KT; g += SC_KG) {
        if (FULL || g < kt) {
#pragma unroll
            for (int j = g; j < g + SC_KG; ++j) {
                const float t = srow[FULL ? j : min(j, kt - 1)] * w;    // rounded product ...
                acc[j] = acc[j] + t;                                    // ... rounded sum: not an FMA
            }
        }
    }
}

// sal[k][p] <- fl(sal[k][p] + fl(scores[m * score_pitch + k] * w_m(p))), m ascending.  p.score = scores, p.sal = f32[K][H][W].
// Grid: (pixel blocks) x (ceil(K / SC_KT) class tiles).  The SC_KT scores of a mask are the same for every thread of the block: their
// address is built from blockIdx.y and the loop counter alone, so the loads go through the scalar path and cost no vector register and no
// per-lane gather.  The class tail: groups at or beyond the tile's count kt are skipped by a block-uniform branch, and inside the last
// group the score index is clamped to the tile's last class -- nothing is read beyond scores[..][K), the accumulators of the clamped
// columns are never stored, nothing is read or written beyond sal[K).
template <class WS>
__global__ __launch_bounds__(SC_THREADS) void saliency_classes_kernel(const SoftParams p, const int score_pitch, const int K) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int hw = p.size * p.size;
    const int pix = blockIdx.x * SC_THREADS + tid;
    const bool active = pix < hw;       // no early return: every thread of the block meets the barriers below
    const int cp = active ? pix : 0;
    const int y = cp / p.size, x = cp - y * p.size;
    const int k0 = blockIdx.y * SC_KT;
    const int kt = min(SC_KT, K - k0);  // 1 .. SC_KT classes in this tile
    float* sal = p.sal + (size_t)k0 * hw + cp;
    float acc[SC_KT];
#pragma unroll
    for (int j = 0; j < SC_KT; ++j) acc[j] = (active && j < kt) ? sal[(size_t)j * hw] : 0.0f;
    const typename WS::Pixel px = WS::pixel(p, cp);
    for (int m_base = 0; m_base < p.M; m_base += STAGE_MT) {
        const int mt = min(STAGE_MT, p.M - m_base);
        if (WS::kLds) {
            WS::stage(p, smem, m_base, mt, tid, SC_THREADS);
            __syncthreads();
        }
        for (int mi = 0; mi < mt; ++mi) {
            const float w = WS::weight(p, smem, px, m_base + mi, mi, cp, y, x, hw);
            const float* srow = p.score + (size_t)(m_base + mi) * score_pitch + k0;
            if (kt == SC_KT) spend_weight<true>(acc, srow, w, kt);
            else spend_weight<false>(acc, srow, w, kt);
        }
        if (WS::kLds) __syncthreads();  // the tile is read out before the next one lands
    }
#pragma unroll
    for (int j = 0; j < SC_KT; ++j)
        if (active && j < kt) sal[(size_t)j * hw] = acc[j];
}

}  // namespace mpx
