// mpx_occlusion.h -- occlusion sensitivity (Zeiler, Fergus, "Visualizing and Understanding Convolutional Networks", ECCV 2014; Captum's
// Occlusion, MATLAB's occlusionSensitivity): a box slides over the image, and every pixel gets the mean, over the boxes that cover it, of
// the drop of the class score from the whole image to the image with the box covered.  The boxes are staged by mpx_softmask.h's BoxWeights
// source; the two kernels here turn the scores of the rows into the map, on the device:
//   box_saliency_classes_kernel   for m ascending, for every pixel p that box m covers:
//                                     sum[k][p] <- fl(sum[k][p] + fl(base[k] - scores[m][k]))      for every class k
//                                     cnt[p]    <- cnt[p] + 1
//                                 a pixel that box m does not cover keeps sum[.][p] and cnt[p] as they are (NOT "+ 0.0": a -0.0 stays -0.0);
//   box_saliency_mean_kernel      out[k][p] = cnt[p] > 0 ? sum[k][p] / float(cnt[p]) : 0.0f        ONE correctly rounded fp32 division.
//
// Bit rules.  One rounded subtraction and one rounded addition per (class, covering box, pixel), accumulated in place from what sum and cnt
// hold, m ascending.  One thread owns a pixel and its class tile (SC_KT accumulators in registers, as saliency_classes_kernel holds them)
// for the whole launch: no atomics, no reduction tree, and the bits depend neither on the grid nor on how the rows are cut into
// consecutive calls.  cnt is counted by every class tile and written by tile 0 alone.  masks.occlusion_sums / occlusion_mean are the
// numpy restatements the kernels are held to bit for bit.
//
// The boxes are walked in tiles of OCC_BT through LDS (16 B a box; every lane reads the same box: a broadcast).  The scores of a row and
// base are the same for every thread of the block -- their addresses are built from blockIdx.y and loop counters alone, so they go through
// the scalar path --, and they are read only in a wave that has a covered lane: a 32 x 32 box covers 2 % of the pixels, so most waves
// branch over most rows and pay an LDS read and four compares for them.  base may point into scores (row 0 of the
// job is the empty box): both are only read.
#pragma once
#include "mpx_saliency_classes.h"

namespace mpx {

constexpr int OCC_BT = 256;         // boxes per LDS tile: 4 KB, one box component per thread and pass of the staging loop
constexpr int OCC_THREADS = 256;

// One thread's walk over the M boxes, tile by tile through LDS: where box m covers the pixel, n <- n + 1 and
// acc[j] <- fl(acc[j] + fl(brow[j] - srow[j])) for the tile's classes; elsewhere nothing changes (no "+ 0.0": a -0.0 stays -0.0).  The body
// sits behind `if (covered)` as ONE block: a wave with no covered lane branches over it (s_cbranch_execz) and reads no score.  FULL: the
// tile holds SC_KT classes; otherwise groups at or beyond the tile's count kt are skipped by a block-uniform branch and the index is
// clamped to the tile's last class, as spend_weight (mpx_saliency_classes.h) does it.  FULL is decided once per block, in front of the
// loops, so that the accumulators stay where they are across the rows.
template <bool FULL>
__device__ __forceinline__ void walk_boxes(float (&acc)[SC_KT], int& n, int* s_box, const int32_t* boxes, const float* srow, const int score_pitch,
                                           const float* brow, const int M, const int kt, const int y, const int x, const int tid) {
#pragma clang fp contract(off)
    for (int m_base = 0; m_base < M; m_base += OCC_BT) {
        const int mt = min(OCC_BT, M - m_base);
        for (int i = tid; i < mt * 4; i += OCC_THREADS) s_box[i] = boxes[(size_t)m_base * 4 + i];
        __syncthreads();
        for (int mi = 0; mi < mt; ++mi, srow += score_pitch) {
            const int4 b = ((const int4*)s_box)[mi];
            if ((y >= b.x) & (y < b.z) & (x >= b.y) & (x < b.w)) {     // & not &&: one 16-byte read, four compares, ONE branch
                n += 1;
#pragma unroll
                for (int g = 0; g < SC_KT; g += SC_KG) {
                    if (FULL || g < kt) {
#pragma unroll
                        for (int j = g; j < g + SC_KG; ++j) {
                            const int jj = FULL ? j : min(j, kt - 1);
                            const float t = brow[jj] - srow[jj];        // rounded difference ...
                            acc[j] = acc[j] + t;                        // ... rounded sum
                        }
                    }
                }
            }
        }
        __syncthreads();                // the tile is read out before the next one lands
    }
}

// Grid: (pixel blocks) x (ceil(K / SC_KT) class tiles).  sum = f32[K][size][size], cnt = i32[size][size], boxes = i32[M][4] half-open
// (y0, x0, y1, x1), compared against and never an index; scores = f32[M][score_pitch], base = f32[K].  A lane beyond the image walks as
// pixel 0 and stores nothing: every thread of the block meets the barriers.
__global__ __launch_bounds__(OCC_THREADS) void box_saliency_classes_kernel(const int32_t* boxes, const float* scores, const int score_pitch,
                                                                           const float* base, const int M, const int K, float* sum,
                                                                           int32_t* cnt, const int size) {
    __shared__ __attribute__((aligned(16))) int s_box[OCC_BT * 4];
    const int tid = threadIdx.x;
    const int hw = size * size;
    const int pix = blockIdx.x * OCC_THREADS + tid;
    const bool active = pix < hw;
    const int cp = active ? pix : 0;
    const int y = cp / size, x = cp - y * size;
    const int k0 = blockIdx.y * SC_KT;
    const int kt = min(SC_KT, K - k0);  // 1 .. SC_KT classes in this tile
    float* out = sum + (size_t)k0 * hw + cp;
    float acc[SC_KT];
#pragma unroll
    for (int j = 0; j < SC_KT; ++j) acc[j] = (active && j < kt) ? out[(size_t)j * hw] : 0.0f;
    int n = cnt[cp];
    if (kt == SC_KT) walk_boxes<true>(acc, n, s_box, boxes, scores + k0, score_pitch, base + k0, M, kt, y, x, tid);
    else walk_boxes<false>(acc, n, s_box, boxes, scores + k0, score_pitch, base + k0, M, kt, y, x, tid);
#pragma unroll
    for (int j = 0; j < SC_KT; ++j)
        if (active && j < kt) out[(size_t)j * hw] = acc[j];
    if (active && blockIdx.y == 0) cnt[cp] = n;
}

// out[k][p] = cnt[p] > 0 ? sum[k][p] / float(cnt[p]) : 0.0f.  Grid: (pixel blocks) x (up to 1024 rows of classes, strided).  out may be
// sum: a thread reads the element it writes, and no other.
__global__ __launch_bounds__(256) void box_saliency_mean_kernel(const float* sum, const int32_t* cnt, const int K, float* out, const int hw) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const int n = cnt[pix];
    const float fn = (float)n;
    for (int k = blockIdx.y; k < K; k += gridDim.y) {
        const size_t o = (size_t)k * hw + pix;
        out[o] = n > 0 ? __fdiv_rn(sum[o], fn) : 0.0f;
    }
}

}  // namespace mpx
