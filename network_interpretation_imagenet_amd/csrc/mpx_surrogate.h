// mpx_surrogate.h -- the moment sums of a linear surrogate over on/off superpixel rows (LIME, KernelSHAP), and the paint of a value per
// superpixel onto the pixels.
//
// Both explainers fit  score ~ c0 + sum_j c_j * z_j  to random coalitions z in {0, 1}^S.  With z~_m = (1, z_m) and a weight per row the
// fit needs two sums over the rows,  A = sum_m w_m z~_m z~_m^T  (f64[S+1][S+1])  and  B = sum_m w_m z~_m score_m^T  (f64[S+1][K]); the
// solve of the (S+1)^2 system stays on the host (masks.lime_solve / masks.shap_solve).  fp32 sums move the coefficients of a system of
// condition 2.5e4 by 1e-4 on a scale of 0.02, sequential fp64 sums by 4e-14, so:
//   surrogate_accumulate_kernel<true>    A[i][j] <- fl64(A[i][j] + (double)w_m)                          where z~_mi and z~_mj are on
//   surrogate_accumulate_kernel<false>   B[i][k] <- fl64(B[i][k] + (double)w_m * (double)scores[m][k])   where z~_mi is on
//   segment_paint_kernel                 out[k][p] = value[k][seg[p]], +0.0f for a label outside [0, S)
//
// Bit rules.  m ascending from the value already in A / B, one fp64 rounding per step: the product of two fp32 numbers has 48 significant
// bits and is exact in fp64, so the multiply-add below and an FMA give the same bits.  An element whose condition is off is not touched:
// the weight and the scores of such a row, NaN included, reach nothing.  One thread owns a row i and a tile of SUR_KT columns whose
// accumulators stay in registers for the whole launch (64 VGPRs of fp64, as mpx_saliency_classes.h's tile): no atomics, no reduction tree,
// and the bits depend neither on the grid nor on how the rows are cut into consecutive calls.  masks.surrogate_sums restates it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mpx {

constexpr int SUR_S_MAX = 1024;     // superpixels: A is at most 1025 x 1025 fp64 = 8.4 MB
constexpr int SUR_KT = 32;          // columns (classes of B, columns of A) per thread
constexpr int SUR_KG = 8;           // a tile is walked in groups behind a block-uniform branch, so K = 1 or 5 pays one group
constexpr int SUR_MT = 64;          // mask rows staged through the LDS at a time
constexpr int SUR_LB = 16;          // loads a lane keeps in flight while a stage lands (SUR_MT is a multiple of 2 * SUR_LB)
constexpr int SUR_THREADS = 64;     // one wave = 64 rows of the matrix; the lanes' on/off bytes are 64 consecutive bytes of a mask row

struct SurParams {
    const uint8_t* onoff;           // u8[M][S], non-zero = on
    const float* weight;            // f32[M]
    const float* scores;            // f32[M][score_pitch]  (B only)
    double* out;                    // A f64[S+1][S+1] or B f64[S+1][K]
    int score_pitch, M, S, K;
};

// MOMENT = true: out = A, the column condition is z~_mj and the term is the weight.  MOMENT = false: out = B, every column is on and the
// term is weight * score.  Grid: (ceil((S + 1) / SUR_THREADS) row blocks) x (ceil(columns / SUR_KT) column tiles).
// Per stage of SUR_MT mask rows the block lands in the LDS, reading each byte of its part of onoff once:
//   rowon[mi][t]   z~ of row i0 + t                     (the lane's own condition)
//   colmask[mi]    bit jj = z~ of column k0 + jj        (MOMENT; the same for every lane: one ballot per two mask rows)
//   wgt[mi]        (double)weight[m]                    (MOMENT)
//   term[mi][jj]   (double)weight[m] * (double)scores[m][k0 + jj], 0.0 at and beyond the tile's count kt   (B)
// A lane walks the masks one after the other, so what a stage costs is the latency of its loads: they are issued SUR_LB at a time into
// registers and stored behind the batch, never one load, one wait, one store.  The index of a mask row beyond the stage's count mt is
// clamped to its last row (read again, stored, never consumed).  Nothing is read beyond scores[..][K); the accumulators of the columns at
// and beyond kt are never stored.
template <bool MOMENT>
__global__ __launch_bounds__(SUR_THREADS) void surrogate_accumulate_kernel(const SurParams p) {
    __shared__ double term[MOMENT ? 1 : SUR_MT][SUR_KT];
    __shared__ double wgt[SUR_MT];
    __shared__ uint32_t colmask[SUR_MT];
    __shared__ uint8_t rowon[SUR_MT][SUR_THREADS];
    const uint8_t* __restrict__ onoff = p.onoff;
    const float* __restrict__ weight = p.weight;
    const float* __restrict__ scores = p.scores;
    const int t = threadIdx.x;
    const int S = p.S, n = S + 1;
    const int ncol = MOMENT ? n : p.K;
    const int i = blockIdx.x * SUR_THREADS + t;
    const bool active = i < n;          // no early return: every thread of the block meets the barriers below
    const int k0 = blockIdx.y * SUR_KT;
    const int kt = min(SUR_KT, ncol - k0);      // 1 .. SUR_KT columns in this tile
    const int half = t >> 5, jj = t & 31, j = k0 + jj;      // the staging of the columns: lanes 0 .. 31 take one mask row, 32 .. 63 the next
    const bool col = jj < kt;
    // every staging load is unconditional, so that a batch is issued back to back: the index is clamped into the row and the value dropped
    const int ic = active ? max(i - 1, 0) : 0;              // the lane's own byte of a mask row (row 0 is the intercept: always on)
    const int jc = col ? max(j - 1, 0) : 0;                 // the byte of column j of A
    const int kc = k0 + min(jj, kt - 1);                    // the score of column jj of B
    double* out = p.out + (size_t)(active ? i : 0) * ncol + k0;
    double acc[SUR_KT];
#pragma unroll
    for (int c = 0; c < SUR_KT; ++c) acc[c] = (active && c < kt) ? out[c] : 0.0;
    for (int m_base = 0; m_base < p.M; m_base += SUR_MT) {
        const int mt = min(SUR_MT, p.M - m_base);
        for (int b = 0; b < mt; b += SUR_LB) {
            uint8_t v[SUR_LB];
#pragma unroll
            for (int u = 0; u < SUR_LB; ++u)
                v[u] = onoff[(size_t)(m_base + min(b + u, mt - 1)) * S + ic];
#pragma unroll
            for (int u = 0; u < SUR_LB; ++u) rowon[b + u][t] = (active && (i == 0 || v[u] != 0)) ? 1 : 0;
        }
        if (MOMENT) {
            if (t < mt) wgt[t] = (double)weight[m_base + t];
            for (int b = 0; b < mt; b += 2 * SUR_LB) {
                uint8_t v[SUR_LB];
#pragma unroll
                for (int u = 0; u < SUR_LB; ++u)
                    v[u] = onoff[(size_t)(m_base + min(b + 2 * u + half, mt - 1)) * S + jc];
#pragma unroll
                for (int u = 0; u < SUR_LB; ++u) {
                    const unsigned long long bal = __ballot(col && b + 2 * u + half < mt && (j == 0 || v[u] != 0));
                    if (t == 0) {
                        colmask[b + 2 * u] = (uint32_t)bal;
                        colmask[b + 2 * u + 1] = (uint32_t)(bal >> 32);
                    }
                }
            }
        } else {
            for (int b = 0; b < mt; b += 2 * SUR_LB) {
                float w[SUR_LB], sc[SUR_LB];
#pragma unroll
                for (int u = 0; u < SUR_LB; ++u) {
                    const size_t m = (size_t)(m_base + min(b + 2 * u + half, mt - 1));
                    w[u] = weight[m];
                    sc[u] = scores[m * p.score_pitch + kc];
                }
#pragma unroll
                for (int u = 0; u < SUR_LB; ++u) term[MOMENT ? 0 : b + 2 * u + half][jj] = col ? (double)w[u] * (double)sc[u] : 0.0;
            }
        }
        __syncthreads();
        for (int mi = 0; mi < mt; ++mi) {
            const double w = MOMENT ? wgt[mi] : 0.0;
            const uint32_t cm = MOMENT ? __builtin_amdgcn_readfirstlane(colmask[mi]) : 0xffffffffu;     // the same word in every lane
            if (rowon[mi][t] != 0) {
#pragma unroll
                for (int g = 0; g < SUR_KT; g += SUR_KG) {
                    if (g < kt) {
#pragma unroll
                        for (int c = g; c < g + SUR_KG; ++c)
                            if ((cm >> c) & 1u) acc[c] = acc[c] + (MOMENT ? w : term[MOMENT ? 0 : mi][c]);
                    }
                }
            }
        }
        __syncthreads();        // the stage is read out before the next one lands
    }
#pragma unroll
    for (int c = 0; c < SUR_KT; ++c)
        if (active && c < kt) out[c] = acc[c];
}

// out[k][p] = value[k * value_pitch + seg[p]], +0.0f where seg[p] lies outside [0, S).  Grid: (pixel blocks) x K.
__global__ __launch_bounds__(256) void segment_paint_kernel(const int32_t* __restrict__ seg, const float* __restrict__ value,
                                                            const int value_pitch, const int S, const int npix, float* __restrict__ out) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= npix) return;
    const int k = blockIdx.y;
    const int s = seg[pix];
    out[(size_t)k * npix + pix] = (unsigned)s < (unsigned)S ? value[(size_t)k * value_pitch + s] : 0.0f;
}

}  // namespace mpx
