// mpx_cam.h -- Score-CAM (Wang, Wang, Du, Yang, Zhang, Ding, Mardziel, Hu, "Score-CAM: Score-Weighted Visual Explanations for
// Convolutional Neural Networks", CVPR-W 2020; ScoreCAM in pytorch-grad-cam): the masks are the network's own activation maps.  Every
// channel of the map the global pool reads is upsampled to 224 x 224, normalised to [0, 1] and scored as a mask; the class activation map
// is the score-weighted sum of the raw channels.  The rows are staged by mpx_softmask.h's MapWeights source; the kernels here are the rest:
//   planes_to_chw_kernel<LOAD>   the tap: the [g * g][pitch] hi / lo planes of one slot of the pool's input -> act f32[C][g][g],
//                                act[c][cell] = LOAD(fl(f32(hi) + f32(lo))), LOAD what global_avgpool_kernel<LOAD> (mpx_kernels.h) applies as
//                                it loads -- nothing, fminf(x, 6), silu_f32(x) -- in that kernel's own expression.  Only the C logical
//                                channels are read.  A transpose: a 32 x 32 tile goes through LDS, so that the reads run along the
//                                channels and the writes along the cells;
//   cam_cells_kernel             per channel c: lo_c / hi_c = min / max over the 224 x 224 values of up(act_c) (NOT over the g * g cells: the
//                                published code normalises the upsampled map, and an interior peak is not reached by any pixel centre),
//                                valid_c = (max cell > min cell) && (hi_c > lo_c), cells_c = fl(fl(act_c - lo_c) / fl(hi_c - lo_c)) where
//                                valid and +0.0 elsewhere.  One workgroup per channel, the cells and one axis table in LDS; min and max are
//                                exact, so the reduction tree does not show in the bits;
//   cam_low_kernel               low[k][cell] = the sum over r = 0 .. R - 1, in this order, of fl(scores[r][k] * act_r[cell]), from +0.0,
//                                each step fl(low + fl(product)): one thread per (k, cell) walks the rows -- no atomics, no tree;
//   cam_sal_kernel               sal[k][p] = v > 0 ? v : +0.0 with v = up(low[k])(p).
//
// up(G)(y, x), G f32[g][g], 2 <= g <= 16 -- bilinear, half-pixel centres, g -> 224; RISE's construction (mpx_softmask.h) with no shift and
// U = 224:
//   t  = max((2y + 1) * g - 224, 0);  i0 = t / 448;  r = t - 448 * i0;  fy = fl(float(r) / 448.0f);  i1 = min(i0 + 1, g - 1)     (x likewise)
//   top = fl(fl(fl(1 - fx) * G[i0][j0]) + fl(fx * G[i0][j1]));  bot the same on row i1;  up = fl(fl(fl(1 - fy) * top) + fl(fy * bot))
// Every product and sum is rounded on its own (contraction off).  t <= 447 * 16 - 224 and i0 <= g - 1 for every y in [0, 224).  This is
// torch.nn.functional.interpolate(G, size=(224, 224), mode="bilinear", align_corners=False) up to rounding; masks.cam_upsample / cam_cells /
// cam_weights / cam_combine are the numpy fp32 restatements the kernels are held to bit for bit.
#pragma once
#include "mpx_kernels.h"
#include "mpx_softmask.h"      // cam_axis, cam_up, CAM_G_MIN / CAM_G_MAX / CAM_IMG: the upsampling the MapWeights source shares

namespace mpx {

constexpr int CAM_T = 32;           // the tap's transpose tile

// The tap.  Grid: (ceil(C / 32), ceil(hw / 32)), 256 threads.  in_hi / in_lo point at the slot's [hw][pitch] planes.
template <PoolLoad LOAD>
__global__ __launch_bounds__(256) void planes_to_chw_kernel(const half_t* __restrict__ in_hi, const half_t* __restrict__ in_lo, const int hw,
                                                            const int C, const int pitch, float* __restrict__ out) {
    __shared__ float tile[CAM_T][CAM_T + 1];
    const int tx = threadIdx.x & (CAM_T - 1), ty = threadIdx.x / CAM_T;        // ty in [0, 8)
    const int c0 = blockIdx.x * CAM_T, p0 = blockIdx.y * CAM_T;
#pragma unroll
    for (int k = 0; k < CAM_T; k += 8) {
        const int cell = p0 + ty + k, c = c0 + tx;
        if (cell < hw && c < C) {
            const size_t o = (size_t)cell * pitch + c;
            const float x = (float)in_hi[o] + (float)in_lo[o];
            tile[ty + k][tx] = LOAD == POOL_CLAMP6 ? fminf(x, 6.f) : LOAD == POOL_SILU ? silu_f32(x) : x;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CAM_T; k += 8) {
        const int c = c0 + ty + k, cell = p0 + tx;
        if (c < C && cell < hw) out[(size_t)c * hw + cell] = tile[tx][ty + k];
    }
}

// min and max of four values across the block's four waves: a wave reduction by shuffles, then 4 x 4 floats through LDS.  Every thread
// returns with the block's values.  min and max are exact: no order shows.
__device__ __forceinline__ void cam_block_minmax(float (&v)[4], float (*s_red)[4], int tid) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v[0] = fminf(v[0], __shfl_xor(v[0], off));
        v[1] = fmaxf(v[1], __shfl_xor(v[1], off));
        v[2] = fminf(v[2], __shfl_xor(v[2], off));
        v[3] = fmaxf(v[3], __shfl_xor(v[3], off));
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s_red[tid >> 6][j] = v[j];
    }
    __syncthreads();
    v[0] = fminf(fminf(s_red[0][0], s_red[1][0]), fminf(s_red[2][0], s_red[3][0]));
    v[1] = fmaxf(fmaxf(s_red[0][1], s_red[1][1]), fmaxf(s_red[2][1], s_red[3][1]));
    v[2] = fminf(fminf(s_red[0][2], s_red[1][2]), fminf(s_red[2][2], s_red[3][2]));
    v[3] = fmaxf(fmaxf(s_red[0][3], s_red[1][3]), fmaxf(s_red[2][3], s_red[3][3]));
}

// One workgroup of 256 threads per channel (blockIdx.x = c).  act f32[C][g][g] -> cells f32[C][g][g], lo / hi f32[C], valid u8[C].
__global__ __launch_bounds__(256) void cam_cells_kernel(const float* __restrict__ act, const int g, float* __restrict__ cells,
                                                        float* __restrict__ lo, float* __restrict__ hi, uint8_t* __restrict__ valid) {
#pragma clang fp contract(off)
    __shared__ float s_g[CAM_G_MAX * CAM_G_MAX];
    __shared__ int s_a0[CAM_IMG], s_a1[CAM_IMG];      // one axis: i0, i1 (the same table serves y and x: there is no shift)
    __shared__ float s_f[CAM_IMG];
    __shared__ float s_red[4][4];
    const int tid = threadIdx.x;
    const int gg = g * g;
    const size_t base = (size_t)blockIdx.x * gg;
    float mine = 0.f;
    if (tid < gg) {
        mine = act[base + tid];
        s_g[tid] = mine;
    }
    if (tid < CAM_IMG) {
        int i0, i1;
        float f;
        cam_axis(tid, g, i0, i1, f);
        s_a0[tid] = i0; s_a1[tid] = i1; s_f[tid] = f;
    }
    __syncthreads();
    float v[4];                         // min / max of the upsampled map, min / max of the cells
    v[0] = INFINITY; v[1] = -INFINITY;
    v[2] = tid < gg ? mine : INFINITY;
    v[3] = tid < gg ? mine : -INFINITY;
    for (int pix = tid; pix < CAM_IMG * CAM_IMG; pix += 256) {
        const int y = pix / CAM_IMG, x = pix - y * CAM_IMG;
        const float u = cam_up(s_g, s_a0[y] * g, s_a1[y] * g, s_a0[x], s_a1[x], s_f[y], s_f[x]);
        v[0] = fminf(v[0], u);
        v[1] = fmaxf(v[1], u);
    }
    cam_block_minmax(v, s_red, tid);
    const bool ok = (v[3] > v[2]) && (v[1] > v[0]);
    if (tid < gg) {
        const float num = mine - v[0], den = v[1] - v[0];     // each rounded; then ONE correctly rounded division
        cells[base + tid] = ok ? __fdiv_rn(num, den) : 0.0f;
    }
    if (tid == 0) {
        lo[blockIdx.x] = v[0];
        hi[blockIdx.x] = v[1];
        valid[blockIdx.x] = ok ? 1 : 0;
    }
}

// low[k][cell] <- the sum of fl(scores[r * score_pitch + k] * act[r][cell]) over r ascending, from +0.0.  One thread per (k, cell).
__global__ __launch_bounds__(256) void cam_low_kernel(const float* __restrict__ act, const float* __restrict__ scores, const int score_pitch,
                                                      const int R, const int gg, const int K, float* __restrict__ low) {
#pragma clang fp contract(off)
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= K * gg) return;
    const int k = idx / gg, cell = idx - k * gg;
    const float* a = act + cell;
    const float* s = scores + k;
    float acc = 0.0f;
    for (int r = 0; r < R; ++r) {
        const float t = s[(size_t)r * score_pitch] * a[(size_t)r * gg];       // rounded product ...
        acc = acc + t;                                                      // ... rounded sum: not an FMA
    }
    low[idx] = acc;
}

// sal[k][p] = max(up(low[k])(p), +0.0) as a select.  Grid: (pixel blocks) x (up to 1024 class rows, strided); low[k] sits in LDS.
__global__ __launch_bounds__(256) void cam_sal_kernel(const float* __restrict__ low, const int g, const int K, float* __restrict__ sal) {
    __shared__ float s_g[CAM_G_MAX * CAM_G_MAX];
    const int tid = threadIdx.x;
    const int gg = g * g;
    const int pix = blockIdx.x * 256 + tid;
    const bool active = pix < CAM_IMG * CAM_IMG;        // no early return: every thread of the block meets the barriers below
    const int cp = active ? pix : 0;
    const int y = cp / CAM_IMG, x = cp - y * CAM_IMG;
    int i0, i1, j0, j1;
    float fy, fx;
    cam_axis(y, g, i0, i1, fy);
    cam_axis(x, g, j0, j1, fx);
    for (int k = blockIdx.y; k < K; k += gridDim.y) {
        if (tid < gg) s_g[tid] = low[(size_t)k * gg + tid];
        __syncthreads();
        const float v = cam_up(s_g, i0 * g, i1 * g, j0, j1, fy, fx);
        if (active) sal[(size_t)k * (CAM_IMG * CAM_IMG) + pix] = v > 0.0f ? v : 0.0f;
        __syncthreads();                // the map is read out before the next one lands
    }
}

}  // namespace mpx
