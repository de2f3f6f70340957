// mpx_kernels.h -- gfx950 (MI355X, CDNA4) device kernels of the masked-perturbation scorer.
//
// Data format between kernels ("split-fp16"): an activation tensor is two fp16 NHWC planes
// hi, lo with x ~= hi + lo (22 significant bits).  A convolution is the implicit GEMM
//   D[cout][pixel] = sum_k W[cout][k] * X[pixel][k],  k = (ky, kx, ci)
// issued on the fp16 MFMA pipe as three products  W_hi*X_lo + W_lo*X_hi + W_hi*X_hi  with
// fp32 accumulation (v_mfma_f32_16x16x32_f16), which reproduces fp32 convolution to ~1e-7
// relative (oracle/precision_study.py) at 1/3 of the fp16 MFMA rate = 5.3x the f32 MFMA rate.
//
// Here: the pools, the head and the small networks' kernels.  K0 (mask-apply + normalise) is softmask_apply_kernel<OnoffWeights> in
// mpx_softmask.h; the pixel and the slot store every staging kernel shares are in mpx_stage.h.
#pragma once
#include "mpx_conv.h"

namespace mpx {

// ------------------------------------------------------------------------------------------
// K3: maxpool 3x3 stride 2 pad 1 on split planes (one thread = 8 channels of one output pixel)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const half_t* __restrict__ in_hi,
                                                            const half_t* __restrict__ in_lo,
                                                            half_t* __restrict__ out_hi,
                                                            half_t* __restrict__ out_lo, int B, int hin,
                                                            int c) {
    const int ho = hin / 2;
    const int cg = c / 8;
    const size_t total = (size_t)B * ho * ho * cg;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const int g = (int)(t % cg);
        size_t r = t / cg;
        const int ox = (int)(r % ho);
        r /= ho;
        const int oy = (int)(r % ho);
        const int n = (int)(r / ho);
        float best[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) best[j] = -INFINITY;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int iy = oy * 2 - 1 + dy;
            if ((unsigned)iy >= (unsigned)hin) continue;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int ix = ox * 2 - 1 + dx;
                if ((unsigned)ix >= (unsigned)hin) continue;
                const size_t o = (((size_t)n * hin + iy) * hin + ix) * c + g * 8;
                const h8 vh = *(const h8*)(in_hi + o);
                const h8 vl = *(const h8*)(in_lo + o);
#pragma unroll
                for (int j = 0; j < 8; ++j) best[j] = fmaxf(best[j], (float)vh[j] + (float)vl[j]);
            }
        }
        h8 oh, ol;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            half_t hi, lo;
            split_f32(best[j], hi, lo);
            oh[j] = hi;
            ol[j] = lo;
        }
        const size_t o = (((size_t)n * ho + oy) * ho + ox) * c + g * 8;
        *(h8*)(out_hi + o) = oh;
        *(h8*)(out_lo + o) = ol;
    }
}

// ------------------------------------------------------------------------------------------
// K3 without padding: K x K stride-2 max pool on split planes, every window inside the map.  K = 2: nn.MaxPool2d(2, 2) of the VGG family
// (hin even, ho = hin / 2).  K = 3: AlexNet's and SqueezeNet's MaxPool2d(3, 2) (hin odd, ho = (hin - 3) / 2 + 1).  One thread = 8 channels
// of one output pixel (16-byte loads and stores, grid-stride); the output pair is the (hi, lo) PAIR of the window's largest hi + lo (the
// sum of two fp16 is exact in fp32), the first in row-major window order on a tie, so the merged output equals F.max_pool2d of the merged
// planes bit for bit, for any sign.  Offsets are 64-bit: one plane of a 224x224x64 map passes 2^31 elements from 669 images on.
// ------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(256) void maxpool_s2p0_kernel(const half_t* __restrict__ in_hi,
                                                            const half_t* __restrict__ in_lo,
                                                            half_t* __restrict__ out_hi,
                                                            half_t* __restrict__ out_lo, int B, int hin,
                                                            int c) {
    const int ho = (hin - K) / 2 + 1;
    const int cg = c / 8;
    const size_t total = (size_t)B * ho * ho * cg;
    const size_t row = (size_t)hin * c;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t g = t % cg;
        const size_t pix = t / cg;                      // output pixel: (n * ho + oy) * ho + ox
        const size_t ox = pix % ho;
        const size_t ny = pix / ho;                     // n * ho + oy
        size_t i00;                                     // the window's first element: rows 2 oy .. 2 oy + K - 1 <= hin - 1, columns likewise
        if constexpr (K == 2) {                         // hin = 2 ho: input row 2 * ny of the image-stacked map, no division by ho
            i00 = ((2 * ny) * hin + 2 * ox) * c + g * 8;
        } else {
            const size_t n = ny / ho, oy = ny - n * ho;
            i00 = ((n * hin + 2 * oy) * hin + 2 * ox) * c + g * 8;
        }
        h8 bh = *(const h8*)(in_hi + i00);
        h8 bl = *(const h8*)(in_lo + i00);
        float best[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) best[j] = (float)bh[j] + (float)bl[j];
#pragma unroll
        for (int q = 1; q < K * K; ++q) {
            const size_t at = i00 + (q / K) * row + (size_t)(q % K) * c;
            const h8 vh = *(const h8*)(in_hi + at);
            const h8 vl = *(const h8*)(in_lo + at);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = (float)vh[j] + (float)vl[j];
                const bool take = v > best[j];
                best[j] = take ? v : best[j];
                bh[j] = take ? vh[j] : bh[j];
                bl[j] = take ? vl[j] : bl[j];
            }
        }
        const size_t o = pix * c + g * 8;
        *(h8*)(out_hi + o) = bh;
        *(h8*)(out_lo + o) = bl;
    }
}

// ------------------------------------------------------------------------------------------
// K4a: global average pool [B][hw][c] -> [B][c] (one thread = 8 channels of one image): the hw values are summed in pixel order in fp32
// and divided by hw once.  LOAD is what a value goes through as it is loaded: nothing; min(x, 6), the ReLU6 of the producing MFMA conv
// (MobileNetV2's features.18, mpx_dw.h); silu(x), the SiLU of the producing MFMA conv (EfficientNet's features.8).
// ------------------------------------------------------------------------------------------
enum PoolLoad { POOL_PLAIN, POOL_CLAMP6, POOL_SILU };

template <PoolLoad LOAD>
__global__ __launch_bounds__(256) void global_avgpool_kernel(const half_t* __restrict__ in_hi,
                                                              const half_t* __restrict__ in_lo,
                                                              half_t* __restrict__ out_hi,
                                                              half_t* __restrict__ out_lo, int B, int hw,
                                                              int c) {
    const int cg = c / 8;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= B * cg) return;
    const int g = t % cg, n = t / cg;
    float sum[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sum[j] = 0.f;
    for (int i = 0; i < hw; ++i) {
        const size_t o = ((size_t)n * hw + i) * c + g * 8;
        const h8 vh = *(const h8*)(in_hi + o);
        const h8 vl = *(const h8*)(in_lo + o);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = (float)vh[j] + (float)vl[j];
            sum[j] += LOAD == POOL_CLAMP6 ? fminf(x, 6.f) : LOAD == POOL_SILU ? silu_f32(x) : x;
        }
    }
    h8 oh, ol;
    const float denom = (float)hw;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        half_t hi, lo;
        split_f32(__fdiv_rn(sum[j], denom), hi, lo);
        oh[j] = hi;
        ol[j] = lo;
    }
    const size_t o = (size_t)n * c + g * 8;
    *(h8*)(out_hi + o) = oh;
    *(h8*)(out_lo + o) = ol;
}

// ------------------------------------------------------------------------------------------
// K4b: softmax + gather(label) + argmax, one wave per image
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_softmax_gather_kernel(const float* __restrict__ logits,
                                                                  const int32_t* __restrict__ label,
                                                                  float* __restrict__ score,
                                                                  int32_t* __restrict__ pred, int B,
                                                                  int ncls, int pitch) {
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
    if (lane == 0) {
        int lb = label[img];
        const bool ok = (unsigned)lb < (unsigned)ncls;
        score[img] = ok ? __fdiv_rn(expf(row[lb] - mx), sum) : 0.f;
        pred[img] = arg;
    }
}

// ------------------------------------------------------------------------------------------
// DownsampleB of the reference's CIFAR ResNet (models/resnet.py:64-74): AvgPool2d(2) on the identity, then zero
// channels up to the block's width.  Planes [B][hin][hin][cin_p] -> [B][hin/2][hin/2][cout_p]; one thread = 8 channels
// of one output pixel; the four taps are summed in torch's order (row-major) and divided by 4 in fp32.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void avgpool2_pad_kernel(const half_t* __restrict__ in_hi, const half_t* __restrict__ in_lo,
                                                           half_t* __restrict__ out_hi, half_t* __restrict__ out_lo, int B,
                                                           int hin, int cin_p, int cout_p) {
    const int ho = hin / 2, cg = cout_p / 8;
    const size_t total = (size_t)B * ho * ho * cg;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const int g = (int)(t % cg);
        size_t r = t / cg;
        const int ox = (int)(r % ho);
        r /= ho;
        const int oy = (int)(r % ho);
        const int n = (int)(r / ho);
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        if (g * 8 < cin_p) {
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const size_t o = (((size_t)n * hin + oy * 2 + dy) * hin + ox * 2 + dx) * cin_p + g * 8;
                    const h8 vh = *(const h8*)(in_hi + o);
                    const h8 vl = *(const h8*)(in_lo + o);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = __fadd_rn(acc[j], (float)vh[j] + (float)vl[j]);
                }
        }
        h8 oh, ol;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            half_t hi, lo;
            split_f32(__fdiv_rn(acc[j], 4.0f), hi, lo);
            oh[j] = hi;
            ol[j] = lo;
        }
        const size_t o = (((size_t)n * ho + oy) * ho + ox) * cout_p + g * 8;
        *(h8*)(out_hi + o) = oh;
        *(h8*)(out_lo + o) = ol;
    }
}

// ------------------------------------------------------------------------------------------
// K0 of the small networks: the CIFAR / MNIST scorers' mask convention (generate_gp_training_data_cifar.py:274-321,
// generate_gp_training_data_mnist.py:167-242): the picture is min-max scaled to [0,255] in place (x255), the SELECTED
// superpixels are switched OFF by a {0,255} mask, the product is min-max scaled to [0,255] again and multiplied by
// f32(1/255).  min(x255 * mask) is exactly 0 (x255 contains an exact 0, and 0 * anything = 0), so the second rescale
// only needs max over the KEPT pixels of fl(x255 * 255) = fl(255 * max kept x255): per-superpixel maxima once per image,
// then a max over each mask's kept superpixels.  Every fp32 operation is rounded in the reference's order.
//   stats[0] = min(x), stats[1] = fl(max(x) - min(x)), stats[2 .. 2+S) = per-superpixel max of x255, then per-mask max.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float minmax255(float x, float mn, float range) {
    return __fmul_rn(__fdiv_rn(__fsub_rn(x, mn), range), 255.0f);
}

__global__ __launch_bounds__(256) void smallnet_image_stats_kernel(const float* __restrict__ img, const int32_t* __restrict__ seg,
                                                                   int C, int hw, int S, float* __restrict__ stats) {
    __shared__ float s_mn[256], s_mx[256];
    __shared__ unsigned s_seg[4096];
    const int tid = threadIdx.x;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = tid; i < C * hw; i += 256) {
        const float v = img[i];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    s_mn[tid] = mn;
    s_mx[tid] = mx;
    for (int i = tid; i < S; i += 256) s_seg[i] = 0u;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            s_mn[tid] = fminf(s_mn[tid], s_mn[tid + o]);
            s_mx[tid] = fmaxf(s_mx[tid], s_mx[tid + o]);
        }
        __syncthreads();
    }
    const float gmn = s_mn[0];
    const float range = __fsub_rn(s_mx[0], gmn);       // = max(x - min): subtraction is monotonic
    for (int i = tid; i < C * hw; i += 256) {
        const int sgm = seg[i % hw];
        if ((unsigned)sgm < (unsigned)S) atomicMax(&s_seg[sgm], __float_as_uint(minmax255(img[i], gmn, range)));   // values >= 0
    }
    __syncthreads();
    if (tid == 0) {
        stats[0] = gmn;
        stats[1] = range;
    }
    for (int i = tid; i < S; i += 256) stats[2 + i] = __uint_as_float(s_seg[i]);
}

__global__ __launch_bounds__(256) void smallnet_mask_max_kernel(const uint8_t* __restrict__ removed, int M, int S,
                                                                const float* __restrict__ stats, float* __restrict__ mask_max) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    float mx = 0.f;                                     // removed pixels contribute 0 * x = 0
    for (int sgm = 0; sgm < S; ++sgm)
        if (!removed[(size_t)m * S + sgm]) mx = fmaxf(mx, stats[2 + sgm]);
    mask_max[m] = __fmul_rn(mx, 255.0f);                // max over pixels of fl(x255 * 255) (the product is monotonic)
}

struct SmallMaskParams {
    const float* img;        // [C][H][W] as the loader yields it
    const int32_t* seg;      // [H][W] ranks
    const uint8_t* removed;  // [M][S], 1 = superpixel switched off
    const float* stats;      // smallnet_image_stats_kernel
    const float* mask_max;   // [M]
    half_t* out_hi;          // staging [slot][H][W][32]
    half_t* out_lo;
    float* out_f32;          // [M][C][H][W] or null
    int C, hw, M, S, slot0;
};

__global__ __launch_bounds__(256) void smallnet_mask_apply_kernel(const SmallMaskParams p) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int m = blockIdx.y;
    if (pix >= p.hw) return;
    const int sgm = p.seg[pix];
    const bool keep = (unsigned)sgm < (unsigned)p.S && !p.removed[(size_t)m * p.S + sgm];
    const float mmax = p.mask_max[m];
    h8 oh, ol;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        oh[j] = (half_t)0.f;
        ol[j] = (half_t)0.f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c >= p.C) break;
        const float x255 = minmax255(p.img[(size_t)c * p.hw + pix], p.stats[0], p.stats[1]);
        const float a = __fmul_rn(x255, keep ? 255.0f : 0.0f);          // org_img * mask
        const float b = __fsub_rn(a, 0.0f);                             // masked -= masked.min()  (the minimum is exactly 0)
        const float d = __fmul_rn(__fdiv_rn(b, mmax), 255.0f);          // /= max; *= 255
        const float v = __fmul_rn(d, 0.003921568859368563f);            // normalize_image: * f32(1/255)
        half_t hi, lo;
        split_f32(v, hi, lo);
        oh[c] = hi;
        ol[c] = lo;
        if (p.out_f32) p.out_f32[((size_t)m * p.C + c) * p.hw + pix] = v;
    }
    const size_t so = ((size_t)(p.slot0 + m) * p.hw + pix) * 32;
    *(h8*)(p.out_hi + so) = oh;        // channels [0,8) of the 32 per pixel; the rest stay zero from mpx_create
    *(h8*)(p.out_lo + so) = ol;
}

// ------------------------------------------------------------------------------------------
// K5: heat-map accumulation  y[p] += sum_m [pred[m] == label[m]] * onoff[m][seg[p]]
// (gp_superpixel_data_imagenet.py:322-323 / gp_regression.py:82-94).  Two tiny launches: per-superpixel
// counts (one thread per superpixel, coalesced over s), then a gather over the 50,176 pixels.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void heatmap_segment_count_kernel(const uint8_t* __restrict__ onoff,
                                                                    const int32_t* __restrict__ pred,
                                                                    const int32_t* __restrict__ label, int M, int S,
                                                                    float* __restrict__ per_segment) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    int count = 0;
    for (int m = 0; m < M; ++m) count += (pred[m] == label[m] && onoff[(size_t)m * S + s]) ? 1 : 0;
    per_segment[s] = (float)count;
}

__global__ __launch_bounds__(256) void heatmap_gather_kernel(const int32_t* __restrict__ seg,
                                                             const float* __restrict__ per_segment, int S, int npix,
                                                             float* __restrict__ heat) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int s = seg[p];
    if ((unsigned)s < (unsigned)S) heat[p] += per_segment[s];
}

// ------------------------------------------------------------------------------------------
// DenseNet: concat-append + BatchNorm + ReLU (torchvision densenet.py: `torch.cat(features, 1)` followed by the NEXT layer's
// norm1 + relu1, a transition's norm + relu, or norm5 + relu).  A dense block keeps its running concatenation RAW (every consumer
// normalises it with statistics of its own) in planes r_* [P][c_total]; a layer's fresh channels arrive dense in f_* [P][f_stride].
// One launch walks channels [c_begin, c_end) of every pixel in units of 8 channels (16 bytes per plane per lane):
//   c <  c_old : the (hi, lo) pair is read from r_*;
//   c >= c_old : it is read from f_* (channel c - c_old) and copied into r_* bit for bit -- the append;
//   and, when y_* is given, split(relu(scale[c] * (hi + lo) + shift[c])) goes to the dense operand y_* [P][c_end] of the next conv
//   (fp32: hi + lo is exact, one multiply and one add rounded separately, then the re-split).
// f_* == NULL: normalise only (every channel from r_*); y_* == NULL: append only (c_begin = c_old).  Consecutive lanes take consecutive
// 16-byte units of a pixel, so every load and store of a wave is one contiguous run; the grid is capped (host: 8 blocks per CU) and
// strides over the rest, advancing (pixel, unit) by a fixed step without a division; offsets are 64-bit.
// ------------------------------------------------------------------------------------------
struct CatNormParams {
    const half_t* f_hi;
    const half_t* f_lo;
    half_t* r_hi;
    half_t* r_lo;
    half_t* y_hi;
    half_t* y_lo;
    const float* scale;
    const float* shift;
    long long npix;
    int f_stride, c_total, c_old, c_begin, c_end;
};

__global__ __launch_bounds__(256) void concat_bn_relu_kernel(const CatNormParams p) {
    const unsigned cg = (unsigned)(p.c_end - p.c_begin) >> 3;       // units per pixel
    const unsigned step = gridDim.x * 256u;                         // <= 2^20 units: 32-bit divisions, once
    const unsigned u0 = blockIdx.x * 256u + threadIdx.x;
    const unsigned dpix = step / cg, dk = step % cg;
    long long pix = u0 / cg;
    unsigned k = u0 % cg;
    const bool fresh = p.f_hi != nullptr, norm = p.y_hi != nullptr;
    while (pix < p.npix) {
        const int c = p.c_begin + (int)(k << 3);
        const size_t at_r = (size_t)pix * p.c_total + c;
        // one load per plane whatever the source (a wave that straddles c_old does not run two load paths one after the other); only
        // the store of the append is predicated
        const bool from_f = fresh && c >= p.c_old;
        const size_t at_f = from_f ? (size_t)pix * p.f_stride + (c - p.c_old) : 0;
        const h8 vh = *(const h8*)(from_f ? p.f_hi + at_f : p.r_hi + at_r);
        const h8 vl = *(const h8*)(from_f ? p.f_lo + at_f : p.r_lo + at_r);
        if (from_f) {
            *(h8*)(p.r_hi + at_r) = vh;
            *(h8*)(p.r_lo + at_r) = vl;
        }
        if (norm) {
            const f4 s0 = *(const f4*)(p.scale + c), s1 = *(const f4*)(p.scale + c + 4);
            const f4 t0 = *(const f4*)(p.shift + c), t1 = *(const f4*)(p.shift + c + 4);
            h8 oh, ol;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = (float)vh[j] + (float)vl[j];
                const float s = j < 4 ? s0[j & 3] : s1[j & 3], t = j < 4 ? t0[j & 3] : t1[j & 3];
                const float v = fmaxf(__fadd_rn(__fmul_rn(s, x), t), 0.f);
                half_t hi, lo;
                split_f32(v, hi, lo);
                oh[j] = hi;
                ol[j] = lo;
            }
            const size_t at_y = (size_t)pix * p.c_end + c;
            *(h8*)(p.y_hi + at_y) = oh;
            *(h8*)(p.y_lo + at_y) = ol;
        }
        pix += dpix;
        k += dk;
        if (k >= cg) { k -= cg; ++pix; }
    }
}

// ------------------------------------------------------------------------------------------
// DenseNet transitions: AvgPool2d(2, 2) on split planes [B][hin][hin][c] -> [B][hin/2][hin/2][c].  One thread = 8 channels of an
// output pixel: the four taps are merged (hi + lo, exact in fp32), summed in row-major order in fp32, multiplied by 0.25 (exact)
// and re-split.  16-byte loads and stores, 64-bit offsets, grid-stride.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void avgpool2x2s2_kernel(const half_t* __restrict__ in_hi, const half_t* __restrict__ in_lo,
                                                           half_t* __restrict__ out_hi, half_t* __restrict__ out_lo, int B,
                                                           int hin, int c) {
    const int ho = hin / 2;
    const int cg = c / 8;
    const size_t total = (size_t)B * ho * ho * cg;
    const size_t row = (size_t)hin * c;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t g = t % cg;
        const size_t pix = t / cg;                      // output pixel: (n * ho + oy) * ho + ox
        const size_t ox = pix % ho;
        const size_t ny = pix / ho;                     // n * ho + oy: input row 2 * ny of the image-stacked map
        const size_t i00 = ((2 * ny) * hin + 2 * ox) * c + g * 8;
        const size_t at[4] = {i00, i00 + c, i00 + row, i00 + row + c};
        float acc[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const h8 vh = *(const h8*)(in_hi + at[q]);
            const h8 vl = *(const h8*)(in_lo + at[q]);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = (float)vh[j] + (float)vl[j];
                acc[j] = q == 0 ? v : __fadd_rn(acc[j], v);
            }
        }
        h8 oh, ol;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            half_t hi, lo;
            split_f32(acc[j] * 0.25f, hi, lo);
            oh[j] = hi;
            ol[j] = lo;
        }
        const size_t o = pix * c + g * 8;
        *(h8*)(out_hi + o) = oh;
        *(h8*)(out_lo + o) = ol;
    }
}

}  // namespace mpx
