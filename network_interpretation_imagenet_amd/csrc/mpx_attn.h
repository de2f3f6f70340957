// mpx_attn.h -- the kernels a Vision Transformer (torchvision's vit_b_16 / vit_b_32) adds to the conv list, gfx950: scaled-dot-product
// attention over a token sequence on split-fp16 planes and the token assembly (class token + position embedding).  (Its LayerNorms,
// encoder.ln on the class-token row of each image included, are mpx_cnext.h's layernorm_c_kernel.)
//
// 1. ATTENTION.  Input: the planes [B][T][3 D] self_attention.in_proj wrote, Q at channel 0, K at D, V at 2 D, head h owning channels
// 64 h .. 64 h + 63 of each (D = heads * 64); output: planes [B][T][D], what out_proj reads.  Q, K and V are split-fp16 as they come, i.e.
// MFMA operands; both products run on v_mfma_f32_16x16x32_f16 as the project's three products into ONE fp32 accumulator, small terms first:
// A_hi * B_lo, A_lo * B_hi, A_hi * B_hi (mpx_conv.h's order).
//
// THE CONTRACT, per query row i of one (image, head), in fp32 with one rounding per operator (contract(off)):
//     s_ij = 0.125f * (q_i . k_j)          the dot product over the 64 channels is two 32-wide MFMA steps (channels 0..31, then 32..63) of three
//                                          products each, K as the A operand (rows = keys), Q as the B operand (columns = queries); 0.125 is exact
//     m_i  = max_j s_ij                    over the keys j < T only; a maximum has no order
//     e_ij = expf(s_ij - m_i)              the s_ij of the second pass are recomputed by the same instructions: the same bits
//     l_i  = ((part_0 + part_1) + part_2) + part_3,   part_g = the sum of e_ij over the keys j with (j >> 2) & 3 == g, j ascending, from 0.f
//     P_ij = split_f32(1024.f * e_ij)      the weights as an MFMA operand; the factor (exact) keeps the lo half of a small weight out of fp16's
//                                          subnormals: without it a weight under 6e-5 would carry an absolute error of 2^-25
//     a_id = sum_j P_ij * v_jd             32 keys per MFMA step, steps ascending, V^T as the A operand (rows = channels), P as the B operand
//     o_id = a_id / (1024.f * l_i)         ONE IEEE division per output element, after the whole sum; then split_f32 and the store
// KEYS j >= T of the last step CONTRIBUTE EXACTLY NOTHING: their K rows are operands of exact zeros (clamped address, bits ANDed with 0, as
// mpx_gconv.h masks a tap outside the map), they take no part in the maximum, their e is the constant 0.f (not expf of a large negative
// number) and their V^T columns in the LDS are exact zeros: every term they add is 0 * 0.  QUERY ROWS >= T of the last block are computed
// from zero operands and never written.
//
// Operands.  K and Q come 16 bytes per lane straight from global memory (mpx_gconv.h's way): a lane's 8 elements are 8 consecutive channels
// of one token, which is how both planes store them.  V is the A operand of the second product and needs 8 consecutive KEYS of one channel
// per lane, the transpose of how the planes store it: one head's V^T (both planes, T padded to a multiple of 32, 59 KB for T = 197) is staged
// in the LDS once per (image, head) by the whole workgroup.  K resident in the LDS as well (106 KB, one workgroup per CU) was not chosen: K is
// read in its storage order, a head's K is 50 KB that stay in L2 while the workgroup's 13 query blocks walk it, and at 59 KB two workgroups
// share a CU so one's staging overlaps the other's MFMAs.
// The accumulators of Q K^T become the B operand of P V without leaving their lane (mpx_btail.h's precedent): an accumulator quad of tile t
// is keys 16 t + 4 g .. + 3 of query (lane & 15) in lane group g = lane >> 4, and an MFMA sums over its 32 K slots in an order of its own, so
// slot 8 g + e of a 32-key step is DEFINED as key 4 g + e (e < 4) or 16 + 4 g + e - 4 (e >= 4) of the step -- the V^T image in the LDS is
// stored in that slot order, one ds_read_b128 per fragment.
//
// Work.  A unit is one (image, head); the host caps the grid and a workgroup strides over the units, its 4 waves over the unit's query blocks
// of 16 rows (no barrier inside that walk).  Two barriers per unit, in front of and behind the staging, with a trip count that is the same
// for every thread of the workgroup.  An output row's bits depend on its (image, head)'s data alone: not on B, not on the image's position
// in the batch, not on the grid.  T, heads and B are run-time values (1 <= T <= AT_MAX_T); head_dim is 64.  Offsets are 64-bit, global
// accesses 16 bytes (8-byte stores of accumulator quads, as mpx_gconv.h's epilogue), no atomics, no scratch.
//
// 2. TOKEN ASSEMBLY: tok[b][0] = class_token + pos[0], tok[b][1 + i] = patch[b][i] + pos[1 + i]: one fp32 add of the exact hi + lo (or the
// fp32 class token) and the fp32 position embedding, re-split.  Planes [B][T - 1][D] -> [B][T][D].
#pragma once
#include <cmath>

#include "mpx_gconv.h"

namespace mpx {

constexpr int AT_NT = 256;          // threads of a workgroup
constexpr int AT_WAVES = 4;
constexpr int AT_HD = 64;           // head_dim
constexpr int AT_MAX_T = 512;       // the V^T image of one head must fit the LDS: 2 * 64 * (512 + 8) * 2 = 130 KB
constexpr float AT_PSCALE = 1024.f; // the weights' operand scale (exact)

__host__ __device__ inline int at_tpad(int T) { return (T + 31) / 32 * 32; }
__host__ __device__ inline int at_pitch(int T) { return at_tpad(T) + 8; }           // halfs per V^T row (16-byte aligned rows off the bank period)
__host__ __device__ inline size_t at_lds_bytes(int T) { return (size_t)2 * AT_HD * at_pitch(T) * sizeof(half_t); }

struct AttnParams {
    const half_t* qkv_hi;    // [B][T][3 D]
    const half_t* qkv_lo;
    half_t* o_hi;            // [B][T][D]
    half_t* o_lo;
    long long units;         // B * heads
    int T, heads, D;
};

__global__ __launch_bounds__(AT_NT) void attention_f16x3_kernel(const AttnParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char at_smem[];
    const int T = p.T, D = p.D;
    const size_t D3 = (size_t)3 * D;
    const int tpad = at_tpad(T), pitch = at_pitch(T);
    half_t* vt_hi = (half_t*)at_smem;
    half_t* vt_lo = vt_hi + AT_HD * pitch;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, col = lane & 15;
    const int nqb = (T + 15) >> 4, nkt = (T + 15) >> 4, nk32 = tpad >> 5;
    for (long long u = blockIdx.x; u < p.units; u += gridDim.x) {
        const long long b = u / p.heads;
        const int hd = (int)(u - b * p.heads);
        const size_t img = (size_t)b * T * D3;          // the image's first QKV element
        const size_t ch = (size_t)hd * AT_HD;           // the head's first channel within Q, K, V and the output row
        __syncthreads();                                // every wave is done with the previous unit's V^T
        for (int idx = threadIdx.x; idx < tpad * 8; idx += AT_NT) {
            const int key = idx >> 3, c8 = (idx & 7) << 3;
            const bool ok = key < T;
            const size_t off = img + (size_t)(ok ? key : 0) * D3 + 2 * (size_t)D + ch + c8;
            const unsigned keep = ok ? 0xffffffffu : 0u;
            const u4 wh = *(const u4*)(p.qkv_hi + off) & keep;
            const u4 wl = *(const u4*)(p.qkv_lo + off) & keep;
            const h8 vh = __builtin_bit_cast(h8, wh), vl = __builtin_bit_cast(h8, wl);
            // slot of the key within its 32-key step: key = 16 * half + 4 * grp + e  ->  8 * grp + 4 * half + e
            const int k32 = key & 31;
            const int pos = (key & ~31) | ((k32 & 12) << 1) | ((k32 & 16) >> 2) | (k32 & 3);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                vt_hi[(c8 + j) * pitch + pos] = vh[j];
                vt_lo[(c8 + j) * pitch + pos] = vl[j];
            }
        }
        __syncthreads();
        for (int qb = wave; qb < nqb; qb += AT_WAVES) {
            const int qi = qb * 16 + col;
            const bool q_ok = qi < T;
            h8 qh[2], ql[2];
            {
                const size_t off = img + (size_t)(q_ok ? qi : 0) * D3 + ch + g * 8;
                const unsigned keep = q_ok ? 0xffffffffu : 0u;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const u4 wh = *(const u4*)(p.qkv_hi + off + ks * 32) & keep;
                    const u4 wl = *(const u4*)(p.qkv_lo + off + ks * 32) & keep;
                    qh[ks] = __builtin_bit_cast(h8, wh);
                    ql[ks] = __builtin_bit_cast(h8, wl);
                }
            }
            // q . k of the 16 keys of tile kt for the 16 queries of the block: lane (g, col), register r = key 16 kt + 4 g + r, query col
            auto s_tile = [&](int kt) -> f4 {
                const int kj = kt * 16 + col;
                const bool ok = kj < T;
                const size_t off = img + (size_t)(ok ? kj : 0) * D3 + (size_t)D + ch + g * 8;
                const unsigned keep = ok ? 0xffffffffu : 0u;
                f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const u4 wh = *(const u4*)(p.qkv_hi + off + ks * 32) & keep;
                    const u4 wl = *(const u4*)(p.qkv_lo + off + ks * 32) & keep;
                    const h8 kh = __builtin_bit_cast(h8, wh), kl = __builtin_bit_cast(h8, wl);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, ql[ks], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl, qh[ks], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, qh[ks], acc, 0, 0, 0);
                }
                return acc;
            };
            // pass 1: the row maximum
            float m = -INFINITY;
            for (int kt = 0; kt < nkt; ++kt) {
                const f4 s = s_tile(kt);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = 0.125f * s[r];
                    m = (kt * 16 + g * 4 + r < T) ? fmaxf(m, v) : m;
                }
            }
            m = fmaxf(m, __shfl_xor(m, 16));
            m = fmaxf(m, __shfl_xor(m, 32));
            // pass 2: the weights, their sum and P V
            float part = 0.f;
            f4 o[4];
#pragma unroll
            for (int f = 0; f < 4; ++f) o[f] = (f4){0.f, 0.f, 0.f, 0.f};
            for (int k2 = 0; k2 < nk32; ++k2) {
                const f4 s0 = s_tile(2 * k2), s1 = s_tile(2 * k2 + 1);
                h8 ph, pl;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int key = k2 * 32 + (e < 4 ? 0 : 16) + g * 4 + (e & 3);
                    const float sv = 0.125f * (e < 4 ? s0[e & 3] : s1[e & 3]);
                    const float ev = key < T ? expf(sv - m) : 0.f;
                    part = part + ev;
                    half_t hi, lo;
                    split_f32(AT_PSCALE * ev, hi, lo);
                    ph[e] = hi;
                    pl[e] = lo;
                }
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    const int at = (f * 16 + col) * pitch + k2 * 32 + g * 8;
                    const h8 vh = *(const h8*)(vt_hi + at);
                    const h8 vl = *(const h8*)(vt_lo + at);
                    o[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pl, o[f], 0, 0, 0);
                    o[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, ph, o[f], 0, 0, 0);
                    o[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph, o[f], 0, 0, 0);
                }
            }
            const float l0 = __shfl(part, col), l1 = __shfl(part, 16 + col), l2 = __shfl(part, 32 + col), l3 = __shfl(part, 48 + col);
            const float den = AT_PSCALE * (((l0 + l1) + l2) + l3);
            // o[f] register r: channel 16 f + 4 g + r of query col
            if (q_ok) {
                const size_t out = ((size_t)b * T + qi) * D + ch + g * 4;
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    h4 oh, ol;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        half_t hi, lo;
                        split_f32(o[f][r] / den, hi, lo);
                        oh[r] = hi;
                        ol[r] = lo;
                    }
                    *(h4*)(p.o_hi + out + f * 16) = oh;
                    *(h4*)(p.o_lo + out + f * 16) = ol;
                }
            }
        }
    }
#endif
}

// ------------------------------------------------------------------------------------------
// 2. Token assembly: planes [B][T - 1][D] (conv_proj's output), fp32 class_token [D] and pos [T][D] -> planes [B][T][D].
//     tok[b][0][c] = class_token[c] + pos[0][c];   tok[b][1 + i][c] = (hi + lo of patch[b][i][c], exact) + pos[1 + i][c]
// one fp32 add each, then the split.  One thread = 8 channels of one token, grid-stride over B * T * D / 8 of them.  No LDS, no barrier.
// ------------------------------------------------------------------------------------------
struct TokParams {
    const half_t* x_hi;      // [B][T - 1][D]
    const half_t* x_lo;
    half_t* y_hi;            // [B][T][D]
    half_t* y_lo;
    const float* cls;        // [D]
    const float* pos;        // [T][D]
    long long chunks;        // B * T * D / 8
    int T, D;
};

__global__ __launch_bounds__(AT_NT) void tokens_assemble_kernel(const TokParams p) {
#pragma clang fp contract(off)
    const int G = p.D >> 3;
    for (long long i = (long long)blockIdx.x * AT_NT + threadIdx.x; i < p.chunks; i += (long long)gridDim.x * AT_NT) {
        const long long row = i / G;
        const int c = (int)(i - row * G) << 3;
        const long long b = row / p.T;
        const int t = (int)(row - b * p.T);
        const float* pe = p.pos + (size_t)t * p.D + c;
        const f4 p0 = *(const f4*)pe, p1 = *(const f4*)(pe + 4);
        float v[8];
        if (t == 0) {
            const f4 c0 = *(const f4*)(p.cls + c), c1 = *(const f4*)(p.cls + c + 4);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = j < 4 ? c0[j & 3] : c1[j & 3];
        } else {
            const size_t at = ((size_t)b * (p.T - 1) + (t - 1)) * p.D + c;
            const h8 vh = *(const h8*)(p.x_hi + at);
            const h8 vl = *(const h8*)(p.x_lo + at);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (float)vh[j] + (float)vl[j];
        }
        h8 oh, ol;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float y = v[j] + (j < 4 ? p0[j & 3] : p1[j & 3]);
            half_t hi, lo;
            split_f32(y, hi, lo);
            oh[j] = hi;
            ol[j] = lo;
        }
        const size_t o = (size_t)row * p.D + c;
        *(h8*)(p.y_hi + o) = oh;
        *(h8*)(p.y_lo + o) = ol;
    }
}

}  // namespace mpx
