// mpx_pool3c.h -- GoogLeNet's 3x3 max pools on split-fp16 NHWC planes, gfx950: one kernel for the windows that are clipped at the map's edge.
//
// torchvision's googlenet.py has twelve of them per forward: maxpool1 / 2 / 3 = MaxPool2d(3, stride 2, ceil_mode=True) on 112 -> 56 -> 28 -> 14
// (hin - 3 is odd, so the ceil-mode map has one more row and column than the floor-mode one and its last window hangs over the edge), and
// branch4.0 = MaxPool2d(3, stride 1, padding 1, ceil_mode=True) of every Inception module, whose border windows are clipped on every side.
// maxpool3x3s2_kernel / maxpool_s2p0_kernel<3> (mpx_kernels.h) assume windows that start at -1 with the floor-mode size, or that lie inside
// the map; they stay as they are.
#pragma once
#include "mpx_conv.h"

namespace mpx {

// ------------------------------------------------------------------------------------------
// 3x3 max pool, stride 1 or 2, pad 0 or 1, planes [B][hin][hin][pitch] -> [B][ho][ho][pitch] with PyTorch's ceil-mode size (host:
// pool3c_out_side).  Taps outside the map are LEFT OUT, never read as zero: an all-negative map stays negative.
// How: a window's row and column indices are clamped into [0, hin - 1].  Every window of the ceil rule holds at least one row and one
// column of the map (it starts at s <= hin - 1 and ends at s + 2 >= 0), so a clamped index is the map's first or last row / column, which
// that window holds anyway: a clipped tap becomes a second read of a tap inside the window and the max does not move.  No bounds
// branch, every load unconditional and inside the planes.
// One thread = 8 channels of a run of W output pixels along x (W = 4 at stride 1, 2 at stride 2).  It walks the run's STRIDE * (W - 1) + 3
// input columns once, keeps the maximum of each column's three rows, and an output is the maximum of its three column maxima: 18 loads per
// plane for four stride-1 outputs where one thread per output pixel issues 36 (the depthwise kernel of that shape is bound by its load
// instructions).  Max is exact, so the order changes no bit.
// As maxpool_s2p0_kernel<2> / <3> the output is the (hi, lo) PAIR of the winning input element (hi + lo is exact in fp32; a
// later element wins only when strictly larger: rows top to bottom inside a column, then columns left to right), so the merged output equals
// F.max_pool2d(merged, 3, stride, pad, 1, ceil_mode=True) bit for bit, for any sign.
// Units (n, oy, run, 8-channel group) are 64-bit, consecutive lanes take consecutive 16-byte groups of a pixel; the grid is capped by the
// host and strides over the rest.  Offsets are 64-bit.  No LDS, no atomics, no scratch (every array below is indexed by unrolled constants).
// ------------------------------------------------------------------------------------------
struct Pool3cParams {
    const half_t* x_hi;
    const half_t* x_lo;
    half_t* y_hi;
    half_t* y_lo;
    long long units;         // B * ho * runs * (pitch / 8)
    int hin, ho, pitch, pad;
    int runs;                // ceil(ho / W)
};

template <int STRIDE>
struct Pool3c {
    static constexpr int W = STRIDE == 1 ? 4 : 2;       // output pixels per thread
    static constexpr int NC = STRIDE * (W - 1) + 3;     // input columns under them
};

template <int STRIDE>
__global__ __launch_bounds__(256) void maxpool3x3_clip_kernel(const Pool3cParams p) {
    constexpr int W = Pool3c<STRIDE>::W, NC = Pool3c<STRIDE>::NC;
    const long long cg = p.pitch >> 3;
    const int last = p.hin - 1;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < p.units; t += (long long)gridDim.x * 256) {
        const long long g = t % cg;
        long long r = t / cg;
        const int run = (int)(r % p.runs);
        r /= p.runs;
        const int oy = (int)(r % p.ho);
        const long long n = r / p.ho;
        const int ox0 = run * W;
        const int iy0 = oy * STRIDE - p.pad, ix0 = ox0 * STRIDE - p.pad;
        size_t row[3];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int iy = min(max(iy0 + dy, 0), last);
            row[dy] = ((size_t)n * p.hin + iy) * p.hin * p.pitch + (size_t)g * 8;
        }
        // column maxima: value, and the pair it came from
        float cv[NC][8];
        h8 ch[NC], cl[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const size_t col = (size_t)min(max(ix0 + c, 0), last) * p.pitch;
            ch[c] = *(const h8*)(p.x_hi + row[0] + col);
            cl[c] = *(const h8*)(p.x_lo + row[0] + col);
#pragma unroll
            for (int j = 0; j < 8; ++j) cv[c][j] = (float)ch[c][j] + (float)cl[c][j];
#pragma unroll
            for (int dy = 1; dy < 3; ++dy) {
                const h8 vh = *(const h8*)(p.x_hi + row[dy] + col);
                const h8 vl = *(const h8*)(p.x_lo + row[dy] + col);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float v = (float)vh[j] + (float)vl[j];
                    const bool take = v > cv[c][j];
                    cv[c][j] = take ? v : cv[c][j];
                    ch[c][j] = take ? vh[j] : ch[c][j];
                    cl[c][j] = take ? vl[j] : cl[c][j];
                }
            }
        }
        const size_t out0 = (((size_t)n * p.ho + oy) * p.ho + ox0) * p.pitch + (size_t)g * 8;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            if (ox0 + k >= p.ho) break;         // the last run of a row may be short
            float bv[8];
            h8 bh = ch[STRIDE * k], bl = cl[STRIDE * k];
#pragma unroll
            for (int j = 0; j < 8; ++j) bv[j] = cv[STRIDE * k][j];
#pragma unroll
            for (int d = 1; d < 3; ++d) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const bool take = cv[STRIDE * k + d][j] > bv[j];
                    bv[j] = take ? cv[STRIDE * k + d][j] : bv[j];
                    bh[j] = take ? ch[STRIDE * k + d][j] : bh[j];
                    bl[j] = take ? cl[STRIDE * k + d][j] : bl[j];
                }
            }
            *(h8*)(p.y_hi + out0 + (size_t)k * p.pitch) = bh;
            *(h8*)(p.y_lo + out0 + (size_t)k * p.pitch) = bl;
        }
    }
}

// Output side of MaxPool2d(3, stride, pad, ceil_mode=True) on a hin x hin map (PyTorch's pooling_output_shape): ceil((hin + 2 pad - 3) /
// stride) + 1, minus one if the last window would start beyond the map and its left / top padding.  0: no such pool (hin + 2 pad < 3).
inline int pool3c_out_side(int hin, int stride, int pad) {
    const int span = hin + 2 * pad - 3;
    if (span < 0) return 0;
    int ho = (span + stride - 1) / stride + 1;
    if ((ho - 1) * stride >= hin + pad) --ho;
    return ho;
}

}  // namespace mpx
