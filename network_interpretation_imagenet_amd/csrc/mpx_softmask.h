// mpx_softmask.h -- the staging kernel of every mask that is a weight per pixel (K0 among them), and the score-weighted sum of the masks.
//
// softmask_apply_kernel<WS> and softmask_saliency_kernel<WS> take a weight w_m(p) per mask m and pixel p from a weight source WS:
//   OnoffWeights     w_m(p) = onoff[m][seg[p]] ? 1 : 0: K0, the binary union of the superpixels of a label map (mpx_mask_apply_normalize).
//                    The tile's STAGE_MT x S on/off bytes are staged in LDS; seg[p] is read once per pixel; a label outside [0, S) weighs 0;
//   ExplicitWeights  w_m(p) = weights[m][p], DEV f32[M][224][224], read coalesced;
//   RiseWeights      w_m(p) synthesised from the s x s bits and the shift of mask m: the masks of RISE (Petsiuk, Das, Saenko, "RISE:
//                    Randomized Input Sampling for Explanation of Black-box Models", BMVC 2018) -- a random s x s grid, upsampled
//                    bilinearly to U x U with half-pixel centres, cropped to 224 x 224 at a random shift (dy, dx).
//   DesignWeights    w_r(p) gathered from the two design matrices A, B (DEV f32[N][D], D = d * d) of a Sobol total-order design over a d x d
//                    grid of piecewise constant cells (Fel, Cadene, Chalvidal, Cord, Vigouroux, Serre, "Look at the Variance! Efficient
//                    Black-box Explanations with Sobol-based Sensitivity Analysis", NeurIPS 2021), at the global row r = row0 + m:
//                      c(p) = ((y * d) / 224) * d + (x * d) / 224                      integer divisions; once per pixel (Pixel)
//                      r <  N:  w = A[r][c]
//                      r >= N:  q = r - N, j = q / D, i = q - j * D;  w = (i == c) ? B[j][c] : A[j][c]
//                    a pure gather, no arithmetic on w.  The tile's 32 (row base, i) pairs are worked out once per block in stage() -- one
//                    integer division per tile row, none per (pixel, row) -- and kept in 256 B of LDS; A and B are read from global memory
//                    (2 N D floats: the L1 / L2 hold them) when the row base changes and kept in the pixel's state: the D consecutive rows
//                    of one j differ in the one replaced cell only, so a row is an LDS read and a select.
//   BoxWeights       w_m(p) = 0 inside the box of row m, 1 outside: the sliding window of occlusion sensitivity (Zeiler, Fergus, "Visualizing
//                    and Understanding Convolutional Networks", ECCV 2014).  boxes[m] = (y0, x0, y1, x1), DEV i32[M][4], half-open: pixel
//                    (y, x) is covered iff y0 <= y < y1 && x0 <= x < x1; an empty box (y0 == y1 or x0 == x1) covers nothing.  The tile's
//                    boxes are 512 B of LDS (every lane reads the same 16 bytes: a broadcast); the kernel COMPARES against the four values
//                    and never indexes by them, so a box outside [0, 224] is memory-safe whatever the caller passes.  With a fill image
//                    (kFill) the blend below is, as values, a select between the pixel and the fill pixel.
//   MapWeights       w_m(p) = min(max(up(maps[m])(p), 0), 1): the activation maps of Score-CAM (Wang et al., CVPR-W 2020; mpx_cam.h) as
//                    masks.  maps DEV f32[M][g][g], 2 <= g <= 16 (the normalised cells mpx_cam_cells writes); up() is the RISE upsampling
//                    below with no shift and U = 224 (cam_axis, cam_up; mpx_cam.h states it).  There is no shift, so the geometry -- i0 * g,
//                    i1 * g, j0, j1, fy, fx -- is the same for every row and is worked out ONCE per pixel and tile (Pixel), which RISE's
//                    source cannot do; a row is four LDS reads, nine rounded operations and the clamp.  The tile's 32 x g * g floats
//                    are staged in LDS (32 KB at g = 16).  The unclamped value leaves [0, 1] by rounding only; the clamp is two selects
//                    (v > 0 ? v : +0.0, then w < 1 ? w : 1), so that a zero weight is +0.0.
// A source is: kLds, kPinPixel (the apply kernel pins the loaded pixel in registers in front of its row loop), lds_bytes(n), stage() (the
// tile's rows into LDS), Pixel + pixel() (what it keeps per pixel across the rows of a tile;
// empty for the explicit and the RISE source) and weight().
//
// The RISE weight, stated exactly (cell = ceil(224 / s), U = (s + 1) * cell, 2 <= s <= 32, 0 <= dy, dx < cell; g = the grid as 0.0f / 1.0f):
//   Y  = y + dy
//   t  = max((2Y + 1) * s - U, 0)                 integers
//   i0 = t / (2U)                                 integer division
//   r  = t - i0 * 2U
//   fy = float(r) / float(2U)                     ONE correctly rounded fp32 division of two exactly represented integers
//   i1 = min(i0 + 1, s - 1)                       the same along x: j0, j1, fx
//   top = fl(fl(fl(1 - fx) * g[i0][j0]) + fl(fx * g[i0][j1]))
//   bot = fl(fl(fl(1 - fx) * g[i1][j0]) + fl(fx * g[i1][j1]))
//   w   = fl(fl(fl(1 - fy) * top) + fl(fy * bot))
// fl() = one fp32 rounding to nearest even.  Every product and every sum is rounded on its own: NO FMA anywhere in w (the functions below
// switch contraction off, which hipcc otherwise applies to a * b + c).  This is torch.nn.functional.interpolate(grid, size=(U, U),
// mode="bilinear", align_corners=False)[dy:dy+224, dx:dx+224] up to rounding; masks.rise_weights is its numpy fp32 restatement, bit for bit.
// An all-ones grid gives exactly 1.0 (fl(fl(1 - f) + f) = 1 for every fp32 f in [0, 1)), an all-zeros grid exactly 0.0, everything else
// lies in [0, 1].
//
// Apply:    o = fl(v * w) per channel (ONE fp32 multiply, no FMA with the split behind it), then split_f32: hi = f16(o), lo = f16(fl(o -
//           f32(hi))).  With a fill image F (kFill, the design and the box source): o = fl(fl(v * w) + fl(F * fl(1 - w))), four fp32 operations each
//           rounded on its own, so that a cell is pulled towards F and not towards zero; w = 1 gives v + F * 0, w = 0 gives v * 0 + F.  For w in {0, 1} that is `x * mask` as numpy does it, the -0.0 of a removed negative pixel included (hi -0.0, lo
//           +0.0), whichever source the weight comes from.  The product is pinned in an fp32 register (fp32_value, mpx_conv.h) before the
//           split: hipcc otherwise folds f16(a * b) into v_fma_mixlo_f16, which rounds the exact product to fp16 once and turns a -0.0
//           product into +0.0.
// Saliency: sal[p] <- fl(sal[p] + fl(weight[m] * w_m(p))) for m = 0, 1, .., M - 1 in this order: a multiply and an add, each rounded, NOT an
//           FMA.  One thread owns a pixel and walks the masks in order -- no atomics, no reduction tree --, so a pixel's bits depend neither on
//           the grid nor on how the rows are cut into consecutive calls.
#pragma once
#include "mpx_stage.h"

namespace mpx {

constexpr int SM_S_MIN = 2;
constexpr int SM_S_MAX = 32;
constexpr int SM_SAL_THREADS = 64;  // saliency: one wave per block, 784 blocks over the 256 CUs
constexpr int SOBOL_GRID_MIN = 2;
constexpr int SOBOL_GRID_MAX = 32;  // D = 1024 cells: mpx_segment_paint's limit (SUR_S_MAX), which paints the indices
constexpr int CAM_G_MIN = 2;
constexpr int CAM_G_MAX = 16;       // include/mpx.h MPX_CAM_GRID_MAX: 32 rows x 16 x 16 floats = 32 KB of LDS per apply tile
constexpr int CAM_IMG = 224;        // the side an activation map is upsampled to

// A launch has ONE weight source, so the design source's fields lie over the other sources' five pointers: the struct keeps its 168 bytes
// and every field its offset, and with them every kernel that takes (SoftParams, ...) its kernel-argument loads.
struct SoftParams {
    const uint8_t* img_u8;   // [H][W][3] or null                          (apply)
    const float* img_f32;    // [3][H][W] or null                          (apply)
    union {
        struct {
            const int32_t* seg;      // [H][W]                             (on/off source)
            const uint8_t* onoff;    // [M][S], non-zero = keep            (on/off source)
            const float* weights;    // [M][H][W]                          (explicit source)
            const uint8_t* cells;    // [M][s][s], non-zero = keep         (RISE source)
            const int32_t* shift;    // [M][2] = (dy, dx)                  (RISE source)
        };
        struct {
            const float* A;          // [N][d * d]                         (design source)
            const float* B;          // [N][d * d]
            const float* fill;       // [3][H][W] or null                  (design source, kFill)
            int N, d, row0;          // designs, grid size, the design row of mask 0
        };
        struct {
            const int32_t* boxes;    // [M][4] = (y0, x0, y1, x1), half-open   (box source; its fill image is the design source's slot)
        };
        struct {
            const float* maps;       // [M][g][g]                          (map source)
            int g;                   // the maps' side
        };
    };
    const float* score;      // [M]: the weight of mask m in the sum       (saliency)
    float* sal;              // [H][W], accumulated in place               (saliency)
    half_t* out_hi;          // engine staging, slot 0 (padded NHWC4)      (apply)
    half_t* out_lo;
    float* out_f32;          // [M][3][H][W] or null                       (apply)
    float mean[3], std[3];
    int M, S, slot0;
    int s, cell, U2;         // RISE: grid size, ceil(224 / s), 2U = 2 * (s + 1) * cell
    float f_U2, inv_U2;      // float(2U) (exact) and 1 / float(2U) (a first guess of the quotient only)
    int size, pad_size, border;   // 224, 230, 3
};

static_assert(sizeof(SoftParams) == 168, "the design source's fields fit over the other sources' pointers");

// One axis of the RISE upsampling at the shifted coordinate Y: i0, i1 and the fraction, from integers.  The quotient t / 2U is guessed in
// fp32 (t < 2U * s < 2^24 is exact as a float, the guess is off by at most one) and fixed up against the integer remainder, so i0 and r ARE
// the integer quotient and remainder; the one rounding of the axis is the division r / 2U.
__device__ __forceinline__ void rise_axis(int Y, const SoftParams& p, int& i0, int& i1, float& f) {
#pragma clang fp contract(off)
    const int t = max((2 * Y + 1) * p.s - (p.U2 >> 1), 0);
    int q = (int)((float)t * p.inv_U2);
    int r = t - q * p.U2;
    if (r < 0) { q -= 1; r += p.U2; }
    if (r >= p.U2) { q += 1; r -= p.U2; }
    i0 = min(q, p.s - 1);           // q <= s - 1 for every shift inside the contract; the clamp keeps a shift outside it inside the grid
    i1 = min(i0 + 1, p.s - 1);
    f = __fdiv_rn((float)r, p.f_U2);
}

// One axis of the map upsampling g -> 224 at pixel coordinate y (no shift, U = 224): i0, i1 and the fraction, from integers; the one
// rounding is the division r / 448.
__device__ __forceinline__ void cam_axis(int y, int g, int& i0, int& i1, float& f) {
    const int t = max((2 * y + 1) * g - CAM_IMG, 0);
    i0 = min(t / (2 * CAM_IMG), g - 1);     // t / 448 <= g - 1 inside [0, 224); the clamp keeps a coordinate outside it inside the grid
    const int r = t - i0 * (2 * CAM_IMG);
    i1 = min(i0 + 1, g - 1);
    f = __fdiv_rn((float)r, (float)(2 * CAM_IMG));
}

// up(G) at one pixel, a0 = i0 * g, a1 = i1 * g: nine operations, each rounded on its own.
__device__ __forceinline__ float cam_up(const float* G, int a0, int a1, int j0, int j1, float fy, float fx) {
#pragma clang fp contract(off)
    const float g00 = G[a0 + j0], g01 = G[a0 + j1], g10 = G[a1 + j0], g11 = G[a1 + j1];
    const float omx = 1.0f - fx, omy = 1.0f - fy;
    const float top = omx * g00 + fx * g01;     // contraction is off: two rounded products, one rounded sum
    const float bot = omx * g10 + fx * g11;
    return omy * top + fy * bot;
}

struct NoPixelState {};

struct OnoffWeights {
    static constexpr bool kLds = true;
    static constexpr bool kPinPixel = false;
    struct Pixel { int s; bool ok; };
    static size_t lds_bytes(int S) { return ((size_t)STAGE_MT * S + 15) & ~(size_t)15; }      // u8[STAGE_MT][S]
    __device__ static __forceinline__ void stage(const SoftParams& p, char* smem, int m_base, int mt, int tid, int nthreads) {
        const uint8_t* src = p.onoff + (size_t)m_base * p.S;
        for (int i = tid; i < mt * p.S; i += nthreads) smem[i] = src[i];
    }
    __device__ static __forceinline__ Pixel pixel(const SoftParams& p, int pix) {
        const int s = p.seg[pix];
        const bool ok = (unsigned)s < (unsigned)p.S;
        return {ok ? s : 0, ok};
    }
    __device__ static __forceinline__ float weight(const SoftParams& p, const char* smem, Pixel px, int, int mi, int, int, int, int) {
        return (px.ok && smem[mi * p.S + px.s]) ? 1.0f : 0.0f;
    }
};

struct ExplicitWeights {
    static constexpr bool kLds = false;
    static constexpr bool kPinPixel = false;
    typedef NoPixelState Pixel;
    static size_t lds_bytes(int) { return 0; }
    __device__ static __forceinline__ void stage(const SoftParams&, char*, int, int, int, int) {}
    __device__ static __forceinline__ Pixel pixel(const SoftParams&, int) { return {}; }
    __device__ static __forceinline__ float weight(const SoftParams& p, const char*, Pixel, int m, int, int pix, int, int, int hw) {
        return p.weights[(size_t)m * hw + pix];
    }
};

struct RiseWeights {
    static constexpr bool kLds = true;
    static constexpr bool kPinPixel = false;
    typedef NoPixelState Pixel;
    // LDS: i32[STAGE_MT][2] shifts, then u8[STAGE_MT][s * s] cells
    static size_t lds_bytes(int s) { return (size_t)STAGE_MT * 8 + (((size_t)STAGE_MT * s * s + 15) & ~(size_t)15); }
    __device__ static __forceinline__ void stage(const SoftParams& p, char* smem, int m_base, int mt, int tid, int nthreads) {
        int* s_shift = (int*)smem;
        uint8_t* s_cells = (uint8_t*)smem + STAGE_MT * 8;
        const int ss = p.s * p.s;
        const uint8_t* src = p.cells + (size_t)m_base * ss;
        for (int i = tid; i < mt * ss; i += nthreads) s_cells[i] = src[i];
        // a shift outside [0, cell) is outside the contract; clamped here so that no coordinate leaves the grid whatever the caller passes
        for (int i = tid; i < mt * 2; i += nthreads) s_shift[i] = min(max(p.shift[(size_t)m_base * 2 + i], 0), p.cell - 1);
    }
    __device__ static __forceinline__ Pixel pixel(const SoftParams&, int) { return {}; }
    __device__ static __forceinline__ float weight(const SoftParams& p, const char* smem, Pixel, int, int mi, int, int y, int x, int) {
#pragma clang fp contract(off)
        const int* s_shift = (const int*)smem;
        const uint8_t* g = (const uint8_t*)smem + STAGE_MT * 8 + mi * p.s * p.s;
        int i0, i1, j0, j1;
        float fy, fx;
        rise_axis(y + s_shift[mi * 2], p, i0, i1, fy);
        rise_axis(x + s_shift[mi * 2 + 1], p, j0, j1, fx);
        const float g00 = g[i0 * p.s + j0] ? 1.0f : 0.0f, g01 = g[i0 * p.s + j1] ? 1.0f : 0.0f;
        const float g10 = g[i1 * p.s + j0] ? 1.0f : 0.0f, g11 = g[i1 * p.s + j1] ? 1.0f : 0.0f;
        const float omx = 1.0f - fx, omy = 1.0f - fy;
        const float top = omx * g00 + fx * g01;     // contraction is off: two rounded products, one rounded sum
        const float bot = omx * g10 + fx * g11;
        return omy * top + fy * bot;
    }
};

struct DesignWeights {
    static constexpr bool kLds = true;
    // Most rows of a tile take their weight from registers: with the pixel (and the fill) pinned in front of the row loop, such a row waits
    // for no load, and so not for the stores of the rows before it either (one counter covers both).
    static constexpr bool kPinPixel = true;
    struct Pixel { int c, base; float a, b; };      // the pixel's cell, and A[j][c] / B[j][c] of the j (row base) they were last read for
    static size_t lds_bytes(int) { return (size_t)STAGE_MT * 8; }                             // i32[STAGE_MT][2] = (row base, i or -1)
    __device__ static __forceinline__ void stage(const SoftParams& p, char* smem, int m_base, int mt, int tid, int) {
        if (tid < mt) {
            const int D = p.d * p.d;
            const int r = p.row0 + m_base + tid;
            int jr = r, i = -1;                 // r < N: row r of A, no cell replaced
            if (r >= p.N) {
                const int q = r - p.N;
                jr = q / D;
                i = q - jr * D;
            }
            ((int*)smem)[tid * 2] = jr * D;     // < N * D, which the entry holds below 2^31
            ((int*)smem)[tid * 2 + 1] = i;
        }
    }
    __device__ static __forceinline__ Pixel pixel(const SoftParams& p, int pix) {
        const int y = pix / p.size, x = pix - y * p.size;
        return {((y * p.d) / p.size) * p.d + (x * p.d) / p.size, -1, 0.f, 0.f};
    }
    // The D rows of one j read the same two floats: they are loaded when the row base changes (every row below N, every D-th row above)
    // and kept in the pixel's state, so that a row costs one LDS read and a select.
    __device__ static __forceinline__ float weight(const SoftParams& p, const char* smem, Pixel& px, int, int mi, int, int, int, int) {
        const int base = ((const int*)smem)[mi * 2], i = ((const int*)smem)[mi * 2 + 1];
        if (base != px.base) {
            px.base = base;
            const float a = p.A[(size_t)base + px.c], b = p.B[(size_t)base + px.c];
            px.a = fp32_value(a);       // used HERE: the wait for the two loads stays inside this branch, and the rows that take the values
            px.b = fp32_value(b);       // from the registers do not wait for the stores of the row before them
        }
        return i == px.c ? px.b : px.a;
    }
};

struct BoxWeights {
    static constexpr bool kLds = true;
    // The weight is an LDS read and four compares: with the pixel (and the fill) pinned in front of the row loop no row waits for a load,
    // and so not for the stores of the rows before it (DesignWeights says why).
    static constexpr bool kPinPixel = true;
    typedef NoPixelState Pixel;
    static size_t lds_bytes(int) { return (size_t)STAGE_MT * 16; }                            // i32[STAGE_MT][4]
    __device__ static __forceinline__ void stage(const SoftParams& p, char* smem, int m_base, int mt, int tid, int) {
        if (tid < mt * 4) ((int*)smem)[tid] = p.boxes[(size_t)m_base * 4 + tid];
    }
    __device__ static __forceinline__ Pixel pixel(const SoftParams&, int) { return {}; }
    __device__ static __forceinline__ float weight(const SoftParams&, const char* smem, Pixel, int, int mi, int, int y, int x, int) {
        const int4 b = ((const int4*)smem)[mi];     // (y0, x0, y1, x1): compared against, never an index
        const bool covered = (y >= b.x) & (y < b.z) & (x >= b.y) & (x < b.w);       // & not &&: one 16-byte read, four compares, no branch
        return covered ? 0.0f : 1.0f;
    }
};

struct MapWeights {
    static constexpr bool kLds = true;
    // The weight comes from LDS and registers: with the pixel pinned in front of the row loop no row waits for a load, and so not for the
    // stores of the rows before it (DesignWeights says why).
    static constexpr bool kPinPixel = true;
    struct Pixel { int a0, a1, j0, j1; float fy, fx; };      // i0 * g, i1 * g, j0, j1 and the fractions: the same for every row
    static size_t lds_bytes(int g) { return (size_t)STAGE_MT * g * g * 4; }                   // f32[STAGE_MT][g * g]
    __device__ static __forceinline__ void stage(const SoftParams& p, char* smem, int m_base, int mt, int tid, int nthreads) {
        const int gg = p.g * p.g;
        const float* src = p.maps + (size_t)m_base * gg;
        for (int i = tid; i < mt * gg; i += nthreads) ((float*)smem)[i] = src[i];
    }
    __device__ static __forceinline__ Pixel pixel(const SoftParams& p, int pix) {
        const int y = pix / p.size, x = pix - y * p.size;
        Pixel px;
        int i0, i1;
        cam_axis(y, p.g, i0, i1, px.fy);
        cam_axis(x, p.g, px.j0, px.j1, px.fx);
        px.a0 = i0 * p.g; px.a1 = i1 * p.g;
        return px;
    }
    __device__ static __forceinline__ float weight(const SoftParams& p, const char* smem, const Pixel& px, int, int mi, int, int, int, int) {
        const float v = cam_up((const float*)smem + mi * p.g * p.g, px.a0, px.a1, px.j0, px.j1, px.fy, px.fx);
        const float w = v > 0.0f ? v : 0.0f;
        return w < 1.0f ? w : 1.0f;
    }
};

// Apply.  One thread = one pixel; a block loops over a tile of STAGE_MT masks (a source with kLds stages what it needs of them in LDS
// first), so the image -- and the on/off source's label map -- is read once per STAGE_MT masks and every store is a coalesced 512-B
// (planes) / 256-B (f32) wave row.  No atomics, no scratch, 64-bit offsets.
// kFill: the fill blend o = fl(fl(v * w) + fl(F * fl(1 - w))) with F = p.fill, read once per pixel; without it the arithmetic is o = fl(v * w).
template <class WS, bool kFill = false>
__global__ __launch_bounds__(256) void softmask_apply_kernel(const SoftParams p) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int m_base = blockIdx.y * STAGE_MT;
    const int mt = min(STAGE_MT, p.M - m_base);
    if (WS::kLds) {
        WS::stage(p, smem, m_base, mt, tid, 256);
        __syncthreads();
    }
    const int hw = p.size * p.size;
    const int pix = blockIdx.x * 256 + tid;
    if (pix >= hw) return;
    const int y = pix / p.size, x = pix - y * p.size;
    typename WS::Pixel px = WS::pixel(p, pix);      // not const: the design source keeps what it last read in it
    float v[3];
    load_normalized_pixel(p.img_u8, p.img_f32, p.mean, p.std, pix, hw, v);
    float f[3] = {0.f, 0.f, 0.f};
    if (kFill) {
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c] = p.fill[(size_t)c * hw + pix];
    }
    if (WS::kPinPixel) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[c] = fp32_value(v[c]);
            if (kFill) f[c] = fp32_value(f[c]);
        }
    }
    const size_t pad_off = staged_pixel_offset(p, y, x);
    for (int mi = 0; mi < mt; ++mi) {
        const int m = m_base + mi;
        const float w = WS::weight(p, smem, px, m, mi, pix, y, x, hw);
        float o[3];
        half_t hi[3], lo[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (kFill) {
                const float omw = 1.0f - w;
                const float a = v[c] * w, b = f[c] * omw;       // contraction is off: two rounded products ...
                o[c] = fp32_value(a + b);                       // ... and one rounded sum, pinned
            } else {
                o[c] = fp32_value(v[c] * w);        // one rounded multiply, pinned: hi and o - hi are taken from the ROUNDED product
            }
            split_f32(o[c], hi[c], lo[c]);
        }
        store_staged_pixel(p, m, pad_off, pix, hw, staged_h4(hi), staged_h4(lo), o);
    }
}

// Saliency: sal[p] <- fl(sal[p] + fl(score[m] * w_m(p))), m ascending, from the value already in sal.  One thread owns a pixel for the whole
// launch and walks all M masks in order (tile by tile through LDS for the RISE source).
template <class WS>
__global__ __launch_bounds__(SM_SAL_THREADS) void softmask_saliency_kernel(const SoftParams p) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int hw = p.size * p.size;
    const int pix = blockIdx.x * SM_SAL_THREADS + tid;
    const bool active = pix < hw;       // no early return: every thread of the block meets the barriers below
    const int cp = active ? pix : 0;
    const int y = cp / p.size, x = cp - y * p.size;
    const typename WS::Pixel px = WS::pixel(p, cp);
    float acc = active ? p.sal[cp] : 0.0f;
    for (int m_base = 0; m_base < p.M; m_base += STAGE_MT) {
        const int mt = min(STAGE_MT, p.M - m_base);
        if (WS::kLds) {
            WS::stage(p, smem, m_base, mt, tid, SM_SAL_THREADS);
            __syncthreads();
        }
        for (int mi = 0; mi < mt; ++mi) {
            const float w = WS::weight(p, smem, px, m_base + mi, mi, cp, y, x, hw);
            const float t = p.score[m_base + mi] * w;       // rounded product ...
            acc = acc + t;                                  // ... rounded sum: not an FMA
        }
        if (WS::kLds) __syncthreads();  // the tile is read out before the next one lands
    }
    if (active) p.sal[cp] = acc;
}

}  // namespace mpx
