// probe: ShuffleNetV2's linear depthwise kernel -- the one-pixel-per-thread form (kept here only) against the committed run form
// (csrc/mpx_dw.h, dwconv_bn_act_kernel<3, STRIDE, false>) on the same planes in the same process, batch 2340, launches alternating; compares the outputs bit for bit.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/probes/dw_run_probe tools/probes/dw_run_probe.hip   (profiles/shufflenet_dw_run_probe.txt)
#include "../../network_interpretation_imagenet_amd/csrc/mpx_dw.h"
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
using namespace mpx;

// the one-pixel-per-thread form, as first written for ShuffleNetV2
__global__ __launch_bounds__(256) void dwconv3x3_bn_onepixel_kernel(const DwParams p) {
#pragma clang fp contract(off)
    const unsigned cg = (unsigned)p.pitch >> 3;                     // units per pixel
    const unsigned step = gridDim.x * 256u;                         // <= 2^20 units: 32-bit divisions, once
    const unsigned u0 = blockIdx.x * 256u + threadIdx.x;
    const unsigned dpix = step / cg, dk = step % cg;
    long long pix = u0 / cg;
    unsigned k = u0 % cg;
    const long long howo = (long long)p.ho * p.ho;
    while (pix < p.npix) {
        const int c = (int)(k << 3);
        const long long n = pix / howo;
        const int rem = (int)(pix - n * howo);
        const int oy = rem / p.ho, ox = rem - oy * p.ho;
        const int iy0 = oy * p.stride - 1, ix0 = ox * p.stride - 1;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = iy0 + ky;
            if ((unsigned)iy >= (unsigned)p.hin) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ix0 + kx;
                if ((unsigned)ix >= (unsigned)p.hin) continue;
                const size_t at = (((size_t)n * p.hin + iy) * p.hin + ix) * p.pitch + c;
                const h8 vh = *(const h8*)(p.x_hi + at);
                const h8 vl = *(const h8*)(p.x_lo + at);
                const float* wt = p.w + (size_t)(ky * 3 + kx) * p.pitch + c;
                const f4 w0 = *(const f4*)wt, w1 = *(const f4*)(wt + 4);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float x = (float)vh[j] + (float)vl[j];
                    acc[j] = __fmaf_rn(j < 4 ? w0[j & 3] : w1[j & 3], x, acc[j]);
                }
            }
        }
        const f4 s0 = *(const f4*)(p.scale + c), s1 = *(const f4*)(p.scale + c + 4);
        const f4 t0 = *(const f4*)(p.shift + c), t1 = *(const f4*)(p.shift + c + 4);
        h8 oh, ol;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float s = j < 4 ? s0[j & 3] : s1[j & 3], t = j < 4 ? t0[j & 3] : t1[j & 3];
            const float m = s * acc[j];
            const float v = m + t;
            half_t hi, lo;
            split_f32(v, hi, lo);
            oh[j] = hi;
            ol[j] = lo;
        }
        const size_t at_y = (size_t)pix * p.pitch + c;
        *(h8*)(p.y_hi + at_y) = oh;
        *(h8*)(p.y_lo + at_y) = ol;
        pix += dpix;
        k += dk;
        if (k >= cg) { k -= cg; ++pix; }
    }
}


#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

int main() {
    int cus = 256;
    CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    const int B = 2340;
    const int shapes[5][3] = {{28, 64, 1}, {14, 128, 1}, {7, 256, 1}, {56, 64, 2}, {28, 128, 2}};
    for (const auto& s : shapes) {
        const int hin = s[0], pitch = s[1], stride = s[2], ho = (hin - 1) / stride + 1;
        const size_t nin = (size_t)B * hin * hin * pitch, nout = (size_t)B * ho * ho * pitch;
        std::vector<uint16_t> hh(nin), hl(nin);
        unsigned st = 12345u + hin;
        for (size_t i = 0; i < nin; ++i) {
            st = st * 1664525u + 1013904223u;
            const float v = ((int)(st >> 8) % 20001 - 10000) * 3e-4f;     // -3 .. 3
            const half_t a = (half_t)v, b = (half_t)(v - (float)a);
            std::memcpy(&hh[i], &a, 2); std::memcpy(&hl[i], &b, 2);
        }
        std::vector<float> w(9 * pitch), sc(pitch), sh(pitch);
        for (int i = 0; i < 9 * pitch; ++i) { st = st * 1664525u + 1013904223u; w[i] = ((int)(st >> 8) % 2001 - 1000) * 1e-3f; }
        for (int i = 0; i < pitch; ++i) { st = st * 1664525u + 1013904223u; sc[i] = 0.5f + ((st >> 8) % 1000) * 1e-3f; sh[i] = ((int)(st >> 20) % 100 - 50) * 1e-2f; }
        half_t *xh, *xl, *y0h, *y0l, *y1h, *y1l; float *dw, *ds, *dt;
        CK(hipMalloc(&xh, nin * 2)); CK(hipMalloc(&xl, nin * 2));
        CK(hipMalloc(&y0h, nout * 2)); CK(hipMalloc(&y0l, nout * 2)); CK(hipMalloc(&y1h, nout * 2)); CK(hipMalloc(&y1l, nout * 2));
        CK(hipMalloc(&dw, w.size() * 4)); CK(hipMalloc(&ds, pitch * 4)); CK(hipMalloc(&dt, pitch * 4));
        CK(hipMemcpy(xh, hh.data(), nin * 2, hipMemcpyHostToDevice)); CK(hipMemcpy(xl, hl.data(), nin * 2, hipMemcpyHostToDevice));
        CK(hipMemcpy(dw, w.data(), w.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(ds, sc.data(), pitch * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(dt, sh.data(), pitch * 4, hipMemcpyHostToDevice));
        CK(hipMemset(y0h, 0xff, nout * 2)); CK(hipMemset(y0l, 0xff, nout * 2)); CK(hipMemset(y1h, 0xee, nout * 2)); CK(hipMemset(y1l, 0xee, nout * 2));
        DwParams p; std::memset(&p, 0, sizeof p);
        p.x_hi = xh; p.x_lo = xl; p.y_hi = y0h; p.y_lo = y0l; p.w = dw; p.scale = ds; p.shift = dt;
        p.npix = (long long)B * ho * ho; p.rows = (long long)B * ho; p.hin = hin; p.ho = ho; p.pitch = pitch; p.stride = stride;
        const unsigned long long units0 = (unsigned long long)p.npix * (pitch / 8);
        const unsigned grid0 = (unsigned)std::min<unsigned long long>((units0 + 255) / 256, (unsigned long long)cus * 8);
        DwParams q = p;
        q.y_hi = y1h; q.y_lo = y1l;
        const int Wd = stride == 1 ? 4 : 2;
        const long long q_units = (long long)B * ho * ((ho + Wd - 1) / Wd) * (pitch / 8);
        hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        for (int cap : {8, 2}) {
            const unsigned grid1 = (unsigned)std::min<long long>((q_units + 255) / 256, (long long)cus * cap);
            float best0 = 1e9f, best1 = 1e9f, sum0 = 0, sum1 = 0;
            const int reps = 7;
            for (int it = -2; it < reps; ++it) {
                float ms;
                CK(hipEventRecord(e0, 0));
                hipLaunchKernelGGL(dwconv3x3_bn_onepixel_kernel, dim3(grid0), dim3(256), 0, 0, p);
                CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
                if (it >= 0) { best0 = std::min(best0, ms); sum0 += ms; }
                CK(hipEventRecord(e0, 0));
                if (stride == 1) hipLaunchKernelGGL((dwconv_bn_act_kernel<3, 1, false>), dim3(grid1), dim3(256), 0, 0, q);
                else hipLaunchKernelGGL((dwconv_bn_act_kernel<3, 2, false>), dim3(grid1), dim3(256), 0, 0, q);
                CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
                if (it >= 0) { best1 = std::min(best1, ms); sum1 += ms; }
            }
            CK(hipGetLastError());
            printf("hin %2d pitch %3d stride %d batch %d cap %d blocks/CU: one-pixel mean %.3f ms (best %.3f), run form mean %.3f ms (best %.3f)\n",
                   hin, pitch, stride, B, cap, sum0 / reps, best0, sum1 / reps, best1);
        }
        std::vector<uint16_t> a(nout), b(nout);
        CK(hipMemcpy(a.data(), y0h, nout * 2, hipMemcpyDeviceToHost)); CK(hipMemcpy(b.data(), y1h, nout * 2, hipMemcpyDeviceToHost));
        const bool same_hi = std::memcmp(a.data(), b.data(), nout * 2) == 0;
        CK(hipMemcpy(a.data(), y0l, nout * 2, hipMemcpyDeviceToHost)); CK(hipMemcpy(b.data(), y1l, nout * 2, hipMemcpyDeviceToHost));
        const bool same_lo = std::memcmp(a.data(), b.data(), nout * 2) == 0;
        printf("hin %2d pitch %3d stride %d: outputs %s\n", hin, pitch, stride, same_hi && same_lo ? "bit-identical" : "DIFFERENT");
        if (!(same_hi && same_lo)) {
            std::vector<uint16_t> a2(nout), b2(nout);
            CK(hipMemcpy(a2.data(), y0h, nout * 2, hipMemcpyDeviceToHost)); CK(hipMemcpy(b2.data(), y1h, nout * 2, hipMemcpyDeviceToHost));
            size_t nd = 0, first = nout;
            for (size_t i = 0; i < nout; ++i) if (a2[i] != b2[i] || a[i] != b[i]) { if (first == nout) first = i; ++nd; }
            auto val = [&](uint16_t hb, uint16_t lb) { half_t x, y; std::memcpy(&x, &hb, 2); std::memcpy(&y, &lb, 2); return (double)(float)x + (double)(float)y; };
            const size_t i = first;
            const int c = (int)(i % pitch); const size_t pix = i / pitch; const int ox = (int)(pix % ho), oy = (int)((pix / ho) % ho); const size_t n = pix / ho / ho;
            float acc = 0.f;
            for (int ky = 0; ky < 3; ++ky) for (int kx = 0; kx < 3; ++kx) {
                const int iy = oy * stride - 1 + ky, ix = ox * stride - 1 + kx;
                if (iy < 0 || iy >= hin || ix < 0 || ix >= hin) continue;
                const size_t at = ((n * hin + iy) * hin + ix) * pitch + c;
                half_t x, y; std::memcpy(&x, &hh[at], 2); std::memcpy(&y, &hl[at], 2);
                acc = fmaf(w[(ky * 3 + kx) * pitch + c], (float)x + (float)y, acc);
            }
            volatile float m = sc[c] * acc; const float unfused = m + sh[c]; const float fused = fmaf(sc[c], acc, sh[c]);
            { int shown = 0; for (size_t q = 0; q < nout && shown < 4; ++q) if (a2[q] != b2[q] || a[q] != b[q]) { printf("    bits at %zu: one-pixel hi %04x lo %04x | run hi %04x lo %04x\n", q, a2[q], a[q], b2[q], b[q]); ++shown; } }
            printf("  %zu of %zu elements differ; first at n %zu oy %d ox %d c %d: one-pixel %.9g run %.9g | host unfused %.9g fused %.9g\n", nd, nout, n, oy, ox, c,
                   val(a2[i], a[i]), val(b2[i], b[i]), (double)unfused, (double)fused);
        }
        fflush(stdout);
        hipFree(xh); hipFree(xl); hipFree(y0h); hipFree(y0l); hipFree(y1h); hipFree(y1l); hipFree(dw); hipFree(ds); hipFree(dt);
    }
    return 0;
}
