// svg-ir_amd/csrc/ssim_tile.hpp -- the SSIM tile of the reference's 11 x 11 Gaussian window (utils/loss_utils.py:21-64), once: the window, the
// zero-padded halo load, the separable window pass through LDS and the per-pixel SSIM arithmetic.  Included by csrc/loss.hip (the training
// loss, forward and backward) and csrc/view_metrics.hip (the eval metric) only; that the two give the same bits rests on these lines.
// Workgroups are LT x LT threads, thread (tx, ty) = (threadIdx.x & 15, threadIdx.x >> 4) owns pixel (tile origin + (tx, ty)).
#pragma once
#include "common.hpp"

namespace svgir {

constexpr int LT = 16, LR = 5, LW = LT + 2 * LR;   // output tile, window radius, input tile with halo

struct SsimWindow { float g[11]; };
inline SsimWindow ssim_window() {
    // utils/loss_utils.py:21-23: fp32 tensor of exp(-(x - 5)^2 / (2 * 1.5^2)), divided by its fp32 sum
    SsimWindow w;
    float s = 0.f;
    for (int i = 0; i < 11; i++) { w.g[i] = (float)exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); s += w.g[i]; }
    for (int i = 0; i < 11; i++) w.g[i] /= s;
    return w;
}

// the workgroup's halo tiles of NP planes: s[q][r][c] = src(q, y * W + x) inside the image, 0 outside (loss_utils.py:45: padding =
// window_size // 2).  No barrier: the caller puts one in front of the first read.
template <int NP, class Src>
__device__ __forceinline__ void ssim_load_halo(float (*s)[LW][LW + 1], int H, int W, Src src) {
    const int x0 = blockIdx.x * LT - LR, y0 = blockIdx.y * LT - LR;
    for (int i = threadIdx.x; i < LW * LW; i += LT * LT) {
        const int r = i / LW, c = i - r * LW;
        const int y = y0 + r, x = x0 + c;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
#pragma unroll
        for (int q = 0; q < NP; q++) s[q][r][c] = in ? src(q, (size_t)y * W + x) : 0.f;
    }
}

// one separable window pass over NP planes: out[p] = (w * plane p) at the thread's pixel.  tap(r, c, v) gives v[0 .. NP) at halo-tile
// position (r, c).  Horizontal pass (rows of the halo tile, 16 output columns) into sH, ONE barrier, vertical pass; taps in order 0 .. 10.
template <int NP, class Tap>
__device__ __forceinline__ void ssim_window_pass(const SsimWindow& win, float (*sH)[LW][LT + 1], Tap tap, float (&out)[NP]) {
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    for (int i = threadIdx.x; i < LW * LT; i += LT * LT) {
        const int r = i / LT, c = i - r * LT;
        float acc[NP] = {};
#pragma unroll
        for (int k = 0; k < 11; k++) {
            const float g = win.g[k];
            float v[NP];
            tap(r, c + k, v);
#pragma unroll
            for (int p = 0; p < NP; p++) acc[p] += g * v[p];
        }
#pragma unroll
        for (int p = 0; p < NP; p++) sH[p][r][c] = acc[p];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < NP; p++) out[p] = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
        const float g = win.g[k];
#pragma unroll
        for (int p = 0; p < NP; p++) out[p] += g * sH[p][ty + k][tx];
    }
}

// the five windowed moments of the image pair in the halo tiles s[0], s[1]: mu1, mu2, E[x^2], E[y^2], E[x y]
__device__ __forceinline__ void ssim_moments(const SsimWindow& win, const float (*s)[LW][LW + 1], float (*sH)[LW][LT + 1], float (&m)[5]) {
    ssim_window_pass<5>(win, sH, [&](int r, int c, float (&v)[5]) {
        const float u = s[0][r][c], w = s[1][r][c];
        v[0] = u; v[1] = w; v[2] = u * u; v[3] = w * w; v[4] = u * w;
    }, m);
}

// the SSIM value of a pixel from its five moments, with the intermediates its derivatives need
struct SsimPixel { float S, A1, A2, iB1, iB2, mu1, mu2; };
__device__ __forceinline__ SsimPixel ssim_pixel(const float (&m)[5]) {
    const float mu1 = m[0], mu2 = m[1], e11 = m[2], e22 = m[3], e12 = m[4];
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float s1 = e11 - mu1 * mu1, s2 = e22 - mu2 * mu2, s12 = e12 - mu1 * mu2;
    // (mu1 * mu1 + mu2 * mu2 is the one sum here that contracts two ways, and the compiler's pick follows the code around it: pinned to
    // the fma both kernels have always had)
    const float A1 = 2.f * mu1 * mu2 + C1, A2 = 2.f * s12 + C2, B1 = __builtin_fmaf(mu2, mu2, mu1 * mu1) + C1, B2 = s1 + s2 + C2;
    const float iB1 = 1.f / B1, iB2 = 1.f / B2;
    const float S = (A1 * A2) * (iB1 * iB2);
    return {S, A1, A2, iB1, iB2, mu1, mu2};
}

}  // namespace svgir
