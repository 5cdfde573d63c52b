// svg-ir_amd/csrc/d2n.hpp -- the per-pixel arithmetic of depth2normal (utils/image_utils.py:61-125) and of its adjoint, shared by
// depth2normal_kernel / depth2normal_bwd_kernel (epilogue.hip) and the fused geometry-loss kernels (geom_loss.hip): ONE device
// function each, so the pseudo normal the surface loss selects on is the one svgir_depth2normal writes.
//
// `at(xx, yy, d, m)` hands out the depth and the raw mask value of an IN-IMAGE pixel (the callers' coordinates are clamped here:
// replicate padding); epilogue.hip reads global memory, geom_loss.hip an LDS tile.
#pragma once
#include <hip/hip_runtime.h>

#if defined(__HIPCC__)
namespace svgir {

// K = diag(focal(FoVy, H), focal(FoVx, W)) as in the reference; principal point in pixels.  T = float everywhere but in the value of
// the fused surface loss, which restates the same arithmetic in double (geom_loss.hip)
template <class T> struct D2nCamT { int W, H; T k00, k11, ppx, ppy; };
using D2nCam = D2nCamT<float>;

template <class T>
__device__ __forceinline__ void d2n_cross(const T* a, const T* b_, T* o) {
    o[0] = a[1] * b_[2] - a[2] * b_[1]; o[1] = a[2] * b_[0] - a[0] * b_[2]; o[2] = a[0] * b_[1] - a[1] * b_[0];
}

// back-project the pixel and its four neighbours (replicate padding), mask, sum of the four cross products of neighbouring
// differences, normalise, mask: out[3] = the pseudo normal of pixel (x, y)
template <class T, class At>
__device__ __forceinline__ void d2n_normal(const D2nCamT<T>& k, int x, int y, At at, T* out) {
    auto cam = [&](int xx, int yy, T* p, T& m) {
        xx = min(max(xx, 0), k.W - 1); yy = min(max(yy, 0), k.H - 1);
        float df, mv;
        at(xx, yy, df, mv);
        const T d = df;
        m = mv != 0.f ? T(1) : T(0);
        p[0] = ((T)xx - k.ppx) * d / k.k00; p[1] = ((T)yy - k.ppy) * d / k.k11; p[2] = d;
    };
    T pc[3], pu[3], pl[3], pb[3], pr[3], mc, mu, ml, mb, mr;
    cam(x, y, pc, mc); cam(x, y - 1, pu, mu); cam(x - 1, y, pl, ml); cam(x, y + 1, pb, mb); cam(x + 1, y, pr, mr);
    T c[3], u[3], l[3], b[3], r[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        c[j] = pc[j] * mc;
        u[j] = (pu[j] - c[j]) * mu; l[j] = (pl[j] - c[j]) * ml; b[j] = (pb[j] - c[j]) * mb; r[j] = (pr[j] - c[j]) * mr;
    }
    T n1[3], n2[3], n3[3], n4[3];
    d2n_cross(u, l, n1); d2n_cross(r, u, n2); d2n_cross(b, r, n3); d2n_cross(l, b, n4);
    T n[3] = {n1[0] + n2[0] + n3[0] + n4[0], n1[1] + n2[1] + n3[1] + n4[1], n1[2] + n2[2] + n3[2] + n4[2]};
    const T len = fmax(sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), (T)1e-12f);   // (the float overloads are fmaxf / sqrtf)
#pragma unroll
    for (int j = 0; j < 3; j++) out[j] = n[j] / len * mc;
}

// adjoint of d2n_normal: gd[q] = d(loss)/d(depth read q) of pixel (x, y) under the gradient g_in[3] of its own normal; the reads are
// q = 0 centre, 1 up, 2 left, 3 bottom, 4 right, at the CLAMPED coordinates (a read that leaves the image lands on the pixel itself)
template <class At>
__device__ __forceinline__ void d2n_adjoint(const D2nCam& k, int x, int y, At at, const float* g_in, float* gd) {
    float ray[5][3], m[5];
    float p[5][3];
    const int ox[5] = {0, 0, -1, 0, 1}, oy[5] = {0, -1, 0, 1, 0};   // centre, up, left, bottom, right
#pragma unroll
    for (int q = 0; q < 5; q++) {
        const int xx = min(max(x + ox[q], 0), k.W - 1), yy = min(max(y + oy[q], 0), k.H - 1);
        float d, mv;
        at(xx, yy, d, mv);
        m[q] = mv != 0.f ? 1.f : 0.f;
        ray[q][0] = ((float)xx - k.ppx) / k.k00; ray[q][1] = ((float)yy - k.ppy) / k.k11; ray[q][2] = 1.f;
        p[q][0] = ((float)xx - k.ppx) * d / k.k00; p[q][1] = ((float)yy - k.ppy) * d / k.k11; p[q][2] = d;
    }
    float c[3], e[5][3];   // e[1..4] = u, l, b, r
#pragma unroll
    for (int j = 0; j < 3; j++) {
        c[j] = p[0][j] * m[0];
#pragma unroll
        for (int q = 1; q < 5; q++) e[q][j] = (p[q][j] - c[j]) * m[q];
    }
    const float *u = e[1], *l = e[2], *b = e[3], *r = e[4];
    float n1[3], n2[3], n3[3], n4[3], n[3];
    d2n_cross(u, l, n1); d2n_cross(r, u, n2); d2n_cross(b, r, n3); d2n_cross(l, b, n4);
#pragma unroll
    for (int j = 0; j < 3; j++) n[j] = n1[j] + n2[j] + n3[j] + n4[j];
    // normal = n / max(|n|, 1e-12) * mask_c
    float g[3] = {g_in[0] * m[0], g_in[1] * m[0], g_in[2] * m[0]};
    const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    float gn[3];
    if (len > 1e-12f) {
        const float dot = (n[0] * g[0] + n[1] * g[1] + n[2] * g[2]) / (len * len);
#pragma unroll
        for (int j = 0; j < 3; j++) gn[j] = (g[j] - n[j] * dot) / len;
    } else {
#pragma unroll
        for (int j = 0; j < 3; j++) gn[j] = g[j] / 1e-12f;
    }
    // n = u x l + r x u + b x r + l x b;  for a x b: d/da = b x g, d/db = g x a
    float t1[3], t2[3], ge[5][3];
    d2n_cross(l, gn, t1); d2n_cross(gn, r, t2);
#pragma unroll
    for (int j = 0; j < 3; j++) ge[1][j] = t1[j] + t2[j];   // u
    d2n_cross(gn, u, t1); d2n_cross(b, gn, t2);
#pragma unroll
    for (int j = 0; j < 3; j++) ge[2][j] = t1[j] + t2[j];   // l
    d2n_cross(r, gn, t1); d2n_cross(gn, l, t2);
#pragma unroll
    for (int j = 0; j < 3; j++) ge[3][j] = t1[j] + t2[j];   // b
    d2n_cross(u, gn, t1); d2n_cross(gn, b, t2);
#pragma unroll
    for (int j = 0; j < 3; j++) ge[4][j] = t1[j] + t2[j];   // r
    float gc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 5; q++) gd[q] = 0.f;
#pragma unroll
    for (int q = 1; q < 5; q++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const float gp = ge[q][j] * m[q];       // e = (p_q - c) m_q
            gd[q] += gp * ray[q][j];
            gc[j] -= gp;
        }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) gd[0] += gc[j] * m[0] * ray[0][j];   // c = p_c m_c
}

}  // namespace svgir
#endif
