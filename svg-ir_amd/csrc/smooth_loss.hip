// svg-ir_amd/csrc/smooth_loss.hip -- the edge-aware smoothness terms and the TV term both training stages add to their loss
// (utils/loss_utils.py:101-117; gaussian_renderer/svgss.py:366-399, render.py:192-196), fused: up to SVGIR_SMOOTH_MAX_TERMS terms of one
// image size in ONE forward launch (+ the small fixed-order reduction) and ONE backward launch; blockIdx.z is the term.
//
//   kind    inputs ([.,H,W] fp32 planes)                              value
//   first   data [C], img [Ci], data_mask / img_mask [1] or NULL      sum_{cb,k,p} |d_k D[c,p]| exp(-|d_k I[ci,p]|) / (Cb H W)
//   second  the same                                                  sum_{cb,k,p} |d_kk D[c,p]| exp(-10 |d_k I[ci,p]|) / (Cb H W)
//   tv      data [C]                                                  mean((x[:,1:,:] - x[:,:-1,:])^2) + mean((x[:,:,1:] - x[:,:,:-1])^2)
//
// D = data * data_mask, I = img * img_mask (one fp32 product each; a NULL mask is 1); C == Ci or one of them 1, Cb = max(C, Ci), c / ci =
// cb or 0 (torch broadcasting); k in {x, y}.  The derivatives are kornia's spatial_gradient(mode='sobel', normalized=True): the
// cross-correlation of the REPLICATE-padded plane with
//   order 1: Kx = (1 2 1)^T (-1 0 1) / 8, Ky = Kx^T;   order 2: Kxx = (1 4 6 4 1)^T (-1 0 2 0 -1) / 64, Kyy = Kxx^T
// (the mixed derivative is never used).  Every tap takes part with its integer weight, the zero ones included: 0 * inf is NaN, as in
// F.conv2d.
// Arithmetic: the VALUE of an element (cb, k, p) is evaluated in double from the fp32 planes (integer-weighted taps, the exact 1/8 or 1/64,
//   exp in double); signs and gradients are fp32 (expf, no contraction).  sign(0) = 0 (torch.abs's backward).  An element whose value is NaN
//   puts NaN into the loss and contributes to no gradient (the convention of geom_loss.hip); tv: a NaN difference likewise.
// forward : the data and img tiles of a 32 x 8 pixel workgroup are staged in LDS with a 2-pixel halo, coordinates clamped (the replicate
//           padding); every workgroup writes one record of 2 doubles per term {sum_a, sum_b} -- wave sums, then the four waves in order --
//           and the reduce kernel (one workgroup per term) adds the records in a fixed order: stats [n][4] = {sum_a, count_a, sum_b, count_b}
//           (first / second: count_a = Cb H W, the b pair 0; tv: a = rows, count C (H-1) W, b = columns, count C H (W-1)) and losses [n] =
//           float32(sum_a / count_a) (tv: float32(sum_a / count_a + sum_b / count_b); an empty mean is 0 / 0 = NaN as in torch).
// backward: a GATHER.  The workgroup recomputes, on its tile and a ring around it (2 pixels for the second-order data derivative, 1
//           otherwise), A[c,k,q] = d(loss)/d(d_k D[c,q]) and B[ci,k,q] = d(loss)/d(d_k I[ci,q]) into LDS (tiles with a 4-pixel halo); pixel p
//           then adds, row by row over the pixels q of its window, K_eff(q -> p) A[.,q], where K_eff is the sum of the taps o with
//           clamp(q + o) == p: one tap in the interior, the folded-back ones of the replicate padding on the border (K is separable, so
//           K_eff is a product of two small integer sums, exact).  d_data and d_img are each written completely when requested, times
//           their mask.  No atomics anywhere: two runs give the same bits.
#include "common.hpp"

namespace svgir {

int report_error(int code, const char* fmt, ...);   // api.hip

namespace {

constexpr int ST_X = 32, ST_Y = 8, ST_THREADS = ST_X * ST_Y, ST_MAXC = 4;
constexpr int SF_H = 2, SF_W = ST_X + 2 * SF_H, SF_R = ST_Y + 2 * SF_H;     // forward tiles: 2-pixel halo
constexpr int SB_H = 4, SB_W = ST_X + 2 * SB_H, SB_R = ST_Y + 2 * SB_H;     // backward tiles: 4-pixel halo
constexpr int SR_H = 2, SR_W = ST_X + 2 * SR_H, SR_R = ST_Y + 2 * SR_H;     // backward ring: up to 2 pixels
enum { KIND_FIRST = 1, KIND_SECOND = 2, KIND_TV = 3 };

struct SmoothArgs {
    int W, H;
    svgir_smooth_term t[SVGIR_SMOOTH_MAX_TERMS];
    double* partial;        // forward
    const double* stats;    // backward
    const float* g;         //          the n upstream scalars
};

// the separable factors of the kernels, as integers: smooth and derivative vector of halo HALO (1: Sobel, 2: the 5 x 5 second order)
template <int HALO> __device__ __forceinline__ int k_smooth(int o);
template <int HALO> __device__ __forceinline__ int k_deriv(int o);
template <> __device__ __forceinline__ int k_smooth<1>(int o) { return o == 0 ? 2 : 1; }
template <> __device__ __forceinline__ int k_deriv<1>(int o) { return o; }
template <> __device__ __forceinline__ int k_smooth<2>(int o) { return o == 0 ? 6 : ((o == 1 || o == -1) ? 4 : 1); }
template <> __device__ __forceinline__ int k_deriv<2>(int o) { return o == 0 ? 2 : ((o == 1 || o == -1) ? 0 : -1); }
template <int HALO> constexpr float k_scale() { return HALO == 1 ? 0.125f : 0.015625f; }

// d_x (K = 0) or d_y (K = 1) of the tile `s` (row stride `stride`) at (r, c), taps in row-major order, every tap with its integer weight
template <int HALO, int K, class T>
__device__ __forceinline__ T stencil(const float* s, int stride, int r, int c) {
    T acc = (T)0;
#pragma unroll
    for (int oy = -HALO; oy <= HALO; oy++)
#pragma unroll
        for (int ox = -HALO; ox <= HALO; ox++) {
            const int w = K == 0 ? k_smooth<HALO>(oy) * k_deriv<HALO>(ox) : k_deriv<HALO>(oy) * k_smooth<HALO>(ox);
            acc += (T)w * (T)s[(r + oy) * stride + (c + ox)];
        }
    return acc * (T)k_scale<HALO>();
}

__device__ __forceinline__ float sgn(float x) { return (float)(x > 0.f) - (float)(x < 0.f); }   // (NaN: 0)
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// `channels` planes of `src` times `mask` (NULL: 1) into LDS tiles [channels][rows][cols] whose origin is pixel (x0, y0); coordinates clamped
__device__ __forceinline__ void load_tile(const float* __restrict__ src, const float* __restrict__ mask, int channels, int W, int H, int x0,
                                          int y0, int rows, int cols, float* dst) {
    const size_t N = (size_t)W * H;
    for (int i = threadIdx.x; i < rows * cols; i += ST_THREADS) {
        const int r = i / cols, c = i - r * cols;
        const size_t pi = (size_t)clampi(y0 + r, H - 1) * W + clampi(x0 + c, W - 1);
        const float m = mask ? mask[pi] : 1.f;
        for (int ch = 0; ch < channels; ch++) dst[(ch * rows + r) * cols + c] = mask ? src[ch * N + pi] * m : src[ch * N + pi];
    }
}

template <int HALO>
__device__ __forceinline__ double edge_value(const svgir_smooth_term& tm, const float* sD, const float* sI, int r, int c, double sharp) {
    double gd[ST_MAXC][2], gi[ST_MAXC][2];
    for (int ch = 0; ch < tm.C; ch++) {
        gd[ch][0] = stencil<HALO, 0, double>(sD + ch * SF_R * SF_W, SF_W, r, c);
        gd[ch][1] = stencil<HALO, 1, double>(sD + ch * SF_R * SF_W, SF_W, r, c);
    }
    for (int ch = 0; ch < tm.Ci; ch++) {
        gi[ch][0] = stencil<1, 0, double>(sI + ch * SF_R * SF_W, SF_W, r, c);
        gi[ch][1] = stencil<1, 1, double>(sI + ch * SF_R * SF_W, SF_W, r, c);
    }
    const int Cb = tm.C > tm.Ci ? tm.C : tm.Ci;
    double v = 0.0;
    for (int cb = 0; cb < Cb; cb++) {
        const int c_ = tm.C == 1 ? 0 : cb, ci = tm.Ci == 1 ? 0 : cb;
        v += fabs(gd[c_][0]) * exp(-sharp * fabs(gi[ci][0]));
        v += fabs(gd[c_][1]) * exp(-sharp * fabs(gi[ci][1]));
    }
    return v;
}

__global__ void __launch_bounds__(ST_THREADS) smooth_loss_fwd_kernel(const SmoothArgs a) {
    __shared__ float sD[ST_MAXC * SF_R * SF_W], sI[ST_MAXC * SF_R * SF_W];
    __shared__ double sRed[2][ST_THREADS / 64];
    const svgir_smooth_term& tm = a.t[blockIdx.z];
    const int t = threadIdx.x, tx = t % ST_X, ty = t / ST_X;
    const int x = blockIdx.x * ST_X + tx, y = blockIdx.y * ST_Y + ty;
    const bool valid = x < a.W && y < a.H;
    const size_t N = (size_t)a.W * a.H;
    double va = 0.0, vb = 0.0;
    if (tm.kind == KIND_TV) {
        if (valid) {
            const size_t i = (size_t)y * a.W + x;
            for (int ch = 0; ch < tm.C; ch++) {
                const double v = (double)tm.data[ch * N + i];
                if (y + 1 < a.H) { const double e = (double)tm.data[ch * N + i + a.W] - v; va += e * e; }
                if (x + 1 < a.W) { const double e = (double)tm.data[ch * N + i + 1] - v; vb += e * e; }
            }
        }
    } else {
        const int x0 = blockIdx.x * ST_X - SF_H, y0 = blockIdx.y * ST_Y - SF_H;
        load_tile(tm.data, tm.data_mask, tm.C, a.W, a.H, x0, y0, SF_R, SF_W, sD);
        load_tile(tm.img, tm.img_mask, tm.Ci, a.W, a.H, x0, y0, SF_R, SF_W, sI);
        __syncthreads();
        if (valid)
            va = tm.kind == KIND_FIRST ? edge_value<1>(tm, sD, sI, ty + SF_H, tx + SF_H, 1.0) : edge_value<2>(tm, sD, sI, ty + SF_H, tx + SF_H, 10.0);
    }
    // workgroup sums in a fixed order: xor butterflies inside the waves, then the four waves in order
    double s[2] = {wave_reduce_add(va), wave_reduce_add(vb)};
    block_sum_ordered(s, sRed);
    if (t == 0) {
        const size_t nblk = (size_t)gridDim.x * gridDim.y, blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        a.partial[2 * (blockIdx.z * nblk + blk)] = s[0];
        a.partial[2 * (blockIdx.z * nblk + blk) + 1] = s[1];
    }
}

// the records of term blockIdx.x -> its stats row and its loss: one workgroup, fixed order, double
__global__ void __launch_bounds__(256) smooth_loss_reduce_kernel(const SmoothArgs a, int nblk, double* __restrict__ stats, float* __restrict__ losses) {
    __shared__ double red[2][4];
    const int k = blockIdx.x;
    const svgir_smooth_term& tm = a.t[k];
    double s[2];
    block_reduce_records(a.partial + 2 * (size_t)k * nblk, nblk, 2, s, red);
    if (threadIdx.x == 0) {
        const double sa = s[0], sb = s[1];
        const double W = a.W, H = a.H, C = tm.C, Cb = tm.C > tm.Ci ? tm.C : tm.Ci;
        const bool tv = tm.kind == KIND_TV;
        const double ca = tv ? C * (H - 1.0) * W : Cb * H * W, cb = tv ? C * H * (W - 1.0) : 0.0;
        stats[4 * k] = sa; stats[4 * k + 1] = ca; stats[4 * k + 2] = tv ? sb : 0.0; stats[4 * k + 3] = cb;
        losses[k] = tv ? (float)(sa / ca + sb / cb) : (float)(sa / ca);   // (an empty mean: 0 / 0 = NaN, as torch's)
    }
}

// A and B of the ring pixels (see the head of the file); DH = the halo of the data derivative
template <int DH>
__device__ __forceinline__ void edge_ring(const svgir_smooth_term& tm, int W, int H, float gs, float sharp, const float* sD, const float* sI,
                                          float* sA, float* sB) {
#pragma clang fp contract(off)
    const int rx0 = blockIdx.x * ST_X - SR_H, ry0 = blockIdx.y * ST_Y - SR_H;
    const int Cb = tm.C > tm.Ci ? tm.C : tm.Ci;
    const bool want_b = tm.d_img != nullptr;
    for (int e = threadIdx.x; e < SR_R * SR_W; e += ST_THREADS) {
        const int r = e / SR_W, c = e - r * SR_W, px = rx0 + c, py = ry0 + r;
        float A[ST_MAXC][2], B[ST_MAXC][2];
#pragma unroll
        for (int ch = 0; ch < ST_MAXC; ch++) { A[ch][0] = A[ch][1] = B[ch][0] = B[ch][1] = 0.f; }
        if (px >= 0 && px < W && py >= 0 && py < H) {
            const int tr = r + SB_H - SR_H, tc = c + SB_H - SR_H;
            float gd[ST_MAXC][2], gi[ST_MAXC][2];
            for (int ch = 0; ch < tm.C; ch++) {
                gd[ch][0] = stencil<DH, 0, float>(sD + ch * SB_R * SB_W, SB_W, tr, tc);
                gd[ch][1] = stencil<DH, 1, float>(sD + ch * SB_R * SB_W, SB_W, tr, tc);
            }
            for (int ch = 0; ch < tm.Ci; ch++) {
                gi[ch][0] = stencil<1, 0, float>(sI + ch * SB_R * SB_W, SB_W, tr, tc);
                gi[ch][1] = stencil<1, 1, float>(sI + ch * SB_R * SB_W, SB_W, tr, tc);
            }
            for (int cb = 0; cb < Cb; cb++) {
                const int c_ = tm.C == 1 ? 0 : cb, ci = tm.Ci == 1 ? 0 : cb;
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const float ad = fabsf(gd[c_][k]), w = expf(-sharp * fabsf(gi[ci][k]));
                    const float v = ad * w;
                    if (v != v) continue;                                  // a NaN element contributes to no gradient
                    A[c_][k] = add_rn(A[c_][k], sgn(gd[c_][k]) * (gs * w));
                    if (want_b) B[ci][k] = add_rn(B[ci][k], sgn(gi[ci][k]) * ((gs * v) * -sharp));
                }
            }
        }
#pragma unroll
        for (int ch = 0; ch < ST_MAXC; ch++) {
#pragma unroll
            for (int k = 0; k < 2; k++) {
                sA[((ch * 2 + k) * SR_R + r) * SR_W + c] = A[ch][k];
                sB[((ch * 2 + k) * SR_R + r) * SR_W + c] = B[ch][k];
            }
        }
    }
}

// sum of v(o) over the taps o of one axis with clamp(q + o) == p, |o| <= HALO: o = p - q in the interior, every tap that the replicate
// padding folds back onto p on the border.  (lo > hi: none.)
__device__ __forceinline__ void tap_range(int p, int q, int n, int halo, int& lo, int& hi) {
    lo = hi = p - q;
    if (p == 0) lo = -halo;
    if (p == n - 1) hi = halo;
    lo = lo < -halo ? -halo : lo;
    hi = hi > halo ? halo : hi;
}

// the gather of pixel (x, y), tile-local (ty, tx), for `channels` planes of the ring buffer s[ch][k][SR_R][SR_W]
template <int HALO>
__device__ __forceinline__ void gather(const float* s, int channels, int W, int H, int x, int y, int ty, int tx, float* out) {
#pragma clang fp contract(off)
    for (int ch = 0; ch < channels; ch++) out[ch] = 0.f;
    for (int dy = -HALO; dy <= HALO; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= H) continue;
        int lo, hi, sy_s = 0, sy_d = 0;
        tap_range(y, qy, H, HALO, lo, hi);
        for (int o = lo; o <= hi; o++) { sy_s += k_smooth<HALO>(o); sy_d += k_deriv<HALO>(o); }
        for (int dx = -HALO; dx <= HALO; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            int sx_s = 0, sx_d = 0;
            tap_range(x, qx, W, HALO, lo, hi);
            for (int o = lo; o <= hi; o++) { sx_s += k_smooth<HALO>(o); sx_d += k_deriv<HALO>(o); }
            const float kx = (float)(sy_s * sx_d) * k_scale<HALO>(), ky = (float)(sy_d * sx_s) * k_scale<HALO>();   // exact
            const int ri = (ty + SR_H + dy) * SR_W + (tx + SR_H + dx);
            for (int ch = 0; ch < channels; ch++) {
                out[ch] = add_rn(out[ch], kx * s[(ch * 2 + 0) * SR_R * SR_W + ri]);
                out[ch] = add_rn(out[ch], ky * s[(ch * 2 + 1) * SR_R * SR_W + ri]);
            }
        }
    }
}

__global__ void __launch_bounds__(ST_THREADS) smooth_loss_bwd_kernel(const SmoothArgs a) {
    __shared__ float sD[ST_MAXC * SB_R * SB_W], sI[ST_MAXC * SB_R * SB_W];
    __shared__ float sA[ST_MAXC * 2 * SR_R * SR_W], sB[ST_MAXC * 2 * SR_R * SR_W];
    const svgir_smooth_term& tm = a.t[blockIdx.z];
    if (!tm.d_data && !tm.d_img) return;
    const int t = threadIdx.x, tx = t % ST_X, ty = t / ST_X;
    const int x = blockIdx.x * ST_X + tx, y = blockIdx.y * ST_Y + ty;
    const bool valid = x < a.W && y < a.H;
    const size_t N = (size_t)a.W * a.H, i = (size_t)y * a.W + x;
    const float g = a.g[blockIdx.z];
    const double* st = a.stats + 4 * blockIdx.z;
    if (tm.kind == KIND_TV) {
#pragma clang fp contract(off)
        if (!valid) return;
        const float ca = (float)st[1], cb = (float)st[3];
        const float ga = ca > 0.f ? 2.f * g / ca : 0.f, gb = cb > 0.f ? 2.f * g / cb : 0.f;   // (an empty mean: zero gradient)
        for (int ch = 0; ch < tm.C; ch++) {
            const float* p = tm.data + ch * N + i;
            const float v = *p;
            float d = 0.f, e;
            if (y > 0) { e = v - p[-a.W]; if (e == e) d = add_rn(d, ga * e); }
            if (y + 1 < a.H) { e = p[a.W] - v; if (e == e) d = add_rn(d, -(ga * e)); }
            if (x > 0) { e = v - p[-1]; if (e == e) d = add_rn(d, gb * e); }
            if (x + 1 < a.W) { e = p[1] - v; if (e == e) d = add_rn(d, -(gb * e)); }
            tm.d_data[ch * N + i] = d;
        }
        return;
    }
    const int x0 = blockIdx.x * ST_X - SB_H, y0 = blockIdx.y * ST_Y - SB_H;
    load_tile(tm.data, tm.data_mask, tm.C, a.W, a.H, x0, y0, SB_R, SB_W, sD);
    load_tile(tm.img, tm.img_mask, tm.Ci, a.W, a.H, x0, y0, SB_R, SB_W, sI);
    __syncthreads();
    const float gs = g / (float)st[1];
    if (tm.kind == KIND_FIRST) edge_ring<1>(tm, a.W, a.H, gs, 1.f, sD, sI, sA, sB);
    else edge_ring<2>(tm, a.W, a.H, gs, 10.f, sD, sI, sA, sB);
    __syncthreads();
    if (!valid) return;
    float out[ST_MAXC];
    if (tm.d_data) {
        if (tm.kind == KIND_FIRST) gather<1>(sA, tm.C, a.W, a.H, x, y, ty, tx, out);
        else gather<2>(sA, tm.C, a.W, a.H, x, y, ty, tx, out);
        const float m = tm.data_mask ? tm.data_mask[i] : 1.f;
        for (int ch = 0; ch < tm.C; ch++) tm.d_data[ch * N + i] = tm.data_mask ? out[ch] * m : out[ch];
    }
    if (tm.d_img) {
        gather<1>(sB, tm.Ci, a.W, a.H, x, y, ty, tx, out);
        const float m = tm.img_mask ? tm.img_mask[i] : 1.f;
        for (int ch = 0; ch < tm.Ci; ch++) tm.d_img[ch * N + i] = tm.img_mask ? out[ch] * m : out[ch];
    }
}

int check_args(const char* what, int32_t W, int32_t H, int32_t n_terms, const svgir_smooth_term* terms, bool backward) {
    if (W < 0 || H < 0) return report_error(SVGIR_ERR_INVALID, "%s: bad image size W=%d H=%d", what, W, H);
    if (n_terms < 1 || n_terms > SVGIR_SMOOTH_MAX_TERMS)
        return report_error(SVGIR_ERR_INVALID, "%s: n_terms=%d outside 1 ... %d", what, n_terms, SVGIR_SMOOTH_MAX_TERMS);
    if (!terms) return report_error(SVGIR_ERR_INVALID, "%s: the term descriptors must be provided", what);
    bool any = false;
    for (int k = 0; k < n_terms; k++) {
        const svgir_smooth_term& t = terms[k];
        if (t.kind < KIND_FIRST || t.kind > KIND_TV)
            return report_error(SVGIR_ERR_INVALID, "%s: term %d has unknown kind %d (1 first, 2 second, 3 tv)", what, k, t.kind);
        if (t.C < 1 || t.C > ST_MAXC) return report_error(SVGIR_ERR_INVALID, "%s: term %d has C=%d outside 1 ... %d", what, k, t.C, ST_MAXC);
        if (!t.data) return report_error(SVGIR_ERR_INVALID, "%s: term %d needs its data plane", what, k);
        if (t.kind == KIND_TV) {
            if (t.Ci != 0 || t.img || t.img_mask || t.data_mask || t.d_img)
                return report_error(SVGIR_ERR_INVALID, "%s: term %d is a tv term: Ci = 0, no img and no masks", what, k);
        } else {
            if (t.Ci < 1 || t.Ci > ST_MAXC) return report_error(SVGIR_ERR_INVALID, "%s: term %d has Ci=%d outside 1 ... %d", what, k, t.Ci, ST_MAXC);
            if (t.C != t.Ci && t.C != 1 && t.Ci != 1)
                return report_error(SVGIR_ERR_INVALID, "%s: term %d cannot broadcast C=%d against Ci=%d", what, k, t.C, t.Ci);
            if (!t.img) return report_error(SVGIR_ERR_INVALID, "%s: term %d needs its img plane", what, k);
        }
        any = any || t.d_data || t.d_img;
    }
    if (backward && !any) return report_error(SVGIR_ERR_INVALID, "%s: no gradient requested", what);
    return 0;
}

SmoothArgs make_args(int32_t W, int32_t H, int32_t n_terms, const svgir_smooth_term* terms) {
    SmoothArgs a{};
    a.W = W; a.H = H;
    for (int k = 0; k < n_terms; k++) a.t[k] = terms[k];
    return a;
}

}  // namespace

}  // namespace svgir

using namespace svgir;

extern "C" {

size_t svgir_smooth_loss_partials(int32_t W, int32_t H, int32_t n_terms) {
    if (W <= 0 || H <= 0 || n_terms <= 0) return 0;
    return (size_t)((W + ST_X - 1) / ST_X) * ((H + ST_Y - 1) / ST_Y) * (size_t)n_terms;
}

int svgir_smooth_loss_forward(int32_t W, int32_t H, int32_t n_terms, const svgir_smooth_term* terms, double* partial, double* stats,
                              float* losses, void* stream) {
    if (int rc = check_args("smooth_loss_forward", W, H, n_terms, terms, false)) return rc;
    if (!partial || !stats || !losses) return report_error(SVGIR_ERR_INVALID, "smooth_loss_forward: partial, stats and losses must be provided");
    if (W == 0 || H == 0) return SVGIR_OK;
    SmoothArgs a = make_args(W, H, n_terms, terms);
    a.partial = partial;
    const dim3 grid((W + ST_X - 1) / ST_X, (H + ST_Y - 1) / ST_Y, n_terms);
    hipStream_t s = (hipStream_t)stream;
    StageMarks tm = stage_begin(s);
    hipLaunchKernelGGL(smooth_loss_fwd_kernel, grid, dim3(ST_THREADS), 0, s, a);
    hipLaunchKernelGGL(smooth_loss_reduce_kernel, dim3(n_terms), dim3(256), 0, s, a, (int)(grid.x * grid.y), stats, losses);
    stage_mark(tm, "smooth_loss_fwd");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SVGIR_OK : report_error(SVGIR_ERR_HIP, "smooth_loss_forward launch failed: %s", hipGetErrorString(e));
}

int svgir_smooth_loss_backward(int32_t W, int32_t H, int32_t n_terms, const svgir_smooth_term* terms, const double* stats, const float* g,
                               void* stream) {
    if (int rc = check_args("smooth_loss_backward", W, H, n_terms, terms, true)) return rc;
    if (!stats || !g) return report_error(SVGIR_ERR_INVALID, "smooth_loss_backward: stats and the upstream gradients must be provided");
    if (W == 0 || H == 0) return SVGIR_OK;
    SmoothArgs a = make_args(W, H, n_terms, terms);
    a.stats = stats; a.g = g;
    const dim3 grid((W + ST_X - 1) / ST_X, (H + ST_Y - 1) / ST_Y, n_terms);
    hipStream_t s = (hipStream_t)stream;
    StageMarks tm = stage_begin(s);
    hipLaunchKernelGGL(smooth_loss_bwd_kernel, grid, dim3(ST_THREADS), 0, s, a);
    stage_mark(tm, "smooth_loss_bwd");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SVGIR_OK : report_error(SVGIR_ERR_HIP, "smooth_loss_backward launch failed: %s", hipGetErrorString(e));
}

}  // extern "C"
