// svg-ir_amd/csrc/geom_loss.hip -- the geometry terms both training stages add to the photometric loss (gaussian_renderer/render.py:157-188,
// svgss.py:297-313, 333-338), fused: ONE forward launch (+ the small fixed-order reduction) and ONE backward launch for up to four terms.
//
//   term     inputs ([.,H,W] fp32 planes)                      value
//   surface  normal [3], depth [1], mask [1], camera            cos_loss(normal, depth2normal(depth, mask, cam)); the pseudo normal lives in
//                                                               registers / LDS only (d2n_normal of d2n.hpp: the function depth2normal_kernel runs)
//   target   normal [3], target [3], weight [1] or NULL (= 1)   cos_loss(normal, target, weight=weight) (the mono-normal term)
//   mask     opacity [1], mask [1]                              mean(opacity * (1 - MaxPool2d(9, 1, 4)(mask)))
//   entropy  opacity [1], mask [1]                              -mean(m log o + (1 - m) log(1 - o)), o = clamp(opacity, lo, hi)
//
// cos_loss (utils/loss_utils.py:119-121): cos = sum_c (output_c * gt_c) * weight; a pixel is selected iff cos < 1 (np.cos(0)); loss =
//   sum_selected (1 - cos) / count.  The compare is `cos < 1.f`: a NaN cos is not selected and gets ZERO gradient (the reference's autograd
//   would give it 0 * NaN).  A background pixel (both normals zero, cos = 0) is selected and contributes 1, as in the reference.
//   count == 0: loss = 0 / 0 = NaN (torch's mean of an empty selection) and every gradient of the term is zero.
//   cos is evaluated in fp32 WITHOUT contraction in the order ((o0 g0) w + (o1 g1) w) + (o2 g2) w (cos3 below), so the selection and the count
//   are a pure function of the inputs; in the surface form gt is the kernel's own fp32 pseudo normal, and a pixel whose exact cos lies
//   within rounding of 1 may fall on either side.  The VALUE of a selected pixel is 1 - cos in double (cos3d below).
// maxpool9: the 9 x 9 window clipped to the image (torch pads with -inf), separable over an LDS tile of the mask with a 4-pixel halo.
// entropy clamp: lo = float32(1e-6), hi = float32(1 - 1e-6); the gradient passes where lo <= opacity <= hi, bounds included; NaN propagates
//   into the loss as torch.clamp's does and gets zero gradient.
//
// forward : every workgroup (a 32 x 8 pixel tile) writes one record of 8 doubles {surface sum, count, target sum, count, mask sum, 0,
//           entropy sum, 0} -- wave sums, then the four waves in order --; the reduce kernel adds the records in a fixed order in double
//           and writes stats [4][2] = {sum, count} per term in double (count = H W for the two means) and the four losses, float32(sum / count).  No atomics: two runs
//           give the same bits.
// backward: upstream gradients are four device floats.  dL_dnormal [3,H,W] (surface + target), dL_ddepth [1,H,W] (through the pseudo
//           normal) and dL_dopacity [1,H,W] are each written completely when requested.  dL_ddepth is a GATHER: the workgroup evaluates
//           the adjoint of depth2normal (d2n_adjoint of d2n.hpp) once per pixel of its tile and a 1-pixel ring around it -- recomputing the
//           ring's pseudo normals, selection and -normal sel / count -- into LDS (depth / mask tile with a 2-pixel halo), and every pixel
//           then adds, in a fixed order, its own centre contribution and what its four neighbours' reads of it (or its own reads that
//           the replicate padding folds back onto it) contribute.  No atomics here either.
#include "common.hpp"
#include "d2n.hpp"

namespace svgir {

int report_error(int code, const char* fmt, ...);   // api.hip (it owns the per-thread message behind svgir_last_error): records it, returns `code`

namespace {

constexpr int GT_X = 32, GT_Y = 8, GT_MH = 4, GT_DH = 2;             // tile, mask halo (9 x 9 pool), depth halo (ring of adjoints)
constexpr int GT_MW = GT_X + 2 * GT_MH, GT_MR = GT_Y + 2 * GT_MH;     // mask tile
constexpr int GT_DW = GT_X + 2 * GT_DH, GT_DR = GT_Y + 2 * GT_DH;     // depth tile
constexpr int GT_RW = GT_X + 2, GT_RR = GT_Y + 2;                     // tile + ring
constexpr int GT_THREADS = GT_X * GT_Y;
enum { TERM_SURFACE = 1, TERM_TARGET = 2, TERM_MASK = 4, TERM_ENTROPY = 8 };

struct GeomLossArgs {
    int W, H, terms;
    D2nCam cam;
    D2nCamT<double> camd;                              // the same camera in double: the VALUE of the surface term (see cos3d)
    const float *normal, *depth, *mask, *opacity, *target, *weight;
    double* partial;                                   // forward
    const double* stats;                               // backward: {sum, count} x 4 of the forward
    const float* g;                                    //           the four upstream scalars
    float *d_normal, *d_depth, *d_opacity;
};

// a + b rounded on its own: never fused with the product that made b, so a gradient with two terms is the fp32 sum of the single ones
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float cos3(const float* o, const float* g, float w) {
#pragma clang fp contract(off)
    const float a = (o[0] * g[0]) * w, b = (o[1] * g[1]) * w, c = (o[2] * g[2]) * w;
    return (a + b) + c;
}

// The VALUE of a selected pixel is 1 - cos with cos in double (the surface form: on the pseudo normal restated in double from the same
// fp32 depth, d2n_normal<double>), so that the loss carries no rounding of its own beyond the final one to fp32; the SELECTION, the count
// and the gradients stay on the fp32 cos3 above.  (1.f - cos3 loses up to 6e-8 per pixel on a cos near 1, which does not average out
// on a small image: it showed as 6e-9 on a loss of 2.7e-3 at 16 x 16.)
__device__ __forceinline__ double cos3d(const float* o, const double* g, float w) {
    return (((double)o[0] * g[0]) * (double)w + ((double)o[1] * g[1]) * (double)w) + ((double)o[2] * g[2]) * (double)w;
}

// the mask tile (-inf outside the image: the pool's padding) and the depth tile of the workgroup
__device__ __forceinline__ void load_tiles(const GeomLossArgs& a, bool want_mask, bool want_depth, float (*sMask)[GT_MW], float (*sDepth)[GT_DW]) {
    const int t = threadIdx.x;
    if (want_mask) {
        const int x0 = blockIdx.x * GT_X - GT_MH, y0 = blockIdx.y * GT_Y - GT_MH;
        for (int i = t; i < GT_MR * GT_MW; i += GT_THREADS) {
            const int r = i / GT_MW, c = i - r * GT_MW, y = y0 + r, x = x0 + c;
            const bool in = y >= 0 && y < a.H && x >= 0 && x < a.W;
            sMask[r][c] = in ? a.mask[(size_t)y * a.W + x] : -INFINITY;
        }
    }
    if (want_depth) {
        const int x0 = blockIdx.x * GT_X - GT_DH, y0 = blockIdx.y * GT_Y - GT_DH;
        for (int i = t; i < GT_DR * GT_DW; i += GT_THREADS) {
            const int r = i / GT_DW, c = i - r * GT_DW, y = y0 + r, x = x0 + c;
            const bool in = y >= 0 && y < a.H && x >= 0 && x < a.W;
            sDepth[r][c] = in ? a.depth[(size_t)y * a.W + x] : 0.f;
        }
    }
}

// horizontal 9-tap maximum of the mask tile (NaN wins, as in torch's max_pool2d); the caller takes the vertical one
__device__ __forceinline__ void pool_rows(const float (*sMask)[GT_MW], float (*sPool)[GT_X]) {
    for (int i = threadIdx.x; i < GT_MR * GT_X; i += GT_THREADS) {
        const int r = i / GT_X, c = i - r * GT_X;
        float m = sMask[r][c];
#pragma unroll
        for (int k = 1; k < 9; k++) { const float v = sMask[r][c + k]; m = (v > m || v != v) ? v : m; }
        sPool[r][c] = m;
    }
}
__device__ __forceinline__ float pool_cols(const float (*sPool)[GT_X], int ty, int tx) {
    float m = sPool[ty][tx];
#pragma unroll
    for (int k = 1; k < 9; k++) { const float v = sPool[ty + k][tx]; m = (v > m || v != v) ? v : m; }
    return m;
}

#define GEOM_LOSS_AT                                                                                                             \
    [&](int xx, int yy, float& d, float& m) {                                                                                    \
        d = sDepth[yy - ((int)blockIdx.y * GT_Y - GT_DH)][xx - ((int)blockIdx.x * GT_X - GT_DH)];                                \
        m = sMask[yy - ((int)blockIdx.y * GT_Y - GT_MH)][xx - ((int)blockIdx.x * GT_X - GT_MH)];                                 \
    }

constexpr float ENT_LO = 1e-6f, ENT_HI = (float)(1.0 - 1e-6);   // float32(1e-6), float32(1 - 1e-6)
// torch.clamp: NaN stays NaN (plain compares are false on NaN)
__device__ __forceinline__ float clamp_nan(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ void __launch_bounds__(GT_THREADS) geom_loss_fwd_kernel(const GeomLossArgs a) {
    __shared__ float sMask[GT_MR][GT_MW], sDepth[GT_DR][GT_DW], sPool[GT_MR][GT_X];
    __shared__ double sRed[6][GT_THREADS / 64];
    const int t = threadIdx.x, tx = t % GT_X, ty = t / GT_X;
    const int x = blockIdx.x * GT_X + tx, y = blockIdx.y * GT_Y + ty;
    const bool valid = x < a.W && y < a.H;
    const size_t N = (size_t)a.W * a.H, i = (size_t)y * a.W + x;
    const bool surface = a.terms & TERM_SURFACE, target = a.terms & TERM_TARGET, maskt = a.terms & TERM_MASK, entropy = a.terms & TERM_ENTROPY;
    load_tiles(a, surface || maskt, surface, sMask, sDepth);
    __syncthreads();
    if (maskt) pool_rows(sMask, sPool);
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // surface sum, count, target sum, count, mask sum, entropy sum
    if (valid) {
        float n[3] = {0.f, 0.f, 0.f};
        if (surface || target) { n[0] = a.normal[i]; n[1] = a.normal[N + i]; n[2] = a.normal[2 * N + i]; }
        if (surface) {
            float gt[3];
            d2n_normal(a.cam, x, y, GEOM_LOSS_AT, gt);
            if (cos3(n, gt, 1.f) < 1.f) {
                double gd[3];
                d2n_normal(a.camd, x, y, GEOM_LOSS_AT, gd);
                v[0] = 1.0 - cos3d(n, gd, 1.f); v[1] = 1.0;
            }
        }
        if (target) {
            const float gt[3] = {a.target[i], a.target[N + i], a.target[2 * N + i]};
            const float w = a.weight ? a.weight[i] : 1.f;
            if (cos3(n, gt, w) < 1.f) {
                const double gd[3] = {(double)gt[0], (double)gt[1], (double)gt[2]};
                v[2] = 1.0 - cos3d(n, gd, w); v[3] = 1.0;
            }
        }
        if (entropy) {
            // (the two logarithms in double: logf's last-bit error does not average out over the image, it showed as 7e-8 of the mean)
            const double o = (double)clamp_nan(a.opacity[i], ENT_LO, ENT_HI), m = (double)a.mask[i];
            v[5] = -(m * log(o) + (1.0 - m) * log(1.0 - o));
        }
    }
    if (maskt) {
        __syncthreads();
        if (valid) v[4] = (double)(a.opacity[i] * (1.f - pool_cols(sPool, ty, tx)));
    }
    // workgroup sums in a fixed order: xor butterflies (wave-uniform branches: a term that is off is 0.0 in every lane), then the four waves in order
#pragma unroll
    for (int q = 0; q < 6; q++) {
        const bool on = q < 2 ? surface : (q < 4 ? target : (q == 4 ? maskt : entropy));
        if (on) v[q] = wave_reduce_add(v[q]);
    }
    block_sum_ordered(v, sRed);
    if (t == 0) {
        double* rec = a.partial + 8 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
#pragma unroll
        for (int q = 0; q < 5; q++) rec[q] = v[q];
        rec[5] = 0.0; rec[6] = v[5]; rec[7] = 0.0;
    }
}

// the records of the tiles -> stats [4][2] = {sum, count} and the four losses: one workgroup, fixed order, double
__global__ void __launch_bounds__(256) geom_loss_reduce_kernel(const double* __restrict__ partial, int nblk, int terms, double npix,
                                                               double* __restrict__ stats, float* __restrict__ losses) {
    __shared__ double red[8][4];
    double s[8];
    block_reduce_records(partial, nblk, 8, s, red);
#pragma unroll
    for (int k = 0; k < 4; k++) {   // thread k writes term k (k is a constant per copy of the body: s[] stays in registers)
        if ((int)threadIdx.x != k) continue;
        const bool on = (terms >> k) & 1;
        const double sum = s[2 * k];
        const double cnt = k < 2 ? s[2 * k + 1] : npix;
        stats[2 * k] = on ? sum : 0.0;
        stats[2 * k + 1] = on ? cnt : 0.0;
        losses[k] = on ? (float)(sum / cnt) : 0.f;   // (an empty selection: 0 / 0 = NaN, torch's mean of nothing)
    }
}

__global__ void __launch_bounds__(GT_THREADS) geom_loss_bwd_kernel(const GeomLossArgs a) {
    __shared__ float sMask[GT_MR][GT_MW], sDepth[GT_DR][GT_DW], sPool[GT_MR][GT_X];
    __shared__ float sG[5][GT_RR][GT_RW];   // the ring pixels' d(loss)/d(their five depth reads): centre, up, left, bottom, right
    __shared__ float sN[3][GT_RR][GT_RW];   // d(surface term)/d(rendered normal)
    const int t = threadIdx.x, tx = t % GT_X, ty = t / GT_X;
    const int x = blockIdx.x * GT_X + tx, y = blockIdx.y * GT_Y + ty;
    const bool valid = x < a.W && y < a.H;
    const size_t N = (size_t)a.W * a.H, i = (size_t)y * a.W + x;
    const bool surface = a.terms & TERM_SURFACE, target = a.terms & TERM_TARGET, maskt = a.terms & TERM_MASK, entropy = a.terms & TERM_ENTROPY;
    const bool want_mask = (surface && (a.d_normal || a.d_depth)) || (maskt && a.d_opacity);
    load_tiles(a, want_mask, surface, sMask, sDepth);
    __syncthreads();
    if (maskt && a.d_opacity) pool_rows(sMask, sPool);
    if (surface && (a.d_normal || a.d_depth)) {
        const float cnt = (float)a.stats[1];
        const float gs = cnt > 0.f ? a.g[0] / cnt : 0.f;    // (an empty selection: every gradient of the term is zero)
        const int rx0 = blockIdx.x * GT_X - 1, ry0 = blockIdx.y * GT_Y - 1;
        for (int e = t; e < GT_RR * GT_RW; e += GT_THREADS) {
            const int r = e / GT_RW, c = e - r * GT_RW, px = rx0 + c, py = ry0 + r;
            float gd[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, dn[3] = {0.f, 0.f, 0.f};
            if (px >= 0 && px < a.W && py >= 0 && py < a.H) {
                const size_t pi = (size_t)py * a.W + px;
                const float n[3] = {a.normal[pi], a.normal[N + pi], a.normal[2 * N + pi]};
                float gt[3];
                d2n_normal(a.cam, px, py, GEOM_LOSS_AT, gt);
                if (cos3(n, gt, 1.f) < 1.f) {
#pragma unroll
                    for (int j = 0; j < 3; j++) dn[j] = -gs * gt[j];
                    if (a.d_depth) {
                        const float g[3] = {-gs * n[0], -gs * n[1], -gs * n[2]};
                        d2n_adjoint(a.cam, px, py, GEOM_LOSS_AT, g, gd);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 5; q++) sG[q][r][c] = gd[q];
#pragma unroll
            for (int j = 0; j < 3; j++) sN[j][r][c] = dn[j];
        }
    }
    __syncthreads();
    if (!valid) return;
    if (a.d_depth) {
        float dd = 0.f;
        if (surface) {
            const int r = ty + 1, c = tx + 1;
            dd = sG[0][r][c];
            dd += y > 0 ? sG[3][r - 1][c] : sG[1][r][c];             // the upper neighbour's bottom read, or the own up read folded back
            dd += x > 0 ? sG[4][r][c - 1] : sG[2][r][c];
            dd += y < a.H - 1 ? sG[1][r + 1][c] : sG[3][r][c];
            dd += x < a.W - 1 ? sG[2][r][c + 1] : sG[4][r][c];
        }
        a.d_depth[i] = dd;
    }
    if (a.d_normal) {
        float dn[3] = {0.f, 0.f, 0.f};
        if (surface) { dn[0] = sN[0][ty + 1][tx + 1]; dn[1] = sN[1][ty + 1][tx + 1]; dn[2] = sN[2][ty + 1][tx + 1]; }
        if (target) {
            const float cnt = (float)a.stats[3];
            const float gt_ = cnt > 0.f ? a.g[1] / cnt : 0.f;
            const float n[3] = {a.normal[i], a.normal[N + i], a.normal[2 * N + i]};
            const float tg[3] = {a.target[i], a.target[N + i], a.target[2 * N + i]};
            const float w = a.weight ? a.weight[i] : 1.f;
            if (cos3(n, tg, w) < 1.f) {
#pragma unroll
                for (int j = 0; j < 3; j++) dn[j] = add_rn(dn[j], -gt_ * (tg[j] * w));
            }
        }
#pragma unroll
        for (int j = 0; j < 3; j++) a.d_normal[(size_t)j * N + i] = dn[j];
    }
    if (a.d_opacity) {
        float d_o = 0.f;
        const float inv = 1.f / ((float)a.W * (float)a.H);
        if (maskt) d_o = a.g[2] * inv * (1.f - pool_cols(sPool, ty, tx));
        if (entropy) {
            const float op = a.opacity[i], m = a.mask[i];
            if (op >= ENT_LO && op <= ENT_HI) d_o = add_rn(d_o, a.g[3] * inv * -(m / op - (1.f - m) / (1.f - op)));
        }
        a.d_opacity[i] = d_o;
    }
}

int check_args(const char* what, int32_t W, int32_t H, int32_t terms, const float* normal, const float* depth, const float* mask,
               const float* opacity, const float* target) {
    if (W <= 0 || H <= 0) return report_error(SVGIR_ERR_INVALID, "%s: bad image size W=%d H=%d", what, W, H);
    if (terms == 0) return report_error(SVGIR_ERR_INVALID, "%s: no term requested (bits: 1 surface, 2 target, 4 mask, 8 entropy)", what);
    if (terms < 0 || terms > 15) return report_error(SVGIR_ERR_INVALID, "%s: unknown term bits in terms=%d", what, terms);
    if ((terms & TERM_SURFACE) && (!normal || !depth || !mask))
        return report_error(SVGIR_ERR_INVALID, "%s: the surface term needs the normal, depth and mask planes", what);
    if ((terms & TERM_TARGET) && (!normal || !target))
        return report_error(SVGIR_ERR_INVALID, "%s: the target term needs the normal and target planes", what);
    if ((terms & (TERM_MASK | TERM_ENTROPY)) && (!opacity || !mask))
        return report_error(SVGIR_ERR_INVALID, "%s: the mask and entropy terms need the opacity and mask planes", what);
    return 0;
}

GeomLossArgs make_args(int32_t W, int32_t H, int32_t terms, const float* normal, const float* depth, const float* mask, const float* opacity,
                       const float* target, const float* weight, float fovx, float fovy, float prcp_x, float prcp_y) {
    GeomLossArgs a{};
    a.W = W; a.H = H; a.terms = terms;
    a.cam = D2nCam{W, H, (float)H / (2.f * tanf(fovy * 0.5f)), (float)W / (2.f * tanf(fovx * 0.5f)), prcp_x * (float)W, prcp_y * (float)H};
    a.camd = D2nCamT<double>{W, H, (double)H / (2.0 * tan((double)fovy * 0.5)), (double)W / (2.0 * tan((double)fovx * 0.5)),
                             (double)(prcp_x * (float)W), (double)(prcp_y * (float)H)};   // (the principal point multiplies in fp32, as in depth2normal)
    a.normal = normal; a.depth = depth; a.mask = mask; a.opacity = opacity; a.target = target; a.weight = weight;
    return a;
}

}  // namespace

}  // namespace svgir

using namespace svgir;

extern "C" {

size_t svgir_geometry_loss_partials(int32_t W, int32_t H) {
    if (W <= 0 || H <= 0) return 0;
    return (size_t)((W + GT_X - 1) / GT_X) * ((H + GT_Y - 1) / GT_Y);
}

int svgir_geometry_loss_forward(int32_t W, int32_t H, int32_t terms, const float* normal, const float* depth, const float* mask,
                                const float* opacity, const float* target, const float* weight, float fovx, float fovy, float prcp_x,
                                float prcp_y, double* partial, double* stats, float* losses, void* stream) {
    if (int rc = check_args("geometry_loss_forward", W, H, terms, normal, depth, mask, opacity, target)) return rc;
    if (!partial || !stats || !losses) return report_error(SVGIR_ERR_INVALID, "geometry_loss_forward: partial, stats and losses must be provided");
    GeomLossArgs a = make_args(W, H, terms, normal, depth, mask, opacity, target, weight, fovx, fovy, prcp_x, prcp_y);
    a.partial = partial;
    const dim3 grid((W + GT_X - 1) / GT_X, (H + GT_Y - 1) / GT_Y);
    hipStream_t s = (hipStream_t)stream;
    StageMarks tm = stage_begin(s);
    hipLaunchKernelGGL(geom_loss_fwd_kernel, grid, dim3(GT_THREADS), 0, s, a);
    hipLaunchKernelGGL(geom_loss_reduce_kernel, dim3(1), dim3(256), 0, s, partial, (int)(grid.x * grid.y), terms, (double)W * (double)H, stats,
                       losses);
    stage_mark(tm, "geom_loss_fwd");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SVGIR_OK : report_error(SVGIR_ERR_HIP, "geometry_loss_forward launch failed: %s", hipGetErrorString(e));
}

int svgir_geometry_loss_backward(int32_t W, int32_t H, int32_t terms, const float* normal, const float* depth, const float* mask,
                                 const float* opacity, const float* target, const float* weight, float fovx, float fovy, float prcp_x,
                                 float prcp_y, const double* stats, const float* g_dev, float* dL_dnormal, float* dL_ddepth,
                                 float* dL_dopacity, void* stream) {
    if (int rc = check_args("geometry_loss_backward", W, H, terms, normal, depth, mask, opacity, target)) return rc;
    if (!stats || !g_dev) return report_error(SVGIR_ERR_INVALID, "geometry_loss_backward: stats and the upstream gradients must be provided");
    if (!dL_dnormal && !dL_ddepth && !dL_dopacity) return report_error(SVGIR_ERR_INVALID, "geometry_loss_backward: no gradient requested");
    GeomLossArgs a = make_args(W, H, terms, normal, depth, mask, opacity, target, weight, fovx, fovy, prcp_x, prcp_y);
    a.stats = stats; a.g = g_dev; a.d_normal = dL_dnormal; a.d_depth = dL_ddepth; a.d_opacity = dL_dopacity;
    const dim3 grid((W + GT_X - 1) / GT_X, (H + GT_Y - 1) / GT_Y);
    hipStream_t s = (hipStream_t)stream;
    StageMarks tm = stage_begin(s);
    hipLaunchKernelGGL(geom_loss_bwd_kernel, grid, dim3(GT_THREADS), 0, s, a);
    stage_mark(tm, "geom_loss_bwd");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SVGIR_OK : report_error(SVGIR_ERR_HIP, "geometry_loss_backward launch failed: %s", hipGetErrorString(e));
}

}  // extern "C"
