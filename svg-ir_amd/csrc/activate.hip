// svg-ir_amd/csrc/activate.hip -- the model's activation getters, fused: the step from the optimizer's raw parameters to the tensors the
// shading and the rasterizer consume (`GaussianModel.get_scaling / get_rotation / get_opacity / get_geo_normal / get_shading_normal /
// get_base_color / get_albedo / get_roughness`, scene/gaussian_model.py:104-125, 270-355; `viewdirs`, gaussian_renderer/svgss.py:109; the
// regulariser `mse_loss(_normal, 0)`, svgss.py:316).  ONE forward launch (+ a one-workgroup reduction when normal_reg is asked for) and ONE
// backward launch replace a few dozen elementwise torch launches each way.
//
//   output (fp32)            definition (per surfel p; raw inputs fp32)
//   scales [P,3]             exp(s); NaN -> 1e-6, +inf (fp32 overflow) -> FLT_MAX
//   rotations [P,4]          q / max(|q|, 1e-12); NaN -> 1e-6 (a row whose norm is not finite: finite / inf = 0, inf / inf = NaN -> 1e-6)
//   opacities [P,1]          sigmoid(o)
//   geo_normal [P,3]         (2 (x z + r y), 2 (y z - r x), 1 - 2 (x x + y y)) of the activated (r, x, y, z); not renormalised
//   shading_normal [P,4,3]   corner v, channel c: normalize(geo + normal[p, c * 4 + v]), clamp 1e-12
//   shading_normal12 [P,12]  the same numbers at index c * 4 + v
//   base_color [P,12]        (sigmoid(b_j) * 0.77 + 0.03) * base_color_scale[j / 4]
//   roughness [P,4]          sigmoid(r) * 0.9 + 0.09; NaN -> 1e-8
//   viewdirs [P,3]           normalize(campos - xyz), clamp 1e-12
//   normal_reg               mean(normal^2) over 12 P elements
//
// ARITHMETIC.  The kernels are memory-bound (39 floats in, 54 out per surfel: 372 B; the backward reads 93 and writes 39: 528 B), so every value is evaluated in
// DOUBLE from the fp32 inputs -- exp included -- and rounded to fp32 once: an output carries its final rounding and nothing else, and a
// difference such as 1 - 2 (x x + y y) near zero loses nothing.  sigmoid(x) is evaluated from e = exp(-|x|) as 1 / (1 + e) or e / (1 + e), its
// derivative as e / (1 + e)^2 (no 1 - s cancellation at either end).  Norms are double, so they do not overflow where an fp32 norm would.
// The value of a replaced element is the fp32 constant (1e-6f, 1e-8f, FLT_MAX); geo_normal of a replaced rotation uses 1e-6.
//
// BACKWARD = autograd of the reference's lines, normalize's clamp included (norm < 1e-12: g / 1e-12, finite; else (g - u (g . u)) / norm),
// recomputed from the raw inputs (the forward saves nothing).  ONE DECISION of this project's own: where nan_to_num replaced a value the raw
// element gets ZERO gradient -- scaling elements whose exp is NaN or overflows, roughness elements that are NaN, and the WHOLE rotation row when
// its norm is not finite.  Torch yields NaN there, which the reference scrubs in replace_nangrad_to_zero.  Everything else propagates: a NaN
// opacity / base_color / normal offset / position gives a NaN gradient, and upstream NaNs pass through.  An upstream pointer that is NULL is
// an output outside the graph: it contributes nothing (not 0 * NaN).
//
// LAYOUT.  One lane per surfel, 256 surfels per workgroup.  The 4- and 12-float rows are read and written as float4 (16 B per lane, the
// three float4 of a row back to back); the 3-float rows (xyz, scaling, scales, geo_normal, viewdirs and their gradients) move lane-linearly
// over the flattened array -- lane i of the workgroup touches float base + i, + 256, + 512 -- through an LDS tile that the owning lane reads at
// stride 3 (3 is odd: no bank conflict).  Plain vector stores, no atomics.  normal_reg: per-lane double sum of the 12 squares in index order,
// xor butterfly per wave, the four waves in order -> one double per workgroup; the reduce kernel adds those in a fixed order.
#include <cfloat>
#include <cmath>

#include "common.hpp"

namespace svgir {

int report_error(int code, const char* fmt, ...);   // api.hip (it owns the per-thread message behind svgir_last_error)

namespace {

constexpr int AT = BLOCK;          // surfels per workgroup, one lane each
constexpr int AT3 = 3 * AT;
constexpr double NORM_EPS = 1e-12;   // F.normalize's eps

struct ActArgs {
    svgir_activation a;
    svgir_activation_grads g;   // backward only
    int has_bcs;                // base_color_scale != NULL (NULL = ones)
};

__device__ __forceinline__ void tile_load3(const float* __restrict__ src, size_t base3, int n3, float* s) {
    if (!src) return;
    for (int i = threadIdx.x; i < n3; i += AT) s[i] = src[base3 + i];
}
__device__ __forceinline__ void tile_store3(float* __restrict__ dst, size_t base3, int n3, const float* s) {
    if (!dst) return;
    for (int i = threadIdx.x; i < n3; i += AT) dst[base3 + i] = s[i];
}

// e = exp(-|x|): s = sigmoid(x), ds = s (1 - s); NaN -> NaN, +-inf -> (1 | 0, 0)
__device__ __forceinline__ void sigmoid_d(double x, double& s, double& ds) {
    const double e = exp(-fabs(x)), r = 1.0 / (1.0 + e);
    s = x >= 0.0 ? r : e * r;
    ds = e * r * r;
}

// torch.clamp_min(norm, eps): NaN stays NaN
__device__ __forceinline__ double clamp_norm(double m) { return m < NORM_EPS ? NORM_EPS : m; }

// adjoint of u = w / max(|w|, eps) for a vector of N: g -> dw (u = the forward's result, m = |w|)
template <int N>
__device__ __forceinline__ void normalize_bwd(const double* u, double m, const double* g, double* dw) {
    if (m < NORM_EPS) {
#pragma unroll
        for (int c = 0; c < N; c++) dw[c] = g[c] / NORM_EPS;
    } else {
        double dot = 0.0;
#pragma unroll
        for (int c = 0; c < N; c++) dot += g[c] * u[c];
        const double inv = 1.0 / m;
#pragma unroll
        for (int c = 0; c < N; c++) dw[c] = (g[c] - u[c] * dot) * inv;
    }
}

// the activated quaternion in double (replaced components = 1e-6), its raw norm, and whether nan_to_num's row rule applies
__device__ __forceinline__ void activate_rotation(const float4 q4, double* u, double& n, bool& bad) {
    const double q[4] = {(double)q4.x, (double)q4.y, (double)q4.z, (double)q4.w};
    n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    bad = !(n <= DBL_MAX);   // NaN or inf
    const double den = clamp_norm(n);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        u[k] = q[k] / den;
        if (u[k] != u[k]) u[k] = 1e-6;
    }
}
// (no contraction: x z and r y are rounded alike, so the replaced quaternion (1e-6, 1e-6, 1e-6, 1e-6) gives y z - r x = 0 exactly)
__device__ __forceinline__ void geo_from(const double* u, double* geo) {
#pragma clang fp contract(off)
    const double r = u[0], x = u[1], y = u[2], z = u[3];
    geo[0] = 2.0 * (x * z + r * y);
    geo[1] = 2.0 * (y * z - r * x);
    geo[2] = 1.0 - 2.0 * (x * x + y * y);
}
__device__ __forceinline__ float nan_to_num_f(float v, float nan_value) {
    return v != v ? nan_value : (v == INFINITY ? FLT_MAX : (v == -INFINITY ? -FLT_MAX : v));
}
__device__ __forceinline__ void unpack12(const float4* __restrict__ p, size_t row, float* o) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float4 v = p[3 * row + j];
        o[4 * j] = v.x; o[4 * j + 1] = v.y; o[4 * j + 2] = v.z; o[4 * j + 3] = v.w;
    }
}
__device__ __forceinline__ void pack12(float4* __restrict__ p, size_t row, const float* o) {
#pragma unroll
    for (int j = 0; j < 3; j++) p[3 * row + j] = make_float4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
}

__global__ void __launch_bounds__(AT) activate_fwd_kernel(const ActArgs A) {
    __shared__ float sXyz[AT3], sScl[AT3], sOut[3][AT3];   // in: xyz, scaling; out: scales, geo_normal, viewdirs
    __shared__ double sRed[1][AT / 64];
    const svgir_activation& a = A.a;
    const int t = threadIdx.x;
    const size_t p0 = (size_t)blockIdx.x * AT, p = p0 + t, base3 = 3 * p0;
    const int n = (int)min((size_t)AT, (size_t)a.P - p0), n3 = 3 * n;
    const bool valid = t < n;
    const bool want_geo = a.geo_normal || a.shading_normal || a.shading_normal12;
    if (a.viewdirs) tile_load3(a.xyz, base3, n3, sXyz);
    if (a.scales) tile_load3(a.scaling, base3, n3, sScl);
    __syncthreads();
    double reg = 0.0;
    if (valid) {
        if (a.scales) {
#pragma unroll
            for (int k = 0; k < 3; k++) sOut[0][3 * t + k] = nan_to_num_f((float)exp((double)sScl[3 * t + k]), 1e-6f);
        }
        if (a.viewdirs) {
            double w[3], m2 = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) { w[k] = (double)a.campos[k] - (double)sXyz[3 * t + k]; m2 += w[k] * w[k]; }
            const double den = clamp_norm(sqrt(m2));
#pragma unroll
            for (int k = 0; k < 3; k++) sOut[2][3 * t + k] = (float)(w[k] / den);
        }
        if (a.opacities) { double s, ds; sigmoid_d((double)a.opacity[p], s, ds); a.opacities[p] = (float)s; }
        double geo[3] = {0.0, 0.0, 0.0};
        if (a.rotations || want_geo) {
            double u[4], nrm; bool bad;
            activate_rotation(((const float4*)a.rotation)[p], u, nrm, bad);
            // (|u| <= 1, so no infinity can arise; a replaced component rounds to the fp32 constant 1e-6f)
            if (a.rotations) ((float4*)a.rotations)[p] = make_float4((float)u[0], (float)u[1], (float)u[2], (float)u[3]);
            geo_from(u, geo);
            if (a.geo_normal) {
#pragma unroll
                for (int k = 0; k < 3; k++) sOut[1][3 * t + k] = (float)geo[k];
            }
        }
        if (a.shading_normal || a.shading_normal12 || a.normal_reg) {
            float o[12];
            unpack12((const float4*)a.normal, p, o);
            if (a.normal_reg) {
#pragma unroll
                for (int j = 0; j < 12; j++) reg += (double)o[j] * (double)o[j];
            }
            if (a.shading_normal || a.shading_normal12) {
                float sn[12], sn12[12];
#pragma unroll
                for (int v = 0; v < 4; v++) {
                    double w[3], m2 = 0.0;
#pragma unroll
                    for (int c = 0; c < 3; c++) { w[c] = geo[c] + (double)o[c * 4 + v]; m2 += w[c] * w[c]; }
                    const double den = clamp_norm(sqrt(m2));
#pragma unroll
                    for (int c = 0; c < 3; c++) sn[v * 3 + c] = sn12[c * 4 + v] = (float)(w[c] / den);
                }
                if (a.shading_normal) pack12((float4*)a.shading_normal, p, sn);
                if (a.shading_normal12) pack12((float4*)a.shading_normal12, p, sn12);
            }
        }
        if (a.out_base_color) {
            float b[12];
            unpack12((const float4*)a.base_color, p, b);
#pragma unroll
            for (int j = 0; j < 12; j++) {
                double s, ds;
                sigmoid_d((double)b[j], s, ds);
                const double v = s * 0.77 + 0.03;
                b[j] = (float)(A.has_bcs ? v * (double)a.base_color_scale[j >> 2] : v);
            }
            pack12((float4*)a.out_base_color, p, b);
        }
        if (a.out_roughness) {
            const float4 r4 = ((const float4*)a.roughness)[p];
            float r[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                double s, ds;
                sigmoid_d((double)r[j], s, ds);
                r[j] = nan_to_num_f((float)(s * 0.9 + 0.09), 1e-8f);
            }
            ((float4*)a.out_roughness)[p] = make_float4(r[0], r[1], r[2], r[3]);
        }
    }
    __syncthreads();
    tile_store3(a.scales, base3, n3, sOut[0]);
    tile_store3(a.geo_normal, base3, n3, sOut[1]);
    tile_store3(a.viewdirs, base3, n3, sOut[2]);
    if (a.normal_reg) {   // (workgroup-uniform)
        double s[1] = {wave_reduce_add(reg)};
        block_sum_ordered(s, sRed);
        if (t == 0) a.partial[blockIdx.x] = s[0];
    }
}

// the workgroups' partial sums -> the double sum and the fp32 mean: one workgroup, fixed order
__global__ void __launch_bounds__(256) activate_reduce_kernel(const double* __restrict__ partial, int nblk, double count,
                                                              double* __restrict__ sum, float* __restrict__ mean) {
    __shared__ double red[1][4];
    double tot[1];
    block_reduce_records(partial, nblk, 1, tot, red);
    if (threadIdx.x == 0) {
        *sum = tot[0];
        *mean = (float)(tot[0] / count);
    }
}

__global__ void __launch_bounds__(AT) activate_bwd_kernel(const ActArgs A) {
    // in: xyz, scaling, dL_dscales, dL_dgeo_normal, dL_dviewdirs; out (over sIn[0], sIn[1] after the barrier): dL_dxyz, dL_dscaling
    __shared__ float sIn[5][AT3];
    const svgir_activation& a = A.a;
    const svgir_activation_grads& g = A.g;
    const int t = threadIdx.x;
    const size_t p0 = (size_t)blockIdx.x * AT, p = p0 + t, base3 = 3 * p0;
    const int n = (int)min((size_t)AT, (size_t)a.P - p0), n3 = 3 * n;
    const bool valid = t < n;
    const bool up_sn = g.dL_dshading_normal || g.dL_dshading_normal12;
    const bool do_sn = up_sn && (g.dL_drotation || g.dL_dnormal);
    const bool do_rot = g.dL_drotation && (g.dL_drotations || g.dL_dgeo_normal || up_sn);
    if (g.dL_dxyz && g.dL_dviewdirs) { tile_load3(a.xyz, base3, n3, sIn[0]); tile_load3(g.dL_dviewdirs, base3, n3, sIn[4]); }
    if (g.dL_dscaling && g.dL_dscales) { tile_load3(a.scaling, base3, n3, sIn[1]); tile_load3(g.dL_dscales, base3, n3, sIn[2]); }
    if (do_rot && g.dL_dgeo_normal) tile_load3(g.dL_dgeo_normal, base3, n3, sIn[3]);
    __syncthreads();
    float dxyz[3] = {0.f, 0.f, 0.f}, dscl[3] = {0.f, 0.f, 0.f};
    if (valid) {
        if (g.dL_dxyz && g.dL_dviewdirs) {
            double w[3], m2 = 0.0, u[3], gv[3], dw[3];
#pragma unroll
            for (int k = 0; k < 3; k++) { w[k] = (double)a.campos[k] - (double)sIn[0][3 * t + k]; m2 += w[k] * w[k]; gv[k] = (double)sIn[4][3 * t + k]; }
            const double m = sqrt(m2), den = clamp_norm(m);
#pragma unroll
            for (int k = 0; k < 3; k++) u[k] = w[k] / den;
            normalize_bwd<3>(u, m, gv, dw);
#pragma unroll
            for (int k = 0; k < 3; k++) dxyz[k] = (float)-dw[k];
        }
        if (g.dL_dscaling && g.dL_dscales) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double e = exp((double)sIn[1][3 * t + k]);
                const float ef = (float)e;
                const bool replaced = ef != ef || ef == INFINITY;
                dscl[k] = replaced ? 0.f : (float)((double)sIn[2][3 * t + k] * e);
            }
        }
        if (g.dL_dopacity) {
            float d = 0.f;
            if (g.dL_dopacities) { double s, ds; sigmoid_d((double)a.opacity[p], s, ds); d = (float)((double)g.dL_dopacities[p] * ds); }
            g.dL_dopacity[p] = d;
        }
        // ---- rotation and normal offsets: the shading normals feed both, through geo_normal and directly
        double ggeo[3] = {0.0, 0.0, 0.0}, dn[12];
#pragma unroll
        for (int j = 0; j < 12; j++) dn[j] = 0.0;
        double u[4] = {0.0, 0.0, 0.0, 0.0}, nrm = 0.0;
        bool bad = false;
        float o[12];
        if (do_rot || do_sn) activate_rotation(((const float4*)a.rotation)[p], u, nrm, bad);
        if (do_sn || (g.dL_dnormal && g.dL_dnormal_reg)) unpack12((const float4*)a.normal, p, o);
        if (do_sn) {
            double geo[3];
            geo_from(u, geo);
            float g1[12], g2[12];
            if (g.dL_dshading_normal) unpack12((const float4*)g.dL_dshading_normal, p, g1);
            if (g.dL_dshading_normal12) unpack12((const float4*)g.dL_dshading_normal12, p, g2);
#pragma unroll
            for (int v = 0; v < 4; v++) {
                double w[3], m2 = 0.0, sn[3], gs[3], dw[3];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    w[c] = geo[c] + (double)o[c * 4 + v];
                    m2 += w[c] * w[c];
                    gs[c] = (g.dL_dshading_normal ? (double)g1[v * 3 + c] : 0.0) + (g.dL_dshading_normal12 ? (double)g2[c * 4 + v] : 0.0);
                }
                const double m = sqrt(m2), den = clamp_norm(m);
#pragma unroll
                for (int c = 0; c < 3; c++) sn[c] = w[c] / den;
                normalize_bwd<3>(sn, m, gs, dw);
#pragma unroll
                for (int c = 0; c < 3; c++) { dn[c * 4 + v] = dw[c]; ggeo[c] += dw[c]; }
            }
        }
        if (g.dL_drotation) {
            float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
            if (do_rot && !bad) {
                if (g.dL_dgeo_normal) {
#pragma unroll
                    for (int k = 0; k < 3; k++) ggeo[k] += (double)sIn[3][3 * t + k];
                }
                const double r = u[0], x = u[1], y = u[2], z = u[3];
                double G[4] = {2.0 * (y * ggeo[0] - x * ggeo[1]), 2.0 * (z * ggeo[0] - r * ggeo[1]) - 4.0 * x * ggeo[2],
                               2.0 * (r * ggeo[0] + z * ggeo[1]) - 4.0 * y * ggeo[2], 2.0 * (x * ggeo[0] + y * ggeo[1])};
                if (g.dL_drotations) {
                    const float4 gr = ((const float4*)g.dL_drotations)[p];
                    G[0] += (double)gr.x; G[1] += (double)gr.y; G[2] += (double)gr.z; G[3] += (double)gr.w;
                }
                double dq[4];
                normalize_bwd<4>(u, nrm, G, dq);
                out = make_float4((float)dq[0], (float)dq[1], (float)dq[2], (float)dq[3]);
            }
            ((float4*)g.dL_drotation)[p] = out;
        }
        if (g.dL_dnormal) {
            float d[12];
            const double k2 = g.dL_dnormal_reg ? (double)g.dL_dnormal_reg[0] * 2.0 / (12.0 * (double)a.P) : 0.0;
#pragma unroll
            for (int j = 0; j < 12; j++) d[j] = (float)(g.dL_dnormal_reg ? dn[j] + k2 * (double)o[j] : dn[j]);
            pack12((float4*)g.dL_dnormal, p, d);
        }
        if (g.dL_dbase_color) {
            float d[12];
            if (g.dL_dout_base_color) {
                float b[12];
                unpack12((const float4*)a.base_color, p, b);
                unpack12((const float4*)g.dL_dout_base_color, p, d);
#pragma unroll
                for (int j = 0; j < 12; j++) {
                    double s, ds;
                    sigmoid_d((double)b[j], s, ds);
                    const double v = (double)d[j] * (0.77 * ds);
                    d[j] = (float)(A.has_bcs ? v * (double)a.base_color_scale[j >> 2] : v);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 12; j++) d[j] = 0.f;
            }
            pack12((float4*)g.dL_dbase_color, p, d);
        }
        if (g.dL_droughness) {
            float d[4] = {0.f, 0.f, 0.f, 0.f};
            if (g.dL_dout_roughness) {
                const float4 r4 = ((const float4*)a.roughness)[p], g4 = ((const float4*)g.dL_dout_roughness)[p];
                const float r[4] = {r4.x, r4.y, r4.z, r4.w}, gr[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    double s, ds;
                    sigmoid_d((double)r[j], s, ds);
                    d[j] = r[j] != r[j] ? 0.f : (float)((double)gr[j] * (0.9 * ds));   // (a NaN raw value was replaced by 1e-8)
                }
            }
            ((float4*)g.dL_droughness)[p] = make_float4(d[0], d[1], d[2], d[3]);
        }
    }
    __syncthreads();
    if (valid) {
#pragma unroll
        for (int k = 0; k < 3; k++) { sIn[0][3 * t + k] = dxyz[k]; sIn[1][3 * t + k] = dscl[k]; }
    }
    __syncthreads();
    tile_store3(g.dL_dxyz, base3, n3, sIn[0]);
    tile_store3(g.dL_dscaling, base3, n3, sIn[1]);
}

bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace

}  // namespace svgir

using namespace svgir;

extern "C" {

size_t svgir_activate_partials(int32_t P) { return P <= 0 ? 0 : ((size_t)P + AT - 1) / AT; }

int svgir_activate_forward(const svgir_activation* a, void* stream) {
    if (!a) return report_error(SVGIR_ERR_INVALID, "activate_forward: the parameter block must be provided");
    if (a->P < 0) return report_error(SVGIR_ERR_INVALID, "activate_forward: bad P=%d", a->P);
    const bool want_sn = a->shading_normal || a->shading_normal12, want_geo = a->geo_normal || want_sn;
    if (a->scales && !a->scaling) return report_error(SVGIR_ERR_INVALID, "activate_forward: scales needs the raw scaling");
    if ((a->rotations || want_geo) && !a->rotation)
        return report_error(SVGIR_ERR_INVALID, "activate_forward: rotations, geo_normal and the shading normals need the raw rotation");
    if (a->opacities && !a->opacity) return report_error(SVGIR_ERR_INVALID, "activate_forward: opacities needs the raw opacity");
    if ((want_sn || a->normal_reg) && !a->normal)
        return report_error(SVGIR_ERR_INVALID, "activate_forward: the shading normals and normal_reg need the raw normal offsets");
    if (a->out_base_color && !a->base_color) return report_error(SVGIR_ERR_INVALID, "activate_forward: base_color needs the raw base_color");
    if (a->out_roughness && !a->roughness) return report_error(SVGIR_ERR_INVALID, "activate_forward: roughness needs the raw roughness");
    if (a->viewdirs && (!a->xyz || !a->campos)) return report_error(SVGIR_ERR_INVALID, "activate_forward: viewdirs needs xyz and campos");
    if (a->normal_reg && (!a->partial || !a->normal_reg_sum))
        return report_error(SVGIR_ERR_INVALID, "activate_forward: normal_reg needs partial and normal_reg_sum");
    if (misaligned(a->rotation) || misaligned(a->normal) || misaligned(a->base_color) || misaligned(a->roughness) || misaligned(a->rotations) ||
        misaligned(a->shading_normal) || misaligned(a->shading_normal12) || misaligned(a->out_base_color) || misaligned(a->out_roughness))
        return report_error(SVGIR_ERR_INVALID, "activate_forward: the 4- and 12-float rows must be 16-byte aligned (they move as float4)");
    if (a->P == 0) return SVGIR_OK;
    if (!a->scales && !a->rotations && !a->opacities && !want_geo && !a->out_base_color && !a->out_roughness && !a->viewdirs && !a->normal_reg)
        return report_error(SVGIR_ERR_INVALID, "activate_forward: no output requested");
    ActArgs A{};
    A.a = *a;
    A.has_bcs = a->base_color_scale != nullptr;
    const unsigned blocks = (unsigned)svgir_activate_partials(a->P);
    hipStream_t s = (hipStream_t)stream;
    StageMarks tm = stage_begin(s);
    hipLaunchKernelGGL(activate_fwd_kernel, dim3(blocks), dim3(AT), 0, s, A);
    if (a->normal_reg)
        hipLaunchKernelGGL(activate_reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)a->partial, (int)blocks, 12.0 * (double)a->P,
                           a->normal_reg_sum, a->normal_reg);
    stage_mark(tm, "activate_fwd");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SVGIR_OK : report_error(SVGIR_ERR_HIP, "activate_forward launch failed: %s", hipGetErrorString(e));
}

int svgir_activate_backward(const svgir_activation* a, const svgir_activation_grads* g, void* stream) {
    if (!a || !g) return report_error(SVGIR_ERR_INVALID, "activate_backward: both parameter blocks must be provided");
    if (a->P < 0) return report_error(SVGIR_ERR_INVALID, "activate_backward: bad P=%d", a->P);
    const bool up_sn = g->dL_dshading_normal || g->dL_dshading_normal12;
    if (!g->dL_dxyz && !g->dL_dscaling && !g->dL_drotation && !g->dL_dopacity && !g->dL_dnormal && !g->dL_dbase_color && !g->dL_droughness)
        return report_error(SVGIR_ERR_INVALID, "activate_backward: no gradient requested");
    if (g->dL_dxyz && (!a->xyz || !a->campos)) return report_error(SVGIR_ERR_INVALID, "activate_backward: dL_dxyz needs xyz and campos");
    if (g->dL_dscaling && !a->scaling) return report_error(SVGIR_ERR_INVALID, "activate_backward: dL_dscaling needs the raw scaling");
    if (g->dL_drotation && !a->rotation) return report_error(SVGIR_ERR_INVALID, "activate_backward: dL_drotation needs the raw rotation");
    if (g->dL_dopacity && !a->opacity) return report_error(SVGIR_ERR_INVALID, "activate_backward: dL_dopacity needs the raw opacity");
    if (g->dL_dnormal && !a->normal) return report_error(SVGIR_ERR_INVALID, "activate_backward: dL_dnormal needs the raw normal offsets");
    if (up_sn && (g->dL_drotation || g->dL_dnormal) && (!a->rotation || !a->normal))
        return report_error(SVGIR_ERR_INVALID, "activate_backward: the shading normals' gradient needs the raw rotation and normal offsets");
    if (g->dL_dbase_color && !a->base_color) return report_error(SVGIR_ERR_INVALID, "activate_backward: dL_dbase_color needs the raw base_color");
    if (g->dL_droughness && !a->roughness) return report_error(SVGIR_ERR_INVALID, "activate_backward: dL_droughness needs the raw roughness");
    if (misaligned(a->rotation) || misaligned(a->normal) || misaligned(a->base_color) || misaligned(a->roughness) || misaligned(g->dL_drotations) ||
        misaligned(g->dL_dshading_normal) || misaligned(g->dL_dshading_normal12) || misaligned(g->dL_dout_base_color) ||
        misaligned(g->dL_dout_roughness) || misaligned(g->dL_drotation) || misaligned(g->dL_dnormal) || misaligned(g->dL_dbase_color) ||
        misaligned(g->dL_droughness))
        return report_error(SVGIR_ERR_INVALID, "activate_backward: the 4- and 12-float rows must be 16-byte aligned (they move as float4)");
    if (a->P == 0) return SVGIR_OK;
    ActArgs A{};
    A.a = *a;
    A.g = *g;
    A.has_bcs = a->base_color_scale != nullptr;
    const unsigned blocks = (unsigned)svgir_activate_partials(a->P);
    hipStream_t s = (hipStream_t)stream;
    StageMarks tm = stage_begin(s);
    hipLaunchKernelGGL(activate_bwd_kernel, dim3(blocks), dim3(AT), 0, s, A);
    stage_mark(tm, "activate_bwd");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SVGIR_OK : report_error(SVGIR_ERR_HIP, "activate_backward launch failed: %s", hipGetErrorString(e));
}

}  // extern "C"
