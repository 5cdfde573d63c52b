// svg-ir_amd/csrc/irradiance.hip -- the pbgi irradiance kernels (the get_radiance_loss / calculate_radiance row).
//
// Replaces `Renderer.render_irradiance_sample` (pbgi/renderer.py:181-226, 748-751; pbgi/bvhworkers/intersect_test.slang:1140-1360, forward
// and backward: the radiance-consistency loss of GaussianModel.get_radiance_loss) and `Renderer.render_irradiance` (intersect_test.slang:
// 901-1138: GaussianModel.calculate_radiance).  The kernels trace nothing: per entry (a row i with its chosen sample p, or every (i, p)) they
// follow the cached first hit h = hit_indices[i,p] and sum, over the S secondary samples of h that escaped (hit_indices[h,s] == -1), the
// corner-blended GGX brdf of `shading_brdf_simple` (pbgi/bvhworkers/pbr.slang:283-329) times envmap[h,s] / S.  The contract, with the three
// decisions the reference leaves open (a missed primary is zero, the sum is a sum, nothing reads out of bounds) and the fourth that is
// this project's own (n0 without the cancellation of the reference's form), is in
// include/svgir_raster.h.
//
// One wave per entry, lane = secondary sample, S > 64 in passes of 64, S < 64 a masked tail.  The row of the hit surfel is contiguous
// (ray_d[h], hit_indices[h], uvs[h], envmap[h]), so every gather is a coalesced row read; the view direction, the 12 normals, 12 albedos
// and the roughnesses of h are wave-uniform.  Every lane keeps its partial sums over the passes in a fixed order and the wave adds them
// with the DPP scan of common.hpp (wave_sum): the forward has no atomics and gives the same bits for the same input.
//
// The backward of the sample form keeps the wave-per-row shape: d_albedos / d_roughnesses are summed over the wave first (13 atomics per
// row), d_envmap[h] is added as contiguous 256-byte wave-instructions (the lanes' {s, c} values are transposed to element order with
// shuffles first).  Several rows may share one h, hence the atomics; the call clears the three gradient arrays itself.
//
// A term is evaluated without contraction to fused multiply-adds, with correctly rounded divides and square roots, in the order the
// header gives: the numpy fp32 restatement of tests/radiance_cases.py then differs from a term only by exp2's rounding.
//
// The second half of the file is the whole radiance-consistency loss around that sum as one forward and one backward kernel
// (svgir_radiance_loss_forward / _backward; GaussianModel.get_radiance_loss, scene/gaussian_model.py:544-575): the selection of the
// sample, the light of the hit surfel's escaped samples looked up in the kernel (env_lookup.hpp, the f(env) table of the shading
// kernels) and the L1 against the cached radiance.  No [N,S,3] light tensor and no [N,S,3] gradient exist on that path.  See the comment
// in front of radiance_loss_fwd_kernel.  Both kernels are instantiated for the lat-long texture and for the spherical-Gaussian light
// (sg_light.hpp; svgir_radiance_loss_forward_sg / _backward_sg): the light of a sample and the scatter of its adjoint are the only
// light-specific parts, on the device and behind the four entry points (rl_forward<LIGHT> / rl_backward<LIGHT>).
//
// Shared: irr_load_corners / irr_light / irr_spec (corners, a sample's light direction, a corner's specular term), irr_row_corners (the row
// prologue of irradiance_kernel, irradiance_sample_bwd_kernel and radiance_loss_fwd_kernel) and wave.hpp's block_tree_sum (the fixed tree
// of radiance_loss_final_kernel, 1024 doubles, and of the two d_ratio sums, BLOCK doubles).  Kept as copies ON PURPOSE, because one helper
// changed the generated code of the kernel named (profiles/irradiance_refactor_isa.txt has the numbers):
//   * the per-sample forward body (irradiance_kernel<FULL>, radiance_loss_fwd_kernel<LIGHT>): other address arithmetic in
//     irradiance_kernel, svgir_pbgi_irradiance + 2.4 %, the fused texture forward + 1.2 %;
//   * the per-sample backward body (irradiance_sample_bwd_kernel and both light branches of radiance_loss_bwd_kernel<LIGHT>), the row
//     epilogue and the wave-ordered workgroup sum: radiance_loss_bwd_kernel<LIGHT> got 3 - 5 more SGPR spill lanes and another
//     instruction stream behind every one of them, the row prologue included, so that kernel keeps all of its text.
// A change of the per-sample body or of the skip rule (a channel without upstream is SKIPPED in the loss, multiplied in the sample form)
// is made at each of these sites.
#include <cmath>

#include "common.hpp"
#include "env_lookup.hpp"
#include "sg_light.hpp"

namespace svgir {

namespace {

constexpr int IRR_WAVE = 64;
constexpr int IRR_WAVES = BLOCK / IRR_WAVE;   // entries per workgroup
constexpr float IRR_PI = 3.14159265358979323846f;
constexpr float IRR_4PI = 12.566370614359172f;
constexpr float IRR_1_PI = 0.3183098861837907f;

// what is wave-uniform for one entry: the normalised view direction and the four corners of the hit surfel
struct IrrCorners {
    float v[3];
    float n[4][3];     // normalised
    float nraw[4][3];  // as stored (the full form's cosine uses it)
    float nov[4], r[4], a2[4], k[4], n1[4];
    float alb[3][4];   // [channel][corner]
};

// the terms of the contract are evaluated as written: no contraction anywhere in this file
#pragma clang fp contract(off)

__device__ __forceinline__ float irr_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ float irr_clamp(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
__device__ __forceinline__ void irr_normalize(const float* a, float* o) {
    const float len = sqrtf(irr_dot(a, a));
    o[0] = a[0] / len; o[1] = a[1] / len; o[2] = a[2] / len;
}

template <bool FULL>
__device__ __forceinline__ void irr_load_corners(IrrCorners& c, const float* vdir, size_t h, const float* __restrict__ normals,
                                                 const float* __restrict__ albedos, const float* __restrict__ roughnesses) {
    const float mv[3] = {-vdir[0], -vdir[1], -vdir[2]};
    irr_normalize(mv, c.v);
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            c.nraw[k][ch] = normals[h * 12 + ch * 4 + k];
            c.alb[ch][k] = albedos[h * 12 + ch * 4 + k];
        }
        irr_normalize(c.nraw[k], c.n[k]);
        c.nov[k] = irr_clamp(irr_dot(c.n[k], c.v), 1e-6f, 1.0f);
        const float r = roughnesses[h * 4 + (FULL ? k : 0)];   // (the sample form: corner 0's roughness for all four, as in the reference)
        const float a = r * r;
        c.r[k] = r;
        c.a2[k] = a * a;
        c.k[k] = ((a + 2.0f * r) + 1.0f) / 8.0f;
        c.n1[k] = c.nov[k] * (1.0f - c.k[k]) + c.k[k];
    }
}
// the row prologue (every kernel but radiance_loss_bwd_kernel, which keeps its own text): the view direction is ray p of row i, the
// corners are those of its hit h
template <bool FULL>
__device__ __forceinline__ void irr_row_corners(IrrCorners& c, const float* ray_d, size_t i, int S, int p, size_t h, const float* normals,
                                                const float* albedos, const float* roughnesses) {
    const float* vd = ray_d + (i * (size_t)S + p) * 3;
    const float vdir[3] = {vd[0], vd[1], vd[2]};
    irr_load_corners<FULL>(c, vdir, h, normals, albedos, roughnesses);
}

// per lane: the light direction of one secondary sample
struct IrrLight {
    float l[3], hv[3], fres;
    float w[4];
};
__device__ __forceinline__ void irr_light(IrrLight& q, const IrrCorners& c, const float* ldir, float u, float v) {
    irr_normalize(ldir, q.l);
    const float s[3] = {c.v[0] + q.l[0], c.v[1] + q.l[1], c.v[2] + q.l[2]};
    irr_normalize(s, q.hv);
    const float voh = irr_clamp(irr_dot(c.v, q.hv), 1e-6f, 1.0f);
    q.fres = 0.04f + 0.96f * exp2f((-5.55473f * voh - 6.98316f) * voh);
    q.w[0] = (1.0f - u) * (1.0f - v);
    q.w[1] = u * (1.0f - v);
    q.w[2] = (1.0f - u) * v;
    q.w[3] = u * v;
}

// specular term of corner k; with GRAD also d spec / d roughness (the clamp passes the denominator's derivative inside [1e-6, 4 pi])
template <bool GRAD>
__device__ __forceinline__ float irr_spec(const IrrCorners& c, const IrrLight& q, int k, float* dspec) {
    const float nol = irr_clamp(irr_dot(c.n[k], q.l), 1e-6f, 1.0f);
    // n0 = NoH^2 (a2 - 1) + 1 = (1 - NoH^2) + NoH^2 a2 cancels as NoH -> 1 at small roughness; 1 - NoH^2 is taken as |H - (n.H) n|^2,
    // which is the same number for unit vectors and keeps its relative accuracy (csrc/shade.hip does the same)
    const float nohr = irr_dot(c.n[k], q.hv);
    const float noh = irr_clamp(nohr, 1e-6f, 1.0f);
    const float pr[3] = {q.hv[0] - nohr * c.n[k][0], q.hv[1] - nohr * c.n[k][1], q.hv[2] - nohr * c.n[k][2]};
    const float s2 = fminf(irr_dot(pr, pr), 1.0f);
    const float n0 = nohr >= 1e-6f ? s2 * (1.0f - c.a2[k]) + c.a2[k] : (noh * noh) * (c.a2[k] - 1.0f) + 1.0f;
    const float n2 = nol * (1.0f - c.k[k]) + c.k[k];
    const float raw = (((IRR_4PI * n0) * n0) * c.n1[k]) * n2;
    const float den = irr_clamp(raw, 1e-6f, IRR_4PI);
    const float frac = q.fres * c.a2[k];
    if (GRAD) {
        const float r = c.r[k];
        const float da2 = 4.0f * ((r * r) * r);
        const float dk = (r + 1.0f) / 4.0f;
        float dden = 0.0f;
        if (raw >= 1e-6f && raw <= IRR_4PI) {
            const float dn0 = (noh * noh) * da2, dn1 = (1.0f - c.nov[k]) * dk, dn2 = (1.0f - nol) * dk;
            dden = IRR_4PI * ((((2.0f * n0) * dn0) * c.n1[k]) * n2 + (n0 * n0) * (dn1 * n2 + c.n1[k] * dn2));
        }
        *dspec = (q.fres * da2) / den - (frac * dden) / (den * den);
    }
    return frac / den;
}

// entry e -> (row i, sample p, hit h); h < 0: the entry is a miss (or an index is out of range) and its result is zero
template <bool FULL>
__device__ __forceinline__ int irr_entry(size_t e, int N, int S, const int32_t* __restrict__ sample_indices, const int32_t* __restrict__ hit,
                                         size_t& i, int& p) {
    if (FULL) { i = e / (size_t)S; p = (int)(e - i * (size_t)S); }
    else { i = e; p = sample_indices[e]; }
    if (p < 0 || p >= S) return -1;
    const int h = hit[i * (size_t)S + p];
    return (h < 0 || h >= N) ? -1 : h;
}

// ---- forward: FULL = false: out [N,3] (the sample form); FULL = true: out [N,S,3] ---------------------------------------------------
template <bool FULL>
__global__ void __launch_bounds__(BLOCK) irradiance_kernel(int N, int S, size_t entries, const int32_t* __restrict__ sample_indices,
                                                           const float* __restrict__ ray_d, const float* __restrict__ envmap,
                                                           const float* __restrict__ normals, const float* __restrict__ albedos,
                                                           const float* __restrict__ roughnesses, const int32_t* __restrict__ hit,
                                                           const float* __restrict__ uvs, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const size_t e = (size_t)blockIdx.x * IRR_WAVES + (threadIdx.x >> 6);
    if (e >= entries) return;   // (whole waves leave)
    size_t i;
    int p;
    const int hh = __builtin_amdgcn_readfirstlane(irr_entry<FULL>(e, N, S, sample_indices, hit, i, p));
    float acc[3] = {0.f, 0.f, 0.f};
    if (hh >= 0) {
        const size_t h = (size_t)hh;
        IrrCorners c;
        irr_row_corners<FULL>(c, ray_d, i, S, p, h, normals, albedos, roughnesses);
        const float fs = (float)S;
        for (int s = lane; s < S; s += IRR_WAVE) {
            const size_t hs = h * (size_t)S + s;
            if (hit[hs] != -1) continue;   // occluded secondary
            const float ld[3] = {ray_d[hs * 3], ray_d[hs * 3 + 1], ray_d[hs * 3 + 2]};
            IrrLight q;
            irr_light(q, c, ld, uvs[hs * 2], uvs[hs * 2 + 1]);
            // (the per-sample forward body stands here and in radiance_loss_fwd_kernel: routed through one helper both measured slower)
            float b[4], cosn[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                b[k] = irr_spec<false>(c, q, k, nullptr);
                if (FULL) cosn[k] = irr_clamp(irr_dot(c.nraw[k], q.l), 1e-6f, 1.0f);
            }
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                float t[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    t[k] = b[k] + c.alb[ch][k] * IRR_1_PI;
                    if (FULL) t[k] = t[k] * cosn[k];
                }
                const float irr = ((q.w[0] * t[0] + q.w[1] * t[1]) + q.w[2] * t[2]) + q.w[3] * t[3];
                acc[ch] += (irr * envmap[hs * 3 + ch]) / fs;
            }
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ch++) acc[ch] = wave_sum(acc[ch]);
    if (lane < 3) out[e * 3 + lane] = lane == 0 ? acc[0] : lane == 1 ? acc[1] : acc[2];
}

// ---- backward of the sample form ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) irradiance_sample_bwd_kernel(int N, int S, const int32_t* __restrict__ sample_indices,
                                                                      const float* __restrict__ ray_d, const float* __restrict__ envmap,
                                                                      const float* __restrict__ normals, const float* __restrict__ albedos,
                                                                      const float* __restrict__ roughnesses, const int32_t* __restrict__ hit,
                                                                      const float* __restrict__ uvs, const float* __restrict__ d_out,
                                                                      float* __restrict__ d_envmap, float* __restrict__ d_albedos,
                                                                      float* __restrict__ d_roughnesses) {
    const int lane = threadIdx.x & 63;
    const size_t e = (size_t)blockIdx.x * IRR_WAVES + (threadIdx.x >> 6);
    if (e >= (size_t)N) return;
    size_t i;
    int p;
    const int hh = __builtin_amdgcn_readfirstlane(irr_entry<false>(e, N, S, sample_indices, hit, i, p));
    if (hh < 0) return;   // (wave-uniform)
    const size_t h = (size_t)hh;
    const float g[3] = {d_out[i * 3], d_out[i * 3 + 1], d_out[i * 3 + 2]};
    IrrCorners c;
    irr_row_corners<false>(c, ray_d, i, S, p, h, normals, albedos, roughnesses);
    const float fs = (float)S;
    float dalb[3][4] = {}, drough = 0.f;
    // passes of 64 samples; every lane takes part in the shuffles of a pass, also behind the tail
    for (int s0 = 0; s0 < S; s0 += IRR_WAVE) {
        const int s = s0 + lane;
        float denv[3] = {0.f, 0.f, 0.f};
        if (s < S) {
            const size_t hs = h * (size_t)S + s;
            if (hit[hs] == -1) {
                const float ld[3] = {ray_d[hs * 3], ray_d[hs * 3 + 1], ray_d[hs * 3 + 2]};
                IrrLight q;
                irr_light(q, c, ld, uvs[hs * 2], uvs[hs * 2 + 1]);
                const float env[3] = {envmap[hs * 3], envmap[hs * 3 + 1], envmap[hs * 3 + 2]};
                float b[4], ds[4];
#pragma unroll
                for (int k = 0; k < 4; k++) b[k] = irr_spec<true>(c, q, k, &ds[k]);
                const float dq = ((q.w[0] * ds[0] + q.w[1] * ds[1]) + q.w[2] * ds[2]) + q.w[3] * ds[3];
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    float t[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        t[k] = b[k] + c.alb[ch][k] * IRR_1_PI;
                        dalb[ch][k] += (((g[ch] * q.w[k]) * env[ch]) * IRR_1_PI) / fs;
                    }
                    const float irr = ((q.w[0] * t[0] + q.w[1] * t[1]) + q.w[2] * t[2]) + q.w[3] * t[3];
                    denv[ch] = (g[ch] * irr) / fs;
                }
                drough += (((g[0] * env[0]) / fs + (g[1] * env[1]) / fs) + (g[2] * env[2]) / fs) * dq;
            }
        }
        // d_envmap[h, s0 .. s0+63, :] is 192 consecutive floats: three 256-byte wave-instructions, element j * 64 + lane each
        const int left = min(S - s0, IRR_WAVE) * 3;
        float* row = d_envmap + (h * (size_t)S + s0) * 3;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int el = j * IRR_WAVE + lane, src = el / 3, ch = el - src * 3;
            const float v0 = __shfl(denv[0], src), v1 = __shfl(denv[1], src), v2 = __shfl(denv[2], src);
            const float v = ch == 0 ? v0 : ch == 1 ? v1 : v2;
            if (el < left && v != 0.f) atomicAdd(row + el, v);
        }
    }
    float mine = 0.f;   // lane 4 * ch + k: d_albedos[h, 4 ch + k]; lane 12: d_roughnesses[h, 0]
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float t = wave_sum(dalb[ch][k]);
            if (lane == ch * 4 + k) mine = t;
        }
    const float tr = wave_sum(drough);
    if (lane == 12) mine = tr;
    if (lane < 12) atomicAdd(d_albedos + h * 12 + lane, mine);
    else if (lane == 12) atomicAdd(d_roughnesses + h * 4, mine);
}

bool irr_args_ok(int32_t N, int32_t S, const void* a, const void* b, const void* c, const void* d, const void* e2, const void* f,
                 const void* g) {
    if (N < 0 || S < 1) return false;
    if ((size_t)N * (size_t)S > ((size_t)1 << 31) - 1) return false;   // (entries / IRR_WAVES is the grid; rows stay int32-indexable)
    return N == 0 || (a && b && c && d && e2 && f && g);
}


// ---- the fused radiance-consistency loss -----------------------------------------------------------------------------------------------
// Forward, one wave per row i (IRR_WAVES rows per workgroup), lanes over samples in passes of 64:
//   1. selection: score_s = dot(d[i,s], r) * (1 - vis[i,s]) with v = (xyz_i - c) / max(|xyz_i - c|, 1e-12), r = (2 (g_i.v)) g_i + v, every
//      operation a separate fp32 one in the reference's order; p = torch.argmax's index: the first NaN if there is one, else the first index
//      of the maximum (+0 == -0).  Every lane keeps its best (value, index) over the passes -- a later equal value never displaces an earlier
//      index -- and a butterfly over the wave takes the best of the 64 under the same order.
//   2. the irradiance of h = hit[i,p] as in irradiance_kernel<false>, the light of a sample being (scale * bilinear(f(env))(d[h,s])) *
//      area[h,s] from the taps of the raw direction (env_taps<double>) and the f(env) float4 table.
//   3. T = nan_to_num(radiances[i,p] * ratio, nan = 0); the row's |R - T| (fp32 differences) is summed in double: wave, then workgroup
//      partials in wave order, then radiance_loss_final_kernel's fixed tree.  Same bits on every run.
// Backward, one wave per row in persistent workgroups of RLB_WAVES waves: d_R = g sign(R - T) / 3N from the saved p and R (zero where R or
// T is not finite), d_albedos / d_roughnesses as irradiance_sample_bwd_kernel, the env gradient scattered to the four taps of every
// contributing sample -- into a workgroup-private double table in LDS when it fits (flushed once per workgroup with float atomics), with
// global float atomics otherwise -- and d_ratio through per-workgroup partials.  radiance_loss_env_grad_kernel applies f'(env).
constexpr int RLB_WAVES = 8;                      // rows per pass of a backward workgroup
constexpr int RLB_MAX_BLOCKS = 1024;              // backward workgroups (= d_ratio partials) at most
constexpr size_t RL_LDS_BYTES = 160 * 1024;       // as shade_backward_impl: the double table must fit beside the kernel's other LDS

struct RadLossArgs {
    int N, S;
    const float *xyz, *cam, *geo, *ray_d, *area, *vis, *normals, *albedos, *roughnesses, *uvs, *radiances, *ratio;
    const int32_t* hit;
    const float4* env_tab;
    int env_h, env_w;
    float env_scale;
    const float* transform;   // device [9], row-major: the lookup direction is T d (EnvLight); null: none
    // forward
    int32_t* sample_out;
    float* R_out;
    double* partial;          // [ceil(N / IRR_WAVES)]
    // backward
    const int32_t* sample_in;
    const float *R_in, *g;
    float *d_albedos, *d_roughnesses, *d_envtab;   // d_envtab [He*We*3] (null: the env gets no gradient)
    double* ratio_part;       // [gridDim.x]
    int env_in_lds, ntex3;
};

struct RlTransform { float t[9]; bool on; };
__device__ __forceinline__ RlTransform rl_transform(const RadLossArgs& a) {
    RlTransform T;
    T.on = a.transform != nullptr;
#pragma unroll
    for (int j = 0; j < 9; j++) T.t[j] = T.on ? a.transform[j] : 0.f;
    return T;
}

// The coordinate type of the loss's lookup (env_taps<T>, env_lookup.hpp).  double: the gradient of a texel is a sum of (upstream *
// weight) terms and is held to a bound relative to those terms, so a weight must be good relative to ITSELF, and an fp32 coordinate --
// about We eps32 texels off, absolutely -- gives a weight of 0.01 only three digits.  (The forward value alone would not need it.)  The
// direction goes through the light's transform in the same type for the same reason.
using RlCoord = double;

// the light of one sample: taps of the (transformed) raw direction, env[c] = (scale * sum_j w_j f(env)[tap_j, c]) * area.  grid_sample's two
// corner rules as in backdrop.hip: a tap outside the map adds exactly 0, a tap inside is multiplied even at weight 0.  A direction with
// |d.z| > 1 has no latitude: acos is NaN, and the light is NaN as the reference's arccos makes it (`nan` says so whatever index the
// taps of a NaN coordinate got: env_taps range-checks them); a NaN light makes the row's R NaN, see the non-finite rule.
__device__ __forceinline__ void rl_light(const RadLossArgs& a, const RlTransform& T, const float* ld, float area, EnvTap& t, float* env) {
    RlCoord d[3] = {(RlCoord)ld[0], (RlCoord)ld[1], (RlCoord)ld[2]};
    if (T.on) {
#pragma unroll
        for (int j = 0; j < 3; j++) d[j] = ((RlCoord)T.t[3 * j] * ld[0] + (RlCoord)T.t[3 * j + 1] * ld[1]) + (RlCoord)T.t[3 * j + 2] * ld[2];
    }
    env_taps<RlCoord>(d, a.env_h, a.env_w, t);
    const bool nan = !(d[2] >= (RlCoord)-1 && d[2] <= (RlCoord)1) || d[0] != d[0] || d[1] != d[1];
    float4 tex[4];
#pragma unroll
    for (int j = 0; j < 4; j++) tex[j] = a.env_tab[t.idx[j] >= 0 ? t.idx[j] : 0];
    float E[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const bool ok = t.idx[j] >= 0;
        E[0] += ok ? t.w[j] * tex[j].x : 0.f;
        E[1] += ok ? t.w[j] * tex[j].y : 0.f;
        E[2] += ok ? t.w[j] * tex[j].z : 0.f;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ch++) env[ch] = nan ? NAN : (E[ch] * a.env_scale) * area;
}

// LIGHT_SG (svgir_radiance_loss_forward_sg / _backward_sg): envmap[h,s,c] = L_c(ray_d[h,s]) * areas[h,s] with L the unclamped fp32 SG light
// of the raw direction (sg_eval, m ascending; the prepared table in LDS).  No latitude, no transform: nothing to range-check.
__device__ __forceinline__ void rl_light_sg(const float4* __restrict__ st, int M, const float* ld, float area, float* env) {
    float L[3];
    sg_eval(st, M, ld, L);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) env[ch] = L[ch] * area;
}

// torch.argmax's order on (value, index) pairs: does (nv, ni) come before (bv, bi)?  An index < 0 is "no element".
__device__ __forceinline__ bool rl_before(float nv, int ni, float bv, int bi) {
    if (ni < 0) return false;
    if (bi < 0) return true;
    const bool nn = nv != nv, bn = bv != bv;
    if (nn || bn) return nn && (!bn || ni < bi);
    return nv > bv || (nv == bv && ni < bi);
}

__device__ __forceinline__ int rl_hit_of(const RadLossArgs& a, size_t i, int p) {
    if (p < 0 || p >= a.S) return -1;
    const int h = a.hit[i * (size_t)a.S + p];
    return (h < 0 || h >= a.N) ? -1 : h;
}

__global__ void __launch_bounds__(BLOCK) radiance_loss_table_kernel(const ShadeTables t, float* z0, size_t n0, float* z1, size_t n1) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < (size_t)t.entries()) shade_table_entry(t, (int)i);
    if (i < (size_t)t.nzero) t.zero[i] = 0.f;   // backward: the env-gradient table and the two per-surfel gradients
    if (i < n0) z0[i] = 0.f;
    if (i < n1) z1[i] = 0.f;
}

// LIGHT: the light kind (sg_light.hpp), a template parameter so that the texture kernels are the code they were.  The SG light travels in the
// otherwise unread env fields of RadLossArgs: env_tab = the prepared lobe table, env_w = the lobe count, d_envtab = the table-space sums.
template <int LIGHT>
__global__ void __launch_bounds__(BLOCK) radiance_loss_fwd_kernel(const RadLossArgs a) {
    __shared__ double wsum[IRR_WAVES];
    const float4* sgt = nullptr;
    if constexpr (LIGHT == LIGHT_SG) {
        __shared__ float4 st[2 * SVGIR_SG_MAX_LOBES];
        for (int k = threadIdx.x; k < 2 * a.env_w; k += BLOCK) st[k] = a.env_tab[k];
        __syncthreads();
        sgt = st;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t i = (size_t)blockIdx.x * IRR_WAVES + wave;
    const int S = a.S;
    double rowsum = 0.0;
    if (i < (size_t)a.N) {   // (wave-uniform)
        // 1. selection
        float v[3] = {a.xyz[i * 3] - a.cam[0], a.xyz[i * 3 + 1] - a.cam[1], a.xyz[i * 3 + 2] - a.cam[2]};
        const float len = fmaxf(sqrtf(irr_dot(v, v)), 1e-12f);
        v[0] = v[0] / len; v[1] = v[1] / len; v[2] = v[2] / len;
        const float gn[3] = {a.geo[i * 3], a.geo[i * 3 + 1], a.geo[i * 3 + 2]};
        const float two = 2.0f * irr_dot(gn, v);
        const float r[3] = {two * gn[0] + v[0], two * gn[1] + v[1], two * gn[2] + v[2]};
        float bv = 0.f;
        int bi = -1;
        for (int s = lane; s < S; s += IRR_WAVE) {
            const size_t is = i * (size_t)S + s;
            const float d[3] = {a.ray_d[is * 3], a.ray_d[is * 3 + 1], a.ray_d[is * 3 + 2]};
            const float sc = irr_dot(d, r) * (1.0f - a.vis[is]);
            if (rl_before(sc, s, bv, bi)) { bv = sc; bi = s; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float ov = __shfl_xor(bv, m);
            const int oi = __shfl_xor(bi, m);
            if (rl_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        const int p = __builtin_amdgcn_readfirstlane(bi);   // (S >= 1: a valid index)
        // 2. the irradiance of the hit surfel under the looked-up light
        const int hh = __builtin_amdgcn_readfirstlane(rl_hit_of(a, i, p));
        float acc[3] = {0.f, 0.f, 0.f};
        if (hh >= 0) {
            const size_t h = (size_t)hh;
            IrrCorners c;
            irr_row_corners<false>(c, a.ray_d, i, S, p, h, a.normals, a.albedos, a.roughnesses);
            const RlTransform T = rl_transform(a);
            const float fs = (float)S;
            for (int s = lane; s < S; s += IRR_WAVE) {
                const size_t hs = h * (size_t)S + s;
                if (a.hit[hs] != -1) continue;   // occluded secondary
                const float ld[3] = {a.ray_d[hs * 3], a.ray_d[hs * 3 + 1], a.ray_d[hs * 3 + 2]};
                IrrLight q;
                irr_light(q, c, ld, a.uvs[hs * 2], a.uvs[hs * 2 + 1]);
                EnvTap tp;
                float env[3];
                if constexpr (LIGHT == LIGHT_SG) rl_light_sg(sgt, a.env_w, ld, a.area[hs], env);
                else rl_light(a, T, ld, a.area[hs], tp, env);
                float b[4];
#pragma unroll
                for (int k = 0; k < 4; k++) b[k] = irr_spec<false>(c, q, k, nullptr);
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    float t[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) t[k] = b[k] + c.alb[ch][k] * IRR_1_PI;
                    const float irr = ((q.w[0] * t[0] + q.w[1] * t[1]) + q.w[2] * t[2]) + q.w[3] * t[3];
                    acc[ch] += (irr * env[ch]) / fs;
                }
            }
        }
        // 3. target and L1
        const float ratio = a.ratio[0];
        float diff[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            acc[ch] = wave_sum(acc[ch]);
            float t = a.radiances[(i * (size_t)S + p) * 3 + ch] * ratio;
            t = t != t ? 0.f : t;   // nan_to_num(nan = 0): +-inf stays
            diff[ch] = fabsf(acc[ch] - t);
        }
        rowsum = ((double)diff[0] + (double)diff[1]) + (double)diff[2];
        if (lane == 0) a.sample_out[i] = p;
        if (lane < 3) a.R_out[i * 3 + lane] = lane == 0 ? acc[0] : lane == 1 ? acc[1] : acc[2];
    }
    if (lane == 0) wsum[wave] = rowsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < IRR_WAVES; w++) t += wsum[w];
        a.partial[blockIdx.x] = t;
    }
}

constexpr int RL_FINAL = 1024;
// one workgroup: thread t adds partial[t], partial[t + 1024], ... in order, then a fixed tree.  sum_out = the sum, loss = fp32(sum / count)
__global__ void __launch_bounds__(RL_FINAL) radiance_loss_final_kernel(const double* __restrict__ partial, size_t n, double count,
                                                                       double* __restrict__ sum_out, float* __restrict__ loss) {
    const double t = block_tree_sum<double, RL_FINAL>(partial, n);
    if (threadIdx.x == 0) {
        *sum_out = t;
        *loss = (float)(t / count);
    }
}

// LIGHT_SG: sEnv holds the lobes' 8 M table-space sums (ntex3 = 8 M, env_in_lds = 1), behind it the prepared table (8 M floats) and every
// wave's 64 parked samples (direction, adjoint of L: two float4 each).  The sample loop runs in wave-uniform passes of 64: a lane parks the
// adjoint g_c = d_R[i,c] * irr_c / S * areas[h,s] of its sample's light (zeros for an occluded or absent sample, and for a channel without
// upstream) and the wave turns the pass into the lobes' sums with sg_adjoint_accumulate (sg_light.hpp).
template <int LIGHT>
__global__ void __launch_bounds__(RLB_WAVES * 64) radiance_loss_bwd_kernel(const RadLossArgs a) {
    extern __shared__ __attribute__((aligned(16))) double rl_smem[];   // [RLB_WAVES] the waves' d_ratio sums, then the env-gradient table [ntex3] (env_in_lds)
    double* sEnv = rl_smem + RLB_WAVES;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = a.S, N = a.N;
    float4 *sgt = nullptr, *recD = nullptr, *recG = nullptr;
    if constexpr (LIGHT == LIGHT_SG) {
        sgt = reinterpret_cast<float4*>(sEnv + a.ntex3);
        recD = sgt + 2 * a.env_w + wave * 128;
        recG = recD + 64;
        for (int k = threadIdx.x; k < 2 * a.env_w; k += RLB_WAVES * 64) sgt[k] = a.env_tab[k];
    }
    if (a.env_in_lds) {
        for (int k = threadIdx.x; k < a.ntex3; k += RLB_WAVES * 64) sEnv[k] = 0.0;
        __syncthreads();
    }
    const float gscale = a.g[0] / (float)(3.0 * (double)N);
    const float ratio = a.ratio[0];
    const RlTransform T = rl_transform(a);
    const float fs = (float)S;
    double ratio_acc = 0.0;   // (wave-uniform)
    for (size_t row0 = (size_t)blockIdx.x * RLB_WAVES; row0 < (size_t)N; row0 += (size_t)gridDim.x * RLB_WAVES) {
        const size_t i = row0 + wave;
        if (i >= (size_t)N) continue;   // (wave-uniform; no barrier inside the loop)
        const int p = __builtin_amdgcn_readfirstlane(a.sample_in[i]);
        if (p < 0 || p >= S) continue;
        float g[3];
        bool any = false;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float R = a.R_in[i * 3 + ch];
            const float raw = a.radiances[(i * (size_t)S + p) * 3 + ch];
            const float tr = raw * ratio;
            const float t = tr != tr ? 0.f : tr;
            // the non-finite rule: a non-finite R or T makes the loss NaN and gives no gradient
            const bool ok = fabsf(R) < INFINITY && fabsf(t) < INFINITY;
            const float df = R - t;
            const float sg = !ok ? 0.f : df > 0.f ? 1.f : df < 0.f ? -1.f : 0.f;
            g[ch] = sg * gscale;
            if (sg != 0.f && fabsf(tr) < INFINITY) ratio_acc += (double)(-(g[ch] * raw));   // nan_to_num passes the gradient of finite products only
            any = any || g[ch] != 0.f;
        }
        const int hh = __builtin_amdgcn_readfirstlane(rl_hit_of(a, i, p));
        if (hh < 0 || !any) continue;
        const size_t h = (size_t)hh;
        const float* vd = a.ray_d + (i * (size_t)S + p) * 3;
        const float vdir[3] = {vd[0], vd[1], vd[2]};
        IrrCorners c;
        irr_load_corners<false>(c, vdir, h, a.normals, a.albedos, a.roughnesses);
        float dalb[3][4] = {}, drough = 0.f;
        for (int s = lane; (LIGHT == LIGHT_SG ? s - lane : s) < S; s += IRR_WAVE) {   // (LIGHT_SG: whole passes, the wave stays together)
            const size_t hs = h * (size_t)S + s;
            if constexpr (LIGHT == LIGHT_SG) {
                float4 pd = make_float4(0.f, 0.f, 0.f, 0.f), pg = pd;
                if (s < S && a.hit[hs] == -1) {
                    const float ld[3] = {a.ray_d[hs * 3], a.ray_d[hs * 3 + 1], a.ray_d[hs * 3 + 2]};
                    IrrLight q;
                    irr_light(q, c, ld, a.uvs[hs * 2], a.uvs[hs * 2 + 1]);
                    const float area = a.area[hs];
                    float env[3];
                    rl_light_sg(sgt, a.env_w, ld, area, env);
                    float b[4], ds[4], gl[3] = {0.f, 0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < 4; k++) b[k] = irr_spec<true>(c, q, k, &ds[k]);
                    const float dq = ((q.w[0] * ds[0] + q.w[1] * ds[1]) + q.w[2] * ds[2]) + q.w[3] * ds[3];
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) {
                        float t[4];
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            t[k] = b[k] + c.alb[ch][k] * IRR_1_PI;
                            if (g[ch] != 0.f) dalb[ch][k] += (((g[ch] * q.w[k]) * env[ch]) * IRR_1_PI) / fs;   // (skipped, not multiplied by 0: see below)
                        }
                        const float irr = ((q.w[0] * t[0] + q.w[1] * t[1]) + q.w[2] * t[2]) + q.w[3] * t[3];
                        if (g[ch] != 0.f) gl[ch] = ((g[ch] * irr) / fs) * area;   // d L / d L_ch(ray_d[h,s])
                    }
                    const float ge[3] = {g[0] != 0.f ? (g[0] * env[0]) / fs : 0.f, g[1] != 0.f ? (g[1] * env[1]) / fs : 0.f,
                                         g[2] != 0.f ? (g[2] * env[2]) / fs : 0.f};
                    drough += ((ge[0] + ge[1]) + ge[2]) * dq;
                    pd = make_float4(ld[0], ld[1], ld[2], 0.f);
                    pg = make_float4(gl[0], gl[1], gl[2], 0.f);
                }
                if (a.d_envtab) {   // (uniform)
                    recD[lane] = pd; recG[lane] = pg;
                    wave_lds_sync();
                    sg_adjoint_accumulate(recD, recG, min(IRR_WAVE, S - (s - lane)), sgt, sEnv, a.env_w, lane, IRR_WAVE);
                    wave_lds_sync();
                }
                continue;
            }
            if (a.hit[hs] != -1) continue;
            const float ld[3] = {a.ray_d[hs * 3], a.ray_d[hs * 3 + 1], a.ray_d[hs * 3 + 2]};
            IrrLight q;
            irr_light(q, c, ld, a.uvs[hs * 2], a.uvs[hs * 2 + 1]);
            const float area = a.area[hs];
            EnvTap tp;
            float env[3];
            rl_light(a, T, ld, area, tp, env);
            float b[4], ds[4];
#pragma unroll
            for (int k = 0; k < 4; k++) b[k] = irr_spec<true>(c, q, k, &ds[k]);
            const float dq = ((q.w[0] * ds[0] + q.w[1] * ds[1]) + q.w[2] * ds[2]) + q.w[3] * ds[3];
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                float t[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    t[k] = b[k] + c.alb[ch][k] * IRR_1_PI;
                    // (a channel without upstream is SKIPPED, not multiplied by 0: its light may be the NaN / inf that made R[i,ch] non-finite)
                    if (g[ch] != 0.f) dalb[ch][k] += (((g[ch] * q.w[k]) * env[ch]) * IRR_1_PI) / fs;
                }
                const float irr = ((q.w[0] * t[0] + q.w[1] * t[1]) + q.w[2] * t[2]) + q.w[3] * t[3];
                if (a.d_envtab && g[ch] != 0.f) {
                    const float de = (((g[ch] * irr) / fs) * area) * a.env_scale;   // d L / d (the bilinear value of channel ch)
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const float dv = de * tp.w[j];
                        if (tp.idx[j] >= 0 && dv != 0.f) {
                            if (a.env_in_lds) atomicAdd(&sEnv[tp.idx[j] * 3 + ch], (double)dv);   // ds_add_f64
                            else atomic_add_f32(a.d_envtab + (size_t)tp.idx[j] * 3 + ch, dv);
                        }
                    }
                }
            }
            const float ge[3] = {g[0] != 0.f ? (g[0] * env[0]) / fs : 0.f, g[1] != 0.f ? (g[1] * env[1]) / fs : 0.f,
                                 g[2] != 0.f ? (g[2] * env[2]) / fs : 0.f};
            drough += ((ge[0] + ge[1]) + ge[2]) * dq;
        }
        float mine = 0.f;   // lane 4 * ch + k: d_albedos[h, 4 ch + k]; lane 12: d_roughnesses[h, 0]
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float t = wave_sum(dalb[ch][k]);
                if (lane == ch * 4 + k) mine = t;
            }
        const float tr = wave_sum(drough);
        if (lane == 12) mine = tr;
        if (lane < 12) atomicAdd(a.d_albedos + h * 12 + lane, mine);
        else if (lane == 12) atomicAdd(a.d_roughnesses + h * 4, mine);
    }
    if (lane == 0) rl_smem[wave] = ratio_acc;
    __syncthreads();   // (also: every wave's LDS adds are done)
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < RLB_WAVES; w++) t += rl_smem[w];
        a.ratio_part[blockIdx.x] = t;
    }
    if (a.env_in_lds) {
        for (int k = threadIdx.x; k < a.ntex3; k += RLB_WAVES * 64) {
            const float v = (float)sEnv[k];
            if (v != 0.f) atomic_add_f32(&a.d_envtab[k], v);
        }
    }
}

// d_ratio = the backward workgroups' partial sums in a fixed tree (one workgroup of BLOCK threads)
__device__ __forceinline__ void rl_ratio_tree(const double* __restrict__ ratio_part, int nparts, float* __restrict__ d_ratio) {
    const double t = block_tree_sum<double, BLOCK>(ratio_part, nparts);
    if (threadIdx.x == 0) *d_ratio = (float)t;
}

// d_env = d f(env) * f'(env) (softplus' = sigmoid; an element nothing was added to is exactly 0, whatever env holds there) and, in
// workgroup 0, d_ratio = the workgroups' partial sums in a fixed tree
__global__ void __launch_bounds__(BLOCK) radiance_loss_env_grad_kernel(const float* __restrict__ env, const float* __restrict__ dtab,
                                                                       float* __restrict__ denv, int n, int softplus,
                                                                       const double* __restrict__ ratio_part, int nparts,
                                                                       float* __restrict__ d_ratio) {
    if (d_ratio && blockIdx.x == 0) rl_ratio_tree(ratio_part, nparts, d_ratio);
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (!denv || i >= n) return;
    const float d = dtab[i], x = env[i];
    denv[i] = d == 0.f ? 0.f : softplus ? d * (x > 20.f ? 1.f : 1.f / (1.f + expf(-x))) : d;
}

// the work buffer of both lights: [the light's table | the light's gradient table, floats | partial sums, doubles].  Texture: the f(env)
// float4 table and the env-gradient table [He*We*3]; SG: no table (the prepared one is light->work) and the 8 M table-space sums.
struct RlWork { size_t tab, dtab, part, bytes, nparts; };
RlWork rl_work(int32_t N, size_t tab_bytes, size_t dtab_floats) {
    RlWork w;
    w.tab = 0;
    w.dtab = tab_bytes;
    w.part = w.dtab + ((dtab_floats * 4 + 15) & ~(size_t)15);
    w.nparts = std::max(((size_t)N + IRR_WAVES - 1) / IRR_WAVES, (size_t)RLB_MAX_BLOCKS);
    w.bytes = w.part + w.nparts * 8;
    return w;
}

// (sg: the _sg entry points, which do not read the env* fields)
bool rl_args_ok(const svgir_radiance_loss_params* p, bool sg = false) {
    if (!p || p->N < 0 || p->S < 1 || (!sg && (p->env_h < 1 || p->env_w < 1))) return false;
    if ((size_t)p->N * (size_t)p->S > ((size_t)1 << 31) - 1 || (!sg && (int64_t)p->env_h * p->env_w > (int64_t)1 << 26)) return false;
    if (p->N == 0) return true;
    return p->xyz && p->camera_center && p->geo_normal && p->ray_d && p->areas && p->visibility && p->normals && p->albedos && p->roughnesses &&
           p->hit_indices && p->uvs && p->radiances && p->radiance_ratio && (sg || p->env) && p->work && !((uintptr_t)p->work & 15);
}

// The backward's persistent grid: as many workgroups as are resident at once (registers and the LDS table both bound the workgroups per
// CU: one at ~230 VGPRs whatever the table), RLB_MAX_BLOCKS at most -- every further workgroup would zero and flush a table of its own for
// nothing.  Per device and light kind: the opt-in for > 64 KB of dynamic LDS, set once, and the resident count of the last LDS size asked
// for (a training run has one map size; both are idempotent, so races are harmless).  0: a HIP call failed.
template <int LIGHT>
size_t rl_resident(size_t lds) {
    struct DevState { bool attr_set; size_t lds, resident; };
    static DevState state[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    const bool slot = dev >= 0 && dev < 64;
    if (!slot || !state[dev].attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(radiance_loss_bwd_kernel<LIGHT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)RL_LDS_BYTES) != hipSuccess)
            return 0;
        if (slot) state[dev].attr_set = true;
    }
    if (slot && state[dev].resident != 0 && state[dev].lds == lds) return state[dev].resident;
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(radiance_loss_bwd_kernel<LIGHT>), RLB_WAVES * 64, lds) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return 0;
    const size_t resident = (size_t)std::max(per_cu, 1) * (size_t)std::max(cus, 1);
    if (slot) { state[dev].resident = 0; state[dev].lds = lds; state[dev].resident = resident; }
    return resident;
}

// prologue of both SG calls: the prepared table; backward: the clear of the table-space sums and of the two per-surfel gradients
__global__ void __launch_bounds__(BLOCK) radiance_loss_sg_table_kernel(const float* __restrict__ lobes, int M, float4* __restrict__ tab,
                                                                       float* __restrict__ zero, int nzero, float* z0, size_t n0, float* z1, size_t n1) {
    sg_table_build(lobes, M, tab, zero, nzero);
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n0) z0[i] = 0.f;
    if (i < n1) z1[i] = 0.f;
}

// epilogue of the SG backward (one workgroup): the pull-back of the table-space sums to d_lobes [M,7] and d_ratio = the workgroups' partial
// sums in radiance_loss_env_grad_kernel's fixed tree
__global__ void __launch_bounds__(BLOCK) radiance_loss_sg_grad_kernel(const float* __restrict__ lobes, const float4* __restrict__ tab,
                                                                      const float* __restrict__ dtab, float* __restrict__ dlobes, int M,
                                                                      const double* __restrict__ ratio_part, int nparts, float* __restrict__ d_ratio) {
    if (d_ratio) rl_ratio_tree(ratio_part, nparts, d_ratio);
    if (dlobes && (int)threadIdx.x < M) sg_pullback(lobes, tab, dtab, threadIdx.x, dlobes);
}

static_assert(SVGIR_SG_MAX_LOBES <= BLOCK, "radiance_loss_sg_grad_kernel: one thread per lobe, one block");

// ---- the host side of the four loss calls, per light kind (l: the SG light, null for the texture, whose light is in p) --------------------
template <int LIGHT>
RlWork rl_work_of(const svgir_radiance_loss_params* p, const svgir_sg_light* l) {
    if (LIGHT == LIGHT_SG) return rl_work(p->N, 0, (size_t)8 * l->count);
    return rl_work(p->N, (size_t)p->env_h * p->env_w * 16, (size_t)p->env_h * p->env_w * 3);
}

template <int LIGHT>
RadLossArgs rl_args(const svgir_radiance_loss_params* p, const svgir_sg_light* l, const RlWork& w) {
    RadLossArgs a{};
    a.N = p->N; a.S = p->S;
    a.xyz = p->xyz; a.cam = p->camera_center; a.geo = p->geo_normal; a.ray_d = p->ray_d; a.area = p->areas; a.vis = p->visibility;
    a.normals = p->normals; a.albedos = p->albedos; a.roughnesses = p->roughnesses; a.uvs = p->uvs; a.radiances = p->radiances;
    a.ratio = p->radiance_ratio; a.hit = p->hit_indices;
    if constexpr (LIGHT == LIGHT_SG) {
        a.env_tab = (const float4*)l->work; a.env_h = 1; a.env_w = l->count; a.env_scale = 1.f;
    } else {
        a.env_tab = (const float4*)((char*)p->work + w.tab);
        a.env_h = p->env_h; a.env_w = p->env_w; a.env_scale = p->env_scale; a.transform = p->env_transform;
        a.ntex3 = p->env_h * p->env_w * 3;
    }
    return a;
}

// prologue of every call: the light's table; backward: the clear of a.d_envtab and of the two per-surfel gradients z0 [n0], z1 [n1]
template <int LIGHT>
void rl_prologue(const svgir_radiance_loss_params* p, const svgir_sg_light* l, const RlWork& w, const RadLossArgs& a, float* z0, size_t n0,
                 float* z1, size_t n1, hipStream_t s) {
    if constexpr (LIGHT == LIGHT_SG) {
        hipLaunchKernelGGL(radiance_loss_sg_table_kernel, dim3((unsigned)std::max<size_t>((n0 + BLOCK - 1) / BLOCK, 1)), dim3(BLOCK), 0, s, l->lobes,
                           l->count, (float4*)l->work, a.d_envtab, a.ntex3, z0, n0, z1, n1);
    } else {
        ShadeTables t;
        t.env = p->env; t.env_tab = (float4*)((char*)p->work + w.tab); t.ntexel = p->env_h * p->env_w; t.softplus = p->env_softplus;
        t.zero = a.d_envtab; t.nzero = a.d_envtab ? a.ntex3 : 0;
        const size_t items = std::max(std::max((size_t)t.ntexel, (size_t)t.nzero), n0);
        hipLaunchKernelGGL(radiance_loss_table_kernel, dim3((unsigned)((items + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, t, z0, n0, z1, n1);
    }
}

// table prologue -> radiance_loss_fwd_kernel<LIGHT> -> radiance_loss_final_kernel; false: a launch failed
template <int LIGHT>
bool rl_forward(const svgir_radiance_loss_params* p, const svgir_sg_light* l, int32_t* sample_indices, float* radiance, double* loss_sum,
                float* loss, hipStream_t s) {
    const RlWork w = rl_work_of<LIGHT>(p, l);
    RadLossArgs a = rl_args<LIGHT>(p, l, w);
    a.sample_out = sample_indices; a.R_out = radiance; a.partial = (double*)((char*)p->work + w.part);
    const size_t blocks = ((size_t)p->N + IRR_WAVES - 1) / IRR_WAVES;
    rl_prologue<LIGHT>(p, l, w, a, nullptr, 0, nullptr, 0, s);
    hipLaunchKernelGGL(radiance_loss_fwd_kernel<LIGHT>, dim3((unsigned)blocks), dim3(BLOCK), 0, s, a);
    hipLaunchKernelGGL(radiance_loss_final_kernel, dim3(1), dim3(RL_FINAL), 0, s, (const double*)a.partial, blocks, 3.0 * (double)p->N, loss_sum,
                       loss);
    return hipGetLastError() == hipSuccess;
}

// table prologue and clears -> radiance_loss_bwd_kernel<LIGHT> in persistent workgroups -> the light's gradient epilogue, which also sums
// d_ratio.  d_light: d_env [He,We,3] or d_lobes [M,7] (null: the light gets no gradient).  Returns what failed, null when nothing did.
template <int LIGHT>
const char* rl_backward(const svgir_radiance_loss_params* p, const svgir_sg_light* l, const int32_t* sample_indices, const float* radiance,
                        const float* d_loss, float* d_light, float* d_albedos, float* d_roughnesses, float* d_radiance_ratio, hipStream_t s) {
    const RlWork w = rl_work_of<LIGHT>(p, l);
    RadLossArgs a = rl_args<LIGHT>(p, l, w);
    a.sample_in = sample_indices; a.R_in = radiance; a.g = d_loss; a.d_albedos = d_albedos; a.d_roughnesses = d_roughnesses;
    a.d_envtab = d_light ? (float*)((char*)p->work + w.dtab) : nullptr;
    a.ratio_part = (double*)((char*)p->work + w.part);
    size_t lds = (size_t)RLB_WAVES * 8;   // the waves' d_ratio sums, then the light's fp64 sums
    if constexpr (LIGHT == LIGHT_SG) {
        // ... the prepared table, the waves' parked samples (two float4 per lane): 29 KB at M = 128
        a.env_in_lds = 1; a.ntex3 = d_light ? 8 * l->count : 0;
        lds += (size_t)a.ntex3 * 8 + (size_t)8 * l->count * 4 + (size_t)RLB_WAVES * 128 * 16;
    } else if (d_light && lds + (size_t)a.ntex3 * 8 <= RL_LDS_BYTES) {
        a.env_in_lds = 1; lds += (size_t)a.ntex3 * 8;
    }
    const size_t resident = rl_resident<LIGHT>(lds);   // (persistent workgroups)
    if (!resident) return "querying the device failed";
    const int blocks = (int)std::min<size_t>(((size_t)p->N + RLB_WAVES - 1) / RLB_WAVES, std::min<size_t>(resident, RLB_MAX_BLOCKS));
    rl_prologue<LIGHT>(p, l, w, a, d_albedos, (size_t)p->N * 12, d_roughnesses, (size_t)p->N * 4, s);
    hipLaunchKernelGGL(radiance_loss_bwd_kernel<LIGHT>, dim3(blocks), dim3(RLB_WAVES * 64), lds, s, a);
    if (d_light || d_radiance_ratio) {
        if constexpr (LIGHT == LIGHT_SG)
            hipLaunchKernelGGL(radiance_loss_sg_grad_kernel, dim3(1), dim3(BLOCK), 0, s, l->lobes, (const float4*)l->work, (const float*)a.d_envtab,
                               d_light, l->count, (const double*)a.ratio_part, blocks, d_radiance_ratio);
        else
            hipLaunchKernelGGL(radiance_loss_env_grad_kernel, dim3(d_light ? (a.ntex3 + BLOCK - 1) / BLOCK : 1), dim3(BLOCK), 0, s, p->env,
                               (const float*)a.d_envtab, d_light, a.ntex3, p->env_softplus, (const double*)a.ratio_part, blocks, d_radiance_ratio);
    }
    return hipGetLastError() == hipSuccess ? nullptr : "launch failed";
}

}  // namespace

}  // namespace svgir

extern "C" {

size_t svgir_radiance_loss_work_bytes(int32_t N, int32_t env_h, int32_t env_w) {
    if (N < 0 || env_h < 1 || env_w < 1 || (int64_t)env_h * env_w > (int64_t)1 << 26) return 0;
    return svgir::rl_work(N, (size_t)env_h * env_w * 16, (size_t)env_h * env_w * 3).bytes;
}

int svgir_radiance_loss_forward(const svgir_radiance_loss_params* p, int32_t* sample_indices, float* radiance, double* loss_sum, float* loss,
                                void* stream) {
    using namespace svgir;
    if (!rl_args_ok(p) || (p->N > 0 && (!sample_indices || !radiance || !loss_sum || !loss))) return SVGIR_ERR_INVALID;
    if (p->N == 0) return 0;
    return rl_forward<LIGHT_TEX>(p, nullptr, sample_indices, radiance, loss_sum, loss, (hipStream_t)stream) ? 0 : SVGIR_ERR_HIP;
}

int svgir_radiance_loss_backward(const svgir_radiance_loss_params* p, const int32_t* sample_indices, const float* radiance, const float* d_loss,
                                 float* d_env, float* d_albedos, float* d_roughnesses, float* d_radiance_ratio, void* stream) {
    using namespace svgir;
    if (!rl_args_ok(p) || (p->N > 0 && (!sample_indices || !radiance || !d_loss || !d_albedos || !d_roughnesses))) return SVGIR_ERR_INVALID;
    if (p->N == 0) return 0;
    return rl_backward<LIGHT_TEX>(p, nullptr, sample_indices, radiance, d_loss, d_env, d_albedos, d_roughnesses, d_radiance_ratio,
                                  (hipStream_t)stream) ? SVGIR_ERR_HIP : 0;
}

size_t svgir_radiance_loss_sg_work_bytes(int32_t N, int32_t count) {
    if (N < 0 || count < 1 || count > SVGIR_SG_MAX_LOBES) return 0;
    return svgir::rl_work(N, 0, (size_t)8 * count).bytes;
}

int svgir_radiance_loss_forward_sg(const svgir_radiance_loss_params* p, const svgir_sg_light* light, int32_t* sample_indices, float* radiance,
                                   double* loss_sum, float* loss, void* stream) {
    using namespace svgir;
    if (int rc = sg_light_valid(light, "radiance_loss_forward_sg")) return rc;
    if (!rl_args_ok(p, true) || (p->N > 0 && (!sample_indices || !radiance || !loss_sum || !loss)))
        return report_error(SVGIR_ERR_INVALID, "radiance_loss_forward_sg: bad N / S, a NULL input or output, or a NULL / misaligned work");
    if (p->N == 0) return 0;
    return rl_forward<LIGHT_SG>(p, light, sample_indices, radiance, loss_sum, loss, (hipStream_t)stream)
               ? 0 : report_error(SVGIR_ERR_HIP, "radiance_loss_forward_sg: launch failed");
}

int svgir_radiance_loss_backward_sg(const svgir_radiance_loss_params* p, const svgir_sg_light* light, const int32_t* sample_indices,
                                    const float* radiance, const float* d_loss, float* d_lobes, float* d_albedos, float* d_roughnesses,
                                    float* d_radiance_ratio, void* stream) {
    using namespace svgir;
    if (int rc = sg_light_valid(light, "radiance_loss_backward_sg")) return rc;
    if (!rl_args_ok(p, true) || (p->N > 0 && (!sample_indices || !radiance || !d_loss || !d_albedos || !d_roughnesses)))
        return report_error(SVGIR_ERR_INVALID, "radiance_loss_backward_sg: bad N / S, a NULL input or output, or a NULL / misaligned work");
    if (p->N == 0) return 0;
    const char* failed = rl_backward<LIGHT_SG>(p, light, sample_indices, radiance, d_loss, d_lobes, d_albedos, d_roughnesses, d_radiance_ratio,
                                               (hipStream_t)stream);
    return failed ? report_error(SVGIR_ERR_HIP, "radiance_loss_backward_sg: %s", failed) : 0;
}

int svgir_pbgi_irradiance_sample(int32_t N, int32_t S, const int32_t* sample_indices, const float* ray_d, const float* envmap,
                                 const float* normals, const float* albedos, const float* roughnesses, const int32_t* hit_indices,
                                 const float* uvs, float* out, void* stream) {
    using namespace svgir;
    if (!irr_args_ok(N, S, ray_d, envmap, normals, albedos, roughnesses, hit_indices, uvs) || (N > 0 && (!sample_indices || !out)))
        return SVGIR_ERR_INVALID;
    if (N == 0) return 0;
    hipLaunchKernelGGL(irradiance_kernel<false>, dim3((unsigned)(((size_t)N + IRR_WAVES - 1) / IRR_WAVES)), dim3(BLOCK), 0, (hipStream_t)stream, N, S,
                       (size_t)N, sample_indices, ray_d, envmap, normals, albedos, roughnesses, hit_indices, uvs, out);
    return hipGetLastError() == hipSuccess ? 0 : SVGIR_ERR_HIP;
}

int svgir_pbgi_irradiance_sample_backward(int32_t N, int32_t S, const int32_t* sample_indices, const float* ray_d, const float* envmap,
                                          const float* normals, const float* albedos, const float* roughnesses,
                                          const int32_t* hit_indices, const float* uvs, const float* d_out, float* d_envmap,
                                          float* d_albedos, float* d_roughnesses, void* stream) {
    using namespace svgir;
    if (!irr_args_ok(N, S, ray_d, envmap, normals, albedos, roughnesses, hit_indices, uvs) ||
        (N > 0 && (!sample_indices || !d_out || !d_envmap || !d_albedos || !d_roughnesses)))
        return SVGIR_ERR_INVALID;
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d_envmap, 0, (size_t)N * S * 3 * sizeof(float), s) != hipSuccess ||
        hipMemsetAsync(d_albedos, 0, (size_t)N * 12 * sizeof(float), s) != hipSuccess ||
        hipMemsetAsync(d_roughnesses, 0, (size_t)N * 4 * sizeof(float), s) != hipSuccess)
        return SVGIR_ERR_HIP;
    hipLaunchKernelGGL(irradiance_sample_bwd_kernel, dim3((unsigned)(((size_t)N + IRR_WAVES - 1) / IRR_WAVES)), dim3(BLOCK), 0, s, N, S, sample_indices,
                       ray_d, envmap, normals, albedos, roughnesses, hit_indices, uvs, d_out, d_envmap, d_albedos, d_roughnesses);
    return hipGetLastError() == hipSuccess ? 0 : SVGIR_ERR_HIP;
}

int svgir_pbgi_irradiance(int32_t N, int32_t S, const float* ray_d, const float* envmap, const float* normals, const float* albedos,
                          const float* roughnesses, const int32_t* hit_indices, const float* uvs, float* out, void* stream) {
    using namespace svgir;
    if (!irr_args_ok(N, S, ray_d, envmap, normals, albedos, roughnesses, hit_indices, uvs) || (N > 0 && !out)) return SVGIR_ERR_INVALID;
    if (N == 0) return 0;
    const size_t entries = (size_t)N * S;
    hipLaunchKernelGGL(irradiance_kernel<true>, dim3((unsigned)((entries + IRR_WAVES - 1) / IRR_WAVES)), dim3(BLOCK), 0, (hipStream_t)stream, N, S,
                       entries, (const int32_t*)nullptr, ray_d, envmap, normals, albedos, roughnesses, hit_indices, uvs, out);
    return hipGetLastError() == hipSuccess ? 0 : SVGIR_ERR_HIP;
}

}  // extern "C"
