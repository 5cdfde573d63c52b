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
#include <cmath>

#include "common.hpp"

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
        const float* vd = ray_d + (i * (size_t)S + p) * 3;
        const float vdir[3] = {vd[0], vd[1], vd[2]};
        IrrCorners c;
        irr_load_corners<FULL>(c, vdir, h, normals, albedos, roughnesses);
        const float fs = (float)S;
        for (int s = lane; s < S; s += IRR_WAVE) {
            const size_t hs = h * (size_t)S + s;
            if (hit[hs] != -1) continue;   // occluded secondary
            const float ld[3] = {ray_d[hs * 3], ray_d[hs * 3 + 1], ray_d[hs * 3 + 2]};
            IrrLight q;
            irr_light(q, c, ld, uvs[hs * 2], uvs[hs * 2 + 1]);
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
    const float* vd = ray_d + (i * (size_t)S + p) * 3;
    const float vdir[3] = {vd[0], vd[1], vd[2]};
    const float g[3] = {d_out[i * 3], d_out[i * 3 + 1], d_out[i * 3 + 2]};
    IrrCorners c;
    irr_load_corners<false>(c, vdir, h, normals, albedos, roughnesses);
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

}  // namespace

}  // namespace svgir

extern "C" {

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
