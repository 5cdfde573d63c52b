// svg-ir_amd/csrc/sg_light.hpp -- the lobe arithmetic of the spherical-Gaussian direct light (scene/direct_light_sg.py:
// render_envmap_sg / DirectLightSG.direct_light), shared by the prepared-table prologue, svgir_sg_eval and the SG instantiations of the
// shading kernels (csrc/shade.hip), and -- the second half of the file: the gradient's building blocks -- also by the light's other
// consumers: the eval backward (csrc/sg_light.hip), the eval view's backdrop (csrc/backdrop.hip) and the fused radiance-consistency loss
// (csrc/irradiance.hip).
//
// Raw parameters: lobes [M,7] = (xi.xyz, lambda, mu.rgb).  Light of a direction d (used as given):
//   a = xi / |xi|,  e = exp(|lambda| (d.a - 1)),  L_c = sum_m |mu_mc| e_m      (fp32, m ascending, the accurate expf: |lambda| is in the
//   hundreds and the exponent's argument spans the whole range down to the underflow)
// Prepared table (svgir_sg_light.work): two float4 per lobe, {a.xyz, |lambda|} and {|mu|.rgb, 1 / |xi|} -- the normalisation, the abs and
// the division happen once per call instead of once per (sample, lobe).
#pragma once
#include "common.hpp"

namespace svgir {

constexpr int LIGHT_TEX = 0, LIGHT_SG = 1;   // the light kind of a shading-kernel instantiation

#if defined(__HIPCC__)
// table entry of lobe m.  A plain sqrt of the sum of squares and a plain division, as torch.norm and `/` do: no clamp -- a zero or
// non-finite axis makes the lobe (and with it the light of every direction) NaN, as in the reference.
__device__ __forceinline__ void sg_table_entry(const float* __restrict__ lobes, int m, float4* __restrict__ tab) {
    const float* l = lobes + 7 * m;
    float nrm;
    {
#pragma clang fp contract(off)
        nrm = sqrtf(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
    }
    tab[2 * m] = make_float4(l[0] / nrm, l[1] / nrm, l[2] / nrm, fabsf(l[3]));
    tab[2 * m + 1] = make_float4(fabsf(l[4]), fabsf(l[5]), fabsf(l[6]), 1.f / nrm);
}

// The accurate exponential, the way the device library's expf is built: x log2(e) as a two-float product ph + pl, the integer part of ph
// through ldexp, so that v_exp_f32 (1 ulp) only ever sees |r| <= 1/2 -- at x = -300 the plain exp2(x * log2e) is off by 3e-5 relative from
// the product's rounding alone.  Without expf's range special cases (their constants cost the backward kernel, which sits at its register
// limit, two spilled dwords): ldexp saturates to 0 / inf by itself and NaN passes through; x = +-inf gives NaN (inf - inf), which is
// what the contract asks of a non-finite lobe.
__device__ __forceinline__ float sg_exp(float x) {
    const float ph = x * 1.44269502e+0f;
    const float pl = fmaf(x, 1.92596299e-8f, fmaf(x, 1.44269502e+0f, -ph));
    const float n = rintf(ph);
    return ldexpf(__builtin_amdgcn_exp2f((ph - n) + pl), (int)n);
}

// d.a - 1 and e of one lobe
__device__ __forceinline__ float sg_lobe(const float4 al, const float* d, float& t) {
    t = d[0] * al.x + d[1] * al.y + d[2] * al.z - 1.f;
    return sg_exp(al.w * t);
}

// L[3] = the unclamped light of direction d; `tab` usually lives in LDS (every lane reads the same entry: a broadcast)
__device__ __forceinline__ void sg_eval(const float4* __restrict__ tab, int M, const float* d, float* L) {
    float l0 = 0.f, l1 = 0.f, l2 = 0.f;
    for (int m = 0; m < M; m++) {
        const float4 al = tab[2 * m], mu = tab[2 * m + 1];
        float t;
        const float e = sg_lobe(al, d, t);
        l0 += mu.x * e; l1 += mu.y * e; l2 += mu.z * e;
    }
    L[0] = l0; L[1] = l1; L[2] = l2;
}

// torch.clamp(L, 0, 64): NaN stays NaN (fminf / fmaxf would return the bound)
__device__ __forceinline__ float sg_clamp(float L) { return L != L ? L : fminf(64.f, fmaxf(0.f, L)); }

// ---- the building blocks of the light's kernels (shade.hip, sg_light.hip, backdrop.hip, irradiance.hip).  A kernel cannot be launched
// across translation units, so each unit wraps these in small __global__ kernels of its own.

// the prepared table of the whole light and the clear of `zero` [nzero], by every thread of a 1-D grid of at least M threads
__device__ __forceinline__ void sg_table_build(const float* __restrict__ lobes, int M, float4* __restrict__ tab, float* __restrict__ zero, int nzero) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < M) sg_table_entry(lobes, i, tab);
    for (int j = i; j < nzero; j += gridDim.x * blockDim.x) zero[j] = 0.f;
}

// The lobes' share of `cnt` parked samples: sD[s] = {d.xyz, -} the direction and sG[s] = {g.rgb, -} the adjoint of the sample's unclamped
// light, both in LDS.  The `nthr` threads that call it together (a power of two: a wave, or a workgroup) are split into groups of
// lpg = the power of two >= M (at most nthr) threads, tid % lpg = the lobe (several lobes per thread when M > nthr) and group j walks the
// samples j, j + ngroups, ...: records are LDS broadcasts, e is recomputed, and the seven table-space sums of a lobe
//     d|mu|_c = sum e g_c,   d|lambda| = sum (d.a - 1) s,   G = sum s d      with s = sum_c |mu_c| e g_c   (dL/da = |lambda| G)
// stay private to the thread for the call; they then go to the fp64 accumulator acc[8 M] = {G.xyz, d|lambda|, d|mu|.rgb, -} in LDS with
// seven ds_add_f64 (the layout and the scheme of shade.hip's sg_chunk_adjoint, which stays a copy of this loop over the shading backward's
// own records: routed through here that kernel measured 1.4 % slower).  A sample whose adjoint is all zero is skipped.
// The caller orders the records' writes before the call and their reuse after it (a barrier, or wave_lds_sync for wave-private records).
__device__ __forceinline__ void sg_adjoint_accumulate(const float4* __restrict__ sD, const float4* __restrict__ sG, int cnt,
                                                      const float4* __restrict__ tab, double* __restrict__ acc, int M, int tid, int nthr) {
    const int full = 31 - __builtin_clz((unsigned)nthr);
    const int lpg_shift = min(full, 32 - __builtin_clz((unsigned)max(M, 2) - 1u));
    const int lpg = 1 << lpg_shift, lm = tid & (lpg - 1), grp = tid >> lpg_shift, ngrp = nthr >> lpg_shift;
    for (int m = lm; m < M; m += lpg) {
        const float4 al = tab[2 * m], mu = tab[2 * m + 1];
        float gm[3] = {0.f, 0.f, 0.f}, ga[3] = {0.f, 0.f, 0.f}, gl = 0.f;
        for (int s = grp; s < cnt; s += ngrp) {
            const float4 dq = sD[s], gq = sG[s];
            if (gq.x == 0.f && gq.y == 0.f && gq.z == 0.f) continue;
            const float d[3] = {dq.x, dq.y, dq.z};
            float t;
            const float e = sg_lobe(al, d, t);
            const float e0 = e * gq.x, e1 = e * gq.y, e2 = e * gq.z;
            const float sv = mu.x * e0 + mu.y * e1 + mu.z * e2;
            gm[0] += e0; gm[1] += e1; gm[2] += e2;
            gl += t * sv;
            ga[0] += sv * d[0]; ga[1] += sv * d[1]; ga[2] += sv * d[2];
        }
        double* o = acc + 8 * m;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            if (ga[j] != 0.f) atomicAdd(&o[j], (double)ga[j]);        // ds_add_f64
            if (gm[j] != 0.f) atomicAdd(&o[4 + j], (double)gm[j]);
        }
        if (gl != 0.f) atomicAdd(&o[3], (double)gl);
    }
}

// the workgroup's fp64 sums acc[8 M] (LDS) to the table-space sums dtab[8 M] in global memory: one float atomic per non-zero sum
__device__ __forceinline__ void sg_adjoint_flush(const double* __restrict__ acc, float* __restrict__ dtab, int M, int tid, int nthr) {
    for (int i = tid; i < 8 * M; i += nthr) {
        const float v = (float)acc[i];
        if (v != 0.f) unsafeAtomicAdd(&dtab[i], v);
    }
}

// The pull-back of lobe m: the table-space sums dtab[8 m ..] = {G.xyz, d|lambda|, d|mu|.rgb, -} to the raw row out[7 m ..]:
// a = xi / |xi|  =>  dxi = |lambda| (G - a (a.G)) / |xi|;  |.|  =>  the sign of the raw value, sign(0) = 0 as for torch's abs
__device__ __forceinline__ void sg_pullback(const float* __restrict__ lobes, const float4* __restrict__ tab, const float* __restrict__ dtab, int m,
                                            float* __restrict__ out) {
    auto sgn = [](float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); };
    const float4 al = tab[2 * m], mu = tab[2 * m + 1];
    const float* g = dtab + 8 * m;
    const float* l = lobes + 7 * m;
    const float ag = al.x * g[0] + al.y * g[1] + al.z * g[2];
    const float sc = al.w * mu.w;   // |lambda| / |xi|
    float* o = out + 7 * m;
    o[0] = sc * (g[0] - al.x * ag); o[1] = sc * (g[1] - al.y * ag); o[2] = sc * (g[2] - al.z * ag);
    o[3] = sgn(l[3]) * g[3];
    o[4] = sgn(l[4]) * g[4]; o[5] = sgn(l[5]) * g[5]; o[6] = sgn(l[6]) * g[6];
}
#endif

int report_error(int code, const char* fmt, ...);   // api.hip: records the per-thread message behind svgir_last_error, returns `code`

// what every entry point asks of a svgir_sg_light, before any HIP call
inline int sg_light_valid(const svgir_sg_light* l, const char* who) {
    if (!l) return report_error(SVGIR_ERR_INVALID, "%s: light is NULL", who);
    if (l->count < 1 || l->count > SVGIR_SG_MAX_LOBES)
        return report_error(SVGIR_ERR_INVALID, "%s: light.count = %d, 1 ... %d lobes", who, l->count, SVGIR_SG_MAX_LOBES);
    if (!l->lobes || !l->work) return report_error(SVGIR_ERR_INVALID, "%s: light.lobes / light.work is NULL", who);
    if ((uintptr_t)l->work & 15) return report_error(SVGIR_ERR_INVALID, "%s: light.work must be 16-byte aligned (read as float4)", who);
    return 0;
}

}  // namespace svgir
