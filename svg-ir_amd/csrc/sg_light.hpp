// svg-ir_amd/csrc/sg_light.hpp -- the lobe arithmetic of the spherical-Gaussian direct light (scene/direct_light_sg.py:
// render_envmap_sg / DirectLightSG.direct_light), shared by the prepared-table prologue, svgir_sg_eval and the SG instantiations of the
// shading kernels (csrc/shade.hip).
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
#endif

}  // namespace svgir
