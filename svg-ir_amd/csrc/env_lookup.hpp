// svg-ir_amd/csrc/env_lookup.hpp -- the lat-long environment lookup shared by the shading kernels (csrc/shade.hip) and the eval view's
// environment backdrop (csrc/backdrop.hip): the normalisation, the four bilinear taps of a direction, and (shade_tables.hpp) the
// f(env) float4 table both read.  One definition: a surfel's incident light and the backdrop behind it come from the same arithmetic.
#pragma once
#include "common.hpp"
#include "shade_tables.hpp"

namespace svgir {

#if defined(__HIPCC__)
constexpr float kEnvInvPi = 0.31830988618379067154f;

#ifndef SHADE_PRECISE
#define SHADE_PRECISE 2
#endif
// 1 / max(sqrt(x2), 1e-12) for the normalisations.  At the glossy end of the reference's roughness range (0.09: alpha^2 = 6.6e-5) the GGX
// denominator N.H^2 (alpha^2 - 1) + 1 amplifies an error of N.H 15 000 times, so the unit vectors must be as good as the reference's
// (torch: correctly rounded sqrt and division): the hardware's 1-ulp rsq gets one Newton step.
__device__ __forceinline__ float inv_norm(float x2) {
    const float y = fminf(__builtin_amdgcn_rsqf(x2), 1e12f);
#if SHADE_PRECISE >= 1
    return x2 > 1e-24f ? y * fmaf(-0.5f * x2 * y, y, 1.5f) : y;
#else
    return y;
#endif
}

// (the f(env) table -- one float4 per texel {f(r), f(g), f(b), 0}: a bilinear tap is ONE 16-byte gather instead of three dwords -- is
// built by shade_table_entry, shade_tables.hpp)

// Lat-long bilinear lookup (grid_sample, align_corners=True, zero padding) of direction d.
struct EnvTap { int idx[4]; float w[4]; };
__device__ __forceinline__ void env_taps(const float* d, int He, int We, EnvTap& t) {
    const float phi = acosf(d[2]) - 1e-6f;
    const float theta = atan2f(d[1], d[0]);
    const float gy = phi * (2.f * kEnvInvPi) - 1.f;
    const float gx = -theta * kEnvInvPi;
    const float x = (gx + 1.f) * 0.5f * (float)(We - 1);
    const float y = (gy + 1.f) * 0.5f * (float)(He - 1);
    const float x0f = floorf(x), y0f = floorf(y);
    const float fx = x - x0f, fy = y - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int xi = x0 + (j & 1), yi = y0 + (j >> 1);
        const bool ok = xi >= 0 && xi < We && yi >= 0 && yi < He;
        t.idx[j] = ok ? yi * We + xi : -1;   // texel index (the table holds one float4 per texel)
        t.w[j] = ((j & 1) ? fx : 1.f - fx) * ((j >> 1) ? fy : 1.f - fy);
    }
}
#endif

}  // namespace svgir
