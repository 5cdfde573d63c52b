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

// Lat-long bilinear lookup (grid_sample, align_corners=True, zero padding) of direction d.  ONE definition of the grid, the range check
// and the tap order for every coordinate type T: float is what the shading kernels and the backdrop use (the reference's fp32 lines);
// double is the fused radiance loss's (csrc/irradiance.hip), whose texel gradients need weights that are good relative to themselves.
// The weights leave as fp32 either way.
struct EnvTap { int idx[4]; float w[4]; };
template <class T> struct EnvCoord;
template <> struct EnvCoord<float> {
    static __device__ __forceinline__ float acos_(float x) { return acosf(x); }
    static __device__ __forceinline__ float atan2_(float y, float x) { return atan2f(y, x); }
    static __device__ __forceinline__ float floor_(float x) { return floorf(x); }
    static __device__ __forceinline__ float eps() { return 1e-6f; }
    static __device__ __forceinline__ float inv_pi() { return kEnvInvPi; }
};
template <> struct EnvCoord<double> {
    static __device__ __forceinline__ double acos_(double x) { return acos(x); }
    static __device__ __forceinline__ double atan2_(double y, double x) { return atan2(y, x); }
    static __device__ __forceinline__ double floor_(double x) { return floor(x); }
    static __device__ __forceinline__ double eps() { return 1e-6; }
    static __device__ __forceinline__ double inv_pi() { return 0.31830988618379067154; }
};
template <class T>
__device__ __forceinline__ void env_taps(const T* d, int He, int We, EnvTap& t) {
    using C = EnvCoord<T>;
    const T phi = C::acos_(d[2]) - C::eps();
    const T theta = C::atan2_(d[1], d[0]);
    const T gy = phi * (T(2) * C::inv_pi()) - T(1);
    const T gx = -theta * C::inv_pi();
    const T x = (gx + T(1)) * T(0.5) * (T)(We - 1);
    const T y = (gy + T(1)) * T(0.5) * (T)(He - 1);
    const T x0f = C::floor_(x), y0f = C::floor_(y);
    const T fx = x - x0f, fy = y - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int xi = x0 + (j & 1), yi = y0 + (j >> 1);
        const bool ok = xi >= 0 && xi < We && yi >= 0 && yi < He;
        t.idx[j] = ok ? yi * We + xi : -1;   // texel index (the table holds one float4 per texel)
        t.w[j] = (float)(((j & 1) ? fx : T(1) - fx) * ((j >> 1) ? fy : T(1) - fy));
    }
}
#endif

}  // namespace svgir
