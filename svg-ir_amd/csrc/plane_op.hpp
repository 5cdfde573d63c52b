// svg-ir_amd/csrc/plane_op.hpp -- the PLANE OPERAND of include/svgir_raster.h composed on load, shared by csrc/view_metrics.hip and
// csrc/lpips.hip (device code only).
#pragma once
#include "common.hpp"
#include "srgb.hpp"

namespace svgir {

// element i of channel c of a plane operand; N = H W.  No contraction: plain operators under the pragma (__fmul_rn / __fadd_rn are
// operators in a header to the compiler and are fused like any other, csrc/knn.hip); srgb() keeps the arithmetic it has everywhere else.  SRGB = false: for callers
// that have refused sRGB operands on the host (no powf in their code)
template <bool SRGB = true>
__device__ __forceinline__ float compose(const svgir_plane_op& p, int c, size_t N, size_t i) {
#pragma clang fp contract(off)
    float x = p.src[(size_t)c * N + i];
    if (p.scale != 1.f || p.offset != 0.f) x = (x * p.scale) + p.offset;
    if (p.mask) {
        const float m = p.mask[i];
        const float f = p.fill ? p.fill[(size_t)c * N + i] : p.bg[c];
        x = (x * m) + ((1.f - m) * f);
    }
    if (SRGB && p.srgb) x = srgb(x);
    return x;
}

// what every entry point that takes plane operands refuses before its first launch
inline const char* check_op(const svgir_plane_op& p) {
    if (!p.src) return "an operand has no src";
    if (p.fill && !p.mask) return "an operand has a fill plane but no mask";
    return nullptr;
}

}  // namespace svgir
