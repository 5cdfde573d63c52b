// svg-ir_amd/csrc/geom_bwd.hpp -- the per-Gaussian backward with the forward's blend weights (geom_bwd.hip).
#pragma once
#include "common.hpp"

namespace svgir {

// launch_geom_bwd (common.hpp) with `weights` = the forward's out_weights [P], or nullptr.  Without a list (a.list == nullptr) a Gaussian
// is then processed only if its weight is positive -- some pixel blended it; every other Gaussian has exactly-zero composite gradients
// and keeps its cleared outputs -- instead of if radii > 0.  With a list, or without weights: launch_geom_bwd.
void launch_geom_bwd_blended(const GeomBwdArgs& a, const float* weights, hipStream_t s);

}  // namespace svgir
