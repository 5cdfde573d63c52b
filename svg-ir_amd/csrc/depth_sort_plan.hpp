// svg-ir_amd/csrc/depth_sort_plan.hpp -- which of the two plans sorts a view's P depth keys, and the launch of the second one.
//
//   kLsd      stable 8-bit LSD passes over all P keys (binning.hip launch_radix_sort): 4, or 3 under a speculated common top byte
//   kBuckets  under a speculated top byte, for P <= DEPTH_BUCKET_MAX_P: ONE stable pass on bits 16..23 that carries the visible keys only
//             (a culled Gaussian emits nothing: where it would land is immaterial), then one workgroup per value of that digit finishes its
//             bucket -- a contiguous range -- on bits 0..15 inside LDS (launch_depth_bucket_sort).  Three launches instead of six.
//
// The plan function is plain C++ (host tests compile this header with g++); the launch declaration needs common.hpp and is only seen by
// the files that include that first.
#pragma once
#include <cstdlib>
#include <cstring>

namespace svgir {

enum class DepthSortPlan { kLsd = 0, kBuckets = 1 };

constexpr int DEPTH_BUCKET_MAX_P = 1 << 19;   // above: a bucket of the one 8-bit pass no longer fits a workgroup (cfg5: 48 812 of 2 M keys)
constexpr int DEPTH_BUCKET_CAP = 8192;        // keys a workgroup sorts inside LDS (144 KiB of the CU's 160); also the chunk of the oversize path
constexpr int DEPTH_BUCKET_CAP_MIN = 64;

// SVGIR_DEPTH_SORT=lsd forces the LSD plan (A/B runs, forced-path tests); anything else, or unset: the plan function decides
inline bool depth_sort_forced_lsd(const char* env) { return env && std::strcmp(env, "lsd") == 0; }
// SVGIR_DEPTH_BUCKET_CAP=<n> LOWERS the in-LDS capacity (tests reach the oversize paths with a few hundred keys); out of range: clamped
inline int depth_bucket_cap(const char* env) {
    if (!env || !env[0]) return DEPTH_BUCKET_CAP;
    const long v = std::strtol(env, nullptr, 10);
    return v < DEPTH_BUCKET_CAP_MIN ? DEPTH_BUCKET_CAP_MIN : (v > DEPTH_BUCKET_CAP ? DEPTH_BUCKET_CAP : (int)v);
}

// spec_top: the speculated common top byte of the visible depth keys, -1: none
inline DepthSortPlan depth_sort_plan(int P, int spec_top, bool forced_lsd) {
    return (!forced_lsd && spec_top >= 0 && P > 0 && P <= DEPTH_BUCKET_MAX_P) ? DepthSortPlan::kBuckets : DepthSortPlan::kLsd;
}

#if defined(__HIPCC__)
// The kBuckets plan over the n (key, value) pairs in slot 0 of the ping/pong buffers, keys of equal top byte among the pairs that weigh
// something (w.tiles[2 value] != 0).  Result: val[1][0 .. V) = the V weighing values, stable by the low 24 key bits; w.offsets[0 .. V) = the
// exclusive prefix of their weights; val[1][V .. n) = the other values in input order (val[1] is a permutation of the input values: the fused
// shading walks its back), offsets at and behind V are unspecified.  Publishes what the weighted LSD pass publishes (common.hpp
// RadixWeights), with counters[3] = V; w.wtable is not used.  `table` as for launch_radix_sort (group totals zero on entry); slot 0 of the
// buffers is scratch afterwards.  cap: depth_bucket_cap().
void launch_depth_bucket_sort(uint32_t* const key[2], uint32_t* const val[2], int n, uint32_t* table, int cap, hipStream_t s, const RadixWeights& w);
#endif

}  // namespace svgir
