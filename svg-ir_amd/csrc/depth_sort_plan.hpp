// svg-ir_amd/csrc/depth_sort_plan.hpp -- which of the two plans sorts a view's P depth keys, and the launch of the second one.
//
//   kLsd      stable 8-bit LSD passes over all P keys (binning.hip launch_radix_sort): 4, or 3 under a speculated common top byte
//   kBuckets  under a speculated top byte, for P <= DEPTH_BUCKET_MAX_P: ONE stable pass on bits 16..23 that carries the visible keys only
//             (a culled Gaussian emits nothing: where it would land is immaterial), then one workgroup per value of that digit finishes its
//             bucket -- a contiguous range -- on bits 0..15 inside LDS (launch_depth_bucket_sort).  ONE launch instead of six: the
//             producer of the keys, preprocess_kernel, already groups every row of DEPTH_ROW consecutive Gaussians by that digit
//             (DepthRows below), and the bucket's workgroup gathers its keys from the rows.
//
// The plan function is plain C++ (host tests compile this header with g++); the launch declarations need common.hpp and are only seen by
// the files that include that first.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace svgir {

enum class DepthSortPlan { kLsd = 0, kBuckets = 1 };

constexpr int DEPTH_BUCKET_MAX_P = 1 << 19;   // above: a bucket of the one 8-bit pass no longer fits a workgroup (cfg5: 48 812 of 2 M keys)
constexpr int DEPTH_BUCKET_CAP = 8192;        // keys a workgroup sorts inside LDS (144 KiB of the CU's 160); also the chunk of the oversize path
constexpr int DEPTH_BUCKET_CAP_MIN = 64;
// Gaussians per row = threads of a preprocess workgroup under the bucket plan.  One row-table row per 1024 Gaussians is what the LSD
// passes' tables hold (common.hpp sort_blocks): the rows' tables take their place.  The bucket kernel scans a column with one row per thread.
constexpr int DEPTH_ROW = 1024;
constexpr int DEPTH_ROWS_MAX = DEPTH_BUCKET_MAX_P / DEPTH_ROW;
inline int depth_rows(int P) { return (P + DEPTH_ROW - 1) / DEPTH_ROW; }

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

// What preprocess_kernel leaves for the bucket kernel.  Row b = Gaussians [b DEPTH_ROW, (b + 1) DEPTH_ROW) and the same range of the three
// arrays: its V_b visible ones -- tile count != 0 -- stably grouped by digit d = key bits 16..23, {key, id, tile count}; behind them, in
// id[] alone, its other ids by index.  Per row and digit the exclusive prefix over the digits of the row's counts and of its tile counts,
// and per row {V_b, sum of its tile counts}.  Every entry of a row is written by the row's workgroup: nothing is zeroed, no atomics.
struct DepthRows {
    uint32_t *key, *id, *w;   // [n]
    uint32_t* cscan;          // [rows][256]
    uint32_t* wscan;          // [rows][256]
    uint32_t* tot;            // [rows][2]
};

#if defined(__HIPCC__)
// launch_preprocess (common.hpp) under this plan: workgroups of DEPTH_ROW Gaussians, each leaves its row in `rows` and writes neither
// a.key nor a.idx; a.zero_words is not cleared (the plan has no group totals).
void launch_preprocess_rows(const PreArgs& a, const DepthRows& rows, bool svgss, hipStream_t s);
// The kBuckets plan over the n Gaussians whose rows `rows` holds, keys of equal top byte among the visible ones.  Result: val1[0 .. V) = the
// V visible ids, stable by the low 24 key bits; w.offsets[0 .. V) = the exclusive prefix of their tile counts; val1[V .. n) = the other ids
// by index (val1 is a permutation of 0 .. n-1: the fused shading walks its back), offsets at and behind V are unspecified.  Publishes what
// the weighted LSD pass publishes (common.hpp RadixWeights), with counters[3] = V; of `w` the tiles (oversize buckets), the counters, the
// key summaries and the host words are used.  key1[n] is scratch (oversize buckets); none of the rows' arrays may be key1, val1 or
// w.offsets.  cap: depth_bucket_cap().
void launch_depth_bucket_sort(const DepthRows& rows, uint32_t* key1, uint32_t* val1, int n, int cap, hipStream_t s, const RadixWeights& w);
#endif

}  // namespace svgir
