// svg-ir_amd/csrc/binning.hip -- tile binning: depth sort (its last pass also yields the instance offsets), key emit, tile sort, tile ranges.
//
// Replaces cub::DeviceScan::InclusiveSum (rasterizer_impl.cu:307), duplicateWithKeys (:70-111),
// cub::DeviceRadixSort::SortPairs on 64-bit (tile|depth) keys (:333-338) and identifyTileRanges (:116-138).
//
// MI355X-first re-design (same result, ~1/4 of the sort traffic):
//   the reference sorts R (Gaussian,tile) instances by a 64-bit key in 6 radix passes.  Here the P Gaussians
//   are sorted ONCE by their 32-bit depth key (stable, ties by ascending id), instances are emitted in that
//   order, and the R instances are then stably sorted by the tile id alone (ceil(log2 T) bits => 2 passes of
//   6-7 bits at 800x800 / 1600x1600).  A stable sort by tile of a depth-ordered list is exactly the
//   (tile, depth, id) order the reference's stable 64-bit sort produces (quirk Q12).
//
// The radix pass is a hand-written stable LSD pass of TWO kernels: per-block digit histogram (+ per-group-of-32-blocks
// digit totals) -> stable scatter.  The scatter block derives its own output cursors from the group totals and the
// <= 31 histogram rows of the preceding blocks of its group (a two-level prefix, ~50 coalesced 1 KB row reads per
// block), so no separate scan kernel sits between the two; the in-wave rank uses wave-level digit matching (ballots).
#include <algorithm>
#include <cassert>

#include "common.hpp"
#include "depth_sort_plan.hpp"

namespace svgir {

namespace {

// ---- radix pass --------------------------------------------------------------------------------------------
// Digit table layout: table[block][256] counts; gtot[group][256] = counts summed over the GS blocks of a group.
constexpr int GS = 32;

// fold of two depth-key summaries {AND << 8 | OR} (identity 0xff00)
__device__ __forceinline__ uint32_t key_top_fold(uint32_t a, uint32_t b) { return (a & b & 0xff00u) | ((a | b) & 0xffu); }

// The WEIGHTED form of a pass (W = true: the last pass of the geometry depth sort, launch_radix_sort's `weights`) sums, next to every
// count of keys, the weights of those keys -- value g weighs tiles[2 g] -- in a second table row per block (wtable), a second set of
// group totals (wgtot) and a second, weighted rank inside the block: the exclusive prefix of the weights in sorted order (the instance
// offsets) falls out of the same arithmetic as the output position.  Integer sums: the result does not depend on any order.
struct WeightArgs {
    const uint32_t* vals;   // the pass's input values (the histogram kernel gathers through them)
    uint32_t* wgtot;        // [groups][256], zero on entry
    RadixWeights w;
};

template <int ITEMS, bool W = false>
__global__ void __launch_bounds__(BLOCK) radix_hist_kernel(const uint32_t* __restrict__ keys, int n_cap,
                                                           const uint32_t* __restrict__ n_dev, int bit_lo,
                                                           uint32_t mask, uint32_t* __restrict__ table,
                                                           uint32_t* __restrict__ gtot, WeightArgs wa) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t whist[W ? 256 : 1];   // W: sum of the weights per digit
    // element count: launch-time bound n_cap, or -- when the count is still being computed on the device at launch
    // time (speculative launch before the host has read it) -- the device-side value clamped to that bound
    const int n = n_dev ? (int)min((uint32_t)n_cap, n_dev[0]) : n_cap;
    hist[threadIdx.x] = 0;
    if constexpr (W) whist[threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * (BLOCK * ITEMS);
    uint32_t k[ITEMS];   // all loads first (clamped index), then the LDS atomics: one memory latency, not ITEMS
#pragma unroll
    for (int i = 0; i < ITEMS; i++) k[i] = keys[max(0, min(base + i * BLOCK + (int)threadIdx.x, n - 1))];
    uint32_t w[W ? ITEMS : 1];   // W: the keys' weights -- the values, then ONE round of gathers through them (a second latency, not ITEMS)
    if constexpr (W) {
        uint32_t g[ITEMS];
#pragma unroll
        for (int i = 0; i < ITEMS; i++) g[i] = wa.vals[max(0, min(base + i * BLOCK + (int)threadIdx.x, n - 1))];
#pragma unroll
        for (int i = 0; i < ITEMS; i++) w[i] = wa.w.tiles[2 * (size_t)g[i]];   // (common.hpp GeomLayout::tiles: {count, rectangle})
    }
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const int e = base + i * BLOCK + threadIdx.x;
        if (e < n) atomicAdd(&hist[(k[i] >> bit_lo) & mask], 1u);
        if constexpr (W) if (e < n && w[i] != 0u) atomicAdd(&whist[(k[i] >> bit_lo) & mask], w[i]);
    }
    __syncthreads();
    const uint32_t c = hist[threadIdx.x];
    table[(size_t)blockIdx.x * 256 + threadIdx.x] = c;
    if (c) atomicAdd(&gtot[(size_t)(blockIdx.x / GS) * 256 + threadIdx.x], c);
    if constexpr (W) {   // the same row and the same group slot once more, for the weights
        const uint32_t wc = whist[threadIdx.x];
        wa.w.wtable[(size_t)blockIdx.x * 256 + threadIdx.x] = wc;
        if (wc) atomicAdd(&wa.wgtot[(size_t)(blockIdx.x / GS) * 256 + threadIdx.x], wc);
    }
}

template <int ITEMS, bool W = false>
__global__ void __launch_bounds__(BLOCK) radix_scatter_kernel(const uint32_t* __restrict__ kin,
                                                              const uint32_t* __restrict__ vin,
                                                              uint32_t* __restrict__ kout, uint32_t* __restrict__ vout,
                                                              int n_cap, const uint32_t* __restrict__ n_dev, int bit_lo, int nbits,
                                                              const uint32_t* __restrict__ table,
                                                              const uint32_t* __restrict__ gtot, int ngroups, WeightArgs wa) {
    __shared__ uint32_t wcnt[4][256];   // per-wave digit counters, later the waves' output cursors
    __shared__ uint32_t wtot[4];
    __shared__ uint32_t wtot2[W ? 4 : 1], ksum[W ? 4 : 1], smax[W ? 4 : 1];   // W: a second scan's wave sums, key summaries, span
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t mask = (1u << nbits) - 1;
    const int n = n_dev ? (int)min((uint32_t)n_cap, n_dev[0]) : n_cap;
    // wave w owns the w-th quarter of the block's keys (consecutive keys: round-major, lane-minor = key order)
    const int base = blockIdx.x * (BLOCK * ITEMS) + wave * (64 * ITEMS);
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    // all loads of the block up front
    uint32_t ks[ITEMS], vs[ITEMS], rk[ITEMS];
#pragma unroll
    for (int c = 0; c < ITEMS; c++) {
        const int e = base + c * 64 + lane;
        ks[c] = e < n ? kin[e] : 0u;
        vs[c] = e < n ? vin[e] : 0u;
    }
    uint32_t ws[W ? ITEMS : 1];   // W: the keys' weights, one round of gathers through the values (in flight during the cursor sums)
    if constexpr (W) {
#pragma unroll
        for (int c = 0; c < ITEMS; c++) ws[c] = base + c * 64 + lane < n ? wa.w.tiles[2 * (size_t)vs[c]] : 0u;
        if (blockIdx.x == 0) {   // the publishing block folds the preprocess waves' depth-key summaries {AND << 8 | OR}
            uint32_t kv = 0xff00u;
#pragma unroll 8
            for (int j = t; j < wa.w.n_key_top; j += BLOCK) kv = key_top_fold(kv, wa.w.key_top[j]);
            kv = wave_reduce(kv, key_top_fold);
            if (lane == 0) ksum[wave] = kv;   // (read behind the barrier of the cursor scan)
        }
    }
#pragma unroll
    for (int w = 0; w < 4; w++) wcnt[w][t] = 0;
    // Output cursor of digit t for this block:
    //   sum_{d < t} total[d]  +  sum_{groups before mine} gtot[g][t]  +  sum_{blocks before me in my group} table[b][t]
    uint32_t cursor;
    uint32_t wcursor = 0;   // W: the same three sums over the weights = the instance offset of the block's first key of digit t
    {
        const int g = blockIdx.x / GS;
        uint32_t tot = 0, pre = 0, wsum = 0, wpre = 0;
#pragma unroll 8
        for (int gg = 0; gg < ngroups; gg++) {
            const uint32_t v = gtot[(size_t)gg * 256 + t];
            tot += v;
            pre += gg < g ? v : 0u;
            if constexpr (W) {
                const uint32_t wv = wa.wgtot[(size_t)gg * 256 + t];
                wsum += wv;
                wpre += gg < g ? wv : 0u;
            }
        }
#pragma unroll 8
        for (int b = g * GS; b < (int)blockIdx.x; b++) {
            pre += table[(size_t)b * 256 + t];
            if constexpr (W) wpre += wa.w.wtable[(size_t)b * 256 + t];
        }
        cursor = block_excl_scan<4>(tot, wtot) + pre;   // (its barrier also: the wave counters are zero)
        if constexpr (W) {
            uint32_t R;   // the sum of all weights: every block has it, the first one publishes it -- as early as the count can be known
            wcursor = block_excl_scan<4>(wsum, wtot2, &R) + wpre;
            if (blockIdx.x == 0 && t == 0) {
                const uint32_t summary = key_top_fold(key_top_fold(ksum[0], ksum[1]), key_top_fold(ksum[2], ksum[3]));
                wa.w.counters[0] = R;
                wa.w.counters[2] = summary;
                // the host's copy: tagged 8-byte stores into pinned host memory -- no copy operation and no event on the stream; the host
                // recognises the values of THIS forward by the tag (api.hip): {R} and {prefilter violation << 16 | summary}
                if (wa.w.host_out) {
                    const uint32_t viol = wa.w.violation ? (wa.w.violation[0] != 0u ? 1u : 0u) : 0u;
                    __hip_atomic_store(wa.w.host_out, ((unsigned long long)wa.w.host_tag << 32) | R, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(wa.w.host_out + 1, ((unsigned long long)wa.w.host_tag << 32) | (viol << 16) | summary, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        }
    }
    // rank of every key among the keys of its WAVE with the same digit: wave-level digit matching (ballots) against a
    // wave-private digit counter in LDS -- no workgroup barrier inside the ranking
#pragma unroll
    for (int c = 0; c < ITEMS; c++) {
        const bool valid = base + c * 64 + lane < n;
        const uint32_t d = (ks[c] >> bit_lo) & mask;
        const unsigned long long same = wave_match(d, nbits, valid);
        const uint32_t in_round = (uint32_t)__popcll(same & lt_mask);
        const uint32_t prior = wcnt[wave][d];   // (the DS operations of a wave execute in order: every lane reads before the leader writes)
        rk[c] = prior + in_round;
        if (valid && in_round == 0) wcnt[wave][d] = prior + (uint32_t)__popcll(same);
    }
    __syncthreads();
    if constexpr (W) {
        // The block's values, weights and digits go through LDS in digit-then-key order (the staging order of the large variant below): ONE
        // exclusive scan over the staged weights ranks every key by weight among the block's keys of its digit, scan[lp] - scan[bstart[d]].
        __shared__ uint32_t sV[BLOCK * ITEMS];
        __shared__ __attribute__((aligned(16))) uint32_t sS[BLOCK * ITEMS];   // weights, then their exclusive scan
        __shared__ uint8_t sD[BLOCK * ITEMS];
        __shared__ uint32_t bstart[256], gcur[256], wgcur[256];
        const uint32_t c0 = wcnt[0][t], c1 = wcnt[1][t], c2 = wcnt[2][t], c3 = wcnt[3][t];
        const uint32_t bs = block_excl_scan<4>(c0 + c1 + c2 + c3, wtot);   // (wtot was last read in front of the barrier above)
        bstart[t] = bs; gcur[t] = cursor; wgcur[t] = wcursor;
        wcnt[0][t] = bs; wcnt[1][t] = bs + c0; wcnt[2][t] = bs + c0 + c1; wcnt[3][t] = bs + c0 + c1 + c2;   // the waves' staging cursors
        __syncthreads();
        uint32_t span = 0;   // 1 + the last output position of a key of this thread with a non-zero weight
#pragma unroll
        for (int c = 0; c < ITEMS; c++) {
            if (base + c * 64 + lane < n) {
                const uint32_t d = (ks[c] >> bit_lo) & mask;
                const uint32_t lp = wcnt[wave][d] + rk[c];
                sV[lp] = vs[c]; sS[lp] = ws[c]; sD[lp] = (uint8_t)d;
                if (ws[c] != 0u) span = max(span, gcur[d] + (lp - bstart[d]) + 1u);
            }
        }
        span = wave_reduce_max(span);
        if (lane == 0) smax[wave] = span;
        __syncthreads();
        const int nblk = min(BLOCK * ITEMS, n - (int)blockIdx.x * (BLOCK * ITEMS));
        // thread t scans the ITEMS consecutive staged weights t ITEMS .. (16-byte LDS accesses); slots behind the block's keys count 0
        uint32_t wv[ITEMS], sum = 0;
#pragma unroll
        for (int c = 0; c < ITEMS; c += 4) {
            const uint4 q = reinterpret_cast<const uint4*>(sS)[(t * ITEMS + c) >> 2];
            wv[c] = q.x; wv[c + 1] = q.y; wv[c + 2] = q.z; wv[c + 3] = q.w;
        }
#pragma unroll
        for (int c = 0; c < ITEMS; c++) { wv[c] = t * ITEMS + c < nblk ? wv[c] : 0u; sum += wv[c]; }
        // (every thread scans slots that only it reads and writes; wtot2 was last read far above.  The barrier that the scanned weights need
        // is the one in front of the output loop below)
        uint32_t run = block_excl_scan<4>(sum, wtot2);
#pragma unroll
        for (int c = 0; c < ITEMS; c += 4) {
            uint4 q;
            q.x = run; run += wv[c]; q.y = run; run += wv[c + 1]; q.z = run; run += wv[c + 2]; q.w = run; run += wv[c + 3];
            reinterpret_cast<uint4*>(sS)[(t * ITEMS + c) >> 2] = q;
        }
        // counters[3] = the visible span of the depth order: order[0 .. span) holds every Gaussian with tiles > 0 (they sort in front of the
        // culled ones) -- the working set of the fused shading (api.hip).  One atomic per block that holds a visible Gaussian.
        if (t == 0) {
            const uint32_t m = max(max(smax[0], smax[1]), max(smax[2], smax[3]));
            if (m != 0u) atomicMax(wa.w.counters + 3, m);
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < ITEMS; c++) {
            const int i = c * BLOCK + t;
            if (i < nblk) {
                const uint32_t d = sD[i], b = bstart[d];
                const uint32_t pos = gcur[d] + ((uint32_t)i - b);
                vout[pos] = sV[i];                                // (the sorted keys of the last pass have no reader: kout stays unwritten)
                wa.w.offsets[pos] = wgcur[d] + (sS[i] - sS[b]);
            }
        }
        return;
    }
    if (ITEMS >= 16) {
        // Large inputs (bandwidth, not launch latency, sets the time): the block's keys are first put in digit order in LDS, then
        // written out -- consecutive lanes write consecutive addresses of a digit's run (a block of 4096 keys holds runs of ~32 per 7-bit
        // digit) instead of 64 lanes writing to 64 different runs.
        __shared__ uint32_t sK[BLOCK * (ITEMS >= 16 ? ITEMS : 1)], sV[BLOCK * (ITEMS >= 16 ? ITEMS : 1)];
        __shared__ uint32_t bstart[256], gcur[256];
        const uint32_t c0 = wcnt[0][t], c1 = wcnt[1][t], c2 = wcnt[2][t], c3 = wcnt[3][t];
        const uint32_t bc = c0 + c1 + c2 + c3;            // keys of digit t in this block
        // first slot of digit t in the block's staging order (wtot was last read in front of the barrier above)
        const uint32_t bs = block_excl_scan<4>(bc, wtot);
        bstart[t] = bs; gcur[t] = cursor;
        wcnt[0][t] = bs; wcnt[1][t] = bs + c0; wcnt[2][t] = bs + c0 + c1; wcnt[3][t] = bs + c0 + c1 + c2;   // the waves' staging cursors
        __syncthreads();
#pragma unroll
        for (int c = 0; c < ITEMS; c++) {
            if (base + c * 64 + lane < n) {
                const uint32_t lp = wcnt[wave][(ks[c] >> bit_lo) & mask] + rk[c];
                sK[lp] = ks[c]; sV[lp] = vs[c];
            }
        }
        __syncthreads();
        const int nblk = min(BLOCK * ITEMS, n - (int)blockIdx.x * (BLOCK * ITEMS));
#pragma unroll
        for (int c = 0; c < ITEMS; c++) {
            const int i = c * BLOCK + t;
            if (i < nblk) {
                const uint32_t k = sK[i], d = (k >> bit_lo) & mask;
                const uint32_t pos = gcur[d] + ((uint32_t)i - bstart[d]);
                kout[pos] = k;
                vout[pos] = sV[i];
            }
        }
        return;
    }
    {   // digit t: the waves' cursors = block cursor + counts of the waves in front
        const uint32_t c0 = wcnt[0][t], c1 = wcnt[1][t], c2 = wcnt[2][t];
        __syncthreads();
        wcnt[0][t] = cursor; wcnt[1][t] = cursor + c0; wcnt[2][t] = cursor + c0 + c1; wcnt[3][t] = cursor + c0 + c1 + c2;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < ITEMS; c++) {
        if (base + c * 64 + lane < n) {
            const uint32_t pos = wcnt[wave][(ks[c] >> bit_lo) & mask] + rk[c];
            kout[pos] = ks[c];
            vout[pos] = vs[c];
        }
    }
}

// ---- bucket plan of the geometry depth sort (depth_sort_plan.hpp) -------------------------------------------------
// Under a speculated common top byte 24 key bits are left, and the culled Gaussians -- more than half of a closed surface's surfels -- emit
// nothing.  preprocess_kernel leaves every row of DEPTH_ROW consecutive Gaussians stably grouped by bits 16..23 of the visible keys
// (DepthRows).  Rows taken in index order are a stable pass on that digit: bucket d is, row by row, the rows' groups d.  One workgroup per
// bucket gathers it, finishes it on bits 0..15 inside LDS and scans the weights in final order: the instance offsets.  One launch instead
// of three passes of two.

constexpr int DB_THREADS = 1024, DB_WAVES = DB_THREADS / 64, DB_ROUNDS = DEPTH_BUCKET_CAP / DB_THREADS;

// One stable 8-bit counting pass of the whole workgroup (DB_THREADS threads, all of them) over m <= DEPTH_BUCKET_CAP items.  get(i) is
// item i = {sort word, payload}, its digit (word >> shift) & 255; put(pos, item) stores it.  Wave w ranks the w-th run of consecutive items
// (wave_match against wave-private counters, no workgroup barrier inside), thread d < 256 then turns the 16 counts of digit d into the
// waves' cursors.  CARRY = false: positions 0 .. m, the digit bases are the exclusive scan of this call's counts.  CARRY = true: the bases
// are cur[256], which the call advances -- a pass over a longer range, chunk by chunk in order (ties that straddle two chunks stay in
// order).  Ends with a barrier: the items are in place, every scratch array is free.
template <bool CARRY, class Get, class Put>
__device__ __forceinline__ void bucket_pass(int m, int shift, Get get, Put put, uint32_t (*wcnt)[256], uint32_t* cur, uint32_t* wsum) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int i = t; i < DB_WAVES * 256; i += DB_THREADS) (&wcnt[0][0])[i] = 0u;
    __syncthreads();
    const int per = ((m + DB_WAVES - 1) / DB_WAVES + 63) & ~63;   // (<= 64 DB_ROUNDS)
    const int base = wave * per;
    uint2 it[DB_ROUNDS];
    uint32_t rk[DB_ROUNDS];
#pragma unroll
    for (int r = 0; r < DB_ROUNDS; r++) {
        if (r * 64 < per) {   // (uniform over the workgroup)
            const int i = base + r * 64 + lane;
            const bool valid = i < m;
            it[r] = valid ? get(i) : make_uint2(0u, 0u);
            const uint32_t d = (it[r].x >> shift) & 255u;
            const unsigned long long same = wave_match(d, 8, valid);
            const uint32_t in_round = (uint32_t)__popcll(same & lt_mask);
            const uint32_t prior = wcnt[wave][d];   // (the DS operations of a wave execute in order: every lane reads before the leader writes)
            rk[r] = prior + in_round;
            if (valid && in_round == 0) wcnt[wave][d] = prior + (uint32_t)__popcll(same);
        }
    }
    __syncthreads();
    uint32_t c[DB_WAVES], total = 0;
#pragma unroll
    for (int q = 0; q < DB_WAVES; q++) { c[q] = t < 256 ? wcnt[q][t] : 0u; total += c[q]; }
    uint32_t run;
    if constexpr (CARRY) run = t < 256 ? cur[t] : 0u;
    else run = block_excl_scan<DB_WAVES>(total, wsum);
    if (t < 256) {   // (column t of the counters is this thread's alone until the barrier)
#pragma unroll
        for (int q = 0; q < DB_WAVES; q++) { wcnt[q][t] = run; run += c[q]; }
        if constexpr (CARRY) cur[t] = run;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < DB_ROUNDS; r++) {
        if (r * 64 < per) {
            const int i = base + r * 64 + lane;
            if (i < m) put(wcnt[wave][(it[r].x >> shift) & 255u] + rk[r], it[r]);
        }
    }
    __syncthreads();
}

// Workgroup d finishes bucket d: the visible keys whose bits 16..23 are d.  Column d of the row tables -- one row per thread -- gives, summed
// over the rows, the bucket's position `start` in the order, its size n and its weight base, and scanned over the rows where item j of the
// bucket lies: in the last row b with prefix[b] <= j, at the row's base + the row's scan[d] + (j - prefix[b]).
//   n <= cap: keys {low 16 bits | local index}, ids and weights gathered into LDS, two in-LDS passes, the weights scanned in final order, out.
//   n > cap, low 16 bits all equal: the gathered order is the order; the weights (gathered through the ids) are scanned chunk by chunk.
//   n > cap otherwise: the two passes run chunk by chunk through global memory -- out of the rows into the bucket's own range of two scratch
//     arrays, and from there into the order -- then that scan.
// Of the order, nothing outside [start, start + n) is touched: the buckets are disjoint.  Behind the V visible ids follow the rows' other
// ids, row b's run by workgroup b mod 256; workgroup 0 publishes R, V, the key summary and the host words (RadixWeights).
__device__ __forceinline__ int bucket_row_of(const uint32_t* prefix, int nrows, uint32_t j) {   // the last row b with prefix[b] <= j
    int lo = 0, hi = nrows;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(DB_THREADS) depth_bucket_sort_kernel(const DepthRows rows, int nrows, int P, uint32_t* key1, uint32_t* val1,
                                                                       uint32_t* offsets, int cap, const RadixWeights w) {
    __shared__ uint32_t sA[DEPTH_BUCKET_CAP], sB[DEPTH_BUCKET_CAP], sI[DEPTH_BUCKET_CAP], sW[DEPTH_BUCKET_CAP];
    __shared__ uint32_t wcnt[DB_WAVES][256];
    __shared__ uint32_t cur[256], wsum[DB_WAVES], wsum2[DB_WAVES], tot3[3][DB_WAVES], ksum[DB_WAVES], red[2][DB_WAVES];
    // the rows' prefixes live in sB, which is free until the first pass stores into it
    static_assert(3 * (DEPTH_ROWS_MAX + 1) <= DEPTH_BUCKET_CAP && DEPTH_ROWS_MAX <= DB_THREADS, "row prefixes: one row per thread, inside sB");
    static_assert(sizeof(uint32_t) * (4 * DEPTH_BUCKET_CAP + DB_WAVES * 256 + 256 + 8 * DB_WAVES) <= 160 * 1024, "LDS of one CU");
    uint32_t* const prefix = sB;                              // [nrows + 1] items of this bucket in the rows in front
    uint32_t* const rowsrc = sB + (DEPTH_ROWS_MAX + 1);       // [nrows] where item j of the row's share lies, minus j
    uint32_t* const vprefix = sB + 2 * (DEPTH_ROWS_MAX + 1);  // [nrows + 1] visible Gaussians in the rows in front
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t d = blockIdx.x;
    uint32_t c0 = 0, c1 = 0, w0 = 0;
    uint2 rt = make_uint2(0u, 0u);
    if (t < nrows) {
        rt = reinterpret_cast<const uint2*>(rows.tot)[t];
        c0 = rows.cscan[(size_t)t * 256 + d];
        c1 = d < 255u ? rows.cscan[(size_t)t * 256 + d + 1] : rt.x;
        w0 = rows.wscan[(size_t)t * 256 + d];
    }
    uint32_t kv = 0xff00u;
    if (d == 0u) {   // the publishing workgroup folds the preprocess waves' depth-key summaries {AND << 8 | OR}
#pragma unroll 4
        for (int j = t; j < w.n_key_top; j += DB_THREADS) kv = key_top_fold(kv, w.key_top[j]);
    }
    uint32_t n_u, V;
    const uint32_t pre = block_excl_scan<DB_WAVES>(c1 - c0, wsum, &n_u);
    const uint32_t vpre = block_excl_scan<DB_WAVES>(rt.x, wsum2, &V);
    {
        const uint32_t s0 = wave_reduce_add(c0), s1 = wave_reduce_add(w0), s2 = wave_reduce_add(rt.y);
        kv = wave_reduce(kv, key_top_fold);
        if (lane == 0) { tot3[0][wave] = s0; tot3[1][wave] = s1; tot3[2][wave] = s2; ksum[wave] = kv; }
    }
    if (t < nrows) { prefix[t] = pre; rowsrc[t] = (uint32_t)t * DEPTH_ROW + c0 - pre; vprefix[t] = vpre; }
    if (t == nrows) { prefix[t] = n_u; vprefix[t] = V; }
    if (t == 0 && nrows == DB_THREADS) { prefix[nrows] = n_u; vprefix[nrows] = V; }
    __syncthreads();
    uint32_t start = 0, wbase = 0, R = 0;
#pragma unroll
    for (int q = 0; q < DB_WAVES; q++) { start += tot3[0][q]; wbase += tot3[1][q]; R += tot3[2][q]; }
    const int n = (int)n_u;
    if (d == 0u && t == 0) {
        uint32_t summary = 0xff00u;
#pragma unroll
        for (int q = 0; q < DB_WAVES; q++) summary = key_top_fold(summary, ksum[q]);
        w.counters[0] = R;
        w.counters[2] = summary;
        w.counters[3] = V;
        if (w.host_out) {   // (tag format: radix_scatter_kernel)
            const uint32_t viol = w.violation ? (w.violation[0] != 0u ? 1u : 0u) : 0u;
            __hip_atomic_store(w.host_out, ((unsigned long long)w.host_tag << 32) | R, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(w.host_out + 1, ((unsigned long long)w.host_tag << 32) | (viol << 16) | summary, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    // (the ids without weight follow the visible ones, by index: val[1] stays a permutation of the ids, and the fused shading walks its
    // back to clear the rows of the surfels this view does not shade -- shade.hip zero_rest_rows)
    for (int b = (int)d; b < nrows; b += 256) {
        const uint32_t vb = vprefix[b], nv = vprefix[b + 1] - vb;
        const int len = min(DEPTH_ROW, P - b * DEPTH_ROW) - (int)nv;
        const uint32_t* src = rows.id + (size_t)b * DEPTH_ROW + nv;
        uint32_t* dst = val1 + V + ((uint32_t)b * DEPTH_ROW - vb);   // (every row in front of b is full)
        for (int i = t; i < len; i += DB_THREADS) dst[i] = src[i];
    }
    if (n == 0) return;
    if (n <= cap) {
        for (int i = t; i < n; i += DB_THREADS) {
            const uint32_t src = rowsrc[bucket_row_of(prefix, nrows, (uint32_t)i)] + (uint32_t)i;
            sA[i] = (rows.key[src] << 16) | (uint32_t)i;
            sI[i] = rows.id[src];
            sW[i] = rows.w[src];
        }
        // (the barrier behind the passes' clearing of the counters also orders these stores, and the reads of the prefixes in sB)
        bucket_pass<false>(n, 16, [&](int i) { return make_uint2(sA[i], 0u); }, [&](uint32_t pos, uint2 it) { sB[pos] = it.x; }, wcnt, cur, wsum);
        bucket_pass<false>(n, 24, [&](int i) { return make_uint2(sB[i], 0u); }, [&](uint32_t pos, uint2 it) { sA[pos] = it.x; }, wcnt, cur, wsum);
        // the weights in final order, DB_ROUNDS consecutive ones per thread, and their exclusive scan (into sB)
        uint32_t wv[DB_ROUNDS], sum = 0;
#pragma unroll
        for (int j = 0; j < DB_ROUNDS; j++) {
            const int i = t * DB_ROUNDS + j;
            wv[j] = i < n ? sW[sA[i] & 0xffffu] : 0u;
            sum += wv[j];
        }
        uint32_t run = block_excl_scan<DB_WAVES>(sum, wsum2);
#pragma unroll
        for (int j = 0; j < DB_ROUNDS; j++) {
            const int i = t * DB_ROUNDS + j;
            if (i < n) sB[i] = run;
            run += wv[j];
        }
        __syncthreads();
        for (int i = t; i < n; i += DB_THREADS) {
            val1[start + i] = sI[sA[i] & 0xffffu];
            offsets[start + i] = wbase + sB[i];
        }
        return;
    }
    // oversize.  (The rows' arrays are read-only here -- other workgroups gather from them -- so the passes' intermediate lives in the
    // bucket's own range of two arrays that hold nothing before this workgroup's last stores: the offsets and the keys of slot 1.)
    const auto item = [&](int i) {
        const uint32_t src = rowsrc[bucket_row_of(prefix, nrows, (uint32_t)i)] + (uint32_t)i;
        return make_uint2(rows.key[src], rows.id[src]);
    };
    {   // do the low 16 bits differ at all?
        uint32_t a = 0xffffu, o = 0u;
        for (int i = t; i < n; i += DB_THREADS) { const uint32_t k = item(i).x & 0xffffu; a &= k; o |= k; }
        a = wave_reduce(a, [](uint32_t x, uint32_t y) { return x & y; });
        o = wave_reduce(o, [](uint32_t x, uint32_t y) { return x | y; });
        if (lane == 0) { red[0][wave] = a; red[1][wave] = o; }
        __syncthreads();
        a = 0xffffu; o = 0u;
#pragma unroll
        for (int q = 0; q < DB_WAVES; q++) { a &= red[0][q]; o |= red[1][q]; }
        if (a == o) {   // the gathered order is the order
            for (int i = t; i < n; i += DB_THREADS) val1[start + i] = item(i).y;
        } else {
            uint32_t* const tk = offsets + start;
            uint32_t* const tv = key1 + start;
            for (int pass = 0; pass < 2; pass++) {   // rows -> {tk, tv} on bits 0..7, {tk, tv} -> the ids of slot 1 on bits 8..15
                const int shift = 8 * pass;
                if (t < 256) cur[t] = 0u;
                __syncthreads();
                for (int i = t; i < n; i += DB_THREADS) atomicAdd(&cur[((pass ? tk[i] : item(i).x) >> shift) & 255u], 1u);
                __syncthreads();
                const uint32_t ex = block_excl_scan<DB_WAVES>(t < 256 ? cur[t] : 0u, wsum);
                if (t < 256) cur[t] = ex;   // (read behind the first barrier of the pass below)
                for (int c0 = 0; c0 < n; c0 += cap) {
                    if (pass == 0)
                        bucket_pass<true>(min(cap, n - c0), shift, [&](int i) { return item(c0 + i); },
                                          [&](uint32_t pos, uint2 it) { tk[pos] = it.x; tv[pos] = it.y; }, wcnt, cur, wsum);
                    else
                        bucket_pass<true>(min(cap, n - c0), shift, [&](int i) { return make_uint2(tk[c0 + i], tv[c0 + i]); },
                                          [&](uint32_t pos, uint2 it) { val1[start + pos] = it.y; }, wcnt, cur, wsum);
                }
                __threadfence_block();   // (the next pass, and the scan below, read what other waves of this workgroup stored)
                __syncthreads();
            }
        }
        __threadfence_block();
        __syncthreads();
    }
    uint32_t carry = wbase;
    for (int c0 = 0; c0 < n; c0 += DB_THREADS * DB_ROUNDS) {
        uint32_t wv[DB_ROUNDS], sum = 0;
#pragma unroll
        for (int j = 0; j < DB_ROUNDS; j++) {
            const int i = c0 + t * DB_ROUNDS + j;
            wv[j] = i < n ? w.tiles[2 * (size_t)val1[start + i]] : 0u;
            sum += wv[j];
        }
        uint32_t all;
        uint32_t run = carry + block_excl_scan<DB_WAVES>(sum, wsum, &all);
#pragma unroll
        for (int j = 0; j < DB_ROUNDS; j++) {
            const int i = c0 + t * DB_ROUNDS + j;
            if (i < n) offsets[start + i] = run;
            run += wv[j];
        }
        carry += all;
        __syncthreads();   // (wsum is free again)
    }
}

// ---- single-pass tile sort (T <= 4096 tiles) ----------------------------------------------------------------------
// The tile id has <= 12 bits at 800 x 800 and below: instead of two 6-bit radix passes (four launches) + a ranges kernel, ONE stable
// counting sort over the whole id -- (1) per-workgroup histograms of TS12K keys over the tile ids (LDS atomics), (2) per tile
// the exclusive prefix over the workgroups and the tile's total, (3) scatter: every workgroup scans the totals itself (tile bases = the
// tiles' RANGES: workgroup 0 writes them out, identifyTileRanges for free), adds its row of prefixes, ranks its keys stably (wave-level
// matching on the 12 bits against wave-private 16-bit LDS counters) and writes the values -- not the sorted tile ids: nothing reads them.
// Rows hold nbins = T rounded up to the workgroup size counters.
// A workgroup = 512 threads and 4096 keys: half the table rows of 256 x 2048 (cfg2: 165 rows of 2560 counters; column scan 7.3 -> 5.2 us,
// histogram 5.2 -> 5.0, scatter unchanged: profiles/tile_bin_ab.txt); -DTS12_THREADS_V=256 builds the smaller one for A/B runs.
// The launches are sized by an instance CAPACITY (api.hip: a speculative one lies 12.5 % above the count): every kernel bounds its work
// by the key blocks of the count it reads on the device -- no histogram row for a block without keys, the column scan walks the written
// rows only, a scatter workgroup without keys returns (workgroup 0 still writes every range).
#ifndef TS12_THREADS_V
#define TS12_THREADS_V 512
#endif
constexpr int TS12T = TS12_THREADS_V, TS12W = TS12T / 64, TS12K = 8 * TS12T;   // threads, waves and keys of a workgroup
static_assert(TS12K >= TS12_KEYS && TS12_BINS % TS12T == 0, "common.hpp tile12_table_words sizes the table for rows of TS12_KEYS keys");
__host__ __device__ constexpr int ts12_blocks(int n) { return (n + TS12K - 1) / TS12K; }   // key blocks that hold keys
__global__ void __launch_bounds__(TS12T) ts12_hist_kernel(const uint32_t* __restrict__ keys, int n_cap, const uint32_t* __restrict__ n_dev,
                                                          uint32_t* __restrict__ table, int nbins) {
    __shared__ uint32_t hist[TS12_BINS];
    const int n = n_dev ? (int)min((uint32_t)n_cap, n_dev[0]) : n_cap;
    if ((int)blockIdx.x >= ts12_blocks(n)) return;   // (a launch sized by a capacity: no row for a block without keys)
    const int t = threadIdx.x;
    for (int i = t; i < nbins; i += TS12T) hist[i] = 0u;
    __syncthreads();
    const int base = blockIdx.x * TS12K;
    uint32_t k[TS12K / TS12T];
#pragma unroll
    for (int i = 0; i < TS12K / TS12T; i++) k[i] = keys[max(0, min(base + i * TS12T + t, n - 1))];
#pragma unroll
    for (int i = 0; i < TS12K / TS12T; i++)
        if (base + i * TS12T + t < n) atomicAdd(&hist[k[i] & (TS12_BINS - 1)], 1u);
    __syncthreads();
    uint32_t* row = table + (size_t)blockIdx.x * nbins;
    for (int i = t; i < nbins; i += TS12T) row[i] = hist[i];
}

// per tile id: exclusive prefix of the workgroups' counts (in place) and the total.  A workgroup = 16 tile ids x 16 row segments: a thread
// first sums its segment (loads only: all in flight together), the 16 segment sums of a tile meet in LDS, then the thread rewrites its
// segment as running prefixes -- two short memory round trips instead of one per row.
__global__ void __launch_bounds__(BLOCK) ts12_colscan_kernel(uint32_t* __restrict__ table, int nb_cap, int n_cap, const uint32_t* __restrict__ n_dev,
                                                             uint32_t* __restrict__ totals, int nbins) {
    __shared__ uint32_t psum[16][17];
    // (the rows that were written: the key blocks of the count; the totals still sit behind the nb_cap rows of the launch)
    const int nb = n_dev ? (int)min((uint32_t)nb_cap, (uint32_t)ts12_blocks((int)min((uint32_t)n_cap, n_dev[0]))) : nb_cap;
    const int col = threadIdx.x & 15, seg = threadIdx.x >> 4;
    const int d = blockIdx.x * 16 + col;
    const int rps = (nb + 15) / 16, r0 = min(nb, seg * rps), r1 = min(nb, r0 + rps);
    uint32_t* colp = table + d;
    uint32_t sum = 0;
    int r = r0;
    for (; r + 8 <= r1; r += 8) {
        uint32_t c[8];
#pragma unroll
        for (int j = 0; j < 8; j++) c[j] = colp[(size_t)(r + j) * nbins];
#pragma unroll
        for (int j = 0; j < 8; j++) sum += c[j];
    }
    for (; r < r1; r++) sum += colp[(size_t)r * nbins];
    psum[seg][col] = sum;
    __syncthreads();
    uint32_t run = 0, all = 0;
#pragma unroll
    for (int sg = 0; sg < 16; sg++) { const uint32_t v = psum[sg][col]; run += sg < seg ? v : 0u; all += v; }
    if (seg == 0) totals[d] = all;
    r = r0;
    for (; r + 8 <= r1; r += 8) {
        uint32_t c[8];
#pragma unroll
        for (int j = 0; j < 8; j++) c[j] = colp[(size_t)(r + j) * nbins];
#pragma unroll
        for (int j = 0; j < 8; j++) { colp[(size_t)(r + j) * nbins] = run; run += c[j]; }
    }
    for (; r < r1; r++) { const uint32_t c = colp[(size_t)r * nbins]; colp[(size_t)r * nbins] = run; run += c; }
}

__global__ void __launch_bounds__(TS12T) ts12_scatter_kernel(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ vin,
                                                             uint32_t* __restrict__ vout, int n_cap,
                                                             const uint32_t* __restrict__ n_dev, const uint32_t* __restrict__ table,
                                                             const uint32_t* __restrict__ totals, uint32_t* __restrict__ ranges, int T, int nbins) {
    __shared__ uint32_t cur[TS12_BINS];          // global position of this workgroup's first key of every tile
    __shared__ uint16_t wcnt[TS12W][TS12_BINS];  // per-wave tile counters (a wave holds 512 keys)
    uint32_t* wtot = cur;                        // (scan scratch in the cursors' first words: with it two workgroups are exactly a CU's 160 KiB)
    constexpr int PERMAX = TS12_BINS / TS12T;    // up to 8 consecutive tiles per thread in the scan
    constexpr int ROUNDS = TS12K / TS12T;        // 8 rounds of 64 keys per wave
    const int per = nbins / TS12T;               // (nbins is a multiple of the workgroup size)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = n_dev ? (int)min((uint32_t)n_cap, n_dev[0]) : n_cap;
    // (no keys: nothing to place; workgroup 0 still writes every range, all of them (0, 0) when the view has no instance)
    if (blockIdx.x != 0 && (int)blockIdx.x >= ts12_blocks(n)) return;
    const int base = blockIdx.x * TS12K + wave * (64 * ROUNDS);   // wave w owns the w-th run of 512 keys, round-major = key order
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint32_t ks[ROUNDS], vs[ROUNDS];
    uint16_t rk[ROUNDS];
#pragma unroll
    for (int c = 0; c < ROUNDS; c++) {
        const int e = base + c * 64 + lane;
        ks[c] = e < n ? kin[e] : 0u;
        vs[c] = e < n ? vin[e] : 0u;
    }
    // ---- tile bases: exclusive scan of the totals (thread t owns tiles per t .. per t + per - 1) ----
    uint32_t tot[PERMAX], pre[PERMAX];
    {
        const uint32_t* tp = totals + t * per;
        const uint32_t* rp = table + (size_t)blockIdx.x * nbins + t * per;
#pragma unroll
        for (int j = 0; j < PERMAX; j++) { tot[j] = j < per ? tp[j] : 0u; pre[j] = j < per ? rp[j] : 0u; }
    }
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < PERMAX; j++) sum += tot[j];
#pragma unroll
    for (int w = 0; w < TS12W; w++)
        for (int i = t; i < nbins / 2; i += TS12T) reinterpret_cast<uint32_t*>(&wcnt[w][0])[i] = 0u;
    uint32_t run = block_excl_scan<TS12W>(sum, wtot);   // (its barrier also: the wave counters are zero)
    __syncthreads();   // (every wave has read the scan scratch: the cursors may be written)
#pragma unroll
    for (int j = 0; j < PERMAX; j++) {
        if (j < per) {
            const int tile = t * per + j;
            cur[tile] = run + pre[j];
            if (blockIdx.x == 0 && tile < T) {   // identifyTileRanges (rasterizer_impl.cu:116-138): [start, end), empty tiles stay (0, 0)
                ranges[2 * tile] = tot[j] ? run : 0u;
                ranges[2 * tile + 1] = tot[j] ? run + tot[j] : 0u;
            }
            run += tot[j];
        }
    }
    // ---- stable rank of every key among the keys of its WAVE with the same tile id ----
#pragma unroll
    for (int c = 0; c < ROUNDS; c++) {
        const bool valid = base + c * 64 + lane < n;
        const uint32_t d = ks[c] & (TS12_BINS - 1);
        const unsigned long long same = wave_match(d, 12, valid);
        const uint32_t in_round = (uint32_t)__popcll(same & lt_mask);
        const uint32_t prior = wcnt[wave][d];   // (the DS operations of a wave execute in order: every lane reads before the leader writes)
        rk[c] = (uint16_t)(prior + in_round);
        if (valid && in_round == 0) wcnt[wave][d] = (uint16_t)(prior + (uint32_t)__popcll(same));
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < ROUNDS; c++) {
        if (base + c * 64 + lane < n) {
            const uint32_t d = ks[c] & (TS12_BINS - 1);
            uint32_t pos = cur[d] + rk[c];
#pragma unroll
            for (int w = 0; w < TS12W - 1; w++)
                if (wave > w) pos += wcnt[w][d];
            vout[pos] = vs[c];   // (the sorted tile ids are not written: nothing reads them, the ranges come from the totals)
        }
    }
}

// ---- emit --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) emit_kernel(int P, const uint32_t* __restrict__ order,
                                                     const uint32_t* __restrict__ tiles,
                                                     const uint32_t* __restrict__ offsets, float* __restrict__ rec,
                                                     const int32_t* __restrict__ radii, int gx, int gy,
                                                     uint32_t* __restrict__ tile_keys, uint32_t* __restrict__ vals,
                                                     uint32_t cap, uint32_t* __restrict__ ranges, int n_ranges,
                                                     uint32_t* __restrict__ seg_count, uint32_t* __restrict__ gtot,
                                                     int n_gtot, const uint32_t* __restrict__ span,
                                                     uint32_t* __restrict__ disp_ctr) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    // piggy-backed initialisation of four small tables used by later stages (saves as many memset launches)
    for (int j = i; j < n_ranges; j += gridDim.x * BLOCK) ranges[j] = 0u;
    for (int j = i; j < n_gtot; j += gridDim.x * BLOCK) gtot[j] = 0u;
    for (int j = i; j < DISP_CTR_WORDS; j += gridDim.x * BLOCK) disp_ctr[j] = 0u;   // (the cull's dispatch buckets: common.hpp DISP_NCLS)
    if (i == 0) seg_count[0] = 0u;
    // One wave = 64 consecutive Gaussians of the depth order; their instances are one contiguous run of the output (offsets is the
    // exclusive scan in this order).  The run is written COOPERATIVELY: instance j of the wave goes to lane j & 63 of round j >> 6, which
    // finds its Gaussian by a binary search over the lanes' local offsets (6 steps through the LDS crossbar) -- every store instruction
    // writes 256 contiguous bytes and no lane idles while another one walks a large rectangle.  (A thread per Gaussian looping over its
    // rectangle wrote 64 dwords 24 bytes apart per instruction and ran as long as the wave's largest splat: 80 us for 5.5 M instances.)
    const int lane = threadIdx.x & 63;
    // (order[0 .. *span) holds every Gaussian that touches a tile -- the culled ones, more than half of a closed surface's surfels, sort
    // behind them)
    const uint32_t nvis = min((uint32_t)P, span[0]);
    if ((uint32_t)(i - lane) >= nvis) return;   // (uniform: the whole wave lies behind the visible span)
    const bool valid = (uint32_t)i < nvis;
    const uint32_t g = valid ? order[i] : 0u;
    const uint32_t off = valid ? offsets[i] : 0u;
    // (requested together, one latency behind `order`: the Gaussian's tile count and rectangle, as the preprocess stage computed them --
    // auxiliary.h:53-63 -- in one 8-byte gather)
    const uint2 tr = valid ? reinterpret_cast<const uint2*>(tiles)[g] : make_uint2(0u, 0u);
    const uint32_t n = tr.x, rect = tr.y;
    if (n != 0u) {   // for the backward's gradient rows: first instance index (emit order) and tile rectangle of this Gaussian
        rec[(size_t)g * REC + R_IBASE] = __builtin_bit_cast(float, off);
        rec[(size_t)g * REC + R_RECT] = __builtin_bit_cast(float, rect);
    }
    // local exclusive offsets of the wave's Gaussians and the run's length
    const uint32_t incl = wave_incl_scan_u32(n);   // (every lane of the wave is here: the exit above is per wave)
    const uint32_t loc = incl - n;
    const uint32_t M = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    const uint32_t base = (uint32_t)__builtin_amdgcn_readfirstlane((int)(off - loc));   // (lane 0 is valid; off = base + loc on every valid lane)
    for (uint32_t j0 = 0; j0 < M; j0 += 64u) {
        const uint32_t j = j0 + (uint32_t)lane;
        // owner = the last lane whose local offset is <= j (lanes without instances share their successor's offset and lose to it)
        int lo = 0;
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) {
            const int mid = lo + step;   // (<= 63)
            const uint32_t v = (uint32_t)__builtin_amdgcn_ds_bpermute(mid << 2, (int)loc);
            lo = v <= j ? mid : lo;
        }
        const uint32_t t = j - (uint32_t)__builtin_amdgcn_ds_bpermute(lo << 2, (int)loc);
        const uint32_t go = (uint32_t)__builtin_amdgcn_ds_bpermute(lo << 2, (int)g);
        const uint32_t ro = (uint32_t)__builtin_amdgcn_ds_bpermute(lo << 2, (int)rect);
        const uint32_t w = max(ro >> 20, 1u), ty = t / w, tx = t - ty * w;
        const uint32_t pos = base + j;
        if (j < M && pos < cap) {   // (pos >= cap only ever for a speculative launch whose capacity guess was too small)
            tile_keys[pos] = (((ro >> 10) & 1023u) + ty) * (uint32_t)gx + ((ro & 1023u) + tx);
            vals[pos] = go;
        }
    }
}

__global__ void __launch_bounds__(BLOCK) ranges_kernel(int R_cap, const uint32_t* __restrict__ R_dev,
                                                       const uint32_t* __restrict__ tile_keys,
                                                       uint32_t* __restrict__ ranges) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    const int R = R_dev ? (int)min((uint32_t)R_cap, R_dev[0]) : R_cap;
    if (i >= R) return;
    const uint32_t cur = tile_keys[i];
    if (i == 0) ranges[2 * cur] = 0;
    else {
        const uint32_t prev = tile_keys[i - 1];
        if (cur != prev) { ranges[2 * prev + 1] = (uint32_t)i; ranges[2 * cur] = (uint32_t)i; }
    }
    if (i == R - 1) ranges[2 * cur + 1] = (uint32_t)R;
}

// Dispatch order, first gradient row and first state slot of every sub-tile, and the view's totals, for launches that fill the machine
// several times over (api.hip high_fill; at low fill the cull publishes all of it itself: common.hpp DISP_NCLS): counting sorts of the
// sub-tiles by descending count -- 1024 size buckets, one per count below 1023, everything longer shares the first -- exclusive prefix
// sums, in index order, of the counts and of seg_slots(count), and their sums (device + tagged host copy).  ONE LONGEST-FIRST LIST PER
// XCD, and one workgroup per XCD to build it.  Workgroups are dealt to the eight XCDs round-robin (workgroup b of the composite runs on XCD b & 7), and
// each XCD has its own 4 MiB L2: with one global order the ~3 sub-tiles that gather a splat's record and vfeature rows run on three
// different XCDs, and each L2 fetches them again.  Here the image is cut into blocks of 4 x 4 tiles, block (bx, by) belongs to XCD
// (bx + 3 by) & 7 (common.hpp xcd_of_tile); workgroup c counting-sorts the sub-tiles of XCD c by descending count and writes its j-th item
// to order[8 j + c] (the lists differ in length by a few blocks: the tail is padded with ORDER_NONE up to order_n = order_entries()).
// With tens of thousands of waves the XCDs' sums are balanced to a few per cent; with one round of waves they are not (the exact order
// wins there: cfg4 render 220 vs 231 us).  The index-order prefixes are split eight ways too: workgroup c scans the c-th eighth of the
// items behind a reduction of everything in front of it (every workgroup reads all n counts twice: 40 loads per thread at 1600 x 1600),
// and the last one -- which has seen every item -- publishes the totals.  cfg5 (40 000 sub-tiles): 49 us for the single workgroup.
__global__ void __launch_bounds__(1024) order_xcd_kernel(const uint32_t* __restrict__ counts, int n, uint32_t* __restrict__ order,
                                                         uint32_t* __restrict__ prefix, uint32_t* __restrict__ slot_prefix,
                                                         uint32_t* __restrict__ total, unsigned long long* __restrict__ host_total,
                                                         uint32_t host_tag, uint32_t cap_R, long long cap_slots, uint32_t magic, int gx,
                                                         int order_n) {
    __shared__ uint32_t hist[1024];
    __shared__ uint32_t wsum[16];
    __shared__ unsigned long long wsum2[16];
    __shared__ uint32_t wzero[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t c = blockIdx.x;   // XCD whose list this workgroup builds; also its eighth of the prefixes
    hist[t] = 0;
    auto both = [](uint32_t v) { return (unsigned long long)v | ((unsigned long long)seg_slots(v) << 32); };
    const int per = ((n + 7) / 8 + 1023) / 1024 * 1024;       // items per workgroup (prefix part), a multiple of the workgroup size
    const int p0 = min(n, (int)c * per), p1 = min(n, p0 + per);
    __syncthreads();
    // ---- pass 1 over ALL items: histogram of this XCD's items; sum (counts | slots) and number of empty items in front of p0
    unsigned long long before = 0;
    uint32_t zeros = 0;
    for (int i = t; i < n; i += 1024) {
        const uint32_t len = counts[i];
        const int tile = i >> 2;
        if (xcd_of_tile(tile % gx, tile / gx) == c) atomicAdd(&hist[1023u - min(1023u, len)], 1u);
        if (i < p0) before += both(len);
        zeros += len == 0u ? 1u : 0u;
    }
    before = wave_reduce_add(before);
    zeros = wave_reduce_add(zeros);
    if (lane == 0) { wsum2[wave] = before; wzero[wave] = zeros; }
    __syncthreads();
    unsigned long long run = 0;
    uint32_t n_empty = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) { run += wsum2[w]; n_empty += wzero[w]; }
    // ---- bucket cursors of this XCD
    uint32_t n_mine;
    hist[t] = block_excl_scan<16>(hist[t], wsum, &n_mine);
    __syncthreads();
    // ---- prefixes of this workgroup's eighth, in index order: 1024 items per round (wave scans + a scan over the 16 wave totals)
    for (int i0 = p0; i0 < p1; i0 += 1024) {
        const int i = i0 + t;
        const unsigned long long v = both(i < p1 ? counts[i] : 0u);
        // (the two halves are scanned on their own: no carry from the counts into the slots inside a wave)
        const unsigned long long inc = (unsigned long long)wave_incl_scan_u32((uint32_t)v) | ((unsigned long long)wave_incl_scan_u32((uint32_t)(v >> 32)) << 32);
        __syncthreads();   // (wsum2 of the previous round has been read)
        unsigned long long all;
        const unsigned long long ex = run + block_excl_scan<16>(v, inc, wsum2, &all);
        if (i < p1) {
            if (prefix) prefix[i] = (uint32_t)ex;
            if (slot_prefix) slot_prefix[i] = (uint32_t)(ex >> 32);
        }
        run += all;
    }
    // (the workgroup that owns the last eighth has now summed every item: it publishes the totals; an eighth may be empty: p0 == p1 == n)
    if (c == 7 && t == 0) {
        if (total) {
            total[1] = (uint32_t)run; total[2] = (uint32_t)(run >> 32);
            total[3] = magic; total[4] = cap_R; total[5] = (uint32_t)(unsigned long long)cap_slots; total[6] = (uint32_t)((unsigned long long)cap_slots >> 32);
        }
        if (host_total) {
            __hip_atomic_store(host_total + 2, ((unsigned long long)host_tag << 32) | (unsigned long long)((uint32_t)n - n_empty), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_total, ((unsigned long long)host_tag << 32) | (run & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_total + 1, ((unsigned long long)host_tag << 32) | (run >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    // ---- pass 2: this XCD's items to order[8 j + c] (equal sizes in arrival order), then the padding behind the list
    for (int i = t; i < n; i += 1024) {
        const int tile = i >> 2;
        if (xcd_of_tile(tile % gx, tile / gx) != c) continue;
        const uint32_t len = counts[i];
        order[8u * atomicAdd(&hist[1023u - min(1023u, len)], 1u) + c] = (uint32_t)i;
    }
    for (uint32_t j = n_mine + (uint32_t)t; 8u * j + c < (uint32_t)order_n; j += 1024u) order[8u * j + c] = ORDER_NONE;
}

}  // namespace

void launch_order_desc(const uint32_t* counts, int n, uint32_t* order, uint32_t* prefix, uint32_t* slot_prefix, uint32_t* totals,
                       unsigned long long* host_totals, uint32_t host_tag, uint32_t cap_R, long long cap_slots, uint32_t magic, int gx, int order_n,
                       hipStream_t s) {
    hipLaunchKernelGGL(order_xcd_kernel, dim3(8), dim3(1024), 0, s, counts, n, order, prefix, slot_prefix, totals, host_totals,
                       host_tag, cap_R, cap_slots, magic, gx, order_n);
}

template <int ITEMS>
static void radix_sort_impl(uint32_t* const key[2], uint32_t* const val[2], int n, const uint32_t* n_dev, int total_bits,
                            int bits_per_pass, uint32_t* tbl, uint32_t* gtot, hipStream_t s, const RadixWeights* weights) {
    const int per = BLOCK * ITEMS;
    const int nb = (n + per - 1) / per;
    const int ng = (nb + GS - 1) / GS;
    const int passes = (total_bits + bits_per_pass - 1) / bits_per_pass;
    // the weighted pass: count known at launch (block 0 publishes it for the host), digits staged as bytes, its totals in the slot behind four passes'
    assert(!weights || (n_dev == nullptr && bits_per_pass <= 8 && passes <= RADIX_WGTOT_SLOT));
    for (int p = 0; p < passes; p++) {
        const int lo = p * bits_per_pass, nbits = std::min(bits_per_pass, total_bits - lo);
        uint32_t* gt = gtot + (size_t)p * ng * 256;
        if (weights && p == passes - 1) {
            const WeightArgs wa{val[p & 1], gtot + (size_t)RADIX_WGTOT_SLOT * ng * 256, *weights};
            hipLaunchKernelGGL((radix_hist_kernel<ITEMS, true>), dim3(nb), dim3(BLOCK), 0, s, key[p & 1], n, n_dev, lo,
                               (1u << nbits) - 1, tbl, gt, wa);
            hipLaunchKernelGGL((radix_scatter_kernel<ITEMS, true>), dim3(nb), dim3(BLOCK), 0, s, key[p & 1], val[p & 1],
                               key[(p + 1) & 1], val[(p + 1) & 1], n, n_dev, lo, nbits, tbl, gt, ng, wa);
            break;
        }
        hipLaunchKernelGGL((radix_hist_kernel<ITEMS>), dim3(nb), dim3(BLOCK), 0, s, key[p & 1], n, n_dev, lo,
                           (1u << nbits) - 1, tbl, gt, WeightArgs{});
        hipLaunchKernelGGL((radix_scatter_kernel<ITEMS>), dim3(nb), dim3(BLOCK), 0, s, key[p & 1], val[p & 1],
                           key[(p + 1) & 1], val[(p + 1) & 1], n, n_dev, lo, nbits, tbl, gt, ng, WeightArgs{});
    }
}

// Stable LSD radix sort of (u32 key, u32 value) pairs on bits [0, total_bits) in passes of bits_per_pass (<= 8);
// the result lands in slot (passes & 1) of the ping/pong buffers.  `n` sizes the launch and the scratch
// (`table`: radix_table_words(n) counters, its radix_gtot() part zeroed by the caller); if `n_dev` is not null the element count is min(n, *n_dev), read on the
// device (the count need not be known on the host at launch time).
// `weights`: see common.hpp RadixWeights.
void launch_radix_sort(uint32_t* const key[2], uint32_t* const val[2], int n, const uint32_t* n_dev, int total_bits,
                       int bits_per_pass, uint32_t* table, hipStream_t s, const RadixWeights* weights) {
    if (n <= 0) return;
    uint32_t* gtot = radix_gtot(table, n);  // [passes <= 4, + the weighted pass's slot][groups][256] group totals, zero on entry
    if (n <= (1 << 20)) radix_sort_impl<4>(key, val, n, n_dev, total_bits, bits_per_pass, table, gtot, s, weights);
    else radix_sort_impl<16>(key, val, n, n_dev, total_bits, bits_per_pass, table, gtot, s, weights);
}

// depth_sort_plan.hpp
void launch_depth_bucket_sort(const DepthRows& rows, uint32_t* key1, uint32_t* val1, int n, int cap, hipStream_t s, const RadixWeights& w) {
    if (n <= 0) return;
    assert(n <= DEPTH_BUCKET_MAX_P && cap >= DEPTH_BUCKET_CAP_MIN && cap <= DEPTH_BUCKET_CAP);
    hipLaunchKernelGGL(depth_bucket_sort_kernel, dim3(256), dim3(DB_THREADS), 0, s, rows, depth_rows(n), n, key1, val1, w.offsets, cap, w);
}

void launch_emit(int P, const uint32_t* order, const uint32_t* tiles, const uint32_t* offsets, float* rec,
                 const int32_t* radii, int gx, int gy, uint32_t* tile_keys, uint32_t* vals, int cap, uint32_t* ranges,
                 uint32_t* seg_count, uint32_t* sort_table, const uint32_t* span, uint32_t* disp_ctr, hipStream_t s) {
    hipLaunchKernelGGL(emit_kernel, dim3((P + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, P, order, tiles, offsets, rec,
                       radii, gx, gy, tile_keys, vals, (uint32_t)cap, ranges, 2 * gx * gy + (gx * gy + 255) / 256 * SEG_BLOCK_STRIDE, seg_count,
                       radix_gtot(sort_table, cap), (int)radix_gtot_words(cap), span, disp_ctr);
}

void launch_tile_sort12(uint32_t* const key[2], uint32_t* const val[2], int n, const uint32_t* n_dev, uint32_t* table, uint32_t* ranges, int T,
                        hipStream_t s) {
    if (n <= 0) return;
    const int nb = ts12_blocks(n);
    const int nbins = (T + TS12T - 1) / TS12T * TS12T;   // (<= TS12_BINS: tile_sort_plan)
    uint32_t* totals = table + (size_t)nb * nbins;
    hipLaunchKernelGGL(ts12_hist_kernel, dim3(nb), dim3(TS12T), 0, s, key[0], n, n_dev, table, nbins);
    hipLaunchKernelGGL(ts12_colscan_kernel, dim3(nbins / 16), dim3(BLOCK), 0, s, table, nb, n, n_dev, totals, nbins);
    hipLaunchKernelGGL(ts12_scatter_kernel, dim3(nb), dim3(TS12T), 0, s, key[0], val[0], val[1], n, n_dev, table, totals, ranges, T, nbins);
}

// `ranges` must already be zero (launch_emit clears it)
void launch_ranges(int R, const uint32_t* R_dev, const uint32_t* tile_keys, uint32_t* ranges, int T, hipStream_t s) {
    if (R > 0) hipLaunchKernelGGL(ranges_kernel, dim3((R + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, R, R_dev, tile_keys, ranges);
}

}  // namespace svgir
