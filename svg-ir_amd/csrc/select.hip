// svg-ir_amd/csrc/select.hip -- the exact per-column LOWER MEDIAN of an fp32 [n, C] view (torch.median(x, dim=0), C = 1 ... 4) by radix
// select, and its two consumers fused on load: the albedo scale the relighting eval applies (eval_relighting_tensoIR.py:227-237) and
// stage 1's lambda_surface term exp(-mean |xyz - median(xyz)|) (gaussian_renderer/render.py:217-222).
//
// KEYS.  A float becomes an order-preserving uint32: sign bit flipped for x >= 0, all bits flipped for x < 0; -0 is +0 first (one value,
//   it comes out as +0) and every NaN is the one key 0xffffffff, above +inf.  The value handed back is the key turned round again, so it
//   is bit for bit an element of the column.
// RANK.  k = (count - 1) / 2 of the count selected rows -- the lower median -- unless the column holds a NaN: then k = count - 1, the
//   largest key, which IS the NaN key (torch.median propagates NaN).  count == 0: NaN, index -1, counts 0.
// PASSES.  SEL_PASSES = 4 most-significant-digit passes of SEL_BITS = 8 bits.  Pass p histograms digit p of the rows whose higher digits
//   equal the prefix chosen so far, into scratch word [p][c][bin] with integer atomics (their sums do not depend on order).  No launch
//   picks a digit: every workgroup of pass p derives {prefix, rank} ITSELF from what pass p - 1 left -- one 256-thread block_excl_scan
//   per column over the 256 bins, the thread whose bin holds the rank extends the prefix -- and workgroup 0 leaves the pair in scratch
//   for pass p + 1, so a pass does one scan per column, not p.  The key is recomputed from the source in every pass (nothing per row is
//   stored: 4 reads of 7.7 MB at 800 x 800 cost less than a key plane and its write).
// THE HOT BIN.  Clamped ratios sit on `hi` or `lo`, coordinates share an exponent: most rows of a wave share their digit.  hist_add()
//   aggregates per wave before it touches LDS -- a wave-uniform digit is ONE add of the lane count; otherwise wave_match() elects one
//   lane per distinct digit -- and the workgroup flushes only its non-zero bins to scratch (the atomic optimiser is off, csrc/Makefile).
// INDEX / COUNTS.  A fifth pass over the rows (the column form and the loss; the albedo scale has no use for it) takes the SMALLEST row
//   whose key equals the median's -- DECISION: torch leaves the choice among ties open; in a NaN column it is the first NaN row -- as an
//   atomicMax of 0xffffffff - row (0 = none, so one memset of zeros initialises everything).  n_less / n_greater, the rows strictly
//   below / above the median value, need no pass: they are the histogram bins below / above the chosen digit, summed over the passes.
//   They are counted on the keys, so in a NaN column n_less is the number of rows that are not NaN and n_greater is 0.
// LAUNCHES.  One memset of the scratch (16.5 KB) + 4 passes + index pass + one single-workgroup finish: 6 kernels whatever n is; the
//   albedo scale 5; the loss forward 6 (its fifth pass also sums |x - c|, its finish also reduces the records), backward 1.
// No host wait, no allocation, no float atomics: two runs give the same bits, whatever the scratch held.
#include "common.hpp"
#include "srgb.hpp"

namespace svgir {

int report_error(int code, const char* fmt, ...);   // api.hip

namespace {

constexpr int SEL_BITS = 8, SEL_BINS = 1 << SEL_BITS, SEL_PASSES = 32 / SEL_BITS, SEL_MAXC = 4;
constexpr int SEL_PER_THREAD = 8;                       // rows per thread
constexpr int SEL_ROWS = BLOCK * SEL_PER_THREAD;        // rows per workgroup
static_assert(SEL_BINS == BLOCK, "one thread per bin in derive()");
// the scratch, in uint32 words
constexpr int SEL_HIST = 0;                                               // [SEL_PASSES][SEL_MAXC][SEL_BINS]
constexpr int SEL_STATE = SEL_HIST + SEL_PASSES * SEL_MAXC * SEL_BINS;    // [SEL_PASSES][SEL_MAXC][2] {prefix, rank} pass p starts from (p >= 1)
constexpr int SEL_NAN = SEL_STATE + SEL_PASSES * SEL_MAXC * 2;            // [SEL_MAXC] NaN rows
constexpr int SEL_INDEX = SEL_NAN + SEL_MAXC;                             // [SEL_MAXC] 0xffffffff - smallest median row; 0 = none
constexpr int SEL_WORDS = SEL_INDEX + SEL_MAXC;
static_assert(SEL_WORDS % 2 == 0, "the loss puts its double records behind the scratch");
constexpr uint32_t KEY_NAN = 0xffffffffu;

__device__ __forceinline__ uint32_t key_of(float x) {
    if (x != x) return KEY_NAN;
    const uint32_t u = x == 0.f ? 0u : __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t k) {
    if (k == KEY_NAN) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// ---- key sources: load(i, key) gives the C keys of row i and whether the row is selected at all ---------------------------------------
struct ColumnSource {   // x[i, c] = base[i * row_stride + c * col_stride]
    const float* base;
    long long row_stride, col_stride;
    uint32_t n;
    int C;
    __device__ __forceinline__ bool load(uint32_t i, uint32_t (&key)[SEL_MAXC]) const {
#pragma unroll
        for (int c = 0; c < SEL_MAXC; c++)
            if (c < C) key[c] = key_of(base[(long long)i * row_stride + (long long)c * col_stride]);
        return true;
    }
};

// clamp(gt / srgb_to_rgb?(render), lo, hi) of the pixels with ((r0 + r1) + r2) / 3 > 0, fp32 in torch's operation order, nothing fused;
// the clamp passes NaN (0 / 0) and turns x / 0 = inf into hi
struct AlbedoSource {
    const float *render, *gt;
    float lo, hi;
    int srgb;
    uint32_t n;
    int C;
    __device__ __forceinline__ bool load(uint32_t i, uint32_t (&key)[SEL_MAXC]) const {
#pragma clang fp contract(off)
        float r[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float x = render[(size_t)c * n + i];
            r[c] = srgb ? srgb_to_rgb(x) : x;
        }
        if (!(__fdiv_rn((r[0] + r[1]) + r[2], 3.f) > 0.f)) return false;   // render_albedo.mean(dim=0) > 0
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float q = __fdiv_rn(gt[(size_t)c * n + i], r[c]);
            key[c] = key_of(q < lo ? lo : (q > hi ? hi : q));
        }
        return true;
    }
};

// ---- one digit per lane into the workgroup's histogram, aggregated per wave before LDS sees it (wave-uniform control flow only) ---------
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t digit, bool valid) {
    const unsigned long long act = __ballot(valid);
    if (act == 0) return;
    const int lane = threadIdx.x & 63;
    const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)digit, __ffsll((long long)act) - 1);
    if (__ballot(valid && digit != first) == 0) {   // the hot bin: one add for the whole wave
        if (lane == 0) atomicAdd(&hist[first], (uint32_t)__popcll(act));
        return;
    }
    const unsigned long long same = wave_match(digit, SEL_BITS, valid);
    if (valid && (same & ((1ull << lane) - 1ull)) == 0) atomicAdd(&hist[digit], (uint32_t)__popcll(same));   // the first lane of each digit
}

struct SelShared {
    uint32_t wsum[SEL_MAXC][4];
    uint32_t st[SEL_MAXC][2];
};

// {prefix, rank} per column that pass `pass` (1 ... SEL_PASSES; SEL_PASSES: the prefix is the median's whole key) starts from, in every
// thread of the 256-thread workgroup, from the histogram and the pair of pass - 1.  An empty selection gives zeros throughout.
__device__ __forceinline__ void derive(const uint32_t* __restrict__ scr, int pass, int C, SelShared& sh, uint32_t (&prefix)[SEL_MAXC],
                                       uint32_t (&rank)[SEL_MAXC]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < SEL_MAXC; c++) {
        prefix[c] = rank[c] = 0;
        if (c >= C) continue;   // (uniform)
        const uint32_t h = scr[SEL_HIST + ((pass - 1) * SEL_MAXC + c) * SEL_BINS + t];
        const uint32_t* prev = scr + SEL_STATE + ((pass - 1) * SEL_MAXC + c) * 2;
        const uint32_t p0 = pass == 1 ? 0u : prev[0];
        if (t == 0) { sh.st[c][0] = p0 << SEL_BITS; sh.st[c][1] = 0; }   // what stands when no row is selected
        uint32_t total;
        const uint32_t excl = block_excl_scan<4>(h, sh.wsum[c], &total);   // (its barrier is behind the two writes above)
        const uint32_t k0 = pass == 1 ? (total == 0 ? 0u : (scr[SEL_NAN + c] ? total - 1 : (total - 1) / 2)) : prev[1];
        if (h > 0 && excl <= k0 && k0 - excl < h) { sh.st[c][0] = (p0 << SEL_BITS) | (uint32_t)t; sh.st[c][1] = k0 - excl; }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < SEL_MAXC; c++)
        if (c < C) { prefix[c] = sh.st[c][0]; rank[c] = sh.st[c][1]; }
}

template <class Src>
__global__ void __launch_bounds__(BLOCK) select_pass_kernel(const Src src, uint32_t* __restrict__ scr, int pass) {
    __shared__ uint32_t hist[SEL_MAXC][SEL_BINS];
    __shared__ SelShared sh;
    const int t = threadIdx.x, C = src.C;
#pragma unroll
    for (int c = 0; c < SEL_MAXC; c++) hist[c][t] = 0;
    uint32_t prefix[SEL_MAXC] = {0, 0, 0, 0}, rank[SEL_MAXC];
    if (pass > 0) {
        derive(scr, pass, C, sh, prefix, rank);
        if (blockIdx.x == 0 && t < C) {   // for pass + 1 (this launch reads the pair of pass - 1 only)
            scr[SEL_STATE + (pass * SEL_MAXC + t) * 2] = sh.st[t][0];
            scr[SEL_STATE + (pass * SEL_MAXC + t) * 2 + 1] = sh.st[t][1];
        }
    }
    __syncthreads();
    const int shift = 32 - SEL_BITS * (pass + 1);
    uint32_t nan[SEL_MAXC] = {0, 0, 0, 0};
    for (int j = 0; j < SEL_PER_THREAD; j++) {
        const unsigned long long i = (unsigned long long)blockIdx.x * SEL_ROWS + (unsigned)(j * BLOCK + t);
        uint32_t key[SEL_MAXC] = {0, 0, 0, 0};
        const bool row = i < src.n && src.load((uint32_t)i, key);
#pragma unroll
        for (int c = 0; c < SEL_MAXC; c++) {
            if (c >= C) continue;
            // (the 64-bit shift: pass 0 shifts by 32 and compares 0 with the empty prefix)
            const bool valid = row && (uint32_t)((unsigned long long)key[c] >> (shift + SEL_BITS)) == prefix[c];
            hist_add(hist[c], (key[c] >> shift) & (SEL_BINS - 1), valid);
            nan[c] += row && key[c] == KEY_NAN;
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < SEL_MAXC; c++) {
        if (c >= C) continue;
        const uint32_t v = hist[c][t];
        if (v) atomicAdd(&scr[SEL_HIST + (pass * SEL_MAXC + c) * SEL_BINS + t], v);
        if (pass == 0) {
            const uint32_t m = wave_reduce_add(nan[c]);
            if ((t & 63) == 0 && m) atomicAdd(&scr[SEL_NAN + c], m);
        }
    }
}

// the smallest row whose key is the median's, per column, into scr[SEL_INDEX] (every lane of the wave calls it)
__device__ __forceinline__ void index_put(uint32_t* __restrict__ scr, int C, const uint32_t (&inv)[SEL_MAXC]) {
#pragma unroll
    for (int c = 0; c < SEL_MAXC; c++) {
        if (c >= C) continue;
        const uint32_t m = wave_reduce_max(inv[c]);
        if ((threadIdx.x & 63) == 0 && m) atomicMax(&scr[SEL_INDEX + c], m);
    }
}

__global__ void __launch_bounds__(BLOCK) select_index_kernel(const ColumnSource src, uint32_t* __restrict__ scr) {
    __shared__ SelShared sh;
    const int t = threadIdx.x, C = src.C;
    uint32_t med[SEL_MAXC], rank[SEL_MAXC], inv[SEL_MAXC] = {0, 0, 0, 0};
    derive(scr, SEL_PASSES, C, sh, med, rank);
    for (int j = 0; j < SEL_PER_THREAD; j++) {
        const unsigned long long i = (unsigned long long)blockIdx.x * SEL_ROWS + (unsigned)(j * BLOCK + t);
        uint32_t key[SEL_MAXC] = {0, 0, 0, 0};
        if (!(i < src.n && src.load((uint32_t)i, key))) continue;
#pragma unroll
        for (int c = 0; c < SEL_MAXC; c++)
            if (c < C && key[c] == med[c]) inv[c] = max(inv[c], 0xffffffffu - (uint32_t)i);
    }
    index_put(scr, C, inv);
}

// What a finished selection says per column, in every thread of ONE 256-thread workgroup: the median's key, the number of selected rows,
// the rows strictly below / above it (the bins below / above the chosen digit of every pass) and the smallest median row (-1: none).
struct SelResult {
    uint32_t key[SEL_MAXC], count[SEL_MAXC], less[SEL_MAXC], greater[SEL_MAXC];
    int32_t index[SEL_MAXC];
};
__device__ __forceinline__ void finish(const uint32_t* __restrict__ scr, int C, SelShared& sh, uint32_t (*cnt)[3], SelResult& r) {
    const int t = threadIdx.x;
    if (t < SEL_MAXC * 3) cnt[t / 3][t % 3] = 0;
    uint32_t rank[SEL_MAXC];
    derive(scr, SEL_PASSES, C, sh, r.key, rank);   // (its barriers are behind the clear)
#pragma unroll
    for (int c = 0; c < SEL_MAXC; c++) {
        if (c >= C) continue;
        uint32_t v[3] = {0, 0, 0};   // count, less, greater
#pragma unroll
        for (int p = 0; p < SEL_PASSES; p++) {
            const uint32_t h = scr[SEL_HIST + (p * SEL_MAXC + c) * SEL_BINS + t];
            const uint32_t d = (r.key[c] >> (32 - SEL_BITS * (p + 1))) & (SEL_BINS - 1);
            if (p == 0) v[0] += h;
            v[1] += (uint32_t)t < d ? h : 0u;
            v[2] += (uint32_t)t > d ? h : 0u;
        }
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const uint32_t m = wave_reduce_add(v[q]);
            if ((t & 63) == 0 && m) atomicAdd(&cnt[c][q], m);
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < SEL_MAXC; c++) {
        r.count[c] = r.less[c] = r.greater[c] = 0; r.index[c] = -1;
        if (c >= C) continue;
        r.count[c] = cnt[c][0]; r.less[c] = cnt[c][1]; r.greater[c] = cnt[c][2];
        const uint32_t inv = scr[SEL_INDEX + c];
        r.index[c] = inv ? (int32_t)(0xffffffffu - inv) : -1;
    }
}

__global__ void __launch_bounds__(BLOCK) column_median_finish_kernel(const uint32_t* __restrict__ scr, int C, int empty, float* __restrict__ values,
                                                                      int32_t* __restrict__ indices, int32_t* __restrict__ n_less,
                                                                      int32_t* __restrict__ n_greater) {
    __shared__ SelShared sh;
    __shared__ uint32_t cnt[SEL_MAXC][3];
    SelResult r{};
    if (!empty) finish(scr, C, sh, cnt, r);   // (uniform; n == 0: the scratch was never touched)
#pragma unroll
    for (int c = 0; c < SEL_MAXC; c++) {   // thread c writes column c (c is a constant per copy of the body: r stays in registers)
        if ((int)threadIdx.x != c || c >= C) continue;
        values[c] = empty ? value_of(KEY_NAN) : value_of(r.key[c]);
        indices[c] = empty ? -1 : r.index[c];
        if (n_less) n_less[c] = (int32_t)r.less[c];
        if (n_greater) n_greater[c] = (int32_t)r.greater[c];
    }
}

__global__ void __launch_bounds__(BLOCK) albedo_median_finish_kernel(const uint32_t* __restrict__ scr, float* __restrict__ scale3,
                                                                      int32_t* __restrict__ count) {
    __shared__ SelShared sh;
    __shared__ uint32_t cnt[SEL_MAXC][3];
    SelResult r{};
    finish(scr, 3, sh, cnt, r);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if ((int)threadIdx.x != c) continue;
        scale3[c] = r.count[c] ? value_of(r.key[c]) : value_of(KEY_NAN);   // an empty selection: NaN and 0
        if (c == 0) count[0] = (int32_t)r.count[0];
    }
}

// ---- lambda_surface ---------------------------------------------------------------------------------------------------------------
constexpr int SC_STATS = 11;   // sum, 3 P, then {index, n_less, n_greater} per column

// the fifth pass of the loss: the smallest median rows, and one double per workgroup: the sum of the fp32 values |x_ic - c_c| (wave
// butterfly, then the four waves in a fixed order)
__global__ void __launch_bounds__(BLOCK) surface_center_fwd_kernel(const ColumnSource src, uint32_t* __restrict__ scr, double* __restrict__ partial) {
    __shared__ SelShared sh;
    __shared__ double red[1][4];
    const int t = threadIdx.x;
    uint32_t med[SEL_MAXC], rank[SEL_MAXC], inv[SEL_MAXC] = {0, 0, 0, 0};
    derive(scr, SEL_PASSES, 3, sh, med, rank);
    const float center[3] = {value_of(med[0]), value_of(med[1]), value_of(med[2])};
    double s = 0.0;
    for (int j = 0; j < SEL_PER_THREAD; j++) {
        const unsigned long long i = (unsigned long long)blockIdx.x * SEL_ROWS + (unsigned)(j * BLOCK + t);
        uint32_t key[SEL_MAXC] = {0, 0, 0, 0};
        if (!(i < src.n && src.load((uint32_t)i, key))) continue;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if (key[c] == med[c]) inv[c] = max(inv[c], 0xffffffffu - (uint32_t)i);
            s += (double)fabsf(value_of(key[c]) - center[c]);   // (-0 reads as +0: the same difference)
        }
    }
    index_put(scr, 3, inv);
    double v[1] = {wave_reduce_add(s)};
    block_sum_ordered(v, red);
    if (t == 0) partial[blockIdx.x] = v[0];
}

__global__ void __launch_bounds__(256) surface_center_reduce_kernel(const uint32_t* __restrict__ scr, const double* __restrict__ partial, int nblk,
                                                                    double P, double* __restrict__ stats, float* __restrict__ loss) {
    __shared__ SelShared sh;
    __shared__ uint32_t cnt[SEL_MAXC][3];
    __shared__ double red[1][4];
    if (nblk == 0) {   // P == 0: NaN, nothing else written
        if (threadIdx.x == 0) loss[0] = value_of(KEY_NAN);
        return;
    }
    double s[1];
    block_reduce_records(partial, nblk, 1, s, red);
    SelResult r{};
    finish(scr, 3, sh, cnt, r);
    if (threadIdx.x == 0) {
        stats[0] = s[0]; stats[1] = 3.0 * P;
        loss[0] = (float)exp(-s[0] / (3.0 * P));
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if ((int)threadIdx.x != c) continue;
        stats[2 + 3 * c] = (double)r.index[c]; stats[3 + 3 * c] = (double)r.less[c]; stats[4 + 3 * c] = (double)r.greater[c];
    }
}

// dL_dxyz [P,3], every element: -g L sign(x_ic - c_c) / (3 P), and + g L (n_greater_c - n_less_c) / (3 P) more in the median's own row
// (torch's subgradient of median through `center`); evaluated in double, rounded once.  c_c is read back from its row.  A NaN loss
// (a NaN coordinate) makes the coefficient NaN and with it every element, sign(0) = 0 included (NaN * 0).
__global__ void __launch_bounds__(BLOCK) surface_center_bwd_kernel(const float* __restrict__ xyz, long long P, const double* __restrict__ stats,
                                                                   const float* __restrict__ g, float* __restrict__ d_xyz) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P) return;
    const double L = (double)(float)exp(-stats[0] / stats[1]);
    const double coef = (double)g[0] * L / stats[1];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const long long idx = (long long)stats[2 + 3 * c];
        const float center = idx >= 0 && idx < P ? xyz[idx * 3 + c] : value_of(KEY_NAN);   // (stats that are not a forward's: NaN, no wild read)
        const float d = xyz[i * 3 + c] - center;
        double v = -coef * (d > 0.f ? 1.0 : (d < 0.f ? -1.0 : 0.0));
        if (i == idx) v += coef * (stats[4 + 3 * c] - stats[3 + 3 * c]);
        d_xyz[i * 3 + c] = (float)v;
    }
}

inline unsigned select_blocks(long long n) { return (unsigned)((n + SEL_ROWS - 1) / SEL_ROWS); }

// memset + the four digit passes
template <class Src>
void launch_passes(const Src& src, uint32_t* scr, hipStream_t s) {
    (void)hipMemsetAsync(scr, 0, SEL_WORDS * sizeof(uint32_t), s);
    for (int pass = 0; pass < SEL_PASSES; pass++)
        hipLaunchKernelGGL(select_pass_kernel<Src>, dim3(select_blocks(src.n)), dim3(BLOCK), 0, s, src, scr, pass);
}

constexpr long long SEL_MAX_N = 0x7fffffffLL;   // rows are 31-bit: the index is an int32

}  // namespace

}  // namespace svgir

using namespace svgir;

extern "C" {

size_t svgir_column_median_scratch_bytes(int64_t n, int32_t C) {
    if (n < 0 || n > SEL_MAX_N || C < 1 || C > SEL_MAXC) return 0;
    return SEL_WORDS * sizeof(uint32_t);
}

int svgir_column_median(const float* base, int64_t n, int32_t C, int64_t row_stride, int64_t col_stride, void* scratch, float* values,
                        int32_t* indices, int32_t* n_less, int32_t* n_greater, void* stream) {
    if (C < 1 || C > SEL_MAXC) return report_error(SVGIR_ERR_INVALID, "column_median: C = %d, 1 ... %d columns per call", C, SEL_MAXC);
    if (n < 0 || n > SEL_MAX_N) return report_error(SVGIR_ERR_INVALID, "column_median: n = %lld is outside 0 ... 2^31 - 1", (long long)n);
    if (!values || !indices || (n > 0 && (!base || !scratch)))
        return report_error(SVGIR_ERR_INVALID, "column_median: base, scratch, values and indices must be provided");
    hipStream_t s = (hipStream_t)stream;
    StageMarks tm = stage_begin(s);
    uint32_t* scr = (uint32_t*)scratch;
    if (n > 0) {
        const ColumnSource src{base, (long long)row_stride, (long long)col_stride, (uint32_t)n, C};
        launch_passes(src, scr, s);
        hipLaunchKernelGGL(select_index_kernel, dim3(select_blocks(n)), dim3(BLOCK), 0, s, src, scr);
    }
    hipLaunchKernelGGL(column_median_finish_kernel, dim3(1), dim3(BLOCK), 0, s, (const uint32_t*)scr, (int)C, (int)(n == 0), values, indices,
                       n_less, n_greater);
    stage_mark(tm, "column_median");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SVGIR_OK : report_error(SVGIR_ERR_HIP, "column_median launch failed: %s", hipGetErrorString(e));
}

size_t svgir_albedo_scale_median_scratch_bytes(int32_t W, int32_t H) {
    if (W <= 0 || H <= 0 || (long long)W * H > SEL_MAX_N) return 0;
    return SEL_WORDS * sizeof(uint32_t);
}

int svgir_albedo_scale_median(int32_t W, int32_t H, const float* render_albedo, const float* gt_albedo, int32_t render_srgb, float lo, float hi,
                              void* scratch, float* scale3, int32_t* count, void* stream) {
    if (W <= 0 || H <= 0) return report_error(SVGIR_ERR_INVALID, "albedo_scale_median: bad image size W=%d H=%d", W, H);
    if ((long long)W * H > SEL_MAX_N) return report_error(SVGIR_ERR_INVALID, "albedo_scale_median: image %d x %d exceeds the supported size", W, H);
    if (!(lo <= hi)) return report_error(SVGIR_ERR_INVALID, "albedo_scale_median: the clamp needs lo <= hi, got lo=%g hi=%g", (double)lo, (double)hi);
    if (!render_albedo || !gt_albedo || !scratch || !scale3 || !count)
        return report_error(SVGIR_ERR_INVALID, "albedo_scale_median: render_albedo, gt_albedo, scratch, scale3 and count must be provided");
    hipStream_t s = (hipStream_t)stream;
    StageMarks tm = stage_begin(s);
    uint32_t* scr = (uint32_t*)scratch;
    const AlbedoSource src{render_albedo, gt_albedo, lo, hi, (int)(render_srgb != 0), (uint32_t)((long long)W * H), 3};
    launch_passes(src, scr, s);
    hipLaunchKernelGGL(albedo_median_finish_kernel, dim3(1), dim3(BLOCK), 0, s, (const uint32_t*)scr, scale3, count);
    stage_mark(tm, "albedo_scale_median");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SVGIR_OK : report_error(SVGIR_ERR_HIP, "albedo_scale_median launch failed: %s", hipGetErrorString(e));
}

size_t svgir_surface_center_loss_partials(int64_t P) {
    if (P < 0 || P > SEL_MAX_N) return 0;
    return SEL_WORDS / 2 + (size_t)select_blocks(P);   // the selection's scratch in front, then one double per workgroup
}

int svgir_surface_center_loss_forward(int64_t P, const float* xyz, double* partial, double* stats, float* loss, void* stream) {
    if (P < 0 || P > SEL_MAX_N) return report_error(SVGIR_ERR_INVALID, "surface_center_loss_forward: P = %lld is outside 0 ... 2^31 - 1", (long long)P);
    if (!stats || !loss || (P > 0 && (!xyz || !partial)))
        return report_error(SVGIR_ERR_INVALID, "surface_center_loss_forward: xyz, partial, stats and loss must be provided");
    hipStream_t s = (hipStream_t)stream;
    StageMarks tm = stage_begin(s);
    uint32_t* scr = (uint32_t*)partial;
    double* rec = partial ? partial + SEL_WORDS / 2 : nullptr;
    const unsigned blocks = select_blocks(P);
    if (P > 0) {
        const ColumnSource src{xyz, 3, 1, (uint32_t)P, 3};
        launch_passes(src, scr, s);
        hipLaunchKernelGGL(surface_center_fwd_kernel, dim3(blocks), dim3(BLOCK), 0, s, src, scr, rec);
    }
    hipLaunchKernelGGL(surface_center_reduce_kernel, dim3(1), dim3(256), 0, s, (const uint32_t*)scr, (const double*)rec, (int)blocks, (double)P,
                       stats, loss);
    stage_mark(tm, "surface_center_fwd");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SVGIR_OK : report_error(SVGIR_ERR_HIP, "surface_center_loss_forward launch failed: %s", hipGetErrorString(e));
}

int svgir_surface_center_loss_backward(int64_t P, const float* xyz, const double* stats, const float* g, float* dL_dxyz, void* stream) {
    if (P < 0 || P > SEL_MAX_N) return report_error(SVGIR_ERR_INVALID, "surface_center_loss_backward: P = %lld is outside 0 ... 2^31 - 1", (long long)P);
    if (P > 0 && (!xyz || !stats || !g || !dL_dxyz))
        return report_error(SVGIR_ERR_INVALID, "surface_center_loss_backward: xyz, stats, g and dL_dxyz must be provided");
    if (P == 0) return SVGIR_OK;
    hipStream_t s = (hipStream_t)stream;
    StageMarks tm = stage_begin(s);
    hipLaunchKernelGGL(surface_center_bwd_kernel, dim3((unsigned)((P + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, xyz, (long long)P, stats, g, dL_dxyz);
    stage_mark(tm, "surface_center_bwd");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SVGIR_OK : report_error(SVGIR_ERR_HIP, "surface_center_loss_backward launch failed: %s", hipGetErrorString(e));
}

}  // extern "C"
