// svg-ir_amd/csrc/knn.hip -- exact k-nearest-neighbour search over a point cloud (the simple_knn / custom_knn row).
//
// Replaces simple_knn's `distCUDA2` (submodules/simple-knn/simple_knn.cu:147-221: mean squared distance to the 3 nearest
// neighbours, the initial scales of create_from_pcd) and custom_knn's `topKdistCUDA2` (no source upstream: the 8 nearest
// neighbours' squared distances and indices of get_knn_loss).  Both are ONE search kernel, K = 3 and K = 8.
//
// The result is a pure function of the input (include/svgir_raster.h): candidates are ordered by the u64 key
// bits(dist) << 32 | original index, dist = (dx*dx + dy*dy) + dz*dz in fp32 without contraction; a NaN / +inf dist is no
// neighbour.  The spatial structure only prunes, and only conservatively: a box is skipped when its fp32 lower bound -- the
// same operations on the clamped difference, so by monotone rounding never above a contained point's dist -- is STRICTLY
// greater than the lane's current k-th distance.  Ties therefore never depend on the traversal.
//
// The structure: 30-bit Morton codes inside the box of the finite points, the rasterizer's radix sort, a Morton-ordered copy
// {x, y, z, original id} padded with NaN points to whole groups of 64, one box per 64 sorted points (fine) and one per 64 fine
// boxes (coarse).  One wave serves 64 consecutive sorted queries: it takes its own fine box first (that seeds every lane's k-th
// bound), then walks the coarse boxes outward from its own in Morton order and the fine boxes of every coarse box some lane still
// needs (ballot).  A visited fine box is loaded once, one point per lane, and broadcast lane by lane (readlane): all 64 queries
// update their k-best in registers.  Every loop bound is a box count: nothing spins on degenerate clouds, and nothing waits on
// the host.
#include <algorithm>
#include <cfloat>

#include "common.hpp"
#include "lbvh.hpp"

namespace svgir {

namespace {

constexpr int KNN_GROUP = 64;              // sorted points per fine box = queries per wave
constexpr int KNN_FAN = 64;                // fine boxes per coarse box
constexpr uint32_t KNN_INF = 0x7f800000u;  // bits(+inf): a dist below it (as an integer) is finite, and neither NaN nor negative

struct KnnLayout {
    uint32_t* whole;      // [8] box of the finite points as order-preserving integers
    uint32_t* key[2];     // [P] Morton codes ping/pong
    uint32_t* val[2];     // [P] point ids ping/pong (val[0] = Morton order once sorted)
    uint32_t* radix_tbl;  // radix scratch
    float4* pts;          // [nf * 64] {x, y, z, bits(id)} in Morton order; the tail is {NaN, NaN, NaN, ~0}
    float4* fine;         // [nf][2] {lo.xyz, hi.x} {hi.yz, -, -} over the finite points of the group (none: lo = +inf, hi = -inf)
    float4* coarse;       // [nc][2] the same over 64 fine boxes
    int nf, nc;
    size_t bytes;
};
KnnLayout knn_layout(char* base, int P) {
    KnnLayout k;
    BlobCursor c{base};
    const size_t p = (size_t)(P > 0 ? P : 1);
    k.nf = (int)((p + KNN_GROUP - 1) / KNN_GROUP);
    k.nc = (k.nf + KNN_FAN - 1) / KNN_FAN;
    k.whole = c.take<uint32_t>(32);
    k.key[0] = c.take<uint32_t>(p * 4); k.key[1] = c.take<uint32_t>(p * 4);
    k.val[0] = c.take<uint32_t>(p * 4); k.val[1] = c.take<uint32_t>(p * 4);
    k.radix_tbl = c.take<uint32_t>(radix_table_words(P) * 4);
    k.pts = c.take<float4>((size_t)k.nf * KNN_GROUP * 16);
    k.fine = c.take<float4>((size_t)k.nf * 32);
    k.coarse = c.take<float4>((size_t)k.nc * 32);
    k.bytes = c.off;
    return k;
}

__device__ __forceinline__ bool knn_finite(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;   // (false for NaN)
}

// ---- whole box of the finite points (a point at infinity would flatten every Morton code to one cell) ---------------------------
// A fixed, small grid that strides over the points: whole_box_add is one atomic per wave and component on six addresses, and one
// wave per 64 points made this the longest kernel in front of the search (214 us at P = 200 k).
constexpr int KNN_WHOLE_BLOCKS = 64;
__global__ void __launch_bounds__(BLOCK) knn_whole_kernel(int P, const float* __restrict__ points, uint32_t* __restrict__ whole) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < (size_t)P; i += (size_t)gridDim.x * BLOCK) {
        const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
        if (knn_finite(p[0], p[1], p[2])) {
#pragma unroll
            for (int c = 0; c < 3; c++) { lo[c] = fminf(lo[c], p[c]); hi[c] = fmaxf(hi[c], p[c]); }
        }
    }
    whole_box_add(lo, hi, whole);
}

// ---- 30-bit Morton codes; an axis without extent, or a non-finite point, lands in cell 0 (the code only orders the search) ------
__global__ void __launch_bounds__(BLOCK) knn_morton_kernel(int P, const float* __restrict__ points, const uint32_t* __restrict__ whole,
                                                           uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P) return;
    uint32_t code = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float wl = ord2f(whole[c]), wu = ord2f(whole[3 + c]);
        float p = (points[3 * (size_t)i + c] - wl) / (wu - wl);
        p = fminf(fmaxf(p * 1024.0f, 0.0f), 1023.0f);   // (fmaxf drops a NaN: 0)
        code |= expand_bits((uint32_t)p) << c;
    }
    keys[i] = code;
    vals[i] = (uint32_t)i;
}

// wave reduce of a box; every lane ends with the result
__device__ __forceinline__ void knn_wave_box(float lo[3], float hi[3]) {
#pragma unroll
    for (int c = 0; c < 3; c++) { lo[c] = wave_reduce_min(lo[c]); hi[c] = wave_reduce_max(hi[c]); }
}

// ---- Morton-ordered copy of the points + one box per 64 of them (a wave = a group) ------------------------------------------------
__global__ void __launch_bounds__(BLOCK) knn_gather_kernel(int P, int nf, const uint32_t* __restrict__ id, const float* __restrict__ points,
                                                           float4* __restrict__ pts, float4* __restrict__ fine) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (size_t)nf * KNN_GROUP) return;   // (whole waves leave: BLOCK is a multiple of the group)
    float4 q = make_float4(NAN, NAN, NAN, __builtin_bit_cast(float, 0xffffffffu));
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < (size_t)P) {
        const uint32_t g = id[i];
        q = make_float4(points[3 * (size_t)g], points[3 * (size_t)g + 1], points[3 * (size_t)g + 2], __builtin_bit_cast(float, g));
        if (knn_finite(q.x, q.y, q.z)) { lo[0] = hi[0] = q.x; lo[1] = hi[1] = q.y; lo[2] = hi[2] = q.z; }
    }
    pts[i] = q;
    knn_wave_box(lo, hi);
    if ((threadIdx.x & 63) == 0) {
        const size_t f = i / KNN_GROUP;
        fine[2 * f] = make_float4(lo[0], lo[1], lo[2], hi[0]);
        fine[2 * f + 1] = make_float4(hi[1], hi[2], 0.f, 0.f);
    }
}

// ---- one box per 64 fine boxes (a wave = a coarse box) -----------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) knn_coarse_kernel(int nf, int nc, const float4* __restrict__ fine, float4* __restrict__ coarse) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (size_t)nc * KNN_FAN) return;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < (size_t)nf) {
        const float4 a = fine[2 * i], b = fine[2 * i + 1];
        lo[0] = a.x; lo[1] = a.y; lo[2] = a.z; hi[0] = a.w; hi[1] = b.x; hi[2] = b.y;
    }
    knn_wave_box(lo, hi);
    if ((threadIdx.x & 63) == 0) {
        const size_t c = i / KNN_FAN;
        coarse[2 * c] = make_float4(lo[0], lo[1], lo[2], hi[0]);
        coarse[2 * c + 1] = make_float4(hi[1], hi[2], 0.f, 0.f);
    }
}

// the contract's distance: fp32, this order, no contraction (the pragma: __fmul_rn / __fadd_rn are plain operators to the compiler
// and are fused like them)
__device__ __forceinline__ float knn_dist(float dx, float dy, float dz) {
#pragma clang fp contract(off)
    return (dx * dx + dy * dy) + dz * dz;
}
// lower bound of knn_dist over the points of a box: per axis the difference to the nearer face (0 inside), then the same operations.
// An empty box (lo = +inf) gives +inf, a non-finite query NaN or +inf: neither is ever wanted.
__device__ __forceinline__ float knn_box_bound(const float4 a, const float4 b, float x, float y, float z) {
    const float dx = fmaxf(fmaxf(a.x - x, x - a.w), 0.f), dy = fmaxf(fmaxf(a.y - y, y - b.x), 0.f), dz = fmaxf(fmaxf(a.z - z, z - b.y), 0.f);
    return (x == x && y == y && z == z) ? knn_dist(dx, dy, dz) : NAN;   // (fmaxf would drop a NaN query's difference)
}

template <int K>
struct KnnBest {
    unsigned long long k[K];   // ascending; an unused slot is {+inf, own id}: what topk reports for a missing neighbour
    __device__ __forceinline__ uint32_t kth_bits() const { return (uint32_t)(k[K - 1] >> 32); }
    // a box is wanted unless its bound is strictly greater than the k-th distance; +inf and NaN bounds hold no neighbour
    __device__ __forceinline__ bool wants(float bound) const {
        const uint32_t b = __builtin_bit_cast(uint32_t, bound);
        return b < KNN_INF && b <= kth_bits();
    }
    __device__ __forceinline__ void offer(float dist, uint32_t j) {
        const uint32_t b = __builtin_bit_cast(uint32_t, dist);
        unsigned long long key = ((unsigned long long)b << 32) | j;
        if (b < KNN_INF && key < k[K - 1]) {
#pragma unroll
            for (int s = 0; s < K; s++) {
                const unsigned long long old = k[s];
                const bool less = key < old;
                k[s] = less ? key : old;
                key = less ? old : key;
            }
        }
    }
};

// all 64 queries of the wave against the 64 points of group f
template <int K>
__device__ __forceinline__ void knn_visit(KnnBest<K>& best, const float4* __restrict__ pts, int f, float x, float y, float z, uint32_t me) {
    const float4 c = pts[(size_t)f * KNN_GROUP + (threadIdx.x & 63)];
    const int cx = __builtin_bit_cast(int, c.x), cy = __builtin_bit_cast(int, c.y), cz = __builtin_bit_cast(int, c.z), cw = __builtin_bit_cast(int, c.w);
#pragma unroll 8
    for (int l = 0; l < KNN_GROUP; l++) {
        const float px = __builtin_bit_cast(float, __builtin_amdgcn_readlane(cx, l)), py = __builtin_bit_cast(float, __builtin_amdgcn_readlane(cy, l)),
                    pz = __builtin_bit_cast(float, __builtin_amdgcn_readlane(cz, l));
        const uint32_t j = (uint32_t)__builtin_amdgcn_readlane(cw, l);
        const float d = knn_dist(px - x, py - y, pz - z);
        if (j != me) best.offer(d, j);   // (a padding point is NaN: never taken)
    }
}

// K = 3: out_mean[id]; K = 8: out_dist[id][8], out_idx[id][8].  One wave per workgroup, one workgroup per 64 sorted queries.
template <int K>
__global__ void __launch_bounds__(KNN_GROUP) knn_search_kernel(int P, int nf, int nc, const float4* __restrict__ pts, const float4* __restrict__ fine,
                                                               const float4* __restrict__ coarse, float* __restrict__ out_mean,
                                                               float* __restrict__ out_dist, int32_t* __restrict__ out_idx) {
    const int w = blockIdx.x;   // own group
    const float4 q = pts[(size_t)w * KNN_GROUP + threadIdx.x];
    const float x = q.x, y = q.y, z = q.z;
    const uint32_t me = __builtin_bit_cast(uint32_t, q.w);
    KnnBest<K> best;
#pragma unroll
    for (int s = 0; s < K; s++) best.k[s] = ((unsigned long long)KNN_INF << 32) | me;
    knn_visit<K>(best, pts, w, x, y, z, me);
    // coarse boxes outward from the own one: +0, -1, +1, -2, ... ; 2 nc steps cover every box from every start
    const int c0 = w / KNN_FAN;
    for (int step = 0; step < 2 * nc; step++) {
        const int c = (step & 1) ? c0 - ((step + 1) >> 1) : c0 + (step >> 1);
        if (c < 0 || c >= nc) continue;
        if (__ballot(best.wants(knn_box_bound(coarse[2 * c], coarse[2 * c + 1], x, y, z))) == 0) continue;
        const int f1 = min(nf, (c + 1) * KNN_FAN);
        for (int f = c * KNN_FAN; f < f1; f++) {
            if (f == w) continue;
            if (__ballot(best.wants(knn_box_bound(fine[2 * f], fine[2 * f + 1], x, y, z))) == 0) continue;
            knn_visit<K>(best, pts, f, x, y, z, me);
        }
    }
    if (me >= (uint32_t)P) return;   // padding lane
    if (K == 3) {
        // simple_knn.cu:154-182: missing neighbours stay FLT_MAX; ((b0 + b1) + b2) / 3 with a correctly rounded divide
        float b[3];
#pragma unroll
        for (int s = 0; s < 3; s++) {
            const uint32_t bits = (uint32_t)(best.k[s] >> 32);
            b[s] = bits == KNN_INF ? FLT_MAX : __builtin_bit_cast(float, bits);
        }
        out_mean[me] = ((b[0] + b[1]) + b[2]) / 3.0f;
    } else {
#pragma unroll
        for (int s = 0; s < K; s++) {
            out_dist[(size_t)me * K + s] = __builtin_bit_cast(float, (uint32_t)(best.k[s] >> 32));
            out_idx[(size_t)me * K + s] = (int32_t)(uint32_t)best.k[s];
        }
    }
}

// sort + structure + search on `s`; exactly one of out_mean / (out_dist, out_idx) is set
int knn_run(int P, const float* points, float* out_mean, float* out_dist, int32_t* out_idx, char* work, hipStream_t s) {
    const KnnLayout L = knn_layout(work, P);
    const int nb = (P + BLOCK - 1) / BLOCK;
    if (hipMemsetAsync(L.whole, 0xff, 12, s) != hipSuccess || hipMemsetAsync(L.whole + 3, 0, 12, s) != hipSuccess ||
        hipMemsetAsync(radix_gtot(L.radix_tbl, P), 0, radix_gtot_words(P) * 4, s) != hipSuccess)
        return SVGIR_ERR_HIP;
    hipLaunchKernelGGL(knn_whole_kernel, dim3(std::min(nb, KNN_WHOLE_BLOCKS)), dim3(BLOCK), 0, s, P, points, L.whole);
    hipLaunchKernelGGL(knn_morton_kernel, dim3(nb), dim3(BLOCK), 0, s, P, points, L.whole, L.key[0], L.val[0]);
    launch_radix_sort(L.key, L.val, P, nullptr, LBVH_SORT_BITS, 8, L.radix_tbl, s);   // (four passes: sorted ids end in val[0])
    hipLaunchKernelGGL(knn_gather_kernel, dim3((unsigned)(((size_t)L.nf * KNN_GROUP + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, P, L.nf, L.val[0],
                       points, L.pts, L.fine);
    hipLaunchKernelGGL(knn_coarse_kernel, dim3((unsigned)(((size_t)L.nc * KNN_FAN + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, L.nf, L.nc, L.fine,
                       L.coarse);
    if (out_mean)
        hipLaunchKernelGGL(knn_search_kernel<3>, dim3(L.nf), dim3(KNN_GROUP), 0, s, P, L.nf, L.nc, L.pts, L.fine, L.coarse, out_mean, nullptr, nullptr);
    else
        hipLaunchKernelGGL(knn_search_kernel<8>, dim3(L.nf), dim3(KNN_GROUP), 0, s, P, L.nf, L.nc, L.pts, L.fine, L.coarse, nullptr, out_dist, out_idx);
    return hipGetLastError() == hipSuccess ? 0 : SVGIR_ERR_HIP;
}

}  // namespace

}  // namespace svgir

extern "C" {

size_t svgir_knn_bytes(int32_t P) { return svgir::knn_layout(nullptr, P).bytes; }

int svgir_knn_mean_dist(int32_t P, const float* points, float* out_mean, char* work, void* stream) {
    if (P < 0 || (P > 0 && (!points || !out_mean || !work))) return SVGIR_ERR_INVALID;
    if (P == 0) return 0;
    return svgir::knn_run(P, points, out_mean, nullptr, nullptr, work, (hipStream_t)stream);
}

int svgir_knn_topk(int32_t P, const float* points, float* out_dist, int32_t* out_idx, char* work, void* stream) {
    if (P < 0 || (P > 0 && (!points || !out_dist || !out_idx || !work))) return SVGIR_ERR_INVALID;
    if (P == 0) return 0;
    return svgir::knn_run(P, points, nullptr, out_dist, out_idx, work, (hipStream_t)stream);
}

}  // extern "C"
