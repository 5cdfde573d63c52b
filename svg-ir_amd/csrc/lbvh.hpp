// svg-ir_amd/csrc/lbvh.hpp -- the linear BVH builder of both tracers (bvh.hip: visibility, pbgi.hip: radiance).
//
// A tracer computes its own element boxes and 30-bit Morton codes (the arithmetic is its reference's) between lbvh_begin and
// lbvh_finish; everything else is here: the storage (LbvhTree), the whole-box reduction, the sort (the rasterizer's radix sort,
// binning.hip), the Karras 2012 hierarchy and the bottom-up refit in ONE launch.  What differs per tracer is a `Keys` type (how two
// sorted keys are told apart, how a leaf is named) and a `Sink` type (what else the refit writes per node).
//
// The tree: per internal node one 64-byte record {box of child 0, box of child 1, child ids, parent link} -- a trace kernel
// fetches it once per visited node and has both slab tests from it.  The refit hands the boxes upward through the parents'
// records with one device-scope acquire-release arrival counter per node: no second pass lays the child boxes out.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace svgir {

// order-preserving float <-> uint (for atomicMin / atomicMax on floats)
__device__ __forceinline__ uint32_t f2ord(float f) {
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o) {
    return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
// 10 bits -> every third bit of 30
__device__ __forceinline__ uint32_t expand_bits(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
// The codes are sorted on their 30 bits in four 8-bit passes: an even number, so the sorted keys / values END IN SLOT 0 of the
// ping/pong buffers they started in (launch_radix_sort, common.hpp).
constexpr int LBVH_SORT_BITS = 30;

// bump allocator over a blob; base == nullptr only sizes
struct BlobCursor {
    char* base;
    size_t off = 0;
    template <class T> T* take(size_t bytes) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += align_up(bytes);
        return p;
    }
};

struct LbvhTree {
    float* box;             // [P][6] element boxes lower.xyz, upper.xyz (element order)
    uint32_t* whole;        // [8] whole box as order-preserving integers: min xyz, max xyz
    uint32_t* key[2];       // [P] Morton codes ping/pong
    uint32_t* val[2];       // [P] element ids ping/pong (val[0] = Morton order once sorted)
    uint32_t* radix_tbl;    // radix scratch
    float4* pair;           // [P-1][4]: {lo0.xyz, hi0.x} {hi0.yz, lo1.xy} {lo1.z, hi1.xyz} {child0, child1, parent | slot << 31, -} (bits)
    uint32_t* leaf_parent;  // [P] internal node above the leaf of sorted position j | slot << 31
    uint32_t* arrive;       // [P-1] refit arrival counters
};
inline LbvhTree lbvh_tree_layout(BlobCursor& c, int P) {
    LbvhTree t;
    const size_t p = (size_t)(P > 0 ? P : 1);
    t.box = c.take<float>(p * 24);
    t.whole = c.take<uint32_t>(32);
    t.key[0] = c.take<uint32_t>(p * 4); t.key[1] = c.take<uint32_t>(p * 4);
    t.val[0] = c.take<uint32_t>(p * 4); t.val[1] = c.take<uint32_t>(p * 4);
    t.radix_tbl = c.take<uint32_t>(radix_table_words(P) * 4);
    t.pair = c.take<float4>(p * 64);
    t.leaf_parent = c.take<uint32_t>(p * 4);
    t.arrive = c.take<uint32_t>(p * 4);
    return t;
}

// the tail of a box kernel, reached by EVERY lane (lanes without an element bring the identity box): wave reduce, one atomic per
// wave and component
__device__ __forceinline__ void whole_box_add(const float lo[3], const float hi[3], uint32_t* __restrict__ whole) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float mn = wave_reduce_min(lo[c]), mx = wave_reduce_max(hi[c]);
        if ((threadIdx.x & 63) == 0) { atomicMin(&whole[c], f2ord(mn)); atomicMax(&whole[3 + c], f2ord(mx)); }
    }
}

// ---- Karras 2012 hierarchy on the sorted keys: thread i makes internal node i ------------------------------------------------
// Keys::delta(i, j) = length of the common prefix of the keys at sorted positions i and j, -1 for j outside [0, P); the keys are
// UNIQUE under it, so the two neighbours of an interior key never tie and node 0's range ends at P - 1.  Keys::leaf(j) = the id
// of the leaf of sorted position j (an internal node's id is its index).
template <class Keys>
__global__ void __launch_bounds__(BLOCK) lbvh_hierarchy_kernel(int P, Keys keys, float4* __restrict__ pair, uint32_t* __restrict__ leaf_parent) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P - 1) return;
    const int dl = keys.delta(i, i - 1), dr = keys.delta(i, i + 1);
    const int d = dr > dl ? 1 : -1;
    const int dmin = min(dl, dr);
    int lmax = 2;
    while (keys.delta(i, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int t = lmax >> 1; t > 0; t >>= 1)
        if (keys.delta(i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int first = min(i, j), last = max(i, j);
    // split: highest key bit that differs inside [first, last]
    const int dnode = keys.delta(first, last);
    int split = first, stride = last - first;
    do {
        stride = (stride + 1) >> 1;
        const int mid = split + stride;
        if (mid < last && keys.delta(first, mid) > dnode) split = mid;
    } while (stride > 1);
    // children: a leaf when the range ends there, internal node otherwise
    const bool lleaf = first == split, rleaf = last == split + 1;
    const uint32_t c0 = lleaf ? keys.leaf(split) : (uint32_t)split, c1 = rleaf ? keys.leaf(split + 1) : (uint32_t)(split + 1);
    // (component stores: .z of this record is written by the parent's thread)
    pair[4 * i + 3].x = __builtin_bit_cast(float, c0); pair[4 * i + 3].y = __builtin_bit_cast(float, c1);
    if (i == 0) pair[3].z = __builtin_bit_cast(float, 0xffffffffu);
    // parent links (slot in bit 31)
    if (lleaf) leaf_parent[split] = (uint32_t)i; else pair[4 * split + 3].z = __builtin_bit_cast(float, (uint32_t)i);
    if (rleaf) leaf_parent[split + 1] = (uint32_t)i | 0x80000000u;
    else pair[4 * (split + 1) + 3].z = __builtin_bit_cast(float, (uint32_t)i | 0x80000000u);
}

// ---- bottom-up refit: every leaf walks up; the second child to arrive at a node carries the union on -------------------------
// sink.leaf(j, lo, hi): the box of the leaf of sorted position j; sink.node(i, lo, hi, c0, c1): the box of internal node i (the
// union of its children's, in arrival order: min / max are exact) and its child ids.
struct LbvhNoSink {
    __device__ void leaf(int, const float*, const float*) const {}
    __device__ void node(uint32_t, const float*, const float*, uint32_t, uint32_t) const {}
};
template <class Sink>
__global__ void __launch_bounds__(BLOCK) lbvh_refit_kernel(int P, const uint32_t* __restrict__ id, const float* __restrict__ box, float4* pair,
                                                           const uint32_t* __restrict__ leaf_parent, uint32_t* arrive, Sink sink) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P) return;
    const uint32_t g = id[i];
    float lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { lo[c] = box[6 * g + c]; hi[c] = box[6 * g + 3 + c]; }
    sink.leaf(i, lo, hi);
    if (P == 1) return;   // (a lone leaf has no parent)
    uint32_t link = leaf_parent[i];
    for (int guard = 0; guard < 128; guard++) {
        const uint32_t parent = link & 0x7fffffffu;
        const int slot = (int)(link >> 31);
        float* f = reinterpret_cast<float*>(pair + 4 * (size_t)parent);
        float* mine = f + 6 * slot;
        // (write-through stores: plain ones stay dirty in L2 until the release below has to flush them -- measured at 200 k leaves,
        // 630 against 766 us for the whole refit)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            __hip_atomic_store(mine + c, lo[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(mine + 3 + c, hi[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // release our box / acquire the sibling's: device-scope acquire-release on the arrival counter
        const uint32_t old = __hip_atomic_fetch_add(&arrive[parent], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (old == 0) return;   // first to arrive: the sibling's thread finishes this node
        const float* s = f + 6 * (1 - slot);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            lo[c] = fminf(lo[c], __hip_atomic_load(s + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            hi[c] = fmaxf(hi[c], __hip_atomic_load(s + 3 + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
        sink.node(parent, lo, hi, __builtin_bit_cast(uint32_t, f[12]), __builtin_bit_cast(uint32_t, f[13]));
        link = __builtin_bit_cast(uint32_t, __hip_atomic_load(f + 14, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (link == 0xffffffffu) return;   // the root
    }
}

// ---- host side: lbvh_begin, then the tracer's box kernel (T.box, whole_box_add into T.whole) and Morton kernel (T.key[0],
// T.val[0]), then lbvh_finish -----------------------------------------------------------------------------------------------
inline bool lbvh_begin(const LbvhTree& T, int P, hipStream_t s) {
    return hipMemsetAsync(T.whole, 0xff, 12, s) == hipSuccess && hipMemsetAsync(T.whole + 3, 0, 12, s) == hipSuccess &&
           hipMemsetAsync(radix_gtot(T.radix_tbl, P), 0, radix_gtot_words(P) * 4, s) == hipSuccess &&
           hipMemsetAsync(T.arrive, 0, (size_t)P * 4, s) == hipSuccess;
}
// `keys` reads the SORTED codes / ids (T.key[0], T.val[0]).  A lone leaf (P == 1) has no hierarchy, and is refitted only for
// what a sink writes.
template <class Keys, class Sink>
void lbvh_finish(const LbvhTree& T, int P, Keys keys, Sink sink, hipStream_t s) {
    const int nb = (P + BLOCK - 1) / BLOCK;
    launch_radix_sort(T.key, T.val, P, nullptr, LBVH_SORT_BITS, 8, T.radix_tbl, s);
    if (P > 1) hipLaunchKernelGGL(lbvh_hierarchy_kernel, dim3(nb), dim3(BLOCK), 0, s, P, keys, T.pair, T.leaf_parent);
    if (P > 1 || !std::is_empty<Sink>::value)
        hipLaunchKernelGGL(lbvh_refit_kernel, dim3(nb), dim3(BLOCK), 0, s, P, T.val[0], T.box, T.pair, T.leaf_parent, T.arrive, sink);
}

}  // namespace svgir
