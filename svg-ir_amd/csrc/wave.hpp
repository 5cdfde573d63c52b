// svg-ir_amd/csrc/wave.hpp -- wave64 and workgroup primitives shared by every kernel file (device code only; common.hpp includes it).
//
// Two contracts hold for everything below unless a helper says otherwise:
//   ALL LANES ACTIVE.  The helpers use DPP, ballots and the LDS crossbar: what they read from a lane that is switched off is not the
//     identity of the operation.  Call them from wave-uniform control flow only; a lane without an element takes part with the
//     identity (0 for sums, `valid = false` for wave_match).
//   BARRIERS.  A workgroup helper that takes an LDS array has exactly ONE __syncthreads(), between its write of that array and its reads;
//     every thread of the workgroup must reach it.  When it returns other waves may still be reading the array: the caller puts a
//     barrier in front of its next write to it (calling any helper again with the same array included).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#if defined(__HIPCC__)
namespace svgir {

// v of the lane the DPP control CTRL names, within the rows of ROWS; 0 where it names none
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ uint32_t dpp(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xf, false); }
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ float dpp(float v) { return __builtin_bit_cast(float, dpp<CTRL, ROWS>(__builtin_bit_cast(uint32_t, v))); }
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ unsigned long long dpp(unsigned long long v) {
    return (unsigned long long)dpp<CTRL, ROWS>((uint32_t)v) | ((unsigned long long)dpp<CTRL, ROWS>((uint32_t)(v >> 32)) << 32);
}
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) { return dpp<CTRL>(v); }

// THE inclusive wave64 scan (sum) on the VALU: DPP row shifts + row broadcasts (gfx9 family).  All 64 lanes must be active.
template <class T>
__device__ __forceinline__ T wave_incl_scan(T v) {
    v += dpp<0x111>(v);        // row_shr:1
    v += dpp<0x112>(v);        // row_shr:2
    v += dpp<0x114>(v);        // row_shr:4
    v += dpp<0x118>(v);        // row_shr:8
    v += dpp<0x142, 0xa>(v);   // row_bcast:15 -> rows 1, 3
    v += dpp<0x143, 0xc>(v);   // row_bcast:31 -> rows 2, 3
    return v;
}
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v) { return wave_incl_scan(v); }
// (u64: one 64-bit add per step -- the carry of the low half reaches the high half, packed counters must not overflow their fields)
__device__ __forceinline__ unsigned long long wave_incl_scan_u64(unsigned long long v) { return wave_incl_scan(v); }
__device__ __forceinline__ float wave_scan_last(float v) { return wave_incl_scan(v); }   // the total lands in lane 63
__device__ __forceinline__ float wave_sum(float v) {  // uniform result
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wave_scan_last(v)), 63));
}

// xor butterfly over the wave with an associative, commutative op; the result is in every lane.  T: anything __shfl_xor moves.
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, (T)__shfl_xor(v, d));
    return v;
}
template <class T>
__device__ __forceinline__ T wave_reduce_add(T v) { return wave_reduce(v, [](T a, T b) { return a + b; }); }
__device__ __forceinline__ uint32_t wave_reduce_max(uint32_t v) { return wave_reduce(v, [](uint32_t a, uint32_t b) { return max(a, b); }); }
__device__ __forceinline__ float wave_reduce_min(float v) { return wave_reduce(v, [](float a, float b) { return fminf(a, b); }); }
__device__ __forceinline__ float wave_reduce_max(float v) { return wave_reduce(v, [](float a, float b) { return fmaxf(a, b); }); }

// Ordering point for LDS traffic that is private to ONE wave (single-wave workgroups, or per-wave LDS regions): the DS
// operations of a wave execute in issue order, so only the compiler has to be kept from moving LDS accesses across it.
// Unlike __syncthreads() it does not drain vmcnt, i.e. it never waits for outstanding global atomics / stores.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Exclusive prefix of v over the WAVES * 64 threads of the workgroup (thread order); *total (may be null) = the sum over all of them.
// `incl` = the thread's inclusive wave scan of v.  wsum[WAVES]: see BARRIERS above.
template <int WAVES, class T>
__device__ __forceinline__ T block_excl_scan(T v, T incl, T* wsum, T* total = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    T woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) { const T x = wsum[w]; woff += w < wave ? x : (T)0; tot += x; }
    if (total) *total = tot;
    return woff + incl - v;
}
template <int WAVES, class T>
__device__ __forceinline__ T block_excl_scan(T v, T* wsum, T* total = nullptr) { return block_excl_scan<WAVES>(v, wave_incl_scan(v), wsum, total); }
// sum of v over the WAVES * 64 threads of the workgroup, in every thread.  lds[WAVES]: see BARRIERS.
template <int WAVES>
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* lds) {
    v = wave_reduce_add(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) s += lds[w];
    return s;
}
// THE fixed-order floating-point sum over the four waves of a 256-thread workgroup, N quantities at once, in every thread: w[q] comes in as
// the caller's own per-wave total (wave_sum or wave_reduce_add: the two give different float bits, so the wave step stays the caller's) and
// goes out as (wave 0 + wave 1) + (wave 2 + wave 3).  lds[N][4]: see BARRIERS.  The losses' bit-reproducibility rests on this one tree.
// (csrc/irradiance.hip's radiance loss keeps its own orders -- block_tree_sum's halving tree below and a serial wave loop: another order changes its bits.)
template <int N, class T>
__device__ __forceinline__ void block_sum_put(const T (&w)[N], T (*lds)[4]) {
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < N; q++) lds[q][threadIdx.x >> 6] = w[q];
    }
}
template <int N, class T>
__device__ __forceinline__ void block_sum_get(T (&w)[N], const T (*lds)[4]) {
#pragma unroll
    for (int q = 0; q < N; q++) w[q] = (lds[q][0] + lds[q][1]) + (lds[q][2] + lds[q][3]);
}
template <int N, class T>
__device__ __forceinline__ void block_sum_ordered(T (&w)[N], T (*lds)[4]) {
    block_sum_put(w, lds);
    __syncthreads();
    block_sum_get(w, lds);
}
// (quantities of two types behind the same single barrier)
template <int N, class T, int M, class U>
__device__ __forceinline__ void block_sum_ordered(T (&w)[N], T (*lds)[4], U (&u)[M], U (*ldu)[4]) {
    block_sum_put(w, lds); block_sum_put(u, ldu);
    __syncthreads();
    block_sum_get(w, lds); block_sum_get(u, ldu);
}
// The record reduction of ONE 256-thread workgroup: s[q] = the sum of column q of the n records rec[i * stride + q] (float or double), in
// every thread.  Thread t adds records t, t + 256, ... in double, then the xor butterfly, then the tree above.  lds[N][4]: see BARRIERS.
template <int N, class T>
__device__ __forceinline__ void block_reduce_records(const T* __restrict__ rec, int n, size_t stride, double (&s)[N], double (*lds)[4]) {
#pragma unroll
    for (int q = 0; q < N; q++) s[q] = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
#pragma unroll
        for (int q = 0; q < N; q++) s[q] += (double)rec[(size_t)i * stride + q];
    }
#pragma unroll
    for (int q = 0; q < N; q++) s[q] = wave_reduce_add(s[q]);
    block_sum_ordered(s, lds);
}
// THE halving tree over the THREADS threads of ONE workgroup: part[t] += part[t + h] for h = THREADS / 2 ... 1, every thread bringing `mine`;
// the sum comes back in every thread.  The tree's shape decides the bits: a call site keeps its THREADS and its T.  The array is the
// helper's own and there is no barrier in front of its first write: ONE call per kernel (a second one would overwrite part[] while
// slower threads still read the first result).
template <typename T, int THREADS>
__device__ __forceinline__ T block_tree_sum(T mine) {
    __shared__ T part[THREADS];
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int h = THREADS / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    return part[0];
}
// ... of n values in memory: thread t adds src[t], src[t + THREADS], ... in that order first
template <typename T, int THREADS, typename Count>
__device__ __forceinline__ T block_tree_sum(const T* __restrict__ src, Count n) {
    T t = 0;
    for (Count k = threadIdx.x; k < n; k += THREADS) t += src[k];
    return block_tree_sum<T, THREADS>(t);
}
// sum of block_sums[0 .. nbefore) -- the totals of the workgroups in front of this one -- in every thread
template <int WAVES>
__device__ __forceinline__ uint32_t blocks_before(const uint32_t* __restrict__ block_sums, int nbefore, uint32_t* lds) {
    uint32_t pre = 0;
    for (int b = threadIdx.x; b < nbefore; b += WAVES * 64) pre += block_sums[b];
    return block_sum<WAVES>(pre, lds);
}

// stable wave-level digit matching: the valid lanes of the wave that hold the same low `nbits` of `digit` as this lane (one ballot per
// bit).  Invalid lanes take part in the ballots -- nobody matches them -- and must not use their own result.
__device__ __forceinline__ unsigned long long wave_match(uint32_t digit, int nbits, bool valid) {
    unsigned long long same = __ballot(valid);
    for (int b = 0; b < nbits; b++) {
        const unsigned long long m = __ballot((digit >> b) & 1u);
        same &= ((digit >> b) & 1u) ? m : ~m;
    }
    return same;
}

}  // namespace svgir
#endif
