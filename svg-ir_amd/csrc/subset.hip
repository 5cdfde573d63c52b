// svg-ir_amd/csrc/subset.hip -- "shade only what the rasterizer reads": selection of a view's working set of surfels.
//
// The reference shades all P surfels of the model for every view (gaussian_renderer/svgss.py:116-141: rendering_equation4 over every
// point, chunked by 100 k) although the only consumer of the result is the rasterizer call behind it (svgss.py:143-182), which reads the
// packed rows of the surfels that survive its culls (svgss forward.cu:267-395 per Gaussian, and the alpha threshold per pixel).  Here the
// working set of a view is made explicit as a PARTITION of 0..P-1: list[0 .. n) = the selected surfels in index order, list[P-1-j] = the
// j-th unselected one; the shading kernels walk the front (csrc/shade.hip, svgir_shade_params.subset), a small kernel zero-fills the
// output rows of the back, so every output is still written completely.
//   forward : selected <=> the surfel is a candidate of at least one 8x8 sub-tile (flag byte set by cull_kernel);
//   backward: selected <=> out_weights > 0 (every other surfel has exactly-zero dL_dfeatures / dL_dvfeatures rows).
// The selection is the project's one stream compaction (two launches: per-chunk counts, then every workgroup sums the counts in front of
// it and scatters); the mask scan of csrc/optim.hip is its front-only form.
#include <algorithm>

#include "common.hpp"

namespace svgir {

namespace {

// Sel: SelNonZero / SelPositive (common.hpp).  BACK: also list the unselected ids from the end, list[n-1-j] = the j-th of them; without
// it nothing is written beyond list[count).
template <class Sel>
__global__ void __launch_bounds__(BLOCK) select_count_kernel(Sel sel, int n, uint32_t* __restrict__ block_sums) {
    __shared__ uint32_t wsum[BLOCK / 64];
    const uint32_t s = select_count_chunk(sel, (int)blockIdx.x, n, wsum);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = s;
}

template <class Sel, bool BACK>
__global__ void __launch_bounds__(BLOCK) select_scatter_kernel(Sel sel, int n, const uint32_t* __restrict__ block_sums, int nblocks,
                                                               uint32_t* __restrict__ list, uint32_t* __restrict__ count_out) {
    __shared__ uint32_t psum[BLOCK / 64], wsum[BLOCK / 64];
    const int t = threadIdx.x;
    const uint32_t before = blocks_before<BLOCK / 64>(block_sums, (int)blockIdx.x, psum);
    const int base = blockIdx.x * SCAN_BLOCK_ELEMS + t * 8;
    uint32_t k[8], c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { k[i] = (base + i < n && sel(base + i)) ? 1u : 0u; c += k[i]; }
    uint32_t pos = before + block_excl_scan<BLOCK / 64>(c, wsum);   // selected elements in front of this thread's first
    uint32_t npos = (uint32_t)base - pos;                           // unselected ones in front of it
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (base + i >= n) break;
        if (k[i]) list[pos++] = (uint32_t)(base + i);
        else if (BACK) list[(uint32_t)n - 1u - npos++] = (uint32_t)(base + i);
    }
    if ((int)blockIdx.x == nblocks - 1 && t == BLOCK - 1) count_out[0] = pos;
}

// work_out: the chunk counts are written first (the count launch); null: `work` already holds them
template <class Sel, bool BACK>
void launch_select(Sel sel, int n, uint32_t* list, uint32_t* work_out, const uint32_t* work, uint32_t* count_dev, hipStream_t s) {
    if (n <= 0) return;
    const int nb = scan_blocks(n);
    if (work_out) hipLaunchKernelGGL(select_count_kernel<Sel>, dim3(nb), dim3(BLOCK), 0, s, sel, n, work_out);
    hipLaunchKernelGGL((select_scatter_kernel<Sel, BACK>), dim3(nb), dim3(BLOCK), 0, s, sel, n, work, nb, list, count_dev);
}

struct ZeroRows {
    float* ptr[6]; int row_floats[6]; int n;
};
// one wave per unselected surfel (grid-stride): its row in each of the `n` tensors is zeroed with consecutive lanes
__global__ void __launch_bounds__(BLOCK) zero_rows_kernel(const uint32_t* __restrict__ list, const uint32_t* __restrict__ count, int P,
                                                          const ZeroRows z) {
    const int lane = threadIdx.x & 63;
    const uint32_t nsel = min(*count, (uint32_t)P);
    const uint32_t nrest = (uint32_t)P - nsel;
    const uint32_t waves = gridDim.x * (BLOCK / 64);
    for (uint32_t j = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); j < nrest; j += waves) {
        const size_t g = list[(uint32_t)P - 1u - j];
        for (int t = 0; t < z.n; t++) {
            float* row = z.ptr[t] + g * (size_t)z.row_floats[t];
            for (int e = lane; e < z.row_floats[t]; e += 64) row[e] = 0.f;
        }
    }
}

}  // namespace

size_t partition_work_words(int P) { return (size_t)scan_blocks(P) + 2; }

void launch_partition(int P, const uint8_t* flags, const float* positive, uint32_t* list, uint32_t* work, uint32_t* count_dev, hipStream_t s) {
    if (flags) launch_select<SelNonZero, true>(SelNonZero{flags}, P, list, work, work, count_dev, s);
    else launch_select<SelPositive, true>(SelPositive{positive}, P, list, work, work, count_dev, s);
}

void launch_partition_scatter(int P, const float* positive, uint32_t* list, const uint32_t* work, uint32_t* count_dev, hipStream_t s) {
    launch_select<SelPositive, true>(SelPositive{positive}, P, list, nullptr, work, count_dev, s);
}

void launch_compact(int P, const uint8_t* flags, uint32_t* list, uint32_t* work, uint32_t* count_dev, hipStream_t s) {
    launch_select<SelNonZero, false>(SelNonZero{flags}, P, list, work, work, count_dev, s);
}

void launch_zero_rows(int P, const uint32_t* list, const uint32_t* count_dev, float* const* tensors, const int* row_floats, int n, hipStream_t s) {
    ZeroRows z;
    z.n = 0;
    for (int i = 0; i < n && z.n < 6; i++)
        if (tensors[i] && row_floats[i] > 0) { z.ptr[z.n] = tensors[i]; z.row_floats[z.n] = row_floats[i]; z.n++; }
    if (P <= 0 || z.n == 0) return;
    const int blocks = std::min((P + BLOCK / 64 - 1) / (BLOCK / 64), 256 * 8);
    hipLaunchKernelGGL(zero_rows_kernel, dim3(blocks), dim3(BLOCK), 0, s, list, count_dev, P, z);
}

}  // namespace svgir
