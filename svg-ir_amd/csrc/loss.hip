// svg-ir_amd/csrc/loss.hip -- image losses right behind the rasterizer: L1 and SSIM with the
// reference's 11 x 11 Gaussian window, forward and backward.
//
// Replaces `F.l1_loss(image, gt)` + `ssim(image, gt)` as the reference calls them after render_view
// (gaussian_renderer/svgss.py:281-289, render.py:150-151; utils/loss_utils.py:21-64: `gaussian(11, 1.5)`, zero-padded
// depthwise conv2d of img1, img2, img1^2, img2^2, img1 img2, the SSIM map with C1 = 0.01^2, C2 = 0.03^2, its mean).
// The reference runs 5 convolutions + ~15 element-wise kernels over [3,H,W] planes forward and their autograd adjoints
// backward (~40 launches, every intermediate map through HBM).  Here:
//   forward : one kernel, one 16 x 16 output tile per workgroup: both images are read once (26 x 26 tile with halo), the five
//             windowed moments are a separable pass through LDS, and the kernel emits per-workgroup partial sums of the SSIM
//             map and of |img1 - img2| plus -- for the backward -- the three partial-derivative maps of the SSIM map w.r.t. the
//             windowed moments of img1 (mu1, E[x^2], E[x y]);
//   backward: one kernel, the same tiling: dL/dimg1 = w * dmu1 + 2 img1 (w * de11) + img2 (w * de12) (the window is
//             symmetric and the padding is zero, so the adjoint of the convolution is the convolution) + the L1 sign term.
// Only img1 (the rendered image) gets a gradient; img2 is the ground truth.
#include "common.hpp"
#include "ssim_tile.hpp"

namespace svgir {

namespace {

__global__ void __launch_bounds__(LT * LT) ssim_fwd_kernel(const float* __restrict__ img1, const float* __restrict__ img2, int H, int W,
                                                           SsimWindow win, float* __restrict__ partial, float* __restrict__ dmaps) {
    __shared__ float sT[2][LW][LW + 1];   // img1, img2
    __shared__ float sH[5][LW][LT + 1];
    __shared__ float sRed[2][4];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int ch = blockIdx.z;
    const size_t N = (size_t)H * W;
    const float* a = img1 + ch * N;
    const float* b = img2 + ch * N;
    ssim_load_halo<2>(sT, H, W, [&](int q, size_t i) { return (q ? b : a)[i]; });
    __syncthreads();
    float m[5];
    ssim_moments(win, sT, sH, m);
    const int x = blockIdx.x * LT + tx, y = blockIdx.y * LT + ty;
    const bool valid = x < W && y < H;
    const SsimPixel p = ssim_pixel(m);
    const float S = p.S, A1 = p.A1, A2 = p.A2, iB1 = p.iB1, iB2 = p.iB2, mu1 = p.mu1, mu2 = p.mu2;
    float ssim = valid ? S : 0.f;
    float l1 = valid ? fabsf(sT[0][ty + LR][tx + LR] - sT[1][ty + LR][tx + LR]) : 0.f;
    if (dmaps && valid) {
        // d S / d(mu1, E[x^2], E[xy]) with sigma1 = E[x^2] - mu1^2, sigma12 = E[xy] - mu1 mu2
        const float de11 = -S * iB2;
        const float de12 = 2.f * A1 * (iB1 * iB2);
        const float dmu1 = 2.f * mu2 * A2 * (iB1 * iB2) - S * 2.f * mu1 * iB1 - de12 * mu2 - de11 * 2.f * mu1;
        const size_t o = (size_t)ch * N + (size_t)y * W + x;
        const size_t CN = (size_t)gridDim.z * N;
        dmaps[o] = dmu1; dmaps[CN + o] = de11; dmaps[2 * CN + o] = de12;
    }
    // workgroup partial sums (fixed order: wave DPP sums, then the four waves in order)
    float s[2] = {wave_sum(ssim), wave_sum(l1)};
    block_sum_ordered(s, sRed);
    if (threadIdx.x == 0) {
        const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[2 * blk] = s[0]; partial[2 * blk + 1] = s[1];
    }
}

__global__ void __launch_bounds__(LT * LT) ssim_bwd_kernel(const float* __restrict__ img1, const float* __restrict__ img2,
                                                           const float* __restrict__ dmaps, int H, int W, SsimWindow win,
                                                           float g_ssim, float g_l1, const float* __restrict__ g_dev,
                                                           float* __restrict__ dL_dimg1) {
    if (g_dev) { g_ssim *= g_dev[0]; g_l1 *= g_dev[1]; }   // upstream scalars still on the device (no host read-back)
    __shared__ float sM[3][LW][LW + 1];
    __shared__ float sH[3][LW][LT + 1];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int ch = blockIdx.z;
    const size_t N = (size_t)H * W, CN = (size_t)gridDim.z * N;
    ssim_load_halo<3>(sM, H, W, [&](int q, size_t i) { return dmaps[q * CN + (size_t)ch * N + i]; });
    __syncthreads();
    float c[3];
    ssim_window_pass<3>(win, sH, [&](int r, int k, float (&v)[3]) { v[0] = sM[0][r][k]; v[1] = sM[1][r][k]; v[2] = sM[2][r][k]; }, c);
    const int x = blockIdx.x * LT + tx, y = blockIdx.y * LT + ty;
    if (x >= W || y >= H) return;
    const size_t o = (size_t)ch * N + (size_t)y * W + x;
    const float u = img1[o], v = img2[o];
    const float d = u - v;
    const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);   // torch: sign(0) = 0
    dL_dimg1[o] = g_ssim * (c[0] + 2.f * u * c[1] + v * c[2]) + g_l1 * sgn;
}

// the two means from the per-tile partial sums: one workgroup, fixed order, double accumulation
__global__ void __launch_bounds__(256) ssim_reduce_kernel(const float* __restrict__ partial, int nblk, double inv, float* __restrict__ out2) {
    __shared__ double red[2][4];
    double s[2];
    block_reduce_records(partial, nblk, 2, s, red);
    if (threadIdx.x == 0) {
        out2[0] = (float)(s[0] * inv); out2[1] = (float)(s[1] * inv);
    }
}

}  // namespace

}  // namespace svgir

extern "C" {

size_t svgir_l1_ssim_partials(int32_t C, int32_t H, int32_t W) {
    return (size_t)C * ((H + svgir::LT - 1) / svgir::LT) * ((W + svgir::LT - 1) / svgir::LT);
}

int svgir_l1_ssim_forward(const float* img1, const float* img2, int32_t C, int32_t H, int32_t W, float* partial, float* dmaps,
                          float* means2, void* stream) {
    if (C <= 0 || H <= 0 || W <= 0 || !img1 || !img2 || !partial) return SVGIR_ERR_INVALID;
    const dim3 grid((W + svgir::LT - 1) / svgir::LT, (H + svgir::LT - 1) / svgir::LT, C);
    hipLaunchKernelGGL(svgir::ssim_fwd_kernel, grid, dim3(svgir::LT * svgir::LT), 0, (hipStream_t)stream, img1, img2, H, W,
                       svgir::ssim_window(), partial, dmaps);
    if (means2)
        hipLaunchKernelGGL(svgir::ssim_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, (int)(grid.x * grid.y * grid.z),
                           1.0 / ((double)C * (double)H * (double)W), means2);
    return hipGetLastError() == hipSuccess ? SVGIR_OK : SVGIR_ERR_HIP;
}

int svgir_l1_ssim_backward(const float* img1, const float* img2, const float* dmaps, int32_t C, int32_t H, int32_t W,
                           float g_ssim_mean, float g_l1_mean, const float* g_dev, float* dL_dimg1, void* stream) {
    if (C <= 0 || H <= 0 || W <= 0 || !img1 || !img2 || !dmaps || !dL_dimg1) return SVGIR_ERR_INVALID;
    const float inv = 1.f / ((float)C * (float)H * (float)W);   // both losses are means over all C H W elements
    const dim3 grid((W + svgir::LT - 1) / svgir::LT, (H + svgir::LT - 1) / svgir::LT, C);
    hipLaunchKernelGGL(svgir::ssim_bwd_kernel, grid, dim3(svgir::LT * svgir::LT), 0, (hipStream_t)stream, img1, img2, dmaps, H, W,
                       svgir::ssim_window(), g_ssim_mean * inv, g_l1_mean * inv, g_dev, dL_dimg1);
    return hipGetLastError() == hipSuccess ? SVGIR_OK : SVGIR_ERR_HIP;
}

}  // extern "C"
