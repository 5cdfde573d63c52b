// svg-ir_amd/csrc/view_metrics.hip -- the tail of an eval view: per-view metrics, the 8-bit images that get written and
// the albedo scale of the relighting eval.
//
// Replaces what the reference runs after `render_fn` on every eval frame (eval_relighting_tensoIR.py:333-378; also eval_nvs.py:79,
// train.py:276-301) -- about sixty eager launches over 800 x 800 planes: a `x * mask + (1 - mask) * bg` composite per captured quantity,
// torchvision's `mul(255).add_(0.5).clamp_(0, 255).to(uint8)` behind an fp32 device-to-host copy per capture, psnr / ssim / mse on two image
// pairs and mse on the normals (utils/image_utils.py:32-37, utils/loss_utils.py:21-64) -- and, once per light, the boolean-indexed albedo
// scale that blocks the host (:284-294).  Here:
//   svgir_view_metrics : up to 4 operand pairs of one image size per call.  The operands are PLANE OPERANDS (include/svgir_raster.h):
//                        src, optional affine, optional mask composite over a constant or a fill plane, optional sRGB, composed ON LOAD in
//                        fp32 without contraction, so no composed plane ever exists in HBM and the value has the bits torch would hold.
//                        Terms with SSIM share the tiling and the SSIM arithmetic of csrc/loss.hip's ssim_fwd_kernel (csrc/ssim_tile.hpp:
//                        16 x 16 tile, 26 x 26 halo tile that is zero padding applied after composition); terms without are another
//                        instantiation that loads no halo and runs no LDS passes.  d = a - b in fp32; d^2 (exact in double) and |d| are summed in double per
//                        workgroup (wave reduction, then the four waves in order); one workgroup per term adds the records in a fixed order
//                        and writes the row of 10 doubles.
//   svgir_capture_u8   : up to 16 operands -> [n,H,W,3] bytes, (uint8) clamp((x * 255) + 0.5, 0, 255).  A thread owns 12 consecutive bytes
//                        (four pixels) behind the image's first 4-byte boundary: three dword stores; the bytes in front of that boundary
//                        and the last partial group are stored byte by byte.
//   svgir_albedo_scale : selection ((r + g) + b) / 3 > 0, per-channel double sums of clamp(gt / render, 1e-6, 1) and the count, reduced by
//                        one workgroup; the result stays on the device.
// No atomics, no host wait.
#include "common.hpp"
#include "plane_op.hpp"
#include "srgb.hpp"
#include "ssim_tile.hpp"

namespace svgir {

int report_error(int code, const char* fmt, ...);   // api.hip

namespace {

constexpr int VM_REC = 3;                             // doubles per workgroup record: sum d^2, sum |d|, sum of the SSIM map

struct MetricArgs {
    int W, H;
    int term[SVGIR_METRIC_MAX_TERMS];   // the terms of this launch: blockIdx.z = 3 * slot + channel
    svgir_metric_term t[SVGIR_METRIC_MAX_TERMS];
    double* partial;                    // [n_terms][3][tiles][VM_REC]
};

template <bool SSIM>
__global__ void __launch_bounds__(LT * LT) view_metrics_kernel(const MetricArgs a, const SsimWindow win) {
    __shared__ float sT[2][SSIM ? LW : 1][LW + 1];   // a, b
    __shared__ float sH[SSIM ? 5 : 1][SSIM ? LW : 1][LT + 1];
    __shared__ double sRed[2][4];
    __shared__ float sRedS[1][4];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, t = threadIdx.x;
    const int slot = blockIdx.z / 3, ch = blockIdx.z - 3 * slot;
    const int k = a.term[slot];
    const svgir_metric_term& T = a.t[k];
    const int H = a.H, W = a.W;
    const size_t N = (size_t)H * W;
    const int x = blockIdx.x * LT + tx, y = blockIdx.y * LT + ty;
    const bool valid = x < W && y < H;
    float u = 0.f, v = 0.f, ssim = 0.f;
    if constexpr (SSIM) {
        // (the zero padding is that of the COMPOSED operand)
        ssim_load_halo<2>(sT, H, W, [&](int q, size_t i) { return compose(q ? T.b : T.a, ch, N, i); });
        __syncthreads();
        float m[5];
        ssim_moments(win, sT, sH, m);
        ssim = valid ? ssim_pixel(m).S : 0.f;
        u = sT[0][ty + LR][tx + LR]; v = sT[1][ty + LR][tx + LR];
    } else if (valid) {
        u = compose(T.a, ch, N, (size_t)y * W + x);
        v = compose(T.b, ch, N, (size_t)y * W + x);
    }
    const float d = valid ? u - v : 0.f;
    // workgroup sums in a fixed order: the wave butterfly (the SSIM float: the DPP sum, as ssim_fwd_kernel), then the four waves in order
    double s[2] = {wave_reduce_add((double)d * (double)d), wave_reduce_add((double)fabsf(d))};
    float ss[1] = {ssim};
    if constexpr (SSIM) ss[0] = wave_sum(ssim);
    block_sum_ordered(s, sRed, ss, sRedS);
    if (t == 0) {
        const size_t tiles = (size_t)gridDim.x * gridDim.y;
        double* rec = a.partial + (((size_t)k * 3 + ch) * tiles + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * VM_REC;
        rec[0] = s[0]; rec[1] = s[1];
        rec[2] = SSIM ? (double)ss[0] : 0.0;
    }
}

// one workgroup per term: the records of its three channels in a fixed order, then the row
__global__ void __launch_bounds__(256) view_metrics_reduce_kernel(const double* __restrict__ partial, int tiles, double HW, int ssim_bits,
                                                                  double* __restrict__ rows) {
    __shared__ double red[VM_REC][4];
    const int k = blockIdx.x;
    double sq[3], ab[3], ss[3];
    for (int c = 0; c < 3; c++) {
        double s[VM_REC];
        if (c) __syncthreads();   // (red is written again)
        block_reduce_records(partial + ((size_t)k * 3 + c) * (size_t)tiles * VM_REC, tiles, VM_REC, s, red);
        sq[c] = s[0]; ab[c] = s[1]; ss[c] = s[2];
    }
    if (threadIdx.x == 0) {
        double* row = rows + (size_t)k * SVGIR_METRIC_COLS;
        double mse[3], psnr[3];
        for (int c = 0; c < 3; c++) {
            mse[c] = sq[c] / HW;
            psnr[c] = -10.0 * log10(mse[c]);   // = 20 log10(1 / sqrt(mse)); mse == 0: +inf
            row[c] = mse[c]; row[3 + c] = psnr[c];
        }
        row[6] = ((mse[0] + mse[1]) + mse[2]) / 3.0;
        row[7] = ((psnr[0] + psnr[1]) + psnr[2]) / 3.0;
        row[8] = ((ssim_bits >> k) & 1) ? ((ss[0] + ss[1]) + ss[2]) / (3.0 * HW) : __builtin_nan("");
        row[9] = ((ab[0] + ab[1]) + ab[2]) / (3.0 * HW);
    }
}

// ---- 8-bit captures ----------------------------------------------------------------------------------------------------------------
struct CaptureArgs {
    int W, H;
    svgir_plane_op op[SVGIR_CAPTURE_MAX];
    uint8_t* out;
};

// torchvision.utils.save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8); NaN -> 0 (include/svgir_raster.h)
__device__ __forceinline__ uint32_t quantise(float x) {
#pragma clang fp contract(off)
    const float v = (x * 255.f) + 0.5f;
    if (!(v > 0.f)) return 0u;          // negative, -inf, NaN
    return v > 255.f ? 255u : (uint32_t)v;   // the cast truncates
}

// byte j of image `op`: pixel j / 3, channel j % 3
__device__ __forceinline__ uint32_t capture_byte(const svgir_plane_op& op, size_t N, size_t j) {
    const size_t p = j / 3;
    return quantise(compose<false>(op, (int)(j - 3 * p), N, p));
}

__global__ void __launch_bounds__(BLOCK) capture_u8_kernel(const CaptureArgs a) {
    const svgir_plane_op& op = a.op[blockIdx.y];
    const size_t N = (size_t)a.W * a.H, L = 3 * N;            // bytes of one image
    uint8_t* base = a.out + (size_t)blockIdx.y * L;
    size_t head = (size_t)((4 - ((uintptr_t)base & 3)) & 3);  // bytes in front of the image's first 4-byte boundary
    if (head > L) head = L;
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t == 0)
        for (size_t j = 0; j < head; j++) base[j] = (uint8_t)capture_byte(op, N, j);
    const size_t start = head + 12 * t;
    if (start >= L) return;
    if (start + 12 <= L) {   // four pixels' worth of bytes, three aligned dwords
        uint32_t w[3];
#pragma unroll
        for (int q = 0; q < 3; q++) {
            w[q] = 0;
#pragma unroll
            for (int e = 0; e < 4; e++) w[q] |= capture_byte(op, N, start + 4 * q + e) << (8 * e);
        }
        uint32_t* dst = (uint32_t*)(base + start);
        dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2];
    } else {                 // the image's tail
        for (size_t j = start; j < L; j++) base[j] = (uint8_t)capture_byte(op, N, j);
    }
}

// ---- albedo scale ------------------------------------------------------------------------------------------------------------------
constexpr int AS_PER_THREAD = 4, AS_TILE = BLOCK * AS_PER_THREAD;   // pixels per workgroup
constexpr int AS_REC = 4;                                           // doubles per record: three ratio sums, the count

__global__ void __launch_bounds__(BLOCK) albedo_scale_kernel(const float* __restrict__ render, const float* __restrict__ gt, size_t N, int gt_srgb,
                                                             double* __restrict__ partial) {
    __shared__ double red[AS_REC][4];
    double s[3] = {0.0, 0.0, 0.0}, n = 0.0;
    for (int q = 0; q < AS_PER_THREAD; q++) {
        const size_t i = (size_t)blockIdx.x * AS_TILE + (size_t)q * BLOCK + threadIdx.x;
        if (i >= N) continue;
        const float r[3] = {render[i], render[N + i], render[2 * N + i]};
        if (!(__fdiv_rn((r[0] + r[1]) + r[2], 3.f) > 0.f)) continue;   // render_albedo.mean(dim=0) > 0
        n += 1.0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float g = gt[(size_t)c * N + i];
            if (gt_srgb) g = srgb(g);
            const float ratio = __fdiv_rn(g, r[c]);
            s[c] += (double)(ratio < 1e-6f ? 1e-6f : (ratio > 1.f ? 1.f : ratio));   // clamp(1e-6, 1), NaN passes
        }
    }
    double v[AS_REC] = {wave_reduce_add(s[0]), wave_reduce_add(s[1]), wave_reduce_add(s[2]), wave_reduce_add(n)};
    block_sum_ordered(v, red);
    if (threadIdx.x == 0)
        for (int c = 0; c < AS_REC; c++) partial[(size_t)blockIdx.x * AS_REC + c] = v[c];
}

__global__ void __launch_bounds__(256) albedo_scale_reduce_kernel(const double* __restrict__ partial, int nblk, float* __restrict__ scale3,
                                                                  int32_t* __restrict__ count) {
    __shared__ double red[AS_REC][4];
    double v[AS_REC];
    block_reduce_records(partial, nblk, AS_REC, v, red);
    if (threadIdx.x == 0) {
        for (int c = 0; c < 3; c++) scale3[c] = (float)(v[c] / v[3]);   // empty selection: 0 / 0 = NaN, torch's mean of nothing
        count[0] = (int32_t)v[3];
    }
}

}  // namespace

}  // namespace svgir

using namespace svgir;

extern "C" {

size_t svgir_view_metrics_partials(int32_t W, int32_t H, int32_t n_terms) {
    if (W <= 0 || H <= 0 || n_terms <= 0) return 0;
    return (size_t)n_terms * 3 * ((size_t)(H + LT - 1) / LT) * ((size_t)(W + LT - 1) / LT) * VM_REC;
}

int svgir_view_metrics(int32_t W, int32_t H, int32_t n_terms, const svgir_metric_term* terms, double* partial, double* rows, void* stream) {
    if (n_terms < 1 || n_terms > SVGIR_METRIC_MAX_TERMS)
        return report_error(SVGIR_ERR_INVALID, "view_metrics: n_terms = %d, 1 ... %d terms per call", n_terms, SVGIR_METRIC_MAX_TERMS);
    if (W <= 0 || H <= 0) return report_error(SVGIR_ERR_INVALID, "view_metrics: bad image size W=%d H=%d", W, H);
    if (!terms || !partial || !rows) return report_error(SVGIR_ERR_INVALID, "view_metrics: terms, partial and rows must be provided");
    for (int k = 0; k < n_terms; k++)
        for (const svgir_plane_op* p : {&terms[k].a, &terms[k].b})
            if (const char* why = check_op(*p)) return report_error(SVGIR_ERR_INVALID, "view_metrics: term %d: %s", k, why);
    const unsigned gx = (unsigned)((W + LT - 1) / LT), gy = (unsigned)((H + LT - 1) / LT);
    if (gy > 65535u) return report_error(SVGIR_ERR_INVALID, "view_metrics: image %d x %d exceeds the supported size", W, H);
    MetricArgs with{}, without{};
    int n_with = 0, n_without = 0, bits = 0;
    with.W = without.W = W; with.H = without.H = H; with.partial = without.partial = partial;
    for (int k = 0; k < n_terms; k++) {
        with.t[k] = without.t[k] = terms[k];
        if (terms[k].want_ssim) { with.term[n_with++] = k; bits |= 1 << k; }
        else without.term[n_without++] = k;
    }
    hipStream_t s = (hipStream_t)stream;
    StageMarks tm = stage_begin(s);
    const SsimWindow win = ssim_window();
    if (n_with) hipLaunchKernelGGL(view_metrics_kernel<true>, dim3(gx, gy, 3 * n_with), dim3(LT * LT), 0, s, with, win);
    if (n_without) hipLaunchKernelGGL(view_metrics_kernel<false>, dim3(gx, gy, 3 * n_without), dim3(LT * LT), 0, s, without, win);
    stage_mark(tm, "view_metrics");
    hipLaunchKernelGGL(view_metrics_reduce_kernel, dim3(n_terms), dim3(256), 0, s, partial, (int)(gx * gy), (double)W * (double)H, bits, rows);
    stage_mark(tm, "view_metrics_reduce");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SVGIR_OK : report_error(SVGIR_ERR_HIP, "view_metrics launch failed: %s", hipGetErrorString(e));
}

int svgir_capture_u8(int32_t W, int32_t H, int32_t n, const svgir_plane_op* ops, uint8_t* out, void* stream) {
    if (n < 1 || n > SVGIR_CAPTURE_MAX) return report_error(SVGIR_ERR_INVALID, "capture_u8: n = %d, 1 ... %d operands per call", n, SVGIR_CAPTURE_MAX);
    if (W <= 0 || H <= 0) return report_error(SVGIR_ERR_INVALID, "capture_u8: bad image size W=%d H=%d", W, H);
    if (!ops || !out) return report_error(SVGIR_ERR_INVALID, "capture_u8: ops and out must be provided");
    CaptureArgs a{};
    for (int k = 0; k < n; k++) {
        if (const char* why = check_op(ops[k])) return report_error(SVGIR_ERR_INVALID, "capture_u8: operand %d: %s", k, why);
        if (ops[k].srgb)
            return report_error(SVGIR_ERR_INVALID, "capture_u8: operand %d: srgb operands are not supported (powf differs from torch's pow by ulps; "
                                "no byte contract holds)", k);
        a.op[k] = ops[k];
    }
    a.W = W; a.H = H; a.out = out;
    const size_t L = 3 * (size_t)W * H;
    const size_t blocks = (L / 12 + 2 + BLOCK - 1) / BLOCK;   // one thread per 12 bytes behind the head, the tail's included
    if (blocks > 0x7fffffffu) return report_error(SVGIR_ERR_INVALID, "capture_u8: image %d x %d exceeds the supported size", W, H);
    hipStream_t s = (hipStream_t)stream;
    StageMarks tm = stage_begin(s);
    hipLaunchKernelGGL(capture_u8_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(BLOCK), 0, s, a);
    stage_mark(tm, "capture_u8");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SVGIR_OK : report_error(SVGIR_ERR_HIP, "capture_u8 launch failed: %s", hipGetErrorString(e));
}

size_t svgir_albedo_scale_partials(int32_t W, int32_t H) {
    if (W <= 0 || H <= 0) return 0;
    return (((size_t)W * H + AS_TILE - 1) / AS_TILE) * AS_REC;
}

int svgir_albedo_scale(int32_t W, int32_t H, const float* render_albedo, const float* gt_albedo, int32_t gt_srgb, double* partial,
                       float* scale3, int32_t* count, void* stream) {
    if (W <= 0 || H <= 0) return report_error(SVGIR_ERR_INVALID, "albedo_scale: bad image size W=%d H=%d", W, H);
    if (!render_albedo || !gt_albedo || !partial || !scale3 || !count)
        return report_error(SVGIR_ERR_INVALID, "albedo_scale: render_albedo, gt_albedo, partial, scale3 and count must be provided");
    const size_t N = (size_t)W * H, blocks = (N + AS_TILE - 1) / AS_TILE;
    if (blocks > 0x7fffffffu) return report_error(SVGIR_ERR_INVALID, "albedo_scale: image %d x %d exceeds the supported size", W, H);
    hipStream_t s = (hipStream_t)stream;
    StageMarks tm = stage_begin(s);
    hipLaunchKernelGGL(albedo_scale_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, s, render_albedo, gt_albedo, N, (int)gt_srgb, partial);
    hipLaunchKernelGGL(albedo_scale_reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, (int)blocks, scale3, count);
    stage_mark(tm, "albedo_scale");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SVGIR_OK : report_error(SVGIR_ERR_HIP, "albedo_scale launch failed: %s", hipGetErrorString(e));
}

}  // extern "C"
