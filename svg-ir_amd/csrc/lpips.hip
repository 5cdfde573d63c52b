// svg-ir_amd/csrc/lpips.hip -- LPIPS with the VGG16 backbone (lpipsPyTorch/modules/{lpips,networks,utils}.py; called as
// lpips(a, b, net_type='vgg') at train.py:398, eval_nvs.py:81, eval_relighting_tensoIR.py:370/375), forward only, fp32 throughout.
//
// Activations are CHANNELS-CONTIGUOUS ([image][y][x][c]); image 2 p is operand a of pair p, image 2 p + 1 operand b.  Every image runs
// through the same code with the same tiling whatever else the call holds, so its bits depend on nothing but its own pixels.
//   lpips_stem_kernel  : plane operands composed on load, (x - mean) / std, zero padding AFTER the z-score, conv1_1 (K = 27) + bias + ReLU
//                        on the VALU: a 16 x 16 pixel tile per workgroup, the 18 x 18 x 3 halo and the 27 x 64 weights in LDS.
//   lpips_conv_kernel  : the twelve other 3 x 3 / pad 1 convolutions as implicit GEMM on v_mfma_f32_32x32x2_f32.  A workgroup computes an
//                        8 x 16 pixel patch x 64 output channels; wave w owns rows 2 w, 2 w + 1 of the patch (M = 32 pixels) and both
//                        32-channel halves (two accumulators).  Per chunk of 16 input channels the patch's 10 x 18 halo and the
//                        9 x 64 x 16 weight block (pre-packed in that order) are staged in LDS once and reused by all nine taps.  Every
//                        64 input channels (K = 576) are ONE fmaf chain per output in a fixed order (chunk, tap, then channels
//                        0 4 1 5 2 6 3 7 | 8 12 ... of the chunk: a lane's ds_read_b128 feeds four MFMAs); the chains of the Cin / 64
//                        groups are added in order, the bias last, ReLU keeps NaN.
//   lpips_pool_kernel  : 2 x 2 / stride 2 max pool, floor sizes, NaN-propagating.
//   lpips_tap_kernel   : per pixel of a tapped layer and pair: n = sqrt(sum_c f^2) for both images, u = f / (n + 1e-10), the sum over c of
//                        w_c (u_a - u_b)^2; 16 lanes per pixel, xor butterflies; double sums per workgroup through block_sum_ordered.
//   lpips_reduce_kernel: one workgroup per pair: the records of each tap in a fixed order, the mean, the five taps and their sum.
// No atomics, no host wait, no allocation.
#include "common.hpp"
#include "plane_op.hpp"

namespace svgir {

int report_error(int code, const char* fmt, ...);   // api.hip

namespace {

constexpr int LP_CONVS = 13, LP_TAPS = 5, LP_MAX_IMG = 2 * SVGIR_METRIC_MAX_TERMS;
// torchvision's configuration D up to relu5_3
constexpr int LP_CIN[LP_CONVS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int LP_COUT[LP_CONVS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int LP_TAP_AFTER[LP_TAPS] = {1, 3, 6, 9, 12};   // relu1_2, relu2_2, relu3_3, relu4_3, relu5_3; a pool follows all but the last
constexpr int LP_TAP_C[LP_TAPS] = {64, 128, 256, 512, 512};
const char* const LP_STAGE[LP_CONVS] = {"lpips_conv1_1", "lpips_conv1_2", "lpips_conv2_1", "lpips_conv2_2", "lpips_conv3_1", "lpips_conv3_2",
                                        "lpips_conv3_3", "lpips_conv4_1", "lpips_conv4_2", "lpips_conv4_3", "lpips_conv5_1", "lpips_conv5_2",
                                        "lpips_conv5_3"};

constexpr int CV_PH = 8, CV_PW = 16;                       // pixel patch of a workgroup
constexpr int CV_N = 64;                                   // output channels of a workgroup
constexpr int CV_CK = 16;                                  // input channels per LDS stage
constexpr int CV_ST = 20;                                  // LDS row stride in floats: 16-byte aligned, 16 consecutive rows cover the 64 banks of a b128 read
constexpr int CV_HW = CV_PW + 2, CV_HALO = (CV_PH + 2) * CV_HW;
constexpr int CV_WBLOCK = 9 * CV_N * CV_CK;                // floats of one packed (Cout block, Cin chunk) weight block
constexpr int TAP_PIX = 64;                                // pixels per workgroup of the tap kernel

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));   // (a plain vector: the staging registers below must be promotable)

// the packed network: float offsets.  Stem weights [27][64] (k = c 9 + ky 3 + kx), the other weights [Cout / 64][Cin / 16][9][64][16]
struct LpipsLayout {
    size_t w[LP_CONVS], b[LP_CONVS], lin[LP_TAPS], total;
};
LpipsLayout lpips_layout() {
    LpipsLayout L{};
    size_t o = 0;
    for (int l = 0; l < LP_CONVS; l++) {
        L.w[l] = o; o += (size_t)LP_COUT[l] * LP_CIN[l] * 9;
        L.b[l] = o; o += (size_t)LP_COUT[l];
    }
    for (int k = 0; k < LP_TAPS; k++) { L.lin[k] = o; o += (size_t)LP_TAP_C[k]; }
    L.total = o;   // every offset is a multiple of 64 floats
    return L;
}

__device__ __forceinline__ float relu_nan(float v) { return v < 0.f ? 0.f : v; }                      // relu(NaN) = NaN
__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }      // NaN wins, as torch's max_pool2d

// ---- packing -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) lpips_pack_stem_kernel(const float* __restrict__ w, float* __restrict__ dst) {
    const int d = blockIdx.x * BLOCK + threadIdx.x;
    if (d >= 27 * 64) return;
    const int k = d >> 6, co = d & 63;
    dst[d] = w[co * 27 + k];
}
__global__ void __launch_bounds__(BLOCK) lpips_pack_conv_kernel(const float* __restrict__ w, int Cin, int Cout, float* __restrict__ dst) {
    const size_t d = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (d >= (size_t)Cout * Cin * 9) return;
    const int ci = (int)(d % CV_CK), co = (int)((d / CV_CK) % CV_N), tap = (int)((d / (CV_CK * CV_N)) % 9);
    const size_t blk = d / CV_WBLOCK;
    const int nchunk = Cin / CV_CK, ch = (int)(blk % nchunk), nb = (int)(blk / nchunk);
    dst[d] = w[((size_t)(nb * CV_N + co) * Cin + (size_t)(ch * CV_CK + ci)) * 9 + tap];
}
__global__ void __launch_bounds__(BLOCK) lpips_copy_kernel(const float* __restrict__ src, int n, float* __restrict__ dst) {
    const int d = blockIdx.x * BLOCK + threadIdx.x;
    if (d < n) dst[d] = src[d];
}

// ---- stem --------------------------------------------------------------------------------------------------------------------------
struct StemArgs {
    int W, H;
    svgir_plane_op op[LP_MAX_IMG];
    const float *wk, *bias;   // [27][64], [64]
    float* out;               // [n_img][H][W][64]
};

__global__ void __launch_bounds__(256) lpips_stem_kernel(const StemArgs a) {
    __shared__ float sIn[3][18][19];
    __shared__ __attribute__((aligned(16))) float sW[27 * 64];
    __shared__ __attribute__((aligned(16))) float sB[64];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int H = a.H, W = a.W, img = blockIdx.z;
    const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
    const size_t N = (size_t)H * W;
    const svgir_plane_op& op = a.op[img];
    for (int i = t; i < 3 * 18 * 18; i += 256) {
        const int c = i / 324, r = (i - c * 324) / 18, cc = i - c * 324 - r * 18;
        const int gy = y0 + r - 1, gx = x0 + cc - 1;
        float v = 0.f;   // the zero padding is applied to the z-scored image
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const float mean = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f), sd = c == 0 ? .458f : (c == 1 ? .448f : .450f);
            v = __fdiv_rn(__fsub_rn(compose(op, c, N, (size_t)gy * W + gx), mean), sd);
        }
        sIn[c][r][cc] = v;
    }
    for (int i = t; i < 27 * 64; i += 256) sW[i] = a.wk[i];
    if (t < 64) sB[t] = a.bias[t];
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    float* dst = a.out + (((size_t)img * H + y) * W + x) * 64;
    for (int p = 0; p < 4; p++) {
        float acc[16];
#pragma unroll
        for (int j = 0; j < 16; j++) acc[j] = 0.f;
#pragma unroll
        for (int k = 0; k < 27; k++) {
            const float v = sIn[k / 9][ty + (k % 9) / 3][tx + k % 3];
#pragma unroll
            for (int j = 0; j < 16; j++) acc[j] = fmaf(v, sW[k * 64 + p * 16 + j], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 16; j += 4) {
            float4 o;
            o.x = relu_nan(acc[j] + sB[p * 16 + j]); o.y = relu_nan(acc[j + 1] + sB[p * 16 + j + 1]);
            o.z = relu_nan(acc[j + 2] + sB[p * 16 + j + 2]); o.w = relu_nan(acc[j + 3] + sB[p * 16 + j + 3]);
            *(float4*)(dst + p * 16 + j) = o;
        }
    }
}

// ---- 3 x 3 convolution, implicit GEMM on the fp32-input MFMA -------------------------------------------------------------------------
// in [n_img][H][W][Cin], out [n_img][H][W][Cout]; Cin and Cout multiples of 64.  grid: (tiles_x * tiles_y, Cout / 64, n_img).
__global__ void __launch_bounds__(256) lpips_conv_kernel(const float* __restrict__ in, const float* __restrict__ wp,
                                                         const float* __restrict__ bias, float* __restrict__ out, int H, int W, int Cin,
                                                         int Cout, int tiles_x) {
    __shared__ __attribute__((aligned(16))) float sA[CV_HALO * CV_ST];       // [halo pixel][16 channels]
    __shared__ __attribute__((aligned(16))) float sB[9 * CV_N * CV_ST];      // [tap][output channel][16 channels]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int y0 = tile_y * CV_PH, x0 = tile_x * CV_PW, nb = blockIdx.y;
    const int nchunk = Cin / CV_CK;
    const float* src = in + (size_t)blockIdx.z * H * W * Cin;
    const int i = lane & 31, h = lane >> 5;
    const int prow = 2 * wave + (i >> 4), pcol = i & 15;
    f32x16 acc0, acc1, tot0, tot1;   // acc: the fmaf chain of the current group of four chunks (K = 576); tot: the groups, added in order
#pragma unroll
    for (int r = 0; r < 16; r++) { acc0[r] = 0.f; acc1[r] = 0.f; tot0[r] = 0.f; tot1[r] = 0.f; }

    // a thread's share of a stage: 3 float4 of the halo (720 in all, the last round partly idle) and 9 of the weight block.  All twelve
    // loads are issued before the first LDS store, so a stage costs one memory latency, not twelve
    constexpr int NA = (CV_HALO * 4 + 255) / 256, NB = CV_WBLOCK / 4 / 256;
    static_assert(NB * 256 * 4 == CV_WBLOCK, "the weight block is a whole number of rounds");
    long a_off[NA];   // float offset of the element in the image, chunk 0; -1: padding (or no element)
    int a_lds[NA];    // < 0: no element
#pragma unroll
    for (int j = 0; j < NA; j++) {
        const int q = t + 256 * j, p = q >> 2, v4 = q & 3, r = p / CV_HW, c = p - r * CV_HW;
        const int gy = y0 + r - 1, gx = x0 + c - 1;
        a_lds[j] = q < CV_HALO * 4 ? p * CV_ST + v4 * 4 : -1;
        a_off[j] = (q < CV_HALO * 4 && gy >= 0 && gy < H && gx >= 0 && gx < W) ? ((long)gy * W + gx) * Cin + v4 * 4 : -1;
    }
    for (int ch = 0; ch < nchunk; ch++) {
        f32x4 ra[NA], rb[NB];
#pragma unroll
        for (int j = 0; j < NA; j++) {
            ra[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (a_off[j] >= 0) ra[j] = *(const f32x4*)(src + a_off[j] + ch * CV_CK);
        }
        const float* wsrc = wp + (size_t)(nb * nchunk + ch) * CV_WBLOCK;
#pragma unroll
        for (int j = 0; j < NB; j++) rb[j] = *(const f32x4*)(wsrc + (size_t)(t + 256 * j) * 4);
        if (ch) __syncthreads();   // (the previous chunk's reads)
#pragma unroll
        for (int j = 0; j < NA; j++)
            if (a_lds[j] >= 0) *(f32x4*)&sA[a_lds[j]] = ra[j];
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const int q = t + 256 * j;
            *(f32x4*)&sB[(q >> 2) * CV_ST + (q & 3) * 4] = rb[j];
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const float* pa = &sA[((prow + tap / 3) * CV_HW + pcol + tap % 3) * CV_ST + 4 * h];
            const float* pb = &sB[(tap * CV_N + i) * CV_ST + 4 * h];
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const float4 va = *(const float4*)(pa + 8 * s);
                const float4 b0 = *(const float4*)(pb + 8 * s), b1 = *(const float4*)(pb + 32 * CV_ST + 8 * s);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va.x, b0.x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(va.x, b1.x, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va.y, b0.y, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(va.y, b1.y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va.z, b0.z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(va.z, b1.z, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va.w, b0.w, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(va.w, b1.w, acc1, 0, 0, 0);
            }
        }
        if ((ch & 3) == 3) {   // (Cin is a multiple of 64 in every layer: no group is left open)
#pragma unroll
            for (int r = 0; r < 16; r++) { tot0[r] += acc0[r]; tot1[r] += acc1[r]; acc0[r] = 0.f; acc1[r] = 0.f; }
        }
    }
    // C/D map of the 32 x 32 forms: column (output channel) = lane & 31, row (pixel of the wave's 2 x 16) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int co = nb * CV_N + i;
    const float bias0 = bias[co], bias1 = bias[co + 32];
    float* dst = out + (size_t)blockIdx.z * H * W * Cout;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int m = (r & 3) + 8 * (r >> 2) + 4 * h;
        const int gy = y0 + 2 * wave + (m >> 4), gx = x0 + (m & 15);
        if (gy < H && gx < W) {
            float* o = dst + ((size_t)gy * W + gx) * Cout + co;
            o[0] = relu_nan(tot0[r] + bias0);
            o[32] = relu_nan(tot1[r] + bias1);
        }
    }
}

// ---- 2 x 2 max pool ------------------------------------------------------------------------------------------------------------------
// in [n_img][H][W][C] -> out [n_img][H / 2][W / 2][C]; one thread per four channels of an output pixel
__global__ void __launch_bounds__(BLOCK) lpips_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C, size_t total4) {
    const size_t d = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (d >= total4) return;
    const int C4 = C >> 2, Ho = H >> 1, Wo = W >> 1;
    const int c4 = (int)(d % C4);
    size_t p = d / C4;
    const int xo = (int)(p % Wo); p /= Wo;
    const int yo = (int)(p % Ho);
    const size_t img = p / Ho;
    const float* s = in + ((img * H + 2 * yo) * W + 2 * xo) * C + 4 * c4;
    const float4 a = *(const float4*)s, b = *(const float4*)(s + C), c = *(const float4*)(s + (size_t)W * C), e = *(const float4*)(s + (size_t)W * C + C);
    float4 o;
    o.x = max_nan(max_nan(a.x, b.x), max_nan(c.x, e.x)); o.y = max_nan(max_nan(a.y, b.y), max_nan(c.y, e.y));
    o.z = max_nan(max_nan(a.z, b.z), max_nan(c.z, e.z)); o.w = max_nan(max_nan(a.w, b.w), max_nan(c.w, e.w));
    *(float4*)(out + d * 4) = o;
}

// ---- tap -----------------------------------------------------------------------------------------------------------------------------
// sum over the 16 lanes of a pixel's group, in every lane of it
__device__ __forceinline__ float group16_sum(float v) {
    v += __shfl_xor(v, 8); v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
    return v;
}

// feat [2 n_pairs][HW][C], C = 64 V; grid (blocks of TAP_PIX pixels, n_pairs); partial [n_pairs][gridDim.x]
template <int V>
__global__ void __launch_bounds__(256) lpips_tap_kernel(const float* __restrict__ feat, const float* __restrict__ lin, int HW,
                                                        double* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double red[1][4];
    constexpr int C = 64 * V;
    const int t = threadIdx.x, g = t >> 4, l = t & 15;
    const float* fa = feat + (size_t)(2 * blockIdx.y) * HW * C;
    const float* fb = fa + (size_t)HW * C;
    float4 w[V];
#pragma unroll
    for (int v = 0; v < V; v++) w[v] = *(const float4*)(lin + 64 * v + 4 * l);
    double sum = 0.0;
    for (int it = 0; it < TAP_PIX / 16; it++) {
        const int p = blockIdx.x * TAP_PIX + it * 16 + g;
        const bool ok = p < HW;
        float4 x[V], y[V];
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int v = 0; v < V; v++) {
            x[v] = y[v] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) {
                x[v] = *(const float4*)(fa + (size_t)p * C + 64 * v + 4 * l);
                y[v] = *(const float4*)(fb + (size_t)p * C + 64 * v + 4 * l);
            }
            sx = (((sx + x[v].x * x[v].x) + x[v].y * x[v].y) + x[v].z * x[v].z) + x[v].w * x[v].w;
            sy = (((sy + y[v].x * y[v].x) + y[v].y * y[v].y) + y[v].z * y[v].z) + y[v].w * y[v].w;
        }
        const float dx = __fsqrt_rn(group16_sum(sx)) + 1e-10f, dy = __fsqrt_rn(group16_sum(sy)) + 1e-10f;
        float s = 0.f;
#pragma unroll
        for (int v = 0; v < V; v++) {
            float d;
            d = __fdiv_rn(x[v].x, dx) - __fdiv_rn(y[v].x, dy); s = s + w[v].x * (d * d);
            d = __fdiv_rn(x[v].y, dx) - __fdiv_rn(y[v].y, dy); s = s + w[v].y * (d * d);
            d = __fdiv_rn(x[v].z, dx) - __fdiv_rn(y[v].z, dy); s = s + w[v].z * (d * d);
            d = __fdiv_rn(x[v].w, dx) - __fdiv_rn(y[v].w, dy); s = s + w[v].w * (d * d);
        }
        s = group16_sum(s);
        if (ok && l == 0) sum += (double)s;
    }
    double r[1] = {wave_reduce_add(sum)};
    block_sum_ordered(r, red);
    if (t == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = r[0];
}

struct ReduceArgs {
    const double* partial[LP_TAPS];   // [n_pairs][nblk[k]]
    int nblk[LP_TAPS];
    double HW[LP_TAPS];
    float *taps, *score;
};
__global__ void __launch_bounds__(256) lpips_reduce_kernel(const ReduceArgs a) {
    __shared__ double red[1][4];
    const int pair = blockIdx.x;
    double tap[LP_TAPS];
    for (int k = 0; k < LP_TAPS; k++) {
        double s[1];
        if (k) __syncthreads();   // (red is written again)
        block_reduce_records(a.partial[k] + (size_t)pair * a.nblk[k], a.nblk[k], 1, s, red);
        tap[k] = s[0] / a.HW[k];
    }
    if (threadIdx.x == 0) {
        for (int k = 0; k < LP_TAPS; k++) a.taps[pair * LP_TAPS + k] = (float)tap[k];
        a.score[pair] = (float)((((tap[0] + tap[1]) + tap[2]) + tap[3]) + tap[4]);
    }
}

// [n_img][HW][C] -> [n_img][C][HW], for tests
__global__ void __launch_bounds__(BLOCK) lpips_nchw_kernel(const float* __restrict__ in, float* __restrict__ out, int HW, int C, size_t total) {
    const size_t d = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (d >= total) return;
    const int p = (int)(d % HW);
    const size_t q = d / HW;
    const int c = (int)(q % C);
    const size_t img = q / C;
    out[d] = in[(img * HW + p) * C + c];
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

// float offsets of the five partial arrays (doubles first) and the two activation buffers inside the workspace
struct WorkLayout {
    size_t partial[LP_TAPS];   // in doubles
    int nblk[LP_TAPS], Hk[LP_TAPS], Wk[LP_TAPS];
    size_t buf_off, buf_bytes, total;   // bytes
};
WorkLayout work_layout(int W, int H, int n_pairs) {
    WorkLayout L{};
    size_t o = 0;
    int h = H, w = W;
    for (int k = 0; k < LP_TAPS; k++) {
        L.Hk[k] = h; L.Wk[k] = w;
        L.nblk[k] = (int)(((size_t)h * w + TAP_PIX - 1) / TAP_PIX);
        L.partial[k] = o; o += (size_t)n_pairs * L.nblk[k];
        h >>= 1; w >>= 1;
    }
    L.buf_off = (o * sizeof(double) + 255) / 256 * 256;
    L.buf_bytes = ((size_t)2 * n_pairs * H * W * 64 * sizeof(float) + 255) / 256 * 256;   // the widest level: [n_img][H][W][64]
    L.total = L.buf_off + 2 * L.buf_bytes;
    return L;
}

// every launch's block count and every int pixel index: H W fits an int; the largest grids are the tap maps' copy (n_img H W 64 elements
// at level 0) and the convolutions' patches
bool lpips_size_ok(int W, int H, int n_pairs) {
    const size_t tiles1 = (size_t)((H + CV_PH - 1) / CV_PH) * (size_t)((W + CV_PW - 1) / CV_PW);
    return (size_t)H * W <= 0x7fffffffu && (H + 15) / 16 <= 65535 && tiles1 <= 0x7fffffffu &&
           ((size_t)2 * n_pairs * H * W * 64 + BLOCK - 1) / BLOCK <= 0x7fffffffu;
}

}  // namespace

}  // namespace svgir

using namespace svgir;

extern "C" {

size_t svgir_lpips_packed_floats(void) { return lpips_layout().total; }

int svgir_lpips_pack(const float* const conv_w[13], const float* const conv_b[13], const float* const lin_w[5], float* packed, void* stream) {
    if (!conv_w || !conv_b || !lin_w || !packed) return report_error(SVGIR_ERR_INVALID, "lpips_pack: conv_w, conv_b, lin_w and packed must be provided");
    if ((uintptr_t)packed & 15) return report_error(SVGIR_ERR_INVALID, "lpips_pack: packed must be 16-byte aligned");
    for (int l = 0; l < LP_CONVS; l++)
        if (!conv_w[l] || !conv_b[l]) return report_error(SVGIR_ERR_INVALID, "lpips_pack: convolution %d has no weight or no bias", l);
    for (int k = 0; k < LP_TAPS; k++)
        if (!lin_w[k]) return report_error(SVGIR_ERR_INVALID, "lpips_pack: linear layer %d has no weight", k);
    const LpipsLayout L = lpips_layout();
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(lpips_pack_stem_kernel, dim3(blocks_for(27 * 64)), dim3(BLOCK), 0, s, conv_w[0], packed + L.w[0]);
    for (int l = 0; l < LP_CONVS; l++) {
        if (l) hipLaunchKernelGGL(lpips_pack_conv_kernel, dim3(blocks_for((size_t)LP_COUT[l] * LP_CIN[l] * 9)), dim3(BLOCK), 0, s, conv_w[l],
                                  LP_CIN[l], LP_COUT[l], packed + L.w[l]);
        hipLaunchKernelGGL(lpips_copy_kernel, dim3(blocks_for(LP_COUT[l])), dim3(BLOCK), 0, s, conv_b[l], LP_COUT[l], packed + L.b[l]);
    }
    for (int k = 0; k < LP_TAPS; k++)
        hipLaunchKernelGGL(lpips_copy_kernel, dim3(blocks_for(LP_TAP_C[k])), dim3(BLOCK), 0, s, lin_w[k], LP_TAP_C[k], packed + L.lin[k]);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SVGIR_OK : report_error(SVGIR_ERR_HIP, "lpips_pack launch failed: %s", hipGetErrorString(e));
}

size_t svgir_lpips_work_bytes(int32_t W, int32_t H, int32_t n_pairs) {
    if (W < 16 || H < 16 || n_pairs < 1 || n_pairs > SVGIR_METRIC_MAX_TERMS || !lpips_size_ok(W, H, n_pairs)) return 0;
    return work_layout(W, H, n_pairs).total;
}

int svgir_lpips(int32_t W, int32_t H, int32_t n_pairs, const svgir_lpips_pair* pairs, const float* packed, void* work, float* taps,
                float* score, float* const* tap_maps, void* stream) {
    if (n_pairs < 1 || n_pairs > SVGIR_METRIC_MAX_TERMS)
        return report_error(SVGIR_ERR_INVALID, "lpips: n_pairs = %d, 1 ... %d pairs per call", n_pairs, SVGIR_METRIC_MAX_TERMS);
    if (W < 16 || H < 16)
        return report_error(SVGIR_ERR_INVALID, "lpips: image %d x %d is smaller than 16 x 16 (relu5_3 would be empty)", W, H);
    if (!pairs || !packed || !work || !taps || !score)
        return report_error(SVGIR_ERR_INVALID, "lpips: pairs, packed, work, taps and score must be provided");
    if (((uintptr_t)packed & 15) || ((uintptr_t)work & 15)) return report_error(SVGIR_ERR_INVALID, "lpips: packed and work must be 16-byte aligned");
    for (int p = 0; p < n_pairs; p++)
        for (const svgir_plane_op* o : {&pairs[p].a, &pairs[p].b})
            if (const char* why = check_op(*o)) return report_error(SVGIR_ERR_INVALID, "lpips: pair %d: %s", p, why);
    if (tap_maps)
        for (int k = 0; k < LP_TAPS; k++)
            if (!tap_maps[k]) return report_error(SVGIR_ERR_INVALID, "lpips: tap_maps, when given, holds five pointers; entry %d is NULL", k);
    const int n_img = 2 * n_pairs;
    if (!lpips_size_ok(W, H, n_pairs)) return report_error(SVGIR_ERR_INVALID, "lpips: image %d x %d exceeds the supported size", W, H);

    const LpipsLayout P = lpips_layout();
    const WorkLayout L = work_layout(W, H, n_pairs);
    double* partial = (double*)work;
    float* buf[2] = {(float*)((char*)work + L.buf_off), (float*)((char*)work + L.buf_off + L.buf_bytes)};
    hipStream_t s = (hipStream_t)stream;
    StageMarks tm = stage_begin(s);

    StemArgs st{};
    st.W = W; st.H = H; st.wk = packed + P.w[0]; st.bias = packed + P.b[0]; st.out = buf[0];
    for (int p = 0; p < n_pairs; p++) { st.op[2 * p] = pairs[p].a; st.op[2 * p + 1] = pairs[p].b; }
    hipLaunchKernelGGL(lpips_stem_kernel, dim3((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16), (unsigned)n_img), dim3(256), 0, s, st);
    stage_mark(tm, LP_STAGE[0]);

    int cur = 0, h = H, w = W, tap = 0;   // buf[cur] holds the activation at h x w
    for (int l = 1; l < LP_CONVS; l++) {
        const int tx = (w + CV_PW - 1) / CV_PW, ty = (h + CV_PH - 1) / CV_PH;
        hipLaunchKernelGGL(lpips_conv_kernel, dim3((unsigned)(tx * ty), (unsigned)(LP_COUT[l] / CV_N), (unsigned)n_img), dim3(256), 0, s,
                           (const float*)buf[cur], packed + P.w[l], packed + P.b[l], buf[cur ^ 1], h, w, LP_CIN[l], LP_COUT[l], tx);
        cur ^= 1;
        stage_mark(tm, LP_STAGE[l]);
        if (l != LP_TAP_AFTER[tap]) continue;
        const int C = LP_TAP_C[tap], HW = h * w;
        const dim3 tg((unsigned)L.nblk[tap], (unsigned)n_pairs);
        double* part = partial + L.partial[tap];
        const float* lin = packed + P.lin[tap];
        switch (C) {
            case 64: hipLaunchKernelGGL(lpips_tap_kernel<1>, tg, dim3(256), 0, s, (const float*)buf[cur], lin, HW, part); break;
            case 128: hipLaunchKernelGGL(lpips_tap_kernel<2>, tg, dim3(256), 0, s, (const float*)buf[cur], lin, HW, part); break;
            case 256: hipLaunchKernelGGL(lpips_tap_kernel<4>, tg, dim3(256), 0, s, (const float*)buf[cur], lin, HW, part); break;
            default: hipLaunchKernelGGL(lpips_tap_kernel<8>, tg, dim3(256), 0, s, (const float*)buf[cur], lin, HW, part); break;
        }
        if (tap_maps) {
            const size_t total = (size_t)n_img * C * HW;
            hipLaunchKernelGGL(lpips_nchw_kernel, dim3(blocks_for(total)), dim3(BLOCK), 0, s, (const float*)buf[cur], tap_maps[tap], HW, C, total);
        }
        stage_mark(tm, "lpips_tap");
        tap++;
        if (tap < LP_TAPS) {
            const size_t total4 = (size_t)n_img * (h >> 1) * (w >> 1) * (C >> 2);
            hipLaunchKernelGGL(lpips_pool_kernel, dim3(blocks_for(total4)), dim3(BLOCK), 0, s, (const float*)buf[cur], buf[cur ^ 1], h, w, C, total4);
            cur ^= 1; h >>= 1; w >>= 1;
            stage_mark(tm, "lpips_pool");
        }
    }
    ReduceArgs ra{};
    for (int k = 0; k < LP_TAPS; k++) {
        ra.partial[k] = partial + L.partial[k]; ra.nblk[k] = L.nblk[k]; ra.HW[k] = (double)L.Hk[k] * (double)L.Wk[k];
    }
    ra.taps = taps; ra.score = score;
    hipLaunchKernelGGL(lpips_reduce_kernel, dim3((unsigned)n_pairs), dim3(256), 0, s, ra);
    stage_mark(tm, "lpips_reduce");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SVGIR_OK : report_error(SVGIR_ERR_HIP, "lpips launch failed: %s", hipGetErrorString(e));
}

}  // extern "C"
