// oracle/bvh_oracle.cpp -- CPU restatement of the reference's surfel visibility tracer (submodules/bvh).
//
// TEST INFRASTRUCTURE ONLY (tests/, __graft_entry__.smoke()); the product never links or loads this file.
//
// Parity status.  The reference tracer is CUDA + thrust (src/*.cu): not buildable here, and the reference holds no tests or
// vectors for it => the per-ray arithmetic below is "parity unpinned" by the reference's own outputs.  What IS pinned by the
// reference run in the authoring container (scripts/make_golden_bvh.py -> tests/golden/bvh.npz): the leaf boxes, the
// argument order and the 0.05 origin offset of `RayTracer` (__init__.py:28-71, imported with a recording stub for `_C`).
//
// What it restates:
//   orc_bvh_leaf_boxes  __init__.py:30-58 (build_rotation utils/general_utils.py:82-103): box of the eight corners
//                       mean +- 3 s_a a +- 3 s_b b +- 3 s_c c.
//   orc_bvh_trace       trace_bvh_opacity_cuda (src/trace.cu:186-262) with ray_intersects / gaussian_fn of
//                       include/utility.cuh:35-121.  The reference walks a BVH, but a leaf is reached exactly when its own
//                       box passes the slab test (every ancestor's box contains it; only the root is entered untested), so
//                       the walk is restated as a loop over ALL surfels gated by the slab test of their leaf box -- no tree,
//                       nothing shared with the product's builder.  Surfels are taken in index order; the reference's order
//                       (tree order) only changes the rounding of the running product and the moment the 0.9 cut-off is met.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <omp.h>

namespace {

template <typename F>
inline void slab(const F* lo, const F* hi, const F* o, const F* d, F& tmin_out, F& tmax_out) {
    // utility.cuh:35-90 (divisions, thrust::swap, the two early returns {-1,-1})
    F tmin = (lo[0] - o[0]) / d[0], tmax = (hi[0] - o[0]) / d[0];
    if (tmin > tmax) { F t = tmin; tmin = tmax; tmax = t; }
    F tymin = (lo[1] - o[1]) / d[1], tymax = (hi[1] - o[1]) / d[1];
    if (tymin > tymax) { F t = tymin; tymin = tymax; tymax = t; }
    if (tmin > tymax || tymin > tmax) { tmin_out = -1; tmax_out = -1; return; }
    if (tymin > tmin) tmin = tymin;
    if (tymax < tmax) tmax = tymax;
    F tzmin = (lo[2] - o[2]) / d[2], tzmax = (hi[2] - o[2]) / d[2];
    if (tzmin > tzmax) { F t = tzmin; tzmin = tzmax; tzmax = t; }
    if (tmin > tzmax || tzmin > tmax) { tmin_out = -1; tmax_out = -1; return; }
    if (tzmin > tmin) tmin = tzmin;
    if (tzmax < tmax) tmax = tzmax;
    tmin_out = tmin; tmax_out = tmax;
}

// ---- decision margins (tests/tracer_cases.py: which rays sit on a threshold) ---------------------------------------------------
// A surfel counts for a ray when a conjunction of comparisons holds (the slab overlaps, tmax > 0, facing dot <= 0, t >= 0.01,
// power <= 0).  The margin of one comparison a ? b is |a - b| over the magnitude the rounding errors of a and b scale with:
// max(|box plane|, |origin|) / |direction| for slab distances, the sum of the absolute terms for the dot products and quadratic forms.
// A conjunction that holds is as safe as its weakest comparison; one that fails is as safe as its most clearly failing comparison.
// Comparisons between non-finite values (infinite slab planes, 0 / 0) are decided without rounding and carry no margin.
struct Conj {
    double pass_min = INFINITY, fail_max = -1;
    bool ok = true;
    void add(bool holds, double m) {
        if (holds) pass_min = std::fmin(pass_min, m);
        else { ok = false; fail_max = std::fmax(fail_max, m); }
    }
    double margin() const { return ok ? pass_min : fail_max; }
};
inline double rel_margin(double a, double sa, double b, double sb) {
    if (!std::isfinite(a) || !std::isfinite(b)) return INFINITY;
    const double s = std::fmax(std::fmax(sa, sb), 1e-300);
    return std::isfinite(s) ? std::fabs(a - b) / s : INFINITY;
}
template <typename F>
void slab_margin(const F* lo, const F* hi, const F* o, const F* d, Conj& cj) {
    // the five comparisons of slab() that decide (the swaps and the narrowing selects only order values) + trace.cu:250-262 tmax > 0
    double t0[3], t1[3], sc[3];
    for (int c = 0; c < 3; c++) {
        double a = (double)((lo[c] - o[c]) / d[c]), b = (double)((hi[c] - o[c]) / d[c]);
        if (a > b) std::swap(a, b);
        t0[c] = a; t1[c] = b;
        sc[c] = std::fmax(std::fmax(std::fabs((double)lo[c]), std::fabs((double)hi[c])), std::fabs((double)o[c])) / std::fabs((double)d[c]);
    }
    double tmin = t0[0], tmax = t1[0], smin = sc[0], smax = sc[0];
    cj.add(!(tmin > t1[1]), rel_margin(tmin, smin, t1[1], sc[1]));
    cj.add(!(t0[1] > tmax), rel_margin(t0[1], sc[1], tmax, smax));
    if (t0[1] > tmin) { tmin = t0[1]; smin = sc[1]; }
    if (t1[1] < tmax) { tmax = t1[1]; smax = sc[1]; }
    cj.add(!(tmin > t1[2]), rel_margin(tmin, smin, t1[2], sc[2]));
    cj.add(!(t0[2] > tmax), rel_margin(t0[2], sc[2], tmax, smax));
    if (t1[2] < tmax) { tmax = t1[2]; smax = sc[2]; }
    cj.add(tmax > 0, rel_margin(tmax, smax, 0.0, 0.0));
}

// The smallest margin of any decision of one ray: whether each surfel counts (every surfel, also behind the 0.9 cut-off: the kernel
// meets them in tree order), and the product of ALL counted factors against 0.9 (the partial products only fall, so the order in
// which the factors arrive decides nothing else).
template <typename F>
double ray_margin(int P, const float* boxes, const F* o, const F* d, const float* means, const float* cov, const float* opacity,
                  const float* normals) {
    double worst = INFINITY;
    F prod = 1;
    int count = 0;
    for (int g = 0; g < P; g++) {
        if (opacity[g] < 1.f / 255.f) continue;   // (an exact comparison of an input: no rounding in it)
        Conj cj;
        if (P > 1) {
            F lo[3], hi[3];
            for (int c = 0; c < 3; c++) { lo[c] = (F)boxes[6 * g + c]; hi[c] = (F)boxes[6 * g + 3 + c]; }
            slab_margin<F>(lo, hi, o, d, cj);
        }
        const F n[3] = {(F)normals[3 * g], (F)normals[3 * g + 1], (F)normals[3 * g + 2]};
        const double fd = (double)(n[0] * d[0] + n[1] * d[1] + n[2] * d[2]);
        const double fs = std::fabs((double)(n[0] * d[0])) + std::fabs((double)(n[1] * d[1])) + std::fabs((double)(n[2] * d[2]));
        cj.add(!(fd > 0), rel_margin(fd, fs, 0.0, 0.0));
        F c[6];
        for (int k = 0; k < 6; k++) c[k] = (F)cov[6 * g + k];
        const F m[3] = {(F)means[3 * g], (F)means[3 * g + 1], (F)means[3 * g + 2]};
        const F mm[3] = {m[0] - o[0], m[1] - o[1], m[2] - o[2]};
        const F C[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
        F t1 = 0, t2 = 0;
        double a1 = 0, a2 = 0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                t1 += C[i][j] * mm[i] * d[j]; a1 += std::fabs((double)(C[i][j] * mm[i] * d[j]));
                t2 += C[i][j] * d[i] * d[j]; a2 += std::fabs((double)(C[i][j] * d[i] * d[j]));
            }
        const F t = t1 / t2;
        const double ts = (a1 + std::fabs((double)t) * a2) / std::fabs((double)t2);
        cj.add(!((double)t < 0.01), rel_margin((double)t, ts, 0.01, 0.0));
        const F dd[3] = {m[0] - (o[0] + t * d[0]), m[1] - (o[1] + t * d[1]), m[2] - (o[2] + t * d[2])};
        F sum = 0;
        double as = 0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) { sum += dd[i] * dd[j] * C[i][j]; as += std::fabs((double)(dd[i] * dd[j] * C[i][j])); }
        const F power = (F)(-0.5 * (double)sum);
        cj.add(!(power > 0), rel_margin((double)sum, as, 0.0, 0.0));
        worst = std::fmin(worst, cj.margin());
        if (cj.ok) { count++; prod *= 1 - (F)opacity[g] * (F)std::exp((double)power); }
    }
    if (count) worst = std::fmin(worst, std::fabs((double)prod - 0.9) / 0.9);
    return worst;
}

template <typename F>
void trace(int P, const float* boxes, long long num_rays, const float* rays_o, const float* rays_d, float t_offset,
           const float* means, const float* cov, const float* opacity, const float* normals, int32_t* contribute,
           float* visibility, float* margin) {
#pragma omp parallel for schedule(dynamic, 16)
    for (long long r = 0; r < num_rays; r++) {
        F o[3], d[3];
        for (int c = 0; c < 3; c++) {
            d[c] = (F)rays_d[3 * r + c];
            // RayTracer.trace_visibility: rays_o + rays_d * 0.05 (fp32 tensor ops in the reference)
            o[c] = sizeof(F) == 4 ? (F)(rays_o[3 * r + c] + (float)(rays_d[3 * r + c] * t_offset))
                                  : (F)rays_o[3 * r + c] + d[c] * (F)t_offset;
        }
        int count = 0;
        F ray_opacity = 1;
        bool blocked = false;
        for (int g = 0; g < P && !blocked; g++) {
            if (P > 1) {   // (the root is entered without a test: a single surfel is always examined)
                F lo[3], hi[3], tmin, tmax;
                for (int c = 0; c < 3; c++) { lo[c] = (F)boxes[6 * g + c]; hi[c] = (F)boxes[6 * g + 3 + c]; }
                slab<F>(lo, hi, o, d, tmin, tmax);
                if (!(tmax > 0)) continue;   // trace.cu:250-262: a child is pushed when intersection.y > 0
            }
            if (opacity[g] < 1.f / 255.f) continue;                                              // trace.cu:222
            const F nx = (F)normals[3 * g], ny = (F)normals[3 * g + 1], nz = (F)normals[3 * g + 2];
            if (nx * d[0] + ny * d[1] + nz * d[2] > 0) continue;                                 // :224
            const F* dummy = nullptr; (void)dummy;
            F c[6];
            for (int k = 0; k < 6; k++) c[k] = (F)cov[6 * g + k];
            const F m[3] = {(F)means[3 * g], (F)means[3 * g + 1], (F)means[3 * g + 2]};
            const F mx = m[0] - o[0], my = m[1] - o[1], mz = m[2] - o[2];
            // utility.cuh:99-110
            const F t1 = c[0] * mx * d[0] + c[1] * mx * d[1] + c[2] * mx * d[2] + c[1] * my * d[0] + c[3] * my * d[1] + c[4] * my * d[2] +
                         c[2] * mz * d[0] + c[4] * mz * d[1] + c[5] * mz * d[2];
            const F t2 = c[0] * d[0] * d[0] + c[1] * d[0] * d[1] + c[2] * d[0] * d[2] + c[1] * d[1] * d[0] + c[3] * d[1] * d[1] +
                         c[4] * d[1] * d[2] + c[2] * d[2] * d[0] + c[4] * d[2] * d[1] + c[5] * d[2] * d[2];
            const F t = t1 / t2;
            if ((double)t < 0.01) continue;                                                      // :227 (0.01 is a double literal: the float is promoted)
            const F pos[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
            const F dx = m[0] - pos[0], dy = m[1] - pos[1], dz = m[2] - pos[2];
            // utility.cuh:113-120: -0.5 (double) * float sum, returned as float
            const F sum = dx * dx * c[0] + dy * dy * c[3] + dz * dz * c[5] + 2 * dx * dy * c[1] + 2 * dx * dz * c[2] + 2 * dy * dz * c[4];
            const F power = (F)(-0.5 * (double)sum);
            if (power > 0) continue;                                                             // :236
            count += 1;
            const F alpha = (F)opacity[g] * (sizeof(F) == 4 ? (F)expf((float)power) : (F)exp((double)power));
            ray_opacity *= 1 - alpha;
            if ((double)ray_opacity < 0.9) blocked = true;                                        // :240-243 (0.9: double literal)
        }
        contribute[r] = blocked ? 0 : count;          // the early return leaves the zero-initialised count (bvh.cu:97)
        visibility[r] = blocked ? 0.0f : (float)ray_opacity;
        if (margin) margin[r] = (float)ray_margin<F>(P, boxes, o, d, means, cov, opacity, normals);
    }
}

}  // namespace

extern "C" {

void orc_bvh_leaf_boxes(int P, const float* means, const float* scales, const float* rots, float* boxes) {
    for (int i = 0; i < P; i++) {
        float q[4] = {rots[4 * i], rots[4 * i + 1], rots[4 * i + 2], rots[4 * i + 3]};
        const float nrm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (int k = 0; k < 4; k++) q[k] = q[k] / nrm;
        const float r = q[0], x = q[1], y = q[2], z = q[3];
        const float R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)},
                               {2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)},
                               {2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)}};
        const float s[3] = {3 * scales[3 * i], 3 * scales[3 * i + 1], 3 * scales[3 * i + 2]};
        for (int c = 0; c < 3; c++) {
            float mn = 0, mx = 0;
            for (int k = 0; k < 8; k++) {
                // x111 = means3D + a*sa + b*sb + c*sc, ... (left to right)
                const float v = ((means[3 * i + c] + ((k & 4) ? 1.f : -1.f) * (R[c][0] * s[0])) + ((k & 2) ? 1.f : -1.f) * (R[c][1] * s[1])) +
                                ((k & 1) ? 1.f : -1.f) * (R[c][2] * s[2]);
                mn = k == 0 ? v : fminf(mn, v);
                mx = k == 0 ? v : fmaxf(mx, v);
            }
            boxes[6 * i + c] = mn; boxes[6 * i + 3 + c] = mx;
        }
    }
}

void orc_bvh_trace(int P, const float* boxes, long long num_rays, const float* rays_o, const float* rays_d, float t_offset,
                   const float* means, const float* cov_inv, const float* opacity, const float* normals, int32_t* contribute,
                   float* visibility, int fp64) {
    if (fp64) trace<double>(P, boxes, num_rays, rays_o, rays_d, t_offset, means, cov_inv, opacity, normals, contribute, visibility, nullptr);
    else trace<float>(P, boxes, num_rays, rays_o, rays_d, t_offset, means, cov_inv, opacity, normals, contribute, visibility, nullptr);
}

// The same trace + margin[num_rays]: the smallest relative margin of any decision of the ray (see Conj above), in the chosen precision.
void orc_bvh_trace_margin(int P, const float* boxes, long long num_rays, const float* rays_o, const float* rays_d, float t_offset,
                          const float* means, const float* cov_inv, const float* opacity, const float* normals, int32_t* contribute,
                          float* visibility, int fp64, float* margin) {
    if (fp64) trace<double>(P, boxes, num_rays, rays_o, rays_d, t_offset, means, cov_inv, opacity, normals, contribute, visibility, margin);
    else trace<float>(P, boxes, num_rays, rays_o, rays_d, t_offset, means, cov_inv, opacity, normals, contribute, visibility, margin);
}

}  // extern "C"
