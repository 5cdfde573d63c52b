/* include/svgir_raster.h -- C ABI of libsvgir_raster.so (MI355X / gfx950 surfel rasterizer).
 *
 * This is the drop-in boundary for the hot path of learner-shx/SVG-IR: it replaces the two
 * `CudaRasterizer::Rasterizer` classes that the reference's torch glue binds
 *     svgss_rasterization/cuda_rasterizer/rasterizer.h:24-115   (forward / backward / markVisible, "svgss")
 *     rgss-rasterization/cuda_rasterizer/rasterizer.h:24-104    (same, "rgss")
 * and that `svgss_rasterization/rasterize_points.cu:35-286` / `rgss-rasterization/rasterize_points.cu:36-264`
 * call with raw device pointers.  No torch, HIP or C++ types appear in the signatures: plain pointers, sizes and
 * a `void*` stream (a hipStream_t).  All pointers are DEVICE pointers unless stated otherwise.  All arithmetic
 * is fp32; images are CHW row-major; per-Gaussian tensors are row-major [P,k] exactly as the reference's.
 *
 * Errors: every entry point returns a negative svgir_status on failure and sets a thread-local message
 * retrievable with svgir_last_error() (the reference throws std::runtime_error / AT_ERROR instead,
 * rasterize_points.cu:65-67, rasterizer_impl.cu:264-267; the host bindings convert the code to RuntimeError).
 */
#ifndef SVGIR_RASTER_H_
#define SVGIR_RASTER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVGIR_ABI_VERSION 14

enum svgir_variant { SVGIR_RGSS = 0, SVGIR_SVGSS = 1 };

enum svgir_status {
    SVGIR_OK = 0,
    SVGIR_ERR_INVALID = -1,  /* bad shapes / missing inputs / unsupported channel counts */
    SVGIR_ERR_HIP = -2,      /* a HIP runtime call or kernel launch failed */
    SVGIR_ERR_ALLOC = -3     /* a blob allocation callback returned NULL */
};

/* Blob allocator: must return a device pointer to at least `bytes` bytes (256-byte aligned), valid until the
 * matching backward has run.  Replaces the reference's std::function<char*(size_t)> resize lambdas
 * (rasterize_points.cu:27-33). */
typedef char* (*svgir_alloc_fn)(size_t bytes, void* ctx);

typedef struct svgir_fused_shade svgir_fused_shade;   /* below, behind the shading entry points */

/* Inputs of one view.  Field-for-field the arguments of Rasterizer::forward
 * (svgss rasterizer_impl.cu:209-242, rgss :209-241). */
typedef struct svgir_params {
    int32_t variant;            /* svgir_variant */
    int32_t P;                  /* #Gaussians */
    int32_t S;                  /* #feature channels (svgss <= 50, rgss <= 33; Q9) */
    int32_t VS;                 /* #vfeature channels, multiple of 4, VS/4 <= 20 (svgss only) */
    int32_t D;                  /* active SH degree 0..3 */
    int32_t M;                  /* SH coefficients per colour channel in `shs` */
    int32_t W, H;               /* image size */
    const float* background;    /* [3] */
    const float* means3D;       /* [P,3] */
    const float* shs;           /* [P,M,3] or NULL */
    const float* colors_precomp;/* [P,3] or NULL (exactly one of shs / colors_precomp) */
    const float* features;      /* [P,S] or NULL when S == 0 */
    const float* vfeatures;     /* [P,VS] or NULL when VS == 0 */
    const float* opacities;     /* [P] */
    const float* scales;        /* [P,3] or NULL */
    const float* rotations;     /* [P,4] (r,x,y,z), NOT normalised in-kernel (Q3), or NULL */
    const float* cov3D_precomp; /* [P,6] or NULL (exactly one of scales+rotations / cov3D_precomp) */
    const float* viewmatrix;    /* [16] = W2C transposed (column-major W2C) */
    const float* projmatrix;    /* [16] = full projection, same convention */
    const float* cam_pos;       /* [3] */
    const float* prcppoint;     /* [2]  svgss; carried for API parity, unused by the arithmetic (Q11) */
    const float* patchbbox;     /* [4]  svgss: h0,w0,h1,w1 in pixels */
    const float* config;        /* [config_len] floats ON THE DEVICE, read by the kernels like the reference does;
                                   svgss: surface, normalize_depth, per_pixel_depth, (lrn_cam).  Entries >=
                                   config_len read as 0 (Q7: the reference reads config[3] out of bounds).
                                   rgss ignores it (compile-time {1,1,1} in the reference). */
    int32_t config_len;
    float scale_modifier;
    float tan_fovx, tan_fovy;
    float cx, cy;               /* rgss: principal point for surface_xyz */
    int32_t prefiltered;
    int32_t computer_pseudo_normal; /* rgss */
    int32_t backward_geometry;      /* rgss */
    int32_t debug;                  /* synchronise + check after every kernel (reference CHECK_CUDA) */
    void* features_ready;           /* optional (NULL: `features` / `vfeatures` are complete on `stream` at call time): a HIP
                                       event (hipEvent_t) recorded on ANOTHER stream that is still producing them.  Only the
                                       composite kernel of svgir_forward waits for it -- everything in front of the composite
                                       (preprocess, sorts, emit, ranges, cull) neither reads the features nor waits -- which
                                       is how the per-splat shading (svgir_shade_forward on a side stream) overlaps the
                                       binning of the same view.  Must stay alive until svgir_forward returns; ignored by
                                       svgir_backward.  (ABI 9: replaces the thread-local svgir_forward_wait_features of
                                       ABI 8 -- no state survives between calls.) */
    int32_t forward_only;           /* != 0 (ABI 12): no backward will follow (evaluation loops).  The composite keeps no blend states for
                                       the backward's depth segments -- nothing is dumped, the binning blob holds no state slots.  A
                                       svgir_backward on such a forward still works: it replays the composite once to produce them. */
    const svgir_fused_shade* shade; /* optional (svgss, ABI 12): the per-splat shading of this view, run INSIDE svgir_forward /
                                       svgir_backward for the surfels the view's composite actually reads (see svgir_fused_shade);
                                       `features` / `vfeatures` are then OUTPUT buffers of svgir_forward.  NULL: the caller shaded. */
    int32_t workload_scope;         /* (ABI 14) scope of the speculation history, 0 = the process-wide default.  svgir_forward sizes its
                                       speculative launches (instance capacity, state slots, three-pass depth sort) from the recent views of
                                       the same WORKLOAD = (device, W, H, S, VS, variant, workload_scope, Gaussian count within a factor of
                                       two).  Two models that share all of that and alternate in one process would feed one history: give
                                       each its own scope id.  Results never depend on it -- only how often a view's dependent stages are
                                       re-run.  See svgir_reset_workload_history. */
} svgir_params;

/* Outputs of forward.  Every buffer is written completely: the caller need not clear any of them (the reference's glue
 * hands zero-filled tensors to its kernels, rasterize_points.cu:76-88; here the kernels that run anyway write the zeros). */
typedef struct svgir_outputs {
    float* out_color;         /* [3,H,W] */
    float* out_normal;        /* [3,H,W] */
    float* out_depth;         /* [1,H,W] */
    float* out_opacity;       /* [1,H,W] */
    float* out_feature;       /* [S,H,W] */
    float* out_vfeature;      /* [VS/4,H,W]  svgss */
    float* out_pseudo_normal; /* [3,H,W]     rgss; zero without computer_pseudo_normal and at pixels with a
                                 degenerate stencil (forward.cu:620-622) */
    float* out_surface_xyz;   /* [3,H,W]     rgss; zero without computer_pseudo_normal */
    float* out_weights;       /* [P] */
    int32_t* radii;           /* [P] */
} svgir_outputs;

/* Upstream gradients and gradient outputs of backward (Rasterizer::backward, svgss rasterizer_impl.cu:386-432,
 * rgss :411-449).  The caller need not clear the dL_d* outputs (the reference's glue zero-fills them,
 * rasterize_points.cu:195-211): svgir_backward clears them itself before the per-Gaussian kernels write the gradients of
 * the visible Gaussians.  A caller that lays all outputs out in one allocation (16-byte aligned, a multiple of 16 bytes) passes it as
 * clear_base / clear_bytes: the waves of the composite backward -- which accumulates in the scratch, not in these tensors -- then zero
 * it in passing, no memset and no second stream; without the hint the tensors are cleared one by one on an internal side stream that is
 * joined behind the composite backward. */
typedef struct svgir_grads {
    /* upstream gradients: any of the six may be NULL = all zero (an output that took no part in the loss: the training loss of the
     * reference reads one image, svgss.py:281-289) -- nothing is read for it, and the binder need not allocate and fill a zero image */
    const float* dL_dout_color;    /* [3,H,W] */
    const float* dL_dout_normal;   /* [3,H,W] */
    const float* dL_dout_depth;    /* [1,H,W] */
    const float* dL_dout_opacity;  /* [1,H,W] */
    const float* dL_dout_feature;  /* [S,H,W] */
    const float* dL_dout_vfeature; /* [VS/4,H,W] svgss */
    float* dL_dmeans2D;   /* [P,3] (x,y used) */
    float* dL_dconic;     /* [P,4] (x,y,w used) */
    float* dL_dopacity;   /* [P] */
    float* dL_dcolors;    /* [P,3] */
    float* dL_dfeatures;  /* [P,S] */
    float* dL_dvfeatures; /* [P,VS] svgss */
    float* dL_dnormal;    /* [P,3] */
    float* dL_ddepth;     /* [P] */
    float* dL_dmeans3D;   /* [P,3] */
    float* dL_dcov3D;     /* [P,6] */
    float* dL_dsh;        /* [P,M,3] */
    float* dL_dscales;    /* [P,3] */
    float* dL_drotations; /* [P,4] */
    float* dL_dviewmat;   /* [16] svgss (zero unless config[3] > 0) */
    float* dL_dprojmat;   /* [16] svgss */
    float* dL_dcampos;    /* [3]  svgss */
    void* clear_base;     /* optional: a region that contains every dL_d* output above and nothing the library must */
    size_t clear_bytes;   /*           preserve (NULL / 0: the outputs are cleared one by one) */
    /* Fused shading (svgir_params.shade != NULL; ABI 12): gradients of the shading inputs, layouts as svgir_shade_backward's outputs,
     * every one written completely (rows of surfels that received no blend weight in this view are zero).  The four per-surfel tensors
     * MAY lie inside clear_base (all four or none): their zero rows then come from the composite backward's clearing sweep instead of a
     * zero-fill launch; dL_denv and env_grad_work must lie outside. */
    float* dL_dbase_color;      /* [P,12] */
    float* dL_droughness;       /* [P,4] */
    float* dL_dshade_normals;   /* [P,4,3] */
    float* dL_dradiance;        /* [P,Ns,3]; may be NULL when shade->sp.radiance_ratio is set (ABI 13: the cache is detached) */
    float* dL_denv;             /* [env_h,env_w,3] */
    float* env_grad_work;       /* scratch, env_h*env_w*3 (+ SVGIR_SHADE_RATIO_WORK with dL_dradiance_ratio) floats */
    const float* dL_dreduced;   /* optional [P,70]: upstream gradient of svgir_fused_shade.reduced (needs all_surfels != 0) */
    const float* out_weights;   /* optional (required by the fused shading): the forward's out_weights [P].  A surfel that received no
                                 * blend weight has no gradient rows and all-zero composite gradients; with the weights at hand the
                                 * per-Gaussian kernels behind the composite (row reduction, cov2D / preprocess / SH backward, the fused
                                 * shading's backward) walk the list of blended surfels -- 13-29 % of the model on the BASELINE scenes --
                                 * instead of all P.  Used where building the list costs less than it saves: svgss with vfeatures from 50 000
                                 * surfels on, otherwise from 400 000. */
    float* dL_dradiance_ratio;  /* optional [1] (ABI 13; needs shade->sp.radiance_ratio): see svgir_shade_backward */
    /* Appended within ABI 14 (a zero-initialised svgir_grads keeps the earlier behaviour, bit for bit): the fused shading's gradient
     * w.r.t. the RAW view directions sp.viewdirs, see svgir_shade_backward_view.  Optional (NULL: not computed; needs
     * svgir_params.shade); written completely, rows of surfels that received no blend weight are zero.  It follows the placement rule
     * of the four per-surfel tensors above: inside clear_base together with them, or outside together with them. */
    float* dL_dviewdirs;        /* optional [P,3] */
} svgir_grads;

int svgir_abi_version(void);

/* Sizes of the three opaque scratch blobs (the reference's required<GeometryState/ImageState/BinningState>,
 * rasterizer_impl.h:73-84). */
size_t svgir_geom_bytes(int32_t P);
size_t svgir_image_bytes(int32_t W, int32_t H);
/* The binning blob also holds the per-segment forward states that parallelise the backward over depth, hence the
 * dependence on the image size and channel counts (S features, VS vfeature floats; VS = 0 for rgss). */
size_t svgir_binning_bytes(int32_t num_rendered, int32_t W, int32_t H, int32_t S, int32_t VS);   /* worst case: the forward asks its
 * allocator for less once it has seen a view of the workload (state slots from the pair statistics of recent views; such blobs are
 * an odd multiple of 128 bytes long and belong to the forward that laid them out: pass them to svgir_backward unchanged) */
/* Byte offset of the int32 n_contrib[H*W] plane inside the image blob (rgss returns a view of it, Q10). */
size_t svgir_image_ncontrib_offset(int32_t W, int32_t H);

/* Forward pass.  Replaces CudaRasterizer::Rasterizer::forward (svgss rasterizer_impl.cu:209-382,
 * rgss :209-407).  Calls geom(), image() and binning().  From the second call on, binning() is called -- and the
 * count-dependent stages (emit, tile sort, ranges, composite) are launched -- speculatively for a capacity derived
 * from the previous call's instance count, while the GPU still computes the count; the stages read the count on the
 * device.  The count reaches the host as a tagged store into pinned memory (no copy, no event) and then only confirms the guess (no
 * GPU idle time); if the guess was too small, binning() is called again and those stages are re-run (only the LAST pointer it returned is
 * used).
 * Returns num_rendered (R >= 0) or a negative svgir_status. */
int svgir_forward(const svgir_params* p, const svgir_outputs* o,
                  svgir_alloc_fn geom, void* geom_ctx,
                  svgir_alloc_fn binning, void* binning_ctx,
                  svgir_alloc_fn image, void* image_ctx,
                  void* stream);

/* Several views in flight from ONE host thread (ABI 12).  Every view is begun -- validated, its blobs allocated, ALL of its kernels
 * launched on its stream, the count-dependent ones speculatively -- before the first view's instance count is awaited.  Views on distinct
 * streams overlap on the GPU (a single 800 x 800 view leaves the SIMDs under-occupied: two views in flight render 1.3x the surfels per
 * second); the results are bit-identical to `count` svgir_forward calls.  num_rendered receives each view's R or its negative status;
 * the return value is 0 or the first error.  The reference has no counterpart (its forward blocks on a cudaMemcpy per view,
 * rasterizer_impl.cu:307-312; eval_relighting_tensoIR.py:303-378 renders its views one after the other). */
typedef struct svgir_view_call {
    const svgir_params* params; const svgir_outputs* outputs;
    svgir_alloc_fn geom; void* geom_ctx;
    svgir_alloc_fn binning; void* binning_ctx;
    svgir_alloc_fn image; void* image_ctx;
    void* stream;
    int32_t num_rendered;   /* out */
} svgir_view_call;
int svgir_forward_batch(svgir_view_call* views, int32_t count);

/* What the speculative launches of svgir_forward did so far in this process (monitoring / tests; ABI 11):
 * out5 = {forwards, views re-run because the instance capacity guessed from the previous views was too small, views whose blend states
 * were dumped again by their backward because the state-slot capacity was, views re-run because a visible depth key did not carry the
 * top byte the last views' keys shared (the depth sort then runs three 8-bit passes instead of four), views whose depth sort ran three
 * passes}.  The reference has no counterpart: its forward waits for the
 * instance count (rasterizer_impl.cu:307-312) and always sorts 64-bit keys. */
void svgir_speculation_stats(int64_t* out5);
/* Forgets the speculation history (ABI 14) of one scope (svgir_params.workload_scope), or of every scope (scope < 0): the next view of
 * such a workload is launched like a first view (exact instance capacity after a host wait, state slots sized from its own cull, four
 * depth passes).  For callers that recycle scope ids, or that switch scenes under one id.  Blobs of earlier forwards stay valid. */
void svgir_reset_workload_history(int32_t scope);

/* Backward pass.  Replaces CudaRasterizer::Rasterizer::backward (svgss rasterizer_impl.cu:386-523,
 * rgss :411-535).  `R` and the three blobs are what the matching svgir_forward produced; `radii` is its
 * radii output.  `binning_bytes` is the size the binning callback was last asked for: the blob is laid out for an
 * instance capacity >= R that the backward recovers from it (the forward sizes the blob before it knows R). */
int svgir_backward(const svgir_params* p, const svgir_grads* g, int32_t R, const int32_t* radii,
                   char* geom_blob, char* binning_blob, size_t binning_bytes, char* image_blob,
                   char* scratch, size_t scratch_bytes, void* stream);
/* Size of the backward scratch (device memory, contents irrelevant on entry, only needed during the call; REQUIRED).
 * The composite backward reduces every per-Gaussian gradient over the 64 pixels of a wave and then
 *   svgss: stores one complete gradient row per (instance, sub-tile) pair, summed per Gaussian in a fixed order by a
 *          second kernel (no atomics, bit-reproducible gradients): a 4-byte reverse-map entry per possible pair (4 * capacity)
 *          + the rows (worst case 4 * capacity; see svgir_backward_scratch_bytes_for);
 *   rgss : accumulates with float atomics into ONE packed row per Gaussian (P rows), unpacked into the dL_d* tensors
 *          by the per-Gaussian backward kernel.
 * The reference accumulates with one global float atomic per (pixel, splat, output) straight into its dL_d* tensors
 * (backward.cu:880-930) and needs no scratch; a binder allocates this buffer next to them. */
size_t svgir_backward_scratch_bytes(int32_t variant, int32_t P, size_t binning_bytes, int32_t W, int32_t H, int32_t S,
                                    int32_t VS);
/* The same for ONE view: `image_blob` is the image blob of the svgir_forward whose backward is about to run.  svgss with vfeatures
 * then gets one gradient row per (sub-tile, instance) pair that survived that view's cull (1.2 per instance on the BASELINE scenes)
 * instead of four per instance: the forward reads the pair count back asynchronously behind its cull, and this call returns at once
 * unless that count is still on its way (then it waits: polling, and beyond 50 ms blocking on the device).  A blob the library has not
 * seen in its last 1024 forwards is read itself (the image blob carries the view's counts and capacities); NULL gets the
 * worst case; svgir_backward accepts either size for the view it belongs to.  (ABI 10) */
size_t svgir_backward_scratch_bytes_for(int32_t variant, int32_t P, size_t binning_bytes, const char* image_blob, int32_t W, int32_t H,
                                        int32_t S, int32_t VS);

/* Introspection of the state blobs for tests / debugging (the blobs stay opaque to the rendering path): byte offset of
 * the depth-sorted instance list `point_list` (uint32 Gaussian ids, R entries; BinningState::point_list,
 * rasterizer_impl.h:66-76) inside the binning blob, and of the per-tile `ranges` (uint2 per tile; ImageState::ranges,
 * rasterizer_impl.h:49-63) inside the image blob. */
size_t svgir_binning_point_list_offset(size_t binning_bytes, const char* image_blob, int32_t W, int32_t H, int32_t S, int32_t VS);
size_t svgir_image_ranges_offset(int32_t W, int32_t H);

/* Replaces CudaRasterizer::Rasterizer::markVisible (rasterizer_impl.cu:141-153).  `present` is a byte per
 * Gaussian.  svgss: the reference kernel body is commented out, so `present` is left untouched (all false, Q14);
 * rgss: present = view-space z > 0.2. */
int svgir_mark_visible(int32_t variant, int32_t P, const float* means3D, const float* viewmatrix,
                       const float* projmatrix, uint8_t* present, void* stream);

/* ---- per-splat spatially-varying BRDF shading ---------------------------------------------
 * Fused replacement of the PyTorch `rendering_equation4` + `GGX_specular4` (gaussian_renderer/svgss.py:537-631) with
 * the lat-long env lookup of `DirectLightMap.direct_light` / `EnvLight.direct_light`
 * (scene/direct_light_map.py:70-83, scene/envmap.py:53-72) and the feature packing of svgss.py:143-166.  There is no
 * reference C/CUDA counterpart (the reference does this with ~40 broadcasting torch ops and [P,Ns,4,3] temporaries).
 *
 * Layouts as in the reference: base_color [P,12] (channel*4 + corner), roughness [P,4], normals [P,4,3] (world
 * space), viewdirs [P,3], radiance / incident_dirs [P,Ns,3], visibility / incident_areas [P,Ns,1],
 * env [env_h, env_w, 3].  The looked-up light is env_scale * bilinear(f(env)) with f = softplus when
 * env_softplus != 0 (DirectLightMap: softplus, scale 2) or identity (EnvLight: scale 1), clamped to [0, 64].
 * `env_work` is a caller-provided, 16-byte aligned scratch of env_h*env_w*4 floats (holds f(env) as one float4 per texel).
 *
 * reduced [P,70]: pbr[12] diffuse_light[12] specular[12] direct[12] indirect[12] mean_incident[3] mean_local[3]
 *                 mean_global[3] mean_visibility[1]   (means over the Ns samples, like `.mean(-2)` in svgss.py)
 * features / vfeatures (either may be NULL): the rasterizer inputs of svgss.py:143-166;
 *   training != 0: features [P,4]  = [mean_vis, mean_local]; vfeatures [P,52] = [pbr, base_color, normal_view,
 *                  roughness, diffuse_light];   training == 0: features [P,7] = [mean_incident, mean_local, mean_vis],
 *                  vfeatures [P,64] = [pbr, base_color, normal_view, roughness, direct, indirect];
 *   normal_view = normals @ viewmatrix[:3,:3], stored channel*4 + corner. */
typedef struct svgir_shade_params {
    int32_t P, Ns, env_h, env_w;
    int32_t env_softplus;
    int32_t training;
    float env_scale;
    const float* base_color;
    const float* roughness;
    const float* normals;
    const float* viewdirs;
    const float* radiance;
    const float* visibility;
    const float* incident_dirs;
    const float* incident_areas;
    const float* env;
    const float* viewmatrix;   /* [16], only for the packed vfeatures; may be NULL when vfeatures is NULL */
    float* env_work;
    const float* env_transform; /* [9] row-major 3x3 or NULL: the env lookup uses transform * dir (EnvLight.transform,
                                 * scene/envmap.py:57-60); every other term keeps the untransformed direction */
    /* Incident directions generated in the kernels instead of streamed: when incident_dirs is
     * NULL, sample i of surfel g is the reference's Fibonacci hemisphere lattice around lattice_normals[g]
     * (fibonacci_sphere_sampling + rotation_between_z, utils/graphics_utils.py:9-37, utils/sh_utils.py:36-68; what
     * sample_incident_rays stores in pc._incident_dirs, scene/gaussian_model.py:23-31), with the per-surfel random
     * azimuth offset lattice_offsets[g] of the training branch (NULL: evaluation lattice).  incident_areas may then be
     * NULL too (the lattice's areas are the constant 2 pi).  lattice_work: scratch of 4 * Ns floats. */
    const float* lattice_normals;   /* [P,3] unit */
    const float* lattice_offsets;   /* [P] radians or NULL */
    float* lattice_work;
    /* Shade a SUBSET of the P surfels (ABI 12; both NULL: all of them).  `subset` [P] is a permutation of 0..P-1 in device memory whose
     * first *subset_count entries (a device uint32) are the surfels to shade; the output rows of the others (reduced / features /
     * vfeatures; the backward's dL_dbase_color, dL_droughness, dL_dnormals, dL_dradiance) are ZERO-filled by the same call, so every
     * output is still written completely.  Rows of shaded surfels are bit-identical to an all-P call. */
    const uint32_t* subset;
    const uint32_t* subset_count;
    /* The reference's radiance cache enters the shading as  get_radiances = nan_to_num(_radiances.detach() * _radiance_ratio, nan=0)
     * (scene/gaussian_model.py:323-324): a [P,Ns,3] product and its clean-up per iteration, and in the backward a [P,Ns,3] gradient
     * whose only use is the sum that gives dL/d_radiance_ratio.  ABI 13: `radiance_ratio` (NULL: `radiance` is used as it is) points
     * to that scalar in device memory; the kernels then use nan_to_num(radiance * ratio) (torch.nan_to_num: NaN -> 0, +-inf -> the
     * largest finite floats) -- the same fp32 product, bit for bit -- and the backward can return the scalar's gradient directly. */
    const float* radiance_ratio;
} svgir_shade_params;

#define SVGIR_SHADE_REDUCED 70
#define SVGIR_SHADE_RATIO_WORK 256   /* extra floats of env_grad_work when dL_dradiance_ratio is requested */

int svgir_shade_forward(const svgir_shade_params* p, float* reduced, float* features, float* vfeatures, void* stream);

/* Backward of svgir_shade_forward w.r.t. base_color, roughness, normals, radiance and the env texels, given any of
 * dL/d(reduced) [P,70], dL/d(features) [P,S] and dL/d(vfeatures) [P,VS] (each may be NULL, not all three; the
 * packed rows follow p->training as in the forward and need p->viewmatrix; the gradient of mean_visibility is
 * ignored: visibility is not differentiable in the reference either).  The packing's direct terms (vfeatures
 * carries base_color, view-space normals and roughness, svgss.py:152-166) are included.  All outputs are
 * overwritten; dL_denv [env_h,env_w,3] is the gradient w.r.t. the RAW env (softplus' included).
 * `env_grad_work`: scratch of env_h*env_w*3 floats.
 * With p->radiance_ratio (ABI 13): dL_dradiance is the gradient w.r.t. the RAW radiance (ratio and the nan_to_num mask included) and
 * may be NULL (the reference detaches the cache); dL_dradiance_ratio [1] (optional, NULL without p->radiance_ratio) receives
 * sum(dL/d(incident) * isfinite(radiance * ratio) * radiance), what autograd returns for the scalar -- summed per workgroup and then
 * in a fixed order (reproducible); env_grad_work then holds SVGIR_SHADE_RATIO_WORK more floats. */
int svgir_shade_backward(const svgir_shade_params* p, const float* dL_dreduced, const float* dL_dfeatures,
                         const float* dL_dvfeatures, float* dL_dbase_color,
                         float* dL_droughness, float* dL_dnormals, float* dL_dradiance, float* dL_denv,
                         float* env_grad_work, float* dL_dradiance_ratio, void* stream);

/* svgir_shade_backward plus the gradient w.r.t. the view directions (added within ABI 14; svgir_shade_backward itself is unchanged and
 * returns what it returned before).  In the reference `viewdirs = normalize(camera_center - means3D)` is a differentiable function of
 * the surfel positions (gaussian_renderer/svgss.py:109) and the specular lobe uses it in V = normalize(viewdirs), H = normalize((L + V)
 * / 2), N.V, N.H and the Schlick term's V.H (svgss.py:595-631); sign(V.N) has no gradient.  dL_dviewdirs [P,3] is required, written
 * completely (rows outside a subset are zero) and is the gradient w.r.t. the RAW rows of p->viewdirs, the normalisation
 * v / max(|v|, 1e-12) included; svgir_activate_backward turns it into dL_dxyz.  Summed without atomics: two calls give the same bits.
 * It is a second pass behind the kernel of svgir_shade_backward, which runs unchanged: every other output has the bits that entry
 * point writes (dL_denv: float atomics, the same sum in the order of the day). */
int svgir_shade_backward_view(const svgir_shade_params* p, const float* dL_dreduced, const float* dL_dfeatures,
                              const float* dL_dvfeatures, float* dL_dbase_color,
                              float* dL_droughness, float* dL_dnormals, float* dL_dradiance, float* dL_denv,
                              float* env_grad_work, float* dL_dradiance_ratio, float* dL_dviewdirs, void* stream);

/* Spherical-Gaussian direct light (added within ABI 14: new entry points and one new struct, nothing existing changes).
 * The reference's second learnable light, scene/direct_light_sg.py:DirectLightSG, is a mixture of M lobes evaluated exactly per incident
 * direction (render_envmap_sg); train.py:65-66 switches between it and the lat-long texture.  The entry points below are
 * svgir_shade_forward / svgir_shade_backward(_view) with that mixture as the global light: the M lobes replace the staging's four
 * texture taps and the backward's texel scatter, nothing of the GGX / transport arithmetic changes.
 *
 * Raw parameters: `lobes` [M,7] fp32 row-major, row = (xi.x, xi.y, xi.z, lambda, mu.r, mu.g, mu.b), 1 <= M <= SVGIR_SG_MAX_LOBES.
 * Light of a direction d -- used as given: NOT normalised, and no lookup transform (DirectLightSG.direct_light ignores its `transform`):
 *     a_m = xi_m / |xi_m|                 (a plain sqrt of the sum of squares and a plain division, as torch.norm: no clamp)
 *     e_m = expf(|lambda_m| (d.a_m - 1))  (the accurate expf, not the fast intrinsic: |lambda| is in the hundreds)
 *     L_c(d) = sum_m |mu_mc| e_m          (fp32, m ascending)
 * Shading: global = clamp(L, 0, 64) * visibility; everything downstream -- transport, GGX, the 70 reduced columns, the packing into
 * features / vfeatures at training and eval widths, radiance_ratio, explicit directions and the in-kernel lattice -- is what the texture
 * path does with its `global`.
 * Gradients w.r.t. the raw lobes: with g_c the adjoint of L_c (= the adjoint of global_c x visibility x the clamp mask 0 <= L_c <= 64,
 * which passes at equality as torch.clamp does) and s = sum_c |mu_c| e g_c, summed over all P Ns samples:
 *     dmu_c = sign(mu_c) e g_c,   dlambda = sign(lambda) (d.a - 1) s,   dxi = |lambda| s (d - a (a.d)) / |xi|,   sign(0) = 0 (torch's abs).
 * The gradients of base_color, roughness, normals, radiance / radiance_ratio and viewdirs are those of the texture path with this global.
 * Non-finite lobes: a lobe with |xi| = 0 or a non-finite entry makes the light NaN for EVERY sample, as in torch (NaN * 0 = NaN): the
 * forward returns NaN in the light-dependent columns; nothing faults or hangs; gradients are unspecified in that case.
 *
 * `work`: caller-provided, 16-byte aligned, 8 * count floats -- the prepared table a small prologue kernel builds on every call, per lobe
 * {a.xyz, |lambda|} and {|mu|.rgb, 1 / |xi|} (the role env_work plays for the texture).
 * Invalid input is rejected with SVGIR_ERR_INVALID and a message before any launch: count outside 1 ... SVGIR_SG_MAX_LOBES, NULL lobes /
 * work, a misaligned work, a non-NULL subset / subset_count (subset shading belongs to the rasterizer-fused path).
 * The bare light's gradient (svgir_sg_eval_backward), the eval backdrop (svgir_env_backdrop_sg) and the fused radiance-consistency loss
 * (svgir_radiance_loss_forward_sg / _backward_sg) follow below and next to their texture counterparts.
 * The shading fused into the rasterizer calls has its twins too: svgir_forward_sg / svgir_backward_sg, behind svgir_fused_shade below. */
#define SVGIR_SG_MAX_LOBES 128
typedef struct svgir_sg_light {
    int32_t count;        /* M */
    const float* lobes;   /* [M,7] raw */
    float* work;          /* [8 M] scratch, 16-byte aligned */
} svgir_sg_light;

/* out [n,3] = the UNCLAMPED L of dirs [n,3]: DirectLightSG.direct_light / render_envmap_sg. */
int svgir_sg_eval(const svgir_sg_light* light, int64_t n, const float* dirs, float* out, void* stream);

/* The gradient of svgir_sg_eval (added within ABI 14).  With a, e, |mu|, |lambda| as above, g = dL_dout [n,3] of one direction (no clamp:
 * the light is the unclamped L) and s_m = e_m sum_c |mu_mc| g_c:
 *     dmu_mc = sign(mu_mc) sum_n e_m g_c,   dlambda_m = sign(lambda_m) sum_n (d.a_m - 1) s_m,
 *     dxi_m = |lambda_m| (G_m - a_m (a_m.G_m)) / |xi_m|  with  G_m = sum_n s_m d,   sign(0) = 0
 *     dL_ddirs[n] = sum_m |lambda_m| s_m a_m      (fp32, m ascending; no atomics: the same bits on every run)
 * dL_dlobes [M,7] and dL_ddirs [n,3] are each optional (NULL), not both; every element of a requested output is written.  The 7 M sums
 * are accumulated per workgroup in LDS in fp64, flushed once per workgroup with float atomics into `grad_work`
 * (svgir_sg_grad_work_bytes(count) bytes, cleared by the call; the layout svgir_shade_backward_sg uses) and pulled back by a one-block
 * kernel: dL_dlobes is repeatable only up to the order of those adds.  light->work is built by the call.  n = 0 writes zeros to
 * dL_dlobes and launches nothing else.
 * Rejected with SVGIR_ERR_INVALID and a message before any HIP call: count outside 1 ... SVGIR_SG_MAX_LOBES, NULL lobes / work /
 * grad_work, a misaligned work, n < 0, both outputs NULL, NULL dirs or dL_dout with n > 0.  Non-finite lobes: outputs are unspecified;
 * nothing faults or hangs. */
int svgir_sg_eval_backward(const svgir_sg_light* light, int64_t n, const float* dirs, const float* dL_dout, float* dL_dlobes,
                           float* dL_ddirs, float* grad_work, void* stream);

/* svgir_shade_forward with the SG light.  The env* fields of `p` (env, env_h, env_w, env_softplus, env_scale, env_work, env_transform) are
 * ignored and may be NULL / 0; p->subset must be NULL. */
int svgir_shade_forward_sg(const svgir_shade_params* p, const svgir_sg_light* light, float* reduced, float* features, float* vfeatures,
                           void* stream);

/* svgir_shade_backward (dL_dviewdirs != NULL: svgir_shade_backward_view) with the SG light: dL_dlobes [M,7] takes dL_denv's place, all
 * outputs are overwritten.  dL_dradiance_ratio and dL_dviewdirs are optional (NULL) as there.  `grad_work`: scratch of
 * svgir_sg_grad_work_bytes(count) bytes (the table-space sums + SVGIR_SHADE_RATIO_WORK floats).  The 7 M sums over all samples are
 * accumulated per workgroup in LDS in fp64 and flushed once per workgroup with float atomics (dL_dlobes: the same sum in the order of the
 * day, like dL_denv); a small epilogue kernel applies the normalisation's Jacobian and the signs. */
size_t svgir_sg_grad_work_bytes(int32_t count);
int svgir_shade_backward_sg(const svgir_shade_params* p, const svgir_sg_light* light, const float* dL_dreduced, const float* dL_dfeatures,
                            const float* dL_dvfeatures, float* dL_dbase_color, float* dL_droughness, float* dL_dnormals, float* dL_dradiance,
                            float* dL_dlobes, float* grad_work, float* dL_dradiance_ratio, float* dL_dviewdirs, void* stream);

/* Shading fused into the rasterizer calls (svgir_params.shade; ABI 12).  The only consumers of the shading's outputs are the packed
 * `features` / `vfeatures` rows the svgss composite blends (gaussian_renderer/svgss.py:143-182), and it reads the rows of the surfels
 * that survive the view's culls only -- 44 % of the surfels pass the preprocess culls on the BASELINE scenes, ~30 % survive the per-tile
 * cull as well, and 13-29 % ever receive a blend weight -- while the reference (and svgir_shade_forward on its own) shades all P.
 *   svgir_forward : runs preprocess / sorts / per-tile cull first, then shades exactly the surfels that are a candidate of at least one
 *       8x8 sub-tile -- or, when sp.Ns >= 128 (evaluation sample counts: shading a surfel costs far more than compositing it), the
 *       surfels a geometry-only pre-pass of the composite finds to receive a blend weight -- writes their `features` [P,S] / `vfeatures` [P,VS] rows (S, VS = 4, 52 when sp.training, else 7, 64) and zero-fills
 *       the others, then composites.  sp.P must equal svgir_params.P; sp.subset / sp.subset_count are ignored (the library's own list,
 *       kept in the geometry blob, is used).
 *   svgir_backward: after the rasterizer's backward has produced dL_dfeatures / dL_dvfeatures, differentiates the shading of the
 *       surfels with out_weights > 0 (all others have exactly-zero feature gradients) into svgir_grads.dL_dbase_color ...; the rest of
 *       those rows is zero-filled.  Pass the SAME struct (same `features` / `vfeatures` contents) as to the forward.
 * all_surfels != 0 shades / differentiates all P surfels (needed when `reduced` feeds a loss of its own, e.g. the reference's
 * lambda_light term, svgss.py:359-364).  Results are bit-identical to the unfused sequence (svgir_shade_forward -> svgir_forward,
 * svgir_backward -> svgir_shade_backward) except dL_denv, whose float atomics are summed in a different order. */
struct svgir_fused_shade {
    svgir_shade_params sp;
    float* reduced;        /* [P,70] or NULL; rows of unshaded surfels are zero */
    int32_t all_surfels;
};

/* The fused shading under a spherical-Gaussian light (added within ABI 14: two entry points, no struct changes).  svgir_forward /
 * svgir_backward with params->shade != NULL (required here: svgss, S / VS = 4 / 52 when sp.training, else 7 / 64) and `light` as the
 * global light of the shading, as in svgir_shade_forward_sg / svgir_shade_backward_sg: the env* fields of params->shade->sp are ignored
 * and may be NULL / 0, light->work is built by each call.  In svgir_grads, dL_denv receives dL_dlobes [M,7] and env_grad_work is scratch of
 * svgir_sg_grad_work_bytes(M) bytes (both outside clear_base, as for the texture).  Everything else is what the texture calls do:
 * all_surfels, reduced, dL_dreduced, dL_dradiance_ratio, dL_dviewdirs, out_weights, the clear_base carve-out, the working sets (the
 * forward shades the surfels that touch a tile, or from sp.Ns >= 128 on those the contribution pre-pass finds; the backward
 * differentiates the blended ones).
 * Results are bit-identical to the unfused sequence svgir_shade_forward_sg -> svgir_forward and svgir_backward ->
 * svgir_shade_backward_sg, except dL_dlobes: fp64 LDS sums per workgroup plus float atomics across workgroups, the same sum in the order
 * of the day.  Every element of every requested output is written, dL_dlobes included; a view that blends nothing gives zero dL_dlobes
 * and zero dL_dradiance_ratio.  Non-finite lobes give NaN in the light-dependent columns and never a fault.
 * Rejected with SVGIR_ERR_INVALID and a message before any launch: a NULL light, count outside 1 ... SVGIR_SG_MAX_LOBES, NULL lobes / work,
 * a misaligned work, params->shade == NULL, the rgss variant, widths that do not match sp.training, a missing dL_denv / env_grad_work /
 * per-surfel gradient output, dL_dreduced without all_surfels.
 * The lobe table, the lattice table and (backward) the cleared accumulator come from one small launch in front of the shading kernel; the
 * texture path's kernels, which carry the texture's tables in passing, are untouched.
 * Not provided: svgir_forward_batch with an SG light -- svgir_view_call has no room for one. */
int svgir_forward_sg(const svgir_params* p, const svgir_sg_light* light, const svgir_outputs* o,
                     svgir_alloc_fn geom, void* geom_ctx,
                     svgir_alloc_fn binning, void* binning_ctx,
                     svgir_alloc_fn image, void* image_ctx,
                     void* stream);
int svgir_backward_sg(const svgir_params* p, const svgir_sg_light* light, const svgir_grads* g, int32_t R, const int32_t* radii,
                      char* geom_blob, char* binning_blob, size_t binning_bytes, char* image_blob,
                      char* scratch, size_t scratch_bytes, void* stream);

/* Materialises the incident-direction lattice: dirs [P,Ns,3] and / or areas [P,Ns,1] (either may be NULL), the return
 * values of the reference's fibonacci_sphere_sampling(normals, Ns, random_rotate) with `offsets` [P] standing for its
 * random draw (NULL = random_rotate False).  lattice_work: scratch of 4 * Ns floats. */
int svgir_incident_dirs(int32_t P, int32_t Ns, const float* normals, const float* offsets, float* lattice_work,
                        float* dirs, float* areas, void* stream);

/* Bilinear resize of an [H,W,C] image to [out_h,out_w,C] with the half-pixel convention of
 * F.interpolate(mode='bilinear', align_corners=False): EnvLight.direct_light's 32x64 down-sample of its HDR map
 * (scene/envmap.py:62-63). */
int svgir_resample_bilinear(const float* src, int32_t H, int32_t W, int32_t C, float* dst, int32_t out_h, int32_t out_w,
                            void* stream);

/* ---- image-space epilogue right after the svgss rasterizer ----------------------------------
 * Fused replacement of the PyTorch tail of render_view (gaussian_renderer/svgss.py:187-246): feature / vfeature planes
 * divided by the rendered opacity (clamp_min 1e-5), channel split, rgb_to_srgb (utils/graphics_utils.py:198-215),
 * compositing over `bg` [3].  opacity [1,H,W], feature [S,H,W], vfeature [VS/4,H,W] are the rasterizer's outputs at the
 * training (S=4, VS=52) or evaluation (S=7, VS=64) widths; `out` receives svgir_unpack_planes(training) planes [.,H,W]:
 *   training  (21): pbr | normal | base_color | roughness | diffuse | local_lights | visibility
 *   evaluation(27): pbr | normal | base_color | roughness | direct | indirect | lights | local_lights | visibility
 * (three planes per quantity; one-channel quantities are broadcast over the three background channels as in the
 * reference).  The backward maps dL/d(out) to dL/d(opacity, feature, vfeature); all outputs are overwritten.
 * Clamps behave as torch's: the opacity clamp passes its gradient AT opacity == 1e-5f (clamp_min: self >= min), and NaN inputs stay
 * NaN through the opacity clamp and the sRGB clip (torch.clamp / clamp_min propagate NaN); a non-finite pixel affects no other pixel,
 * forward or backward.  The same holds for svgir_unpack_rgss_* below. */
int svgir_unpack_planes(int32_t training);
int svgir_unpack_forward(int32_t W, int32_t H, int32_t training, const float* bg, const float* opacity, const float* feature,
                         const float* vfeature, float* out, void* stream);
int svgir_unpack_backward(int32_t W, int32_t H, int32_t training, const float* bg, const float* opacity, const float* feature,
                          const float* vfeature, const float* dL_dout, float* dL_dopacity, float* dL_dfeature,
                          float* dL_dvfeature, void* stream);
/* Stage 1 (rgss) counterparts (gaussian_renderer/render.py:83-91, 107-114).
 * pack: features [P,5] = [geometric normal (world) 3, view depth d, d^2], d = (xyz1 @ viewmatrix).z; the backward maps
 *       dL/d(features) to dL/d(means3D) and dL/d(normals).
 * unpack: x_c = feature_c / max(opacity, 1e-5) * (num_contrib > 0) for the 5 feature planes; out [6,H,W] = [x_0 .. x_4,
 *       depth_var = x_4 - depth^2]; the backward maps dL/d(out) to dL/d(opacity, depth, feature). */
int svgir_pack_rgss_forward(int32_t P, const float* means3D, const float* normals, const float* viewmatrix, float* features,
                            void* stream);
int svgir_pack_rgss_backward(int32_t P, const float* means3D, const float* viewmatrix, const float* dL_dfeatures,
                             float* dL_dmeans3D, float* dL_dnormals, void* stream);
int svgir_unpack_rgss_forward(int32_t W, int32_t H, const int32_t* num_contrib, const float* opacity, const float* depth,
                              const float* feature, float* out, void* stream);
int svgir_unpack_rgss_backward(int32_t W, int32_t H, const int32_t* num_contrib, const float* opacity, const float* depth,
                               const float* feature, const float* dL_dout, float* dL_dopacity, float* dL_ddepth,
                               float* dL_dfeature, void* stream);

/* depth2normal (utils/image_utils.py:61-125): depth, mask [1,H,W] -> normal [3,H,W]; fovx / fovy in radians, prcp = the
 * camera's principal point as a fraction of the image (Camera.prcppoint). */
int svgir_depth2normal(int32_t W, int32_t H, const float* depth, const float* mask, float fovx, float fovy, float prcp_x,
                       float prcp_y, float* normal, void* stream);
/* adjoint of svgir_depth2normal w.r.t. the depth plane (the reference's depth2normal is differentiable and the stage-1 loss
 * `cos_loss(rendered_normal, d2n)` uses it without detaching, gaussian_renderer/render.py:158-160): dL_ddepth [1,H,W] is
 * written completely; the mask gets no gradient. */
int svgir_depth2normal_backward(int32_t W, int32_t H, const float* depth, const float* mask, const float* dL_dnormal, float fovx,
                                float fovy, float prcp_x, float prcp_y, float* dL_ddepth, void* stream);

/* The environment backdrop that ends every eval view (gaussian_renderer/svgss.py:255-260; forward only, the reference runs it
 * under no_grad): per pixel (u, v) the camera direction ((u - cx) / fx, (v - cy) / fy, 1), normalised and rotated by c2w[:3,:3]
 * (Camera.get_world_directions, scene/cameras.py:96-108), then by the light's lookup transform if one is given (EnvLight's
 * `dirs @ transform.T`), is looked up in the lat-long map exactly as the shading kernels do it (grid_sample, align_corners=True, zero
 * padding; env = env_scale * bilinear(f(env)), f = softplus when env_softplus != 0 -- DirectLightMap: softplus, scale 2; EnvLight's
 * 32 x 64 resample: identity, scale 1).  d.z is clamped to [-1, 1] before the acos: where the reference's rounded unit vector has
 * |z| = 1 + ulp and turns the pixel NaN, this looks up the pole.
 *   intr         HOST  {fx, fy, cx, cy} in pixels (Camera.intrinsics); fx, fy finite and non-zero
 *   c2w_rot      HOST  c2w[:3,:3], row-major 9 floats
 *   env_transform HOST 9 floats row-major, or NULL
 *   env          [env_h, env_w, 3] raw map; env_work: env_h * env_w * 4 floats of scratch, 16-byte aligned (the f(env) table)
 *   image [3,H,W], opacity [1,H,W], vfeature [>= 3,H,W] (planes 0..2 = the rasterized pbr): the rasterizer's raw outputs
 *   out [9,H,W], every element written: env_only = srgb(env) | render_env = image + (1 - o) srgb(env) |
 *                pbr_env = srgb(pbr o + (1 - o) env), pbr = vfeature[0:3] / max(o, 1e-5)
 * Invalid arguments are rejected with SVGIR_ERR_INVALID and a message before any HIP call. */
int svgir_env_backdrop(int32_t W, int32_t H, const float* intr, const float* c2w_rot, const float* env_transform, const float* env,
                       int32_t env_h, int32_t env_w, int32_t env_softplus, float env_scale, float* env_work, const float* image,
                       const float* opacity, const float* vfeature, float* out, void* stream);

/* svgir_env_backdrop under a spherical-Gaussian light (added within ABI 14).  The pixel directions are exactly those above -- the camera
 * direction, normalised, rotated by c2w[:3,:3] -- and are used as they are: DirectLightSG.direct_light ignores a lookup transform, and
 * there is no latitude to clamp.  env = L(d), the UNCLAMPED fp32 light of svgir_sg_eval (m ascending), and the three images are composed
 * from it exactly as above (the same sRGB, the same max(o, 1e-5)); every element of out [9,H,W] is written.  light->work (8 * count
 * floats, 16-byte aligned) is built by this call.  Invalid arguments -- those of svgir_env_backdrop and those of a svgir_sg_light -- are
 * rejected with SVGIR_ERR_INVALID and a message before any HIP call. */
int svgir_env_backdrop_sg(int32_t W, int32_t H, const float* intr, const float* c2w_rot, const svgir_sg_light* light,
                          const float* image, const float* opacity, const float* vfeature, float* out, void* stream);

/* Image losses behind render_view: L1 and SSIM with the reference's 11 x 11 Gaussian window
 * (`F.l1_loss(image, gt)` and `ssim(image, gt)`, gaussian_renderer/svgss.py:281-289, render.py:150-151;
 * utils/loss_utils.py:21-64), img1 / img2 = [C,H,W] planes.
 *   forward : writes 2 floats per 16x16 tile and channel -- the tile's sums of the SSIM map and of |img1 - img2| -- into
 *             `partial` [svgir_l1_ssim_partials(C,H,W)][2], if `dmaps` [3,C,H,W] is not NULL what the backward needs, and if
 *             `means2` is not NULL the two means {mean SSIM, mean |img1 - img2|} (device floats: fixed-order double sum of
 *             the partials by a second small kernel);
 *   backward: dL_dimg1 [C,H,W] = g_ssim_mean * d(mean SSIM)/d(img1) + g_l1_mean * d(mean |img1 - img2|)/d(img1), written
 *             completely; if `g_dev` is not NULL the two host scalars are multiplied by g_dev[0] / g_dev[1] read on the
 *             device (upstream gradients that never visit the host).  img2 (the ground truth) gets no gradient. */
size_t svgir_l1_ssim_partials(int32_t C, int32_t H, int32_t W);
int svgir_l1_ssim_forward(const float* img1, const float* img2, int32_t C, int32_t H, int32_t W, float* partial, float* dmaps,
                          float* means2, void* stream);
int svgir_l1_ssim_backward(const float* img1, const float* img2, const float* dmaps, int32_t C, int32_t H, int32_t W,
                           float g_ssim_mean, float g_l1_mean, const float* g_dev, float* dL_dimg1, void* stream);

/* The geometry terms both training stages add to the photometric loss (gaussian_renderer/render.py:157-188, svgss.py:297-313,
 * 333-338), fused: one forward launch plus a small fixed-order reduction, one backward launch.  `terms` is a bit set:
 *   1 surface  cos_loss(normal, depth2normal(depth, mask, camera)): normal [3,H,W], depth, mask [1,H,W], fovx / fovy / prcp as above;
 *              the pseudo normal is never stored and is the one the depth2normal entry point above writes (one device function)
 *   2 target   cos_loss(normal, target, weight=weight): target [3,H,W], weight [1,H,W] or NULL (= 1)  (the mono-normal term)
 *   4 mask     mean(opacity * (1 - maxpool9(mask))): opacity, mask [1,H,W]; the 9 x 9 window is clipped to the image
 *   8 entropy  -mean(m log o + (1 - m) log(1 - o)), o = clamp(opacity, float32(1e-6), float32(1 - 1e-6))
 * The planes of a term that is not requested may be NULL.  W or H <= 0, no term, or a term without its planes: -1 and a message.
 * cos_loss (utils/loss_utils.py:119-121): cos = sum_c (output_c * gt_c) * weight, evaluated in fp32 without contraction in the order
 * ((o0 g0) w + (o1 g1) w) + (o2 g2) w; a pixel is selected iff cos < 1.f (a NaN cos is not selected and gets zero gradient; a
 * background pixel, cos = 0, is selected and contributes 1); loss = sum_selected (1 - cos) / count; count == 0 gives NaN (torch's mean
 * of an empty selection) and zero gradients.  The selection, the count and the gradients use that fp32 cos; the VALUE of a selected
 * pixel is 1 - cos with cos in double (the surface form: on the pseudo normal restated in double from the same fp32 depth), so a loss
 * carries no rounding beyond its final one to fp32.  The entropy gradient passes where lo <= opacity <= hi, bounds included.
 *   forward : `partial` = 8 doubles per workgroup, as many workgroups as the partials function returns; `stats` [4][2] = {sum, count} per
 *             term in bit order (count = H W for the two means), device doubles, and `losses` [4] = float32(sum / count), device
 *             floats, both written for all four terms (zeros for the ones not requested).  No atomics: two runs give the same bits.
 *   backward: `stats` as the forward wrote it; `g_dev` [4] = the upstream gradients of the four losses, device floats the host never
 *             reads.  Each of dL_dnormal [3,H,W] (surface + target), dL_ddepth [1,H,W] (through the pseudo normal; a gather, no
 *             atomics) and dL_dopacity [1,H,W] (mask + entropy) that is not NULL is written completely.  The mask, the target and the
 *             weight get no gradient. */
size_t svgir_geometry_loss_partials(int32_t W, int32_t H);
int svgir_geometry_loss_forward(int32_t W, int32_t H, int32_t terms, const float* normal, const float* depth, const float* mask,
                                const float* opacity, const float* target, const float* weight, float fovx, float fovy, float prcp_x,
                                float prcp_y, double* partial, double* stats, float* losses, void* stream);
int svgir_geometry_loss_backward(int32_t W, int32_t H, int32_t terms, const float* normal, const float* depth, const float* mask,
                                 const float* opacity, const float* target, const float* weight, float fovx, float fovy, float prcp_x,
                                 float prcp_y, const double* stats, const float* g_dev, float* dL_dnormal, float* dL_ddepth,
                                 float* dL_dopacity, void* stream);

/* The edge-aware smoothness terms and the TV term of both training stages (utils/loss_utils.py:101-117 `second_order_edge_aware_loss`,
 * `first_order_edge_aware_loss`, `tv_loss`; gaussian_renderer/svgss.py:366-399, render.py:192-196), fused: up to SVGIR_SMOOTH_MAX_TERMS
 * terms of one image size in one forward launch plus a small fixed-order reduction, and one backward launch.  `terms` is a HOST array
 * of descriptors, read during the call; every plane is fp32 [.,H,W], contiguous, on the device.
 *   kind 1 first : sum_{cb,k,p} |d_k D[c,p]| exp(-|d_k I[ci,p]|) / (Cb H W)
 *   kind 2 second: sum_{cb,k,p} |d_kk D[c,p]| exp(-10 |d_k I[ci,p]|) / (Cb H W)   (the FIRST derivative of I weights the second of D)
 *   kind 3 tv    : mean((x[:,1:,:] - x[:,:-1,:])^2) + mean((x[:,:,1:] - x[:,:,:-1])^2), x = data; Ci = 0, no img, no masks
 * D = data * data_mask and I = img * img_mask, one fp32 product each (a NULL mask is 1; masks are [1,H,W]); C == Ci or one of them is 1,
 * Cb = max(C, Ci), c / ci = cb or 0 (torch broadcasting); k in {x, y}.  The derivatives are kornia's spatial_gradient(mode='sobel',
 * normalized=True): the cross-correlation of the REPLICATE-padded plane with Kx = (1 2 1)^T (-1 0 1) / 8, Ky = Kx^T (order 1) and
 * Kxx = (1 4 6 4 1)^T (-1 0 2 0 -1) / 64, Kyy = Kxx^T (order 2).  Every tap takes part, the zero ones included (0 * inf = NaN, as in
 * F.conv2d).  The VALUE of an element (cb, k, p) is evaluated in double from the fp32 planes; signs and gradients are fp32, sign(0) = 0.
 * An element whose value is NaN puts NaN into the loss and contributes to no gradient.
 *   partials: the number of 2-double records `partial` must hold: n_terms per 32 x 8 pixel tile.
 *   forward : `stats` [n_terms][4] = {sum_a, count_a, sum_b, count_b}, device doubles: first / second {sum, Cb H W, 0, 0}; tv {row sum,
 *             C (H-1) W, column sum, C H (W-1)}.  `losses` [n_terms] = float32(sum_a / count_a), tv float32(sum_a / count_a + sum_b /
 *             count_b), device floats; an empty tv mean (H or W = 1) is NaN as in torch.  No atomics: two runs give the same bits.
 *   backward: `stats` as the forward wrote it; `g` [n_terms] = the upstream gradients of the losses, device floats the host never reads.
 *             Each d_data [C,H,W] / d_img [Ci,H,W] that is not NULL is written completely, times its mask (a gather: the adjoint of the
 *             replicate padding folds every out-of-image tap back onto the border pixel it was clamped to; no atomics).  Masks get no
 *             gradient; an empty tv mean gives zero gradient.
 * n_terms outside 1 ... SVGIR_SMOOTH_MAX_TERMS, an unknown kind, C / Ci outside 1 ... 4 or not broadcastable, a missing plane, or a
 * backward that requests no gradient: -1 and a message, before any HIP call.  W * H == 0 launches nothing. */
#define SVGIR_SMOOTH_MAX_TERMS 4
typedef struct svgir_smooth_term {
    int32_t kind;                    /* 1 first, 2 second, 3 tv */
    int32_t C, Ci;                   /* 1..4; tv: Ci = 0 */
    const float *data, *img, *data_mask, *img_mask;
    float *d_data, *d_img;           /* backward only; NULL = not wanted */
} svgir_smooth_term;
size_t svgir_smooth_loss_partials(int32_t W, int32_t H, int32_t n_terms);
int svgir_smooth_loss_forward(int32_t W, int32_t H, int32_t n_terms, const svgir_smooth_term* terms, double* partial, double* stats,
                              float* losses, void* stream);
int svgir_smooth_loss_backward(int32_t W, int32_t H, int32_t n_terms, const svgir_smooth_term* terms, const double* stats, const float* g,
                               void* stream);

/* The tail of an eval view (eval_relighting_tensoIR.py:284-294, 333-378; eval_nvs.py:79; train.py:276-301): the per-view metrics, the 8-bit
 * images that get written and the albedo scale, fused in csrc/view_metrics.hip.  No entry point waits for the device, none uses atomics
 * (two runs give the same bits); invalid arguments are rejected with SVGIR_ERR_INVALID and a message before any HIP call.
 *
 * A PLANE OPERAND describes how a [3,H,W] operand is formed per pixel from what the caller holds; it is never stored.  fp32, in torch's
 * operation order, every product and sum rounded on its own (no contraction), so the composed value has the bits torch would hold:
 *   x = src[c]
 *   x = (x * scale) + offset                  skipped when scale == 1 and offset == 0        (normal * 0.5 + 0.5)
 *   x = (x * m) + ((1 - m) * f)               when mask != NULL; f = fill[c] if fill != NULL, else bg[c]
 *   x = srgb(x)                               when srgb != 0: rgb_to_srgb (utils/graphics_utils.py:198-215), NaN-propagating clip
 * src, fill: [3,H,W]; mask: [1,H,W]; contiguous fp32 device planes.  bg: three host floats.  fill without mask is invalid. */
typedef struct svgir_plane_op {
    const float *src, *mask, *fill;
    float bg[3];
    float scale, offset;
    int32_t srgb;
} svgir_plane_op;

/* Metrics of up to SVGIR_METRIC_MAX_TERMS operand pairs of one image size from one call: one launch over 16 x 16 tiles for the terms with
 * SSIM (the tiling and the SSIM arithmetic of the L1 + SSIM forward above; operands composed on load, the 26 x 26 halo is zero padding
 * applied AFTER composition), one for the terms without (no halo, no LDS passes), and a small reduction, one workgroup per term.  Per
 * pixel d = a - b in fp32; d^2 (exact in double) and |d| are summed in double per workgroup in a fixed order (wave reduction, then the
 * four waves in order), the workgroup records then in a fixed order per term.  `terms` is a HOST array read during the call.
 *   partial  svgir_view_metrics_partials(W, H, n_terms) doubles of device scratch
 *   rows     [n_terms][SVGIR_METRIC_COLS] device doubles, the caller's (e.g. row v of a [views, terms, 10] table; nothing else is touched):
 *            mse_0, mse_1, mse_2, psnr_0, psnr_1, psnr_2, mean(mse_c), mean(psnr_c), ssim, l1
 *            mse_c = mean over H W of d^2 (utils/image_utils.py:32-33); psnr_c = -10 log10(mse_c) in double = 20 log10(1 / sqrt(mse_c))
 *            (:36-37), +inf where mse_c == 0; ssim = the mean SSIM map over 3 H W, NaN when want_ssim == 0; l1 = mean |d| over 3 H W.
 *            A NaN pixel makes its own channel's columns, the two means, ssim and l1 NaN, and nothing else.
 * n_terms outside 1 ... SVGIR_METRIC_MAX_TERMS, a NULL src, fill without mask, a NULL partial / rows, W or H <= 0: -1 and a message. */
#define SVGIR_METRIC_MAX_TERMS 4
#define SVGIR_METRIC_COLS 10
typedef struct svgir_metric_term {
    svgir_plane_op a, b;
    int32_t want_ssim;
} svgir_metric_term;
size_t svgir_view_metrics_partials(int32_t W, int32_t H, int32_t n_terms);
int svgir_view_metrics(int32_t W, int32_t H, int32_t n_terms, const svgir_metric_term* terms, double* partial, double* rows, void* stream);

/* The arrays torchvision's save_image hands to PIL, for up to SVGIR_CAPTURE_MAX operands in one launch: out [n,H,W,3] uint8,
 *   out = (uint8) clamp((x * 255) + 0.5, 0, 255)
 * (torchvision.utils.save_image: `mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8)`, restated from its source;
 * unpinned by torchvision itself, which is not a dependency of this project).  The product and the sum are rounded separately in fp32,
 * the cast truncates.  DECISION: NaN gives 0 (torch leaves the cast of NaN undefined); +inf gives 255, -inf gives 0.  Every byte of out is
 * written.  An operand with srgb != 0 is rejected: powf differs from torch's pow by ulps, a byte contract cannot hold there.
 * `ops` is a HOST array read during the call.  n outside 1 ... SVGIR_CAPTURE_MAX, a NULL src / out, fill without mask, srgb != 0,
 * W or H <= 0: -1 and a message. */
#define SVGIR_CAPTURE_MAX 16
int svgir_capture_u8(int32_t W, int32_t H, int32_t n, const svgir_plane_op* ops, uint8_t* out, void* stream);

/* The albedo scale of the relighting eval (eval_relighting_tensoIR.py:285-294): over the pixels with ((r + g) + b) / 3 > 0 of
 * render_albedo [3,H,W] (fp32, that order: render_albedo.mean(dim=0) > 0), per channel the mean of clamp(gt / render, 1e-6, 1), gt =
 * gt_albedo [3,H,W], through srgb first when gt_srgb != 0.  The division is the correctly rounded fp32 one; the clamp propagates NaN
 * (gt / 0 = inf clamps to 1; 0 / 0 = NaN makes that channel NaN).  Double sums in a fixed order.
 *   partial  svgir_albedo_scale_partials(W, H) doubles of device scratch
 *   scale3   3 device floats; count: 1 device int32, the number of selected pixels.  An empty selection gives NaN and 0 (torch's mean
 *            of nothing).  scale3 can be handed on as svgir_activation.base_color_scale without visiting the host.
 * A NULL pointer, W or H <= 0: -1 and a message. */
size_t svgir_albedo_scale_partials(int32_t W, int32_t H);
int svgir_albedo_scale(int32_t W, int32_t H, const float* render_albedo, const float* gt_albedo, int32_t gt_srgb, double* partial,
                       float* scale3, int32_t* count, void* stream);

/* The exact per-column LOWER MEDIAN of an fp32 view x [n, C], C = 1 ... 4, x[i, c] = base[i * row_stride + c * col_stride] (strides in
 * elements: row_stride = C, col_stride = 1 is a row-major [n, C]; row_stride = 1, col_stride = n a planar [C, n]): the contract of
 * torch.median(x, dim=0), by radix select in csrc/select.hip -- four 8-bit digit passes over order-preserving uint32 keys, a pass over the
 * rows for the index and one single-workgroup finish: one memset and 6 launches whatever n is.  No host wait, no allocation, integer
 * atomics only: two runs give the same bits, and nothing depends on what `scratch` held before.
 *   values    [C] device floats: the element of rank (n - 1) / 2 (0-based, integer division) of each column, bit for bit an element of
 *             the column.  DECISIONS (torch leaves them open or differs): -0 and +0 are one value and come out as +0; a column with at
 *             least one NaN gives NaN (as torch); +-inf are ordinary values; n == 0 gives NaN, index -1 and counts 0 (torch raises).
 *   indices   [C] device int32: the SMALLEST row whose value equals the median (torch leaves the choice among ties unspecified); in a
 *             NaN column the smallest row that holds a NaN.
 *   n_less, n_greater   [C] device int32 each, or NULL: the rows strictly below / strictly above the median value, exact.  They are counted
 *             on the keys, where NaN stands above +inf: in a NaN column n_less is the number of rows that are not NaN, n_greater 0.
 *   scratch   svgir_column_median_scratch_bytes(n, C) bytes of device memory, 4-byte aligned (0 for arguments the call refuses).
 * C outside 1 ... 4, n < 0 or n >= 2^31, a NULL values / indices, a NULL base / scratch with n > 0: -1 and a message before any HIP call. */
size_t svgir_column_median_scratch_bytes(int64_t n, int32_t C);
int svgir_column_median(const float* base, int64_t n, int32_t C, int64_t row_stride, int64_t col_stride, void* scratch, float* values,
                        int32_t* indices, int32_t* n_less, int32_t* n_greater, void* stream);

/* The albedo scale the relighting eval APPLIES (eval_relighting_tensoIR.py:227-237; svgir_albedo_scale above is the variant of :285-294,
 * which the reference computes and never uses): per pixel, fp32 in torch's operation order, every operation rounded on its own,
 *   r_c = srgb_to_rgb(render_albedo[c]) when render_srgb != 0, else render_albedo[c]
 *         srgb_to_rgb (utils/graphics_utils.py:218-229): x <= 0.04045 ? x / 12.92 : powf((x + 0.055) / 1.055, 2.4); NaN stays NaN
 *   the pixel is selected iff ((r_0 + r_1) + r_2) / 3 > 0
 *   key_c = clamp(gt_albedo[c] / r_c, lo, hi), the clamp passing NaN: x / 0 = inf becomes hi, 0 / 0 makes that channel's scale NaN and no other
 * and scale3[c] = the lower median of key_c over the selected pixels by the selection of svgir_column_median (same rules for zeros and
 * NaN), the keys recomputed in each of its four passes: one memset and 5 launches.  render_albedo, gt_albedo: [3,H,W] contiguous device
 * floats.  The eval uses lo = 1e-6, hi = 10.
 *   scale3    3 device floats; count: 1 device int32, the number of selected pixels.  An empty selection gives NaN and 0.  scale3 can be
 *             handed on as svgir_activation.base_color_scale without visiting the host.
 *   scratch   svgir_albedo_scale_median_scratch_bytes(W, H) bytes of device memory, 4-byte aligned
 * A NULL pointer, W or H <= 0, W * H >= 2^31, lo > hi (or a NaN bound): -1 and a message before any HIP call. */
size_t svgir_albedo_scale_median_scratch_bytes(int32_t W, int32_t H);
int svgir_albedo_scale_median(int32_t W, int32_t H, const float* render_albedo, const float* gt_albedo, int32_t render_srgb, float lo, float hi,
                              void* scratch, float* scale3, int32_t* count, void* stream);

/* Stage 1's lambda_surface term (gaussian_renderer/render.py:217-222): loss = exp(-mean |xyz - median(xyz, dim=0)|), xyz [P,3] contiguous
 * device floats.  (svgir_geometry_loss_* holds the cos term the harness calls surface_loss; this is the other one.)
 *   partials: the number of DOUBLES `partial` must hold: the selection's scratch, then one record per 2048 rows.
 *   forward : the median c of svgir_column_median (its rules: a NaN coordinate makes c_c NaN), then the fp32 values |x_ic - c_c| summed in
 *             double in a fixed order (wave butterfly, the four waves in order, the workgroup records in order): one memset and 6 launches.
 *             `stats` [11] device doubles = {sum, 3 P, then per column c: index_c, n_less_c, n_greater_c}; `loss` 1 device float =
 *             float32(exp(-sum / (3 P))), the exp in double.  No float atomics: two runs give the same bits.
 *   backward: `stats` as the forward wrote it; `g` 1 device float the host never reads.  dL_dxyz [P,3] is written completely by one
 *             elementwise launch without atomics: -g L sign(x_ic - c_c) / (3 P) with sign(0) = 0, and in row index_c of column c
 *             additionally +g L (n_greater_c - n_less_c) / (3 P): torch's subgradient of median, which hands the gradient of `center`
 *             to the row it returned (here: the smallest such row).  Evaluated in double from L = the fp32 loss, rounded once.
 *             A NaN anywhere in xyz makes the loss and every element of dL_dxyz NaN, as in torch.
 * P == 0: the loss is NaN and nothing else is written (torch raises).  P < 0 or P >= 2^31, a NULL stats / loss, any other NULL pointer with
 * P > 0: -1 and a message before any HIP call. */
size_t svgir_surface_center_loss_partials(int64_t P);
int svgir_surface_center_loss_forward(int64_t P, const float* xyz, double* partial, double* stats, float* loss, void* stream);
int svgir_surface_center_loss_backward(int64_t P, const float* xyz, const double* stats, const float* g, float* dL_dxyz, void* stream);

/* LPIPS with the VGG16 backbone (lpipsPyTorch/modules/{lpips,networks,utils}.py as called with net_type='vgg' at train.py:398,
 * eval_nvs.py:81, eval_relighting_tensoIR.py:370/375), forward only, fp32 throughout, fused in csrc/lpips.hip: a stem (operands composed
 * on load, z-score, conv1_1), twelve 3 x 3 convolutions as implicit GEMM on the fp32-input MFMA, four 2 x 2 max pools, five tap kernels
 * and one reduction -- 23 launches per call, whatever n_pairs is.  No entry point waits for the device, allocates or uses atomics; two
 * runs give the same bits, and the result does not depend on what the workspace held before.
 *
 * THE NETWORK.  svgir_lpips_pack turns torch's tensors (device fp32, contiguous) into the kernels' layout, once: conv_w[l] [Cout,Cin,3,3]
 * and conv_b[l] [Cout] of the thirteen convolutions of torchvision's vgg16().features in order (features.0, 2, 5, 7, 10, 12, 14, 17, 19, 21,
 * 24, 26, 28), lin_w[k] [C_k] of the five 1 x 1 layers (C_k = 64, 128, 256, 512, 512).  conv_w / conv_b / lin_w are HOST arrays of device
 * pointers read during the call.  packed: svgir_lpips_packed_floats floats of device memory, 16-byte aligned.
 *
 * THE ARITHMETIC, per image (image 2 p is operand a of pair p, image 2 p + 1 operand b; an image's bits depend on its own pixels only, not
 * on its position in the call nor on the other images, so a pair of equal images scores exactly 0 and a pair scores the same alone or
 * among four):
 *   x    = the plane operand (above), used as given: no rescale to [-1, 1]
 *   z    = (x - mean_c) / std_c            mean = -0.030, -0.088, -0.188; std = 0.458, 0.448, 0.450; the correctly rounded fp32 division
 *   conv = 3 x 3, zero padding 1 applied to z (not to x); per output one fmaf chain over (input channel, ky, kx) for every 64 input channels,
 *          the chains added in channel order, the bias last, then ReLU -- an order that depends on the layer's shape only
 *   pool = 2 x 2 / stride 2 maximum, floor sizes, after relu1_2, relu2_2, relu3_3, relu4_3 (never after relu5_3)
 * NaN propagates as in torch: relu(NaN) = NaN, a pooled NaN stays NaN; a non-finite input pixel gives a NaN score.
 *   tap_k, k = 0 ... 4, from f = relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 BEFORE the pool, per pixel, all fp32, no contraction:
 *          n   = sqrt(sum_c f_c^2)                      for a and for b
 *          u_c = f_c / (n + 1e-10)                      (an all-zero vector gives zeros, not NaN)
 *          s   = sum_c w_kc * ((ua_c - ub_c) * (ua_c - ub_c))
 *          tap_k = (float)(the mean of s over the H_k W_k pixels, summed in double in a fixed order)
 *   score = (float)((((tap_0 + tap_1) + tap_2) + tap_3) + tap_4), the taps as doubles
 *   work      svgir_lpips_work_bytes bytes of device scratch, 16-byte aligned: two activation buffers of [2 n_pairs][H][W][64] floats
 *             (channels-contiguous) and the workgroup records
 *   taps      [n_pairs][5] device floats; score [n_pairs] device floats; every element is written
 *   tap_maps  NULL, or a HOST array of five device pointers: tap k's feature maps f as [2 n_pairs, C_k, H_k, W_k] floats (NCHW, H_k =
 *             H >> k, W_k = W >> k), written completely; for tests (five more launches)
 * `pairs` is a HOST array read during the call.  n_pairs outside 1 ... SVGIR_METRIC_MAX_TERMS, W or H below 16 (relu5_3 would be empty;
 * torch raises there too), a NULL src, fill without mask, a NULL or misaligned packed / work, a NULL taps / score / tap_maps entry: -1 and a
 * message before any HIP call.  svgir_lpips_work_bytes returns 0 for arguments the call would refuse.
 * Unpinned by the published weights: the arithmetic is tested against torch with seeded weights of the same shapes. */
typedef struct svgir_lpips_pair {
    svgir_plane_op a, b;
} svgir_lpips_pair;
size_t svgir_lpips_packed_floats(void);
int svgir_lpips_pack(const float* const conv_w[13], const float* const conv_b[13], const float* const lin_w[5], float* packed, void* stream);
size_t svgir_lpips_work_bytes(int32_t W, int32_t H, int32_t n_pairs);
int svgir_lpips(int32_t W, int32_t H, int32_t n_pairs, const svgir_lpips_pair* pairs, const float* packed, void* work, float* taps,
                float* score, float* const* tap_maps, void* stream);

/* The model's activation getters, fused (scene/gaussian_model.py:104-125, 270-355: get_scaling, get_rotation, get_opacity, get_geo_normal,
 * get_shading_normal, get_base_color / get_albedo, get_roughness; gaussian_renderer/svgss.py:109: viewdirs; svgss.py:316: the regulariser
 * mse_loss(_normal, 0)): the step from the optimizer's raw parameters to what the shading and the rasterizer consume, one forward launch
 * (plus a one-workgroup reduction when normal_reg is requested) and one backward launch.  All tensors are device fp32, contiguous; the 4-
 * and 12-float rows must be 16-byte aligned (they move as float4).
 *   raw inputs : xyz [P,3], scaling [P,3], rotation [P,4] as (r,x,y,z), opacity [P,1], normal [P,12] (index c * 4 + v: channel c of corner
 *                v), base_color [P,12], roughness [P,4]; base_color_scale [3] (NULL = ones), campos [3].  A raw input may be NULL when no
 *                requested output (backward: no requested result) reads it -- stage 1 passes no material pointers.
 *   outputs    : each optional (NULL = not produced); every element of a requested one is written, no other memory is touched.
 *     scales [P,3]            exp(s); NaN -> 1e-6, +inf (an exp that overflows fp32) -> FLT_MAX
 *     rotations [P,4]         q / max(|q|, 1e-12); NaN -> 1e-6.  A row whose norm is not finite: finite / inf = 0, inf / inf = NaN -> 1e-6
 *                             (+-inf would become +-FLT_MAX as in nan_to_num, but cannot arise: |q / |q|| <= 1)
 *     opacities [P,1]         sigmoid(o)
 *     geo_normal [P,3]        (2 (x z + r y), 2 (y z - r x), 1 - 2 (x x + y y)) of the ACTIVATED rotation; not renormalised
 *     shading_normal [P,4,3]  corner v, channel c: normalize(geo_normal + normal[p, c * 4 + v]), norm clamped at 1e-12
 *     shading_normal12 [P,12] the same numbers at index c * 4 + v (the transpose(1, 2).reshape get_radiance_loss builds)
 *     out_base_color [P,12]   (sigmoid(b_j) * 0.77 + 0.03) * base_color_scale[j / 4]
 *     out_roughness [P,4]     sigmoid(r) * 0.9 + 0.09; NaN -> 1e-8
 *     viewdirs [P,3]          normalize(campos - xyz), norm clamped at 1e-12
 *     normal_reg              float32(sum / (12 P)), sum = sum of normal^2 over the 12 P elements in double: `partial` =
 *                             svgir_activate_partials(P) doubles (one per workgroup: lane sums in index order, xor butterfly per wave,
 *                             the waves in order), added in a fixed order by the reduce kernel into normal_reg_sum (device double) and
 *                             normal_reg (device float).  No atomics: two runs give the same bits.  The reference's 0.1 stays in the caller.
 *   Arithmetic: every value is evaluated in double from the fp32 inputs (exp included; sigmoid from e = exp(-|x|) as 1 / (1 + e) or
 *   e / (1 + e), its derivative as e / (1 + e)^2) and rounded to fp32 once.  Norms are double and do not overflow where an fp32 norm would.
 *   A replaced element holds the fp32 constant (1e-6f, 1e-8f, FLT_MAX).  The same code runs whatever set of outputs is requested: an
 *   output requested alone has the bits it has when all are requested.
 *   backward   : autograd of the lines above, recomputed from the raw inputs (the forward saves nothing).  svgir_activation_grads holds one
 *     upstream gradient per output (NULL = the output is outside the graph and contributes nothing; dL_dnormal_reg is ONE device float, the
 *     caller's weight included) and one result per raw input; each result that is not NULL is WRITTEN COMPLETELY (no accumulation, no
 *     pre-clear).  dL_drotation collects rotations, geo_normal and the shading normals through geo_normal; dL_dnormal the shading normals
 *     (both layouts) and the regulariser (g 2 normal / (12 P)); dL_dxyz only viewdirs (the caller adds the rasterizer's).  normalize's
 *     clamp as in torch: norm < 1e-12 gives g / 1e-12 (a zero quaternion: finite), else (g - u (g . u)) / norm.
 *     ONE DECISION of this project's own: where nan_to_num replaced a value, the raw element gets ZERO gradient -- a scaling element whose
 *     exp is NaN or overflows, a NaN roughness element, and the WHOLE rotation row when its norm is not finite.  Torch yields NaN there,
 *     which the reference scrubs in replace_nangrad_to_zero.  Everything else propagates as in autograd (a NaN opacity, base_color, offset
 *     or position gives NaN), and upstream NaNs pass through unchanged.
 *   P == 0: success, nothing launched.  P < 0, a requested output / result whose raw input (or campos; normal_reg: partial and
 *   normal_reg_sum) is missing, the shading normals' gradient without both rotation and normal, a misaligned row, nothing requested: -1 and
 *   a message, before any HIP call. */
typedef struct svgir_activation {
    int32_t P;
    const float *xyz, *scaling, *rotation, *opacity, *normal, *base_color, *roughness;   /* raw parameters */
    const float *base_color_scale, *campos;
    float *scales, *rotations, *opacities, *geo_normal, *shading_normal, *shading_normal12, *out_base_color, *out_roughness, *viewdirs;
    double *partial, *normal_reg_sum;
    float *normal_reg;
} svgir_activation;
typedef struct svgir_activation_grads {
    const float *dL_dscales, *dL_drotations, *dL_dopacities, *dL_dgeo_normal, *dL_dshading_normal, *dL_dshading_normal12;
    const float *dL_dout_base_color, *dL_dout_roughness, *dL_dviewdirs, *dL_dnormal_reg;
    float *dL_dxyz, *dL_dscaling, *dL_drotation, *dL_dopacity, *dL_dnormal, *dL_dbase_color, *dL_droughness;
} svgir_activation_grads;
size_t svgir_activate_partials(int32_t P);
int svgir_activate_forward(const svgir_activation* a, void* stream);
int svgir_activate_backward(const svgir_activation* a, const svgir_activation_grads* g, void* stream);

/* The consumers of the rasterizer's gradients: Adam over the per-Gaussian parameter block, the
 * densification statistics, and the row compaction behind pruning (scene/gaussian_model.py:737-773, 1020-1062, 1270-1276).
 *
 * svgir_adam_step: one launch for up to SVGIR_ADAM_MAX_TENSORS parameter tensors -- torch.optim.Adam's update (amsgrad
 *   off, no weight decay) with a learning rate and a step count per tensor (`step` = the count AFTER this update, >= 1;
 *   bias corrections in double precision on the host, like torch).  Tensors with n = 0 are skipped.
 * svgir_densify_stats: GaussianModel.add_densification_stats -- weights_accum += weights (if given);
 *   for rows with update_filter: xyz_gradient_accum += |viewspace_grad[:, :2]|, denom += 1.  grad_stride = floats per row
 *   of viewspace_grad (3 in the reference).
 * svgir_mask_scan: order-preserving list `kept` [<= P] of the rows with keep != 0 and their number (count_dev[0], device
 *   memory); `work` = svgir_mask_scan_work_words(P) uint32 of scratch.
 * svgir_gather_rows: dst[t][r] = src[t][kept[r]] for r < min(rows_max, *count_dev), for up to SVGIR_ADAM_MAX_TENSORS
 *   tensors with rows of row_bytes (multiple of 4) in one launch: the `tensor[mask]` of _prune_optimizer for every
 *   parameter, both Adam moments and the bookkeeping arrays at once. */
#define SVGIR_ADAM_MAX_TENSORS 32
/* svgir_adam_tensor.flags -- GaussianModel.step() (scene/gaussian_model.py:775-813) folded into the Adam pass:
 *   SVGIR_ADAM_SCRUB_NAN : replace_nangrad_to_zero -- NaN gradient entries are replaced by `nan_value` (0 or 1e-6 by group)
 *                          before the update, and in the gradient tensor itself;
 *   SVGIR_ADAM_ZERO_GRAD : optimizer.zero_grad() -- the gradient tensor is left zero-filled. */
#define SVGIR_ADAM_SCRUB_NAN 1
#define SVGIR_ADAM_ZERO_GRAD 2
typedef struct svgir_adam_tensor {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
    int64_t n;        /* elements */
    double lr;
    int32_t step;
    int32_t flags;    /* SVGIR_ADAM_* (the gradient is written when a flag is set) */
    float nan_value;
} svgir_adam_tensor;
typedef struct svgir_row_tensor { const void* src; void* dst; int32_t row_bytes; } svgir_row_tensor;
int svgir_adam_step(const svgir_adam_tensor* tensors, int32_t count, double beta1, double beta2, double eps, void* stream);
int svgir_densify_stats(int32_t P, const float* viewspace_grad, int32_t grad_stride, const uint8_t* update_filter,
                        const float* weights, float* weights_accum, float* xyz_gradient_accum, float* denom, void* stream);
size_t svgir_mask_scan_work_words(int32_t P);
int svgir_mask_scan(int32_t P, const uint8_t* keep, uint32_t* kept, uint32_t* work, uint32_t* count_dev, void* stream);
int svgir_gather_rows(const svgir_row_tensor* tensors, int32_t count, const uint32_t* kept, const uint32_t* count_dev,
                      int32_t rows_max, void* stream);

/* The producer of the visibility the shading kernels stream: a linear BVH over the surfels and the
 * visibility tracer of submodules/bvh (`RayTracer`, __init__.py:28-71; `create_bvh` src/bvh.cu:8-28 + src/construct.cu:151-265;
 * `trace_bvh_opacity` src/bvh.cu:86-115 + src/trace.cu:186-262).
 *   svgir_bvh_bytes : size of the opaque BVH blob for P surfels.
 *   svgir_bvh_build : leaf boxes from the eight corners mean +- 3 (s_a a +- s_b b +- s_c c) (a, b, c = columns of the
 *       rotation of the normalised quaternion), Morton sort, hierarchy, bottom-up refit.  means3D [P,3], scales [P,3],
 *       rotations [P,4] (r,x,y,z; need not be normalised).
 *   svgir_bvh_trace_visibility : per ray, origin rays_o + t_offset * rays_d (the reference's caller passes 0.05), the
 *       product of (1 - opacity exp(power)) over the surfels whose leaf box the ray enters, with opacity >= 1/255, facing
 *       the ray (normal . d <= 0), t >= 0.01 and power <= 0, where t = (m^T C d) / (d^T C d) and
 *       power = -1/2 (mean - x(t))^T C (mean - x(t)); visibility = 0 (and contribute = 0) as soon as the product drops
 *       below 0.9, else the product and the number of contributing surfels.  means3D [P,3], cov_inv [P,6] (symmetric,
 *       xx xy xz yy yz zz), opacity [P], normals [P,3] may differ from the arrays the BVH was built from (they do in the
 *       reference: build from scaling/rotation, trace with the inverse covariance); rays_o / rays_d [num_rays,3];
 *       contribute [num_rays] int32, visibility [num_rays]. */
size_t svgir_bvh_bytes(int32_t P);
int svgir_bvh_build(int32_t P, const float* means3D, const float* scales, const float* rotations, char* bvh, void* stream);
int svgir_bvh_trace_visibility(int32_t P, char* bvh, int64_t num_rays, const float* rays_o, const float* rays_d, float t_offset,
                               const float* means3D, const float* cov_inv, const float* opacity, const float* normals,
                               int32_t* contribute, float* visibility, void* stream);

/* The producer of the incident-radiance cache (the other half of row f3): the linear BVH and the closest-hit radiance
 * tracer of the reference's point-based-GI renderer (pbgi/bvhhelpers.py:96-156 `get_gs_bvh`; pbgi/renderer.py:582-615
 * `build_bvh`, `render_radiance_with_sampling_SH`; the slang kernels under pbgi/bvhworkers/: get_elements,
 * lbvh_morton_codes, lbvh_single_radixsort, lbvh_hierarchy, lbvh_bounding_boxes, intersect_test:1879-1990, sh_utils),
 * called by GaussianModel.update_radiace (scene/gaussian_model.py:469-522).
 *   svgir_pbgi_bvh_bytes  : size of the opaque blob for P >= 1 primitives.
 *   svgir_pbgi_bvh_build  : boxes centre +- 3 max|scale| (centers [P,3], scales [P,3]), 30-bit Morton codes of the box
 *       centres in the scene extent, stable sort by code, Karras hierarchy (equal codes resolved by sorted position),
 *       bottom-up box unions.  The tree is the reference's tree node for node (the tracer's result depends on it).
 *   svgir_pbgi_bvh_export : the tree as the reference's tensors: info [2P-1][3] int32 = {left, right, primitive}
 *       (`LBVHNode_info`), aabb [2P-1][6] (`LBVHNode_aabb`); optionally the sorted (code, primitive) pairs [P][2].
 *   svgir_pbgi_trace_radiance : N rows x S rays; ray_o [N,3] (one origin per row), ray_d [N,S,3].  Per ray: repeated
 *       closest-hit queries over t in [0.042 (0.01 after the first hit), 0.2] from the moving origin; each accepted hit adds
 *       eval_sh(degree 3, shs [P,16,3], direction origin -> hit centre) * alpha * T and multiplies T by (1 - alpha), until
 *       T <= 0.001, no hit, or the hit is the primitive whose index equals the ROW of the ray.  Outputs: radiance [N,S,3]
 *       clamped to [0,10], visibility [N,S] (T, or 0 once T < 0.2), hit_indices [N,S] int32 (first hit or -1), uvs [N,S,2].
 *       rotations [P,4] (r,x,y,z), normals [P,3], opacity [P], cov3D_inverse [P,6] (xx xy xz yy yz zz).
 *       oracle/pbgi_oracle.cpp lists the reference's traversal quirks that are reproduced.
 *       The blob is NOT read-only during a trace: the per-call leaf records, the row order of the call and its ray queue live in it.
 *       Calls that share one blob (build, trace) must therefore be ordered on ONE stream (or by events); concurrent traces from several
 *       streams / threads need one blob each (a build is 6 launches). */
size_t svgir_pbgi_bvh_bytes(int32_t P);
int svgir_pbgi_bvh_build(int32_t P, const float* centers, const float* scales, char* bvh, void* stream);
int svgir_pbgi_bvh_export(int32_t P, char* bvh, int32_t* info, float* aabb, int32_t* sorted, void* stream);
int svgir_pbgi_trace_radiance(int32_t P, char* bvh, int32_t N, int32_t S, const float* ray_o, const float* ray_d, const float* centers,
                              const float* scales, const float* rotations, const float* normals, const float* opacity,
                              const float* cov3D_inverse, const float* shs, float* radiance, float* visibility, int32_t* hit_indices,
                              float* uvs, void* stream);

/* The consumers of those caches: the pbgi irradiance kernels (pbgi/renderer.py:100-226, 743-751 `render_irradiance`,
 * `render_irradiance_sample`; pbgi/bvhworkers/intersect_test.slang:901-1360; the brdf is `shading_brdf_simple`, pbr.slang:283-329), called
 * by GaussianModel.get_radiance_loss on every stage-2 iteration and by GaussianModel.calculate_radiance at relighting
 * (scene/gaussian_model.py:530-575).  They trace nothing: they gather through the cached first hits.
 *   All arithmetic is fp32, all indices int32, and N = P: rows and hit surfels index the same arrays.
 *   ray_d [N,S,3]; envmap [N,S,3] (the caller's direct_light(incident_dirs) * incident_areas); normals [N,12] and albedos [N,12] as
 *   channel * 4 + corner (get_shading_normal.transpose(1,2).reshape(N,-1)); roughnesses [N,4]; hit_indices [N,S] (first hit or -1);
 *   uvs [N,S,2]; sample_indices [N] (the sample form).
 *   brdf(V, L, n, albedo, r): n, V, L normalised (x / sqrt((x.x*x.x + x.y*x.y) + x.z*x.z)), H = normalize(V + L); NoL, NoV, NoH, VoH =
 *   clamp(dot, 1e-6, 1) (the reference's abs on NoV is overwritten and has no effect); a = r*r, a2 = a*a, k = ((a + 2r) + 1) / 8;
 *   F = 0.04 + 0.96 * 2^((-5.55473 VoH - 6.98316) VoH); n0 = NoH*NoH*(a2 - 1) + 1, n1 = NoV (1 - k) + k, n2 = NoL (1 - k) + k;
 *   spec = (F a2) / clamp(4pi n0 n0 n1 n2, 1e-6, 4pi); brdf = spec + albedo * (1/pi).
 *   Corner weights of uv = (u, v): w = ((1-u)(1-v), u(1-v), (1-u)v, uv).
 *   svgir_pbgi_irradiance_sample : out [N,3].  Per row i: p = sample_indices[i], h = hit_indices[i,p],
 *       out[i,c] = sum over s with hit_indices[h,s] == -1 of
 *                  (sum_k w_k(uvs[h,s]) brdf(-ray_d[i,p], ray_d[h,s], normal_k[h], albedo_k[h], roughnesses[h,0])_c) * envmap[h,s,c] / S.
 *       Two quirks of the reference are kept: corner 0's roughness serves all four corners, and there is no n.l cosine factor.
 *   svgir_pbgi_irradiance : out [N,S,3], forward only.  Per (i,p) the same sum with roughnesses[h,k] per corner and every corner term
 *       multiplied by clamp(dot(normal_k[h], normalize(ray_d[h,s])), 1e-6, 1) (the stored normal, not the normalised one).
 *   svgir_pbgi_irradiance_sample_backward : with g = d_out [N,3], summed over all rows i and samples s that contribute:
 *       d_albedos[h,4c+k] += g_c w_k envmap[h,s,c] / (pi S);  d_envmap[h,s,c] += g_c irr_c / S (irr = the corner-blended brdf);
 *       d_roughnesses[h,0] += (sum_c g_c envmap[h,s,c] / S) (sum_k w_k d spec_k / d r): where the denominator lies inside
 *       [1e-6, 4pi] its derivative is passed, outside it is zero; columns 1-3 of d_roughnesses are zero.  Directions, normals and uvs
 *       get no gradient (no_diff in the reference).  The call writes every element of d_envmap [N,S,3], d_albedos [N,12] and
 *       d_roughnesses [N,4]: it clears them itself.
 *   Three things the reference leaves undefined are decided here:
 *     - A missed primary ray gives zeros.  When h == -1 the row (the [i,p] entry) is zero and contributes no gradient.  (The
 *       reference stores through a three-index access into its [N,3] result there; the intended value is the zero the tensor was
 *       created with.)
 *     - The sum is a sum.  The reference accumulates with a non-atomic += from S threads; here the result is the mathematical sum
 *       over s, in a free but fixed order: the forward gives the same bits for the same input.  The backward adds with float
 *       atomics where rows share a hit surfel and is repeatable only up to the order of those adds.
 *     - Nothing reads out of bounds.  sample_indices[i] outside [0,S), or a first hit h outside [-1,N), is treated as a miss.  The
 *       hit index of a SECONDARY sample is never used as an address: the sample contributes when it is exactly -1.
 *   A fourth decision is this project's own:
 *     - n0 is evaluated without cancellation.  Where n.H >= 1e-6 the kernels compute n0 = |H - (n.H) n|^2 (1 - a2) + a2 instead of
 *       the reference's NoH*NoH*(a2 - 1) + 1.  For unit vectors it is the same number, so the contract's value is unchanged, but
 *       the reference's form loses fp32's absolute 1e-7 against an n0 that goes down to a2 (4e-4 of a term at r = 0.14,
 *       NoH = 0.9997; this form 2e-5 there).  The results therefore differ from an fp32 evaluation of the reference's formula
 *       by that formula's own error: up to 2e-2 absolute in single outputs at N = 200 k.
 *   With -ray_d[i,p] == ray_d[h,s] (a zero half vector) or non-finite inputs the arithmetic propagates as it does in the reference.
 *   The reference's kernels also read metallics, opacities, SHs, centers, scales, rotates and the LBVH tensors; none of them reaches
 *   the result (eval_sh is dead code there), so they are no arguments here.
 * Everything is launched on `stream`; nothing waits on the host; N = 0 launches nothing. */
int svgir_pbgi_irradiance_sample(int32_t N, int32_t S, const int32_t* sample_indices, const float* ray_d, const float* envmap,
                                 const float* normals, const float* albedos, const float* roughnesses, const int32_t* hit_indices,
                                 const float* uvs, float* out, void* stream);
int svgir_pbgi_irradiance_sample_backward(int32_t N, int32_t S, const int32_t* sample_indices, const float* ray_d, const float* envmap,
                                          const float* normals, const float* albedos, const float* roughnesses,
                                          const int32_t* hit_indices, const float* uvs, const float* d_out, float* d_envmap,
                                          float* d_albedos, float* d_roughnesses, void* stream);
int svgir_pbgi_irradiance(int32_t N, int32_t S, const float* ray_d, const float* envmap, const float* normals, const float* albedos,
                          const float* roughnesses, const int32_t* hit_indices, const float* uvs, float* out, void* stream);

/* The whole radiance-consistency loss of GaussianModel.get_radiance_loss (scene/gaussian_model.py:544-575) as one forward and one backward
 * call: the selection of the sample, the light of the hit surfel looked up inside the kernel, the irradiance sum above and the L1 against
 * the cached radiance.  L = mean over [N,3] of |R - T|.  No [N,S,3] light tensor and no [N,S,3] gradient exist on this path.
 *   Inputs (svgir_radiance_loss_params; all device pointers, fp32 / int32, contiguous): xyz [N,3], camera_center [3], geo_normal [N,3],
 *   ray_d [N,S,3] (the incident directions: both the selection's and the kernels' ray_d), areas [N,S], visibility [N,S], normals /
 *   albedos [N,12], roughnesses [N,4], hit_indices [N,S], uvs [N,S,2] as above; radiances [N,S,3] (the raw cache), radiance_ratio [1];
 *   the light: env [env_h,env_w,3] with env_softplus / env_scale (f = softplus, scale 2: DirectLightMap; f = identity, scale 1: EnvLight's
 *   32 x 64 resample) and env_transform (device [9], row-major, or null: the lookup direction is transform * d, EnvLight.transform).
 *   work: svgir_radiance_loss_work_bytes(N, env_h, env_w) bytes of scratch, 16-byte aligned (the f(env) table, the env-gradient table, the
 *   partial sums); written by each call and free again when its kernels have run; the backward needs no content from the forward.
 *   Selection, per row i: v = (xyz_i - c) / max(|xyz_i - c|, 1e-12), r = (2 (g_i . v)) g_i + v, score_s = dot(ray_d[i,s], r) *
 *   (1 - visibility[i,s]); every operation a separate fp32 one (no contraction; dot = (x*x + y*y) + z*z; correctly rounded sqrt and
 *   divide).  p = sample_indices[i] follows torch.argmax: the first index of the maximum; a NaN score beats every number and the first
 *   NaN wins; +0 and -0 tie.  (A surfel at the camera centre has v = 0, every score +-0, p = 0.)
 *   R [N,3] = svgir_pbgi_irradiance_sample's sum for (i, p) -- both quirks and all four decisions above hold -- with
 *   envmap[h,s,c] = (env_scale * bilinear(f(env))(ray_d[h,s]))_c * areas[h,s]: the lat-long lookup of the shading kernels on the RAW
 *   direction d (phi = acos(d.z) - 1e-6, theta = atan2(d.y, d.x); grid_sample with align_corners, zero padding: a tap outside the map
 *   adds exactly 0, a tap inside is multiplied even at weight 0) on the same f(env) table, with the transform, the angles and the grid
 *   coordinates in fp64 and the four weights rounded to fp32 at the end: a texel's gradient is a sum of (upstream * weight) terms, and
 *   an fp32 coordinate, off by about env_w * 2^-24 texels absolutely, would leave a small weight few digits.  |d.z| > 1 has no
 *   latitude: the acos is NaN, the sample's light is NaN (as the reference's arccos makes it) and so is R of every row that sums it.
 *   T[i,c] = radiances[i,p,c] * radiance_ratio with NaN replaced by 0 (get_radiances' nan_to_num(nan = 0)); +-inf stays -- torch's
 *   nan_to_num would also clamp an infinite product to the largest finite number; here it stays infinite and falls under the non-finite
 *   rule below.
 *   svgir_radiance_loss_forward writes sample_indices [N], radiance = R [N,3], *loss_sum = sum |R - T| (each difference fp32, summed in
 *       double: per row, per workgroup, then a fixed tree) and *loss = fp32(loss_sum / 3N).  The same input gives the same bits.
 *   svgir_radiance_loss_backward, from the forward's sample_indices and radiance and the upstream scalar *d_loss (device): d_R[i,c] =
 *       d_loss * sign(R - T) / 3N, d_albedos [N,12] and d_roughnesses [N,4] as svgir_pbgi_irradiance_sample_backward gives for d_out = d_R;
 *       d_env [env_h,env_w,3] (may be null: not wanted) = f'(env) * sum over contributing (i, s, c) and the four taps j of
 *       d_R[i,c] irr_c / S * areas[h,s] * env_scale * w_j; *d_radiance_ratio (may be null) = sum -d_R[i,c] radiances[i,p,c] over the
 *       elements whose product radiances * ratio is finite.  Every element of every output is written; the call clears what it
 *       accumulates into.  Rows that share a hit surfel and samples that share a texel add with float atomics: the backward is
 *       repeatable only up to the order of those adds (d_radiance_ratio is a fixed tree and is repeatable).
 *   One more decision of this project's own:
 *     - A non-finite value gives no gradient.  Where R[i,c] or T[i,c] is not finite the loss is NaN, as in torch, but d_R[i,c] = 0: the
 *       element contributes to no gradient.  The rule is per element: a light that is NaN or infinite in one channel only is left
 *       out of that channel's sums (skipped, not multiplied by 0) and the other channels of the row contribute as usual.  (Torch propagates sign(NaN) = NaN into every gradient the row touches and from there into
 *       the whole env map.)  An element of d_env nothing was added to is exactly 0 whatever env holds there.
 *   N = 0 launches nothing and writes nothing; the loss of no rows is NaN (torch's mean of an empty tensor), which is the caller's to
 *   return.  Everything is launched on `stream`; nothing waits on the host. */
typedef struct svgir_radiance_loss_params {
    int32_t N, S;
    const float* xyz;
    const float* camera_center;
    const float* geo_normal;
    const float* ray_d;
    const float* areas;
    const float* visibility;
    const float* normals;
    const float* albedos;
    const float* roughnesses;
    const int32_t* hit_indices;
    const float* uvs;
    const float* radiances;
    const float* radiance_ratio;
    const float* env;
    int32_t env_h, env_w, env_softplus;
    float env_scale;
    const float* env_transform;
    void* work;
} svgir_radiance_loss_params;
size_t svgir_radiance_loss_work_bytes(int32_t N, int32_t env_h, int32_t env_w);
int svgir_radiance_loss_forward(const svgir_radiance_loss_params* p, int32_t* sample_indices, float* radiance, double* loss_sum, float* loss,
                                void* stream);
int svgir_radiance_loss_backward(const svgir_radiance_loss_params* p, const int32_t* sample_indices, const float* radiance,
                                 const float* d_loss, float* d_env, float* d_albedos, float* d_roughnesses, float* d_radiance_ratio,
                                 void* stream);

/* The fused radiance-consistency loss under a spherical-Gaussian light (added within ABI 14; GaussianModel.get_radiance_loss with
 * train.py:65-66's DirectLightSG).  The env* fields of `p` are ignored; p->work has svgir_radiance_loss_sg_work_bytes(N, count) bytes,
 * 16-byte aligned (the lobes' table-space sums and the partial sums; 0 for N < 0 or a count outside 1 ... SVGIR_SG_MAX_LOBES);
 * light->work is built by each call.  Everything above holds word for word -- the selection (it does not see the light), the hit rules,
 * the four irradiance decisions, the target, the loss sum's order, the per-element non-finite rule, complete writes, N = 0 -- except
 *     envmap[h,s,c] = L_c(ray_d[h,s]) * areas[h,s],   L the unclamped fp32 light of svgir_sg_eval on the raw direction (m ascending).
 * Backward: the adjoint of L_c at (h,s) is g_c = d_R[i,c] irr_c / S * areas[h,s] (a channel without upstream is skipped, not multiplied
 * by 0); it feeds the seven sums per lobe of svgir_sg_eval_backward -- fp64 in LDS per workgroup, one float-atomic flush, the pull-back
 * -- and d_lobes [M,7] (may be null: not wanted) is written completely.  d_lobes, like d_env, is repeatable only up to the order of
 * those adds; d_albedos / d_roughnesses / d_radiance_ratio are as above.  An invalid light or parameter block is rejected with
 * SVGIR_ERR_INVALID and a message before any HIP call. */
size_t svgir_radiance_loss_sg_work_bytes(int32_t N, int32_t count);
int svgir_radiance_loss_forward_sg(const svgir_radiance_loss_params* p, const svgir_sg_light* light, int32_t* sample_indices,
                                   float* radiance, double* loss_sum, float* loss, void* stream);
int svgir_radiance_loss_backward_sg(const svgir_radiance_loss_params* p, const svgir_sg_light* light, const int32_t* sample_indices,
                                    const float* radiance, const float* d_loss, float* d_lobes, float* d_albedos, float* d_roughnesses,
                                    float* d_radiance_ratio, void* stream);

/* Exact k-nearest-neighbour search over a point cloud: simple_knn's `distCUDA2` (submodules/simple-knn/simple_knn.cu:147-221; the initial
 * scales of GaussianModel.create_from_pcd) and custom_knn's `topKdistCUDA2` (no source upstream; get_knn_loss,
 * scene/gaussian_model.py:577-592).  points [P,3]; `work` is svgir_knn_bytes bytes of scratch, written by the call and free again when the
 * call's kernels have run; everything is launched on `stream` and nothing waits on the host.
 *   The result is a pure function of the input.  For point i and every j != i: d = p_j - p_i per component,
 *   dist = (d.x*d.x + d.y*d.y) + d.z*d.z in fp32, each operation rounded (no fused multiply-add).  Candidates are ordered by
 *   (dist, j) ascending; a candidate whose dist is NaN or +inf is not a neighbour.  i is never its own neighbour; a coincident point is
 *   one, at distance 0.
 *   svgir_knn_bytes     : size of the scratch for P points.
 *   svgir_knn_mean_dist : out_mean [P] = ((b0 + b1) + b2) / 3.0f in fp32 (correctly rounded), b = the three smallest dist in ascending
 *       order, FLT_MAX where there is no neighbour (simple_knn's values: +inf for P <= 2, about 1.13e38 for P = 3).
 *   svgir_knn_topk      : K = 8.  out_dist [P,8], out_idx [P,8] int32, row i = the 8 first candidates of i in the order above; a slot
 *       without a neighbour holds dist = +inf and idx = i (an index that is always in range).
 * P = 0 launches nothing. */
size_t svgir_knn_bytes(int32_t P);
int svgir_knn_mean_dist(int32_t P, const float* points, float* out_mean, char* work, void* stream);
int svgir_knn_topk(int32_t P, const float* points, float* out_dist, int32_t* out_idx, char* work, void* stream);

/* Densification (scene/gaussian_model.py:1064-1248).
 * svgir_densify_masks : the selection of densify_and_clone / densify_and_split from the statistics densify_and_prune
 *   derives (grads = xyz_gradient_accum / denom and normal_gradient_accum / denom, NaN -> 0).  The clone test is on the norm, the
 *   split test on the signed value, as in the reference: clone_mask = (|grads| >= grad_threshold or |grads_normal| >=
 *   normal_threshold) and max(get_scaling) <= size_limit (= percent_dense * scene_extent); split_mask = (grads >= grad_threshold or
 *   grads_normal >= normal_threshold) and max(get_scaling) > size_limit.  normal_gradient_accum may be NULL.
 * svgir_append_rows : cat_tensors_to_optimizer / densification_postfix for up to SVGIR_ADAM_MAX_TENSORS per-row tensors in
 *   one launch: dst = cat(src[0:rows_old], repeat(src[list[0:n]], repeat)), n = min(n_sel_max, *count_dev) (list / count_dev
 *   as produced by svgir_mask_scan); SVGIR_APPEND_ZERO_NEW leaves the new rows zero (the Adam moments of the new points).
 *   dst holds rows_old + n_sel_max * repeat rows of row_bytes (multiple of 4).
 * svgir_split_transform : densify_and_split's new points, in place on the n_new appended copies of the selected rows:
 *   xyz <- R(rotation) (z * exp(scaling)) + xyz, scaling <- log(exp(scaling) / (0.8 N)) with the last axis at -1e10;
 *   z [n_new,3] = the standard-normal draws (torch.normal(mean = 0, std = stds) = stds * z). */
#define SVGIR_APPEND_ZERO_NEW 1
typedef struct svgir_append_tensor { const void* src; void* dst; int32_t row_bytes; int32_t flags; } svgir_append_tensor;
int svgir_densify_masks(int32_t P, const float* xyz_gradient_accum, const float* normal_gradient_accum, const float* denom,
                        const float* scaling_raw, float grad_threshold, float normal_threshold, float size_limit,
                        uint8_t* clone_mask, uint8_t* split_mask, void* stream);
int svgir_append_rows(const svgir_append_tensor* tensors, int32_t count, int64_t rows_old, const uint32_t* list,
                      const uint32_t* count_dev, int64_t n_sel_max, int32_t repeat, void* stream);
int svgir_split_transform(int64_t n_new, int32_t N, const float* z, float* xyz_new, float* scaling_new, const float* rotation_new,
                          void* stream);

/* Per-stage GPU timing.  While enabled, forward/backward record HIP events on the launch stream at every stage
 * boundary (no extra synchronisation); svgir_last_timings() waits for the recorded events and returns, per stage,
 * the AVERAGE duration in milliseconds and the number of samples since profiling was (re-)enabled.
 * Stage names: "preprocess","sort_depth","emit","sort_tile","ranges","render","image",
 *              "render_bwd","geom_bwd".  Returns the number of entries written (<= cap); `counts` may be NULL. */
void svgir_set_profiling(int enabled);
int svgir_last_timings(const char** names, float* avg_ms, int* counts, int cap);

const char* svgir_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SVGIR_RASTER_H_ */
