"""L1 and SSIM of a rendered image against the ground truth, fused (csrc/loss.hip): the reference's
`F.l1_loss(image, gt)` + `ssim(image, gt)` (gaussian_renderer/svgss.py:281-289, render.py:150-151;
utils/loss_utils.py:21-64), one kernel forward, one backward; and the radiance-consistency loss of stage 2 (`radiance_loss`: scene/gaussian_model.py:544-575)
around the irradiance kernel of csrc/irradiance.hip, and the same loss fused end to end (`fused_radiance_loss`); and the geometry terms of both stages (`cos_loss`, `surface_loss`, `mask_loss`,
`mask_entropy_loss`, `geometry_losses`: gaussian_renderer/render.py:157-188, svgss.py:297-313, 333-338), fused in csrc/geom_loss.hip; and the
edge-aware smoothness and TV terms (`first_order_edge_aware_loss`, `second_order_edge_aware_loss`, `tv_loss`, `smoothness_losses`:
utils/loss_utils.py:101-117; svgss.py:366-399, render.py:192-196), fused in csrc/smooth_loss.hip; and stage 1's lambda_surface term
(`surface_center_loss`: render.py:217-222) on the exact median of csrc/select.hip."""
import ctypes as C

import torch

from gaussian_renderer import _native as N

N.lib.svgir_l1_ssim_partials.restype = C.c_size_t
N.lib.svgir_l1_ssim_partials.argtypes = [C.c_int32] * 3
N.lib.svgir_l1_ssim_forward.restype = C.c_int
N.lib.svgir_l1_ssim_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
N.lib.svgir_l1_ssim_backward.restype = C.c_int
N.lib.svgir_l1_ssim_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                         C.c_void_p, C.c_void_p, C.c_void_p]

N.lib.svgir_geometry_loss_partials.restype = C.c_size_t
N.lib.svgir_geometry_loss_partials.argtypes = [C.c_int32] * 2
N.lib.svgir_geometry_loss_forward.restype = C.c_int
N.lib.svgir_geometry_loss_forward.argtypes = [C.c_int32] * 3 + [C.c_void_p] * 6 + [C.c_float] * 4 + [C.c_void_p] * 4
N.lib.svgir_geometry_loss_backward.restype = C.c_int
N.lib.svgir_geometry_loss_backward.argtypes = [C.c_int32] * 3 + [C.c_void_p] * 6 + [C.c_float] * 4 + [C.c_void_p] * 6


def _need_maps(dmaps):
    """The forward keeps the derivative maps only when `image` requires grad; a backward without them was asked for the ground truth's
    gradient alone, which the kernels do not compute (the reference's ssim would)."""
    if dmaps is None:
        raise RuntimeError("l1_ssim: only the rendered image is differentiable; the gradient w.r.t. the ground truth is not implemented "
                           "(the image did not require grad in the forward)")


class _L1Ssim(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, gt):
        dev = img.device
        if dev.type != "cuda":
            raise RuntimeError("l1_ssim: tensors must live on the GPU (libsvgir_raster.so has no CPU path)")
        a, b = N.f32c(img, dev), N.f32c(gt, dev)
        Cc, H, W = a.shape[-3], a.shape[-2], a.shape[-1]
        nblk = N.lib.svgir_l1_ssim_partials(Cc, H, W)
        partial = torch.empty((nblk, 2), dtype=torch.float32, device=dev)
        need = img.requires_grad
        dmaps = torch.empty((3, Cc, H, W), dtype=torch.float32, device=dev) if need else None
        means = torch.empty(2, dtype=torch.float32, device=dev)   # {mean SSIM, mean L1}: reduced on the device
        N.check(N.lib.svgir_l1_ssim_forward(a.data_ptr(), b.data_ptr(), Cc, H, W, partial.data_ptr(), N.ptr(dmaps), means.data_ptr(),
                                            N.stream_ptr(dev)), "l1_ssim forward")
        ctx.save_for_backward(a, b, dmaps)
        return means[1], means[0]   # (l1, ssim)

    @staticmethod
    def backward(ctx, g_l1, g_ssim):
        a, b, dmaps = ctx.saved_tensors
        _need_maps(dmaps)
        Cc, H, W = a.shape[-3], a.shape[-2], a.shape[-1]
        out = torch.empty_like(a)
        # the upstream scalars stay on the device: a 2-float buffer {g_ssim, g_l1} the kernel reads (no blocking read-back)
        zero = torch.zeros((), dtype=torch.float32, device=a.device)
        gdev = torch.stack([zero if g_ssim is None else g_ssim.to(torch.float32), zero if g_l1 is None else g_l1.to(torch.float32)])
        N.check(N.lib.svgir_l1_ssim_backward(a.data_ptr(), b.data_ptr(), dmaps.data_ptr(), Cc, H, W, 1.0, 1.0, gdev.data_ptr(),
                                             out.data_ptr(), N.stream_ptr(a.device)), "l1_ssim backward")
        return out, None


def l1_ssim(image, gt):
    """(F.l1_loss(image, gt), ssim(image, gt)) of the reference, [C,H,W] images; differentiable in `image`."""
    return _L1Ssim.apply(image, gt)


class _L1SsimLoss(torch.autograd.Function):
    """(1 - lambda) * L1 + lambda * (1 - SSIM) as ONE autograd node: the reference composes it from the two scalars with four
    elementwise launches forward and as many backward (train.py:133-134 / gaussian_renderer/svgss.py:281-289); here the weights go into
    the backward kernel as its two host scalars and the forward is one dot product of the two device means."""

    @staticmethod
    def forward(ctx, img, gt, lam):
        dev = img.device
        if dev.type != "cuda":
            raise RuntimeError("l1_ssim_loss: tensors must live on the GPU (libsvgir_raster.so has no CPU path)")
        a, b = N.f32c(img, dev), N.f32c(gt, dev)
        Cc, H, W = a.shape[-3], a.shape[-2], a.shape[-1]
        nblk = N.lib.svgir_l1_ssim_partials(Cc, H, W)
        partial = torch.empty((nblk, 2), dtype=torch.float32, device=dev)
        need = img.requires_grad
        dmaps = torch.empty((3, Cc, H, W), dtype=torch.float32, device=dev) if need else None
        means = torch.empty(2, dtype=torch.float32, device=dev)   # {mean SSIM, mean L1}
        N.check(N.lib.svgir_l1_ssim_forward(a.data_ptr(), b.data_ptr(), Cc, H, W, partial.data_ptr(), N.ptr(dmaps), means.data_ptr(),
                                            N.stream_ptr(dev)), "l1_ssim forward")
        ctx.save_for_backward(a, b, dmaps)
        ctx.lam = float(lam)
        w = _weights(dev, ctx.lam)   # [-lambda, 1 - lambda, lambda]
        return torch.dot(means, w[:2]) + w[2]

    @staticmethod
    def backward(ctx, g):
        a, b, dmaps = ctx.saved_tensors
        _need_maps(dmaps)
        Cc, H, W = a.shape[-3], a.shape[-2], a.shape[-1]
        out = torch.empty_like(a)
        gdev = g.to(torch.float32).reshape(1).expand(2).contiguous()   # the upstream scalar stays on the device
        N.check(N.lib.svgir_l1_ssim_backward(a.data_ptr(), b.data_ptr(), dmaps.data_ptr(), Cc, H, W, -ctx.lam, 1.0 - ctx.lam,
                                             gdev.data_ptr(), out.data_ptr(), N.stream_ptr(a.device)), "l1_ssim backward")
        return out, None, None


_W = {}


def _weights(dev, lam):
    key = (dev.index, lam)
    if key not in _W:
        _W[key] = torch.tensor([-lam, 1.0 - lam, lam], dtype=torch.float32, device=dev)
    return _W[key]


def l1_ssim_loss(image, gt, lambda_dssim=0.2):
    """(1 - lambda_dssim) * F.l1_loss(image, gt) + lambda_dssim * (1 - ssim(image, gt)) -- the reference's photometric loss
    (train.py:133-134; arguments/__init__.py: lambda_dssim = 0.2) -- as one autograd node; differentiable in `image`."""
    return _L1SsimLoss.apply(image, gt, float(lambda_dssim))


def ssim(img1, img2, window_size=11, size_average=True):
    """Drop-in for utils/loss_utils.py:33 (window 11, size_average=True -- the only form the reference calls)."""
    if window_size != 11 or not size_average:
        raise NotImplementedError("only the reference's call form ssim(img1, img2) is implemented")
    return l1_ssim(img1, img2)[1]


def radiance_loss(renderer, xyz, camera_center, geo_normal, incident_dirs, visibility, envmap, normals12, albedos, roughnesses, radiances,
                  radiance_ratio):
    """`GaussianModel.get_radiance_loss` (scene/gaussian_model.py:544-575) on explicit tensors: the view direction of every surfel
    (xyz [N,3] - camera_center [3]) is reflected about its geometric normal, the incident sample that looks most along the reflection
    and is occluded -- the largest (incident_dir . reflection) * (1 - visibility), the first index on ties -- is chosen, the irradiance
    its first hit reflects back is evaluated by `renderer.render_irradiance_sample` (a pbgi.Renderer whose hemi_index_buffers /
    uv_buffers are set) under `envmap` [N,S,3], and the L1 distance to the cached radiance of that sample,
    nan_to_num(radiances.detach() * radiance_ratio) [N,S,3], is returned.  incident_dirs [N,S,3], visibility [N,S,1] or [N,S],
    normals12 / albedos [N,12], roughnesses [N,4].  The selection and the L1 are plain torch ([N,S] work); gradients reach envmap,
    albedos and roughnesses through the kernel's backward and radiance_ratio through autograd."""
    N, S = int(incident_dirs.shape[0]), int(incident_dirs.shape[1])
    view_dirs = torch.nn.functional.normalize(xyz - camera_center, dim=-1)
    view_reflect = 2 * torch.sum(geo_normal * view_dirs, dim=-1, keepdim=True) * geo_normal + view_dirs
    n_d_i = torch.sum(incident_dirs * view_reflect[:, None], dim=-1) * (1 - visibility.reshape(N, S))
    max_idx = torch.argmax(n_d_i.detach(), dim=-1).unsqueeze(-1).int()
    radiance = renderer.render_irradiance_sample(N, S, max_idx, envmap, incident_dirs, None, None, None, normals12, albedos, roughnesses,
                                                 None, None, None)
    target = torch.nan_to_num(radiances.detach() * radiance_ratio, nan=0.0)
    target = target.gather(1, max_idx.long().unsqueeze(-1).expand(-1, -1, 3)).squeeze(-2)
    return torch.nn.functional.l1_loss(radiance, target)


def fused_radiance_loss(renderer, xyz, camera_center, geo_normal, incident_dirs, incident_areas, visibility, light, normals12, albedos,
                        roughnesses, radiances, radiance_ratio, with_rows=False):
    """`GaussianModel.get_radiance_loss` (scene/gaussian_model.py:544-575) as one fused forward and one fused backward
    (`Renderer.radiance_consistency`, csrc/irradiance.hip): what `radiance_loss` computes when it is fed
    envmap = light.direct_light(incident_dirs) * incident_areas, without that [N,S,3] tensor, its gradient, or any [N,S] temporary of the
    selection.  `light` is the reference's DirectLightMap (.env) or EnvLight (.envmap [, .transform]), as for the shading
    (gaussian_renderer.shading._env_of); visibility and incident_areas are [N,S,1] or [N,S].  Gradients reach light.env (when it requires
    grad), albedos, roughnesses and radiance_ratio.  with_rows=True returns (loss, sample_indices [N] int32, radiance [N,3]).
    A row whose radiance or target is not finite makes the loss NaN, as in torch, but contributes to no gradient
    (include/svgir_raster.h)."""
    from gaussian_renderer import shading
    # (an SG light: fused_radiance_loss_sg -- or radiance_loss with envmap = sg_direct_light(lgtSGs, dirs) * areas, which carries the
    # light's gradient through svgir_sg_eval_backward)
    shading._no_sg(light, "fused_radiance_loss")
    env, softplus, scale, transform = shading._env_of(light)
    out = renderer.radiance_consistency(xyz, camera_center, geo_normal, incident_dirs, incident_areas, visibility, env, softplus, scale,
                                        transform, normals12, albedos, roughnesses, radiances, radiance_ratio)
    return out if with_rows else out[0]


def fused_radiance_loss_sg(renderer, xyz, camera_center, geo_normal, incident_dirs, incident_areas, visibility, light, normals12, albedos,
                           roughnesses, radiances, radiance_ratio, with_rows=False):
    """fused_radiance_loss for the reference's DirectLightSG (`light.lgtSGs` [M,7]; `Renderer.radiance_consistency_sg`): what
    `radiance_loss` computes when it is fed envmap = sg_direct_light(light.lgtSGs, incident_dirs) * incident_areas, without that [N,S,3]
    tensor or its gradient.  Gradients reach light.lgtSGs (when it requires grad), albedos, roughnesses and radiance_ratio; the return
    value and the non-finite rule are fused_radiance_loss's."""
    from gaussian_renderer import shading
    if not shading._is_sg(light):
        raise TypeError("fused_radiance_loss_sg: the light must expose .lgtSGs (DirectLightSG); a texture light goes through fused_radiance_loss")
    out = renderer.radiance_consistency_sg(xyz, camera_center, geo_normal, incident_dirs, incident_areas, visibility, light.lgtSGs, normals12,
                                           albedos, roughnesses, radiances, radiance_ratio)
    return out if with_rows else out[0]


# ---- geometry terms (csrc/geom_loss.hip) ------------------------------------------------------------------------------------------
GEOMETRY_TERMS = ("surface", "target", "mask", "entropy")   # bit k of the kernels' `terms`; the order of their stats / losses buffers


def _plane(t, channels, H, W, name):
    """[channels,H,W] view of a plane given as [channels,H,W] (or [H,W] for one channel)."""
    if t is None:
        return None
    if channels == 1 and t.dim() == 2:
        t = t[None]
    if tuple(t.shape) != (channels, H, W):
        raise ValueError(f"geometry_losses: {name} must be [{channels},{H},{W}], got {tuple(t.shape)}")
    return t


class _GeometryLoss(torch.autograd.Function):
    """The requested terms as ONE node: one forward launch (+ its reduction), one backward launch.  Returns the [4] vector of losses in
    GEOMETRY_TERMS order (zeros for the terms not requested) and the kernels' stats [4][2] = {sum, count} per term (doubles); the gradient of the
    loss vector is the kernels' upstream buffer as it is."""

    @staticmethod
    def forward(ctx, terms, cam, normal, depth, opacity, mask, target, weight):
        ref = normal if normal is not None else opacity
        dev = ref.device
        for t in (normal, depth, opacity, mask, target, weight):
            if t is not None and t.device.type != "cuda":
                raise RuntimeError("geometry_losses: tensors must live on the GPU (libsvgir_raster.so has no CPU path)")
        H, W = int(ref.shape[-2]), int(ref.shape[-1])
        shapes = tuple(None if t is None else tuple(t.shape) for t in (normal, depth, opacity))
        planes = [N.f32c(_plane(None if t is None else t.detach(), c, H, W, n), dev)
                  for t, c, n in ((normal, 3, "normal"), (depth, 1, "depth"), (mask, 1, "mask"), (opacity, 1, "opacity"), (target, 3, "target"),
                                  (weight, 1, "weight"))]
        with torch.cuda.device(dev):
            partial = torch.empty((max(N.lib.svgir_geometry_loss_partials(W, H), 1), 8), dtype=torch.float64, device=dev)
            stats = N.out_tensor((4, 2), torch.float64, dev)
            losses = N.out_tensor((4,), torch.float32, dev)
            N.check(N.lib.svgir_geometry_loss_forward(W, H, terms, *[N.ptr(p) for p in planes], *cam, partial.data_ptr(), stats.data_ptr(),
                                                      losses.data_ptr(), N.stream_ptr(dev)), "geometry_loss forward")
        ctx.save_for_backward(stats, *planes)
        ctx.terms, ctx.cam, ctx.shapes, ctx.size = terms, cam, shapes, (H, W)
        ctx.mark_non_differentiable(stats)
        return losses, stats

    @staticmethod
    def backward(ctx, g, _g_stats):
        stats, *planes = ctx.saved_tensors
        H, W = ctx.size
        dev = stats.device
        need = ctx.needs_input_grad[2:5]   # normal, depth, opacity
        outs = [N.out_tensor((c, H, W), torch.float32, dev) if n else None for n, c in zip(need, (3, 1, 1))]
        if any(need):
            gdev = g.to(torch.float32).contiguous()   # the four upstream scalars stay on the device
            with torch.cuda.device(dev):
                N.check(N.lib.svgir_geometry_loss_backward(W, H, ctx.terms, *[N.ptr(p) for p in planes], *ctx.cam, stats.data_ptr(),
                                                           gdev.data_ptr(), *[N.ptr(o) for o in outs], N.stream_ptr(dev)),
                        "geometry_loss backward")
        grads = [None if o is None else o.reshape(sh) for o, sh in zip(outs, ctx.shapes)]
        return (None, None, grads[0], grads[1], grads[2], None, None, None)


def geometry_losses(normal=None, depth=None, mask=None, opacity=None, target=None, weight=None, fovx=None, fovy=None, prcppoint=(0.5, 0.5),
                    terms=None, with_stats=False):
    """The geometry terms of `calculate_loss` (gaussian_renderer/render.py:157-188, svgss.py:297-313, 333-338) from ONE forward launch and
    one autograd node: a dict with
      "surface": cos_loss(normal, depth2normal(depth, mask, camera))   -- normal [3,H,W], depth, mask [1,H,W], fovx, fovy, prcppoint
      "target" : cos_loss(normal, target, weight=weight)                -- target [3,H,W], weight [1,H,W] / [H,W] or None (= 1)
      "mask"   : (opacity * (1 - MaxPool2d(9, 1, 4)(mask))).mean()      -- opacity, mask [1,H,W]
      "entropy": -(mask * log(o) + (1 - mask) * log(1 - o)).mean(), o = opacity.clamp(1e-6, 1 - 1e-6)
    `terms`: the names wanted; None = every term whose inputs are given.  with_stats=True adds "stats": the device tensor [4,2] (float64) of {sum,
    count} per term in GEOMETRY_TERMS order (the count of a cos_loss is its number of selected pixels; a loss is float32(sum / count)).  Differentiable in normal, depth and opacity; the mask, the target
    and the weight get no gradient (a target that requires grad is refused)."""
    have = {"surface": normal is not None and depth is not None and mask is not None and fovx is not None and fovy is not None,
            "target": normal is not None and target is not None,
            "mask": opacity is not None and mask is not None, "entropy": opacity is not None and mask is not None}
    names = tuple(k for k in GEOMETRY_TERMS if have[k]) if terms is None else tuple(terms)
    if not names:
        raise ValueError("geometry_losses: no term requested (give the planes of at least one term)")
    for k in names:
        if k not in GEOMETRY_TERMS:
            raise ValueError(f"geometry_losses: unknown term {k!r}")
        if not have[k]:
            raise ValueError(f"geometry_losses: the {k} term was requested without its planes")
    for t, n in ((target, "target"), (weight, "weight"), (mask, "mask")):
        if t is not None and t.requires_grad:
            raise RuntimeError(f"geometry_losses: the {n} gets no gradient (detach it); the fused surface term differentiates through the "
                               "pseudo normal")
    bits = sum(1 << GEOMETRY_TERMS.index(k) for k in set(names))
    surface = "surface" in names
    cam = (float(fovx), float(fovy), float(prcppoint[0]), float(prcppoint[1])) if surface else (1.0, 1.0, 0.5, 0.5)
    cos = surface or "target" in names
    opac = "mask" in names or "entropy" in names
    out, stats = _GeometryLoss.apply(bits, cam, normal if cos else None, depth if surface else None, opacity if opac else None,
                              mask if surface or opac else None, target if "target" in names else None,
                              weight if "target" in names else None)
    res = {k: out[GEOMETRY_TERMS.index(k)] for k in GEOMETRY_TERMS if k in names}
    if with_stats:
        res["stats"] = stats
    return res


def cos_loss(output, gt, thrsh=0, weight=1):
    """Drop-in for utils/loss_utils.py:119: cos = sum_c output_c * gt_c * weight, mean of 1 - cos over the pixels with cos < 1.
    `thrsh` must be 0 (the only form the reference calls); `weight` is 1 or a [1,H,W] / [H,W] plane.  Differentiable in `output` only:
    for the pseudo normal of the rendered depth use `surface_loss`, which differentiates through it."""
    if thrsh != 0:
        raise NotImplementedError("cos_loss: only thrsh = 0 is implemented (the reference's call form)")
    if not torch.is_tensor(weight):
        if weight != 1:
            raise NotImplementedError("cos_loss: weight is 1 or a [1,H,W] / [H,W] plane")
        weight = None
    if gt.requires_grad:
        raise RuntimeError("cos_loss: only `output` is differentiable; for gt = depth2normal(depth, ...) use surface_loss")
    return geometry_losses(normal=output, target=gt, weight=weight, terms=("target",))["target"]


def surface_loss(normal, depth, mask, fovx, fovy, prcppoint=(0.5, 0.5)):
    """cos_loss(normal, depth2normal(depth, mask, camera)) fused (render.py:158-160, svgss.py:299-301): the pseudo normal is never
    stored.  Differentiable in `normal` and `depth`."""
    return geometry_losses(normal=normal, depth=depth, mask=mask, fovx=fovx, fovy=fovy, prcppoint=prcppoint, terms=("surface",))["surface"]


def mask_loss(opacity, mask):
    """(opacity * (1 - MaxPool2d(9, stride=1, padding=4)(mask))).mean() (render.py:157-159).  Differentiable in `opacity`."""
    return geometry_losses(opacity=opacity, mask=mask, terms=("mask",))["mask"]


def mask_entropy_loss(opacity, mask):
    """-(mask * log(o) + (1 - mask) * log(1 - o)).mean() with o = opacity.clamp(1e-6, 1 - 1e-6) (render.py:184-186, svgss.py:333-336).
    Differentiable in `opacity`."""
    return geometry_losses(opacity=opacity, mask=mask, terms=("entropy",))["entropy"]


# ---- lambda_surface (csrc/select.hip) -----------------------------------------------------------------------------------------------
SURFACE_CENTER_STATS = 11   # sum, 3 P, then {index, n_less, n_greater} per column


class _SurfaceCenterLoss(torch.autograd.Function):
    """exp(-mean |xyz - median(xyz, dim=0)|) as ONE node: the selection and one fixed-order reduction forward, one elementwise launch
    backward.  Returns the loss (a 0-d fp32 device tensor) and the kernels' stats [11] (doubles)."""

    @staticmethod
    def forward(ctx, xyz):
        dev = xyz.device
        if dev.type != "cuda":
            raise RuntimeError("surface_center_loss: tensors must live on the GPU (libsvgir_raster.so has no CPU path)")
        if xyz.dim() != 2 or xyz.shape[1] != 3:
            raise ValueError(f"surface_center_loss: xyz must be [P,3], got {tuple(xyz.shape)}")
        x = N.f32c(xyz.detach(), dev)
        P = int(x.shape[0])
        with torch.cuda.device(dev):
            partial = N.out_tensor((max(N.lib.svgir_surface_center_loss_partials(P), 1),), torch.float64, dev)
            stats = N.out_tensor((SURFACE_CENTER_STATS,), torch.float64, dev)
            loss = N.out_tensor((1,), torch.float32, dev)
            N.check(N.lib.svgir_surface_center_loss_forward(P, N.ptr(x), partial.data_ptr(), stats.data_ptr(), loss.data_ptr(),
                                                            N.stream_ptr(dev)), "surface_center_loss forward")
        ctx.save_for_backward(x, stats)
        ctx.shape = tuple(xyz.shape)
        ctx.mark_non_differentiable(stats)
        return loss[0], stats

    @staticmethod
    def backward(ctx, g, _g_stats):
        x, stats = ctx.saved_tensors
        dev = x.device
        P = int(x.shape[0])
        out = N.out_tensor((P, 3), torch.float32, dev)
        if P:
            gdev = g.to(torch.float32).reshape(1).contiguous()   # the upstream scalar stays on the device
            with torch.cuda.device(dev):
                N.check(N.lib.svgir_surface_center_loss_backward(P, x.data_ptr(), stats.data_ptr(), gdev.data_ptr(), out.data_ptr(),
                                                                 N.stream_ptr(dev)), "surface_center_loss backward")
        return out.reshape(ctx.shape)


def surface_center_loss(xyz, with_stats=False):
    """Stage 1's lambda_surface term (gaussian_renderer/render.py:217-222): torch.exp(-(xyz - torch.median(xyz, dim=0)[0][None]).abs().mean())
    for xyz [P,3], on the exact median of csrc/select.hip (`metrics.column_median`: its rules for ties, zeros and NaN).  Differentiable in
    xyz: every element gets -L sign(x - c) / (3 P), and the median's own row of each column the gradient of `center` on top, as torch's
    median hands it to the row it returned.  A NaN coordinate makes the loss and every gradient NaN, as in torch; P == 0 gives NaN.
    with_stats=True returns (loss, stats), stats the device tensor [11] (float64) {sum, 3 P, then index, n_less, n_greater per column}.
    (`surface_loss` above is the cos term of render.py:158-160; the two share only the reference's word "surface".)"""
    loss, stats = _SurfaceCenterLoss.apply(xyz)
    return (loss, stats) if with_stats else loss


# ---- edge-aware smoothness and TV terms (csrc/smooth_loss.hip) ------------------------------------------------------------------------
SMOOTH_KINDS = {"first": 1, "second": 2, "tv": 3}   # svgir_smooth_term.kind
SMOOTH_MAX_TERMS = 4                                 # SVGIR_SMOOTH_MAX_TERMS


def _descriptors(kinds, planes, grads=None):
    """(svgir_smooth_term * n) over the planes [(data, img, data_mask, img_mask)]; grads [(d_data, d_img)] for the backward."""
    arr = (N.SmoothTerm * len(kinds))()
    for k, (kind, (data, img, dm, im)) in enumerate(zip(kinds, planes)):
        t = arr[k]
        t.kind, t.C, t.Ci = kind, int(data.shape[0]), 0 if img is None else int(img.shape[0])
        t.data, t.img, t.data_mask, t.img_mask = (None if p is None else p.data_ptr() for p in (data, img, dm, im))
        if grads is not None:
            t.d_data, t.d_img = (None if g is None else g.data_ptr() for g in grads[k])
    return arr


class _SmoothLoss(torch.autograd.Function):
    """Up to SMOOTH_MAX_TERMS terms of one image size as ONE node: one forward launch (+ its reduction), one backward launch.  `tensors` =
    (data, img, data_mask, img_mask) per term, None where a term has none.  Returns the [n] vector of losses and the kernels' stats [n,4] =
    {sum_a, count_a, sum_b, count_b} per term (doubles); the gradient of the loss vector is the kernels' upstream buffer as it is."""

    @staticmethod
    def forward(ctx, kinds, *tensors):
        n = len(kinds)
        dev = tensors[0].device
        for t in tensors:
            if t is not None and t.device.type != "cuda":
                raise RuntimeError("smoothness_losses: tensors must live on the GPU (libsvgir_raster.so has no CPU path)")
        H, W = int(tensors[0].shape[-2]), int(tensors[0].shape[-1])
        flat = [None if t is None else N.f32c(t.detach(), dev) for t in tensors]
        planes = [tuple(flat[4 * k:4 * k + 4]) for k in range(n)]
        with torch.cuda.device(dev):
            partial = torch.empty((max(N.lib.svgir_smooth_loss_partials(W, H, n), 1), 2), dtype=torch.float64, device=dev)
            stats = N.out_tensor((n, 4), torch.float64, dev)
            losses = N.out_tensor((n,), torch.float32, dev)
            N.check(N.lib.svgir_smooth_loss_forward(W, H, n, _descriptors(kinds, planes), partial.data_ptr(), stats.data_ptr(), losses.data_ptr(),
                                                    N.stream_ptr(dev)), "smooth_loss forward")
        ctx.save_for_backward(stats, *[p for p in flat if p is not None])
        ctx.kinds, ctx.present, ctx.size = kinds, tuple(p is not None for p in flat), (H, W)
        ctx.mark_non_differentiable(stats)
        return losses, stats

    @staticmethod
    def backward(ctx, g, _g_stats):
        stats, *saved = ctx.saved_tensors
        it = iter(saved)
        flat = [next(it) if here else None for here in ctx.present]
        n = len(ctx.kinds)
        planes = [tuple(flat[4 * k:4 * k + 4]) for k in range(n)]
        dev = stats.device
        need = ctx.needs_input_grad[1:]
        grads = [tuple(N.out_tensor(tuple(planes[k][j].shape), torch.float32, dev) if need[4 * k + j] else None for j in (0, 1)) for k in range(n)]
        if any(o is not None for pair in grads for o in pair):
            gdev = g.to(torch.float32).contiguous()   # the upstream scalars stay on the device
            with torch.cuda.device(dev):
                N.check(N.lib.svgir_smooth_loss_backward(ctx.size[1], ctx.size[0], n, _descriptors(ctx.kinds, planes, grads), stats.data_ptr(),
                                                         gdev.data_ptr(), N.stream_ptr(dev)), "smooth_loss backward")
        out = [None]
        for pair in grads:
            out += [pair[0], pair[1], None, None]
        return tuple(out)


def _smooth_plane(t, name, k, H=None, W=None, one=False):
    if t is None:
        return None
    if not torch.is_tensor(t) or t.dim() != 3 or not 1 <= t.shape[0] <= 4 or (one and t.shape[0] != 1):
        raise ValueError(f"smoothness_losses: term {k}: {name} must be a " + ("[1,H,W]" if one else "[C,H,W] (C = 1 ... 4)") + " tensor, got "
                         + (str(tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
    if H is not None and (int(t.shape[1]), int(t.shape[2])) != (H, W):
        raise ValueError(f"smoothness_losses: term {k}: {name} is {tuple(t.shape)}; every plane of a launch must be [.,{H},{W}]")
    return t


def smoothness_losses(terms, with_stats=False):
    """The smoothness terms of `calculate_loss` (gaussian_renderer/svgss.py:366-399, render.py:192-196) from ONE forward launch and one
    autograd node.  `terms`: a list of up to 4 dicts {kind, data, img=None, data_mask=None, img_mask=None} over one image size,
      kind "first" : first_order_edge_aware_loss(data * data_mask, img * img_mask)     -- data [C,H,W], img [Ci,H,W], C == Ci or one is 1
      kind "second": second_order_edge_aware_loss(data * data_mask, img * img_mask)
      kind "tv"    : tv_loss(data)                                                     -- data [C,H,W]; no img, no masks
    (utils/loss_utils.py:101-117; a kind may also be given as 1, 2, 3).  The masks are [1,H,W] planes or None (= 1): the kernels form the
    fp32 product the reference forms, and multiply the outgoing gradient by the mask.  Returns the [n] vector of losses in the order of
    `terms`; with_stats=True returns (losses, stats), stats the device tensor [n,4] (float64) of {sum_a, count_a, sum_b, count_b} per term
    (a loss is float32(sum_a / count_a), tv float32(sum_a / count_a + sum_b / count_b)).  Differentiable in every `data` and in every `img`
    that requires grad; masks get no gradient (one that requires grad is refused)."""
    terms = list(terms)
    if not 1 <= len(terms) <= SMOOTH_MAX_TERMS:
        raise ValueError(f"smoothness_losses: 1 ... {SMOOTH_MAX_TERMS} terms per launch, got {len(terms)}")
    kinds, flat = [], []
    H = W = None
    for k, t in enumerate(terms):
        unknown = set(t) - {"kind", "data", "img", "data_mask", "img_mask"}
        if unknown:
            raise ValueError(f"smoothness_losses: term {k}: unknown keys {sorted(unknown)}")
        kind = SMOOTH_KINDS.get(t.get("kind"), t.get("kind"))
        if kind not in (1, 2, 3):
            raise ValueError(f"smoothness_losses: term {k}: unknown kind {t.get('kind')!r} (first, second, tv)")
        data = _smooth_plane(t.get("data"), "data", k, H, W)
        if data is None:
            raise ValueError(f"smoothness_losses: term {k} has no data")
        H, W = int(data.shape[1]), int(data.shape[2])
        img, dm, im = (_smooth_plane(t.get(nm), nm, k, H, W, one) for nm, one in (("img", False), ("data_mask", True), ("img_mask", True)))
        if kind == 3:
            if img is not None or dm is not None or im is not None:
                raise ValueError(f"smoothness_losses: term {k}: a tv term takes data only")
        else:
            if img is None:
                raise ValueError(f"smoothness_losses: term {k} has no img")
            if data.shape[0] != img.shape[0] and data.shape[0] != 1 and img.shape[0] != 1:
                raise ValueError(f"smoothness_losses: term {k}: cannot broadcast data {tuple(data.shape)} against img {tuple(img.shape)}")
        for m, nm in ((dm, "data_mask"), (im, "img_mask")):
            if m is not None and m.requires_grad:
                raise RuntimeError(f"smoothness_losses: term {k}: the {nm} gets no gradient (detach it)")
        kinds.append(kind)
        flat += [data, img, dm, im]
    losses, stats = _SmoothLoss.apply(tuple(kinds), *flat)
    return (losses, stats) if with_stats else losses


def first_order_edge_aware_loss(data, img):
    """Drop-in for utils/loss_utils.py:104: (|d data| * exp(-|d img|)).sum(1).mean() over kornia's normalized Sobel derivatives, data
    [C,H,W], img [Ci,H,W].  Differentiable in `data`, and in `img` when it requires grad.  A caller that multiplies by a mask first can
    hand the mask to `smoothness_losses` instead and save the product."""
    return smoothness_losses([dict(kind="first", data=data, img=img)])[0]


def second_order_edge_aware_loss(data, img):
    """Drop-in for utils/loss_utils.py:101: (|d2 data| * exp(-10 |d img|)).sum(1).mean(), the xx / yy second derivatives of `data` weighted
    by the x / y first derivatives of `img`."""
    return smoothness_losses([dict(kind="second", data=data, img=img)])[0]


def tv_loss(x):
    """Drop-in for utils/loss_utils.py:113: mean of the squared row differences + mean of the squared column differences, x [C,H,W] or
    [H,W].  H == 1 or W == 1: NaN (the empty mean, as in torch) and zero gradient."""
    return smoothness_losses([dict(kind="tv", data=x[None] if x.dim() == 2 else x)])[0]
