"""Drop-in for the reference's `gaussian_renderer.rgss_rasterization` (stage-1 Gaussian-surfel rasterizer).

Same public names, argument order, return tuples and gradient tuples as
/root/reference/gaussian_renderer/rgss_rasterization.py:
  * GaussianRasterizationSettings (16 fields, :189-205)
  * GaussianRasterizer(raster_settings).forward(...) -> 11-tuple (num_rendered, num_contrib[H,W] int32, color,
    normal, opacity, depth, feature, pseudo_normal, surface_xyz, weights, radii) (:224-263, :120)
  * _RasterizeGaussians: grads for (means3D, means2D, features, sh, colors_precomp, opacities, scales, rotations,
    cov3Ds_precomp, None) (:173-184); note the opacity/depth gradient order differs from svgss (Q13)
  * `_C` with the pybind argument order of rgss-rasterization/rasterize_points.h:18-73 (23 args -> 14-tuple,
    27 args -> 9-tuple); `num_contrib` is a non-owning int32 view into the image blob (Q10).
What this module shares with svgss_rasterization.py lives in _binding.py.
"""
from typing import NamedTuple

import torch

from . import _binding as B
from . import _native as N
from ._binding import cpu_deep_copy_tuple  # noqa: F401  (a public name of the reference's module)


class _CBinding:
    """Same three entry points as the reference's pybind module (rgss-rasterization/ext.cpp:15-19)."""

    @staticmethod
    def rasterize_gaussians(*args, **kw):
        """The reference's `_C.rasterize_gaussians` (23 positional arguments, rasterize_points.h:18-43); keyword-only extension:
        `forward_only` (no backward will follow: the composite keeps no blend states)."""
        return N.run_forward(_CBinding._forward_steps(*args, **kw))

    @staticmethod
    def rasterize_gaussians_batch(calls, device, streams):
        """Extension: one svgir_forward_batch for several views (_binding.rasterize_gaussians_batch); returns the list of 14-tuples."""
        return B.rasterize_gaussians_batch(_CBinding._forward_steps, calls, device, streams)

    @staticmethod
    def _forward_steps(background, means3D, features, colors, opacity, scales, rotations, scale_modifier,
                       cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, cx, cy, image_height,
                       image_width, sh, degree, campos, prefiltered, computer_pseudo_normal, debug, *, forward_only=False):
        B.check_forward_inputs("rgss", means3D)  # rasterize_points.cu:62-64
        dev, P, S = means3D.device, means3D.size(0), B.width(features)
        H, W = int(image_height), int(image_width)
        rendered, o, blobs = yield from B.forward_call(
            N.RGSS, dev, P, [("out_color", (3, H, W)), ("out_normal", (3, H, W)), ("out_opacity", (1, H, W)), ("out_depth", (1, H, W)),
                             ("out_feature", (S, H, W)), ("out_pseudo_normal", (3, H, W)), ("out_surface_xyz", (3, H, W))], forward_only,
            S, 0, degree, W, H, scale_modifier, tan_fovx, tan_fovy, debug, background, means3D, sh, colors, features, None,
            scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos,
            opacities=opacity, cx=float(cx), cy=float(cy), prefiltered=int(bool(prefiltered)),
            computer_pseudo_normal=int(bool(computer_pseudo_normal)))
        if P != 0:
            img = blobs.get("image")
            off = N.lib.svgir_image_ncontrib_offset(W, H)
            n_contrib = img[off:off + 4 * H * W].view(torch.int32).view(H, W)  # view into the blob (Q10)
        else:
            n_contrib = torch.zeros((H, W), dtype=torch.int32, device=dev)
        return (rendered, n_contrib, o["out_color"], o["out_normal"], o["out_opacity"], o["out_depth"], o["out_feature"],
                o["out_pseudo_normal"], o["out_surface_xyz"], o["out_weights"], o["radii"], *blobs.take("geom", "binning", "image"))

    @staticmethod
    def rasterize_gaussians_backward(background, means3D, features, radii, colors, scales, rotations, scale_modifier,
                                     cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color,
                                     dL_dout_normal, dL_dout_opacity, dL_dout_depth, dL_dout_feature, sh, degree,
                                     campos, geomBuffer, R, binningBuffer, imageBuffer, backward_geometry, debug, *, out_weights=None):
        """`out_weights` (extension, keyword only): the forward's weights [P,1] (_binding.fill_grads: the per-Gaussian backward then processes the blended surfels only)."""
        dev, P, S, M = means3D.device, means3D.size(0), B.width(features), B.sh_count(sh)
        upstream = dict(dL_dout_color=dL_dout_color, dL_dout_normal=dL_dout_normal, dL_dout_depth=dL_dout_depth,
                        dL_dout_opacity=dL_dout_opacity, dL_dout_feature=dL_dout_feature)
        H, W = B.upstream_size(upstream.values())
        g, gblob = B.carve_gradients(dev, [
            ("dL_dmeans3D", (P, 3)), ("dL_dmeans2D", (P, 3)), ("dL_dfeatures", (P, S)), ("dL_dcolors", (P, 3)), ("dL_dnormal", (P, 3)),
            ("dL_ddepth", (P, 1)), ("dL_dconic", (P, 2, 2)), ("dL_dopacity", (P, 1)), ("dL_dcov3D", (P, 6)), ("dL_dsh", (P, M, 3)),
            ("dL_dscales", (P, 3)), ("dL_drotations", (P, 4))], P)
        if P != 0:
            p, keep = B.call_params(N.RGSS, dev, S, 0, degree, W, H, scale_modifier, tan_fovx, tan_fovy, debug, background, means3D, sh,
                                    colors, features, None, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos,
                                    backward_geometry=int(bool(backward_geometry)))
            gs, gkeep = B.fill_grads(dev, upstream, g, gblob, out_weights)
            # scratch: one packed gradient row per Gaussian (include/svgir_raster.h)
            nscr = N.lib.svgir_backward_scratch_bytes(N.RGSS, P, binningBuffer.numel(), W, H, S, 0)
            B.run_backward(dev, p, gs, R, radii, geomBuffer, binningBuffer, imageBuffer, nscr)
        return (g["dL_dmeans2D"], g["dL_dcolors"], g["dL_dopacity"], g["dL_dmeans3D"], g["dL_dfeatures"], g["dL_dcov3D"], g["dL_dsh"],
                g["dL_dscales"], g["dL_drotations"])

    @staticmethod
    def mark_visible(means3D, viewmatrix, projmatrix):
        return B.mark_visible(N.RGSS, means3D, viewmatrix, projmatrix)


_C = _CBinding()


def rasterize_gaussians(
        means3D,
        means2D,
        features,
        sh,
        colors_precomp,
        opacities,
        scales,
        rotations,
        cov3Ds_precomp,
        raster_settings,
):
    # (every channel width the reference accepts runs through the C ABI: widths without a specialised composite kernel
    #  use the run-time-width kernels of csrc/render_generic.hip)
    return _RasterizeGaussians.apply(
        means3D, means2D, features, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings)


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, features, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings):
        args = (
            raster_settings.bg, means3D, features, colors_precomp, opacities, scales, rotations,
            raster_settings.scale_modifier, cov3Ds_precomp, raster_settings.viewmatrix, raster_settings.projmatrix,
            raster_settings.tanfovx, raster_settings.tanfovy, raster_settings.cx, raster_settings.cy,
            raster_settings.image_height, raster_settings.image_width, sh, raster_settings.sh_degree,
            raster_settings.campos, raster_settings.prefiltered, raster_settings.computer_pseudo_normal,
            raster_settings.debug)
        fwd_only = not any(ctx.needs_input_grad)   # (evaluation / no_grad: the composite keeps no blend states for a backward)
        out = B.forward_with_snapshot(_C.rasterize_gaussians, args, dict(forward_only=fwd_only), raster_settings.debug)
        (num_rendered, num_contrib, color, normal, opacity, depth, feature, pseudo_normal, surface_xyz, weights, radii,
         geomBuffer, binningBuffer, imgBuffer) = out
        ctx.raster_settings = raster_settings
        ctx.num_rendered = num_rendered
        ctx.save_for_backward(colors_precomp, means3D, features, scales, rotations, cov3Ds_precomp, radii, sh,
                              geomBuffer, binningBuffer, imgBuffer, weights)
        ctx.mark_non_differentiable(num_contrib, pseudo_normal, surface_xyz, weights, radii)
        return (num_rendered, num_contrib, color, normal, opacity, depth, feature, pseudo_normal, surface_xyz, weights,
                radii)

    @staticmethod
    def backward(ctx, grad_num_rendered, grad_num_contrib, grad_out_color, grad_out_normal, grad_out_opacity,
                 grad_out_depth, grad_out_feature, grad_out_pseudo_normal, grad_out_surface_xyz, grad_out_weights,
                 grad_out_radii):
        raster_settings = ctx.raster_settings
        (colors_precomp, means3D, features, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, binningBuffer,
         imgBuffer, weights) = ctx.saved_tensors
        up = [B.grad_or_empty(g, means3D.device) for g in (grad_out_color, grad_out_normal, grad_out_opacity, grad_out_depth,
                                                            grad_out_feature)]
        args = (raster_settings.bg, means3D, features, radii, colors_precomp, scales, rotations,
                raster_settings.scale_modifier, cov3Ds_precomp, raster_settings.viewmatrix,
                raster_settings.projmatrix, raster_settings.tanfovx, raster_settings.tanfovy, *up, sh,
                raster_settings.sh_degree, raster_settings.campos, geomBuffer, ctx.num_rendered, binningBuffer, imgBuffer,
                raster_settings.backward_geometry, raster_settings.debug)
        res = B.backward_with_snapshot(_C.rasterize_gaussians_backward, args, dict(out_weights=weights), raster_settings.debug)
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_features, grad_cov3Ds_precomp, grad_sh,
         grad_scales, grad_rotations) = res
        _m = B.grad_if_given
        grads = (
            grad_means3D,
            grad_means2D,
            _m(grad_features, features),
            _m(grad_sh, sh),
            _m(grad_colors_precomp, colors_precomp),
            grad_opacities,
            _m(grad_scales, scales),
            _m(grad_rotations, rotations),
            _m(grad_cov3Ds_precomp, cov3Ds_precomp),
            None,
        )
        return grads


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    cx: float
    cy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    backward_geometry: bool
    computer_pseudo_normal: bool
    debug: bool


class GaussianRasterizer(B.RasterizerBase):
    variant = N.RGSS

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, features=None):
        raster_settings = self.raster_settings
        shs, colors_precomp, scales, rotations, cov3D_precomp, features = B.rasterizer_inputs(
            means3D, shs, colors_precomp, scales, rotations, cov3D_precomp, features)

        return rasterize_gaussians(
            means3D, means2D, features, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
            raster_settings)
