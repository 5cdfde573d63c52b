"""Drop-in for the reference's `gaussian_renderer.svgss_rasterization` (stage-2, spatially-varying surfels).

Same public names, argument order, return tuples and gradient tuples as
/root/reference/gaussian_renderer/svgss_rasterization.py:
  * GaussianRasterizationSettings (15 fields, :331-346)
  * GaussianRasterizer(raster_settings).forward(...) -> 9-tuple (:365-411, :183); .markVisible (:354-363)
  * _RasterizeGaussians autograd.Function: grads for (means3D, means2D, features, vfeatures, sh, colors_precomp,
    opacities, scales, rotations, cov3Ds_precomp, viewmatrix, projmatrix, campos, None) (:293-308)
  * `_C` with rasterize_gaussians / rasterize_gaussians_backward / mark_visible in the pybind argument order of
    svgss_rasterization/rasterize_points.h:18-82 (24 args -> 12-tuple, 31 args -> 13-tuple).
The compute runs in libsvgir_raster.so (hand-written HIP for gfx950) through the C ABI of include/svgir_raster.h; what this
module shares with rgss_rasterization.py lives in _binding.py.
"""
from typing import NamedTuple

import ctypes as C

import torch

from . import _binding as B
from . import _native as N
from ._binding import cpu_deep_copy_tuple  # noqa: F401  (a public name of the reference's module)


def _svgss_fields(prcppoint, patchbbox, config):
    """The svgir_params fields only this variant sets, forward and backward (_binding.call_params)."""
    return dict(prcppoint=prcppoint, patchbbox=patchbbox, config=config, config_len=config.numel() if config is not None else 0)


class _CBinding:
    """Same three entry points as the reference's pybind module (svgss_rasterization/ext.cpp:15-19)."""

    @staticmethod
    def rasterize_gaussians(*args, **kw):
        """The reference's `_C.rasterize_gaussians` (24 positional arguments, rasterize_points.h:18-46); keyword-only extensions:
        `features_ready`, `shade`, `forward_only` (see `_forward_steps`), and `sg_light`: a `_native.SgLight`, the spherical-Gaussian
        light of the fused shading (needs `shade`) -- the call is then svgir_forward_sg.  (rasterize_gaussians_batch has no such
        argument: svgir_view_call has no room for a light.)"""
        sg_light = kw.pop("sg_light", None)
        if sg_light is not None and kw.get("shade") is None:
            raise ValueError("rasterize_gaussians: sg_light belongs to the fused shading (pass `shade`)")
        return N.run_forward(_CBinding._forward_steps(*args, **kw), sg_light)

    @staticmethod
    def rasterize_gaussians_batch(calls, device, streams):
        """Extension: one svgir_forward_batch for several views (_binding.rasterize_gaussians_batch); returns the list of 12-tuples."""
        return B.rasterize_gaussians_batch(_CBinding._forward_steps, calls, device, streams)

    @staticmethod
    def _forward_steps(background, means3D, features, vfeatures, colors, opacity, scales, rotations,
                       scale_modifier, cov3D_precomp, viewmatrix, projmatrix, prcppoint, patchbbox, tan_fovx,
                       tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug, config, *,
                       features_ready=None, shade=None, forward_only=False):
        """`features_ready` (extension, keyword only): a torch.cuda.Event recorded on the stream that is still producing
        `features` / `vfeatures` (the shading kernels on a side stream); only the composite kernel waits for it, so the
        shading of a view overlaps its binning.  The caller keeps the tensors alive across streams (`record_stream`).
        `shade` (extension, keyword only): a `_native.FusedShade` -- the library shades the surfels this view's composite reads
        and WRITES `features` / `vfeatures` (pass uninitialised [P,S] / [P,VS] buffers; gaussian_renderer/shading.py).
        `forward_only` (extension, keyword only): no backward will follow -- the composite keeps no blend states."""
        B.check_forward_inputs("svgss", means3D)  # rasterize_points.cu:65-67
        dev, P, S, VS = means3D.device, means3D.size(0), B.width(features), B.width(vfeatures)
        H, W = int(image_height), int(image_width)
        more = dict(_svgss_fields(prcppoint, patchbbox, config), opacities=opacity, cx=W / 2.0, cy=H / 2.0,
                    prefiltered=int(bool(prefiltered)))
        if features_ready is not None:   # (a struct field of this call: nothing survives if anything below raises)
            more["features_ready"] = features_ready.cuda_event
        if shade is not None:
            more["shade"] = C.addressof(shade)
        rendered, o, blobs = yield from B.forward_call(
            N.SVGSS, dev, P, [("out_color", (3, H, W)), ("out_normal", (3, H, W)), ("out_depth", (1, H, W)), ("out_opacity", (1, H, W)),
                              ("out_feature", (S, H, W)), ("out_vfeature", (VS // 4, H, W))], forward_only,
            S, VS, degree, W, H, scale_modifier, tan_fovx, tan_fovy, debug, background, means3D, sh, colors, features, vfeatures,
            scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, **more)
        # note: C++ order is (..., depth, opac, ...) -- the Python wrapper re-orders (svgss_rasterization.py:175,183)
        return (rendered, o["out_color"], o["out_normal"], o["out_depth"], o["out_opacity"], o["out_feature"], o["out_vfeature"],
                o["out_weights"], o["radii"], *blobs.take("geom", "binning", "image"))

    @staticmethod
    def rasterize_gaussians_backward(background, means3D, features, vfeatures, radii, colors, scales, rotations,
                                     scale_modifier, cov3D_precomp, viewmatrix, projmatrix, prcppoint, patchbbox,
                                     tan_fovx, tan_fovy, dL_dout_color, dL_dout_normal, dL_dout_depth, dL_dout_opac,
                                     dL_dout_feature, dL_dout_vfeature, sh, degree, campos, geomBuffer, R,
                                     binningBuffer, imageBuffer, debug, config, *, shade=None, shade_grads=None, out_weights=None,
                                     scratch_feature_grads=False, sg_light=None):
        """`shade` / `shade_grads` (extension, keyword only): the `_native.FusedShade` of the forward and a dict of the shading's
        gradient outputs + `out_weights` (+ optional `dL_dreduced`), written by svgir_backward (gaussian_renderer/shading.py;
        its "_shapes" entry: _binding.carve_gradients).
        `out_weights` (extension, keyword only): the forward's weights [P,1] (_binding.fill_grads).
        `scratch_feature_grads` (with `shade`): dL_dfeatures / dL_dvfeatures are intermediates of the fused call -- written for the blended
        surfels, read back by the shading's backward for exactly those -- so they need no zero rows: they are taken out of the cleared
        allocation (45 MB less to clear at P = 200 k); the rows of unblended surfels in the two returned tensors are then UNDEFINED.
        `sg_light` (with `shade`): the `_native.SgLight` of the forward -- the call is svgir_backward_sg, shade_grads["dL_denv"] is
        dL_dlobes [M,7] and shade_grads["env_grad_work"] holds svgir_sg_grad_work_bytes(M) bytes."""
        if sg_light is not None and shade is None:
            raise ValueError("rasterize_gaussians_backward: sg_light belongs to the fused shading (pass `shade`)")
        dev, P, S, VS, M = means3D.device, means3D.size(0), B.width(features), B.width(vfeatures), B.sh_count(sh)
        upstream = dict(dL_dout_color=dL_dout_color, dL_dout_normal=dL_dout_normal, dL_dout_depth=dL_dout_depth,
                        dL_dout_opacity=dL_dout_opac, dL_dout_feature=dL_dout_feature, dL_dout_vfeature=dL_dout_vfeature)
        H, W = B.upstream_size(upstream.values())
        scratch_fg = bool(scratch_feature_grads) and shade is not None and P != 0
        g, gblob = B.carve_gradients(dev, [
            ("dL_dmeans3D", (P, 3)), ("dL_dmeans2D", (P, 3)), ("dL_dfeatures", (0 if scratch_fg else P, S)),
            ("dL_dvfeatures", (0 if scratch_fg else P, VS)), ("dL_dcolors", (P, 3)), ("dL_dnormal", (P, 3)), ("dL_ddepth", (P, 1)),
            ("dL_dconic", (P, 2, 2)), ("dL_dopacity", (P, 1)), ("dL_dcov3D", (P, 6)), ("dL_dsh", (P, M, 3)), ("dL_dscales", (P, 3)),
            ("dL_drotations", (P, 4)), ("dL_dviewmat", (4, 4)), ("dL_dprojmat", (4, 4)), ("dL_dcampos", (3,))],
            P, shade_grads if shade is not None else None)
        if scratch_fg:   # (outside the cleared region: only the blended surfels' rows are ever written and read)
            g["dL_dfeatures"] = N.out_tensor((P, S), torch.float32, dev)      # (NaN-filled under SVGIR_POISON: the tests see a row that is
            g["dL_dvfeatures"] = N.out_tensor((P, VS), torch.float32, dev)    # read without having been written)
        if P != 0:
            p, keep = B.call_params(N.SVGSS, dev, S, VS, degree, W, H, scale_modifier, tan_fovx, tan_fovy, debug, background, means3D, sh,
                                    colors, features, vfeatures, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos,
                                    **_svgss_fields(prcppoint, patchbbox, config))
            gs, gkeep = B.fill_grads(dev, upstream, g, gblob, out_weights)
            if shade is not None:
                p.shade = C.addressof(shade)
                for k, t in shade_grads.items():
                    setattr(gs, k, N.ptr(t))
            # scratch for the gradient accumulation: one row per (instance, sub-tile) pair that survived this view's cull (the
            # forward read the count back behind its cull), summed per Gaussian
            nscr = N.lib.svgir_backward_scratch_bytes_for(N.SVGSS, P, binningBuffer.numel(), imageBuffer.data_ptr(), W, H, S, VS)
            B.run_backward(dev, p, gs, R, radii, geomBuffer, binningBuffer, imageBuffer, nscr, **({} if sg_light is None else {"sg_light": sg_light}))
        return (g["dL_dmeans2D"], g["dL_dcolors"], g["dL_dopacity"], g["dL_dmeans3D"], g["dL_dfeatures"], g["dL_dvfeatures"],
                g["dL_dcov3D"], g["dL_dsh"], g["dL_dscales"], g["dL_drotations"], g["dL_dviewmat"], g["dL_dprojmat"], g["dL_dcampos"])

    @staticmethod
    def mark_visible(means3D, viewmatrix, projmatrix):
        return B.mark_visible(N.SVGSS, means3D, viewmatrix, projmatrix)


_C = _CBinding()


def forward_args(st, means3D, features, vfeatures, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                 viewmatrix, projmatrix, campos):
    """The 24 positional arguments of `_C.rasterize_gaussians` from the settings tuple `st` and the per-call tensors."""
    return (st.bg, means3D, features, vfeatures, colors_precomp, opacities, scales, rotations, st.scale_modifier, cov3Ds_precomp,
            viewmatrix, projmatrix, st.prcppoint, st.patch_bbox, st.tanfovx, st.tanfovy, st.image_height, st.image_width, sh,
            st.sh_degree, campos, st.prefiltered, st.debug, st.config)


def backward_args(st, means3D, features, vfeatures, radii, colors_precomp, scales, rotations, cov3Ds_precomp, sh, num_rendered,
                  geomBuffer, binningBuffer, imgBuffer, grad_out_color, grad_out_normal, grad_out_opacity, grad_out_depth,
                  grad_out_feature, grad_out_vfeature):
    """The 31 positional arguments of `_C.rasterize_gaussians_backward` (depth's gradient before opacity's: Q13); upstream gradients
    autograd left out (None) become empty tensors."""
    up = [B.grad_or_empty(g, means3D.device) for g in (grad_out_color, grad_out_normal, grad_out_depth, grad_out_opacity,
                                                        grad_out_feature, grad_out_vfeature)]
    return (st.bg, means3D, features, vfeatures, radii, colors_precomp, scales, rotations, st.scale_modifier, cov3Ds_precomp,
            st.viewmatrix, st.projmatrix, st.prcppoint, st.patch_bbox, st.tanfovx, st.tanfovy, *up, sh, st.sh_degree, st.campos,
            geomBuffer, num_rendered, binningBuffer, imgBuffer, st.debug, st.config)


def rasterize_gaussians(
    means3D,
    means2D,
    sh,
    features,
    vfeatures,
    colors_precomp,
    opacities,
    scales,
    rotations,
    cov3Ds_precomp,
    viewmatrix,
    projmatrix,
    campos,
    raster_settings,
):
    # Parameter names are mislabelled in the reference too (Q13); the positional pass-through is what matters.
    # (positionally: sh <- features, features <- vfeatures, vfeatures <- shs; see GaussianRasterizer.forward)
    # (every channel width the reference accepts runs through the C ABI: widths without a specialised composite kernel
    #  use the run-time-width kernels of csrc/render_generic.hip)
    return _RasterizeGaussians.apply(
        means3D, means2D, sh, features, vfeatures, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
        viewmatrix, projmatrix, campos, raster_settings)


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, features, vfeatures, sh, colors_precomp, opacities, scales, rotations,
                cov3Ds_precomp, viewmatrix, projmatrix, campos, raster_settings):
        args = forward_args(raster_settings, means3D, features, vfeatures, sh, colors_precomp, opacities, scales, rotations,
                            cov3Ds_precomp, viewmatrix, projmatrix, campos)
        fwd_only = not any(ctx.needs_input_grad)   # (evaluation / no_grad: the composite keeps no blend states for a backward)
        out = B.forward_with_snapshot(_C.rasterize_gaussians, args, dict(forward_only=fwd_only), raster_settings.debug)
        (num_rendered, color, normal, depth, opacity, feature, vfeature, weights, radii, geomBuffer, binningBuffer,
         imgBuffer) = out
        ctx.raster_settings = raster_settings
        ctx.num_rendered = num_rendered
        ctx.save_for_backward(colors_precomp, means3D, features, vfeatures, scales, rotations, cov3Ds_precomp, radii,
                              sh, geomBuffer, binningBuffer, imgBuffer, weights)
        ctx.mark_non_differentiable(weights, radii)
        return num_rendered, color, normal, opacity, depth, feature, vfeature, weights, radii

    @staticmethod
    def backward(ctx, grad_num_rendered, grad_out_color, grad_out_normal, grad_out_opacity, grad_out_depth,
                 grad_out_feature, grad_out_vfeature, grad_out_weights, grad_out_radii):
        raster_settings = ctx.raster_settings
        (colors_precomp, means3D, features, vfeatures, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer,
         binningBuffer, imgBuffer, weights) = ctx.saved_tensors
        args = backward_args(raster_settings, means3D, features, vfeatures, radii, colors_precomp, scales, rotations,
                             cov3Ds_precomp, sh, ctx.num_rendered, geomBuffer, binningBuffer, imgBuffer, grad_out_color,
                             grad_out_normal, grad_out_opacity, grad_out_depth, grad_out_feature, grad_out_vfeature)
        res = B.backward_with_snapshot(_C.rasterize_gaussians_backward, args, dict(out_weights=weights), raster_settings.debug)
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_features, grad_vfeatures,
         grad_cov3Ds_precomp, grad_sh, grad_scales, grad_rotations, grad_viewmat, grad_projmat, grad_campos) = res
        _m = B.grad_if_given
        grads = (
            grad_means3D,
            grad_means2D,
            _m(grad_features, features),
            _m(grad_vfeatures, vfeatures),
            _m(grad_sh, sh),
            _m(grad_colors_precomp, colors_precomp),
            grad_opacities,
            _m(grad_scales, scales),
            _m(grad_rotations, rotations),
            _m(grad_cov3Ds_precomp, cov3Ds_precomp),
            grad_viewmat,
            grad_projmat,
            grad_campos,
            None,
        )
        return grads


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    patch_bbox: torch.Tensor
    prcppoint: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    config: torch.Tensor


class GaussianRasterizer(B.RasterizerBase):
    variant = N.SVGSS

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, features=None, vfeatures=None):
        raster_settings = self.raster_settings
        shs, colors_precomp, scales, rotations, cov3D_precomp, features, vfeatures = B.rasterizer_inputs(
            means3D, shs, colors_precomp, scales, rotations, cov3D_precomp, features, vfeatures)

        # Invoke the HIP rasterization routine
        return rasterize_gaussians(
            means3D, means2D, features, vfeatures, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
            raster_settings.viewmatrix, raster_settings.projmatrix, raster_settings.campos, raster_settings)
