"""What the svgss and rgss rasterizer bindings share: the set-up of one call through the C ABI (svgir_params / svgir_outputs /
svgir_grads of include/svgir_raster.h), the forward's generator protocol, the backward's gradient allocation and call, and the small
pieces of the reference's Python wrappers that are the same in both modules.  svgss_rasterization.py / rgss_rasterization.py keep what
differs: signatures, which planes and gradients exist, tuple orders."""
import torch
import torch.nn as nn

from . import _native as N


def width(t):
    """Channel count of a [P, C] tensor; 0 for the empty placeholders."""
    return t.size(1) if t.dim() == 2 else 0


def sh_count(sh):
    return sh.size(1) if (sh is not None and sh.numel() != 0) else 0


def call_params(variant, dev, S, VS, degree, W, H, scale_modifier, tan_fovx, tan_fovy, debug, background, means3D, sh, colors,
                features, vfeatures, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, **more):
    """The svgir_params of one forward or backward call (ONE N.new_params(), made on the calling thread) and the list that keeps the
    contiguous fp32 copies behind its pointers alive.  `more`: the fields only one variant or one direction sets, by name; a tensor is
    passed like the fixed ones (fp32, contiguous, kept)."""
    keep = [N.f32c(t, dev) for t in (background, means3D, sh, colors, features, vfeatures, scales, rotations, cov3D_precomp,
                                      viewmatrix, projmatrix, campos)]
    (bg, m3, shc, col, fe, vf, sc, ro, cv, vm, pm, cp) = keep
    p = N.new_params()
    p.variant, p.P, p.S, p.VS, p.D, p.M, p.W, p.H = variant, m3.size(0), S, VS, int(degree), sh_count(shc), W, H
    p.background, p.means3D, p.shs, p.colors_precomp = N.ptr(bg), N.ptr(m3), N.ptr(shc), N.ptr(col)
    p.features, p.vfeatures = N.ptr(fe), N.ptr(vf)
    p.scales, p.rotations, p.cov3D_precomp = N.ptr(sc), N.ptr(ro), N.ptr(cv)
    p.viewmatrix, p.projmatrix, p.cam_pos = N.ptr(vm), N.ptr(pm), N.ptr(cp)
    p.scale_modifier, p.tan_fovx, p.tan_fovy = float(scale_modifier), float(tan_fovx), float(tan_fovy)
    p.debug = int(bool(debug))
    for name, v in more.items():
        if torch.is_tensor(v):
            v = N.f32c(v, dev)
            keep.append(v)
            v = N.ptr(v)
        setattr(p, name, v)
    return p, keep


# ---- forward ------------------------------------------------------------------------------------------------------------------

def check_forward_inputs(what, means3D):
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")  # rasterize_points.cu (both variants)
    if means3D.device.type != "cuda":
        raise RuntimeError(f"{what} rasterizer: tensors must live on the GPU (libsvgir_raster.so has no CPU path)")


def forward_call(variant, dev, P, planes, forward_only, *params, **more):
    """The body of a binding's `_forward_steps` generator (`yield from` it; N.run_forward / N.run_forward_batch drive it).
    `planes`: [(svgir_outputs field, shape)] of the fp32 image planes of the variant; `out_weights` [P,1] and `radii` [P] int32 are
    added.  `params` / `more`: see call_params.  Yields (dev, svgir_params, svgir_outputs, BlobAllocator) where the C call belongs, is
    sent the instance count and returns (count, {field: tensor}, BlobAllocator)."""
    planes = planes + [("out_weights", (P, 1))]
    if P == 0:  # nothing is launched: the reference returns its zero-initialised outputs (rasterize_points.cu:100)
        out = {name: torch.zeros(shape, dtype=torch.float32, device=dev) for name, shape in planes}
        out["radii"] = torch.zeros((P,), dtype=torch.int32, device=dev)
    else:       # every element is written by the library
        out = {name: N.out_tensor(shape, torch.float32, dev) for name, shape in planes}
        out["radii"] = N.out_tensor((P,), torch.int32, dev)
    blobs = N.BlobAllocator(dev)
    rendered = 0
    if P != 0:
        p, keep = call_params(variant, dev, *params, **more)
        p.forward_only = int(bool(forward_only))   # evaluation: no blend states are kept for a backward
        o = N.Outputs()
        for name, t in out.items():
            setattr(o, name, N.ptr(t))
        rendered = yield (dev, p, o, blobs)          # <- svgir_forward / svgir_forward_batch (gaussian_renderer/_native.py)
    return rendered, out, blobs


def rasterize_gaussians_batch(forward_steps, calls, device, streams):
    """`calls` = [(args, kwargs)] of a binding's rasterize_gaussians, one view each, launched with ONE svgir_forward_batch -- view v on
    streams[v], all views in flight before the first instance count is awaited (one host thread).  Returns the list of the binding's
    tuples.  The caller orders `streams` against the producers / consumers of the tensors."""
    return N.run_forward_batch([(lambda a=a, k=k: forward_steps(*a, **k)) for a, k in calls], device, streams)


# ---- backward -----------------------------------------------------------------------------------------------------------------

def upstream_size(upstream):
    """(H, W) from the first non-empty upstream gradient.  (An upstream gradient may be an EMPTY tensor = all zero: an output that
    took no part in the loss; nothing is read for it.)"""
    for t in upstream:
        if t is not None and t.numel():
            return t.size(1), t.size(2)
    raise RuntimeError("rasterize_gaussians_backward: every upstream gradient is empty")


def carve_gradients(dev, shapes, P, shade_grads=None):
    """{svgir_grads field: tensor} for `shapes` = [(field, shape)], carved out of ONE allocation (N.grad_blob: cleared by svgir_backward
    itself, zero-filled here when P == 0 and nothing runs), and that allocation.
    `shade_grads` (fused shading, gaussian_renderer/shading.py and bench.py): the caller asks for further per-surfel gradient tensors by
    shape in shade_grads["_shapes"] = {field: shape}.  The entry is popped, the tensors are carved out of the same allocation behind the
    fixed ones -- so the composite backward's clearing sweep zeroes them too, svgir_backward then writes the differentiated rows -- and
    stored under their names in the CALLER'S dict, which is how the caller reads them back after the call."""
    extra = list(shade_grads.pop("_shapes", {}).items()) if shade_grads is not None else []
    views, gblob = N.grad_blob(dev, [sh for _, sh in shapes] + [tuple(sh) for _, sh in extra], zero=(P == 0))
    for (name, _), v in zip(extra, views[len(shapes):]):
        shade_grads[name] = v
    return {name: v for (name, _), v in zip(shapes, views)}, gblob


def fill_grads(dev, upstream, grads, gblob, out_weights):
    """The svgir_grads of one backward call from {field: upstream gradient} and {field: gradient tensor}, and the keep-alive list.
    `out_weights`: the forward's weights [P,1] or None -- with them the per-Gaussian kernels behind the composite walk the blended
    Gaussians only (all others have zero gradients): through a list from a few hundred thousand surfels on, below that by a test of
    the weight inside the kernel."""
    g = N.Grads()
    keep = []
    for name, t in upstream.items():
        t = N.f32c(t, dev)
        keep.append(t)
        setattr(g, name, N.ptr(t))
    for name, t in grads.items():
        setattr(g, name, N.ptr(t))
    if N.CLEAR_HINT:
        g.clear_base, g.clear_bytes = gblob.data_ptr(), gblob.numel() * 4
    if out_weights is not None:
        w = N.f32c(out_weights, dev)
        keep.append(w)
        g.out_weights = N.ptr(w)
    return g, keep


def run_backward(dev, p, g, R, radii, geomBuffer, binningBuffer, imageBuffer, scratch_bytes, sg_light=None):
    """Allocates the gradient-accumulation scratch (its size is the variant's business) and calls svgir_backward on the current stream
    -- svgir_backward_sg when `sg_light` (a _native.SgLight: the light of the fused shading) is given."""
    rad = radii.contiguous()
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
    rest = (int(R), rad.data_ptr(), geomBuffer.data_ptr(), binningBuffer.data_ptr(), binningBuffer.numel(), imageBuffer.data_ptr(),
            scratch.data_ptr(), scratch_bytes, N.stream_ptr(dev))
    if sg_light is None:
        N.guarded(dev, "backward", N.lib.svgir_backward, p, g, *rest)
    else:
        N.guarded(dev, "backward_sg", N.lib.svgir_backward_sg, p, sg_light, g, *rest)


def mark_visible(variant, means3D, viewmatrix, projmatrix):
    P = means3D.size(0)
    present = torch.zeros((P,), dtype=torch.bool, device=means3D.device)
    if P != 0:
        m3, vm, pm = (N.f32c(t, means3D.device) for t in (means3D, viewmatrix, projmatrix))
        N.guarded(means3D.device, "mark_visible", N.lib.svgir_mark_visible, variant, P, m3.data_ptr(), vm.data_ptr(), pm.data_ptr(),
                  present.data_ptr(), N.stream_ptr(means3D.device))
    return present


# ---- the reference's Python wrappers --------------------------------------------------------------------------------------------

def cpu_deep_copy_tuple(input_tuple):
    copied_tensors = [item.cpu().clone() if isinstance(item, torch.Tensor) else item for item in input_tuple]
    return tuple(copied_tensors)


def call_with_snapshot(fn, args, kwargs, debug, dump_path, message):
    """fn(*args, **kwargs); with `debug` the arguments are copied to the CPU first (before they can be corrupted) and saved to
    `dump_path` if the call raises."""
    if not debug:
        return fn(*args, **kwargs)
    cpu_args = cpu_deep_copy_tuple(args)
    try:
        return fn(*args, **kwargs)
    except Exception as ex:
        torch.save(cpu_args, dump_path)
        print(message)
        raise ex


def forward_with_snapshot(fn, args, kwargs, debug):
    return call_with_snapshot(fn, args, kwargs, debug, "snapshot_fw.dump",
                              "\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")


def backward_with_snapshot(fn, args, kwargs, debug):
    return call_with_snapshot(fn, args, kwargs, debug, "snapshot_bw.dump",
                              "\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")


def grad_or_empty(g, dev):
    """autograd hands None for outputs that did not take part in the loss: an empty tensor = all zero for the library."""
    return g if g is not None else torch.empty(0, dtype=torch.float32, device=dev)


def grad_if_given(g, like):
    """No gradient for an input that was passed as an empty placeholder."""
    return g if (like is not None and like.numel() != 0) else None


def rasterizer_inputs(means3D, shs, colors_precomp, scales, rotations, cov3D_precomp, *features):
    """The argument checks and `empty` defaults of GaussianRasterizer.forward: returns (shs, colors_precomp, scales, rotations,
    cov3D_precomp, *features)."""
    if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
        raise Exception('Please provide excatly one of either SHs or precomputed colors!')

    if ((scales is None or rotations is None) and cov3D_precomp is None) or (
            (scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')

    empty = torch.empty(0, dtype=torch.float32, device=means3D.device)
    given = [empty if t is None else t for t in (shs, colors_precomp, scales, rotations, cov3D_precomp)]
    return (*given, *(torch.empty_like(means3D[..., :0]) if f is None else f for f in features))


class RasterizerBase(nn.Module):
    variant = None   # N.SVGSS / N.RGSS

    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        # Mark visible points (based on frustum culling for camera) with a boolean
        with torch.no_grad():
            raster_settings = self.raster_settings
            visible = mark_visible(self.variant, positions, raster_settings.viewmatrix, raster_settings.projmatrix)
        return visible
