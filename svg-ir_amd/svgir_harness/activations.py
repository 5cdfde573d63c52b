"""The model's activation getters as one HIP kernel pair (csrc/activate.hip; include/svgir_raster.h: svgir_activate_forward /
svgir_activate_backward): the step from the optimizer's raw parameters to the tensors the shading and the rasterizer consume --
`GaussianModel.get_scaling / get_rotation / get_opacity / get_geo_normal / get_shading_normal / get_base_color / get_albedo /
get_roughness` (scene/gaussian_model.py:104-125, 270-355), `viewdirs` (gaussian_renderer/svgss.py:109) and the regulariser
`mse_loss(_normal, 0)` (svgss.py:316).

    act = activate({"xyz": ..., "scaling": ..., "rotation": ..., ...}, campos=camera_center, base_color_scale=None)
    act["scales"], act["rotations"], act["opacities"], act["geo_normal"], act["shading_normal"], act["shading_normal12"],
    act["base_color"], act["roughness"], act["viewdirs"]            (+ act["normal_reg"] with normal_reg=True)

One autograd node: one launch forward, one backward.  The outputs are views of ONE allocation, and so are the raw gradients.  There is
no CPU path and no eager fallback: CPU tensors raise.  One deviation from torch's autograd (include/svgir_raster.h): where nan_to_num
replaced a value, the raw element gets zero gradient instead of NaN."""
import ctypes as C

import torch

from gaussian_renderer import _native as N

RAW = ("xyz", "scaling", "rotation", "opacity", "normal", "base_color", "roughness")
RAW_WIDTH = {"xyz": 3, "scaling": 3, "rotation": 4, "opacity": 1, "normal": 12, "base_color": 12, "roughness": 4}
OUTPUTS = ("scales", "rotations", "opacities", "geo_normal", "shading_normal", "shading_normal12", "base_color", "roughness", "viewdirs")
OUT_SHAPE = {"scales": (3,), "rotations": (4,), "opacities": (1,), "geo_normal": (3,), "shading_normal": (4, 3), "shading_normal12": (12,),
             "base_color": (12,), "roughness": (4,), "viewdirs": (3,)}
# the raw inputs an output reads (viewdirs also needs campos)
READS = {"scales": ("scaling",), "rotations": ("rotation",), "opacities": ("opacity",), "geo_normal": ("rotation",),
         "shading_normal": ("rotation", "normal"), "shading_normal12": ("rotation", "normal"), "base_color": ("base_color",),
         "roughness": ("roughness",), "viewdirs": ("xyz",), "normal_reg": ("normal",)}
_FIELD = {"base_color": "out_base_color", "roughness": "out_roughness"}   # struct fields whose name differs from the output's


def _block(P, raw, campos, bcs):
    a = N.Activation()
    a.P = P
    for k, t in zip(RAW, raw):
        setattr(a, k, N.ptr(t))
    a.campos, a.base_color_scale = N.ptr(campos), N.ptr(bcs)
    return a


class _Activate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, want, normal_reg, campos, bcs, *raw):
        given = [t for t in raw if t is not None]
        if not given:
            raise RuntimeError("activate: no raw parameter given")
        dev = given[0].device
        if any(t.device.type != "cuda" for t in given + [t for t in (campos, bcs) if t is not None]):
            raise RuntimeError("activate: tensors must live on the GPU (libsvgir_raster.so has no CPU path)")
        P = int(given[0].shape[0])
        for k, t in zip(RAW, raw):
            if t is not None and (t.numel() != P * RAW_WIDTH[k] or t.shape[0] != P):
                raise RuntimeError(f"activate: {k} must hold {RAW_WIDTH[k]} values for each of the {P} surfels, got {tuple(t.shape)}")
        raw = [N.f32c(t.detach(), dev) if t is not None else None for t in raw]
        campos = N.f32c(campos.detach().reshape(3), dev) if campos is not None else None
        bcs = N.f32c(bcs.detach().reshape(3), dev) if bcs is not None else None
        views, blob = N.grad_blob(dev, [(P,) + OUT_SHAPE[k] for k in want], zero=P == 0)
        reg = reg_sum = None
        if normal_reg:
            reg, reg_sum = N.out_tensor((1,), torch.float32, dev), N.out_tensor((1,), torch.float64, dev)
        if P:
            a = _block(P, raw, campos, bcs)
            for k, v in zip(want, views):
                setattr(a, _FIELD.get(k, k), v.data_ptr())
            if normal_reg:
                partial = torch.empty(N.lib.svgir_activate_partials(P), dtype=torch.float64, device=dev)
                a.partial, a.normal_reg_sum, a.normal_reg = partial.data_ptr(), reg_sum.data_ptr(), reg.data_ptr()
            N.guarded(dev, "activate forward", N.lib.svgir_activate_forward, C.byref(a), N.stream_ptr(dev))
        elif normal_reg:   # the mean of nothing, as torch's
            reg.fill_(float("nan")); reg_sum.zero_()
        ctx.save_for_backward(campos, bcs, *raw)
        ctx.want, ctx.normal_reg, ctx.P, ctx.dev = want, normal_reg, P, dev
        ctx.set_materialize_grads(False)   # an output outside the graph arrives as None, not as zeros
        out = tuple(views)
        if normal_reg:
            out += (reg[0], reg_sum[0])
            ctx.mark_non_differentiable(out[-1])
        return out

    @staticmethod
    def backward(ctx, *gout):
        campos, bcs, *raw = ctx.saved_tensors
        P, dev = ctx.P, ctx.dev
        need = [bool(n) and t is not None for n, t in zip(ctx.needs_input_grad[4:], raw)]
        if not any(need):
            return (None,) * (4 + len(RAW))
        names = [k for k, n in zip(RAW, need) if n]
        views, _ = N.grad_blob(dev, [tuple(raw[RAW.index(k)].shape) for k in names], zero=P == 0)
        if P:
            g = N.ActivationGrads()
            keep = []
            for k, t in zip(ctx.want, gout):
                if t is not None:
                    t = N.f32c(t, dev)
                    keep.append(t)
                    setattr(g, "dL_d" + _FIELD.get(k, k), t.data_ptr())
            if ctx.normal_reg and gout[len(ctx.want)] is not None:
                t = N.f32c(gout[len(ctx.want)].reshape(1), dev)
                keep.append(t)
                g.dL_dnormal_reg = t.data_ptr()
            for k, v in zip(names, views):
                setattr(g, "dL_d" + k, v.data_ptr())
            a = _block(P, raw, campos, bcs)
            N.guarded(dev, "activate backward", N.lib.svgir_activate_backward, C.byref(a), C.byref(g), N.stream_ptr(dev))
        res = dict(zip(names, views))
        return (None,) * 4 + tuple(res.get(k) for k in RAW)


def activate(raw, campos=None, base_color_scale=None, want=OUTPUTS, normal_reg=False):
    """Activated tensors of the raw parameter dict `raw` (optimizer-group names: xyz [P,3], scaling [P,3], rotation [P,4] as (r,x,y,z),
    opacity [P,1], normal [P,12], base_color [P,12], roughness [P,4]; a group no requested output reads may be absent -- stage 1 passes
    no materials).  `campos` [3]: the camera centre (viewdirs); `base_color_scale` [3] or None (= ones).  `want`: the outputs to
    produce, `normal_reg`: also `normal_reg` = mean(normal^2) (device float; the reference's 0.1 stays with the caller) and
    `normal_reg_sum` (its double sum, not differentiable).  Differentiable in every raw group."""
    want = tuple(want)
    for k in want:
        if k not in OUT_SHAPE:
            raise ValueError(f"activate: unknown output {k!r} (known: {', '.join(OUTPUTS)})")
    for k in want + (("normal_reg",) if normal_reg else ()):
        for r in READS[k]:
            if raw.get(r) is None:
                raise RuntimeError(f"activate: output {k!r} needs the raw parameter {r!r}")
    if "viewdirs" in want and campos is None:
        raise RuntimeError("activate: output 'viewdirs' needs campos")
    read = {r for k in want + (("normal_reg",) if normal_reg else ()) for r in READS[k]}
    out = _Activate.apply(want, bool(normal_reg), campos, base_color_scale, *[raw.get(k) if k in read else None for k in RAW])
    res = dict(zip(want, out))
    if normal_reg:
        res["normal_reg"], res["normal_reg_sum"] = out[len(want)], out[len(want) + 1]
    return res


class ModelActivations:
    """The reference's getter names over a raw parameter dict (scene/gaussian_model.py:270-355).  `refresh(campos)` runs the kernel once
    per iteration; the properties return views of its one output block."""

    def __init__(self, raw_params, base_color_scale=None, want=None, normal_reg=False):
        self.raw, self.base_color_scale, self.normal_reg = raw_params, base_color_scale, normal_reg
        if want is None:
            want = tuple(k for k in OUTPUTS if all(raw_params.get(r) is not None for r in READS[k]))
        self.want = tuple(want)
        self.act = None

    def refresh(self, campos=None):
        want = tuple(k for k in self.want if k != "viewdirs" or campos is not None)
        self.act = activate(self.raw, campos, self.base_color_scale, want, self.normal_reg and self.raw.get("normal") is not None)
        return self.act

    def _get(self, name):
        if self.act is None or name not in self.act:
            raise RuntimeError(f"ModelActivations: {name!r} is not available (call refresh(campos) first, with the raw parameters it reads)")
        return self.act[name]

    get_xyz = property(lambda self: self.raw["xyz"])
    get_normals = property(lambda self: self.raw["normal"])
    get_scaling = property(lambda self: self._get("scales"))
    get_rotation = property(lambda self: self._get("rotations"))
    get_opacity = property(lambda self: self._get("opacities"))
    get_geo_normal = property(lambda self: self._get("geo_normal"))
    get_shading_normal = property(lambda self: self._get("shading_normal"))
    get_shading_normal12 = property(lambda self: self._get("shading_normal12"))
    get_base_color = property(lambda self: self._get("base_color"))
    get_albedo = property(lambda self: self._get("base_color"))
    get_roughness = property(lambda self: self._get("roughness"))
    viewdirs = property(lambda self: self._get("viewdirs"))
    normal_reg_value = property(lambda self: self._get("normal_reg"))
