"""`pbgi.renderer.Renderer` of the reference, the part `GaussianModel.update_radiace` uses (scene/gaussian_model.py:469-522):
`set_proxy_from_gaussian_model` (pbgi/renderer.py:429-466), `build_bvh` (:582-594) and `render_radiance_with_sampling_SH`
(:596-615) with their names, arguments, result order / shapes / dtypes and the attributes the caller reads back
(`LBVHNode_info`, `LBVHNode_aabb`, `hemi_index_buffers`, `uv_buffers`).  The slang kernels are the HIP kernels of
svg-ir_amd/csrc/pbgi.hip; no CPU / PyTorch fallback.

The consumers of those caches are here as well: `render_irradiance_sample` (:181-226, 748-751; the radiance-consistency loss of
`GaussianModel.get_radiance_loss`, scene/gaussian_model.py:544-575) and `render_irradiance` (:100-178, 743-746;
`GaussianModel.calculate_radiance`, :530-542), with the reference's names and positional arguments -> svg-ir_amd/csrc/irradiance.hip.
The contract, and what it decides where the reference is undefined, is in include/svgir_raster.h."""
import types

import torch

from gaussian_renderer import _native

from .bvhhelpers import GsBvh, _lib


def _irradiance_inputs(what, N, S, hit, uvs, envmap, ray_directions, normals, albedos, roughnesses):
    """Contiguous fp32 / int32 views of the kernels' arguments on the caches' device, shapes checked.  (envmap None: the fused loss, which
    has no [N,S,3] light; its slot of the result is None.)"""
    if hit is None or uvs is None:
        raise RuntimeError(f"{what}: hemi_index_buffers / uv_buffers are not set (GaussianModel.update_radiace sets them after "
                           "render_radiance_with_sampling_SH)")
    N, S = int(N), int(S)
    for t in (hit, uvs, envmap, ray_directions, normals, albedos, roughnesses):
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{what} needs CUDA/HIP tensors (there is no CPU path)")
    if hit.numel() != N * S or uvs.numel() != N * S * 2 or int(hit.shape[0]) != N:
        raise ValueError(f"{what}: hemi_index_buffers {tuple(hit.shape)} / uv_buffers {tuple(uvs.shape)} do not hold N = {N} rows of S = {S} samples")
    if S < 1:
        raise ValueError(f"{what}: S must be at least 1")
    dev = hit.device
    f = lambda t, shape: _native.f32c(t.detach(), dev).reshape(shape)
    hit_i = hit.detach().reshape(N, S)
    if hit_i.dtype != torch.int32:
        hit_i = hit_i.to(torch.int32)
    return dev, (f(ray_directions, (N, S, 3)), None if envmap is None else f(envmap, (N, S, 3)), f(normals, (N, 12)), f(albedos, (N, 12)), f(roughnesses, (N, 4)),
                 hit_i.contiguous(), f(uvs, (N, S, 2)))


class _IrradianceSample(torch.autograd.Function):
    """svgir_pbgi_irradiance_sample / _backward: differentiable in envmap, albedos and roughnesses (the reference's DiffTensorViews whose
    gradient is not identically zero); directions, normals, uvs and the indices get none."""

    @staticmethod
    def forward(ctx, N, S, sample_indices, envmap, albedos, roughnesses, ray_directions, normals, hit, uvs):
        dev, t = _irradiance_inputs("render_irradiance_sample", N, S, hit, uvs, envmap, ray_directions, normals, albedos, roughnesses)
        N, S = int(N), int(S)
        if not sample_indices.is_cuda or sample_indices.numel() != N:
            raise ValueError("render_irradiance_sample: sample_indices must be N indices on the GPU")
        idx = sample_indices.detach().reshape(N).to(device=dev, dtype=torch.int32).contiguous()
        with torch.cuda.device(dev):
            out = _native.out_tensor((N, 3), torch.float32, dev)
            _native.check(_lib.svgir_pbgi_irradiance_sample(N, S, _native.ptr(idx), *[_native.ptr(x) for x in t], _native.ptr(out),
                                                            _native.stream_ptr(dev)), "pbgi_irradiance_sample")
        ctx.save_for_backward(idx, *t)
        ctx.dims = (N, S, envmap.shape, albedos.shape, roughnesses.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        idx, *t = ctx.saved_tensors
        N, S, env_shape, alb_shape, rough_shape = ctx.dims
        dev = idx.device
        with torch.cuda.device(dev):
            g = _native.f32c(g, dev)
            d_env = _native.out_tensor((N, S, 3), torch.float32, dev)
            d_alb = _native.out_tensor((N, 12), torch.float32, dev)
            d_rough = _native.out_tensor((N, 4), torch.float32, dev)
            _native.check(_lib.svgir_pbgi_irradiance_sample_backward(N, S, _native.ptr(idx), *[_native.ptr(x) for x in t], _native.ptr(g),
                                                                     _native.ptr(d_env), _native.ptr(d_alb), _native.ptr(d_rough),
                                                                     _native.stream_ptr(dev)), "pbgi_irradiance_sample_backward")
        return (None, None, None, d_env.reshape(env_shape), d_alb.reshape(alb_shape), d_rough.reshape(rough_shape), None, None, None, None)


class _ConsistencyNode(torch.autograd.Function):
    """The whole radiance-consistency loss as one autograd node; what both light kinds share.  A subclass names its two C entry points
    (`FORWARD`, `BACKWARD`) and supplies `light(what, leaf, spec, dev)`: a namespace with `args` (the C arguments behind the parameter
    block), `fields` (plain fields of the block), `tensors(f)` (its tensor fields; f: the shape-checked fp32 view), `held` (what else must
    stay alive), `work_bytes(N)` and `grad_shape`.  Differentiable in leaf (the light's parameter), albedos, roughnesses and
    radiance_ratio; everything else gets None.  Returns (loss, sample_indices [N] int32, radiance [N,3], loss_sum (float64 scalar));
    only the loss carries a graph."""

    @classmethod
    def _forward(cls, ctx, what, leaf, spec, on_device, albedos, roughnesses, radiance_ratio, xyz, camera_center, geo_normal, ray_directions, areas,
                 visibility, normals, radiances, hit, uvs):
        N, S = int(ray_directions.shape[0]), int(ray_directions.shape[1])
        for t in (leaf, xyz, camera_center, geo_normal, areas, visibility, radiances, radiance_ratio) + on_device:
            if not t.is_cuda:
                raise RuntimeError(f"{what} needs CUDA/HIP tensors (there is no CPU path)")
        dev, t = _irradiance_inputs(what, N, S, hit, uvs, None, ray_directions, normals, albedos, roughnesses)
        f = lambda x, shape, name: _rows(what, _native.f32c(x.detach(), dev), shape, name)
        lt = cls.light(what, leaf, spec, dev)
        p = _native.RadianceLossParams()
        keep = dict(xyz=f(xyz, (N, 3), "xyz"), camera_center=f(camera_center, (3,), "camera_center"), geo_normal=f(geo_normal, (N, 3), "geo_normal"),
                    ray_d=t[0], areas=f(areas, (N, S), "incident_areas"), visibility=f(visibility, (N, S), "visibility"), normals=t[2],
                    albedos=t[3], roughnesses=t[4], hit_indices=t[5], uvs=t[6], radiances=f(radiances, (N, S, 3), "radiances"),
                    radiance_ratio=f(radiance_ratio, (1,), "radiance_ratio"), **lt.tensors(f))
        with torch.cuda.device(dev):
            keep["work"] = torch.empty(max(lt.work_bytes(N), 16), dtype=torch.uint8, device=dev)
            p.N, p.S = N, S
            for k, v in lt.fields.items():
                setattr(p, k, v)
            for k, v in keep.items():
                setattr(p, k, _native.ptr(v))
            idx = _native.out_tensor((N,), torch.int32, dev)
            R = _native.out_tensor((N, 3), torch.float32, dev)
            total = _native.out_tensor((), torch.float64, dev)
            loss = _native.out_tensor((), torch.float32, dev)
            if N == 0:   # nothing is launched: the mean of no rows is NaN, as torch's
                total.zero_()
                loss.fill_(float("nan"))
            _native.check(getattr(_lib, cls.FORWARD)(p, *lt.args, _native.ptr(idx), _native.ptr(R), total.data_ptr(), loss.data_ptr(),
                                                     _native.stream_ptr(dev)), cls.FORWARD[len("svgir_"):])
        # The backward reads the inputs through the raw pointers of the parameter block (and of the SG light); `keep` holds the tensors
        # behind them (the fp32 / contiguous copies where one was made, and the work buffer).  Unlike save_for_backward this does not notice
        # an in-place change of an input between forward and backward: the backward then differentiates the changed values.
        ctx.p, ctx.lt, ctx.keep = p, lt, keep
        ctx.save_for_backward(idx, R)
        ctx.shapes = (leaf.shape, albedos.shape, roughnesses.shape, radiance_ratio.shape)
        ctx.mark_non_differentiable(idx, R, total)
        return loss, idx, R, total

    @classmethod
    def _backward(cls, ctx, g):
        idx, R = ctx.saved_tensors
        p, lt = ctx.p, ctx.lt
        N = p.N
        dev = idx.device
        need_light, _, _, need_ratio = ctx.needs_input_grad[:4]
        with torch.cuda.device(dev):
            d_light = _native.out_tensor(lt.grad_shape, torch.float32, dev) if need_light else None
            d_alb = _native.out_tensor((N, 12), torch.float32, dev)
            d_rough = _native.out_tensor((N, 4), torch.float32, dev)
            d_ratio = _native.out_tensor((1,), torch.float32, dev) if need_ratio else None
            if N == 0:
                for t in (d_light, d_ratio):
                    if t is not None:
                        t.zero_()
            gdev = _native.f32c(g.detach(), dev).reshape(1).contiguous()   # the upstream scalar stays on the device
            _native.check(getattr(_lib, cls.BACKWARD)(p, *lt.args, _native.ptr(idx), _native.ptr(R), gdev.data_ptr(), _native.ptr(d_light),
                                                      _native.ptr(d_alb), _native.ptr(d_rough), _native.ptr(d_ratio), _native.stream_ptr(dev)),
                          cls.BACKWARD[len("svgir_"):])
        light_shape, alb_shape, rough_shape, ratio_shape = ctx.shapes
        return (None if d_light is None else d_light.reshape(light_shape), d_alb.reshape(alb_shape), d_rough.reshape(rough_shape),
                None if d_ratio is None else d_ratio.reshape(ratio_shape)) + (None,) * (len(ctx.needs_input_grad) - 4)


class _RadianceConsistency(_ConsistencyNode):
    """The lat-long texture: env is the map, light = (softplus, scale, transform)."""
    FORWARD, BACKWARD = "svgir_radiance_loss_forward", "svgir_radiance_loss_backward"

    @staticmethod
    def light(what, env, spec, dev):
        softplus, scale, transform = spec
        e = _native.f32c(env.detach(), dev)
        if e.dim() < 3 or e.shape[-1] != 3 or e.shape[-3] < 1 or e.shape[-2] < 1 or e.numel() != e.shape[-3] * e.shape[-2] * 3:
            raise ValueError(f"{what}: the light's map must be ONE [He,We,3] map (leading dimensions of 1 are fine), got {tuple(env.shape)}")
        e = e.reshape(e.shape[-3:]).contiguous()
        he, we = int(e.shape[0]), int(e.shape[1])
        return types.SimpleNamespace(
            args=(), fields=dict(env_h=he, env_w=we, env_softplus=int(bool(softplus)), env_scale=float(scale)), held=None,
            tensors=lambda f: dict(env=e, env_transform=None if transform is None else f(transform, (3, 3), "the light's transform")),
            work_bytes=lambda N: _lib.svgir_radiance_loss_work_bytes(N, he, we), grad_shape=(he, we, 3))

    @staticmethod
    def forward(ctx, env, albedos, roughnesses, radiance_ratio, light, *rest):
        return _RadianceConsistency._forward(ctx, "radiance_consistency", env, light, () if light[2] is None else (light[2],), albedos,
                                             roughnesses, radiance_ratio, *rest)

    @staticmethod
    def backward(ctx, g, _gi, _gr, _gt):
        return _RadianceConsistency._backward(ctx, g)


class _RadianceConsistencySG(_ConsistencyNode):
    """A spherical-Gaussian light: the raw lobes [M,7] in the texture's place."""
    FORWARD, BACKWARD = "svgir_radiance_loss_forward_sg", "svgir_radiance_loss_backward_sg"

    @staticmethod
    def light(what, lobes, spec, dev):
        from gaussian_renderer import shading
        lt, held = shading._sg_light(shading.SGLobes(lobes).lobes, dev)
        return types.SimpleNamespace(args=(lt,), fields={}, held=held, tensors=lambda f: {},
                                     work_bytes=lambda N: _lib.svgir_radiance_loss_sg_work_bytes(N, lt.count), grad_shape=(lt.count, 7))

    @staticmethod
    def forward(ctx, lobes, albedos, roughnesses, radiance_ratio, *rest):
        return _RadianceConsistencySG._forward(ctx, "radiance_consistency_sg", lobes, None, (), albedos, roughnesses, radiance_ratio, *rest)

    @staticmethod
    def backward(ctx, g, _gi, _gr, _gt):
        return _RadianceConsistencySG._backward(ctx, g)


def _rows(what, t, shape, name):
    n = 1
    for d in shape:
        n *= d
    if t.numel() != n or (len(shape) > 1 and t.numel() and int(t.shape[0]) != shape[0]):
        raise ValueError(f"{what}: {name} {tuple(t.shape)} does not hold {shape}")
    return t.reshape(shape).contiguous()


class Renderer:
    def __init__(self):
        self.proxy_xyzs = None
        self.hemi_index_buffers = None
        self.uv_buffers = None
        self.hti_indices = None
        self.proxy_rot_mats = None
        self._bvh = None
        self.LBVHNode_info = None
        self.LBVHNode_aabb = None

    def set_proxy_from_gaussian_model(self, pc):
        """Every surfel is a proxy (the reference's opacity filter is `> 0.0` and is only used for `proxy_idx`)."""
        self.set_proxy(pc.get_xyz, pc.get_scaling, pc.get_rotation, pc.get_geo_normal, pc.get_opacity, pc.get_features)

    def set_proxy(self, xyzs, scales, rotates, normals, opacity, features):
        """The tensors the tracer reads (renderer.py:442-454): xyz [P,3], scaling [P,3], rotation [P,4] (r,x,y,z), geometric
        normals [P,3], opacity [P,1] or [P], SH features [P,16,3]."""
        self.proxy_xyzs, self.proxy_scales, self.proxy_rotates = xyzs, scales, rotates
        self.proxy_normals, self.proxy_opacity, self.proxy_features = normals, opacity, features
        self.proxy_idx = torch.nonzero(opacity.reshape(-1) > 0.0)[..., 0].long()

    def build_bvh(self):
        if self.proxy_idx.shape[0] == 0:
            return
        self._bvh = GsBvh(self.proxy_xyzs, self.proxy_scales)
        self.LBVHNode_info, self.LBVHNode_aabb = self._bvh.tensors()

    @torch.no_grad()
    def render_radiance_with_sampling_SH(self, ray_o, ray_d, cov3D_inv, sample_num=64):
        """ray_o [N,3] (one origin per row), ray_d [N,sample_num,3], cov3D_inv [P,6] ->
        (radiance [N,S,3], visibility [N,S,1], hit_indices [N,S,1] int32, uvs [N,S,2])."""
        if self._bvh is None:
            raise RuntimeError("build_bvh() first")
        dev, P = self._bvh.device, self._bvh.P
        N, S = int(ray_d.shape[0]), int(sample_num)
        if tuple(ray_d.shape) != (N, S, 3) or int(self.proxy_features.shape[1]) < 16:
            raise ValueError("ray_d must be [N, sample_num, 3] and the SH features [P, >=16, 3]")
        with torch.cuda.device(dev):
            f = lambda t: _native.f32c(t.detach(), dev)
            ro, rd = f(ray_o.reshape(N, 3)), f(ray_d)
            shs = f(self.proxy_features[:, :16, :])
            args = [f(self.proxy_xyzs), f(self.proxy_scales), f(self.proxy_rotates), f(self.proxy_normals),
                    f(self.proxy_opacity.reshape(-1)), f(cov3D_inv), shs]
            rad = _native.out_tensor((N, S, 3), torch.float32, dev)
            vis = _native.out_tensor((N, S, 1), torch.float32, dev)
            hit = _native.out_tensor((N, S, 1), torch.int32, dev)
            uvs = _native.out_tensor((N, S, 2), torch.float32, dev)
            _native.check(_lib.svgir_pbgi_trace_radiance(P, self._bvh.blob.data_ptr(), N, S, _native.ptr(ro), _native.ptr(rd),
                                                        *[_native.ptr(t) for t in args], rad.data_ptr(), vis.data_ptr(), hit.data_ptr(),
                                                        uvs.data_ptr(), _native.stream_ptr(dev)), "pbgi_trace_radiance")
        return rad, vis, hit, uvs

    def render_irradiance(self, N, S, envmap, ray_directions, centers, scales, rotates, normals, albedos, roughnesses, metallics, opacities, SHs):
        """The incident-radiance cache under `envmap` [N,S,3] (pbgi/renderer.py:743-746): [N,S,3], per (i,p) the irradiance the first hit
        of ray p of surfel i reflects towards i, with per-corner roughness and the n.l cosine.  Reads `self.hemi_index_buffers`
        ([N,S,1] int32) and `self.uv_buffers` ([N,S,2]).  centers, scales, rotates, metallics, opacities and SHs never reach the
        reference's result and are ignored.  FORWARD ONLY: the result carries no autograd graph (nobody differentiates it in the
        reference: calculate_radiance feeds update_radiance_with_calc)."""
        dev, t = _irradiance_inputs("render_irradiance", N, S, self.hemi_index_buffers, self.uv_buffers, envmap, ray_directions, normals,
                                    albedos, roughnesses)
        N, S = int(N), int(S)
        with torch.cuda.device(dev):
            out = _native.out_tensor((N, S, 3), torch.float32, dev)
            _native.check(_lib.svgir_pbgi_irradiance(N, S, *[_native.ptr(x) for x in t], _native.ptr(out), _native.stream_ptr(dev)),
                          "pbgi_irradiance")
        return out

    def render_irradiance_sample(self, N, S, sample_indices, envmap, ray_directions, centers, scales, rotates, normals, albedos, roughnesses,
                                 metallics, opacities, SHs):
        """[N,3]: the same sum for ONE ray per surfel, p = sample_indices[i] ([N] or [N,1] integers), with the reference's two quirks
        (corner 0's roughness for all corners, no cosine; pbgi/renderer.py:748-751).  Differentiable in envmap, albedos and roughnesses;
        every other argument gets no gradient (None).  Reads `self.hemi_index_buffers` and `self.uv_buffers`."""
        return _IrradianceSample.apply(N, S, sample_indices, envmap, albedos, roughnesses, ray_directions, normals, self.hemi_index_buffers,
                                       self.uv_buffers)

    def radiance_consistency(self, xyz, camera_center, geo_normal, incident_dirs, incident_areas, visibility, env, env_softplus, env_scale,
                             env_transform, normals, albedos, roughnesses, radiances, radiance_ratio, with_sum=False):
        """`GaussianModel.get_radiance_loss` (scene/gaussian_model.py:544-575) as ONE autograd node (svgir_radiance_loss_forward /
        _backward, csrc/irradiance.hip): the selection of the sample, the light `env_scale * bilinear(f(env))(incident_dirs) *
        incident_areas` of the hit surfel (f = softplus when `env_softplus`; `env_transform` [3,3] or None rotates the lookup direction),
        the irradiance sum of `render_irradiance_sample` and the L1 against nan_to_num(radiances * radiance_ratio).  Reads
        `self.hemi_index_buffers` and `self.uv_buffers`.  Returns (loss, sample_indices [N] int32, radiance [N,3]) -- with_sum: and the
        float64 sum of |radiance - target| the loss is the rounding of.  Gradients reach env (when it requires grad), albedos,
        roughnesses and radiance_ratio; a row whose radiance or target is not finite makes the loss NaN and gets no gradient
        (include/svgir_raster.h)."""
        out = _RadianceConsistency.apply(env, albedos, roughnesses, radiance_ratio, (env_softplus, env_scale, env_transform), xyz,
                                         camera_center, geo_normal, incident_dirs, incident_areas, visibility, normals, radiances,
                                         self.hemi_index_buffers, self.uv_buffers)
        return out if with_sum else out[:3]

    def radiance_consistency_sg(self, xyz, camera_center, geo_normal, incident_dirs, incident_areas, visibility, lgtSGs, normals, albedos,
                                roughnesses, radiances, radiance_ratio, with_sum=False):
        """radiance_consistency under the reference's DirectLightSG (svgir_radiance_loss_forward_sg / _backward_sg): the light of a
        sample is the unclamped mixture of the raw lobes `lgtSGs` [M,7] along its incident direction times its area; everything else --
        the selection, the hit rules, the target, the non-finite rule, the returned tuple -- is radiance_consistency's.  Gradients reach
        lgtSGs (when it requires grad), albedos, roughnesses and radiance_ratio."""
        out = _RadianceConsistencySG.apply(lgtSGs, albedos, roughnesses, radiance_ratio, xyz, camera_center, geo_normal, incident_dirs,
                                           incident_areas, visibility, normals, radiances, self.hemi_index_buffers, self.uv_buffers)
        return out if with_sum else out[:3]
