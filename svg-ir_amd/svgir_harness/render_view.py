"""End-to-end svgss view: shading -> packing -> rasterizer -> unpacking, the sequence of the reference's
`render_view` (gaussian_renderer/svgss.py:51-262) with explicit tensors instead of its scene / camera classes.

Only the parts that belong to the hot path and its immediate callers are reproduced: the SV-BRDF shading and packing
(svgss.py:125-166, fused: gaussian_renderer/shading.py), the rasterizer call (:170-182) and the image-space unpacking
(:188-246: division by the rendered opacity, channel split, sRGB, compositing over the background) and the environment
backdrop that ends every eval view (:255-260: `environment_backdrop`, from the camera's intrinsics and rotation).  The
`depth2normal` pseudo normal needs the reference's camera class and is left to the caller."""
import ctypes as C

import numpy as np
import torch

from gaussian_renderer import _native as N
from gaussian_renderer import shading
from gaussian_renderer.svgss_rasterization import GaussianRasterizer

from . import runner

N.lib.svgir_unpack_planes.restype = C.c_int
N.lib.svgir_unpack_planes.argtypes = [C.c_int32]
N.lib.svgir_unpack_forward.restype = C.c_int
N.lib.svgir_unpack_forward.argtypes = [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6
N.lib.svgir_unpack_backward.restype = C.c_int
N.lib.svgir_unpack_backward.argtypes = [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 9
N.lib.svgir_depth2normal.restype = C.c_int
N.lib.svgir_depth2normal.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float,
                                    C.c_void_p, C.c_void_p]

for _n, _k in (("svgir_pack_rgss_forward", 5), ("svgir_pack_rgss_backward", 6)):
    getattr(N.lib, _n).restype = C.c_int
    getattr(N.lib, _n).argtypes = [C.c_int32] + [C.c_void_p] * _k
for _n, _k in (("svgir_unpack_rgss_forward", 6), ("svgir_unpack_rgss_backward", 9)):
    getattr(N.lib, _n).restype = C.c_int
    getattr(N.lib, _n).argtypes = [C.c_int32, C.c_int32] + [C.c_void_p] * _k

TRAIN_PLANES = ("pbr", "normal", "base_color", "roughness", "diffuse", "local_lights", "visibility")
EVAL_PLANES = ("pbr", "normal", "base_color", "roughness", "direct", "indirect", "lights", "local_lights", "visibility")


class _Unpack(torch.autograd.Function):
    """svgir_unpack_forward / svgir_unpack_backward (csrc/epilogue.hip): one pass over the rasterizer's planes."""

    @staticmethod
    def forward(ctx, opacity, feature, vfeature, bg, training):
        dev = opacity.device
        if dev.type != "cuda":
            raise RuntimeError("unpack: tensors must live on the GPU (libsvgir_raster.so has no CPU path)")
        op, fe, vf, bgc = (N.f32c(t, dev) for t in (opacity, feature, vfeature, bg))
        H, W = op.shape[-2], op.shape[-1]
        S, VC = (4, 13) if training else (7, 16)
        if fe.shape[0] != S or vf.shape[0] != VC:
            raise RuntimeError(f"unpack: expected {S} feature / {VC} vfeature planes, got {fe.shape[0]} / {vf.shape[0]}")
        out = torch.empty((N.lib.svgir_unpack_planes(int(training)), H, W), dtype=torch.float32, device=dev)
        N.check(N.lib.svgir_unpack_forward(W, H, int(training), bgc.data_ptr(), op.data_ptr(), fe.data_ptr(), vf.data_ptr(),
                                           out.data_ptr(), N.stream_ptr(dev)), "unpack_forward")
        ctx.save_for_backward(op, fe, vf, bgc)
        ctx.training = training
        return out

    @staticmethod
    def backward(ctx, g_out):
        op, fe, vf, bgc = ctx.saved_tensors
        dev = op.device
        H, W = op.shape[-2], op.shape[-1]
        g = N.f32c(g_out, dev)
        d_op, d_fe, d_vf = torch.empty_like(op), torch.empty_like(fe), torch.empty_like(vf)
        N.check(N.lib.svgir_unpack_backward(W, H, int(ctx.training), bgc.data_ptr(), op.data_ptr(), fe.data_ptr(), vf.data_ptr(),
                                            g.data_ptr(), d_op.data_ptr(), d_fe.data_ptr(), d_vf.data_ptr(), N.stream_ptr(dev)),
                "unpack_backward")
        return d_op, d_fe, d_vf, None, None


class _PackRgss(torch.autograd.Function):
    """render.py:83-91: features = [geo normal, view depth, depth^2] (svgir_pack_rgss_forward / _backward)."""

    @staticmethod
    def forward(ctx, means3D, normals, viewmatrix):
        dev = means3D.device
        m3, nr, vm = (N.f32c(t, dev) for t in (means3D, normals, viewmatrix))
        out = torch.empty((m3.shape[0], 5), dtype=torch.float32, device=dev)
        N.check(N.lib.svgir_pack_rgss_forward(m3.shape[0], N.ptr(m3), N.ptr(nr), vm.data_ptr(), N.ptr(out), N.stream_ptr(dev)), "pack_rgss")
        ctx.save_for_backward(m3, vm)
        return out

    @staticmethod
    def backward(ctx, g):
        m3, vm = ctx.saved_tensors
        dev = m3.device
        g = N.f32c(g, dev)
        d_m, d_n = torch.empty_like(m3), torch.empty_like(m3)
        N.check(N.lib.svgir_pack_rgss_backward(m3.shape[0], N.ptr(m3), vm.data_ptr(), N.ptr(g), N.ptr(d_m), N.ptr(d_n), N.stream_ptr(dev)),
                "pack_rgss_backward")
        return d_m, d_n, None


class _UnpackRgss(torch.autograd.Function):
    """render.py:107-114 (svgir_unpack_rgss_forward / _backward): [normal3, depth, depth2, depth_var] planes."""

    @staticmethod
    def forward(ctx, num_contrib, opacity, depth, feature):
        dev = opacity.device
        nc = num_contrib.to(torch.int32).contiguous()
        op, de, fe = (N.f32c(t, dev) for t in (opacity, depth, feature))
        H, W = op.shape[-2], op.shape[-1]
        if fe.shape[0] != 5:
            raise RuntimeError("unpack_rgss: expected the 5 stage-1 feature planes [normal 3, depth, depth^2]")
        out = torch.empty((6, H, W), dtype=torch.float32, device=dev)
        N.check(N.lib.svgir_unpack_rgss_forward(W, H, nc.data_ptr(), op.data_ptr(), de.data_ptr(), fe.data_ptr(), out.data_ptr(),
                                                N.stream_ptr(dev)), "unpack_rgss")
        ctx.save_for_backward(nc, op, de, fe)
        return out

    @staticmethod
    def backward(ctx, g):
        nc, op, de, fe = ctx.saved_tensors
        dev = op.device
        H, W = op.shape[-2], op.shape[-1]
        g = N.f32c(g, dev)
        d_op, d_de, d_fe = torch.empty_like(op), torch.empty_like(de), torch.empty_like(fe)
        N.check(N.lib.svgir_unpack_rgss_backward(W, H, nc.data_ptr(), op.data_ptr(), de.data_ptr(), fe.data_ptr(), g.data_ptr(),
                                                 d_op.data_ptr(), d_de.data_ptr(), d_fe.data_ptr(), N.stream_ptr(dev)), "unpack_rgss_backward")
        return None, d_op, d_de, d_fe


def pack_rgss(means3D, geo_normals, viewmatrix):
    return _PackRgss.apply(means3D, geo_normals, viewmatrix)


def unpack_rgss(rendered):
    """render.py:107-135.  `rendered` = the rgss rasterizer's 11-tuple; returns the reference's result dict entries that are
    derived in image space."""
    (num_rendered, num_contrib, image, normal, opacity, depth, feature, pseudo_normal, surface_xyz, weights, radii) = rendered
    planes = _UnpackRgss.apply(num_contrib, opacity, depth, feature)
    return dict(render=image, opacity=opacity, depth=depth, depth_var=planes[5:6], normal=normal, feature_normal=planes[0:3],
                feature_depth=planes[3:4], surface_xyz=surface_xyz, visibility_filter=radii > 0, radii=radii,
                num_rendered=num_rendered, num_contrib=num_contrib, weights=weights)


N.lib.svgir_depth2normal_backward.restype = C.c_int
N.lib.svgir_depth2normal_backward.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float,
                                             C.c_float, C.c_void_p, C.c_void_p]


class _Depth2Normal(torch.autograd.Function):
    """svgir_depth2normal / svgir_depth2normal_backward: differentiable w.r.t. the depth like the reference's function (the
    stage-1 loss uses the pseudo normal without detaching, gaussian_renderer/render.py:158-160)."""

    @staticmethod
    def forward(ctx, depth, mask, fovx, fovy, px, py):
        dev = depth.device
        d, m = N.f32c(depth.detach(), dev), N.f32c(mask.to(torch.float32), dev)
        H, W = d.shape[-2], d.shape[-1]
        out = N.out_tensor((3, H, W), torch.float32, dev)
        with torch.cuda.device(dev):
            N.check(N.lib.svgir_depth2normal(W, H, d.data_ptr(), m.data_ptr(), fovx, fovy, px, py, out.data_ptr(), N.stream_ptr(dev)),
                    "depth2normal")
        ctx.save_for_backward(d, m)
        ctx.cam = (fovx, fovy, px, py, tuple(depth.shape))
        return out

    @staticmethod
    def backward(ctx, g):
        d, m = ctx.saved_tensors
        fovx, fovy, px, py, shape = ctx.cam
        dev = d.device
        H, W = d.shape[-2], d.shape[-1]
        gd = N.out_tensor((H, W), torch.float32, dev)
        with torch.cuda.device(dev):
            N.check(N.lib.svgir_depth2normal_backward(W, H, d.data_ptr(), m.data_ptr(), N.f32c(g, dev).data_ptr(), fovx, fovy, px, py,
                                                      gd.data_ptr(), N.stream_ptr(dev)), "depth2normal_backward")
        return gd.reshape(shape), None, None, None, None, None


def depth2normal(depth, mask, fovx, fovy, prcppoint=(0.5, 0.5)):
    """utils/image_utils.py:61-125 as one HIP kernel per direction: depth, mask [1,H,W] -> pseudo normal [3,H,W],
    differentiable w.r.t. `depth` (pass `depth.detach()` where the reference detaches, svgss.py:345)."""
    return _Depth2Normal.apply(depth, mask, float(fovx), float(fovy), float(prcppoint[0]), float(prcppoint[1]))


def unpack(rendered, bg_color, is_training):
    """svgss.py:188-246.  `rendered` = the rasterizer's 9-tuple; returns the result dict of the reference."""
    (num_rendered, image, normal, opacity, depth, feature, vfeature, weights, radii) = rendered
    planes = _Unpack.apply(opacity, feature, vfeature, bg_color, bool(is_training))
    res = {k: planes[3 * i:3 * i + 3] for i, k in enumerate(TRAIN_PLANES if is_training else EVAL_PLANES)}
    res.update(render=image, depth=depth, opacity=opacity, visibility_filter=radii > 0, radii=radii,
               num_rendered=num_rendered, weights=weights)
    return res


def _host_f32(x, shape, what, who="environment_backdrop"):
    """A small camera / transform matrix as a contiguous fp32 numpy array (tensors on the GPU are copied to the host)."""
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    if a.shape not in shape:
        raise RuntimeError(f"{who}: {what} must have shape {' or '.join(str(s) for s in shape)}, got {a.shape}")
    return a


def _backdrop_camera(who, intrinsics, c2w, image, opacity, vfeature):
    """The checks both backdrops share: (device, {fx, fy, cx, cy}, c2w[:3,:3]) as the C arrays of the call."""
    dev = image.device
    if dev.type != "cuda" or opacity.device.type != "cuda" or vfeature.device.type != "cuda":
        raise RuntimeError(f"{who}: tensors must live on the GPU (libsvgir_raster.so has no CPU path)")
    K = _host_f32(intrinsics, ((3, 3),), "intrinsics", who)
    R = _host_f32(c2w, ((4, 4), (3, 3)), "c2w", who)[:3, :3]
    return dev, (C.c_float * 4)(K[0, 0], K[1, 1], K[0, 2], K[1, 2]), (C.c_float * 9)(*R.reshape(-1))


def _backdrop_planes(who, dev, image, opacity, vfeature):
    """(image, opacity, vfeature as contiguous fp32, H, W, the poisoned [9,H,W] result) -- the planes' shape check of both backdrops."""
    im, op, vf = (N.f32c(t.detach(), dev) for t in (image, opacity, vfeature))
    H, W = im.shape[-2], im.shape[-1]
    if im.numel() != 3 * H * W or op.numel() != H * W or vf.dim() != 3 or vf.shape[0] < 3 or tuple(vf.shape[1:]) != (H, W):
        raise RuntimeError(f"{who}: expected image [3,H,W], opacity [1,H,W], vfeature [>=3,H,W], got "
                           f"{tuple(image.shape)}, {tuple(opacity.shape)}, {tuple(vfeature.shape)}")
    return im, op, vf, H, W, N.out_tensor((9, H, W), torch.float32, dev)


def environment_backdrop(light, intrinsics, c2w, image, opacity, vfeature):
    """svgss.py:255-260 as one HIP kernel (csrc/backdrop.hip): the light looked up along the camera's world-space pixel directions
    (`Camera.get_world_directions`) and the three images the eval branch builds from it.
    light: DirectLightMap-like (.env) or EnvLight-like (.envmap [, .transform]), as for the shading (shading._env_of);
    intrinsics [3,3] (`Camera.intrinsics`: fx, fy, cx, cy in pixels), c2w [4,4] or [3,3] (`Camera.c2w`): tensors or arrays, read on
    the host; image [3,H,W], opacity [1,H,W], vfeature [>= 3,H,W]: the rasterizer's raw outputs (its first three vfeature planes are
    the pbr).  Returns {env_only, render_env, pbr_env}: [3,H,W] views of one buffer; they never require grad (the reference runs
    this tail under no_grad)."""
    shading._no_sg(light, "environment_backdrop")   # (this kernel samples the lat-long texture; an SG light: sg_environment_backdrop)
    dev, intr, rot = _backdrop_camera("environment_backdrop", intrinsics, c2w, image, opacity, vfeature)
    src = getattr(light, "env", getattr(light, "envmap", None))
    if torch.is_tensor(src) and src.device.type != "cuda":
        raise RuntimeError("environment_backdrop: the light must live on the GPU (libsvgir_raster.so has no CPU path)")
    with torch.no_grad(), torch.cuda.device(dev):
        env, softplus, scale, transform = shading._env_of(light)
        tr = None if transform is None else (C.c_float * 9)(*_host_f32(transform, ((3, 3),), "the light's transform").reshape(-1))
        env = N.f32c(env.detach(), dev)
        env = env.reshape((-1,) + tuple(env.shape[-3:]))[0]
        if env.shape[-1] != 3:
            raise RuntimeError(f"environment_backdrop: the environment map must have 3 channels, got {tuple(env.shape)}")
        im, op, vf, H, W, out = _backdrop_planes("environment_backdrop", dev, image, opacity, vfeature)
        work = torch.empty((env.shape[0] * env.shape[1], 4), dtype=torch.float32, device=dev)
        N.check(N.lib.svgir_env_backdrop(W, H, intr, rot, tr, env.data_ptr(), env.shape[0], env.shape[1], int(softplus), float(scale),
                                         work.data_ptr(), im.data_ptr(), op.data_ptr(), vf.data_ptr(), out.data_ptr(),
                                         N.stream_ptr(dev)), "env_backdrop")
    return dict(env_only=out[0:3], render_env=out[3:6], pbr_env=out[6:9])


def sg_environment_backdrop(light, intrinsics, c2w, image, opacity, vfeature):
    """environment_backdrop under a DirectLightSG-like light (`.lgtSGs` [M,7]; svgir_env_backdrop_sg): the unclamped mixture of lobes
    evaluated along the same pixel directions (no lookup transform: DirectLightSG.direct_light ignores it), the same three images, the
    same argument checks and return dict."""
    who = "sg_environment_backdrop"
    if not shading._is_sg(light):
        raise TypeError(f"{who}: the light must expose .lgtSGs (DirectLightSG); a texture light goes through environment_backdrop")
    dev, intr, rot = _backdrop_camera(who, intrinsics, c2w, image, opacity, vfeature)
    if light.lgtSGs.device.type != "cuda":
        raise RuntimeError(f"{who}: the light must live on the GPU (libsvgir_raster.so has no CPU path)")
    with torch.no_grad(), torch.cuda.device(dev):
        lt, keep = shading._sg_light(shading.SGLobes(light.lgtSGs).lobes, dev)
        im, op, vf, H, W, out = _backdrop_planes(who, dev, image, opacity, vfeature)
        N.check(N.lib.svgir_env_backdrop_sg(W, H, intr, rot, lt, im.data_ptr(), op.data_ptr(), vf.data_ptr(), out.data_ptr(),
                                            N.stream_ptr(dev)), "env_backdrop_sg")
    return dict(env_only=out[0:3], render_env=out[3:6], pbr_env=out[6:9])


def camera_of(sc):
    """The `camera` argument of render_svgss_view for a runner.to_torch() (or numpy) scene, by the reference's formulas:
    `Camera.get_intrinsics` (scene/cameras.py:116-130, fx is None: focal = size / (2 tan(FoV / 2)), principal point at the image
    centre) and `Camera.c2w` = the inverse of the view matrix (:81; sc["viewmatrix"] is the transposed world_view_transform)."""
    W, H = int(sc["W"]), int(sc["H"])
    K = np.array([[W / (2.0 * float(sc["tanfovx"])), 0.0, W / 2.0], [0.0, H / (2.0 * float(sc["tanfovy"])), H / 2.0], [0.0, 0.0, 1.0]])
    vm = sc["viewmatrix"]
    vm = vm.detach().cpu().numpy() if torch.is_tensor(vm) else np.asarray(vm)
    c2w = np.linalg.inv(vm.astype(np.float64).T)
    return dict(intrinsics=torch.from_numpy(K.astype(np.float32)), c2w=torch.from_numpy(c2w.astype(np.float32)))


def _with_backdrop(res, rendered, light, is_training, camera):
    if camera is not None and not is_training:
        backdrop = sg_environment_backdrop if shading._is_sg(light) else environment_backdrop
        res.update(backdrop(light, camera["intrinsics"], camera["c2w"], rendered[1], rendered[3], rendered[6]))
    return res


def render_svgss_view(sc, mat, light, is_training, fused=False, camera=None):
    """sc: runner.to_torch() scene (geometry + camera); mat: dict with base_color [P,12], roughness [P,4], normals
    [P,4,3], viewdirs [P,3], radiance / dirs [P,Ns,3], visibility / areas [P,Ns,1]; light: DirectLightMap-like (.env).
    Returns (results dict, means2D gradient carrier).  fused=True: the shading runs inside the rasterizer calls, for the surfels
    the view reads only (shading.render_shaded); same results.
    camera: dict(intrinsics=[3,3], c2w=[4,4] or [3,3]) (camera_of(sc) derives it from the scene); with is_training=False the results
    gain the eval branch's env_only, render_env and pbr_env (environment_backdrop, from the rasterizer's raw image, opacity and
    vfeature).  None: no backdrop, the results are what they are without this argument."""
    means2D = torch.zeros_like(sc["means3D"], requires_grad=torch.is_grad_enabled())
    if fused:
        rendered, _ = shading.render_shaded(runner.settings(sc, "svgss"), sc["means3D"], means2D, sc["opacities"], sc["shs"],
                                            sc["scales"], sc["rotations"], mat["base_color"], mat["roughness"], mat["normals"],
                                            mat["viewdirs"], mat["radiance"], light, mat["visibility"], mat["dirs"], mat["areas"],
                                            is_training)
        return _with_backdrop(unpack(rendered, sc["bg"], is_training), rendered, light, is_training, camera), means2D
    feats, vfeats, _ = shading.shade_and_pack(mat["base_color"], mat["roughness"], mat["normals"], mat["viewdirs"],
                                              mat["radiance"], light, mat["visibility"], mat["dirs"], mat["areas"],
                                              sc["viewmatrix"], is_training)
    rast = GaussianRasterizer(runner.settings(sc, "svgss"))
    rendered = rast(means3D=sc["means3D"], means2D=means2D, opacities=sc["opacities"], shs=sc["shs"],
                    scales=sc["scales"], rotations=sc["rotations"], features=feats, vfeatures=vfeats)
    return _with_backdrop(unpack(rendered, sc["bg"], is_training), rendered, light, is_training, camera), means2D
