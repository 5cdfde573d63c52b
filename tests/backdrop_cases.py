"""The table of environment-backdrop cases (csrc/backdrop.hip, svgir_harness.render_view.environment_backdrop) and its oracle in two
forms, shared by tests/test_backdrop_edge_inputs.py (CPU: pins the oracle, proves the table) and tests/test_gpu_backdrop.py.

  * oracle64(case): fp64, composed from the pinned restatements so.env_lookup, eo.rgb_to_srgb, eo.resample_bilinear;
  * reference32(case): the reference's own operation order in torch fp32 (scene/cameras.py:96-108, scene/direct_light_map.py:70-83,
    scene/envmap.py:54-73, gaussian_renderer/svgss.py:188-189, 258-260), so that E32(case, output) = max |fp32 - fp64|, the error
    the reference's arithmetic itself makes on the case, is known and the kernel can be held to a multiple of it.
Both clamp d.z to [-1, 1] before the acos, as the kernel does (the reference does not: a unit vector rounded to |z| = 1 + ulp is NaN
there; no case of this table produces one, see test_backdrop_edge_inputs.py).

Every shape is the smallest at which the kernel can go wrong: 1 x 1, 1 x W, H x 1, 37 x 53 (partial 256-thread blocks, odd on both
axes), 40 x 56 (the fixtures' size); maps of 1 x 2, 2 x 4, 8 x 16, 32 x 64 resampled from 48 x 96, 256 x 512.  Builders are seeded; the
arrays are read-only and built once (cases() is cached).

Threshold pixels are conditions, not measurements (condition_masks):
  seam  fp64 direction with d.x < 0 and |d.y| <= 1e-6: three products of unit-bounded terms carry ~8 eps32, so theta may come out as
        +pi or -pi; such a pixel may match either alternative (oracle64(case, seam=+1 / -1)).
  pole  d.x^2 + d.y^2 <= 1e-12: the azimuth is undetermined; the pixel is held to finiteness and to the value range of the env rows at
        that pole (pole_range), 0 included where a row is padding.
  inf   (the +inf case) a tap coordinate within 1e-4 of an integer: a zero weight meets the inf texel or not.
"""
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import epilogue_oracle as eo
from oracle import shading_oracle as so

OUTPUTS = ("env_only", "render_env", "pbr_env")
EPS32 = float(np.finfo(np.float32).eps)
SEAM_Y = 1e-6
POLE_R2 = 1e-12
INF_TAP = 1e-4
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Light:
    """DirectLightMap-like (.env [1,He,We,3]: softplus, x 2) or EnvLight-like (.envmap [Hs,Ws,3] -> 32 x 64, optional .transform)."""

    def __init__(self, kind, tex, transform=None):
        if kind == "dlm":
            self.env = tex
        else:
            self.envmap = tex
            self.transform = transform


def _ro(a, dtype=np.float32):
    a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
    a.setflags(write=False)
    return a


def _rotation(rng):
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] *= -1
    return Q


def _K(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float64)


def _planes(rng, H, W):
    """Generic rasterizer planes: image in [0,1], opacity in (0,1) with a few exact 0 / 1, vfeature (pbr) planes in [0, 1.2]."""
    op = rng.random((1, H, W))
    flat = op.reshape(-1)
    flat[:: 7] = 0.0
    flat[3:: 11] = 1.0
    return rng.random((3, H, W)), op, 1.2 * rng.random((3, H, W))


def _case(name, seed, H, W, K, R, kind, tex, T=None, planes=None, saturates=False, pole=None, seam_row=None, inf=False):
    rng = np.random.default_rng(seed)
    im, op, vf = planes(rng, H, W) if planes else _planes(rng, H, W)
    return dict(name=name, H=H, W=W, K=_ro(K), R=_ro(R), T=None if T is None else _ro(T), kind=kind, tex=_ro(tex), image=_ro(im),
                opacity=_ro(op), vfeature=_ro(vf), saturates=saturates, pole=pole, seam_row=seam_row, inf=inf)


def _dlm(rng, He, We, lo=-6.0, hi=0.0):
    return lo + (hi - lo) * rng.random((1, He, We, 3))


def _hdr(rng, Hs=48, Ws=96):
    return 2.0 * rng.random((Hs, Ws, 3)) ** 2


def _edge_planes(rng, H, W):
    """Opacity 0, 1e-6 (below the 1e-5 clamp), 1 - 1e-6, NaN, 1 and ordinary values, interleaved; pbr planes log-uniform over
    [1e-5, 3]: both sides of the sRGB knee (0.0031308) and above 1."""
    op = rng.random((1, H, W))
    flat = op.reshape(-1)
    for k, v in enumerate((0.0, 1e-6, 1.0 - 1e-6, np.nan, 1.0)):
        flat[k:: 9] = v
    vf = np.exp(rng.uniform(math.log(1e-5), math.log(3.0), (3, H, W)))
    return rng.random((3, H, W)), op, vf


@functools.lru_cache(maxsize=None)
def cases():
    g = np.load(os.path.join(GOLD, "render_view.npz"))
    rng = np.random.default_rng(4242)
    out = []
    # the fixture's camera (a generic rotation, focal lengths from the fields of view)
    out.append(_case("fixture_camera_8x16", 1, 40, 56, g["cam_intrinsics"], g["cam_c2w"][:3, :3], "dlm", _dlm(rng, 8, 16)))
    # identity rotation, integer principal point: pixel (cy, cx) looks exactly along +z (the padded row above the map), and the same
    # looking down -z (the last two rows); the half row left of it has d.y = 0, d.x < 0 exactly: theta = pi
    out.append(_case("pole_plus_z_2x4", 2, 37, 53, _K(40, 40, 26, 18), np.eye(3), "dlm", _dlm(rng, 2, 4), pole=(18, 26), seam_row=(18, 26)))
    out.append(_case("pole_minus_z_8x16", 3, 37, 53, _K(40, 40, 26, 18), np.diag([1.0, -1.0, -1.0]), "dlm", _dlm(rng, 8, 16), pole=(18, 26),
                     seam_row=(18, 26)))
    # the camera looks along world -x (tilted in the x-z plane), its y axis is world y: the pixel row v = cy has d.y = 0, d.x < 0
    b = 0.3
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    P = np.array([[0.0, 0, -1], [0, 1, 0], [1, 0, 0]])     # cam z -> world -x, cam x -> world z
    out.append(_case("seam_row_32x64", 4, 37, 53, _K(45, 45, 26.5, 18), Ry @ P, "el", _hdr(rng), seam_row=(18, 53)))
    out.append(_case("principal_point_off_centre_fx_ne_fy", 5, 40, 56, _K(61.5, 48.25, 19.75, 26.5), _rotation(rng), "el", _hdr(rng)))
    out.append(_case("principal_point_outside", 6, 37, 53, _K(50, 50, -12.5, 60.25), _rotation(rng), "dlm", _dlm(rng, 8, 16)))
    out.append(_case("lookup_transform", 7, 40, 56, _K(70, 66, 28, 20), _rotation(rng), "el", _hdr(rng), T=_rotation(rng)))
    out.append(_case("one_pixel_1x2", 8, 1, 1, _K(1.5, 1.5, 0.25, 0.5), _rotation(rng), "dlm", _dlm(rng, 1, 2)))
    out.append(_case("one_row_2x4", 9, 1, 53, _K(30, 30, 26.5, 0.5), _rotation(rng), "dlm", _dlm(rng, 2, 4)))
    out.append(_case("one_column_8x16", 10, 37, 1, _K(30, 30, 0.5, 18.5), _rotation(rng), "dlm", _dlm(rng, 8, 16)))
    out.append(_case("noise_map_256x512", 11, 37, 53, _K(40, 40, 26.5, 18.5), _rotation(rng), "dlm", _dlm(rng, 256, 512)))
    out.append(_case("opacity_and_knee_edges", 12, 37, 53, _K(40, 40, 26.5, 18.5), _rotation(rng), "dlm", _dlm(rng, 8, 16), planes=_edge_planes))
    out.append(_case("flat_env", 13, 37, 53, _K(40, 40, 26.5, 18.5), _rotation(rng), "dlm", np.full((1, 8, 16, 3), -1.0)))
    tex = _dlm(rng, 8, 16)
    tex[0, 3, 5, 1] = np.inf
    out.append(_case("inf_texel", 14, 37, 53, _K(14, 14, 26.5, 18.5), _rotation(rng), "dlm", tex, inf=True))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fixture_cases():
    """((case, {output: the reference's recorded array}), ...): the reference's own eval render_view runs -- the four camera / light
    combinations of golden/backdrop.npz (scripts/make_golden_backdrop.py) and the eval view of golden/render_view.npz (whose light
    saturates the sRGB clip: env_only is 1.0 everywhere there)."""
    b, g = np.load(os.path.join(GOLD, "backdrop.npz")), np.load(os.path.join(GOLD, "render_view.npz"))
    out = []
    for cam, lname in (("fov", "dlm"), ("pin", "el"), ("pin", "elt"), ("fov", "elt")):
        kind, tex = ("dlm", b["dlm_env"]) if lname == "dlm" else ("el", b["el_envmap"])
        c = dict(name=f"backdrop_npz_{cam}_{lname}", H=40, W=56, K=_ro(b[cam + "_intrinsics"]), R=_ro(b[cam + "_c2w"][:3, :3]),
                 T=_ro(b["elt_transform"]) if lname == "elt" else None, kind=kind, tex=_ro(tex), image=_ro(b["raster_image"]),
                 opacity=_ro(b["raster_opacity"]), vfeature=_ro(b["raster_vfeature"]), saturates=False, pole=None, seam_row=None, inf=False)
        out.append((c, {k: b[f"{cam}_{lname}_{k}"] for k in OUTPUTS}))
    c = dict(name="render_view_npz_eval", H=40, W=56, K=_ro(g["cam_intrinsics"]), R=_ro(g["cam_c2w"][:3, :3]), T=None, kind="dlm",
             tex=_ro(g["env"]), image=_ro(g["eval_raster_image"]), opacity=_ro(g["eval_raster_opacity"]),
             vfeature=_ro(g["eval_raster_vfeature"][:3]), saturates=True, pole=None, seam_row=None, inf=False)
    out.append((c, {k: g["eval_res_" + k] for k in OUTPUTS}))
    return tuple(out)


def case_ids():
    return [c["name"] for c in cases()]


def light_of(case, device=None):
    t = lambda a: torch.from_numpy(np.array(a)).to(device or "cpu")  # noqa: E731  (a copy: the table stays read-only)
    return Light(case["kind"], t(case["tex"]), None if case["T"] is None else t(case["T"]))


# ---- fp64 oracle ---------------------------------------------------------------------------------------------------------------
def directions64(case):
    """[H,W,3] fp64 lookup directions (camera direction, rotated, through the light's transform, z clamped), from the fp32 camera."""
    H, W = case["H"], case["W"]
    K, R = case["K"].astype(np.float64), case["R"].astype(np.float64)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], 0)
    d = d / np.maximum(np.linalg.norm(d, axis=0, keepdims=True), 1e-12)
    d = (R @ d.reshape(3, -1))
    if case["T"] is not None:
        d = case["T"].astype(np.float64) @ d
    d = d.T.reshape(H, W, 3).copy()
    d[..., 2] = np.clip(d[..., 2], -1.0, 1.0)
    return d


def env64(case):
    """(texture fp64 [He,We,3] BEFORE f, softplus flag, scale) the lookup samples."""
    if case["kind"] == "dlm":
        return case["tex"].astype(np.float64)[0], True, 2.0
    return eo.resample_bilinear(case["tex"], 32, 64), False, 1.0


def tap_coords64(case, d=None):
    """fp64 (x, y) texel coordinates of every pixel's lookup [H,W]."""
    d = directions64(case) if d is None else d
    tex, _, _ = env64(case)
    He, We = tex.shape[:2]
    phi = np.arccos(d[..., 2]) - 1e-6
    theta = np.arctan2(d[..., 1], d[..., 0])
    return (-theta / math.pi + 1) * 0.5 * (We - 1), (phi / math.pi * 2 - 1 + 1) * 0.5 * (He - 1)


def condition_masks(case):
    """dict of [H,W] bool masks: seam, pole, inf (see the module docstring)."""
    d = directions64(case)
    seam = (d[..., 0] < 0) & (np.abs(d[..., 1]) <= SEAM_Y)
    pole = d[..., 0] ** 2 + d[..., 1] ** 2 <= POLE_R2
    inf = np.zeros_like(seam)
    if case["inf"]:
        x, y = tap_coords64(case, d)
        inf = (np.abs(x - np.round(x)) <= INF_TAP) | (np.abs(y - np.round(y)) <= INF_TAP)
    return dict(seam=seam & ~pole, pole=pole, inf=inf)


def _compose64(case, env):
    """The three images [3,H,W] fp64 from the looked-up light env [H,W,3] (svgss.py:188-189, 258-260)."""
    env = env.transpose(2, 0, 1)
    op = case["opacity"].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        pbr = case["vfeature"].astype(np.float64)[:3] / np.maximum(op, eo.OPACITY_MIN)
        s = eo.rgb_to_srgb(env)
        return dict(env_only=s, render_env=case["image"].astype(np.float64) + (1 - op) * s, pbr_env=eo.rgb_to_srgb(pbr * op + (1 - op) * env))


def oracle64(case, seam=0):
    """dict of the three images, fp64.  seam = +1 / -1: the alternative in which every seam pixel's d.y is +|d.y| / -|d.y|
    (theta = +pi / -pi side)."""
    d = directions64(case)
    if seam:
        m = condition_masks(case)["seam"]
        d[..., 1] = np.where(m, math.copysign(1.0, seam) * np.abs(d[..., 1]), d[..., 1])
    tex, softplus, scale = env64(case)
    with np.errstate(invalid="ignore", over="ignore"):
        env = so.env_lookup(torch.from_numpy(tex), torch.from_numpy(d), softplus=softplus, scale=scale).numpy()
    return _compose64(case, env)


def pole_range(case):
    """{output: (lo, hi) [3] fp64} at the case's pole pixel: the images composed from the smallest / largest light the two env rows
    around the pole's latitude can give (f(texel) * scale over the whole row; 0 where the row is padding)."""
    py, px = case["pole"]
    tex, softplus, scale = env64(case)
    He = tex.shape[0]
    _, y = tap_coords64(case)
    rows = sorted({int(math.floor(y[py, px] + s)) + k for s in (-1e-3, 1e-3) for k in (0, 1)})
    f = F.softplus(torch.from_numpy(tex)).numpy() if softplus else tex
    vals = [f[r].reshape(-1, 3) * scale if 0 <= r < He else np.zeros((1, 3)) for r in rows]
    vals = np.concatenate(vals, 0)
    one = dict(case, H=1, W=1, image=case["image"][:, py:py + 1, px:px + 1], opacity=case["opacity"][:, py:py + 1, px:px + 1],
               vfeature=case["vfeature"][:, py:py + 1, px:px + 1])
    lo, hi = _compose64(one, vals.min(0).reshape(1, 1, 3)), _compose64(one, vals.max(0).reshape(1, 1, 3))
    return {k: (np.minimum(lo[k], hi[k]).reshape(3), np.maximum(lo[k], hi[k]).reshape(3)) for k in OUTPUTS}


# ---- the reference's fp32 operation order --------------------------------------------------------------------------------------
def _srgb32(img):
    img = torch.where(img > 0.0031308, torch.pow(torch.max(img, torch.tensor(0.0031308)), 1.0 / 2.4) * 1.055 - 0.055, 12.92 * img)
    return torch.clamp(img, 0.0, 1.0)


def directions32(case):
    """[H*W,3] torch fp32: `Camera.get_world_directions` in the reference's operation order (before the light's transform, unclamped)."""
    H, W = case["H"], case["W"]
    K, R = torch.from_numpy(np.array(case["K"])), torch.from_numpy(np.array(case["R"]))
    v, u = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    d = torch.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], torch.ones_like(u)], dim=0)
    d = F.normalize(d, dim=0)
    d = (R @ d.reshape(3, -1)).reshape(3, H, W)
    return d.permute(1, 2, 0).reshape(-1, 3)


def lookup_dirs32(case):
    """directions32 through the light's transform (EnvLight: dirs @ transform.T), still unclamped."""
    dirs = directions32(case)
    return dirs if case["T"] is None else dirs @ torch.from_numpy(np.array(case["T"])).T


def reference32(case):
    """dict of the three images as fp32 numpy arrays, computed the way the reference computes them (torch fp32 on the CPU)."""
    H, W = case["H"], case["W"]
    dirs = lookup_dirs32(case)
    tex = torch.from_numpy(np.array(case["tex"]))
    if case["kind"] == "dlm":
        envir_map, scale = F.softplus(tex).permute(0, 3, 1, 2), 2.0
    else:
        envir_map = F.interpolate(tex.permute(2, 0, 1).unsqueeze(0), size=(32, 64), mode="bilinear", align_corners=False)
        scale = 1.0
    phi = torch.arccos(dirs[:, 2].clamp(-1.0, 1.0)) - 1e-6
    theta = torch.atan2(dirs[:, 1], dirs[:, 0])
    query_y = (phi / np.pi) * 2 - 1
    query_x = -theta / np.pi
    grid = torch.stack((query_x, query_y)).permute(1, 0).unsqueeze(0).unsqueeze(0)
    light = F.grid_sample(envir_map, grid, align_corners=True)[0, :, 0, :].permute(1, 0).reshape(H, W, 3) * scale
    env = light.permute(2, 0, 1)
    image, op, vf = (torch.from_numpy(np.array(case[k])) for k in ("image", "opacity", "vfeature"))
    pbr = vf[:3] / op.clamp_min(1e-5)
    res = dict(env_only=_srgb32(env), render_env=image + (1 - op) * _srgb32(env), pbr_env=_srgb32(pbr * op + (1 - op) * env))
    return {k: t.numpy() for k, t in res.items()}


def measured_mask(case):
    """[H,W] bool: pixels that are measurements (no condition applies)."""
    m = condition_masks(case)
    return ~(m["seam"] | m["pole"] | m["inf"])


@functools.lru_cache(maxsize=None)
def _tables(name):
    case = next(c for c in cases() + tuple(fc for fc, _ in fixture_cases()) if c["name"] == name)
    o64, r32, meas = oracle64(case), reference32(case), measured_mask(case)
    e32, bound = {}, {}
    for k in OUTPUTS:
        a, b = o64[k], r32[k].astype(np.float64)
        ok = np.isfinite(a) & np.isfinite(b) & meas[None]
        e32[k] = float(np.abs(a - b)[ok].max()) if ok.any() else 0.0
        fin = np.isfinite(a)
        bound[k] = 4.0 * e32[k] + 16.0 * EPS32 * max(1.0, float(np.abs(a[fin]).max()) if fin.any() else 0.0)
    for v in o64.values():
        v.setflags(write=False)
    return o64, r32, e32, bound


def shared_oracle(case):
    """(oracle64, reference32, E32, bound) of a case, computed once and shared (read-only): bound[output] =
    4 E32 + 16 eps32 max(1, max |oracle|) -- the floor covers the at most 16 fp32 roundings between a texel and an output and matters
    where E32 is 0 (the flat env)."""
    return _tables(case["name"])
