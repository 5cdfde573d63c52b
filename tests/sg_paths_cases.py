"""The case tables and oracles of the three paths of the spherical-Gaussian light around the shading: the gradient of the bare light
(svgir_sg_eval_backward), the eval view's backdrop (svgir_env_backdrop_sg) and the fused radiance-consistency loss
(svgir_radiance_loss_forward_sg / _backward_sg).  Shared by tests/test_sg_paths_edge_inputs.py (CPU: the oracles are pinned by the
reference's recordings, every case holds what it is named for, what fp32 loses is measured) and tests/test_gpu_sg_paths.py (the kernels).

Everything is composed from the existing tables:
    A  sg_light_cases.sg_light / sg_grad (the contract of include/svgir_raster.h in torch) + `sg_dirs_grad`, the closed form of dL/ddirs;
       G32 per case = the largest per-row error (shading_cases.row_err) of the same arithmetic in torch fp32 against fp64.
    B  backdrop_cases.directions64 / _compose64 with env = sg_light(lobes, d); reference32 = backdrop_cases.directions32 + the fp32 light +
       the reference's composition lines, which gives E32 and the bound 4 E32 + 16 eps32 max(1, max |oracle|).  Pixels whose sRGB argument
       lies within 1e-4 max(|b|, 0.1) of the knee b = 0.0031308 or of the clip b = 1 are threshold pixels (finiteness only).
    C  radiance_loss_cases' geometry, selection and bound with the light replaced: envmap = sg_light(lobes64, ray_d) * areas, and
       d_lobes = sg_grad(lobes, ray_d, d_envmap * areas); the `_abs` sums go through |.| of the same formulas.  E_SG, the relative
       deviation of one fp32 light value, takes E_ENV's place in the bound.

All inputs are fp32-representable.  `rl_case(name)` / `rl_oracle(name)` cache per process; the arrays are read-only."""
import functools
import math

import numpy as np
import torch

import backdrop_cases as bc
import sg_light_cases as sg
import shading_cases as sc
from tests import radiance_cases as rc
from tests import radiance_loss_cases as lc

F32, F64 = np.float32, np.float64
FLT_MAX = float(np.finfo(np.float32).max)
# Measured 2026-10-20 over the table of C (test_sg_paths_edge_inputs.py measures it again and prints it per case): the largest
# |L32 - L64| / sum_m |mu_m| e_m is 1.85e-5 (`physical-M32`, 32 000 directions: |lambda| in the hundreds, and the exponent's argument |lambda| (d.a - 1)
# carries |lambda| eps32 of absolute error from the rounding of d.a alone; 1e-6 - 5e-6 in the small cases).
E_SG = 2.5e-5


def _f32(t):
    return t.float().double()


def lobes_of(M, seed, sharp=20.0):
    """[M,7] fp64, fp32-representable: the reference's initialisation with the sharpness of two lobes in three scaled to `sharp` instead of
    100 (lobes a random direction meets), as sg_light_cases.build."""
    g = torch.Generator().manual_seed(seed)
    lb = torch.randn(M, 7, generator=g, dtype=torch.float64)
    lb[:, 3] *= torch.where(torch.arange(M) % 3 == 2, 100.0, sharp)
    return _f32(lb)


# ---- A: the gradient of the bare light -----------------------------------------------------------------------------------------
def sg_dirs_grad(lobes, dirs, g):
    """The closed form dL/ddirs [n,3] = sum_m |lambda_m| s_m a_m, s_m = e_m sum_c |mu_mc| g_c (include/svgir_raster.h)."""
    xi, lam, mu = lobes[:, :3], lobes[:, 3].abs(), lobes[:, 4:].abs()
    a = xi / torch.sqrt((xi * xi).sum(-1, keepdim=True))
    d, g = dirs.reshape(-1, 3), g.reshape(-1, 3)
    s = torch.exp(lam * (d @ a.T - 1.0)) * (g @ mu.T)          # [n, M]
    return ((s * lam) @ a).reshape(dirs.shape)


def _eval_case(id, n, M, special=None):
    return dict(id=id, n=n, M=M, special=special)


EVAL_CASES = [
    _eval_case("n1-M1", 1, 1), _eval_case("n63-M5", 63, 5), _eval_case("n64-M32", 64, 32), _eval_case("n65-M33", 65, 33),
    _eval_case("n257-M128", 257, 128), _eval_case("n1200-M32", 1200, 32), _eval_case("n1200-M1", 1200, 1),
    _eval_case("signs-and-zeros", 257, 8, "signs"), _eval_case("sharp-on-axis", 65, 4, "sharp"),
    _eval_case("unnormalised-dirs", 257, 5, "unnormalised"), _eval_case("zero-upstream", 65, 5, "zero_up"),
]
EVAL_BY_ID = {c["id"]: c for c in EVAL_CASES}


@functools.lru_cache(maxsize=None)
def eval_build(id):
    """(lobes [M,7], dirs [n,3], up [n,3]) fp64, fp32-representable"""
    c = EVAL_BY_ID[id]
    n, M, sp = c["n"], c["M"], c["special"]
    g = torch.Generator().manual_seed(300 + 7 * n + M)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    unit = lambda v: v / v.norm(dim=-1, keepdim=True)  # noqa: E731
    lobes = lobes_of(M, 500 + n + M).clone()
    dirs = unit(rnd(n, 3))
    k = torch.arange(0, n, 3)
    dirs[k] = unit(unit(lobes[k % M, :3]) + 0.08 * rnd(len(k), 3))     # a third of the directions look into a lobe
    up = rnd(n, 3)
    if sp == "signs":       # sg_light_cases' rows: negative lambda and mu (the abs), lambda = 0, mu = 0 in one channel and in all, -0
        lobes[0, 3] = -abs(lobes[0, 3]); lobes[0, 4:] = -lobes[0, 4:].abs()
        lobes[1, 3] = 0.0
        lobes[2, 5] = 0.0
        lobes[3, 4:] = 0.0
        lobes[4, 4] = -0.0
    elif sp == "sharp":
        lobes[0] = torch.tensor([0.0, 0.0, 2.0, 1000.0, 0.7, 0.4, 0.9], dtype=torch.float64)     # a = +z exactly
        lobes[1] = torch.tensor([0.0, -3.0, 0.0, -1000.0, 0.2, 0.6, 0.3], dtype=torch.float64)   # a = -y exactly
        dirs[0] = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)      # on the axis: e = 1
        dirs[1] = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64)     # opposite: exp(-2000) underflows to 0
        dirs[2] = torch.tensor([0.0, -1.0, 0.0], dtype=torch.float64)
        dirs[3] = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    elif sp == "unnormalised":
        dirs = dirs * (0.4 + 1.2 * torch.rand(n, 1, generator=g, dtype=torch.float64))
        lobes[:, 3] = rnd(M) * 4.0      # (|d| up to 1.6: d.a - 1 up to +0.6)
    elif sp == "zero_up":
        up = torch.zeros_like(up)
    return _f32(lobes), _f32(dirs), _f32(up)


def eval_oracle(lobes, dirs, up, dtype=torch.float64):
    """(d_lobes [M,7], d_dirs [n,3]) by the closed forms in `dtype`"""
    lb, d, u = lobes.to(dtype), dirs.to(dtype), up.to(dtype)
    return sg.sg_grad(lb, d, u), sg_dirs_grad(lb, d, u)


def eval_g32(id):
    """(d_lobes64, d_dirs64, {d_lobes, d_dirs: G32})"""
    lobes, dirs, up = eval_build(id)
    l64, d64 = eval_oracle(lobes, dirs, up)
    l32, d32 = eval_oracle(lobes, dirs, up, torch.float32)
    return l64, d64, {"d_lobes": float(sc.row_err(l32, l64).max()), "d_dirs": float(sc.row_err(d32, d64).max())}


# ---- B: the backdrop -----------------------------------------------------------------------------------------------------------
SRGB_KNEE, SRGB_CLIP, SRGB_REL = 0.0031308, 1.0, 1e-4


def _view(name, seed, H, W, K, M, sharp=6.0, amp=0.1, planes=None):
    rng = np.random.default_rng(seed)
    c = bc._case(name, seed, H, W, K, bc._rotation(rng), "sg", np.zeros((1, 1, 1, 3)), planes=planes)
    lb = lobes_of(M, 900 + seed, sharp=sharp).clone()
    lb[:, 3] = lb[:, 3].clamp(-3 * sharp, 3 * sharp)     # wide lobes: the backdrop is not black between them
    lb[:, 4:] *= amp
    c["lobes"] = bc._ro(_f32(lb).numpy(), np.float64)
    return c


@functools.lru_cache(maxsize=None)
def views():
    return (
        _view("one_pixel_M1", 1, 1, 1, bc._K(1.5, 1.5, 0.25, 0.5), 1, amp=0.5),
        _view("17x13_M32_off_centre_fx_ne_fy", 2, 13, 17, bc._K(21.5, 17.75, 6.25, 8.5), 32, amp=0.1),
        _view("64x48_M128_principal_point_outside", 3, 48, 64, bc._K(50, 50, -12.5, 60.25), 128, amp=0.03),
        _view("17x13_M32_opacity_edges_and_knee", 4, 13, 17, bc._K(20, 20, 8.5, 6.5), 32, sharp=40.0, amp=0.006, planes=bc._edge_planes),
        _view("64x48_M1_above_one", 5, 48, 64, bc._K(40, 44, 30.5, 25.5), 1, sharp=1.0, amp=2.5, planes=bc._edge_planes),
    )


def view_ids():
    return [c["name"] for c in views()]


def view_light64(case):
    d = torch.from_numpy(bc.directions64(case))
    return sg.sg_light(torch.from_numpy(np.array(case["lobes"])), d).numpy()


def view_oracle64(case):
    return bc._compose64(case, view_light64(case))


def view_reference32(case):
    """the reference's lines in torch fp32 on the CPU: get_world_directions, render_envmap_sg (sg_light), svgss.py:188-189, 258-260"""
    H, W = case["H"], case["W"]
    dirs = bc.directions32(case)
    env = sg.sg_light(torch.from_numpy(np.array(case["lobes"])).float(), dirs).reshape(H, W, 3).permute(2, 0, 1)
    image, op, vf = (torch.from_numpy(np.array(case[k])) for k in ("image", "opacity", "vfeature"))
    pbr = vf[:3] / op.clamp_min(1e-5)
    res = dict(env_only=bc._srgb32(env), render_env=image + (1 - op) * bc._srgb32(env), pbr_env=bc._srgb32(pbr * op + (1 - op) * env))
    return {k: t.numpy() for k, t in res.items()}


def view_threshold(case):
    """{output: [3,H,W] bool}: the sRGB argument of the element lies within 1e-4 max(|b|, 0.1) of the knee or of the clip"""
    env = view_light64(case).transpose(2, 0, 1)
    op = case["opacity"].astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        pbr = case["vfeature"].astype(F64)[:3] / np.maximum(op, 1e-5)
        arg = dict(env_only=env, render_env=env, pbr_env=pbr * op + (1 - op) * env)
    near = lambda x: sum(np.abs(x - b) <= SRGB_REL * max(abs(b), 0.1) for b in (SRGB_KNEE, SRGB_CLIP)) > 0  # noqa: E731
    return {k: near(v) for k, v in arg.items()}


@functools.lru_cache(maxsize=None)
def view_tables(name):
    """(oracle64, reference32, E32, bound, threshold) of a view, computed once"""
    case = next(c for c in views() if c["name"] == name)
    o64, r32, thr = view_oracle64(case), view_reference32(case), view_threshold(case)
    e32, bound = {}, {}
    for k in bc.OUTPUTS:
        a, b = o64[k], r32[k].astype(F64)
        ok = np.isfinite(a) & np.isfinite(b) & ~thr[k]
        e32[k] = float(np.abs(a - b)[ok].max()) if ok.any() else 0.0
        fin = np.isfinite(a)
        bound[k] = 4.0 * e32[k] + 16.0 * bc.EPS32 * max(1.0, float(np.abs(a[fin]).max()) if fin.any() else 0.0)
    return o64, r32, e32, bound, thr


# ---- C: the fused loss ---------------------------------------------------------------------------------------------------------
def _rl(geometry, M, seed, **kw):
    return dict(geometry=geometry, M=M, seed=seed, **kw)


# every M once, every geometry once
RL_CASES = {
    "max_positions-M1": _rl("max_positions", 1, 1, sharp=2.0), "tie_3_70-M32": _rl("tie_3_70", 32, 2),
    "contention-M33": _rl("contention", 33, 3), "all_primaries_miss-M32": _rl("all_primaries_miss", 32, 4),
    "hits_out_of_range-M128": _rl("hits_out_of_range", 128, 5), "ratio_zero-M32": _rl("ratio_zero", 32, 6),
    "at_camera-M33": _rl("at_camera", 33, 7), "non_finite-M32": _rl("random_70x64", 32, 8, non_finite=True),
    "random_9x65-M128": _rl("random_9x65", 128, 9), "physical-M32": _rl("physical", 32, 10),
    # the SG backward's whole passes of 64 at the sample counts around them (one sample, one short of a pass, one past two passes), and a
    # backward that is not asked for d_radiance_ratio (ratio_grad=False: the ratio is no leaf)
    "self_hit_1x1-M1": _rl("self_hit_1x1", 1, 11), "random_5x63-M1": _rl("random_5x63", 1, 12), "random_5x129-M1": _rl("random_5x129", 1, 13),
    "random_5x65-M1-fixed_ratio": _rl("random_5x65", 1, 14, ratio_grad=False),
}
RL_NAMES = sorted(RL_CASES)
MAX_EXCLUDED = 0.05     # of the rows and of the lobes of a case


@functools.lru_cache(maxsize=None)
def rl_case(name):
    """the geometry of radiance_loss_cases under `lobes` [M,7]; the targets lie far from R -- radiances in [6, 8] on even rows (R < T) and 0
    on odd rows (R >= 0 = T; every term of R is >= 0, so R = sum |t| is many bounds away from 0 unless it is exactly 0) -- so that the sign
    of the L1 does not hang on rounding"""
    spec = RL_CASES[name]
    c = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in lc.case(spec["geometry"]).items()}
    for k in ("env", "softplus", "scale", "transform"):
        c.pop(k)
    N, S = c["N"], c["S"]
    rng = np.random.default_rng(4000 + spec["seed"])
    rad = rng.uniform(6.0, 8.0, size=(N, S, 3))
    rad[1::2] = 0.0
    lobes = lobes_of(spec["M"], 700 + spec["seed"], sharp=spec.get("sharp", 20.0)).numpy().copy()
    if spec.get("non_finite"):
        sel = lc.selection(lc.case(spec["geometry"]))[0]
        rad[2, sel[2]] = np.inf               # T = +inf in all channels of row 2
        rad[4, sel[4], 0] = np.nan            # nan_to_num: T = 0 in the red channel of row 4, which stays finite
        rad[6, sel[6], 2] = -np.inf
        # two constant lobes (lambda = 0: e = 1 in every direction) whose green amplitudes add up beyond FLT_MAX: L_g = +inf for every
        # sample in fp32 while every lobe is finite; the green channel of every row with a hit is non-finite, red and blue keep gradients
        lobes[0, 3] = lobes[1, 3] = 0.0
        lobes[0, 5] = lobes[1, 5] = 3.0e38
    if spec["geometry"] == "physical":
        # the traced scene's directions are not unit vectors (|d| up to 2; the brdf normalises them).  The light is evaluated along the RAW
        # direction and exp(|lambda| (d.a - 1)) at |d| = 2, |lambda| = 290 is beyond fp32: unit directions, as the reference's incident
        # directions are (radiance_loss_cases._base does the same for its own cases)
        d = c["ray_d"].astype(F64)
        c["ray_d"] = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F32)
    c.update(radiances=rad.astype(F32), lobes=np.ascontiguousarray(lobes, dtype=F32), ratio_grad=spec.get("ratio_grad", True))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def rl_light64(c):
    """(light [N,S,3], its magnitude sum_m |mu| e) in fp64; a value beyond FLT_MAX is what fp32 makes of it: inf"""
    lb, d = torch.from_numpy(c["lobes"].astype(F64)), torch.from_numpy(c["ray_d"].astype(F64))
    L = sg.sg_light(lb, d).numpy()
    return np.where(np.abs(L) > FLT_MAX, np.inf, L), L


def bound(kind, cnt, abs_sum):
    """radiance_loss_cases.bound with E_SG in E_ENV's place"""
    return (cnt * 2.0 ** -24 + 4.0 * (rc.E_TERM[kind] + E_SG)) * abs_sum


def kernel_case(c, sel, grad_out=None, clean=False):
    light, _ = rl_light64(c)
    envmap = light * c["areas"].astype(F64)[..., None]
    if clean:
        envmap = np.where(np.isfinite(envmap), envmap, 0.0)
    return dict(c, sample=np.asarray(sel, np.int32), envmap=envmap, grad_out=np.zeros((c["N"], 3)) if grad_out is None else grad_out)


def lobes_grad(c, d_envmap, dtype=torch.float64):
    """d_lobes [M,7] = sg_grad(lobes, ray_d, d_envmap * areas) in `dtype` (fp32: the same arithmetic, for G32)"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=F64)).to(dtype)  # noqa: E731
    return sg.sg_grad(t(c["lobes"]), t(c["ray_d"]), t(d_envmap * c["areas"].astype(F64)[..., None])).double().numpy()


def rl_oracle_at(c, sel):
    """radiance_loss_cases.oracle_at with the SG light: d_lobes (+ _abs: |.| of every term, i.e. sg_grad's sums over |g| with the signs and
    the projection dropped -- an upper bound of what is added per lobe; G32: the fp32 restatement's per-lobe error) instead of d_env, and
    `unsafe_lobes` [M]: lobes fed by rows whose |R - T| lies within 10 bounds of zero."""
    N, S = c["N"], c["S"]
    rows = np.arange(N)
    sel = np.asarray(sel, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        k1 = rc.oracle_of(kernel_case(c, sel))
        out, out_abs = k1["out"], k1["out_abs"]
        raw = c["radiances"].astype(F64)[rows, sel]
        prod = raw * float(c["radiance_ratio"].reshape(-1)[0])
        target = np.where(np.isnan(prod), 0.0, prod)
        bad = ~np.isfinite(out) | ~np.isfinite(target)
        gap = np.abs(out - target)
        sign = np.where(bad, 0.0, np.sign(out - target))
    g = sign / (3 * N)
    k2 = rc.oracle_of(kernel_case(c, sel, g, clean=True))
    row_bound = bound("out", S, np.where(np.isfinite(out_abs), out_abs, 0.0))
    hit_of = np.full(N, -1)
    hit_of[k2["rows"]] = k2["hits"]
    risky = (~bad & (gap <= 10 * row_bound) & (out_abs > 0)).any(1)
    unsafe = np.zeros(N, bool)
    unsafe[hit_of[risky & (hit_of >= 0)]] = True
    d_lobes = lobes_grad(c, k2["d_envmap"])
    d_lobes32 = lobes_grad(c, k2["d_envmap"], torch.float32)
    fed_by_unsafe = np.abs(lobes_grad(c, np.where(unsafe[:, None, None], k2["d_envmap_abs"], 0.0)))
    unsafe_lobes = (fed_by_unsafe > 1e-6 * np.maximum(np.abs(d_lobes), 1e-300)).any(1) if unsafe.any() else np.zeros(len(d_lobes), bool)
    fin = np.isfinite(prod) & ~bad
    t_ratio = np.where(fin, -g * np.where(fin, raw, 0.0), 0.0)
    ok = ~bad
    return rc._readonly(dict(
        sel=sel, out=out, out_abs=out_abs, target=target, bad=bad, gap=gap,
        loss=float("nan") if bad.any() else gap.sum() / (3 * N), loss_sum=gap[ok].sum(),
        loss_sum_bound=row_bound[ok].sum() + 2.0 ** -23 * (np.abs(out[ok]).sum() + np.abs(target[ok]).sum()),
        kernel=k2, d_lobes=d_lobes, G32=float(sc.row_err(torch.from_numpy(d_lobes32), torch.from_numpy(d_lobes)).max()),
        d_ratio=t_ratio.sum(), d_ratio_abs=np.abs(t_ratio).sum(), unsafe=unsafe, unsafe_lobes=unsafe_lobes,
        unsafe_ratio_abs=np.abs(t_ratio)[risky].sum()))


@functools.lru_cache(maxsize=None)
def rl_oracle(name):
    """rl_oracle_at under the fp64 selection (the geometry's own: the selection does not see the light), with margin, score, threshold"""
    c = rl_case(name)
    sel, margin, score = lc.selection(c)
    o = dict(rl_oracle_at(c, sel))
    o.update(margin=margin, score=score, threshold=(margin > 0) & (margin < 4 * lc.E_SEL))
    return rc._readonly(o)


def rl_measure(name):
    """E_SG of one case: the largest |L32 - L64| / sum_m |mu| e, sg_light in torch fp32 against fp64 (finite values, non-zero magnitude)"""
    c = rl_case(name)
    lb, d = torch.from_numpy(c["lobes"].copy()), torch.from_numpy(c["ray_d"].copy())
    with np.errstate(invalid="ignore", over="ignore"):
        l32 = sg.sg_light(lb, d).double().numpy()
        l64, mag = rl_light64(c)
        ok = np.isfinite(l32) & np.isfinite(l64) & (mag > 0)
        return float((np.abs(l32 - l64)[ok] / mag[ok]).max()) if ok.any() else 0.0
