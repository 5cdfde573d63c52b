"""The case matrix of the shading edge-input tests: one table for tests/test_shading_edge_inputs.py (the fp64 oracle alone: every case
holds what it is named for, few rows sit on a threshold, the reference arithmetic stays finite, and what the reference's own fp32
arithmetic loses) and tests/test_gpu_shading_edges.py (the HIP kernels against the fp64 oracle, within that loss).

A case = a builder of svgir_harness.shade_inputs.edge_case + the floors its probe must reach.  `probe` is an instrumented restatement
of oracle/shading_oracle.py: the same arithmetic, returning the arguments of every clamp, sign and floor instead of the outputs; the
host test ties it to the oracle (the specular term rebuilt from the probe equals so.ggx, the light rebuilt equals so.env_lookup).

Threshold rows.  Where an argument of a clamp or of the sign lies on its bound, fp32 may legitimately take the other side; a row
(surfel) with such an argument anywhere among its samples and corners is held to finiteness only, gets zero upstream weight, and a
case may hold at most MAX_THRESHOLD_SHARE of them.  An argument x is "on" the bound b when, in the fp64 oracle,
  * b = 0 (the sign argument V^.N^, the cosine n^.l^ of `n.l clamp(min=0)`, the env value's lower clamp): 0 < |x| <= 1e-5;
  * b = 1e-6 or 4 pi of the GGX denominator, 64 of the env value, 1e-12 of a norm: |x - b| <= 1e-4 |b|;
  * b = 1e-6 of the four cosines N.L, N.V, N.H, V.H: |x - b| <= 5e-7 -- the 1e-4 relative window of the rule (1e-10) is far inside
    what an fp32 dot product of unit vectors resolves (~1e-7), so the window is the rounding reach instead; x = 0 exactly excluded;
  * b = 1 of N.L, N.V, N.H: x >= 1 - 1e-6 (again the rounding reach: a unit dot product cannot pass 1 otherwise) while the pair's
    GGX denominator is not under its lower clamp -- under it the cosine's adjoint is zero on both sides, in both precisions.  (A
    1e-4 relative window below 1 would declare the whole mirror lobe, N.H > 0.9999, a threshold: every row of `mirror_lobe`.)
    V.H <= 1 has no adjoint (V and L are constants) and its value is continuous: no threshold.
Exact zeros (sign 0, H = 0, a zero normal, a zero view direction) are NOT thresholds: both precisions compute them exactly.
The narrower windows make more rows answer to the budget, never fewer.

Per-row error (`row_err`): max |a - b| over the row / max(max |b| over the row, 1e-6 max |b| over the tensor); d_env is one "row".
"""
import math

import numpy as np
import torch

from oracle import shading_oracle as so
from svgir_harness import shade_inputs

MAX_THRESHOLD_SHARE = 0.05
REL, ABS0, COS_REACH = 1e-4, 1e-5, 5e-7
REDUCED = ("pbr", "diffuse_light", "specular", "direct", "indirect", "mean_incident", "mean_local", "mean_global")
LEAVES = ("base_color", "roughness", "normals", "radiance", "env")
INPUTS = ("base_color", "roughness", "normals", "viewdirs", "radiance", "visibility", "dirs", "areas", "env")

# name -> rows (not a multiple of 16: the quad kernel's last wave is partial) and the floors of tests/test_shading_edge_inputs.py
CASES = {
    "mirror_lobe": dict(n=203),
    "grazing_view": dict(n=245),
    "backfacing_and_opposed": dict(n=219),
    "env_poles_and_seam": dict(n=187),
    "env_clamp": dict(n=171),
    "vector_scales": dict(n=251),
    "material_ends": dict(n=333),
}
LATTICE_CASES = ("grazing_view", "vector_scales", "material_ends", "env_clamp")   # directions not adversarial: also in-kernel lattice
ENV_SIZES = ((16, 32), (32, 64), (64, 128))     # LDS gradient image, LDS gradient image, global-atomic fallback


def _run(case, Ns, He=32, We=64, lattice=False, transform=False, hdr=False, ratio=None):
    tag = f"{case}-Ns{Ns}-{He}x{We}" + ("-lattice" if lattice else "") + ("-rot" if transform else "") + ("-hdr" if hdr else "") + \
        (f"-ratio{ratio:g}" if ratio is not None else "")
    return dict(id=tag, case=case, Ns=Ns, He=He, We=We, lattice=lattice, transform=transform, hdr=hdr, ratio=ratio)


def _runs():
    """Every case on both forward layouts (Ns < 128: quad kernel, with Ns not a multiple of 4 among them; Ns >= 128: one wave per
    surfel, 130 among them; the backward runs on both), the env cases at every env size, light mode and with the lookup rotation, the
    lattice cases in lattice mode, material_ends with a radiance ratio (0.83 with NaN cache entries, and 0)."""
    small = {"mirror_lobe": 61, "grazing_view": 24, "backfacing_and_opposed": 30, "env_poles_and_seam": 45, "env_clamp": 64,
             "vector_scales": 7, "material_ends": 96}
    big = {"mirror_lobe": 130, "grazing_view": 130, "backfacing_and_opposed": 128, "env_poles_and_seam": 130, "env_clamp": 136,
           "vector_scales": 130, "material_ends": 200}
    out = []
    for c in CASES:
        if c in ("env_poles_and_seam", "env_clamp"):
            continue
        out += [_run(c, small[c]), _run(c, big[c])]
    for He, We in ENV_SIZES:
        for tr in (False, True):
            out += [_run("env_poles_and_seam", small["env_poles_and_seam"], He, We, transform=tr)]
        out += [_run("env_poles_and_seam", big["env_poles_and_seam"], He, We, transform=(He == 32))]
        for hdr in (False, True):
            out += [_run("env_clamp", small["env_clamp"] if He != 32 else 61, He, We, hdr=hdr)]
        out += [_run("env_clamp", big["env_clamp"], He, We, hdr=(He != 32))]
    for c in LATTICE_CASES:
        out += [_run(c, 61 if c != "vector_scales" else 24, lattice=True, hdr=(c == "env_clamp"))]
    out += [_run("material_ends", 130, lattice=True)]
    out += [_run("material_ends", 61, ratio=0.83), _run("material_ends", 130, ratio=0.83), _run("material_ends", 61, ratio=0.0)]
    return out


RUNS = _runs()
FUSED_CASES = ("mirror_lobe", "grazing_view", "env_clamp")   # material rows given to the surfels of the fused-path scene


def build(run, dirs=None):
    """(inputs fp64, labels, options) of a RUNS entry; `dirs` [n,Ns,3]: replaces the case's directions (lattice mode: the directions
    the kernels generate, areas 2 pi)."""
    d, lab, opt = shade_inputs.edge_case(run["case"], CASES[run["case"]]["n"], run["Ns"], He=run["He"], We=run["We"],
                                         transform=run["transform"], hdr=run["hdr"])
    if dirs is not None:
        d["dirs"] = dirs.double().cpu()
        d["areas"] = torch.full_like(d["areas"], 2 * math.pi)
    opt["radiance_ratio"] = run["ratio"]
    if run["ratio"] is not None and "nan_cache_entries" in opt:
        e = opt["nan_cache_entries"]
        d["radiance"][e[:, 0], e[:, 1], e[:, 2]] = float("nan")
    return d, lab, opt


def probe(d, opt):
    """The arguments of every clamp, sign and floor of oracle/shading_oracle.py, in the dtype of `d` (see the module docstring)."""
    n_raw, v_raw, l_raw = d["normals"], d["viewdirs"], d["dirs"]
    nn, nv, nl = n_raw.norm(dim=-1), v_raw.norm(dim=-1), l_raw.norm(dim=-1)
    L = (l_raw / nl.clamp_min(1e-12)[..., None])[:, :, None, :]
    V = (v_raw / nv.clamp_min(1e-12)[..., None])[:, None, None, :]
    h_raw = (L + V) / 2.0
    nh = h_raw.norm(dim=-1)[:, :, 0]
    H = h_raw / nh.clamp_min(1e-12)[:, :, None, None]
    N0 = n_raw / nn.clamp_min(1e-12)[..., None]
    sgn_arg = (V[:, 0] * N0).sum(-1)                       # [n,4]
    N = (N0 * sgn_arg.sign()[..., None])[:, None]
    NoL, NoV, NoH, VoH = (N * L).sum(-1), (N * V).sum(-1), (N * H).sum(-1), (V * H).sum(-1)
    r = d["roughness"][:, None, :]
    a = r * r
    a2 = a * a
    k = (a + 2 * r + 1.0) / 8.0
    c = lambda x: x.clamp(1e-6, 1)  # noqa: E731
    nom0 = c(NoH) * c(NoH) * (a2 - 1) + 1
    nom = 4 * math.pi * nom0 * nom0 * (c(NoV) * (1 - k) + k) * (c(NoL) * (1 - k) + k)
    frac = (0.04 + 0.96 * torch.pow(torch.full_like(VoH, 2.0), (-5.55473 * c(VoH) - 6.98316) * c(VoH))) * a2
    ndl = (n_raw[:, None] * l_raw[:, :, None]).sum(-1)     # [n,Ns,4], the argument of clamp(min=0)
    ndl_hat = ndl / (nn[:, None, :] * nl[:, :, None]).clamp_min(1e-300)
    # env lookup (so.env_lookup), value before the clamp and the tap footprint
    env = d["env"]
    sp = (torch.nn.functional.softplus(env) if opt["softplus"] else env).reshape((-1,) + tuple(env.shape[-3:]))[0]
    He, We = sp.shape[0], sp.shape[1]
    ld = l_raw if opt["transform"] is None else l_raw @ opt["transform"].to(l_raw.dtype).T
    x = (-torch.atan2(ld[..., 1], ld[..., 0]) / math.pi + 1) * 0.5 * (We - 1)
    y = ((torch.arccos(ld[..., 2]) - 1e-6) / math.pi * 2 - 1 + 1) * 0.5 * (He - 1)
    x0, y0 = torch.floor(x).long(), torch.floor(y).long()
    fx, fy = x - torch.floor(x), y - torch.floor(y)
    E = torch.zeros(l_raw.shape, dtype=sp.dtype)
    for dy_, wy in ((0, 1 - fy), (1, fy)):
        for dx_, wx in ((0, 1 - fx), (1, fx)):
            xi, yi = x0 + dx_, y0 + dy_
            ok = (xi >= 0) & (xi < We) & (yi >= 0) & (yi < He)
            E = E + torch.where(ok[..., None], sp[yi.clamp(0, He - 1), xi.clamp(0, We - 1)] * (wx * wy)[..., None], torch.zeros_like(E))
    return dict(sgn_arg=sgn_arg, NoL=NoL, NoV=NoV[:, 0], NoH=NoH, VoH=VoH[:, :, 0], nom=nom, fs=frac / nom.clamp(1e-6, 4 * math.pi),
                ndl=ndl, ndl_hat=ndl_hat, env_pre=E * opt["scale"], x0=x0, y0=y0, fx=fx, fy=fy, He=He, We=We,
                norm_n=nn, norm_v=nv, norm_l=nl, norm_h=nh, sp=sp)


def threshold_rows(p):
    """bool [n]: rows with a clamp / sign argument on its bound (module docstring), from a probe of the fp64 oracle."""
    n = p["sgn_arg"].shape[0]
    rows = lambda m: m.reshape(n, -1).any(1)  # noqa: E731
    near0 = lambda x: (x != 0) & (x.abs() <= ABS0)  # noqa: E731
    near = lambda x, b: (x - b).abs() <= REL * abs(b)  # noqa: E731
    t = rows(near0(p["sgn_arg"])) | rows(near0(p["ndl_hat"])) | rows(near0(p["env_pre"])) | rows(near(p["env_pre"], 64.0))
    t |= rows(near(p["nom"], 1e-6)) | rows(near(p["nom"], 4 * math.pi))
    for k in ("norm_n", "norm_v", "norm_l", "norm_h"):
        t |= rows(near(p[k], 1e-12))
    for k in ("NoL", "NoV", "NoH", "VoH"):
        t |= rows((p[k] != 0) & ((p[k] - 1e-6).abs() <= COS_REACH))
    live = p["nom"] >= 1e-6 * (1 - REL)                       # [n,Ns,4]: the denominator's lower clamp is not (safely) active
    t |= rows((p["NoL"] >= 1 - 1e-6) & live) | rows((p["NoH"] >= 1 - 1e-6) & live) | rows((p["NoV"] >= 1 - 1e-6)[:, None, :] & live)
    return t


def row_err(a, b, whole=False):
    """Per-row error [n] of a against b (module docstring); whole=True: one value, normalised by the tensor's maximum."""
    a = torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    tmax = float(b.abs().max()) if b.numel() else 0.0
    if whole:
        return (a - b).abs().max().reshape(1) / max(tmax, 1e-300)
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    den = torch.maximum(b.abs().max(1).values, torch.tensor(1e-6 * tmax, dtype=torch.float64)).clamp_min(1e-300)
    return (a - b).abs().max(1).values / den


def weights(d, thr, seed, training=None):
    """Random upstream weights, zero on the threshold rows `thr` (None: non-zero everywhere): on the eight reduced outputs, or with
    `training` set on features / vfeatures / pbr of the packed call."""
    g = torch.Generator().manual_seed(seed)
    n = d["base_color"].shape[0]
    keep = torch.ones(n, 1, dtype=torch.float64) if thr is None else (~thr).double()[:, None]
    if training is None:
        return {k: torch.randn(n, 12 if i < 5 else 3, generator=g, dtype=torch.float64) * keep for i, k in enumerate(REDUCED)}
    S, VS = (4, 52) if training else (7, 64)
    return {"features": torch.randn(n, S, generator=g, dtype=torch.float64) * keep,
            "vfeatures": torch.randn(n, VS, generator=g, dtype=torch.float64) * keep,
            "pbr": torch.randn(n, 12, generator=g, dtype=torch.float64) * keep}


def oracle_run(d, opt, w, dtype=torch.float64, view=None, training=None):
    """Forward and torch.autograd backward of the oracle in `dtype` under the upstream weights w (fp64): (outputs, gradients).  With a
    radiance ratio the cache is cleaned as nan_to_num(cache * ratio, nan=0) and the ratio is a leaf (`radiance_ratio` in the
    gradients, the cache's NaN entries zeroed beforehand as the kernels skip them); `view` [3,3] + `training`: the packed call."""
    cv = lambda t: t.to(dtype)  # noqa: E731
    lv = {k: cv(d[k]).clone().requires_grad_(True) for k in LEAVES}
    rad = lv["radiance"]
    if opt["radiance_ratio"] is not None:
        lv["radiance_ratio"] = torch.tensor(opt["radiance_ratio"], dtype=dtype, requires_grad=True)
        rad = torch.nan_to_num(cv(d["radiance"]), nan=0.0) * lv["radiance_ratio"]
        del lv["radiance"]
    out = so.shade(lv["base_color"], lv["roughness"], lv["normals"], cv(d["viewdirs"]), rad, cv(d["visibility"]), cv(d["dirs"]),
                   cv(d["areas"]), lv["env"], softplus=opt["softplus"], scale=opt["scale"],
                   transform=None if opt["transform"] is None else cv(opt["transform"]))
    if training is not None:
        f, vf = so.pack(out, lv["base_color"], lv["roughness"], lv["normals"], cv(view), training)
        out = dict(out, features=f, vfeatures=vf)
    sum((out[k] * cv(w[k])).sum() for k in w).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in lv.items()}
    return {k: v.detach() for k, v in out.items()}, grads


def e32(d, opt, w, thr, view=None, training=None):
    """(fp64 outputs, fp64 gradients, E32): E32[tensor] = the largest per-row error of the fp32 oracle against the fp64 oracle over
    the non-threshold rows (d_env: normalised by the tensor's maximum).  Everything must be finite in both precisions."""
    o64, g64 = oracle_run(d, opt, w, torch.float64, view, training)
    o32, g32 = oracle_run(d, opt, w, torch.float32, view, training)
    E = {}
    for tag, r64, r32 in (("", o64, o32), ("d_", g64, g32)):
        for k in r64:
            if k == "mean_vis":
                continue
            assert torch.isfinite(r64[k]).all() and torch.isfinite(r32[k]).all(), f"oracle {tag}{k} is not finite"
            if r64[k].dim() == 0 or k == "env":
                E[tag + k] = float(row_err(r32[k].reshape(1, -1), r64[k].reshape(1, -1), whole=True))
            else:
                e = row_err(r32[k], r64[k])[~thr]
                E[tag + k] = float(e.max()) if e.numel() else 0.0
    return o64, g64, E


def view3x3(seed=5):
    return torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64))[0]
