"""The case table and the oracle of the spherical-Gaussian direct-light tests: tests/test_sg_light_edge_inputs.py (CPU: the oracle against
the reference's recorded results, the gradient formulas, the conditions on the table, what fp32 loses) and tests/test_gpu_sg_light.py (the
HIP kernels against the fp64 oracle within that loss).

Oracle.  `sg_light` is the contract of include/svgir_raster.h in torch at a given dtype -- a = xi / |xi|, e = exp(|lambda| (d.a - 1)),
L_c = sum_m |mu_mc| e_m -- and `shade` composes clamp(L, 0, 64) * visibility with `ggx` and `pack` of oracle/shading_oracle.py; the transport
lines are restated from there.  fp64 is the truth; the same code in fp32 gives E32 (outputs) and G32 (gradients) per case and tensor, the
largest per-row error (shading_cases.row_err; a row of d_lobes is a lobe) over the rows that are not on a threshold of the EXISTING
arithmetic (shading_cases.threshold_rows: the n.i / dot-product clamps and the sign; those rows get zero upstream weight and are held to
finiteness).  The SG light adds one clamp, L at 64 (L >= 0 by construction and the lower bound passes at equality on both sides): the table
keeps every sample's fp64 L_c more than 1e-3 relative away from 64 -- asserted by the CPU test -- so the GPU test excludes nothing for it.

All inputs are fp32-representable: the kernels see exactly the numbers the fp64 oracle sees.
"""
import math

import torch

import shading_cases as sc
from oracle import shading_oracle as so

REDUCED = sc.REDUCED
LEAVES = ("base_color", "roughness", "normals", "radiance", "lobes")


def sg_light(lobes, dirs):
    """[..., 3]: the unclamped light of `dirs` [..., 3] under the raw lobes [M, 7] (DirectLightSG.direct_light)."""
    xi, lam, mu = lobes[:, :3], lobes[:, 3].abs(), lobes[:, 4:].abs()
    a = xi / torch.sqrt((xi * xi).sum(-1, keepdim=True))
    t = (dirs[..., None, :] * a).sum(-1) - 1.0                 # [..., M]
    return (torch.exp(lam * t)[..., None] * mu).sum(-2)


def sg_grad(lobes, dirs, g):
    """The closed-form gradient of sum(L * g) w.r.t. the raw lobes (include/svgir_raster.h), g [..., 3] the adjoint of L."""
    xi, lam, mu = lobes[:, :3], lobes[:, 3], lobes[:, 4:]
    nrm = torch.sqrt((xi * xi).sum(-1, keepdim=True))
    a = xi / nrm
    d, g = dirs.reshape(-1, 3), g.reshape(-1, 3)
    da = d @ a.T                                               # [n, M]
    e = torch.exp(lam.abs() * (da - 1.0))
    s = e * (g @ mu.abs().T)                                   # [n, M]
    d_mu = torch.sign(mu) * (e.T @ g)
    d_lam = torch.sign(lam) * ((da - 1.0) * s).sum(0)
    d_xi = lam.abs()[:, None] * (s.T @ d - a * (s * da).sum(0)[:, None]) / nrm
    return torch.cat([d_xi, d_lam[:, None], d_mu], dim=-1)


def shade(base_color, roughness, normals, viewdirs, radiance, visibility, dirs, areas, lobes):
    """oracle/shading_oracle.py:shade with the SG light as the global light (same keys)."""
    n = dirs.shape[0]
    glob = sg_light(lobes, dirs).clamp(0, 64) * visibility
    loc = radiance
    inc = loc + glob
    ndi = (normals[:, None] * dirs[:, :, None]).sum(-1).clamp(min=0)
    fs = so.ggx(normals, viewdirs, dirs, roughness)
    fd = base_color.reshape(n, 3, 4) / math.pi
    geo = (areas * ndi)[:, :, None, :]
    t, td, ti = inc[:, :, :, None] * geo, glob[:, :, :, None] * geo, loc[:, :, :, None] * geo
    f = fd[:, None] + fs[:, :, None, :]
    return {"pbr": (f * t).mean(1).reshape(n, 12), "diffuse_light": t.mean(1).reshape(n, 12),
            "specular": (fs[:, :, None, :] * t).mean(1).reshape(n, 12), "direct": (f * td).mean(1).reshape(n, 12),
            "indirect": (f * ti).mean(1).reshape(n, 12), "mean_incident": inc.mean(1), "mean_local": loc.mean(1),
            "mean_global": glob.mean(1), "mean_vis": visibility.mean(1)}


# ---- the table ------------------------------------------------------------------------------------------------------------------
# P: 1, 15 / 16 / 17 (the 16 surfels per wave of the quad forward), 65, 257 (one workgroup +- 1).  Ns: 1, 7, 64 / 65 (the backward's
# chunks), 128 / 129 (quad / wide forward), 384.  M: 1, 3 / 4 / 5, 32 / 33, 128 (the backward's lanes-per-lobe groups, two lobes per lane).
# mode: None = the reduced call (rendering_equation4), True / False = the packed call at training / eval width.
def _case(id, P, Ns, M, mode=None, lattice=False, ratio=None, view=False, special=None, grads=True):
    return dict(id=id, P=P, Ns=Ns, M=M, mode=mode, lattice=lattice, ratio=ratio, view=view, special=special, grads=grads)


CASES = [
    _case("P1-Ns1-M1", 1, 1, 1),
    _case("P15-Ns7-M3", 15, 7, 3),
    _case("P16-Ns64-M4-train", 16, 64, 4, mode=True),
    _case("P17-Ns65-M5-lattice", 17, 65, 5, lattice=True),
    _case("P65-Ns128-M32-ratio", 65, 128, 32, ratio=0.83),
    _case("P257-Ns129-M33-view", 257, 129, 33, view=True),
    _case("P17-Ns384-M128-eval", 17, 384, 128, mode=False),
    _case("P65-Ns64-M128-train-lattice-ratio", 65, 64, 128, mode=True, lattice=True, ratio=1.21),
    _case("P33-Ns24-M32-view-train", 33, 24, 32, mode=True, view=True),
    # the two instantiations no row above reaches: the wide forward with a ratio, the view pass with a ratio (P: no multiple of 4, 12, 16, 64)
    _case("P67-Ns129-M5-ratio-view", 67, 129, 5, ratio=0.83, view=True),
    _case("signs-and-zeros", 33, 24, 8, special="signs"),
    _case("sharp-on-axis", 17, 16, 4, special="sharp"),
    _case("clamp64", 33, 24, 5, special="clamp"),
    _case("occluded", 17, 7, 4, special="occluded"),
    _case("unnormalised-dirs", 17, 16, 4, special="unnormalised"),
    _case("zero-norm-lobe", 17, 7, 3, special="zero_norm", grads=False),
]
BY_ID = {c["id"]: c for c in CASES}


def _f32(t):
    return t.float().double()


def build(case, dirs=None):
    """fp64 (fp32-representable) inputs of a case: the shading inputs + `lobes` [M,7] (+ `geo` [P,3], the lattice's axis)."""
    P, Ns, M = case["P"], case["Ns"], case["M"]
    g = torch.Generator().manual_seed(1000 + 7 * P + 3 * Ns + M)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    unit = lambda v: v / v.norm(dim=-1, keepdim=True)  # noqa: E731
    geo = unit(rnd(P, 3))
    d = {
        "base_color": torch.sigmoid(rnd(P, 12)) * 0.77 + 0.03, "roughness": torch.sigmoid(rnd(P, 4)) * 0.9 + 0.09,
        "normals": unit(geo[:, None] + 0.1 * rnd(P, 4, 3)), "viewdirs": unit(geo + 0.5 * rnd(P, 3)),
        "radiance": (0.2 * rnd(P, Ns, 3)).abs(), "visibility": (torch.rand(P, Ns, 1, generator=g, dtype=torch.float64) > 0.3).double(),
        "dirs": unit(geo[:, None] + 0.9 * rnd(P, Ns, 3)), "areas": torch.full((P, Ns, 1), 2 * math.pi, dtype=torch.float64),
    }
    # the reference's initialisation scaled to lobes a random direction meets (sharpness |N(0,1)| * 20 instead of * 100), a third of them
    # at the reference's own sharpness
    lobes = rnd(M, 7)
    lobes[:, 3] *= torch.where(torch.arange(M) % 3 == 2, 100.0, 20.0)
    sp = case["special"]
    if sp == "signs":
        lobes[0, 3] = -abs(lobes[0, 3]); lobes[0, 4:] = -lobes[0, 4:].abs()          # negative lambda and mu (the abs)
        lobes[1, 3] = 0.0                                                             # lambda = 0: a constant lobe
        lobes[2, 5] = 0.0                                                             # mu = 0 in one channel
        lobes[3, 4:] = 0.0                                                            # ... and in all (the sign(0) rows)
        lobes[4, 4] = -0.0
    elif sp == "sharp":
        lobes[0] = torch.tensor([0.0, 0.0, 2.0, 1000.0, 0.7, 0.4, 0.9], dtype=torch.float64)   # a = +z exactly
        lobes[1] = torch.tensor([0.0, -3.0, 0.0, -1000.0, 0.2, 0.6, 0.3], dtype=torch.float64)  # a = -y exactly
        d["dirs"][0, 0] = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)    # on the axis: e = 1
        d["dirs"][0, 1] = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64)   # opposite: exp(-2000) underflows to 0
        d["dirs"][1, 0] = torch.tensor([0.0, -1.0, 0.0], dtype=torch.float64)
        d["dirs"][1, 1] = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
        d["visibility"][:2, :2] = 1.0
    elif sp == "clamp":
        lobes[0] = torch.tensor([0.3, -0.5, 0.8, 3.0, 400.0, 250.0, 90.0], dtype=torch.float64)   # bright and wide: part of the samples pass 64
    elif sp == "occluded":
        d["visibility"].zero_()
    elif sp == "unnormalised":
        d["dirs"] = d["dirs"] * (0.4 + 1.2 * torch.rand(P, Ns, 1, generator=g, dtype=torch.float64))
        lobes[:, 3] = rnd(M) * 4.0     # (|d| up to 1.6: d.a - 1 up to +0.6)
    elif sp == "zero_norm":
        lobes[1, :3] = 0.0
    d["lobes"] = lobes
    d = {k: _f32(v) for k, v in d.items()}
    if sp == "clamp":   # the few samples that land within 2e-3 of the clamp look straight into the bright lobe instead (far above it)
        near = ((sg_light(d["lobes"], d["dirs"]) - 64).abs() <= 2e-3 * 64).any(-1)
        d["dirs"][near] = _f32(d["lobes"][0, :3] / d["lobes"][0, :3].norm())
    d["geo"] = _f32(geo)
    if dirs is not None:     # lattice mode: the directions the kernels generate, areas 2 pi
        d["dirs"] = dirs.double().cpu()
        d["areas"] = torch.full_like(d["areas"], 2 * math.pi)
    return d


def light64(d):
    return sg_light(d["lobes"], d["dirs"])


def threshold_rows(d):
    """bool [P]: rows on a threshold of the existing shading arithmetic (shading_cases.threshold_rows); the probe's texture is a dummy."""
    dd = dict(d, env=torch.zeros(1, 2, 4, 3, dtype=torch.float64))
    return sc.threshold_rows(sc.probe(dd, dict(softplus=False, scale=1.0, transform=None)))


def weights(case, d, thr, seed=11):
    return sc.weights(d, thr, seed, training=case["mode"])


def oracle_run(case, d, w, dtype=torch.float64):
    """(outputs, gradients) of the oracle in `dtype` under the fp64 upstream weights w; with a ratio the cache is multiplied by the leaf
    `radiance_ratio` (the table's caches are finite); with `view` viewdirs is a leaf too."""
    cv = lambda t: t.to(dtype)  # noqa: E731
    lv = {k: cv(d[k]).clone().requires_grad_(True) for k in LEAVES}
    rad = lv["radiance"]
    if case["ratio"] is not None:
        lv["radiance_ratio"] = torch.tensor(case["ratio"], dtype=dtype, requires_grad=True)
        rad = cv(d["radiance"]) * lv["radiance_ratio"]
        del lv["radiance"]
    vd = cv(d["viewdirs"])
    if case["view"]:
        lv["viewdirs"] = vd = vd.clone().requires_grad_(True)
    out = shade(lv["base_color"], lv["roughness"], lv["normals"], vd, rad, cv(d["visibility"]), cv(d["dirs"]), cv(d["areas"]), lv["lobes"])
    if case["mode"] is not None:
        f, vf = so.pack(out, lv["base_color"], lv["roughness"], lv["normals"], cv(sc.view3x3()), case["mode"])
        out = dict(out, features=f, vfeatures=vf)
    grads = {}
    if case["grads"]:
        sum((out[k] * cv(w[k])).sum() for k in w).backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in lv.items()}
    return {k: v.detach() for k, v in out.items()}, grads


def e32(case, d, w, thr):
    """(fp64 outputs, fp64 gradients, E): E[tensor] / E['d_' + leaf] = the largest per-row error of the fp32 oracle against the fp64 one
    over the non-threshold rows (a row of d_lobes is a lobe; a scalar: its relative error)."""
    o64, g64 = oracle_run(case, d, w, torch.float64)
    o32, g32 = oracle_run(case, d, w, torch.float32)
    E = {}
    for tag, r64, r32 in (("", o64, o32), ("d_", g64, g32)):
        for k in r64:
            if k == "mean_vis":
                continue
            assert torch.isfinite(r64[k]).all() and torch.isfinite(r32[k]).all(), f"oracle {tag}{k} is not finite"
            if r64[k].dim() == 0:
                E[tag + k] = float(sc.row_err(r32[k].reshape(1, -1), r64[k].reshape(1, -1), whole=True))
            elif tag + k == "d_lobes":
                E[tag + k] = float(sc.row_err(r32[k], r64[k]).max())
            else:
                e = sc.row_err(r32[k], r64[k])[~thr]
                E[tag + k] = float(e.max()) if e.numel() else 0.0
    return o64, g64, E
