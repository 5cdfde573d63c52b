"""Synthetic inputs of the SV-BRDF shading stage in the reference's shapes (base_color sigma(N)*0.77+0.03
[P,12], roughness sigma(N)*0.9+0.09 [P,4], shading normals = geometric normal + N(0,0.1) offsets [P,4,3], Ns Fibonacci
directions around the normal (utils/graphics_utils.py:9-37 without the random rotation), areas 2*pi, visibility
U(0,1) > 0.3, radiance |N(0,0.2)|, env = U(0,3) raw texels (softplus applied by the light) at 32x64)."""
import math

import torch


class Light:
    """Minimal stand-in with the attribute the shading binding reads from scene.direct_light_map.DirectLightMap."""

    def __init__(self, env):
        self.env = env


class SGLight:
    """Minimal stand-in with the attribute the shading binding reads from scene.direct_light_sg.DirectLightSG: the raw lobes [M, 7]."""

    def __init__(self, lgtSGs):
        self.lgtSGs = lgtSGs


def sg_lobes(M, seed=3, device="cpu"):
    """DirectLightSG.__init__ (scene/direct_light_sg.py:87-88): randn [M, 7] with the sharpness column multiplied by 100."""
    l = torch.randn(M, 7, generator=torch.Generator().manual_seed(seed))
    l[:, 3] *= 100.0
    return l.to(device)


def fibonacci_dirs(normals, Ns):
    """Hemisphere directions around `normals` [P,3] -> [P,Ns,3] (z clamped to sin(10 deg) like the reference)."""
    dev = normals.device
    idx = torch.arange(Ns, dtype=torch.float32, device=dev)
    z = (1 - 2 * idx / (2 * Ns - 1)).clamp_min(math.sin(10 / 180 * math.pi))
    rad = torch.sqrt(1 - z * z)
    theta = math.pi * (3.0 - math.sqrt(5.0)) * idx
    local = torch.stack([torch.sin(theta) * rad, torch.cos(theta) * rad, z], dim=-1)      # [Ns,3]
    n = torch.nn.functional.normalize(normals, dim=-1)
    a = torch.where(n[:, 2:3].abs() < 0.9, torch.tensor([0.0, 0.0, 1.0], device=dev), torch.tensor([1.0, 0.0, 0.0], device=dev))
    t0 = torch.nn.functional.normalize(torch.cross(a.expand_as(n), n, dim=-1), dim=-1)
    t1 = torch.cross(n, t0, dim=-1)
    return local[None, :, 0:1] * t0[:, None] + local[None, :, 1:2] * t1[:, None] + local[None, :, 2:3] * n[:, None]


def make(P, Ns, seed=2, device="cpu", geo_normals=None, env_res=32, with_dirs=True):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    if geo_normals is None:
        geo_normals = torch.nn.functional.normalize(rnd(P, 3), dim=-1)
    geo_normals = geo_normals.float().cpu()
    d = {
        "base_color": torch.sigmoid(rnd(P, 12)) * 0.77 + 0.03,
        "roughness": torch.sigmoid(rnd(P, 4)) * 0.9 + 0.09,
        "normals": torch.nn.functional.normalize(geo_normals[:, None] + 0.1 * rnd(P, 4, 3), dim=-1),
        "viewdirs": torch.nn.functional.normalize(geo_normals + 0.5 * rnd(P, 3), dim=-1),
        "visibility": (torch.rand(P, Ns, 1, generator=g) > 0.3).float(),
        "radiance": (0.2 * rnd(P, Ns, 3)).abs(),
        "env": 3.0 * torch.rand(1, env_res, 2 * env_res, 3, generator=g),
    }
    d = {k: v.to(device) for k, v in d.items()}
    if with_dirs:   # (omitted when the shading kernels generate the lattice themselves: 16 bytes per sample less)
        d["areas"] = torch.full((P, Ns, 1), 2 * math.pi, device=device)
        d["dirs"] = fibonacci_dirs(geo_normals.to(device), Ns).contiguous()
    return d


# ---- edge inputs: the clamps, poles and degenerate vectors of the shading arithmetic (tests/shading_cases.py) ------------------
# One builder per named case; every case is an ordinary input dict in fp64 plus a per-row label naming the construction of the row and
# the options of the call (light mode, lookup rotation, radiance ratio).  Rows labelled "ordinary" are smooth random rows that keep the
# case from consisting of special rows only.  `geo_normals` (the hemisphere axis of the row's incident directions) rides along for the
# callers that replace `dirs` / `areas` by the in-kernel lattice.
EDGE_CASES = ("mirror_lobe", "grazing_view", "backfacing_and_opposed", "env_poles_and_seam", "env_clamp", "vector_scales",
              "material_ends")


def _unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def _perp(v, g):
    """A random unit vector perpendicular to the unit vectors v [..,3]."""
    r = torch.randn(v.shape, generator=g, dtype=torch.float64)
    return _unit(r - (r * v).sum(-1, keepdim=True) * v)


def _off_axis(axis, angle, g):
    """Unit vectors at `angle` (radians, broadcastable to axis[..., 0]) from the unit vectors `axis`."""
    angle = torch.as_tensor(angle, dtype=torch.float64)
    return torch.cos(angle)[..., None] * axis + torch.sin(angle)[..., None] * _perp(axis, g)


def _ordinary(n, Ns, g, He, We):
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    geo = _unit(rnd(n, 3))
    return {
        "base_color": torch.sigmoid(rnd(n, 12)) * 0.77 + 0.03,
        "roughness": torch.sigmoid(rnd(n, 4)) * 0.9 + 0.09,
        "normals": _unit(geo[:, None] + 0.1 * rnd(n, 4, 3)),
        "viewdirs": _unit(geo + 0.5 * rnd(n, 3)),
        "radiance": (0.2 * rnd(n, Ns, 3)).abs(),
        "visibility": (torch.rand(n, Ns, 1, generator=g, dtype=torch.float64) > 0.3).double(),
        "dirs": _unit(geo[:, None] + 0.9 * rnd(n, Ns, 3)),
        "areas": torch.full((n, Ns, 1), 2 * math.pi, dtype=torch.float64),
        "env": 3.0 * torch.rand(1, He, We, 3, generator=g, dtype=torch.float64),
        "geo_normals": geo,
    }


def _latlong_dir(row, col, He, We):
    """The direction whose lookup lands exactly on texel (row, col) -- fractional values allowed -- of a He x We lat-long map."""
    phi = torch.as_tensor(row, dtype=torch.float64) / (He - 1) * math.pi + 1e-6
    theta = -(torch.as_tensor(col, dtype=torch.float64) / (We - 1) * 2 - 1) * math.pi
    return torch.stack([torch.sin(phi) * torch.cos(theta), torch.sin(phi) * torch.sin(theta), torch.cos(phi)], dim=-1)


def edge_case(name, n, Ns, seed=0, He=32, We=64, transform=False, hdr=None):
    """(inputs, labels, options) of the edge case `name` with n rows and Ns incident samples.
    inputs: fp64 dict base_color, roughness, normals, viewdirs, radiance, visibility, dirs, areas, env (+ geo_normals);
    labels: numpy array [n] of str; options: dict(softplus, scale, transform [3,3] | None, radiance_ratio float | None).
    `transform` (env_poles_and_seam): look the map up with rotated directions; `hdr` (env_clamp): EnvLight mode (identity, scale 1)
    instead of softplus, default: softplus."""
    import numpy as np
    assert name in EDGE_CASES, name
    g = torch.Generator().manual_seed(1000 + 17 * seed + EDGE_CASES.index(name))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    uni = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    d = _ordinary(n, Ns, g, He, We)
    lab = np.array(["ordinary"] * n, dtype=object)
    opt = dict(softplus=True, scale=2.0, transform=None, radiance_ratio=None)
    rows = torch.randperm(n, generator=g)   # the special groups take disjoint slices of a shuffled row order

    def take(frac, label, start=[0]):
        k = max(1, int(round(frac * n)))
        idx = rows[start[0]:start[0] + k]
        start[0] += k
        assert start[0] <= n
        lab[idx.numpy()] = label
        return idx

    if name == "mirror_lobe":
        # view direction well above every corner's horizon; samples 0 mod 3: within 1e-3 rad of the reflection of V about corner
        # (s // 3) % 4's normal; 1 mod 3: a ring 0.5 .. 5 degrees off it; 2 mod 3: the wide hemisphere draw
        for label, frac, rlo, rhi in (("mirror_0.09", 0.80, 0.09, 0.09), ("mirror_0.09_0.15", 0.04, 0.09, 0.15)):
            idx = take(frac, label)
            m = idx.numel()
            N = d["normals"][idx]
            V = _unit(d["geo_normals"][idx] + 0.35 * rnd(m, 3))
            low = ((N * V[:, None]).sum(-1) < 0.3).any(1)   # (near the horizon |L + V| is small and 1e-3 rad of L moves H by degrees)
            V[low] = _unit(N[low].sum(1))
            d["viewdirs"][idx] = V
            d["roughness"][idx] = rlo + (rhi - rlo) * uni(m, 4)
            dirs = d["dirs"][idx]
            for s in range(Ns):
                if s % 3 == 2:
                    continue
                Nk = N[:, (s // 3) % 4]
                R = 2 * (Nk * V).sum(-1, keepdim=True) * Nk - V
                ang = 1e-3 * uni(m) if s % 3 == 0 else math.radians(0.5) + math.radians(4.5) * uni(m)
                dirs[:, s] = _off_axis(R, ang, g)
            d["dirs"][idx] = dirs
    elif name == "grazing_view":
        def graze(idx, cosines):   # corner k's unit normal at V . N = cosines[:, k] exactly
            m = idx.numel()
            V = d["viewdirs"][idx]
            T = _perp(V, g)
            for k in range(4):
                Tk = _unit(T + 0.1 * _perp(V, g) * uni(m, 1))
                Tk = _unit(Tk - (Tk * V).sum(-1, keepdim=True) * V)
                c = cosines[:, k:k + 1]
                d["normals"][idx, k] = c * V + torch.sqrt(1 - c * c) * Tk
            d["geo_normals"][idx] = T
            d["dirs"][idx] = _unit(T[:, None] + 0.9 * rnd(m, Ns, 3))
        for mag in (1e-2, 1e-4):
            idx = take(0.2, f"graze_{mag:g}")
            graze(idx, mag * (2.0 * (uni(idx.numel(), 4) > 0.5).double() - 1.0))
        idx = take(0.15, "mixed_sign")
        graze(idx, torch.tensor([1e-2, -1e-2, 1e-4, -1e-4], dtype=torch.float64).expand(idx.numel(), 4).clone())
        # coordinate axes: V along +-e_a (any length), every corner normal in the plane of the other two axes: V . N is 0 exactly in
        # every precision, sign 0 zeroes the GGX normal
        idx = take(0.15, "axis_zero")
        m = idx.numel()
        a = torch.randint(0, 3, (m,), generator=g)
        V = torch.zeros(m, 3, dtype=torch.float64)
        V[torch.arange(m), a] = (2.0 * (uni(m) > 0.5).double() - 1.0) * (0.5 + uni(m))
        Nn = torch.zeros(m, 4, 3, dtype=torch.float64)
        b, c = (a + 1) % 3, (a + 2) % 3
        ar = torch.arange(m)
        Nn[ar, 0, b] = 1.0
        Nn[ar, 1, c] = -1.0
        Nn[ar, 2, b] = 1.0
        Nn[ar, 2, c] = 1.0
        Nn[ar, 3, b] = -0.25
        Nn[ar, 3, c] = 0.75
        d["viewdirs"][idx], d["normals"][idx] = V, Nn
        geo = _unit(Nn[:, 2])
        d["geo_normals"][idx] = geo
        d["dirs"][idx] = _unit(geo[:, None] + 0.9 * rnd(m, Ns, 3))
    elif name == "backfacing_and_opposed":
        idx = take(0.3, "backfacing")     # two thirds of the samples below the horizon of the geometric normal
        m = idx.numel()
        flip = torch.ones(Ns, dtype=torch.float64)
        flip[torch.arange(Ns) % 3 != 0] = -1.0
        d["dirs"][idx] = _unit(d["geo_normals"][idx][:, None] * (0.8 * flip[None, :, None]) + 0.5 * rnd(m, Ns, 3))
        idx = take(0.3, "opposed")        # every other sample is L = -V exactly: H = 0
        dirs = d["dirs"][idx]
        dirs[:, ::2] = -d["viewdirs"][idx][:, None]
        d["dirs"][idx] = dirs
        idx = take(0.1, "zero_view")
        d["viewdirs"][idx] = 0.0
    elif name == "env_poles_and_seam":
        special = [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (-1.0, 0.0, 0.0), (-1.0, -0.0, 0.0), (-1.0, 1e-7, 0.0), (-1.0, -1e-7, 0.0)]
        sp = _unit(torch.tensor(special, dtype=torch.float64))
        # one texel off each of them: a row below the north pole / above the south pole, a column either side of the seam
        off = torch.cat([_latlong_dir([1.0, He - 2.0], [We / 2 - 0.5, We / 2 - 0.5], He, We),
                         _latlong_dir([He / 2 - 0.5] * 4, [1.0, We - 2.0, 0.5, We - 1.5], He, We)])
        pool = torch.cat([sp, off])
        if transform:
            # the lookup uses dirs @ rot.T: a quarter turn about x takes the non-special directions (0, +-1, 0) onto the poles.  Its
            # entries are 0 and +-1, so the rotated z is exact in every precision and every summation order: a generic rotation puts
            # the pole at z = 1 +- one rounding, and arccos of a z above 1 is NaN in the reference itself
            opt["transform"] = torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]], dtype=torch.float64)
            opt.update(softplus=False, scale=1.0)   # (EnvLight.transform, scene/envmap.py: the HDR light is the one with a rotation)
            pool = pool @ opt["transform"]     # (row vectors: pool @ rot = rot^-1 pool -- the special set as seen through the rotation)
            pool = torch.cat([pool, torch.tensor([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]], dtype=torch.float64)])
        idx = take(0.6, "poles_and_seam")   # every other sample of these rows is one of the pool's directions
        m = idx.numel()
        dirs = d["dirs"][idx]
        for s in range(0, Ns, 2):
            pick = torch.randint(0, pool.shape[0], (m,), generator=g)
            dirs[:, s] = pool[pick]
        d["dirs"][idx] = dirs
        d["visibility"][idx] = 1.0
    elif name == "env_clamp":
        # blocks of texels share a class per channel (inside the clamp / beyond it), so that most bilinear footprints are of one class
        # and few lookups land within 1e-4 of a bound (tests/shading_cases.py: threshold rows)
        blk = max(He // 4, 1)
        cls = torch.rand(1, (He + blk - 1) // blk, (We + blk - 1) // blk, 3, generator=g, dtype=torch.float64)
        cls = cls.repeat_interleave(blk, 1).repeat_interleave(blk, 2)[:, :He, :We]
        u = uni(1, He, We, 3)
        if hdr:   # EnvLight: raw texels, scale 1: negative ones, ordinary ones, and a sun above 64 -- per channel independently
            opt.update(softplus=False, scale=1.0)
            d["env"] = torch.where(cls < 0.3, -5.0 + 4.5 * u, torch.where(cls < 0.65, 0.5 + 20.0 * u, 90.0 + 300.0 * u))
        else:     # softplus, x2, raw texels in +-40: 2 softplus(t) > 64 from t > 32; a few strongly negative texels (value ~ 0+)
            d["env"] = torch.where(cls < 0.5, -3.0 + 18.0 * u, 36.0 + 4.0 * u)
            d["env"] = torch.where(uni(1, He, We, 3) < 0.05, -40.0 + 30.0 * u, d["env"])
        lab[:] = "clamped_env"
        d["visibility"] = (uni(n, Ns, 1) > 0.15).double()
    elif name == "vector_scales":
        for sc, label in ((1e-13, "normals_1e-13"), (1e-5, "normals_1e-5"), (7.0, "normals_7"), (1e3, "normals_1e3")):
            idx = take(0.12, label)
            d["normals"][idx] = d["normals"][idx] * sc
        idx = take(0.1, "zero_corner")
        d["normals"][idx, torch.randint(0, 4, (idx.numel(),), generator=g)] = 0.0
        idx = take(0.15, "view_x3")
        d["viewdirs"][idx] = d["viewdirs"][idx] * 3.0
        idx = take(0.15, "dirs_x0.5")
        d["dirs"][idx] = d["dirs"][idx] * 0.5
    elif name == "material_ends":
        for val in (0.0, 1e-3, 1.0):
            idx = take(0.08, f"rough_{val:g}")
            d["roughness"][idx] = val
        idx = take(0.06, "base_0")
        d["base_color"][idx] = 0.0
        idx = take(0.06, "base_1")
        d["base_color"][idx] = 1.0
        idx = take(0.08, "vis_0.37")
        d["visibility"][idx] = 0.37
        idx = take(0.06, "vis_0")
        d["visibility"][idx] = 0.0
        idx = take(0.06, "area_0")
        d["areas"][idx] = 0.0
        idx = take(0.1, "area_varying")
        d["areas"][idx] = 4 * math.pi * uni(idx.numel(), Ns, 1)
        idx = take(0.06, "radiance_0")
        d["radiance"][idx] = 0.0
        idx = take(0.06, "radiance_1e4")
        d["radiance"][idx] = 1e4 * uni(idx.numel(), Ns, 3)
        # entries of the radiance cache that are NaN when the case runs with a radiance ratio (nan_to_num(cache * ratio, nan=0)), in
        # ordinary rows: [m, 3] = (row, sample, channel)
        k = min(6, int((lab == "ordinary").sum()))
        r_ = torch.from_numpy(np.nonzero(lab == "ordinary")[0][:k].copy())
        opt["nan_cache_entries"] = torch.stack([r_, torch.randint(0, Ns, (k,), generator=g), torch.randint(0, 3, (k,), generator=g)], dim=1)
    return d, lab.astype(str), opt
