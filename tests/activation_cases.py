"""Case table, oracles and tolerances of the fused activation getters (csrc/activate.hip, svgir_harness/activations.py), shared by
tests/test_activation_edge_inputs.py (CPU) and tests/test_gpu_activations.py (GPU).

    eager_activate(raw, campos, base_color_scale, want, normal_reg)
        the reference's own lines (scene/gaussian_model.py:270-355, gaussian_renderer/svgss.py:109, :316) in their operation order as a
        torch function on any device and dtype.  In fp32 on the CPU it is `ref32`: what the reference's arithmetic loses (E32 / G32).
    oracle(case, upstream)
        torch fp64 on the CPU, written from the same lines, with the project's one decision explicit: where nan_to_num replaced a value
        (a scaling element whose exp is NaN or overflows fp32, a NaN roughness element, a whole rotation row whose norm is not finite) the
        raw element gets ZERO gradient, where torch's autograd gives NaN.  Everything else is autograd: a NaN opacity / base_color / offset
        / position gives NaN, upstream NaNs pass through, an absent upstream gradient is an output outside the graph.
        Returns values, gradients, Aabs (per raw element, the sum of the absolute values of the terms its gradient is the sum of: the
        adjoint with every local derivative and every upstream gradient replaced by its absolute value, `oracle_aabs`) and the decision
        masks.

Bounds (the GPU test):  value |kernel - oracle| <= 4 max(E32[output], eps32) |oracle| + FLT_MIN
                        grad  |kernel - oracle| <= 4 max(G32[raw], eps32) Aabs + FLT_MIN
4 x what the reference's own fp32 arithmetic loses is the project's margin, eps32 the floor any fp32 result has, FLT_MIN covers
denormal flushing.  E32[output] = max over the table of |ref32 - oracle| / max(|oracle|, FLT_MIN); G32[raw] = max of
(|ref32 gradient - oracle| - FLT_MIN)+ / Aabs, i.e. the smallest constant with which ref32 itself meets the bound's form; decision,
threshold and NaN elements excluded.  Both are measured by test_activation_edge_inputs.py::test_e32_g32_tables, which fails when a
constant below is smaller than what it measures (measured values: DESIGN.md).

Threshold elements: a `_scaling` within 1e-3 of ln(FLT_MAX) = 88.7228 -- its exp may or may not overflow fp32.  Its value must be the
clamped (FLT_MAX) or the unclamped oracle value, its gradient finite.  Only the case `threshold` holds such elements."""
import functools
import math

import numpy as np
import torch

F = torch.nn.functional
EPS32 = float(np.finfo(np.float32).eps)
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)
LN_FLT_MAX = math.log(FLT_MAX)
C6, C8 = float(np.float32(1e-6)), float(np.float32(1e-8))    # the fp32 constants a replaced element holds
WG = 256                                                      # the kernel's workgroup: one lane per surfel

RAW = ("xyz", "scaling", "rotation", "opacity", "normal", "base_color", "roughness")
WIDTH = {"xyz": 3, "scaling": 3, "rotation": 4, "opacity": 1, "normal": 12, "base_color": 12, "roughness": 4}
OUTPUTS = ("scales", "rotations", "opacities", "geo_normal", "shading_normal", "shading_normal12", "base_color", "roughness", "viewdirs")
STAGE1 = ("scales", "rotations", "opacities", "geo_normal", "viewdirs")       # no material inputs
READS = {"scales": ("scaling",), "rotations": ("rotation",), "opacities": ("opacity",), "geo_normal": ("rotation",),
         "shading_normal": ("rotation", "normal"), "shading_normal12": ("rotation", "normal"), "base_color": ("base_color",),
         "roughness": ("roughness",), "viewdirs": ("xyz",)}

# Measured by test_e32_g32_tables (the measured values: DESIGN.md, "Activation getters"); each constant is about twice its measurement,
# room for another CPU's libm and vector width.  geo_normal and the shading normals lose most: 1 - 2 (x x + y y) and x z + r y cancel in
# fp32, and the relative error of a component near zero is what E32 records.  The sigmoids' gradients lose 1 - s for large |x|; an offset's
# gradient inherits the forward error of a shading-normal component near zero wherever its own upstream term is absent (sparse cases).
E32 = {"scales": 2.4e-7, "rotations": 2.8e-7, "opacities": 6.4e-6, "geo_normal": 2.2e-2, "shading_normal": 1.6e-2, "shading_normal12": 1.6e-2,
       "base_color": 4.5e-7, "roughness": 4e-7, "viewdirs": 3.6e-7, "normal_reg": 3.7e-7}
G32 = {"xyz": 8e-7, "scaling": 2.4e-7, "rotation": 3.4e-7, "opacity": 1.3e-4, "normal": 1.6e-3, "base_color": 1.2e-5, "roughness": 1.4e-5}


# ---- the reference's lines ----------------------------------------------------------------------------------------------------------
def eager_activate(raw, campos=None, base_color_scale=None, want=OUTPUTS, normal_reg=False):
    """GaussianModel's getters, render_view's viewdirs and the normal regulariser, line by line (any device, any float dtype).  A tensor
    the lines go on to read (the rotation for geo_normal, geo_normal for the shading normals) is returned as a view of itself: a gradient
    retained on an output is then what the output's consumers sent, not that plus the lines' own."""
    out = {}
    want = tuple(want)
    if "scales" in want:
        out["scales"] = torch.nan_to_num(torch.exp(raw["scaling"]), nan=1e-6)
    if any(k in want for k in ("rotations", "geo_normal", "shading_normal", "shading_normal12")):
        rot = torch.nan_to_num(F.normalize(raw["rotation"]), nan=1e-6)
        if "rotations" in want:
            out["rotations"] = rot.view_as(rot)
        r, x, y, z = rot.split(1, -1)                      # utils/general_utils.py:231-239 quaternion2rotmat
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape([len(rot), 3, 3])
        geo = R[..., 2]
        if "geo_normal" in want:
            out["geo_normal"] = geo.view_as(geo)
        if "shading_normal" in want or "shading_normal12" in want:
            g4 = geo[:, None].repeat(1, 4, 1)
            off = raw["normal"].reshape(-1, 3, 4).transpose(1, 2)
            sn = F.normalize(g4 + off, dim=-1)
            if "shading_normal" in want:
                out["shading_normal"] = sn.view_as(sn)
            if "shading_normal12" in want:
                out["shading_normal12"] = sn.transpose(1, 2).reshape(-1, 12)   # get_radiance_loss
    if "opacities" in want:
        out["opacities"] = torch.sigmoid(raw["opacity"])
    if "base_color" in want:
        b = raw["base_color"]
        scale = torch.ones(3, dtype=b.dtype, device=b.device) if base_color_scale is None else base_color_scale
        out["base_color"] = (torch.sigmoid(b) * 0.77 + 0.03) * scale[None, :].repeat_interleave(repeats=4, dim=1)
    if "roughness" in want:
        out["roughness"] = torch.nan_to_num(torch.sigmoid(raw["roughness"]) * 0.9 + 0.09, nan=1e-8)
    if "viewdirs" in want:
        out["viewdirs"] = F.normalize(campos - raw["xyz"], dim=-1)
    if normal_reg:
        out["normal_reg"] = F.mse_loss(raw["normal"], torch.zeros_like(raw["normal"]))
    return out


# ---- the fp64 oracle ----------------------------------------------------------------------------------------------------------------
def decision_masks(raw):
    """Per raw group the elements the zero-gradient decision covers (fp32 inputs, torch tensors)."""
    m = {k: torch.zeros(raw[k].shape, dtype=torch.bool) for k in raw}
    if "scaling" in raw:
        e = torch.exp(raw["scaling"].double())
        m["scaling"] = torch.isnan(e) | torch.isinf(e.float())             # NaN, or an exp that overflows fp32
    if "rotation" in raw:
        n = torch.sqrt((raw["rotation"].double() ** 2).sum(-1, keepdim=True))
        m["rotation"] = (~torch.isfinite(n)).expand_as(raw["rotation"]).clone()
    if "roughness" in raw:
        m["roughness"] = torch.isnan(raw["roughness"])
    return m


def threshold_mask(scaling):
    return (scaling.double() - LN_FLT_MAX).abs() <= 1e-3


def oracle_outputs(lv, campos, bcs, want, normal_reg):
    """fp64 outputs of the fp64 leaves `lv`; where the decision applies, the replaced constant is not connected to the leaf."""
    out = {}
    if "scales" in want:
        s = lv["scaling"]
        e = torch.exp(s.detach())
        nan, over = torch.isnan(e), torch.isinf(e.float()) & ~torch.isnan(e)
        v = torch.exp(torch.where(nan | over, torch.zeros_like(s), s))
        out["scales"] = torch.where(nan, torch.full_like(v, 1e-6), torch.where(over, torch.full_like(v, FLT_MAX), v))
    if any(k in want for k in ("rotations", "geo_normal", "shading_normal", "shading_normal12")):
        q = lv["rotation"]
        qd = q.detach()
        n = torch.sqrt((qd * qd).sum(-1, keepdim=True))
        bad = ~torch.isfinite(n)
        const = torch.nan_to_num(qd / n, nan=1e-6)                       # finite / inf = 0, inf / inf = NaN -> 1e-6
        qs = torch.where(bad, torch.ones_like(q), q)
        u = qs / torch.linalg.vector_norm(qs, dim=-1, keepdim=True).clamp_min(1e-12)     # (its backward is 0 at the zero vector)
        u = torch.where(bad, const, u)
        if "rotations" in want:
            out["rotations"] = u
        r, x, y, z = u.unbind(-1)
        geo = torch.stack([2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)], -1)
        if "geo_normal" in want:
            out["geo_normal"] = geo.view_as(geo)
        if "shading_normal" in want or "shading_normal12" in want:
            w = geo[:, None, :] + lv["normal"].reshape(-1, 3, 4).transpose(1, 2)
            sn = w / torch.linalg.vector_norm(w, dim=-1, keepdim=True).clamp_min(1e-12)
            if "shading_normal" in want:
                out["shading_normal"] = sn
            if "shading_normal12" in want:
                out["shading_normal12"] = sn.transpose(1, 2).reshape(-1, 12)
    if "opacities" in want:
        out["opacities"] = torch.sigmoid(lv["opacity"])
    if "base_color" in want:
        v = torch.sigmoid(lv["base_color"]) * 0.77 + 0.03
        out["base_color"] = v if bcs is None else v * bcs[None, :].repeat_interleave(4, dim=1)
    if "roughness" in want:
        r = lv["roughness"]
        nan = torch.isnan(r.detach())
        v = torch.sigmoid(torch.where(nan, torch.zeros_like(r), r)) * 0.9 + 0.09
        out["roughness"] = torch.where(nan, torch.full_like(v, 1e-8), v)
    if "viewdirs" in want:
        w = campos[None, :] - lv["xyz"]
        out["viewdirs"] = w / torch.linalg.vector_norm(w, dim=-1, keepdim=True).clamp_min(1e-12)
    if normal_reg:
        out["normal_reg"] = (lv["normal"] ** 2).mean()
    return out


def oracle(raw, campos=None, bcs=None, upstream=None, want=OUTPUTS, normal_reg=False, g_reg=None):
    """raw: dict of fp32 CPU tensors (the groups the requested outputs read).  upstream: dict output name -> fp32 tensor (absent = outside
    the graph); g_reg: python float, the gradient of normal_reg.  Returns dict(values, grads, aabs, decision)."""
    want = tuple(want)
    lv = {k: v.detach().double().clone().requires_grad_(True) for k, v in raw.items()}
    c64 = None if campos is None else campos.double()
    b64 = None if bcs is None else bcs.double()
    out = oracle_outputs(lv, c64, b64, want, normal_reg)
    res = {"values": {k: v.detach() for k, v in out.items()}, "decision": decision_masks(raw)}
    if upstream is None and g_reg is None:
        return res
    upstream = upstream or {}
    names = [k for k in want if upstream.get(k) is not None]
    terms = [(out[k] * upstream[k].double().reshape(out[k].shape)).sum() for k in names]
    if g_reg is not None:
        terms.append(out["normal_reg"] * float(g_reg))
    keys = list(lv)
    gr = torch.autograd.grad(sum(terms), [lv[k] for k in keys], retain_graph=True, allow_unused=True)
    res["grads"] = {k: (torch.zeros_like(lv[k]) if g is None else g) for k, g in zip(keys, gr)}
    res["aabs"] = aabs = oracle_aabs(lv, out, c64, b64, upstream, names, g_reg)
    for k, m in res["decision"].items():
        if k in aabs:
            assert float(res["grads"][k][m].abs().sum()) == 0.0, k     # the decision, explicit: exactly zero
            aabs[k][m] = 0.0
    return res


def _abs_normalize(u, m, a_u):
    """|adjoint| of u = w / max(|w|, 1e-12): the absolute contributions a_u [.., n] make to every component of w."""
    den = m.clamp_min(1e-12)
    through_norm = u.abs() * (a_u * u.abs()).sum(-1, keepdim=True) / den
    return a_u / den + torch.where(m < 1e-12, torch.zeros_like(through_norm), through_norm)


def oracle_aabs(lv, out, campos, bcs, upstream, names, g_reg):
    """Per raw element the sum of the ABSOLUTE values of the terms its gradient is the sum of: the oracle's adjoint with every local
    derivative and every upstream gradient replaced by its absolute value (no term cancels another).  NaN terms count as 0."""
    nn = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)  # noqa: E731
    up = {k: nn(upstream[k].double().reshape(out[k].shape).abs()) for k in names}
    raw = {k: v.detach() for k, v in lv.items()}
    aabs = {k: torch.zeros_like(v) for k, v in raw.items()}
    val = {k: nn(v.detach()) for k, v in out.items()}
    if "scales" in up:
        aabs["scaling"] = up["scales"] * val["scales"]
    sig_abs = lambda x: nn(torch.sigmoid(x) * torch.sigmoid(-x))  # noqa: E731
    if "opacities" in up:
        aabs["opacity"] = up["opacities"] * sig_abs(raw["opacity"])
    if "base_color" in up:
        sc = 1.0 if bcs is None else bcs[None, :].repeat_interleave(4, dim=1).abs()
        aabs["base_color"] = up["base_color"] * 0.77 * sig_abs(raw["base_color"]) * sc
    if "roughness" in up:
        aabs["roughness"] = up["roughness"] * 0.9 * sig_abs(raw["roughness"])
    if "viewdirs" in up:
        w = nn(campos[None, :] - raw["xyz"])
        aabs["xyz"] = _abs_normalize(val["viewdirs"], torch.linalg.vector_norm(w, dim=-1, keepdim=True), up["viewdirs"])
    if any(k in up for k in ("rotations", "geo_normal", "shading_normal", "shading_normal12")):
        q = nn(raw["rotation"])
        n = torch.linalg.vector_norm(q, dim=-1, keepdim=True)
        u = q / n.clamp_min(1e-12)
        r, x, y, z = [t.abs() for t in u.unbind(-1)]
        a_geo = torch.zeros(q.shape[0], 3, dtype=torch.float64)
        if "shading_normal" in up or "shading_normal12" in up:
            a_sn = torch.zeros(q.shape[0], 4, 3, dtype=torch.float64)
            if "shading_normal" in up:
                a_sn = a_sn + up["shading_normal"]
            if "shading_normal12" in up:
                a_sn = a_sn + up["shading_normal12"].reshape(-1, 3, 4).transpose(1, 2)
            geo = torch.stack([2 * (u[:, 1] * u[:, 3] + u[:, 0] * u[:, 2]), 2 * (u[:, 2] * u[:, 3] - u[:, 0] * u[:, 1]),
                               1 - 2 * (u[:, 1] ** 2 + u[:, 2] ** 2)], -1)
            w = geo[:, None, :] + nn(raw["normal"]).reshape(-1, 3, 4).transpose(1, 2)
            m = torch.linalg.vector_norm(w, dim=-1, keepdim=True)
            a_w = _abs_normalize(w / m.clamp_min(1e-12), m, a_sn)
            aabs["normal"] = a_w.transpose(1, 2).reshape(-1, 12)
            a_geo = a_geo + a_w.sum(1)
        if "geo_normal" in up:
            a_geo = a_geo + up["geo_normal"]
        a0, a1, a2 = a_geo.unbind(-1)
        a_u = torch.stack([2 * (y * a0 + x * a1), 2 * (z * a0 + r * a1) + 4 * x * a2, 2 * (r * a0 + z * a1) + 4 * y * a2,
                           2 * (x * a0 + y * a1)], -1)
        if "rotations" in up:
            a_u = a_u + up["rotations"]
        aabs["rotation"] = _abs_normalize(u, n, a_u)
    if g_reg is not None:
        aabs["normal"] = aabs["normal"] + nn((2.0 * raw["normal"] / raw["normal"].numel() * float(g_reg)).abs())
    return aabs


def value_bound(name, ref):
    return 4 * max(E32[name], EPS32) * ref.abs() + FLT_MIN


def grad_bound(name, aabs):
    return 4 * max(G32[name], EPS32) * aabs + FLT_MIN


def mismatches(got, ref, bound, exclude=None):
    """Number of elements where got and ref differ beyond `bound`, NaN positions included (they must coincide)."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.double()
    bad = torch.isnan(got) != torch.isnan(ref)
    fin = ~torch.isnan(ref) & ~torch.isnan(got)
    bad |= fin & ~((got - ref).abs() <= bound)
    if exclude is not None:
        bad &= ~exclude
    return int(bad.sum()), bad


# ---- the case table -----------------------------------------------------------------------------------------------------------------
CAMPOS = (0.3, -0.2, 2.5)


def _random_rows(P, g):
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return {"xyz": 0.8 * rnd(P, 3), "scaling": -3.0 + rnd(P, 3), "rotation": rnd(P, 4) * torch.exp(rnd(P, 1)), "opacity": 2.0 * rnd(P, 1),
            "normal": 0.1 * rnd(P, 12), "base_color": rnd(P, 12), "roughness": rnd(P, 4)}


def edge_rows(nan_offset=True):
    """(raw rows, labels): one dedicated row (or a few) per edge of the arithmetic.  Every row is ordinary except for what its label names.
    nan_offset=False leaves out the row with a NaN normal offset, the one row that turns normal_reg into NaN."""
    g = torch.Generator().manual_seed(99)
    nan, inf = float("nan"), float("inf")
    rows = []

    def row(label, **over):
        d = {k: v[0] for k, v in _random_rows(1, g).items()}
        for k, v in over.items():
            d[k] = v(d[k].clone()) if callable(v) else torch.tensor(v, dtype=torch.float32)
        rows.append((label, d))

    def put(idx, val):
        def f(t):
            t[idx] = val
            return t
        return f
    row("ordinary")
    row("scaling_nan", scaling=put(1, nan))
    row("scaling_all_nan", scaling=[nan, nan, nan])
    row("scaling_+100", scaling=put(0, 100.0))
    row("scaling_-100", scaling=put(2, -100.0))
    row("scaling_+inf", scaling=put(1, inf))
    row("scaling_-inf", scaling=put(0, -inf))
    row("quat_zero", rotation=[0.0, 0.0, 0.0, 0.0])
    row("quat_1e-20", rotation=[1e-20, -2e-20, 0.5e-20, 1e-20])
    row("quat_1e-6", rotation=[1e-6, 2e-6, -1.5e-6, 0.5e-6])     # (no component of its geo_normal cancels to zero)
    row("quat_nan", rotation=put(2, nan))
    row("quat_inf", rotation=put(1, inf))
    row("quat_-inf", rotation=put(3, -inf))
    row("quat_unit", rotation=[0.5, 0.5, 0.5, 0.5])
    row("quat_identity", rotation=[1.0, 0.0, 0.0, 0.0])
    row("opacity_+100", opacity=[100.0])
    row("opacity_-100", opacity=[-100.0])
    row("opacity_nan", opacity=[nan])
    row("base_color_sat", base_color=lambda t: torch.where(torch.arange(12) % 2 == 0, torch.tensor(100.0), torch.tensor(-100.0)))
    row("base_color_nan", base_color=put(5, nan))
    row("roughness_sat", roughness=[100.0, -100.0, 100.0, -100.0])
    row("roughness_nan", roughness=put(2, nan))
    row("offsets_zero", normal=[0.0] * 12)
    # geo_normal of (1, 0, 0, 0) is (0, 0, 1) exactly, of (.5, .5, .5, .5) it is (1, 0, 0): corner 2's offset cancels it exactly
    row("offset_cancels_geo", rotation=[1.0, 0.0, 0.0, 0.0], normal=lambda t: put(slice(2, 12, 4), torch.tensor([0.0, 0.0, -1.0]))(t))
    row("offset_cancels_geo_x", rotation=[0.5, 0.5, 0.5, 0.5], normal=lambda t: put(slice(1, 12, 4), torch.tensor([-1.0, 0.0, 0.0]))(t))
    row("offsets_1e3", normal=lambda t: t * 1e4)
    if nan_offset:
        row("offset_nan", normal=put(6, nan))
    row("xyz_at_campos", xyz=list(CAMPOS))
    row("xyz_nan", xyz=put(0, nan))
    raw = {k: torch.stack([d[k] for _, d in rows]) for k in RAW}
    return raw, np.array([lab for lab, _ in rows])


def threshold_rows():
    s = torch.tensor([[LN_FLT_MAX, -3.0, LN_FLT_MAX - 9e-4], [LN_FLT_MAX + 9e-4, LN_FLT_MAX - 5e-4, -2.0], [-4.0, LN_FLT_MAX + 4e-4, -3.0]])
    return s.float()


CASES = ("p1", "p255", "p256", "p257", "p512", "p5000", "edges", "edges_scaled", "threshold")


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(raw fp32 tensors, campos [3], bcs [3] | None, labels, upstream fp32 per output, g_reg)."""
    g = torch.Generator().manual_seed(500 + CASES.index(name))
    er, el = edge_rows(nan_offset=name in ("edges", "p257"))     # (normal_reg stays finite in the other cases)
    E = el.shape[0]
    if name.startswith("p"):
        P = int(name[1:])
        raw = _random_rows(P, g)
        labels = np.array(["ordinary"] * P, dtype=object)
        if P >= 255:   # the edge rows straddle the first workgroup's end
            at = WG - E // 2 if P > WG + E else P - E
            for k in RAW:
                raw[k][at:at + E] = er[k]
            labels[at:at + E] = el
        bcs = None if P % 2 else torch.tensor([1.0, 0.5, 2.0])
    elif name in ("edges", "edges_scaled"):
        raw, labels = {k: v.clone() for k, v in er.items()}, el
        bcs = torch.tensor([1.0, 0.5, 2.0]) if name == "edges_scaled" else None
    else:
        P = 40
        raw = _random_rows(P, g)
        raw["scaling"][5:8] = threshold_rows()
        labels = np.array(["ordinary"] * P, dtype=object)
        labels[5:8] = "threshold"
        bcs = None
    P = raw["xyz"].shape[0]
    shapes = {"scales": (P, 3), "rotations": (P, 4), "opacities": (P, 1), "geo_normal": (P, 3), "shading_normal": (P, 4, 3),
              "shading_normal12": (P, 12), "base_color": (P, 12), "roughness": (P, 4), "viewdirs": (P, 3)}
    up = {k: torch.randn(*s, generator=g) for k, s in shapes.items()}
    if name in ("p512", "edges_scaled"):   # sparse upstream gradients, as a view that sees part of the surfels sends: where a component's
        for k in up:                       # own term is absent, what is left of its gradient carries the forward error of the others
            up[k] = up[k] * (torch.rand(up[k].shape, generator=g) < 0.3)
    if name == "threshold":   # (an unclamped element's gradient g exp(s) is representable in fp32 only for |g| < 1)
        up["scales"] = torch.rand(P, 3, generator=g) - 0.5
    if name == "edges":   # an upstream NaN passes through (into the first, ordinary, row)
        up["opacities"][0, 0] = float("nan")
        up["base_color"][0, 3] = float("nan")
    return dict(name=name, raw=raw, campos=torch.tensor(CAMPOS), bcs=bcs, labels=np.asarray(labels).astype(str), upstream=up, g_reg=0.1 * 0.73)


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    c = case(name)
    return oracle(c["raw"], c["campos"], c["bcs"], c["upstream"], OUTPUTS, True, c["g_reg"])


@functools.lru_cache(maxsize=None)
def case_ref32(name):
    """ref32: the reference's lines in fp32 on the CPU, values and autograd gradients (NaN where torch gives NaN)."""
    c = case(name)
    lv = {k: v.clone().requires_grad_(True) for k, v in c["raw"].items()}
    out = eager_activate(lv, c["campos"], c["bcs"], OUTPUTS, True)
    loss = sum((out[k] * c["upstream"][k].reshape(out[k].shape)).sum() for k in OUTPUTS) + out["normal_reg"] * np.float32(c["g_reg"])
    gr = torch.autograd.grad(loss, [lv[k] for k in RAW])
    return {"values": {k: v.detach() for k, v in out.items()}, "grads": dict(zip(RAW, gr))}
