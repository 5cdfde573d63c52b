"""Case table of the per-tile composite (csrc/render_fwd.hip, render_generic.hip, render_bwd.hip, render_bwd_plain.hip): blend decisions on
threshold ladders that are known bit for bit, and per-candidate gradients that have a closed form.

Why it can be exact.  The camera is cameras.make_camera(W, H, eye = (0, 0, 4)) with W and H odd; its matrices hold 0 and +-1 outside the
projection's diagonal, so a surfel with means3D = (0, 0, z) projects to exactly ((W - 1) / 2, (H - 1) / 2): the AXIS PIXEL.  There dx = dy = 0,
power = -0, G = 1 and alpha = min(0.99f, opacity) bit for bit, whatever the conic is; the transmittance chain of a stack of such surfels is a
sequence of fp32 roundings that numpy reproduces (chain32).  With the upstream gradient non-zero on the axis pixel only, and only in the colour
planes, every candidate's colour and opacity gradient has a closed form (closed_form64).

  axis_scene(...)    the scene: bwd_rows_cases._scene (tilted, elongated discs) with the means forced to (0, 0, 4 - z), the opacities exact fp32
                     and colors_precomp given.  sigma = 0 (the 0.3 px^2 low-pass alone: alpha = 0.19 opacity one pixel away) where only the
                     axis pixel may pass a threshold.  Surfel ids are shuffled against depth order; `rank[i]` is the list position of id i.
  chain32(op)        fp32 emulation of the reference's blend loop (forward.cu:541-560) on the axis pixel: the set that blends, n_contrib, every
                     T_k, the final T and the opacity plane's value 1.f - T.
  closed_form64(...) fp64: for the upstream colour gradient g on the axis pixel, s_k = c_k . g and w_k = alpha_k T_k,
                       dL/dcolor_k   = w_k g
                       dL/dopacity_k = s_k T_k - (sum_{j > k} w_j s_j + (bg . g) T_final) / (1 - alpha_k)
                     A_k, the same with absolute values (the scale one candidate's rounding errors live on), S = sum_k w_k |s_k| + |bg . g| T_final,
                     the pixel's colour and the sum of absolute values behind it.

ladder(c, n): c with n consecutive fp32 neighbours on either side (2 n + 1 values, c at index n).

Cases (`CASES`, built by build(name, variant, S, VS); every view is at most 31 x 31):
  alpha_axis        opacity over ladder(fp32(1 / 255), 16), sigma 0: a surfel blends exactly from index 16 on.  33 one-surfel views, and PACKED:
                    all 33 in one list in a seeded order in which ladder steps 14 | 15 (no blend) and 16 | 17 (blend) stand in an even and an
                    odd list position each -- the two slots of the forward's candidate pairs.
  clamp_axis        opacity over ladder(0.99f, 4) and 1.0f, one surfel: the opacity plane is min(0.99f, opacity), n_contrib 1.
  cutoff_axis       13 surfels of opacity 0.5 (T = 2^-13), one from ladder(0.1808f, 16), one opaque surfel behind: n_contrib is 14 through
                    ladder index 18, then 13.  `cutoff_mixed`: the same behind a front of 40 seeded opacities in [0.05, 0.3]; the ladder is centred
                    with chain32 by bisection on the first opacity whose T (1 - a) falls below 0.0001f -- there the product's rounding decides.
  cutoff_at(k)      k in 8, 9, 63, 64, 65, 128, 129: that crossing on list position k (1-based) behind a front of k - 1 surfels -- the blend batch,
                    the staging batch, the first and the second state dump.  Three steps: the last opacity that blends, the first that ends the
                    pixel, its successor.
  residues          alpha_axis (packed) and four steps of cutoff_axis around its switch at W = H = 2 c + 1, c = 0 .. 15, and 31 x 3: the axis pixel
                    on every lane row and column of an 8 x 8 sub-tile and in all four sub-tiles.
  alpha_off_axis    one surfel of sigma 3 at 17 x 17; the pixel under test is (cx + 3, cy + 2).  The ladder (32 either side) is centred on the
                    opacity at which the fp64 oracle's alpha crosses 1 / 255 there.  A step is UNDECIDED where |255 alpha64 - 1| <=
                    4 eps32 (1 + |power64|): the rounding of the power, a 1-ulp exp and the product.
  deep              stacks whose candidates blend on every pixel (sigma 16 at 17 x 17): n = 200 at alpha 2^-5, n = 1024 at 2^-7 (16 segments, no
                    termination), n = 700 at 2^-6 (the axis pixel ends at 584, inside the tenth segment).  g = (0.7, -0.4, 0.9), bg = 0.5.
  deep_mixed        n = 193, seeded opacities in [0.004, 0.1]; positions 63, 64 and 127 hold an opacity one ulp below fp32(1 / 255).

tests/test_composite_edge_inputs.py proves every claim on the CPU oracle; tests/test_gpu_composite_edges.py holds the kernels to the table."""
import functools

import numpy as np

import bwd_rows_cases as rc
from svgir_harness import cameras  # noqa: F401  (the camera of rc._scene)

F32 = np.float32
EPS32 = 2.0 ** -24                      # unit roundoff of fp32
ALPHA_MIN = F32(1.0) / F32(255.0)       # the kernels' (1.0f / 255.0f)
ALPHA_MAX = F32(0.99)
T_MIN = F32(0.0001)
T_CLAMP = F32(1 - 0.000001)             # forward.cu:671
G_UP = np.array([0.7, -0.4, 0.9], np.float32)
BG = 0.5
WIDTHS = (("svgss", 3, 8), ("rgss", 5, 0))
EXTRA_WIDTHS = (("svgss", 9, 72), ("rgss", 7, 0), ("rgss", 0, 0), ("svgss", 0, 0))      # run-time widths (render_generic.hip), no features
CUTOFF_AT = (8, 9, 63, 64, 65, 128, 129)
RESIDUE_SIZES = tuple((2 * c + 1, 2 * c + 1) for c in range(16)) + ((31, 3),)
DEEP = ((200, 2.0 ** -5), (1024, 2.0 ** -7), (700, 2.0 ** -6))
DEEP_SIGMA = 16.0
MIXED_N, MIXED_FAINT = 193, (63, 64, 127)
OFF_AXIS = (3, 2)


def wid(v, S, VS):
    return f"{v}_S{S}" + (f"_VS{VS}" if v == "svgss" else "")


def ladder(c, n):
    c = F32(c)
    up, dn = [c], [c]
    for _ in range(n):
        up.append(np.nextafter(up[-1], F32(np.inf)))
        dn.append(np.nextafter(dn[-1], F32(-np.inf)))
    return np.array(dn[:0:-1] + up, dtype=np.float32)


def axis_scene(W, H, z, opacity, sigma, variant, S, VS, colors=None, seed=0):
    """`z`: view depths, increasing: entry k is list position k of every tile the stack touches.  `colors` None keeps the SH colours."""
    assert W % 2 == 1 and H % 2 == 1
    z = np.asarray(z, np.float64)
    n = len(z)
    op = np.asarray(opacity, np.float32).reshape(n)
    sc = rc._scene(W, H, np.full(n, (W - 1) / 2.0), np.full(n, (H - 1) / 2.0), z, np.broadcast_to(np.asarray(sigma, np.float64), (n,)), op,
                   variant, S, seed)
    order = sc["order"]
    m = np.zeros((n, 3), np.float32)
    m[:, 2] = (rc.EYE[2] - z).astype(np.float32)
    assert (np.diff(F32(rc.EYE[2]) - m[:, 2]) > 0).all(), "depths must stay distinct in fp32"
    sc["means3D"] = np.ascontiguousarray(m[order])
    sc["opacities"] = np.ascontiguousarray(op[order].reshape(n, 1))
    if variant == "svgss":
        sc["vfeatures"] = np.random.default_rng(seed + 1).uniform(0, 1, size=(n, VS)).astype(np.float32)
    if colors is not None:
        sc["colors_precomp"] = np.ascontiguousarray(np.asarray(colors, np.float32).reshape(n, 3)[order])
        del sc["shs"]
        sc["sh_degree"] = 0
    sc["rank"] = order            # id i stands at list position rank[i]
    sc["axis"] = ((W - 1) // 2, (H - 1) // 2)
    return sc


def chain32(opacities):
    """The reference's blend loop on the axis pixel in fp32 (one rounding per operation, as the kernels and the fp32 oracle evaluate it)."""
    op = np.asarray(opacities, np.float32).reshape(-1)
    n = len(op)
    T = F32(1.0)
    passed, Tk, alpha = np.zeros(n, bool), np.full(n, np.nan, np.float32), np.minimum(ALPHA_MAX, op)
    last = 0
    for k in range(n):
        a = alpha[k]
        if a < ALPHA_MIN:
            continue
        test_T = F32(T * F32(F32(1.0) - a))
        if test_T < T_MIN:
            break
        passed[k], Tk[k] = True, T
        T = test_T
        last = k + 1
    Tc = min(T_CLAMP, T)
    return dict(passed=passed, n_contrib=last, T=Tk, alpha=alpha, T_final=Tc, opacity=F32(F32(1.0) - Tc))


def closed_form64(alpha, passed, colors, g=G_UP, bg=BG):
    a = np.where(passed, np.asarray(alpha, np.float64), 0.0)
    c = np.asarray(colors, np.float64).reshape(len(a), 3)
    g = np.asarray(g, np.float64)
    bgv = np.full(3, bg, np.float64) if np.ndim(bg) == 0 else np.asarray(bg, np.float64)
    T = np.concatenate([[1.0], np.cumprod(1.0 - a)])
    Tk, Tf = T[:-1], T[-1]
    w = a * Tk
    s = c @ g
    bgd = float(bgv @ g)
    ws, wa = w * s, w * np.abs(s)
    behind = np.concatenate([np.cumsum(ws[::-1])[::-1][1:], [0.0]]) + bgd * Tf
    behind_abs = np.concatenate([np.cumsum(wa[::-1])[::-1][1:], [0.0]]) + abs(bgd) * Tf
    dop = np.where(passed, s * Tk - behind / (1.0 - a), 0.0)
    A = np.where(passed, np.abs(s) * Tk + behind_abs / (1.0 - a), 0.0)
    return dict(dcolor=w[:, None] * g[None], dop=dop, A=A, S=float(wa.sum() + abs(bgd) * Tf), w=w, T=Tk, T_final=Tf,
                color=(w[:, None] * c).sum(0) + bgv * Tf, color_abs=(w[:, None] * np.abs(c)).sum(0) + np.abs(bgv) * Tf)


def upstream(sc, variant, pixel=None, g=G_UP):
    """dL/d(outputs): `g` in the colour planes of one pixel (the axis pixel unless given), exact zeros everywhere else."""
    H, W = sc["H"], sc["W"]
    x, y = sc["axis"] if pixel is None else pixel
    up = {k: np.zeros((c, H, W), np.float32) for k, c in (("color", 3), ("normal", 3), ("depth", 1), ("opacity", 1),
                                                            ("feature", sc["features"].shape[1]))}
    if variant == "svgss":
        up["vfeature"] = np.zeros((sc["vfeatures"].shape[1] // 4, H, W), np.float32)
    up["color"][:, y, x] = g
    return up


def _depths(n):
    return 3.0 + min(0.004, 0.8 / n) * np.arange(n)


def _colors(n, seed):
    return np.random.default_rng(seed).uniform(0.05, 1.0, size=(n, 3)).astype(np.float32)


def _view(name, W, H, op, sigma, variant, S, VS, seed, claims, colors=True):
    """One entry of a case: the scene, its opacities by list position, what chain32 predicts and what the table claims."""
    op = np.asarray(op, np.float32)
    n = len(op)
    col = _colors(n, 1000 + seed) if colors is True else colors
    sc = axis_scene(W, H, _depths(n), op, sigma, variant, S, VS, col, seed)
    return dict(name=name, sc=sc, op=op, colors=col, chain=chain32(op), claims=claims)


# ---- the ladders ------------------------------------------------------------------------------------------------------------------

def _packed_order():
    """A seeded order of the 33 ladder steps in which the steps next to the switch stand in both slots of a candidate pair."""
    for seed in range(1000):
        perm = np.random.default_rng(seed).permutation(33)      # perm[k]: the ladder step at list position k
        pos = np.argsort(perm)
        if {pos[14] % 2, pos[15] % 2} == {0, 1} and {pos[16] % 2, pos[17] % 2} == {0, 1}:
            return perm
    raise AssertionError


def alpha_axis(variant, S, VS, W=17, H=17):
    lad = ladder(ALPHA_MIN, 16)
    return [_view(f"step{i}", W, H, [lad[i]], 0.0, variant, S, VS, i, dict(blends=i >= 16)) for i in range(33)]


def alpha_axis_packed(variant, S, VS, W=17, H=17):
    lad, perm = ladder(ALPHA_MIN, 16), _packed_order()
    return [_view("packed", W, H, lad[perm], 0.0, variant, S, VS, 50, dict(blended=perm >= 16, perm=perm))]


def clamp_axis(variant, S, VS):
    ops = np.concatenate([ladder(ALPHA_MAX, 4), [F32(1.0)]])
    return [_view(f"step{i}", 17, 17, [o], 0.0, variant, S, VS, 60 + i, dict(opacity=min(ALPHA_MAX, o), n_contrib=1)) for i, o in enumerate(ops)]


CUTOFF_FRONT, CUTOFF_SWITCH = 13, 19      # the first ladder index that ends the pixel


def cutoff_axis(variant, S, VS, W=17, H=17, steps=None):
    lad = ladder(F32(0.1808), 16)
    out = []
    for i in (range(33) if steps is None else steps):
        op = np.concatenate([np.full(CUTOFF_FRONT, 0.5), [lad[i]], [0.99]])
        out.append(_view(f"step{i}", W, H, op, 0.0, variant, S, VS, 70, dict(n_contrib=CUTOFF_FRONT + (1 if i < CUTOFF_SWITCH else 0))))
    return out


def crossing(front):
    """The smallest fp32 opacity that, behind `front`, ends the axis pixel (T (1 - a) < 0.0001f), and its predecessor: bisection on chain32
    over the fp32 values between 1 / 255 and 0.99."""
    n = len(front)

    def ends(a):
        return chain32(np.concatenate([front, [a]]))["n_contrib"] == n
    lo, hi = ALPHA_MIN.view(np.int32), ALPHA_MAX.view(np.int32)     # positive floats order like their bit patterns
    assert not ends(ALPHA_MIN) and ends(ALPHA_MAX), "the front must leave the crossing inside (1 / 255, 0.99)"
    while hi - lo > 1:
        mid = np.int32((int(lo) + int(hi)) // 2)
        if ends(mid.view(np.float32)):
            hi = mid
        else:
            lo = mid
    return hi.view(np.float32)


MIXED_FRONT = 40


def _front(k, lo, hi, seed):
    return np.random.default_rng(seed).uniform(lo, hi, size=k).astype(np.float32)


def cutoff_mixed(variant, S, VS):
    front = _front(MIXED_FRONT, 0.05, 0.3, 81)
    lad = ladder(crossing(front), 16)
    out = []
    for i in range(33):
        op = np.concatenate([front, [lad[i]], [0.99]])
        out.append(_view(f"step{i}", 17, 17, op, 0.0, variant, S, VS, 82, dict(n_contrib=MIXED_FRONT + (1 if i < 16 else 0))))
    return out


def cutoff_at(k, variant, S, VS):
    """The crossing on list position k (1-based).  The front's opacities are scaled so that its T is about 5e-4: the crossing opacity is then
    near 0.8, inside (1 / 255, 0.99)."""
    a0 = 1.0 - (5e-4) ** (1.0 / (k - 1))
    front = (a0 * np.random.default_rng(90 + k).uniform(0.85, 1.15, size=k - 1)).astype(np.float32)
    lad = ladder(crossing(front), 1)
    out = []
    for i in range(3):
        op = np.concatenate([front, [lad[i]], [0.99]])
        out.append(_view(f"k{k}_step{i}", 17, 17, op, 0.0, variant, S, VS, 90 + k, dict(n_contrib=k - 1 + (1 if i < 1 else 0))))
    return out


def residues(W, H, variant, S, VS):
    return alpha_axis_packed(variant, S, VS, W, H) + cutoff_axis(variant, S, VS, W, H, steps=(17, 18, 19, 20))


# ---- the deep stacks --------------------------------------------------------------------------------------------------------------

def _signal_colors(alpha, passed, seed):
    """Seeded colours with which every blended candidate's closed-form |dL/dopacity_k| is at least 1e-3 A_k (reseeded until it holds), so that
    "non-zero" is an observation a test can make: the kernels' error on a candidate is a few eps32 A_k.  (A share of the tensor's maximum cannot
    be asked of a deep list: |dL/dopacity_k| <= A_k is proportional to T_k, which falls to 3e-4 there.)"""
    for s in range(seed, seed + 1000):
        col = _colors(len(alpha), s)
        cf = closed_form64(alpha, passed, col)
        if (np.abs(cf["dop"])[passed] >= 1e-3 * cf["A"][passed]).all():
            return col
    raise AssertionError


def deep(n, alpha, variant, S, VS):
    op = np.full(n, alpha, np.float32)
    ch = chain32(op)
    return [_view(f"deep{n}", 17, 17, op, DEEP_SIGMA, variant, S, VS, 200 + n, dict(n=n), colors=_signal_colors(ch["alpha"], ch["passed"], 3000 + n))]


def deep_mixed(variant, S, VS):
    op = np.random.default_rng(193).uniform(0.004, 0.1, size=MIXED_N).astype(np.float32)
    op[list(MIXED_FAINT)] = np.nextafter(ALPHA_MIN, F32(0.0))
    ch = chain32(op)
    return [_view("deep_mixed", 17, 17, op, DEEP_SIGMA, variant, S, VS, 393, dict(faint=MIXED_FAINT),
                  colors=_signal_colors(ch["alpha"], ch["passed"], 3193))]


# ---- off the axis -----------------------------------------------------------------------------------------------------------------

def off_axis_scene(variant, S, VS, opacity):
    return axis_scene(17, 17, [3.0], [opacity], 3.0, variant, S, VS, _colors(1, 77), seed=3)


def off_axis_pixel(sc):
    return sc["axis"][0] + OFF_AXIS[0], sc["axis"][1] + OFF_AXIS[1]


def off_axis_alpha64(o, sc, opacity):
    """(power, alpha) of the pixel under test in fp64, from an fp64 oracle run `o` of the scene."""
    xy = o.get("means2D").reshape(-1, 2)[0].astype(np.float64)
    co = o.get("conic_opacity").reshape(-1, 4)[0].astype(np.float64)
    px, py = off_axis_pixel(sc)
    dx, dy = xy[0] - px, xy[1] - py
    power = -0.5 * (co[0] * dx * dx + co[2] * dy * dy) - co[1] * dx * dy
    return power, min(0.99, float(np.float64(F32(opacity))) * np.exp(power))


def undecided(power64, alpha64):
    return abs(alpha64 * 255.0 - 1.0) <= 4.0 * EPS32 * (1.0 + abs(power64))


# ---- the table --------------------------------------------------------------------------------------------------------------------

AXIS_CASES = {"alpha_axis": alpha_axis, "alpha_axis_packed": alpha_axis_packed, "clamp_axis": clamp_axis, "cutoff_axis": cutoff_axis,
              "cutoff_mixed": cutoff_mixed, "deep_mixed": deep_mixed}
AXIS_CASES.update({f"cutoff_at{k}": functools.partial(cutoff_at, k) for k in CUTOFF_AT})
AXIS_CASES.update({f"deep{n}": functools.partial(deep, n, a) for n, a in DEEP})
AXIS_CASES.update({f"residues_{w}x{h}": functools.partial(residues, w, h) for w, h in RESIDUE_SIZES})
EXTRA_CASES = ("alpha_axis_packed", "cutoff_axis", "deep200")
VALUE_CASES = tuple(f"deep{n}" for n, _ in DEEP) + ("deep_mixed",)
FUSED_CASES = ("alpha_axis_packed", "cutoff_axis", "deep_mixed")
# (case, variant, S, VS): every case at the two specialised widths, three of them at the run-time widths and without features
TABLE = [(c,) + w for c in AXIS_CASES for w in WIDTHS] + [(c,) + w for c in EXTRA_CASES for w in EXTRA_WIDTHS]
VALUE_TABLE = [(c,) + w for c in VALUE_CASES for w in WIDTHS] + [("deep200",) + w for w in EXTRA_WIDTHS]


def table_id(t):
    return f"{t[0]}-{wid(*t[1:])}"


@functools.lru_cache(maxsize=None)
def build(name, variant, S, VS):
    """The views of a case (built once, shared, never modified)."""
    return AXIS_CASES[name](variant, S, VS)


# ---- the CPU oracle on the table (shared by the CPU and the GPU tests) ---------------------------------------------------------------

def by_position(sc, x):
    """A per-surfel array (indexed by id) in list order."""
    x = np.asarray(x)
    out = np.empty_like(x)
    out[sc["rank"]] = x
    return out


def oracle_run(sc, variant, fp64=False, up=None):
    """One oracle evaluation of a scene: the axis-pixel facts, and (with `up`) the opacity and colour gradients in list order."""
    from oracle import oracle as orc
    o = orc.OracleRun(sc, orc.SVGSS if variant == "svgss" else orc.RGSS, fp64=fp64)
    R = o.forward()
    H, W = sc["H"], sc["W"]
    n = sc["means3D"].shape[0]
    res = dict(R=R, means2D=o.get("means2D").reshape(n, -1)[:, :2].copy(), n_contrib=o.get("n_contrib").reshape(H, W).astype(np.int64),
               opacity=o.get("out_opac").reshape(H, W).copy(), color=o.get("out_color").reshape(3, H, W).copy(),
               blended=by_position(sc, o.get("out_weights").reshape(n) > 0), run=o)
    if up is not None:
        o.backward(up["color"], up["normal"], up["depth"], up["opacity"], up["feature"], up.get("vfeature"))
        res["dop"] = by_position(sc, o.get("dL_dopacity").reshape(n).astype(np.float64))
        res["dcolor"] = by_position(sc, o.get("dL_dcolor").reshape(n, 3).astype(np.float64))
    return res


@functools.lru_cache(maxsize=None)
def value_host(name, variant, S, VS):
    """A value case on the host: the view, its closed form, and what the reference's own fp32 arithmetic loses on it -- E32 = max_k
    |oracle32 - closed|_k / A_k for dL/dopacity, E32c = max |oracle32 - closed| / (w_k |g_ch|) for dL/dcolor."""
    v = build(name, variant, S, VS)[0]
    ch = v["chain"]
    cf = closed_form64(ch["alpha"], ch["passed"], v["colors"])
    o32 = oracle_run(v["sc"], variant, up=upstream(v["sc"], variant))
    p = ch["passed"]
    E32 = float((np.abs(o32["dop"] - cf["dop"])[p] / cf["A"][p]).max())
    E32c = float((np.abs(o32["dcolor"] - cf["dcolor"])[p] / (cf["w"][p, None] * np.abs(np.float64(G_UP))[None])).max())
    o32.pop("run")
    return v, cf, o32, E32, E32c


def with_sh(sc, seed=5):
    """The scene with SH colours instead of colors_precomp (the fused shading's rasterizer call takes `shs`)."""
    out = {k: v for k, v in sc.items() if k != "colors_precomp"}
    out["sh_degree"] = 3
    out["shs"] = np.random.default_rng(seed).normal(0, 0.3, size=(sc["means3D"].shape[0], 16, 3)).astype(np.float32)
    return out
