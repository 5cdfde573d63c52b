"""The edge-case scenes of svgir_harness.scenes build the cases they are named for -- checked on the fp32 oracle's own state (no GPU).

tests/test_gpu_edge_cases.py runs the same scenes through the HIP path; these tests make sure that what it covers is really there:
indefinite conics whose overflowing exp shares an 8x8 sub-tile with blending pixels, exact list lengths and termination ranks at the
composite kernels' batch / segment boundaries, bit-identical depths, and the most edge-on surfels the visibility cull admits.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from svgir_harness import scenes

EXP_OVERFLOW = 88.7    # exp(power) is inf in fp32 above ~88.72


def _run(sc, variant):
    o = orc.OracleRun(sc, orc.SVGSS if variant == "svgss" else orc.RGSS)
    o.forward()
    return o


def _powers(o, sc, g, variant):
    """Power and alpha of Gaussian g at every pixel of the tiles its rectangle touches, in the oracle's fp32 operation order
    (svgir_oracle.cpp pair_alpha); returns (px, py, power, blends)."""
    W, H = sc["W"], sc["H"]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    m = o.get("means2D").reshape(-1, 2)[g]
    a, b, c, op = o.get("conic_opacity").reshape(-1, 4)[g]
    r = float(o.get("radii")[g])
    f = np.float32
    x0 = min(gx, max(0, int((m[0] - r) / 16))); x1 = min(gx, max(0, int((m[0] + r + 15) / 16)))
    y0 = min(gy, max(0, int((m[1] - r) / 16))); y1 = min(gy, max(0, int((m[1] + r + 15) / 16)))
    px, py = np.meshgrid(np.arange(16 * x0, min(W, 16 * x1)), np.arange(16 * y0, min(H, 16 * y1)))
    dx, dy = f(m[0]) - px.astype(f), f(m[1]) - py.astype(f)
    if variant == "svgss":
        pw = f(-0.5) * ((a * dx * dx + c * dy * dy) + f(2) * b * dx * dy)
    else:
        pw = f(-0.5) * (a * dx * dx + c * dy * dy) - b * dx * dy
    with np.errstate(over="ignore"):
        alpha = np.minimum(f(0.99), op * np.exp(pw.astype(np.float64)))
    return px, py, pw, (pw <= 0) & (alpha >= 1.0 / 255.0)


def _conic_det(o):
    co = o.get("conic_opacity").reshape(-1, 4).astype(np.float64)
    return co[:, 0] * co[:, 2] - co[:, 1] ** 2     # same sign as det(cov2D)


@pytest.mark.parametrize("variant", ["svgss", "rgss"])
def test_indefinite_scene_overflows_next_to_blending_pixels(variant):
    """Every added Gaussian has det < 0, blends pixels, and shares an 8x8 sub-tile between a blending pixel and one with power > 88.7:
    the (pixel, splat) pairs whose non-finite exp the svgss backward must keep out of the sub-tile's gradient row."""
    kw = dict(S=3, VS=8) if variant == "svgss" else dict(S=5, VS=0)
    sc = scenes.indefinite_conic_scene(variant, **kw)
    o = _run(sc, variant)
    P, n = sc["means3D"].shape[0], sc["n_indefinite"]
    det = _conic_det(o)
    assert n >= 40 and (det[P - n:] < 0).all() and (o.get("radii")[P - n:] > 0).all()
    assert (det[:P - n] > 0).all()
    pl = o.get("point_list")[:o.num_rendered]
    for g in range(P - n, P):
        px, py, pw, bl = _powers(o, sc, g, variant)
        assert bl.sum() >= 1, g
        sub = (py // 8) * 1000 + px // 8
        both = [s for s in np.unique(sub) if bl[sub == s].any() and (pw[sub == s] > EXP_OVERFLOW).any()]
        assert both, f"Gaussian {g}: no sub-tile holds both a blending and an overflowing pixel"
        assert (pl == g).any()
    # the same blend decisions in fp64 (the gradient anchor): no pixel near power 0 or the 1/255 threshold
    o64 = orc.OracleRun(sc, orc.SVGSS if variant == "svgss" else orc.RGSS, fp64=True)
    assert o64.forward() == o.num_rendered
    assert np.array_equal(o64.get("n_contrib"), o.get("n_contrib"))


def test_edge_on_scene_conditioning():
    """The edge-on surfels survive the cull and carry the worst-conditioned projected covariances the scene can make.  fp32 det < 0
    is NOT reached: the visibility cull (p.n > -0.01 is culled) keeps |cos(view ray, normal)| >= 0.01 / |p| ~ 0.03 at depth <= 0.35,
    so the conditioning |det| / (ca cc) ~ cos^2 stays above ~1e-3 (largest reached: 1.4e-3), far from fp32 cancellation (~1e-7).
    The indefinite scene constructs det < 0 directly."""
    for variant in ("svgss", "rgss"):
        kw = dict(S=3, VS=8) if variant == "svgss" else dict(S=5, VS=0)
        sc = scenes.edge_on_near_scene(variant, **kw)
        o = _run(sc, variant)
        P, n = sc["means3D"].shape[0], sc["n_edge"]
        vis = o.get("radii")[P - n:] > 0
        assert vis.sum() >= 0.9 * n
        co = o.get("conic_opacity").reshape(-1, 4).astype(np.float64)[P - n:][vis]
        cond = np.abs(co[:, 0] * co[:, 2] - co[:, 1] ** 2) / np.abs(co[:, 0] * co[:, 2])
        assert cond.min() < 3e-3, cond.min()
        assert (_conic_det(o)[P - n:][vis] > 0).all()
        assert o.get("radii")[P - n:].max() > 1000    # major axes of ~1e5-1e6 px^2


@pytest.mark.parametrize("variant", ["svgss", "rgss"])
def test_stack_scene_hits_every_list_length(variant):
    sc = scenes.stack_scene(variant)
    o = _run(sc, variant)
    rg = o.get("ranges").reshape(-1, 2).astype(np.int64)
    nc = o.get("n_contrib").reshape(sc["H"], sc["W"])
    pl = o.get("point_list")[:o.num_rendered]
    lens = rg[:, 1] - rg[:, 0]
    assert set(scenes.STACK_COUNTS) <= set(int(x) for x in lens)
    for t, n, tie in zip(sc["stack_tiles"], sc["stack_counts"], sc["tie_blocks"]):
        assert lens[t] == n, (t, lens[t], n)
        assert (nc[:, 16 * t:16 * t + 16] == n).all(), (t, np.unique(nc[:, 16 * t:16 * t + 16]))   # every pixel blends all n
        lst = pl[rg[t, 0]:rg[t, 1]]
        pos = np.nonzero(np.isin(lst, tie))[0]
        assert len(tie) == min(n, scenes.STACK_TIE) and len(pos) == len(tie)
        assert (np.diff(pos) == 1).all() and (np.diff(lst[pos].astype(np.int64)) > 0).all()   # consecutive, stable (index) order
        if n >= 70:
            assert pos[0] < 64 <= pos[-1]       # the tied block straddles the first segment boundary
    d = o.get("depths")
    for tie in sc["tie_blocks"]:
        assert np.unique(d[tie].astype(np.float32)).size == 1
    # the tiles in between hold the neighbouring stacks' tails: lengths that are not the stacks'
    between = lens[np.setdiff1d(np.arange(len(lens)), sc["stack_tiles"])]
    assert len(set(between.tolist()) - set(scenes.STACK_COUNTS)) >= 10


@pytest.mark.parametrize("variant", ["svgss", "rgss"])
def test_stack_scene_terminates_at_the_boundaries(variant):
    """Forced termination: the last contributor of some pixel falls on and next to 64 and 128 (T < 1e-4 before / at / after them)."""
    sc = scenes.stack_scene(variant, terminate=True)
    o = _run(sc, variant)
    nc = o.get("n_contrib").reshape(sc["H"], sc["W"])
    seen = set(int(x) for x in np.unique(nc))
    assert {63, 64, 65, 127, 128, 129} <= seen, sorted(seen)
    rg = o.get("ranges").reshape(-1, 2)
    for t, n in zip(sc["stack_tiles"], sc["stack_counts"]):
        assert rg[t, 1] - rg[t, 0] == n
        assert (nc[:, 16 * t:16 * t + 16] < n).any()   # some pixels stop early


def test_frustum_extras_project_beyond_the_clamp():
    sc = scenes.surface_scene(P=2000, W=160, H=120, seed=91, sh_degree=1, variant="svgss", S=3, VS=8, scale_lo=0.01, scale_hi=0.05)
    scenes.frustum_extras(sc, "svgss", seed=5, n_side=16)
    o = _run(sc, "svgss")
    P, m = sc["means3D"].shape[0], sc["n_frustum"]
    rad, mu = o.get("radii")[P - m:], o.get("means2D").reshape(-1, 2)[P - m:]
    assert (rad > 0).all()
    W, H = sc["W"], sc["H"]
    side = mu[:16]
    tx = np.abs(side[:, 0] - (W - 1) / 2) / (W / 2)       # |x / z| / tan(fov_x / 2)
    ty = np.abs(side[:, 1] - (H - 1) / 2) / (H / 2)
    beyond = np.maximum(tx, ty)
    assert (beyond > 1.33).all() and (beyond < 1.39).all(), beyond    # clear of the 1.3 clamp and of svgss's 1.4 margin
    d = o.get("depths")[P - 3:]
    assert (d > 0.205).all() and (d < 0.26).all()
    assert (rad[-3:] > max(W, H)).all()
