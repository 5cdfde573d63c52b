"""Scenes for the two per-surfel kernels every view runs -- csrc/preprocess.hip (forward) and csrc/geom_bwd.hip (backward) -- and for
csrc/grad_reduce.hip between them.  Seeded builders, no GPU; tests/test_surfel_edge_inputs.py proves on the CPU oracle that each scene
holds what it is built for, tests/test_gpu_surfel_edges.py holds the kernels to them.

  lattice(variant, M, D)   one surfel per 16 x 16 tile of a 128 x 128 image, centred on it, tilted and elongated (bwd_rows_cases._scene),
                           longest axis 3.3 sigma <= 8 px, opacity 0.5 - 0.8: no pixel blends two surfels, so every per-Gaussian gradient
                           is a short sum over one tile and can be compared ELEMENT BY ELEMENT.  `M` is the stride of a coefficient row,
                           `D` the active degree; shs[:, nk:] (nk = (D + 1)^2) is N(0, 0.3) like the rest -- a kernel that reads above
                           the active degree shows -- and the DC terms are set so that each of the 8 clamp masks occurs 8 times.
                           Rows of one rasterizer and one D share geometry and leading coefficients: (M, D) and (nk, D) must give the same
                           images and gradients.  LATTICE_ROWS adds `offset`: the floats by which the GPU test shifts the shs view inside
                           its storage (buf[offset:].view(P, M, 3)); 1 and 2 floats break the 16-byte alignment geom_bwd's vector paths need.
  coop_rows(variant)       M 16 / D 3 on a 256 x 128 lattice, P = 512: the four 128-index spans (one two-chunk wave of geom_bwd_kernel<2>
                           each) hold 1, 30, 31 and 66 blended surfels -- the cooperative row copy (5 rows per step, CR = 6 steps in
                           registers) with one row, exactly 30, 30 + 1 in the tail loop, and a second pass with 2.
  clamp_ladder(variant, c) a D 0 lattice whose first 33 surfels carry, in channel c, the 33 consecutive fp32 DC values around the one
                           where fl(fl(kC0 s) + 0.5f) changes sign (a result of exactly 0.0f is NOT clamped).
  cull_ladder(kind, v)     33 overlapping surfels, one parameter stepping through consecutive fp32 values across one decision of the
                           preprocess (CULL_KINDS); the flip is located by bisection on the fp32 oracle.  Forward only.  (`backface`
                           tilts the surfel: `dot` moves ~100 ulps per step.  `backface_exact` moves the surfel along the view axis
                           under a normal of exactly -z: dot = -z, and the last culled value is 0.01f itself, which a comparison in
                           float instead of double would keep.)
  listed(variant, P)       the lattice with 6 faint tiles and three wide translucent surfels to its right (> 16 tiles each): 58 + 3 =
                           61 blended surfels -- odd, no multiple of 4: the blended list ends inside a wave of grad_reduce_kernel<2> and
                           <4> --, every other surfel behind the camera; the visible ones sit on the wave and chunk ends of
                           csrc/subset.hip.  P walks the list thresholds of api.hip and the GK thresholds of grad_reduce.hip.
"""
import functools

import numpy as np

import bwd_rows_cases as br
from oracle import oracle as orc
from svgir_harness import cameras, scenes

F32 = np.float32
EPS = float(np.finfo(np.float32).eps)
TINY = float(np.finfo(np.float32).tiny)
WIDTHS = {"rgss": (5, 0), "svgss": (3, 8)}     # (S, VS)
VARIANTS = ("rgss", "svgss")
FAINT = 0.002                                   # opacity below 1/255: a radius, never a blend weight
MAXM = 25
# (M, D, offset)
LATTICE_ROWS = ((1, 0, 0), (4, 0, 0), (4, 1, 0), (9, 1, 0), (9, 2, 0), (16, 0, 0), (16, 1, 0), (16, 2, 0), (16, 3, 0), (16, 1, 1),
                (16, 3, 1), (16, 3, 2), (17, 3, 0), (25, 2, 0))
PER_SURFEL = ("means2D", "colors", "opacity", "means3D", "features", "vfeatures", "cov3D", "sh", "scales", "rotations")

KC0, KC1 = 0.28209479177387814, 0.4886025119029199
KC2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
KC3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
       -0.5900435899266435)


def nk_of(D):
    return (D + 1) * (D + 1)


def view_dirs(sc):
    """Unit vectors camera -> surfel, fp64, from the fp32 inputs the kernels read."""
    d = sc["means3D"].astype(np.float64) - np.asarray(sc["campos"], np.float64)[None]
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def sh_basis(dirs):
    """(cf, A): the 16 SH basis values of each direction in fp64, and per value the sum of the absolute monomials it is made of (what
    its fp32 evaluation's rounding errors scale with: 2zz - xx - yy cancels, 2zz + xx + yy does not)."""
    x, y, z = dirs.T
    xx, yy, zz = x * x, y * y, z * z
    a = np.abs
    one = np.ones_like(x)
    terms = [  # (constant, signed bracket, absolute bracket)
        (KC0, one, one), (-KC1, y, a(y)), (KC1, z, a(z)), (-KC1, x, a(x)),
        (KC2[0], x * y, a(x * y)), (KC2[1], y * z, a(y * z)), (KC2[2], 2 * zz - xx - yy, 2 * zz + xx + yy), (KC2[3], x * z, a(x * z)),
        (KC2[4], xx - yy, xx + yy),
        (KC3[0], y * (3 * xx - yy), a(y) * (3 * xx + yy)), (KC3[1], x * y * z, a(x * y * z)),
        (KC3[2], y * (4 * zz - xx - yy), a(y) * (4 * zz + xx + yy)), (KC3[3], z * (2 * zz - 3 * xx - 3 * yy), a(z) * (2 * zz + 3 * xx + 3 * yy)),
        (KC3[4], x * (4 * zz - xx - yy), a(x) * (4 * zz + xx + yy)), (KC3[5], z * (xx - yy), a(z) * (xx + yy)),
        (KC3[6], x * (xx - 3 * yy), a(x) * (xx + 3 * yy))]
    cf = np.stack([c * s for c, s, _ in terms], -1)
    A = np.stack([abs(c) * m for c, _, m in terms], -1)
    return cf, A


def quat_rot(q):
    """(R, absR) of UN-normalised (r, x, y, z) quaternions as the kernels build them (no normalisation, quirk Q3), fp64: R[p, i, j] with
    column j the surfel's j-th axis; absR: the sum of the absolute monomials of each entry."""
    r, x, y, z = q.astype(np.float64).T
    a = np.abs
    one = np.ones_like(r)
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                  np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                  np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], axis=1)
    A = np.stack([np.stack([one + 2 * (y * y + z * z), 2 * (a(x * y) + a(r * z)), 2 * (a(x * z) + a(r * y))], -1),
                  np.stack([2 * (a(x * y) + a(r * z)), one + 2 * (x * x + z * z), 2 * (a(y * z) + a(r * x))], -1),
                  np.stack([2 * (a(x * z) + a(r * y)), 2 * (a(y * z) + a(r * x)), one + 2 * (x * x + y * y)], -1)], axis=1)
    return R, A


def scale_grad_from_cov(sc, dcov):
    """(dL_dscale[:, :2], sum of absolute terms) from dL_dcov3D [P, 6] by the formula of geom_bwd.hip (cov3D -> scale), in fp64:
    Sigma = sum_j s_j^2 r_j r_j^T, so dL/ds_j = 2 s_j r_j^T dSigma r_j with dSigma the symmetric matrix whose off-diagonal entries are
    half the stored ones.  The absolute sum expands every entry of R into its monomials (quat_rot)."""
    R, A = quat_rot(sc["rotations"])
    s = float(sc.get("scale_modifier", 1.0)) * sc["scales"].astype(np.float64)
    d = dcov.astype(np.float64)
    dS = np.stack([np.stack([d[:, 0], 0.5 * d[:, 1], 0.5 * d[:, 2]], -1), np.stack([0.5 * d[:, 1], d[:, 3], 0.5 * d[:, 4]], -1),
                   np.stack([0.5 * d[:, 2], 0.5 * d[:, 4], d[:, 5]], -1)], axis=1)
    val = 2 * s[:, :2] * np.einsum("paj,pab,pbj->pj", R, dS, R)[:, :2]
    mag = 2 * np.abs(s[:, :2]) * np.einsum("paj,pab,pbj->pj", A, np.abs(dS), A)[:, :2]
    return val, mag


def oracle(sc, variant, fp64=False, grads=None):
    o = orc.OracleRun(sc, orc.SVGSS if variant == "svgss" else orc.RGSS, fp64=fp64)
    o.forward()
    if grads is not None:
        o.backward(grads["color"], grads["normal"], grads["depth"], grads["opacity"], grads["feature"], grads.get("vfeature"))
    return o


def row_deviation(a, ref):
    """Per surfel (first axis): max |a - ref| over the surfel's row of this tensor, over the row's max |ref| -- THE normalisation of
    the element-wise comparisons (the oracle hands out no per-element sum of absolute pixel contributions).  A row whose reference is all
    zero must be all zero: its deviation is 0 then, inf otherwise."""
    P = ref.shape[0]
    a, ref = np.asarray(a, np.float64).reshape(P, -1), np.asarray(ref, np.float64).reshape(P, -1)
    d, m = np.abs(a - ref).max(1), np.abs(ref).max(1)
    return np.where(m > 0, d / np.where(m > 0, m, 1.0), np.where(d > 0, np.inf, 0.0))


def e32(g32, g64, rows):
    """{tensor: the fp32 oracle's largest row_deviation from the fp64 oracle over the surfels `rows`}."""
    out = {}
    for k in PER_SURFEL:
        if k in g64 and g64[k].size:
            out[k] = float(row_deviation(g32[k], g64[k])[rows].max())
    return out


# ---- lattices ---------------------------------------------------------------------------------------------------------------------

def _attrs(sc, variant, seed):
    """Feature rows at the widths of WIDTHS (bwd_rows_cases._scene builds VS = 0 / degree 3)."""
    rng = np.random.default_rng(seed)
    P = len(sc["means3D"])
    S, VS = WIDTHS[variant]
    sc["features"] = rng.uniform(0, 1, size=(P, S)).astype(F32)
    sc.pop("vfeatures", None)
    if variant == "svgss":
        sc["vfeatures"] = rng.uniform(0, 1, size=(P, VS)).astype(F32)
    sc.pop("shs", None)
    return sc


def lattice_shs(sc, D, seed, masks=None):
    """[P, MAXM, 3] fp32 coefficients, all N(0, 0.3), DC terms solved so that the colour of channel c is -0.15 ... -0.45 (clamped) where
    bit c of the surfel's mask is set and 0.25 ... 0.75 where not.  One draw per (seed, D): every M takes its leading columns."""
    rng = np.random.default_rng(seed)
    P = len(sc["means3D"])
    full = rng.normal(0, 0.3, size=(P, MAXM, 3)).astype(F32)
    if masks is None:
        masks = rng.permutation(P) % 8
    nk = nk_of(D)
    cf, _ = sh_basis(view_dirs(sc))
    hi = np.einsum("pk,pkc->pc", cf[:, 1:nk], full[:, 1:nk].astype(np.float64))
    bit = (masks[:, None] >> np.arange(3)[None]) & 1
    target = np.where(bit == 1, -rng.uniform(0.15, 0.45, size=(P, 3)), rng.uniform(0.25, 0.75, size=(P, 3)))
    full[:, 0] = ((target - 0.5 - hi) / KC0).astype(F32)
    return full, masks


def _grid(gx, gy, seed, faint=(), u0=0.0):
    n = gx * gy
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    op = rng.uniform(0.5, 0.8, n)
    op[list(faint)] = FAINT
    return u0 + 16.0 * (t % gx) + 7.5, 16.0 * (t // gx) + 7.5, rng.uniform(2.5, 3.5, n), np.full(n, 1.4), op


@functools.lru_cache(maxsize=None)
def lattice(variant, M, D, offset=0, faint=(), colors=False):
    """(module docstring).  `colors`: colors_precomp instead of SH coefficients.  The returned dict is shared: do not modify it."""
    seed = 500 + VARIANTS.index(variant)
    u, v, z, sig, op = _grid(8, 8, seed, faint)
    sc = _attrs(br._scene(128, 128, u, v, z, sig, op, variant, WIDTHS[variant][0], seed, shuffle=False), variant, seed + 10)
    sc["sh_degree"] = D
    if colors:
        sc["colors_precomp"] = np.random.default_rng(seed + 20).uniform(0.05, 0.95, size=(64, 3)).astype(F32)
        sc["sh_degree"] = 0
    else:
        full, masks = lattice_shs(sc, D, seed + 30 + D)
        sc["shs"] = np.ascontiguousarray(full[:, :M])
        sc["masks"] = masks
    sc["offset"] = offset
    sc["blended"] = op > 0.1
    return sc


def twin_of(M, D, offset):
    """The lattice row a row must reproduce: without the storage shift, else at the stride of exactly the active coefficients."""
    if offset:
        return (M, D, 0)
    return (nk_of(D), D, 0) if M > nk_of(D) else None


COOP_SPANS = (1, 30, 31, 66)


@functools.lru_cache(maxsize=None)
def coop_rows(variant):
    """(module docstring) 128 blended surfels, one per tile; per span 4 faint ones (on tiles of blended surfels: they blend
    nowhere) and the rest behind the camera."""
    seed = 520 + VARIANTS.index(variant)
    rng = np.random.default_rng(seed)
    P = 512
    kind = np.full(P, "c")
    for j, n in enumerate(COOP_SPANS):
        slots = 128 * j + rng.permutation(128)
        kind[slots[:n]] = "b"
        kind[slots[n:n + 4]] = "f"
    b = np.nonzero(kind == "b")[0]
    tile = np.zeros(P, np.int64)
    tile[b] = rng.permutation(128)
    f = np.nonzero(kind == "f")[0]
    tile[f] = tile[b][rng.integers(0, 128, len(f))]
    tile[kind == "c"] = rng.integers(0, 128, int((kind == "c").sum()))
    op = rng.uniform(0.5, 0.8, P)
    op[f] = FAINT
    z = rng.uniform(2.5, 3.5, P)
    z[kind == "c"] *= -1.0     # behind the camera
    sc = _attrs(br._scene(256, 128, 16.0 * (tile % 16) + 7.5, 16.0 * (tile // 16) + 7.5, z, np.full(P, 1.4), op, variant,
                          WIDTHS[variant][0], seed, shuffle=False), variant, seed + 10)
    sc["scales"] = np.abs(sc["scales"])     # (_scene scales the footprint by the view depth, negative behind the camera)
    full, masks = lattice_shs(sc, 3, seed + 30)
    sc["shs"] = np.ascontiguousarray(full[:, :16])
    sc["sh_degree"], sc["masks"], sc["kinds"], sc["blended"], sc["offset"] = 3, masks, kind, kind == "b", 0
    return sc


def sh_zero_crossing():
    """The largest fp32 DC value s whose colour fl(fl(kC0 s) + 0.5f) is negative, and the fp32 values next to it whose colour is exactly
    0.0f (kC0 s rounds to -0.5 for them; the sum with 0.5f is exact by Sterbenz's lemma)."""
    k = F32(KC0)
    col = lambda s: F32(F32(k * F32(s)) + F32(0.5))
    a, b = F32(-1.8), F32(-1.7)     # colour(a) < 0 <= colour(b)
    assert col(a) < 0 <= col(b)
    while True:
        ia, ib = int(a.view(np.int32)), int(b.view(np.int32))     # (negative floats: the larger bit pattern is the smaller value)
        if ia - ib == 1:
            break
        m = np.array((ia + ib) // 2, np.int32).view(F32)[()]
        if col(m) < 0:
            a = m
        else:
            b = m
    zeros = []
    s = b
    while col(s) == 0:
        zeros.append(s)
        s = np.nextafter(s, F32(0))
    return a, zeros


@functools.lru_cache(maxsize=None)
def clamp_ladder(variant, channel):
    """(module docstring) surfel i < 33 has DC value `last negative` + (i - 16) ulps in `channel`; everything else is a D 0 lattice."""
    sc = dict(lattice(variant, 1, 0))
    a, zeros = sh_zero_crossing()
    vals = (int(a.view(np.int32)) - (np.arange(33) - 16)).astype(np.int32).view(F32)     # ascending values
    shs = sc["shs"].copy()
    shs[:33, 0, channel] = vals
    sc["shs"] = shs
    sc["ladder"], sc["ladder_zeros"], sc["channel"] = vals, np.array(zeros, F32), channel
    return sc


# ---- cull ladders -----------------------------------------------------------------------------------------------------------------

CULL_KINDS = {   # kind: rasterizers
    "near": ("rgss",), "backface": VARIANTS, "backface_exact": ("svgss",), "grazing0": VARIANTS, "grazing1": VARIANTS,
    "patch_x0": ("svgss",), "patch_x1": ("svgss",), "patch_y0": ("svgss",), "patch_y1": ("svgss",),
    "left": VARIANTS, "right": VARIANTS, "top": VARIANTS, "bottom": VARIANTS,
    "radius3": VARIANTS, "radius8": VARIANTS, "radius300": VARIANTS}
CULL_CASES = tuple((k, v) for k, vs in CULL_KINDS.items() for v in vs)
LADDER_W, LADDER_H = 160, 128
PATCH = (32.0, 48.0, 96.0, 128.0)     # (y0, x0, y1, x1): w = 80, h = 64 -- the culls are at x 32 / 144, y 19.2 / 108.8


def _identity_camera(W, H):
    """A camera whose view matrix is the identity (x right, y down, z forward, eye at the origin): view space IS world space, so
    pv.z is the z coordinate and every product with the view matrix is exact."""
    cam = cameras.make_camera(W, H, np.array([0.0, 0.0, -1.0]))
    fovy = 2 * np.arctan(cam["tanfovy"])
    Pm = cameras.projection_matrix(0.01, 100.0, cameras.TENSOIR_FOVX, fovy)
    cam["viewmatrix"] = np.eye(4, dtype=F32)
    cam["projmatrix"] = np.ascontiguousarray(Pm.T.astype(F32))
    cam["campos"] = np.zeros(3, F32)
    return cam


def _ladder_scene(variant, pos, quat, scale, seed=0):
    """n surfels given by fp32 arrays pos [n, 3], quat [n, 4], scale [n, 3] (used as they are: consecutive fp32 values stay
    consecutive), opacity 0.05 (33 of them on one pixel leave T = 0.18: no early termination), SH degree 0."""
    n = len(pos)
    rng = np.random.default_rng(600 + seed)
    sc = {"sh_degree": 0, "bg": np.full(3, 0.5, dtype=F32), "config": np.array([1.0, 1.0, 1.0], dtype=F32), "scale_modifier": 1.0,
          "backward_geometry": True, "computer_pseudo_normal": False}
    sc.update(_identity_camera(LADDER_W, LADDER_H))
    sc["means3D"], sc["rotations"], sc["scales"] = (np.ascontiguousarray(x, F32) for x in (pos, quat, scale))
    sc["opacities"] = np.full((n, 1), 0.05, F32)
    sc["shs"] = rng.normal(0, 0.3, size=(n, 1, 3)).astype(F32)
    return _attrs_keep_shs(sc, variant, 610 + seed)


def _attrs_keep_shs(sc, variant, seed):
    shs = sc["shs"]
    _attrs(sc, variant, seed)
    sc["shs"] = shs
    return sc


FACING = (0.0, 1.0, 0.0, 0.0)     # half a turn about x: the surfel normal is -z, towards the camera of _identity_camera


def _ladder_parts(kind, variant):
    """(make(values) -> scene, lo, hi, decide(oracle) -> bool array) of a kind: `values` is the fp32 parameter per surfel, lo / hi two
    values with different decisions."""
    cam = _identity_camera(LADDER_W, LADDER_H)
    fx, fy = scenes._focal(cam)
    visible = lambda o: o.get("radii") > 0

    def unproj(u, v, z):
        return float((u - (LADDER_W - 1) / 2.0) * z / fx), float((v - (LADDER_H - 1) / 2.0) * z / fy)

    def scene(n, x, y, z, quat=FACING, sx=2.4, sy=2.4, patch=None, wx=None):
        """sx, sy: the footprint's sigmas in pixels (without the 0.3 px^2 low-pass) -> world scales at depth z; wx: scale x as given"""
        one = np.ones(n, F32)
        zz = np.asarray(z, F32) * one
        pos = np.stack([np.asarray(x, F32) * one, np.asarray(y, F32) * one, zz], -1)
        q = np.stack([np.asarray(c, F32) * one for c in quat], -1)
        sc3 = np.stack([F32(sx) * zz / F32(fx) if wx is None else np.asarray(wx, F32), F32(sy) * zz / F32(fx), F32(0.01) * one], -1)
        sc = _ladder_scene(variant, pos, q, sc3, seed=list(CULL_KINDS).index(kind))
        if patch is not None:
            sc["patch_bbox"] = np.array(patch, F32)
        return sc

    if kind == "near":     # pv.z <= 0.2f
        x, y = unproj(60.3, 70.7, 0.2)
        return lambda v: scene(len(v), x, y, v), 0.19, 0.21, visible
    if kind == "backface":     # (double)dot > -0.01: tilt about x at depth 0.5 (|c / m| = 0.02 there: the grazing cull stays out of it)
        x, y = unproj(85.0, 56.0, 0.5)
        return lambda v: scene(len(v), x, y, 0.5, quat=(0.7, v, 0.0, 0.0)), 0.70, 0.78, visible
    if kind == "backface_exact":     # the same cull where `dot` IS the parameter: the normal is exactly -z, so dot = -z in every bit, and z
        x, y = unproj(85.0, 56.0, 0.01)     # steps across 0.01f -- (double)(-0.01f) > -0.01 culls the surfel at z = 0.01f, a comparison in float would not
        return lambda v: scene(len(v), x, y, v), 0.009, 0.011, visible
    if kind == "grazing0":     # |c0 / m0| < 0.01: tilt about x at depth 2 (dot = -0.02 there); the normal's x is 0 and its y negative, so c1 < c0 < 0
        x, y = unproj(90.6, 41.8, 2.0)
        return lambda v: scene(len(v), x, y, 2.0, quat=(0.7, v, 0.0, 0.0)), 0.70, 0.80, visible
    if kind == "grazing1":     # |c1 / m1| < 0.01: tilt about y the other way: the normal's x is negative, its y 0, so c0 < c1 < 0
        x, y = unproj(90.6, 41.8, 2.0)
        return lambda v: scene(len(v), x, y, 2.0, quat=(0.7, 0.0, v, 0.0)), -0.62, -0.80, visible
    if kind.startswith("patch_"):     # pix < x0 - 0.2 w, pix >= x1 + 0.2 w (and in y)
        axis, end = kind[6], kind[7]
        at = {"x0": 32.0, "x1": 144.0, "y0": 19.2, "y1": 108.8}[axis + end]
        inside = 1.0 if end == "0" else -1.0
        if axis == "x":
            y = unproj(0.0, 70.0, 2.0)[1]
            return (lambda v: scene(len(v), v, y, 2.0, patch=PATCH)), unproj(at - inside, 0, 2.0)[0], unproj(at + inside, 0, 2.0)[0], visible
        x = unproj(90.0, 0.0, 2.0)[0]
        return (lambda v: scene(len(v), x, v, 2.0, patch=PATCH)), unproj(0, at - inside, 2.0)[1], unproj(0, at + inside, 2.0)[1], visible
    if kind in ("left", "right", "top", "bottom"):     # the tile rectangle becomes empty; radius 8 (3 sqrt(2.4^2 + 0.3) = 7.4)
        at = {"left": -7.0, "top": -7.0, "right": LADDER_W + 8.0, "bottom": LADDER_H + 8.0}[kind]     # px + r across 1, (px - r) / 16 across gx
        out = -1.0 if kind in ("left", "top") else 1.0
        if kind in ("left", "right"):
            y = unproj(0.0, 50.0, 2.0)[1]
            return (lambda v: scene(len(v), v, y, 2.0)), unproj(at + out, 0, 2.0)[0], unproj(at - out, 0, 2.0)[0], visible
        x = unproj(70.0, 0.0, 2.0)[0]
        return (lambda v: scene(len(v), x, v, 2.0)), unproj(0, at + out, 2.0)[1], unproj(0, at - out, 2.0)[1], visible
    if kind.startswith("radius"):     # ceilf(3 sqrt(lambda)) from r to r + 1: lambda = (fx s / z)^2 + 0.3 (the other axis: 0.1 px)
        r = int(kind[6:])
        x, y = unproj(80.3, 64.4, 2.0)
        s0 = np.sqrt((r / 3.0) ** 2 - 0.3) * 2.0 / fx
        return (lambda v: scene(len(v), x, y, 2.0, wx=v, sy=0.1)), 0.95 * s0, 1.05 * s0, (lambda o: o.get("radii") > r)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def cull_ladder(kind, variant):
    """(module docstring) sc["ladder"]: the parameter per surfel; sc["decision"]: what the fp32 oracle decides per surfel (True: visible /
    the larger radius); sc["flip"]: the decision changes between surfel flip and flip + 1 of a one-surfel probe sequence (16 / 17);
    sc["monotone"]: the 33-surfel scene's decisions change exactly once, there."""
    make, lo, hi, decide = _ladder_parts(kind, variant)
    probe = lambda v: bool(decide(oracle(make(np.array([v], F32)), variant))[0])
    a, b = F32(lo), F32(hi)
    fa, fb = probe(a), probe(b)
    assert fa != fb, (kind, variant, a, b, fa)
    assert (a > 0) == (b > 0) and a != 0 and b != 0
    while True:
        ia, ib = int(a.view(np.int32)), int(b.view(np.int32))
        if abs(ia - ib) == 1:
            break
        m = np.array((ia + ib) // 2, np.int32).view(F32)[()]
        if probe(m) == fa:
            a = m
        else:
            b = m
    step = 1 if ib > ia else -1
    vals = (ia + step * (np.arange(33) - 16)).astype(np.int32).view(F32)     # a is surfel 16, b surfel 17
    sc = make(vals)
    dec = decide(oracle(sc, variant))
    sc["ladder"], sc["decision"], sc["flip"], sc["kind"] = vals, dec, 16, kind
    sc["monotone"] = bool((dec[:17] == fa).all() and (dec[17:] == fb).all())
    sc["decide"] = decide
    return sc


# ---- list sizes -------------------------------------------------------------------------------------------------------------------

# api.hip: the blended list (geom_bwd_kernel<1>, grad_reduce with a list) starts at kListMinPRows = 50 000 (svgss) / kListMinP = 400 000
# (rgss); grad_reduce.hip: grad_reduce_kernel<2> from P >= 500 000, <4> from P >= 1 000 000
LISTED_P = {"svgss": (49_999, 50_000, 500_000, 1_000_000), "rgss": (399_999, 400_000)}
LISTED_W, LISTED_H = 288, 128     # the lattice, a 32 px gap (the wide surfels' alpha falls below 1/255 in it), the second 128 x 128 region
LISTED_FAINT = (10, 13, 27, 36, 45, 60)
LISTED_ENDS = (0, 63, 64, 2047, 2048, 4095, 4096)     # ... and P - 1: wave ends, the 2 048-surfel chunk ends of csrc/subset.hip


@functools.lru_cache(maxsize=None)
def _listed_core(variant, M, D):
    """The 67 surfels with a radius: 64 lattice surfels (6 of them faint), 3 wide ones (sigma 16 px, opacity 0.05 - 0.1)."""
    seed = 540 + VARIANTS.index(variant)
    rng = np.random.default_rng(seed)
    u, v, z, sig, op = _grid(8, 8, seed, LISTED_FAINT)
    u = np.concatenate([u, 224.0 + rng.uniform(-6.0, 6.0, 3)])
    v = np.concatenate([v, 64.0 + rng.uniform(-6.0, 6.0, 3)])
    z = np.concatenate([z, [2.2, 2.3, 2.4]])
    sig = np.concatenate([sig, np.full(3, 16.0)])
    op = np.concatenate([op, rng.uniform(0.05, 0.1, 3)])
    sc = _attrs(br._scene(LISTED_W, LISTED_H, u, v, z, sig, op, variant, WIDTHS[variant][0], seed, shuffle=False), variant, seed + 10)
    full, masks = lattice_shs(sc, D, seed + 30)
    sc["shs"] = np.ascontiguousarray(full[:, :M])
    sc["sh_degree"] = D
    return sc, op > 0.01


def listed_where(P):
    """Indices of the 67 core surfels in a model of P: core surfels 0 ... 7 (blended) on LISTED_ENDS and P - 1, the others seeded."""
    rng = np.random.default_rng(77)
    pool = np.setdiff1d(np.arange(1, 49_998), np.array(LISTED_ENDS))
    rest = rng.choice(pool, size=67 - 8, replace=False)
    return np.concatenate([np.array(LISTED_ENDS + (P - 1,)), rest]).astype(np.int64)


def listed(variant, P, M=1, D=0):
    """(module docstring) sc["where"][j]: the index of core surfel j; sc["blended"]: [P] bool; sc["wide"]: the three wide surfels' indices.
    Not cached: the largest is ~100 MB."""
    core, cblend = _listed_core(variant, M, D)
    rng = np.random.default_rng(900)
    where = listed_where(P)
    S, VS = WIDTHS[variant]
    sc = {k: v for k, v in core.items() if not (isinstance(v, np.ndarray) and v.shape[:1] == (67,))}
    r = lambda *shape: rng.random(shape, dtype=F32)
    pad = {"means3D": np.concatenate([2 * r(P, 2) - 1, 4.5 + 2 * r(P, 1)], -1),     # the camera sits at z = 4 and looks down: behind it
           "scales": 0.01 + 0.05 * r(P, 3), "rotations": r(P, 4) + F32(0.1), "opacities": 0.2 + 0.7 * r(P, 1),
           "shs": 0.6 * r(P, M, 3) - F32(0.3), "features": r(P, S)}
    if variant == "svgss":
        pad["vfeatures"] = r(P, VS)
    for k, a in pad.items():
        a[where] = core[k]
        sc[k] = a
    sc["where"], sc["wide"], sc["offset"] = where, where[64:], 0
    sc["blended"] = np.zeros(P, bool)
    sc["blended"][where[cblend]] = True
    return sc


# ---- shared host side -------------------------------------------------------------------------------------------------------------

def build(case):
    """("lattice", variant, M, D, offset) | ("colors", variant) | ("coop", variant) | ("clamp", variant, channel)"""
    kind, variant = case[:2]
    if kind == "lattice":
        return lattice(variant, *case[2:])
    if kind == "colors":
        return lattice(variant, 0, 0, colors=True)
    if kind == "coop":
        return coop_rows(variant)
    if kind == "clamp":
        return clamp_ladder(variant, case[2])
    raise KeyError(case)


@functools.lru_cache(maxsize=None)
def host(case):
    """(scene, upstream gradients, fp32 oracle, fp64 oracle), both after forward and backward: computed once, shared, never modified."""
    sc = build(case)
    grads = br.upstream(sc, case[1])
    return sc, grads, oracle(sc, case[1], grads=grads), oracle(sc, case[1], fp64=True, grads=grads)


def sh_identity_error(sc, dsh, dcol, clamped, rows):
    """dL_dsh[i, k, c] == cf_k(dir_i) (clamped_ic ? 0 : dL_dcolors[i, c]) for k < nk: the largest |difference| over
    A_k |dL_dcolors[i, c]| (A_k: sh_basis) over the surfels `rows`, in units of eps32."""
    nk = nk_of(sc["sh_degree"])
    cf, A = sh_basis(view_dirs(sc))
    dcol = np.asarray(dcol, np.float64)
    g = np.where(clamped, 0.0, dcol)
    err = np.abs(np.asarray(dsh, np.float64)[:, :nk] - cf[:, :nk, None] * g[:, None, :])
    mag = A[:, :nk, None] * np.abs(dcol)[:, None, :]
    ratio = np.where(mag > 0, err / np.where(mag > 0, mag, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(ratio[rows].max()) / EPS
