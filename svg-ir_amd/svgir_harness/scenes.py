"""Seeded synthetic scenes of SURVEY.md section 8(d) (no datasets, no network).

Every generator returns a dict of float32 numpy arrays named like the reference's tensors plus the camera
fields of cameras.make_camera(); the same dict feeds the oracle (oracle/oracle.py) and, moved to the GPU, the
rasterizer bindings.
"""
import math

import numpy as np

from . import cameras


def _normalize(v, axis=-1):
    return v / np.maximum(np.linalg.norm(v, axis=axis, keepdims=True), 1e-12)


def quat_from_frame(n, rng):
    """Quaternions (r,x,y,z) of rotations whose local z axis is `n` (in-plane angle random)."""
    n = _normalize(n.astype(np.float64))
    a = np.where(np.abs(n[:, 2:3]) < 0.9, np.array([[0.0, 0.0, 1.0]]), np.array([[1.0, 0.0, 0.0]]))
    t0 = _normalize(np.cross(a, n))
    t1 = np.cross(n, t0)
    ang = rng.uniform(0, 2 * np.pi, size=(n.shape[0], 1))
    u = np.cos(ang) * t0 + np.sin(ang) * t1
    v = np.cross(n, u)
    R = np.stack([u, v, n], axis=-1)  # columns
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    q = np.zeros((n.shape[0], 4))
    # robust matrix -> quaternion
    for i in range(n.shape[0]):
        m = R[i]
        t = tr[i]
        if t > 0:
            s = math.sqrt(t + 1.0) * 2
            q[i] = [0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s]
        elif m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
            s = math.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2]) * 2
            q[i] = [(m[2, 1] - m[1, 2]) / s, 0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s]
        elif m[1, 1] > m[2, 2]:
            s = math.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2]) * 2
            q[i] = [(m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s]
        else:
            s = math.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1]) * 2
            q[i] = [(m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s]
    return _normalize(q).astype(np.float32)


def _quat_from_frame_fast(n, rng):
    """Vectorised variant for large P: q = q_align(z->n) * q_spin(z, ang)."""
    n = _normalize(n.astype(np.float64))
    # shortest-arc quaternion from +z to n
    w = 1.0 + n[:, 2]
    xyz = np.stack([-n[:, 1], n[:, 0], np.zeros_like(w)], axis=-1)  # cross(z, n)
    flip = w < 1e-6
    w = np.where(flip, 0.0, w)
    xyz[flip] = np.array([1.0, 0.0, 0.0])
    qa = _normalize(np.concatenate([w[:, None], xyz], axis=-1))
    ang = rng.uniform(0, 2 * np.pi, size=n.shape[0])
    qs = np.stack([np.cos(ang / 2), np.zeros_like(ang), np.zeros_like(ang), np.sin(ang / 2)], axis=-1)
    # Hamilton product qa * qs
    r1, x1, y1, z1 = qa.T
    r2, x2, y2, z2 = qs.T
    q = np.stack([r1 * r2 - x1 * x2 - y1 * y2 - z1 * z2, r1 * x2 + x1 * r2 + y1 * z2 - z1 * y2,
                  r1 * y2 - x1 * z2 + y1 * r2 + z1 * x2, r1 * z2 + x1 * y2 - y1 * x2 + z1 * r2], axis=-1)
    return _normalize(q).astype(np.float32)


def random_cloud(P=10000, W=256, H=256, seed=0, sh_degree=0, variant="svgss", S=0, VS=0):
    """cfg1 "plumbing": uniform cloud, SH degree 0, no BRDF channels, black background."""
    rng = np.random.default_rng(seed)
    M = (sh_degree + 1) ** 2
    sc = {
        "means3D": rng.uniform(-1, 1, size=(P, 3)).astype(np.float32),
        "scales": np.exp(rng.uniform(math.log(0.005), math.log(0.05), size=(P, 3))).astype(np.float32),
        "rotations": _normalize(rng.normal(size=(P, 4))).astype(np.float32),
        "opacities": rng.uniform(0.05, 0.99, size=(P, 1)).astype(np.float32),
        "shs": rng.normal(0, 0.5, size=(P, M, 3)).astype(np.float32),
        "sh_degree": sh_degree,
        "bg": np.zeros(3, dtype=np.float32),
        "config": np.array([1.0, 1.0, 1.0], dtype=np.float32),
        "scale_modifier": 1.0,
    }
    sc["features"] = rng.normal(size=(P, S)).astype(np.float32)
    if variant == "svgss":
        sc["vfeatures"] = rng.normal(size=(P, VS)).astype(np.float32)
    sc.update(cameras.make_camera(W, H, cameras.orbit_eye(4.0, 30.0, 20.0)))
    sc["backward_geometry"] = True
    sc["computer_pseudo_normal"] = False
    return sc


def _surface_points(P, rng):
    """Noisy unit sphere + axis-aligned box mixture; returns (points, outward normals)."""
    n_s = P // 2
    n_b = P - n_s
    d = _normalize(rng.normal(size=(n_s, 3)))
    ps = d * (0.8 + 0.01 * rng.normal(size=(n_s, 1)))
    ns = d
    face = rng.integers(0, 6, size=n_b)
    uv = rng.uniform(-0.45, 0.45, size=(n_b, 2))
    pb = np.zeros((n_b, 3))
    nb = np.zeros((n_b, 3))
    ax = face // 2
    sgn = np.where(face % 2 == 0, 1.0, -1.0)
    for a in range(3):
        m = ax == a
        o = [i for i in range(3) if i != a]
        pb[m, a] = sgn[m] * 0.45
        pb[m, o[0]] = uv[m, 0]
        pb[m, o[1]] = uv[m, 1]
        nb[m, a] = sgn[m]
    pb += np.array([0.0, 0.0, -0.1])
    pts = np.concatenate([ps, pb], axis=0)
    nrm = np.concatenate([ns, nb], axis=0)
    perm = rng.permutation(P)
    return pts[perm], nrm[perm]


def surface_scene(P=200000, W=800, H=800, seed=1, sh_degree=3, variant="rgss", S=5, VS=0, bg=1.0,
                  azimuth=30.0, elevation=25.0, scale_lo=0.004, scale_hi=0.03):
    """cfg2/cfg3/cfg4/cfg5 geometry: surface-aligned surfels (local z = outward normal +- 20 deg jitter)."""
    rng = np.random.default_rng(seed)
    pts, nrm = _surface_points(P, rng)
    jit = nrm + math.tan(math.radians(20.0)) * 0.5 * rng.normal(size=nrm.shape)
    M = (sh_degree + 1) ** 2
    sc = {
        "means3D": pts.astype(np.float32),
        "scales": np.exp(rng.uniform(math.log(scale_lo), math.log(scale_hi), size=(P, 3))).astype(np.float32),
        "rotations": _quat_from_frame_fast(jit, rng),
        "opacities": rng.beta(2.0, 1.0, size=(P, 1)).astype(np.float32),
        "shs": rng.normal(0, 0.3, size=(P, M, 3)).astype(np.float32),
        "sh_degree": sh_degree,
        "bg": np.full(3, bg, dtype=np.float32),
        "config": np.array([1.0, 1.0, 1.0], dtype=np.float32),
        "scale_modifier": 1.0,
        "backward_geometry": True,
        "computer_pseudo_normal": False,
    }
    sc.update(cameras.make_camera(W, H, cameras.orbit_eye(4.0, azimuth, elevation)))
    if variant == "rgss":
        # render.py:83-91: features = [geo normal (world), view depth, depth^2]
        xyz1 = np.concatenate([sc["means3D"], np.ones((P, 1), np.float32)], axis=-1)
        dep = (xyz1 @ sc["viewmatrix"])[:, 2:3]
        f = np.concatenate([_normalize(jit).astype(np.float32), dep, dep * dep], axis=-1).astype(np.float32)
        if S != 5:
            f = rng.normal(size=(P, S)).astype(np.float32)
        sc["features"] = f
    else:
        sc["features"] = rng.uniform(0, 1, size=(P, S)).astype(np.float32)
        sc["vfeatures"] = rng.uniform(0, 1, size=(P, VS)).astype(np.float32)
    return sc


# ---- edge-case scenes: inputs where the composite kernels leave their common path (tests/test_edge_scenes.py checks each case) ----

def _w2c(sc):
    return sc["viewmatrix"].astype(np.float64).T          # viewmatrix = W2C.T


def _focal(sc):
    return sc["W"] / (2.0 * sc["tanfovx"]), sc["H"] / (2.0 * sc["tanfovy"])


def _unproject(sc, u, v, z):
    """World points whose projection is the pixel position (u, v) (the kernels' pixel coordinate: ndc2pix) at view depth z."""
    fx, fy = _focal(sc)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    z = np.broadcast_to(np.asarray(z, np.float64), u.shape)
    pc = np.stack([(u - (sc["W"] - 1) / 2.0) * z / fx, (v - (sc["H"] - 1) / 2.0) * z / fy, z, np.ones_like(u)], axis=-1)
    return (pc @ np.linalg.inv(_w2c(sc)).T)[:, :3]


def _facing(sc, pts, rng):
    """Rotations whose local z axis (the surfel normal) points from `pts` to the camera."""
    return _quat_from_frame_fast(sc["campos"][None].astype(np.float64) - pts, rng)


def _quat_matrix(q):
    """Rotation matrices of (r, x, y, z) quaternions; column 2 is the surfel normal."""
    q = _normalize(q.astype(np.float64))
    r, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                     np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                     np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], axis=1)


def cov3d_of(scales, rotations, surface=True):
    """The 3D covariances (upper triangle, [P, 6], fp64) that scales + rotations describe; `surface` zeroes scale.z (Q1)."""
    Rm = _quat_matrix(rotations)
    s = scales.astype(np.float64).copy()
    if surface:
        s[:, 2] = 0.0
    Sg = np.einsum("pij,pj,pkj->pik", Rm, s * s, Rm)
    return Sg[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]


def _attrs(P, rng, variant, S, VS, sh_degree, opac):
    M = (sh_degree + 1) ** 2
    out = {"opacities": np.asarray(opac, np.float32).reshape(P, 1),
           "shs": rng.normal(0, 0.3, size=(P, M, 3)).astype(np.float32),
           "features": rng.uniform(0, 1, size=(P, S)).astype(np.float32)}
    if variant == "svgss":
        out["vfeatures"] = rng.uniform(0, 1, size=(P, VS)).astype(np.float32)
    return out


def _append(sc, add):
    for k, v in add.items():
        sc[k] = np.ascontiguousarray(np.concatenate([sc[k], v.astype(sc[k].dtype)], axis=0))


def frustum_extras(sc, variant, seed=0, n_side=8, n_near=3):
    """Appends Gaussians at the edges of the view frustum (scales + rotations, facing the camera) to a scene:
      * `n_side` whose projected centre lies beyond the 1.3 tan(fov/2) clamp of the covariance projection (at 1.37 tan: inside
        svgss's 20 % image margin, which ends at 1.4 tan) with a footprint (sigma 30-45 px) that still reaches the image;
      * `n_near` at view depth 0.21-0.25 (rgss culls at 0.2) whose radius covers the whole image.
    Short images (H < 64) get side Gaussians beyond the left / right clamp only (svgss's margin is too thin there)."""
    rng = np.random.default_rng(seed)
    W, H = sc["W"], sc["H"]
    fx, fy = _focal(sc)
    side = rng.integers(0, 2 if H < 64 else 4, size=n_side)   # beyond the x clamp (0, 1) or the y clamp (2, 3)
    k = 1.37 * np.where(side % 2 == 0, 1.0, -1.0)
    t = rng.uniform(-0.8, 0.8, size=n_side)
    ux = np.where(side < 2, k, t) * sc["tanfovx"] * fx + (W - 1) / 2.0
    vy = np.where(side >= 2, k, t) * sc["tanfovy"] * fy + (H - 1) / 2.0
    z = np.concatenate([rng.uniform(2.0, 3.5, size=n_side), rng.uniform(0.21, 0.25, size=n_near)])
    u = np.concatenate([ux, rng.uniform(0.3, 0.7, size=n_near) * W])
    v = np.concatenate([vy, rng.uniform(0.3, 0.7, size=n_near) * H])
    pts = _unproject(sc, u, v, z)
    sig = np.concatenate([rng.uniform(30.0, 45.0, size=n_side), rng.uniform(1.0, 1.5, size=n_near) * max(W, H)])
    s = sig * z / fx
    n = n_side + n_near
    add = {"means3D": pts.astype(np.float32), "scales": np.stack([s, s * rng.uniform(0.7, 1.0, size=n), s], -1).astype(np.float32),
           "rotations": _facing(sc, pts, rng)}
    add.update(_attrs(n, rng, variant, sc["features"].shape[1], sc["vfeatures"].shape[1] if "vfeatures" in sc else 0, sc["sh_degree"],
                      np.concatenate([rng.uniform(0.5, 0.9, size=n_side), rng.uniform(0.15, 0.3, size=n_near)])))
    _append(sc, add)
    sc["n_frustum"] = sc.get("n_frustum", 0) + n
    return sc


def indefinite_conic_scene(variant="svgss", n_bg=3000, n_ind=48, W=192, H=144, seed=61, sh_degree=1, S=3, VS=8, extras=False):
    """Gaussians whose 2D covariance J Sigma J^T + 0.3 I is clearly indefinite (eigenvalues ~ +0.1 / -0.1 px^2: conic entries ~ +-10,
    det < 0) over a background of surface discs.  The bindings take either cov3D_precomp or scales + rotations, so the whole scene
    is cov3D_precomp (no rotations: every surfel normal is the world z axis, and the camera looks down on the scene).  Each
    indefinite Gaussian is centred in an 8x8 sub-tile, 1 px from one of its horizontal edges, with its negative axis within 20 degrees
    of the image's y axis: pixels of the sub-tile along the positive axis blend it (power in [-5.5, 0]) while pixels 5-6 px away along
    the negative one have power > 90, where exp overflows.  No pixel of a tile it touches is within 1e-2 of power 0 or of the 1/255
    alpha threshold, so fp32 and fp64 take the same blend decisions.  The last n_ind Gaussians are the indefinite ones."""
    sc = surface_scene(P=n_bg, W=W, H=H, seed=seed, sh_degree=sh_degree, variant=variant, S=S, VS=VS, scale_lo=0.02, scale_hi=0.08)
    sc.update(cameras.make_camera(W, H, cameras.orbit_eye(4.0, 35.0, 55.0)))
    if variant == "rgss":
        sc["features"] = np.random.default_rng(seed + 1).uniform(0, 1, size=(n_bg, S)).astype(np.float32)
    if extras:
        frustum_extras(sc, variant, seed=seed + 2)
    rng = np.random.default_rng(seed + 3)
    fx, fy = _focal(sc)
    Rwc = _w2c(sc)[:3, :3]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    mu, cov, ops = [], [], []
    for sidx in rng.permutation((W // 8) * (H // 8)):
        if len(mu) == n_ind:
            break
        sx, sy = 8 * (sidx % (W // 8)), 8 * (sidx // (W // 8))
        th = rng.uniform(-np.pi / 9, np.pi / 9)
        Rt = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        c2 = Rt @ np.diag([rng.uniform(0.08, 0.14), -rng.uniform(0.08, 0.14)]) @ Rt.T   # the 2D covariance incl. the 0.3 dilation
        con = np.linalg.inv(c2)
        u = sx + rng.uniform(2.0, 5.0)
        v = sy + (1.0 if rng.random() < 0.5 else 6.0) + rng.uniform(-0.4, 0.4)
        op = rng.uniform(0.6, 0.95)
        la = np.log(255.0 * op)
        # every pixel of the tiles its footprint (radius 2 px) touches
        x0, x1 = max(0, int((u - 2) // 16)), min(gx, int((u + 2 + 15) // 16))
        y0, y1 = max(0, int((v - 2) // 16)), min(gy, int((v + 2 + 15) // 16))
        px, py = np.meshgrid(np.arange(16 * x0, min(W, 16 * x1)), np.arange(16 * y0, min(H, 16 * y1)))
        dx, dy = u - px, v - py
        pw = -0.5 * (con[0, 0] * dx * dx + con[1, 1] * dy * dy) - con[0, 1] * dx * dy
        if np.abs(pw).min() < 1e-2 or np.abs(pw + la).min() < 1e-2:
            continue
        sub = (px // 8 == sx // 8) & (py // 8 == sy // 8)
        if not ((pw[sub] <= 0) & (pw[sub] >= -la)).any() or not (pw[sub] > 90.0).any():
            continue
        z = rng.uniform(2.0, 3.2)
        D = np.diag([z / fx, z / fy])
        Sc = np.zeros((3, 3))
        Sc[:2, :2] = D @ (c2 - 0.3 * np.eye(2)) @ D      # camera space: J Sigma_c J^T = c2 - 0.3 I (its third row and column are 0)
        Sw = Rwc.T @ Sc @ Rwc
        mu.append(_unproject(sc, np.array([u]), np.array([v]), z)[0])
        cov.append(Sw[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]])
        ops.append(op)
    assert len(mu) == n_ind, len(mu)
    cov_bg = cov3d_of(sc["scales"], sc["rotations"])
    del sc["scales"], sc["rotations"]
    add = {"means3D": np.array(mu, np.float32)}
    add.update(_attrs(n_ind, rng, variant, S, VS, sh_degree, ops))
    _append(sc, add)
    sc["cov3D_precomp"] = np.concatenate([cov_bg, np.array(cov)], axis=0).astype(np.float32)
    sc["n_indefinite"] = n_ind
    return sc


def edge_on_near_scene(variant="svgss", n_edge=300, n_bg=3000, W=160, H=120, seed=81, sh_degree=1, S=3, VS=8, extras=False):
    """Flat surfels (surface on: scale.z = 0) close to the near plane and seen nearly edge-on, over a surface_scene background:
    depth 0.21-0.35, in-plane scales 0.3-1.0, the normal at a grazing angle to the view ray at varied in-plane angles.  Both
    rasterizers cull a surfel whose view-space position p and normal n have p.n > -0.01 (svgss auxiliary.h:173-208), so the
    angle cannot come within ~1e-3 rad of edge-on here: it is set so that p.n lies in [-0.014, -0.011], the most edge-on the
    cull admits (|cos| ~ 0.03-0.07).  The projected covariances reach ~1e5-1e6 px^2 along the major axis.  The last n_edge
    Gaussians are the edge-on ones."""
    sc = surface_scene(P=n_bg, W=W, H=H, seed=seed, sh_degree=sh_degree, variant=variant, S=S, VS=VS, scale_lo=0.01, scale_hi=0.05)
    if variant == "rgss":
        sc["features"] = np.random.default_rng(seed + 1).uniform(0, 1, size=(n_bg, S)).astype(np.float32)
    if extras:
        frustum_extras(sc, variant, seed=seed + 2)
    rng = np.random.default_rng(seed + 3)
    z = rng.uniform(0.21, 0.35, size=n_edge)
    pts = _unproject(sc, rng.uniform(0.1, 0.9, size=n_edge) * W, rng.uniform(0.1, 0.9, size=n_edge) * H, z)
    Rwc = _w2c(sc)[:3, :3]
    pv = (pts - sc["campos"][None].astype(np.float64)) @ Rwc.T          # view-space positions
    r = _normalize(pv)
    e = _normalize(np.cross(r, rng.normal(size=(n_edge, 3))))          # a random direction perpendicular to the view ray
    c = rng.uniform(0.011, 0.014, size=n_edge) / np.linalg.norm(pv, axis=-1)
    nv = -c[:, None] * r + np.sqrt(1.0 - c * c)[:, None] * e           # p.n = -|p| c
    s = rng.uniform(0.3, 1.0, size=(n_edge, 3))
    add = {"means3D": pts.astype(np.float32), "scales": s.astype(np.float32), "rotations": _quat_from_frame_fast(nv @ Rwc, rng)}
    add.update(_attrs(n_edge, rng, variant, S, VS, sh_degree, rng.uniform(0.1, 0.4, size=n_edge)))
    _append(sc, add)
    sc["n_edge"] = n_edge
    return sc


STACK_COUNTS = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 191, 192, 193)
# forced termination: (stack length, depth ranks of its opaque splats); a pixel's transmittance falls below 1e-4 at one of them,
# at a rank that depends on the pixel's distance from the stack's centre
STACK_TERMINATE = ((160, (63, 64, 65, 66)), (160, (62, 63, 64, 65)), (193, (127, 128, 129, 130)), (193, (126, 127, 128, 129)))
STACK_SIGMA, STACK_OPACITY, STACK_TIE = 6.0, 0.03, 6


def stack_scene(variant="svgss", counts=STACK_COUNTS, terminate=False, seed=71, sh_degree=1, S=3, VS=8, extras=False):
    """One tile row; every other tile holds a stack of n translucent Gaussians centred on the tile (sigma ~ 6 px, opacity ~ 0.03:
    alpha >= 1/255 at the tile's corners and T > 1e-4 at its centre through 193 of them), so every pixel of the tile blends all n,
    the tile's list is exactly n long and its n_contrib is n.  The tiles in between get the neighbouring stacks' tails.
    `terminate`: the stacks of STACK_TERMINATE, with opaque splats (opacity 0.99, sigma 7 px) at the given depth ranks: a pixel's
    transmittance falls below 1e-4 at the first, second, ... of them depending on its distance from the centre.  In every stack a
    block of STACK_TIE Gaussians (straddling rank 64 where the stack is long enough) shares one position, hence one bit-identical
    depth: their order in the instance list is the stable order of their indices.  Indices are shuffled against depth order."""
    rng = np.random.default_rng(seed)
    plan = list(STACK_TERMINATE) if terminate else [(n, ()) for n in counts]
    W, H = 16 * (2 * len(plan) + 1), 16
    sc = {"sh_degree": sh_degree, "bg": np.full(3, 0.5, dtype=np.float32), "config": np.array([1.0, 1.0, 1.0], dtype=np.float32),
          "scale_modifier": 1.0, "backward_geometry": True, "computer_pseudo_normal": False}
    sc.update(cameras.make_camera(W, H, cameras.orbit_eye(4.0, 20.0, 10.0)))
    fx, _ = _focal(sc)
    pts, sig, ops, ties = [], [], [], []
    for t, (n, opaque) in enumerate(plan):
        z = 3.0 + 0.004 * np.arange(n)
        t0 = max(0, min(n - STACK_TIE, 61))
        z[t0:t0 + STACK_TIE] = z[t0]
        p = _unproject(sc, np.full(n, 16.0 * (2 * t + 1) + 7.5), np.full(n, 7.5), z)
        p[t0:t0 + STACK_TIE] = p[t0]
        s = np.full(n, STACK_SIGMA)
        o = rng.uniform(0.9, 1.1, size=n) * STACK_OPACITY
        for r in opaque:     # (1-based ranks)
            s[r - 1], o[r - 1] = 7.0, 0.99
        ties.append(sum(len(q) for q in pts) + np.arange(t0, min(n, t0 + STACK_TIE)))
        pts.append(p)
        sig.append(np.sqrt(s * s - 0.3) * z / fx)
        ops.append(o)
    pts, sig, ops = np.concatenate(pts), np.concatenate(sig), np.concatenate(ops)
    P = len(pts)
    sc["means3D"] = pts.astype(np.float32)
    sc["scales"] = np.stack([sig, sig, sig], -1).astype(np.float32)
    sc["rotations"] = _facing(sc, pts, rng)
    sc.update(_attrs(P, rng, variant, S, VS, sh_degree, ops))
    perm = rng.permutation(P)
    for k in ("means3D", "scales", "rotations", "opacities", "shs", "features", "vfeatures"):
        if k in sc:
            sc[k] = np.ascontiguousarray(sc[k][perm])
    inv = np.argsort(perm)
    sc["stack_tiles"] = np.array([2 * t + 1 for t in range(len(plan))])
    sc["stack_counts"] = np.array([n for n, _ in plan])
    sc["tie_blocks"] = [np.sort(inv[b]) for b in ties]      # the new indices of each tied block
    if extras:
        frustum_extras(sc, variant, seed=seed + 1)
    return sc


# ---- binning scenes: every surfel's tiles, depth key and rank are known before anything runs (tests/test_binning_scenes.py) ----

BINNING_EYE = (0.0, 0.0, 4.0)     # on the world z axis, looking down it: view depth = 4 - z_world, ONE fp32 rounding, whatever x and y are


def binning_scene(variant="rgss", P=5000, gx=8, gy=6, layout="uniform", depth="spread", edge_frac=0.0, n_culled=0, n_near=0, seed=0,
                  sh_degree=0, S=0, VS=0, opacity=(0.3, 0.9), bg=0.5):
    """P surfels on a gx x gy tile grid (image 16 gx x 16 gy), each with a footprint far below a pixel (world scale 0.05 px: the
    0.3 px^2 low-pass alone sets the radius), placed within 1.5 px of a tile's centre (u = 16 tx + 7.5): its rectangle is that one
    tile.  A share `edge_frac` sits on the tile's right edge instead (u = 16 tx + 15.5): two tiles, tx and tx + 1, except in the
    last column.
      layout: "uniform" over the grid | "one" tile | "eight" tiles spread over the grid, in equal shares | "skewed" (a twentieth of the tiles, weights
              falling geometrically: most tiles stay empty);
      depth:  "spread" over [0.6, 30) (three different top bytes of the fp32 key) | "binade": [2.5, 3.5) (one top byte, 0x40) |
              "same": one bit-identical depth for all (the whole order is the stable order of the indices);
      n_culled of the P surfels are culled (alternately behind the camera and facing away), interleaved by index with the visible ones;
      n_near extra splats (appended: indices P ...) at depth 0.5-0.7 whose 3 sigma is four image widths: their rectangle is the whole grid.
    The camera looks down the world z axis, so a surfel's view depth is 4 - z_world in one fp32 rounding and "same" really is
    bit-identical.  Indices are shuffled against every construction order.
    sc["plan"]: per surfel `tile` (its first tile), `tile2` (the second one, -1: none), `visible`, `depth` (fp32, what the
    preprocess must compute), the grid, and `R`, the instance count all of this implies."""
    rng = np.random.default_rng(seed)
    W, H, T = 16 * gx, 16 * gy, gx * gy
    sc = {"sh_degree": sh_degree, "bg": np.full(3, bg, dtype=np.float32), "config": np.array([1.0, 1.0, 1.0], dtype=np.float32),
          "scale_modifier": 1.0, "backward_geometry": True, "computer_pseudo_normal": False}
    # (the longer image side gets the usual field of view: on a grid one tile wide and hundreds high the other choice is a 170 degree
    # vertical fov, where the perspective Jacobian at the image's ends stretches the radii from 3 to 7 px)
    fov = cameras.TENSOIR_FOVX if gx >= gy else 2.0 * math.atan(math.tan(cameras.TENSOIR_FOVX / 2) * gx / gy)
    sc.update(cameras.make_camera(W, H, np.array(BINNING_EYE), fovx=fov))
    fx, _ = _focal(sc)
    visible = np.ones(P, dtype=bool)
    if n_culled:
        visible[np.round(np.linspace(0, P - 1, n_culled)).astype(np.int64)] = False
        assert (~visible).sum() == n_culled
    if layout == "uniform":
        tile = rng.integers(0, T, size=P)
    elif layout == "one":
        tile = np.full(P, (gy // 2) * gx + gx // 2)
    elif layout == "eight":
        tile = np.full(P, T // 16)
        nv = int(visible.sum())
        tile[visible] = (((np.arange(8) * T) // 8 + T // 16) % T)[rng.permutation(nv) % 8]     # equal shares: no list beyond ceil(visible / 8)
    elif layout == "skewed":
        pool = rng.choice(T, size=max(1, T // 20), replace=False)
        w = 0.8 ** np.arange(len(pool))
        tile = pool[rng.choice(len(pool), size=P, p=w / w.sum())]
    else:
        raise ValueError(layout)
    tx, ty = tile % gx, tile // gx
    edge = rng.random(P) < edge_frac
    u = 16.0 * tx + np.where(edge, 15.5, 7.5 + rng.uniform(-1.5, 1.5, size=P))
    v = 16.0 * ty + 7.5 + rng.uniform(-1.5, 1.5, size=P)
    if depth == "spread":
        z = np.exp(rng.uniform(math.log(0.6), math.log(30.0), size=P))
    elif depth == "binade":
        z = rng.uniform(2.5, 3.5, size=P)
    elif depth == "same":
        z = np.full(P, 3.0)
    else:
        raise ValueError(depth)
    cul = np.nonzero(~visible)[0]
    behind = np.zeros(P, dtype=bool)
    behind[cul[0::2]] = True
    pts = _unproject(sc, u, v, np.where(behind, -z, z))
    nrm = sc["campos"][None].astype(np.float64) - pts
    nrm[cul[1::2]] *= -1.0                                  # facing away
    s = 0.05 * z / fx
    sc["means3D"] = pts.astype(np.float32)
    sc["scales"] = np.stack([s, s, s], -1).astype(np.float32)
    sc["rotations"] = _quat_from_frame_fast(nrm, rng)
    sc.update(_attrs(P, rng, variant, S, VS, sh_degree, rng.uniform(opacity[0], opacity[1], size=P)))
    tile2 = np.where(edge & (tx < gx - 1), tile + 1, -1)
    if n_near:
        zn = rng.uniform(0.5, 0.7, size=n_near)
        pn = _unproject(sc, rng.uniform(0.4, 0.6, size=n_near) * W, rng.uniform(0.4, 0.6, size=n_near) * H, zn)
        sn = (4.0 * max(W, H) / 3.0) * zn / fx
        add = {"means3D": pn.astype(np.float32), "scales": np.stack([sn, sn, sn], -1).astype(np.float32), "rotations": _facing(sc, pn, rng)}
        add.update(_attrs(n_near, rng, variant, S, VS, sh_degree, rng.uniform(0.05, 0.15, size=n_near)))
        _append(sc, add)
    sc["plan"] = {"gx": gx, "gy": gy, "T": T, "n_near": n_near, "tile": tile.astype(np.int64), "tile2": tile2.astype(np.int64),
                  "visible": visible, "depth": np.float32(BINNING_EYE[2]) - sc["means3D"][:, 2],
                  "R": int(visible.sum() + (tile2[visible] >= 0).sum() + n_near * T)}
    return sc


def binning_expected(sc):
    """(point_list, ranges [T, 2]) that sc["plan"] implies: instances ordered by (tile, fp32 depth bits, index), plain numpy."""
    pl = sc["plan"]
    T, Pn = pl["T"], len(pl["tile"])
    vis = np.nonzero(pl["visible"])[0]
    two = vis[pl["tile2"][vis] >= 0]
    near = np.arange(Pn, Pn + pl["n_near"])
    idx = np.concatenate([vis, two, np.repeat(near, T)])
    til = np.concatenate([pl["tile"][vis], pl["tile2"][two], np.tile(np.arange(T), pl["n_near"])])
    key = np.ascontiguousarray(pl["depth"]).view(np.uint32)[idx]
    order = np.lexsort((idx, key, til))
    cnt = np.bincount(til, minlength=T)
    end = np.cumsum(cnt)
    ranges = np.stack([end - cnt, end], -1)
    ranges[cnt == 0] = 0
    return idx[order].astype(np.uint32), ranges.astype(np.uint32)


def upstream_grads(sc, variant, seed=101):
    """dL/d(outputs) ~ N(0,1)/(H*W) for every differentiable output."""
    rng = np.random.default_rng(seed)
    H, W = sc["H"], sc["W"]
    S = sc["features"].shape[1]
    g = {k: (rng.normal(size=(c, H, W)) / (H * W)).astype(np.float32)
         for k, c in (("color", 3), ("normal", 3), ("depth", 1), ("opacity", 1), ("feature", S))}
    if variant == "svgss":
        g["vfeature"] = (rng.normal(size=(sc["vfeatures"].shape[1] // 4, H, W)) / (H * W)).astype(np.float32)
    return g


CONFIGS = {
    # name: (generator, kwargs)  -- BASELINE.json configs[0..4]
    "cfg1": (random_cloud, dict(P=10000, W=256, H=256, seed=0, sh_degree=0, variant="svgss", S=0, VS=0)),
    "cfg2": (surface_scene, dict(P=200000, W=800, H=800, seed=1, sh_degree=3, variant="rgss", S=5, VS=0, bg=1.0)),
    "cfg3_train": (surface_scene, dict(P=200000, W=800, H=800, seed=2, sh_degree=3, variant="svgss", S=4, VS=52, bg=1.0)),
    "cfg3_eval": (surface_scene, dict(P=200000, W=800, H=800, seed=2, sh_degree=3, variant="svgss", S=7, VS=64, bg=1.0)),
    "cfg4": (surface_scene, dict(P=300000, W=800, H=800, seed=3, sh_degree=3, variant="svgss", S=7, VS=64, bg=1.0)),
    "cfg5": (surface_scene, dict(P=2000000, W=1600, H=1600, seed=4, sh_degree=3, variant="svgss", S=7, VS=64, bg=1.0,
                                 scale_lo=0.002, scale_hi=0.012)),
    # the same 2 M-surfel stress scene at the generator's default surfel scales (0.004-0.03, as in cfg2-cfg4): ~4x the instances
    # (R = 18.3 M), the size SURVEY 8(a) a1 budgets the state blobs for -- the configuration where the composite kernels are nearest
    # to the HBM roof
    "cfg5_dense": (surface_scene, dict(P=2000000, W=1600, H=1600, seed=4, sh_degree=3, variant="svgss", S=7, VS=64, bg=1.0)),
}


def make(name, **override):
    gen, kw = CONFIGS[name]
    kw = dict(kw)
    kw.update(override)
    return gen(**kw)
