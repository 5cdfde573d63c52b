"""Scenes for the blended-only backward: geom_bwd (csrc/geom_bwd.hip) processes a surfel only if the forward gave it a blend weight.
Every scene is a 64 x 64 image (16 tiles) whose surfels fall, by construction, into the classes that rule has to tell apart:

  culled      behind the camera or facing away: radius 0;
  occluded    radius > 0, opacity 0.9, but behind a wall of opaque surfels where every pixel has terminated: weight 0;
  faint       radius > 0 in the open, opacity 0.003 < 1/255: no pixel blends it, weight 0;
  blended     weight > 0 (the wall included);
  idle wave   one 64-aligned run of indices (a wave of geom_bwd) without a blended surfel.

`build(P, variant)`: P = 300 holds all of them, the run being the indices 64..127; the indices 128..255, one wave's two chunks in
geom_bwd, hold more than 64 blended surfels (the wave runs its body twice), the last wave is partial.  P = 65: the same classes
with a three-surfel wall, the run being the last, partial wave (index 64 is culled).  P = 1: one blended surfel, nothing else fits.  `build(..., nothing=True)`:
every surfel culled, R = 0.  `classes()` derives the masks from the CPU oracle; tests/test_gpu_blended_only.py asserts on the host that
they are non-empty before anything runs on the GPU."""
import numpy as np

from svgir_harness import cameras, scenes

W = H = 64
EYE = (0.0, 0.0, 4.0)
WALL_UV = (20.0, 20.0)       # centre of the opaque wall (pixels); the occluded surfels sit within 2 px of it
# (svgss: gradient rows + grad_reduce, far below the row-list threshold; rgss_generic: a width without a specialised composite)
VARIANTS = {"rgss": dict(S=5, VS=0), "svgss": dict(S=4, VS=52), "rgss_generic": dict(S=2, VS=0)}


def kernel_variant(variant):
    """The rasterizer a case runs on."""
    return variant.split("_")[0]


def _kinds(P):
    """Class of every index: 'w'all, 'b'lended, 'o'ccluded, 'f'aint, 'c'ulled."""
    if P == 1:
        return np.array(list("b"))
    if P == 65:
        k = np.array(list("b" * 65))
        k[[3, 30, 50]] = "w"
        k[[5, 33]] = "o"
        k[[7, 40]] = "f"
        k[[9, 21, 64]] = "c"
        return k
    assert P >= 192
    k = np.array(list("b" * P))
    k[np.arange(0, P, 7)] = "c"
    k[np.arange(3, P, 11)] = "f"
    k[np.arange(5, P, 13)] = "o"
    k[64:128] = np.array(list("cfo" * 22))[:64]      # the idle wave
    free = np.nonzero(k == "b")[0]
    k[free[np.linspace(0, len(free) - 1, 8).astype(int)]] = "w"
    return k


def build(P, variant, seed=0, nothing=False):
    rng = np.random.default_rng(1000 * P + seed)
    wd = VARIANTS[variant]
    sc = {"sh_degree": 3, "bg": np.full(3, 0.5, dtype=np.float32), "config": np.array([1.0, 1.0, 1.0], dtype=np.float32),
          "scale_modifier": 1.0, "backward_geometry": True, "computer_pseudo_normal": False}
    sc.update(cameras.make_camera(W, H, np.array(EYE)))
    fx = W / (2.0 * sc["tanfovx"])
    k = _kinds(P)
    if nothing:
        k = np.array(list("c" * P))
    n = {c: int((k == c).sum()) for c in "wbofc"}
    u, v, z, sig, op = (np.zeros(P) for _ in range(5))
    # the wall: opaque, in front of everything (its layers 0.01 apart in depth).  Eight layers of sigma 10 px: alpha >= 0.77 within 7 px of
    # the centre, T < 1e-4 there behind them, and nothing left of them 16 px away, where the open area begins.  Three layers (P = 65)
    # must be nearly flat to terminate a pixel: sigma 40 px, alpha >= 0.97 within 7 px (T: 0.03, 9e-4, then the cut-off), <= 0.91 in the open
    m = k == "w"
    u[m], v[m], z[m], op[m] = WALL_UV[0] + 0.37, WALL_UV[1] + 0.41, 1.5 + 0.01 * np.arange(n["w"]), 0.99
    sig[m] = 10.0 if n["w"] > 3 else 40.0
    # occluded: small, opaque enough, right behind the wall's centre
    m = k == "o"
    u[m], v[m] = WALL_UV[0] + rng.uniform(-2, 2, n["o"]), WALL_UV[1] + rng.uniform(-2, 2, n["o"])
    z[m], sig[m], op[m] = rng.uniform(3.0, 3.5, n["o"]), 1.5, 0.9
    # blended and faint: in the open (x >= 36: more than 3 sigma of the wall away is not needed -- they lie in FRONT of nothing opaque)
    for c, lo, hi in (("b", 0.3, 0.9), ("f", 0.003, 0.003)):
        m = k == c
        u[m], v[m] = rng.uniform(36.0, 60.0, n[c]), rng.uniform(4.0, 60.0, n[c])
        z[m], sig[m], op[m] = rng.uniform(2.0, 3.0, n[c]), rng.uniform(1.0, 3.0, n[c]), rng.uniform(lo, hi, n[c])
    # culled: alternately behind the camera and facing away
    m = np.nonzero(k == "c")[0]
    u[m], v[m], z[m], sig[m], op[m] = rng.uniform(8, 56, len(m)), rng.uniform(8, 56, len(m)), rng.uniform(2.0, 3.0, len(m)), 2.0, 0.8
    z[m[0::2]] *= -1.0
    pts = scenes._unproject(sc, u, v, z)
    nrm = sc["campos"][None].astype(np.float64) - pts
    nrm[m[1::2]] *= -1.0
    s = np.sqrt(np.maximum(sig * sig - 0.3, 1e-4)) * np.abs(z) / fx
    sc["means3D"] = pts.astype(np.float32)
    sc["scales"] = np.stack([s, s, s], -1).astype(np.float32)
    sc["rotations"] = scenes._quat_from_frame_fast(nrm, rng)
    sc.update(scenes._attrs(P, rng, kernel_variant(variant), wd["S"], wd["VS"], 3, op))
    sc["kinds"] = "".join(k)      # (a string: the scene's arrays are what goes to the GPU)
    return sc


def classes(sc, o):
    """The masks of the docstring from a forward of the CPU oracle `o` (oracle.OracleRun after forward())."""
    im = o.images()
    radii, w = im["radii"].reshape(-1), im["weights"].reshape(-1)
    opq = sc["opacities"].reshape(-1)
    P = len(w)
    idle = [i for i in range(0, P, 64) if not (w[i:i + 64] > 0).any()]
    return dict(culled=radii == 0, occluded=(radii > 0) & (w == 0) & (opq >= 1.0 / 255.0), faint=(radii > 0) & (w == 0) & (opq < 1.0 / 255.0),
                blended=w > 0, idle_waves=idle)
