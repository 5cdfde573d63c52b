"""Scenes for the plain backward composite (csrc/render_bwd_plain.hip): the kernel walks a sub-tile's consumed candidates back to
front in blocks of 8, contracts the blend weights of a PAIR of blocks in one MFMA set, and adds each candidate's sums into its packed
gradient row (common.hpp packed_row_geom).  Every scene is the smallest at which one piece of that can go wrong:

  stack(n)          one 16 x 16 tile, n translucent splats centred on it (sigma 8 px, opacity ~0.03: alpha >= 1/255 at the tile's corners,
                    T ~ 0.97^n > 1e-4 through 129 of them): every pixel blends all n, so each of the four sub-tiles consumes exactly n.
                    COUNTS: a single block, a pair, an odd number of blocks, a full 64-candidate segment, a second and a third segment.
  live_bits()       one tile; per sub-tile 8 blending splats in front, then 16 that pass the sub-tile's rectangle cull and blend nowhere,
                    then 8 blending splats.  A "miss" has no extent of its own (its 2D covariance is the 0.3 px^2 low-pass alone), opacity
                    0.006 and its centre BETWEEN four pixels of its sub-tile: inside the rectangle the cull tests (alpha at the centre
                    0.006 >= 1/255), alpha at the nearest pixels, 0.71 px away, 0.006 exp(-0.83) = 0.0026 < 1/255.  The walk (deepest
                    first) is then [live][not live][not live][live]: a pair whose second block is not live, and one whose first is not.
  start_past(f, m)  one tile; f translucent splats in front, then three opaque ones (opacity 0.99, sigma 200 px: alpha 0.988 everywhere, so T
                    falls to 1.2e-2, 1.4e-4, and the third -- behind a translucent front already the second -- ends every pixel without
                    being blended), then m more splats behind them, all within the forward's first staging batch of 64.  The forward
                    consumes whole batches, so the sub-tile's consumed count is f + 3 + m while its last contributor is entry f + 2 (or
                    f + 1): the m + 1 (m + 2) deepest entries lie behind every pixel and the replay starts at block (m + 1) // 8 -- an odd
                    block for m = 8 and 24, an even one for m = 16 -- with one or (f = 12) two blocks left to walk.
Footprints: `sigma` is the smallest extent of a tilted, elongated disc (see _scene), so the coverage above holds a fortiori.
  alignment(P)      a 32 x 32 image (4 tiles); P = 13: the surfels 0..7 and the last one are blended, 8..11 have opacity 0.002 and are
                    never blended; P = 5: all but surfel 2; P = 1.  Rows 0..7 cover every start offset of an 80-byte row in a 64-byte
                    segment and both halves of a 256-byte line of 128-byte rows.

`expect(sc)` lists what a scene claims; tests/test_bwd_rows_scenes.py checks the claims with the CPU oracle."""
import numpy as np

from svgir_harness import cameras, scenes

EYE = (0.0, 0.0, 4.0)
COUNTS = (1, 7, 8, 9, 15, 16, 17, 24, 25, 63, 64, 65, 129)
START_PAST = ((0, 8), (0, 16), (0, 24), (12, 8), (12, 24))
ALIGN_P = (1, 5, 13)
# the CASE list of launch_render_bwd_plain: (rasterizer, S); VS = 0 throughout
WIDTHS = (("rgss", 0), ("rgss", 1), ("rgss", 3), ("rgss", 5), ("svgss", 0), ("svgss", 5))
STACK_SIGMA, STACK_OPACITY = 8.0, 0.03
MISS_OPACITY = 0.006
TILT_MARGIN = 1.15
SCENES = [f"stack{n}" for n in COUNTS] + ["live_bits"] + [f"start_past_{f}_{m}" for f, m in START_PAST] + [f"align{p}" for p in ALIGN_P]


def _scene(W, H, u, v, z, sig, op, variant, S, seed, shuffle=True):
    """Camera-facing surfels with projected centre (u, v) px, view depth z, footprint sigma px (0: the low-pass alone), opacity op."""
    rng = np.random.default_rng(seed)
    u, v, z, sig, op = (np.asarray(x, np.float64) for x in (u, v, z, sig, op))
    P = len(u)
    sc = {"sh_degree": 3, "bg": np.full(3, 0.5, dtype=np.float32), "config": np.array([1.0, 1.0, 1.0], dtype=np.float32),
          "scale_modifier": 1.0, "backward_geometry": True, "computer_pseudo_normal": False}
    sc.update(cameras.make_camera(W, H, np.array(EYE)))
    fx, _ = scenes._focal(sc)
    pts = scenes._unproject(sc, u, v, z)
    s = np.sqrt(np.maximum(sig * sig - 0.3, 1e-8)) * z / fx
    sc["means3D"] = pts.astype(np.float32)
    # `sig` is the footprint's smallest extent: the discs are 1.4 times as long as wide and tilted 10 - 25 degrees out of the view
    # direction (cos 25 = 0.91, against the 1.15 of TILT_MARGIN).  A round disc facing the camera has rotation gradients that are
    # zero analytically -- sums of cancelling terms, which no two fp32 evaluations agree on -- and the tail quantiles of the parity
    # budgets are the MAXIMUM of tensors this small.
    s = s * TILT_MARGIN
    sc["scales"] = np.stack([s, 1.4 * s, s], -1).astype(np.float32)
    d = sc["campos"][None].astype(np.float64) - pts
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    t = rng.normal(size=d.shape)
    t -= (t * d).sum(-1, keepdims=True) * d
    t /= np.linalg.norm(t, axis=-1, keepdims=True)
    ang = np.radians(rng.uniform(10.0, 25.0, size=(P, 1)))
    sc["rotations"] = scenes._quat_from_frame_fast(np.cos(ang) * d + np.sin(ang) * t, rng)
    sc.update(scenes._attrs(P, rng, variant, S, 0, 3, op))
    order = rng.permutation(P) if shuffle else np.arange(P)     # surfel ids against depth order
    for k in ("means3D", "scales", "rotations", "opacities", "shs", "features", "vfeatures"):
        if k in sc:
            sc[k] = np.ascontiguousarray(sc[k][order])
    sc["order"] = order      # sc[...][i] is the surfel built as number order[i]
    return sc


def upstream(sc, variant, seed=7):
    """dL/d(outputs): per channel a positive plane a + b x + c y over the image, scaled like scenes.upstream_grads.  White noise makes
    every per-Gaussian gradient a sum of cancelling pixel terms; on tensors of a few entries the parity budgets then compare two
    roundings of nothing."""
    rng = np.random.default_rng(seed)
    g = scenes.upstream_grads(sc, variant, seed=seed)
    H, W = sc["H"], sc["W"]
    y, x = np.mgrid[0:H, 0:W] / float(max(H, W))
    for k, a in g.items():
        c = a.shape[0]
        co = rng.uniform(0.5, 1.0, (c, 1, 1)) + rng.uniform(-0.3, 0.3, (c, 1, 1)) * x[None] + rng.uniform(-0.3, 0.3, (c, 1, 1)) * y[None]
        g[k] = (co / (H * W)).astype(np.float32)
    return g


def stack(n, variant="rgss", S=5):
    rng = np.random.default_rng(n)
    sc = _scene(16, 16, np.full(n, 7.5), np.full(n, 7.5), 3.0 + 0.004 * np.arange(n), np.full(n, STACK_SIGMA),
                STACK_OPACITY * rng.uniform(0.9, 1.1, n), variant, S, seed=100 + n)
    sc["claims"] = dict(kind="stack", n=n)
    return sc


def live_bits(variant="rgss", S=5):
    rng = np.random.default_rng(7)
    u, v, z, sig, op, kind = [], [], [], [], [], []

    def hits(z0):
        for i in range(8):
            u.append(7.5); v.append(7.5); z.append(z0 + 0.004 * i); sig.append(STACK_SIGMA); op.append(STACK_OPACITY * rng.uniform(0.9, 1.1))
            kind.append("h")
    hits(3.0)
    for sub in range(4):
        cells = rng.permutation(49)[:16]     # 16 distinct gaps between the pixels of the sub-tile
        for j, c in enumerate(cells):
            u.append(8 * (sub & 1) + (c % 7) + 0.5); v.append(8 * (sub >> 1) + (c // 7) + 0.5)
            z.append(3.1 + 0.002 * (4 * j + sub)); sig.append(0.0); op.append(MISS_OPACITY)
            kind.append("m")
    hits(3.3)
    sc = _scene(16, 16, u, v, z, sig, op, variant, S, seed=107)
    sc["claims"] = dict(kind="live_bits", built=np.array(kind))
    return sc


def start_past(front, behind, variant="rgss", S=5):
    rng = np.random.default_rng(1000 * front + behind)
    n = front + 3 + behind
    assert n <= 64, "one staging batch of the forward"
    sig = np.full(n, STACK_SIGMA)
    op = STACK_OPACITY * rng.uniform(0.9, 1.1, n)
    sig[front:front + 3], op[front:front + 3] = 200.0, 0.99
    sc = _scene(16, 16, np.full(n, 7.5), np.full(n, 7.5), 3.0 + 0.004 * np.arange(n), sig, op, variant, S, seed=200 + n)
    sc["claims"] = dict(kind="start_past", total=n, last=(front + 1, front + 2), cstart=(behind + 1) // 8 * 8)
    return sc


def alignment(P, variant="rgss", S=5):
    rng = np.random.default_rng(300 + P)
    faint = {13: [8, 9, 10, 11], 5: [2], 1: []}[P]
    op = rng.uniform(0.3, 0.8, P)
    op[faint] = 0.002
    sc = _scene(32, 32, rng.uniform(4.0, 28.0, P), rng.uniform(4.0, 28.0, P), rng.uniform(2.0, 3.0, P), rng.uniform(1.5, 4.0, P), op,
                variant, S, seed=300 + P, shuffle=False)
    blended = np.ones(P, bool)
    blended[faint] = False
    sc["claims"] = dict(kind="alignment", blended=blended)
    return sc


def build(name, variant="rgss", S=5):
    if name.startswith("stack"):
        return stack(int(name[5:]), variant, S)
    if name == "live_bits":
        return live_bits(variant, S)
    if name.startswith("start_past_"):
        f, m = name.split("_")[2:]
        return start_past(int(f), int(m), variant, S)
    if name.startswith("align"):
        return alignment(int(name[5:]), variant, S)
    raise KeyError(name)
