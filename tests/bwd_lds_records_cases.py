"""Scenes for the record path of the plain backward composite (csrc/render_bwd_plain.hip): a block's 8 records are copied global -> LDS
by the DMA path (5 x 16 bytes each, source = rec + gid * 96 bytes), phase A reads them back with broadcast ds_reads, the slots beyond a
segment's end replay the record of its last entry with a slot that never blends, and a wave that takes a second segment reuses the
one record buffer.  Every scene is the smallest at which one piece of that can go wrong:

  far_ids()      one 16 x 16 tile, 20 translucent splats stacked on it (bwd_rows_cases.stack) inside a model of P = 70 000 surfels, all
                 others behind the camera (culled).  The visible ones have the ids 0, P - 1 and seeded random ids in between: the 8
                 records of one block lie megabytes apart, and the 32-bit byte offset gid * 96 is exercised at both ends of the array.
  ragged()       one tile whose four sub-tiles consume 3, 8, 13 and 70 candidates: a stack of 3 over the whole tile in front, then per
                 sub-tile 0 / 5 / 10 / 67 small footprints (sigma 0.6 px, opacity 0.02) centred on one of its four middle pixels, three
                 pixels or more from the neighbouring sub-tile's rectangle.  Segments of 3, 8, 13, 64 and 6 entries: 5, 0, 3, 0 and 2 pad
                 slots.  The entries the pads replay -- the front-most of a segment: the first splat of the front stack, and the 65th entry
                 of the last sub-tile -- have opacity 0.99: a pad that blended would change every gradient of its sub-tile.
  second_item()  a 224 x 224 image (784 sub-tiles) under 2 200 image-filling splats (sigma 108 px or more, alpha 0.0085 at the centre, down
                 to the blending threshold in the corners): T stays above 1e-4 through 1 100 (centre) to all 2 200 (corners) of them,
                 17 to 35 segments per sub-tile and more than 16 384 in all -- the size of the backward launch, so that waves take a
                 second segment.  (Not 208 x 208 under an even alpha of 0.0045: every pixel then walks 2 000 splats down to T = 1e-4,
                 and the composite misses the fp64-anchored budget in dL/dscales (p99 relative error 3.4e-4 against a budget of
                 1.1e-4) and dL/dopacity (4.8e-4) -- the same figures with and without the record path, so a property of how the
                 segments have been replayed all along: probably their start state (final - prefix) / T, a difference of fp32 sums
                 that agree in their leading digits where T is small.  This scene is about the second segment of a wave, and keeps
                 that claim.)

`tests/test_bwd_lds_records_scenes.py` checks the claims with the CPU oracle."""
import numpy as np

import bwd_rows_cases as rc
from svgir_harness import scenes

FAR_P, FAR_VISIBLE = 70000, 20
RAGGED_COUNTS = (3, 8, 13, 70)
RAGGED_FRONT = 3
SMALL_SIGMA, SMALL_OPACITY, PAD_OPACITY = 0.6, 0.02, 0.99
SECOND_W, SECOND_N, SECOND_SIGMA, SECOND_OPACITY = 224, 2200, 108.0, 0.0085
LAUNCH_WAVES = 16384      # render_bwd_plain.hip launch(): BWDP_GRID_MULT * 256 CUs * 4 SIMDs * BWDP_WPE
RAGGED_WIDTHS = (("rgss", 5), ("rgss", 0), ("svgss", 5))
_PER_SURFEL = ("means3D", "scales", "rotations", "opacities", "shs", "features", "vfeatures")


def far_ids(variant="rgss", S=5):
    vis = rc.stack(FAR_VISIBLE, variant, S)
    rng = np.random.default_rng(41)
    P, n = FAR_P, FAR_VISIBLE
    ids = np.concatenate([[0, P - 1], rng.choice(np.arange(1, P - 1), size=n - 2, replace=False)])
    ids = ids[rng.permutation(n)]                      # visible surfel j of `vis` becomes surfel ids[j]
    sc = {k: v for k, v in vis.items() if k not in _PER_SURFEL and k not in ("order", "claims")}
    behind = scenes._unproject(sc, rng.uniform(0.0, 16.0, P), rng.uniform(0.0, 16.0, P), -rng.uniform(1.0, 3.0, P))
    fill = {"means3D": behind, "scales": np.full((P, 3), 0.01), "rotations": np.tile([1.0, 0.0, 0.0, 0.0], (P, 1)),
            "opacities": np.full((P, 1), 0.5)}
    for k in _PER_SURFEL:
        if k not in vis:
            continue
        a = fill[k] if k in fill else rng.uniform(0.0, 1.0, (P,) + vis[k].shape[1:])
        a = np.ascontiguousarray(a.astype(vis[k].dtype))
        a[ids] = vis[k]
        sc[k] = a
    sc["claims"] = dict(kind="far_ids", ids=np.sort(ids))
    return sc


def ragged(variant="rgss", S=5):
    rng = np.random.default_rng(43)
    u, v, z, sig, op, sub_of = [], [], [], [], [], []
    for i in range(RAGGED_FRONT):
        u.append(7.5); v.append(7.5); z.append(3.0 + 0.004 * i); sig.append(rc.STACK_SIGMA)
        op.append(PAD_OPACITY if i == 0 else rc.STACK_OPACITY)
        sub_of.append(-1)
    small = [(s, j) for s, c in enumerate(RAGGED_COUNTS) for j in range(c - RAGGED_FRONT)]
    depth = rng.permutation(len(small))                # the sub-tiles' footprints interleave in depth
    for (s, j), d in zip(small, depth):
        u.append(8 * (s & 1) + 3 + (j & 1)); v.append(8 * (s >> 1) + 3 + ((j >> 1) & 1)); z.append(3.1 + 0.002 * d)
        sig.append(SMALL_SIGMA); op.append(SMALL_OPACITY); sub_of.append(s)
    # entry 64 (from the front) of the last sub-tile's list: the front-most entry of its second segment, which that segment's pads replay
    last = [i for i in np.argsort(z) if sub_of[i] in (-1, len(RAGGED_COUNTS) - 1)]
    op[last[64]] = PAD_OPACITY
    sc = rc._scene(16, 16, u, v, z, sig, op, variant, S, seed=143)
    sc["claims"] = dict(kind="ragged", sub_of=np.array(sub_of), pad_built=(0, int(last[64])))
    return sc


def second_item(variant="rgss", S=5):
    rng = np.random.default_rng(47)
    n, W = SECOND_N, SECOND_W
    c = (W - 1) / 2.0
    sc = rc._scene(W, W, np.full(n, c), np.full(n, c), 3.0 + 0.0004 * np.arange(n), np.full(n, SECOND_SIGMA),
                   SECOND_OPACITY * rng.uniform(0.98, 1.0, n), variant, S, seed=147)
    sc["claims"] = dict(kind="second_item", n=n)
    return sc


def build(name, variant="rgss", S=5):
    return {"far_ids": far_ids, "ragged": ragged, "second_item": second_item}[name](variant, S)
