"""The scenes of tests/bwd_lds_records_cases.py hold what they claim, by the CPU oracle's own forward (no GPU): which ids are visible,
how many candidates each sub-tile consumes and which record its pad slots replay, and that the backward launch has more segments than
waves."""
import functools

import numpy as np

import bwd_lds_records_cases as lc
from oracle import oracle as orc


@functools.lru_cache(maxsize=None)
def _fwd(name):
    sc = lc.build(name)
    o = orc.OracleRun(sc, orc.RGSS)
    R = o.forward()
    return sc, o, R, o.images()


def _tile_list(o, tile=0):
    r = o.get("ranges").reshape(-1, 2)
    return o.get("point_list")[int(r[tile, 0]):int(r[tile, 1])]


def test_far_ids_visible_ids_span_the_model():
    sc, o, R, im = _fwd("far_ids")
    P, n = lc.FAR_P, lc.FAR_VISIBLE
    assert sc["means3D"].shape[0] == P and P * 96 < 2 ** 32
    ids = sc["claims"]["ids"]
    assert ids[0] == 0 and ids[-1] == P - 1 and len(np.unique(ids)) == n
    assert R == n and np.array_equal(np.sort(_tile_list(o)), ids)          # one tile, every other surfel culled
    assert np.array_equal(np.flatnonzero(im["radii"].reshape(-1) > 0), ids)
    assert (o.get("n_contrib").reshape(16, 16) == n).all()                 # every sub-tile consumes all 20: blocks of 8, 8 and 4
    assert np.array_equal(np.flatnonzero(im["weights"].reshape(-1) > 0), ids)
    # the records of one block of 8 lie far apart: consecutive list entries are megabytes from each other on average
    assert np.abs(np.diff(_tile_list(o).astype(np.int64))).mean() * 96 > 1 << 20


def _alpha_on_pixels(o, gid, xs, ys):
    m = o.get("means2D").reshape(-1, 2)[gid].astype(np.float64)
    co = o.get("conic_opacity").reshape(-1, 4)[gid].astype(np.float64)
    dx, dy = m[0] - xs, m[1] - ys
    power = -0.5 * (co[0] * dx * dx + co[2] * dy * dy) - co[1] * dx * dy
    return np.where(power > 0, 0.0, np.minimum(0.99, co[3] * np.exp(power)))


def test_ragged_sub_tiles_consume_3_8_13_70():
    sc, o, R, im = _fwd("ragged")
    lst = _tile_list(o)
    assert len(lst) == R == sum(lc.RAGGED_COUNTS) - 3 * lc.RAGGED_FRONT
    nc = o.get("n_contrib").reshape(16, 16)
    op = sc["opacities"].reshape(-1)
    built = sc["order"]                                                    # surfel id -> index it was built as
    for s, want in enumerate(lc.RAGGED_COUNTS):
        x0, y0 = 8 * (s & 1), 8 * (s >> 1)
        ys, xs = np.mgrid[y0:y0 + 8, x0:x0 + 8].astype(np.float64)
        blends, reach = [], []
        for g in lst:
            blends.append(_alpha_on_pixels(o, g, xs, ys).max() >= 1.0 / 255.0)
            m = o.get("means2D").reshape(-1, 2)[g]
            near = _alpha_on_pixels(o, g, np.clip(m[0], x0, x0 + 7), np.clip(m[1], y0, y0 + 7))   # the most the rectangle can see
            reach.append(float(near))
        blends, reach = np.array(blends), np.array(reach)
        assert blends.sum() == want                                        # the sub-tile's own candidates ...
        assert (reach[~blends] < 0.1 / 255.0).all()                        # ... and nothing else comes near its rectangle
        assert (reach[blends] >= 1.2 / 255.0).all()
        sub_of = sc["claims"]["sub_of"][built[lst]]
        assert np.array_equal(blends, (sub_of == -1) | (sub_of == s))
        # nothing saturates: the deepest candidate of the sub-tile is its last contributor, so the walk covers all `want`
        assert int(nc[y0:y0 + 8, x0:x0 + 8].max()) == int(np.flatnonzero(blends)[-1]) + 1
        # the front-most entry of every 64-candidate segment -- what the segment's pad slots replay -- is nearly opaque
        mine = lst[blends]
        for seg_lo in range(0, want, 64):
            assert op[mine[seg_lo]] == np.float32(lc.PAD_OPACITY), (s, seg_lo)
    assert sorted(int(b) for b in built[np.flatnonzero(op == np.float32(lc.PAD_OPACITY))]) == sorted(sc["claims"]["pad_built"])
    assert (im["weights"].reshape(-1) > 0).all()
    assert float(im["opacity"].max()) < 1.0 - 1e-4                         # T stays above the 1e-4 cut-off behind the opaque entries


def test_second_item_has_more_segments_than_the_launch_has_waves():
    sc, o, R, im = _fwd("second_item")
    W = lc.SECOND_W
    assert W % 16 == 0 and R == (W // 16) ** 2 * lc.SECOND_N               # every splat in every tile
    assert (im["weights"].reshape(-1) > 0).all()                           # every splat blends somewhere: the corners walk the whole list
    nc = o.get("n_contrib").reshape(W // 8, 8, W // 8, 8).max(axis=(1, 3))
    assert nc.size == 784 and nc.min() > 16 * 64 and nc.max() == lc.SECOND_N  # 17 segments or more per sub-tile
    segments = int(np.ceil(nc / 64.0).sum())
    assert segments > lc.LAUNCH_WAVES + 1000, segments
