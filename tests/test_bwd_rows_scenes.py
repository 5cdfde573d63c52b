"""The scenes of tests/bwd_rows_cases.py hold what they claim, by the CPU oracle's own forward (no GPU): consumed counts, saturation,
which surfels receive a blend weight, and the depth order the block pairs of the backward composite depend on."""
import functools

import numpy as np
import pytest

import bwd_rows_cases as rc
from oracle import oracle as orc


@functools.lru_cache(maxsize=None)
def _fwd(name):
    sc = rc.build(name)
    o = orc.OracleRun(sc, orc.RGSS)
    R = o.forward()
    im = o.images()
    return sc, o, R, im


def _tile_list(o, tile=0):
    r = o.get("ranges").reshape(-1, 2)
    return o.get("point_list")[int(r[tile, 0]):int(r[tile, 1])]


@pytest.mark.parametrize("n", rc.COUNTS)
def test_stack_consumes_exactly_n(n):
    sc, o, R, im = _fwd(f"stack{n}")
    assert R == n and len(_tile_list(o)) == n
    nc = o.get("n_contrib").reshape(16, 16)
    assert (nc == n).all()                                   # every pixel of every sub-tile blends down to the deepest splat
    assert (im["weights"].reshape(-1) > 0).all()
    assert float(im["opacity"].max()) < 1.0 - 1e-3           # T stays far above the 1e-4 cut-off: nothing saturates


def test_live_bits_blocks():
    sc, o, R, im = _fwd("live_bits")
    kind = sc["claims"]["built"][sc["order"]]                # class of surfel id i
    w, radii = im["weights"].reshape(-1), im["radii"].reshape(-1)
    assert ((w > 0) == (kind == "h")).all() and (radii[kind == "m"] > 0).all()
    lst = _tile_list(o)
    assert len(lst) == 16 + 64
    # front to back: 8 hits, the 64 misses, 8 hits; per sub-tile the misses keep that order, 16 each (their centres lie inside its rectangle)
    assert "".join(kind[lst]) == "h" * 8 + "m" * 64 + "h" * 8
    assert (o.get("n_contrib").reshape(16, 16) == 80).all()  # the deepest hit is every pixel's last contributor: nothing is skipped
    assert float(im["opacity"].max()) < 1.0 - 1e-3


def test_live_bits_misses_sit_between_pixels_of_their_sub_tile():
    sc, o, R, im = _fwd("live_bits")
    kind = sc["claims"]["built"][sc["order"]]
    c = o.get("means2D").reshape(-1, 2)[kind == "m"].astype(np.float64)
    co = o.get("conic_opacity").reshape(-1, 4)[kind == "m"].astype(np.float64)
    frac = c - np.floor(c)
    assert np.abs(frac - 0.5).max() < 1e-3                   # 0.71 px from the four nearest pixels
    sub = (np.floor(c[:, 0]) // 8 + 2 * (np.floor(c[:, 1]) // 8)).astype(int)
    assert np.array_equal(np.bincount(sub, minlength=4), [16, 16, 16, 16])
    assert (c % 8 > 0.4).all() and (c % 8 < 6.6).all()       # inside the rectangle [x0, x0 + 7] the cull tests, 1.4 px or more from the neighbour's
    # alpha at the centre passes the cull's 1/255, alpha at the nearest pixel does not blend, the neighbouring rectangle is out of reach
    q_pix = (co[:, 0] + co[:, 2] - 2 * np.abs(co[:, 1])) * 0.499 ** 2     # least value of the conic form at the four nearest pixels
    assert (co[:, 3] >= 1.2 / 255.0).all() and (co[:, 3] * np.exp(-0.5 * q_pix) < 0.8 / 255.0).all()
    assert (co[:, 3] * np.exp(-0.5 * np.minimum(co[:, 0], co[:, 2]) * 1.4 * 1.4) < 0.1 / 255.0).all()


@pytest.mark.parametrize("front,behind", rc.START_PAST)
def test_start_past_whole_blocks(front, behind):
    sc, o, R, im = _fwd(f"start_past_{front}_{behind}")
    cl = sc["claims"]
    assert len(_tile_list(o)) == cl["total"] <= 64
    nc = o.get("n_contrib").reshape(16, 16)
    # every pixel saturates on the opaque splats: the third is blended nowhere (behind a translucent front not even the second), and the four
    # sub-tiles have the same deepest contributor
    sub_max = nc.reshape(2, 8, 2, 8).max(axis=(1, 3))
    last = int(sub_max.max())
    assert (sub_max == last).all() and last in cl["last"] and nc.min() >= last - 1
    assert float(im["opacity"].min()) > 0.99 and int(nc.max()) < cl["total"]     # (a pixel ends on the splat that would take T below 1e-4)
    w = im["weights"].reshape(-1)
    built_rank = sc["order"]                                 # surfels were built in depth order
    assert ((w > 0) == (built_rank < last)).all()
    # the forward consumes its whole first staging batch: total - last entries lie behind every pixel; the replay skips whole blocks
    nskip = cl["total"] - last
    assert nskip // 8 * 8 == cl["cstart"] >= 8
    assert (cl["cstart"] // 8) % 2 == (1 if behind in (8, 24) else 0)


@pytest.mark.parametrize("P", rc.ALIGN_P)
def test_alignment_blended_ids(P):
    sc, o, R, im = _fwd(f"align{P}")
    w = im["weights"].reshape(-1)
    assert np.array_equal(w > 0, sc["claims"]["blended"])
    assert sc["claims"]["blended"][-1] and sc["claims"]["blended"][:min(P, 8)].sum() >= min(P, 8) - 1
    if P == 13:
        assert sc["claims"]["blended"][:8].all()
