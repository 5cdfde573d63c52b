"""tests/surfel_cases.py holds what it is built for -- proved on the CPU oracle, no GPU (tests/test_gpu_surfel_edges.py then holds
csrc/preprocess.hip, csrc/geom_bwd.hip and csrc/grad_reduce.hip to the same scenes).

Also measured here, because the GPU tolerances are built from them (DESIGN.md section 5 has the tables):
  E32        per case and gradient tensor, the largest deviation of the fp32 oracle from the fp64 oracle over the blended surfels, each
             surfel's row normalised by the row's max |fp64| (surfel_cases.row_deviation: the oracle hands out no per-element sum of
             absolute pixel contributions, so this normalisation is used throughout);
  identities the fp32 oracle against the two closed forms the GPU test applies to the kernel's own outputs (dL_dsh from dL_dcolors,
             dL_dscales from dL_dcov3D), in units of eps32: at most 8, so the GPU bound stays at 16."""
import numpy as np
import pytest

import surfel_cases as sf

EPS = sf.EPS
LATTICE = [(v,) + row for v in sf.VARIANTS for row in sf.LATTICE_ROWS]
LATTICE_IDS = [f"{v}_M{m}_D{d}" + (f"_off{o}" if o else "") for v, m, d, o in LATTICE]
# every case with a backward: (id, case) -- sf.host(case) builds and caches scene, upstream gradients, fp32 and fp64 oracle
BACKWARD = ([(i, ("lattice",) + c) for i, c in zip(LATTICE_IDS, LATTICE)] + [(f"{v}_colors", ("colors", v)) for v in sf.VARIANTS] +
            [(f"{v}_coop", ("coop", v)) for v in sf.VARIANTS] + [(f"{v}_clamp{c}", ("clamp", v, c)) for v in sf.VARIANTS for c in range(3)])


def _alpha(o, sel, W, H):
    """[len(sel), H, W] alpha of the surfels `sel` at every pixel by the oracle's own conics (0 where the oracle does not blend)."""
    co = o.get("conic_opacity").reshape(-1, 4)[sel].astype(np.float64)
    xy = o.get("means2D").reshape(-1, 2)[sel].astype(np.float64)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    dx, dy = xy[:, 0, None, None] - x[None], xy[:, 1, None, None] - y[None]
    power = -0.5 * (co[:, 0, None, None] * dx * dx + co[:, 2, None, None] * dy * dy) - co[:, 1, None, None] * dx * dy
    al = np.minimum(0.99, co[:, 3, None, None] * np.exp(np.minimum(power, 0.0)))
    return np.where((power <= 0) & (al >= 1.0 / 255.0), al, 0.0)


def _masks(o, rows):
    c = o.get("clamped").reshape(-1, 3)[rows].astype(np.int64)
    return c[:, 0] + 2 * c[:, 1] + 4 * c[:, 2]


# ---- lattices ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", sf.VARIANTS)
def test_lattice_surfels_are_isolated_and_blended(variant):
    sc, _, o32, _ = sf.host(("lattice", variant, 16, 3, 0))
    al = _alpha(o32, np.arange(64), 128, 128)
    assert ((al > 0).sum(0) <= 1).all(), "a pixel blends two surfels"
    r = o32.get("radii")
    assert (r > 0).all() and (r <= 8).all(), r
    assert o32.num_rendered == 64, "one tile per surfel"
    assert (o32.get("out_weights") > 0).all()


@pytest.mark.parametrize("variant,M,D,offset", LATTICE, ids=LATTICE_IDS)
def test_lattice_holds_every_clamp_mask(variant, M, D, offset):
    sc, _, o32, o64 = sf.host(("lattice", variant, M, D, offset))
    m = _masks(o32, np.arange(64))
    assert np.array_equal(m, sc["masks"]) and np.array_equal(m, _masks(o64, np.arange(64)))
    assert (np.bincount(m, minlength=8) >= 4).all(), np.bincount(m, minlength=8)
    if M > sf.nk_of(D):
        assert np.abs(sc["shs"][:, sf.nk_of(D):]).min() > 0, "coefficients above the active degree must not be zero"


@pytest.mark.parametrize("variant,M,D,offset", [c for c in LATTICE if sf.twin_of(*c[1:]) and not c[3]],
                         ids=[i for i, c in zip(LATTICE_IDS, LATTICE) if sf.twin_of(*c[1:]) and not c[3]])
def test_row_stride_does_not_change_the_oracle(variant, M, D, offset):
    """The M / D pin: with M > (D + 1)^2 the oracle's images, R and gradients are bit-identical to the run on the leading
    coefficients alone, and dL_dsh above the active degree is exactly 0."""
    nk = sf.nk_of(D)
    for fp64 in (0, 1):
        a, b = (sf.host(("lattice", variant) + row)[2 + fp64] for row in ((M, D, 0), sf.twin_of(M, D, 0)))
        assert a.num_rendered == b.num_rendered
        ia, ib = a.images(), b.images()
        for k in ia:
            assert np.array_equal(ia[k], ib[k]), k
        ga, gb = a.grads(), b.grads()
        for k in ga:
            if k == "sh":
                assert np.array_equal(ga[k][:, :nk], gb[k]) and (ga[k][:, nk:] == 0).all()
            else:
                assert np.array_equal(ga[k], gb[k]), k


@pytest.mark.parametrize("variant", sf.VARIANTS)
def test_coop_rows_spans(variant):
    sc, _, o32, _ = sf.host(("coop", variant))
    blended = o32.get("out_weights") > 0
    assert np.array_equal(blended, sc["blended"])
    assert tuple(int(blended[128 * j:128 * j + 128].sum()) for j in range(4)) == sf.COOP_SPANS
    r = o32.get("radii")
    assert (r[sc["kinds"] == "f"] > 0).all() and (r[sc["kinds"] == "c"] == 0).all()
    al = _alpha(o32, np.nonzero(blended)[0], 256, 128)
    assert ((al > 0).sum(0) <= 1).all()
    assert (np.bincount(_masks(o32, blended), minlength=8) >= 4).all()


@pytest.mark.parametrize("variant", sf.VARIANTS)
@pytest.mark.parametrize("channel", range(3))
def test_clamp_ladder_flips_inside_the_sweep(variant, channel):
    sc, _, o32, o64 = sf.host(("clamp", variant, channel))
    c32 = o32.get("clamped").reshape(-1, 3)[:33, channel]
    c64 = o64.get("clamped").reshape(-1, 3)[:33, channel]
    assert c32[:17].all() and not c32[17:].any(), c32     # ascending values: the colour is negative up to surfel 16
    assert c64[:13].all() and not c64[21:].any(), "fp32 and fp64 disagree far from the threshold"
    print(f"clamp_ladder {variant} channel {channel}: exactly-zero colours at {len(sc['ladder_zeros'])} fp32 value(s) {sc['ladder_zeros']}, "
          f"fp32 / fp64 disagree on surfels {np.nonzero(c32 != c64)[0]}")
    rgb = o32.get("rgb").reshape(-1, 3)[:33, channel]
    for z in sc["ladder_zeros"]:     # exactly 0.0f is not clamped
        i = int(np.nonzero(sc["ladder"] == z)[0][0])
        assert rgb[i] == 0 and not c32[i]


def test_an_exactly_zero_colour_exists():
    a, zeros = sf.sh_zero_crossing()
    k = np.float32(sf.KC0)
    assert np.float32(np.float32(k * a) + np.float32(0.5)) < 0
    assert len(zeros) >= 1 and all(np.float32(np.float32(k * z) + np.float32(0.5)) == 0 for z in zeros)


# ---- cull ladders -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,variant", sf.CULL_CASES, ids=[f"{k}_{v}" for k, v in sf.CULL_CASES])
def test_cull_ladder_sits_on_its_threshold(kind, variant):
    sc = sf.cull_ladder(kind, variant)
    assert np.array_equal(np.sort(sc["ladder"]), sc["ladder"]) or np.array_equal(np.sort(sc["ladder"])[::-1], sc["ladder"])
    assert len(np.unique(sc["ladder"])) == 33 and np.abs(np.diff(sc["ladder"].view(np.int32))).max() == 1     # consecutive fp32 values
    dec = sc["decision"]
    assert dec.sum() >= 4 and (~dec).sum() >= 4, dec
    r = sf.oracle(sc, variant).get("radii")
    if kind.startswith("radius"):
        assert set(r.tolist()) == {int(kind[6:]), int(kind[6:]) + 1}, r
    else:
        assert (r == 0).sum() >= 4 and (r > 0).sum() >= 4, r
    d64 = sc["decide"](sf.oracle(sc, variant, fp64=True))
    far = np.abs(np.arange(33) - 16.5) > 8
    assert np.array_equal(dec[far], d64[far]), (dec, d64)
    print(f"cull_ladder {kind} {variant}: monotone {sc['monotone']}, fp32 / fp64 disagree on surfels {np.nonzero(dec != d64)[0]}")


# ---- list sizes -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", sf.VARIANTS)
def test_listed_scenes(variant):
    M, D = (1, 0) if variant == "svgss" else (16, 2)
    Rs = []
    for P in sf.LISTED_P[variant]:
        sc = sf.listed(variant, P, M, D)
        o = sf.oracle(sc, variant)
        Rs.append(o.num_rendered)
        blended = o.get("out_weights") > 0
        assert np.array_equal(blended, sc["blended"]) and blended.sum() == 58 + 3 == 61
        assert np.array_equal(np.nonzero(o.get("radii") > 0)[0], np.sort(sc["where"])), "exactly the 67 built for it have a radius"
        assert (o.get("tiles_touched")[sc["wide"]] >= 36).all(), o.get("tiles_touched")[sc["wide"]]
        for i in sf.LISTED_ENDS + (P - 1,):
            assert blended[i], i
        if P == sf.LISTED_P[variant][0]:
            w = sc["where"]
            al = _alpha(o, w, sf.LISTED_W, sf.LISTED_H)
            lat = al[:64].sum(0) > 0
            assert ((al[:64] > 0).sum(0) <= 1).all() and not (lat & (al[64:].sum(0) > 0)).any(), "a lattice pixel blends two surfels"
        del o, sc
    assert len(set(Rs)) == 1, Rs


# ---- what the GPU tolerances are built from ----------------------------------------------------------------------------------------

def _blended_rows(case, sc):
    return np.arange(64) if case[0] in ("lattice", "colors", "clamp") else np.nonzero(sc["blended"])[0]


@pytest.mark.parametrize("name,case", BACKWARD, ids=[b[0] for b in BACKWARD])
def test_fp32_oracle_against_fp64_and_the_closed_forms(name, case):
    sc, _, o32, o64 = sf.host(case)
    rows = _blended_rows(case, sc)
    g32, g64 = o32.grads(), o64.grads()
    if case[0] == "clamp":     # (the one or two values where fp32 and fp64 disagree on the sign)
        rows = rows[(o32.get("clamped") == o64.get("clamped")).reshape(-1, 3)[rows].all(1)]
    e = sf.e32(g32, g64, rows)
    print("E32 " + name + ": " + "  ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert all(np.isfinite(v) for v in e.values()), e
    # surface mode: no gradient reaches the third scale
    assert (g32["scales"][:, 2] == 0).all() and (g64["scales"][:, 2] == 0).all()
    rows = _blended_rows(case, sc)
    for o, g in ((o32, g32), (o64, g64)):
        val, mag = sf.scale_grad_from_cov(sc, g["cov3D"])
        err = (np.abs(g["scales"][:, :2] - val)[rows] / mag[rows]).max() / EPS
        if "shs" in sc:
            err_sh = sf.sh_identity_error(sc, g["sh"], g["colors"], o.get("clamped").reshape(-1, 3) > 0, rows)
        else:
            err_sh = 0.0
        print(f"identities {name} ({'fp64' if o is o64 else 'fp32'}): dL_dscales {err:.2f} eps32, dL_dsh {err_sh:.2f} eps32")
        assert err <= 8 and err_sh <= 8
