"""The image-space edge cases on the fp64 oracle alone (no GPU): every case of tests/image_cases.py holds what it is named for, at most
5 % of its pixels sit on a threshold, at most 15 % of a depth2normal run's pixels are excluded as degenerate, the reference arithmetic
stays finite outside the non-finite cases, the clamp_min tie passes its gradient, and what the reference's own fp32 arithmetic loses on
the SSIM cases (E32, the yardstick of tests/test_gpu_image_edges.py) is measured and held below the recorded ceilings.

Run with -s for the counts and the E32 table; DESIGN.md section 5, "Image-space edge inputs", holds the measured figures."""
import numpy as np
import pytest
import torch

import image_cases as ic
from oracle import epilogue_oracle as eo

SVGSS_RUNS = [r for r in ic.UNPACK_RUNS if r["mode"] != "rgss"]
RGSS_RUNS = [r for r in ic.UNPACK_RUNS if r["mode"] == "rgss"]
_id = lambda r: r["id"]  # noqa: E731


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _oracle_grads(run, d, dtype=torch.float64):
    """Outputs and autograd gradients of the torch restatement under the run's upstream weights (zero on threshold / poisoned pixels)."""
    bg = ic.BACKGROUNDS[run["bg"]]
    keep = ~(ic.threshold_pixels(ic.probe(d, run["mode"], bg)) | ic.nonfinite_pixels(d))
    lv = {k: torch.from_numpy(d[k]).to(dtype).requires_grad_(True) for k in ("opacity", "feature", "vfeature")}
    res = eo.unpack_svgss_torch(lv["opacity"], lv["feature"], lv["vfeature"], torch.tensor(bg, dtype=dtype), run["mode"] == "train")
    names = [g[0] for g in ic.GROUPS[run["mode"]]]
    w = ic.unpack_weights(run, {k: tuple(res[k].shape) for k in names}, keep)
    sum((res[k] * w[k].to(dtype)).sum() for k in names).backward()
    return res, {k: v.grad for k, v in lv.items()}, keep


@pytest.mark.parametrize("run", SVGSS_RUNS, ids=_id)
def test_probe_restates_the_oracle_and_few_pixels_sit_on_a_threshold(run):
    d = ic.build_unpack(run)
    bg = ic.BACKGROUNDS[run["bg"]]
    S, VC = ic.PLANES[run["mode"]]
    assert d["opacity"].shape == (1, run["H"], run["W"]) and d["feature"].shape[0] == S and d["vfeature"].shape[0] == VC
    assert all(d[k].dtype == np.float32 for k in ("opacity", "feature", "vfeature"))
    p = ic.probe(d, run["mode"], bg)
    ref = eo.unpack_svgss(d["opacity"], d["feature"], d["vfeature"], bg, run["mode"] == "train")
    for k, v in ic.rebuild(p, d, bg).items():
        assert np.array_equal(np.broadcast_to(ref[k], v.shape), v, equal_nan=True), k
    thr, bad = ic.threshold_pixels(p), ic.nonfinite_pixels(d)
    assert thr.mean() <= ic.MAX_THRESHOLD_SHARE and bad.mean() <= 0.05, (thr.mean(), bad.mean())
    assert np.array_equal(bad, d["special"])
    # the reference arithmetic is finite everywhere outside the poisoned pixels, gradients on the threshold pixels included
    res, grads, keep = _oracle_grads(run, d)
    for k in p:
        assert np.isfinite(ref[k][..., ~bad]).all(), k
    for k, g in grads.items():
        assert torch.isfinite(g[..., torch.from_numpy(~bad)]).all(), k
    assert keep.mean() >= 0.9 or run["H"] * run["W"] == 1


def _sides(x, b):
    with np.errstate(invalid="ignore"):
        return int((x < b).sum()), int((x == b).sum()), int((x > b).sum())


@pytest.mark.parametrize("run", [r for r in SVGSS_RUNS if r["case"] == "opacity_ends" and r["H"] * r["W"] >= ic.BLOCK], ids=_id)
def test_opacity_ends_holds_every_opacity_class(run):
    d = ic.build_unpack(run)
    op = d["opacity"][0]
    raw_any = (d["vfeature"] != 0).any(0)
    counts = {float(v): int((op == v).sum()) for v in ic.OPACITY_ENDS}
    print(run["id"], counts, "o = 0 with raw = 0 / != 0:", int(((op == 0) & ~raw_any).sum()), int(((op == 0) & raw_any).sum()))
    assert len(counts) == 9 and min(counts.values()) >= run["H"] * run["W"] // 9 - 1 >= 27
    below, tie, above = _sides(op, ic.OPMIN)
    assert tie > 0 and below >= 3 * (tie - 1) and above >= 5 * (tie - 1)     # three classes below the clamp, five above
    assert ((op == 0) & ~raw_any).sum() >= 10 and ((op == 0) & raw_any).sum() >= 10
    # o = 0 with a non-zero plane: x = plane * 1e5 is an ordinary value
    x = ic.probe(d, run["mode"], ic.BACKGROUNDS[run["bg"]])["roughness"]["x"][0][(op == 0) & raw_any]
    assert 0.19 < x.min() and x.max() < 0.96
    # every plane kind is present in both modes' tables
    assert {g[1] for g in ic.GROUPS[run["mode"]]} >= {ic.SRGB_OF_OVER, ic.PLAIN, ic.OVER_SRGB, ic.OVER_LIN}
    assert run["mode"] == "train" or ic.SRGB in {g[1] for g in ic.GROUPS["eval"]}


@pytest.mark.parametrize("run", [r for r in SVGSS_RUNS if r["case"] == "srgb_knee_and_clips" and r["H"] * r["W"] >= ic.BLOCK], ids=_id)
def test_srgb_knee_and_clips_reaches_every_bound_from_both_sides_in_every_plane_kind(run):
    d = ic.build_unpack(run)
    p = ic.probe(d, run["mode"], ic.BACKGROUNDS[run["bg"]])
    assert set(np.unique(d["opacity"])) == {0.25, 0.5, 1.0}
    thr = ic.threshold_pixels(p)
    by_kind = {}
    for q in p.values():
        if q["arg"] is not None:
            by_kind.setdefault(q["kind"], []).append(q)
    assert set(by_kind) == ({ic.SRGB_OF_OVER, ic.OVER_SRGB} | ({ic.SRGB} if run["mode"] == "eval" else set()))
    for kind, qs in by_kind.items():
        arg = np.concatenate([q["arg"] for q in qs])
        y = np.concatenate([q["y"] for q in qs])
        off = np.broadcast_to(~thr, arg.shape[1:])[None].repeat(arg.shape[0], 0)    # counted on the pixels whose gradients are compared
        knee = _sides(arg[off], float(ic.KNEE))
        lo = _sides(y[off], 0.0)
        hi = _sides(y[off], 1.0)
        on_knee, on_one = int(ic.near(arg, float(ic.KNEE)).sum()), int(ic.near(y, 1.0).sum())
        print(f"{run['id']} {kind}: knee below / tie / above {knee}, clip 0 {lo}, clip 1 {hi}; on the knee {on_knee}, on 1 {on_one}")
        # (the unclipped sRGB of 1 is 1 - 1 ulp: the tie y == 1 is not reachable; x = 1 counts among the values on the bound)
        assert min(knee) >= 1 and min(lo) >= 1 and hi[0] >= 1 and hi[2] >= 1 and on_knee >= 2 and on_one >= 3


@pytest.mark.parametrize("run", [r for r in ic.UNPACK_RUNS if r["case"] == "nonfinite"], ids=_id)
def test_nonfinite_poisons_few_scattered_pixels_of_each_kind(run):
    d = ic.build_unpack(run)
    sp = d["special"]
    assert 0 < sp.mean() <= 0.05
    planes = np.concatenate([d["feature"], d["vfeature"]]) if run["mode"] != "rgss" else d["feature"]
    kinds = (int(np.isnan(planes).sum()), int(np.isposinf(planes).sum()), int(np.isneginf(planes).sum()), int(np.isnan(d["opacity"]).sum()))
    print(run["id"], "NaN / +Inf / -Inf plane entries, NaN opacities:", kinds)
    assert min(kinds) >= 1
    assert (~np.isfinite(planes)).sum(0).max() == 1 and not (np.isnan(d["opacity"][0]) & ~np.isfinite(planes).all(0)).any()
    if run["H"] > 1:
        assert len(np.unique(np.nonzero(sp)[0])) >= 3 and len(np.unique(np.nonzero(sp)[1])) >= 3    # scattered, no run of pixels


@pytest.mark.parametrize("run", RGSS_RUNS, ids=_id)
def test_rgss_cases_cross_opacity_classes_with_contributor_counts(run):
    d = ic.build_unpack(run)
    ref = eo.unpack_rgss(d["num_contrib"], d["opacity"], d["depth"], d["feature"])
    bad = ic.nonfinite_pixels(d)
    assert np.array_equal(bad, d["special"]) and bad.mean() <= 0.05
    for k in ic.RGSS_KEYS:
        assert np.isfinite(ref[k][..., ~bad]).all(), k
    tt = eo.unpack_rgss_torch(torch.from_numpy(d["num_contrib"]), _t(d["opacity"]), _t(d["depth"]), _t(d["feature"]))
    for k in ref:
        assert np.array_equal(tt[k].numpy(), ref[k], equal_nan=True), k
    if run["case"] == "opacity_ends" and run["H"] * run["W"] >= ic.BLOCK:
        op, nc = d["opacity"][0], d["num_contrib"]
        table = {(float(o), n): int(((op == o) & (nc == n)).sum()) for o in ic.OPACITY_ENDS for n in ic.NUM_CONTRIB}
        print(run["id"], "smallest (opacity, num_contrib) class:", min(table.values()))
        assert min(table.values()) >= 5          # num_contrib = 0 with o > 0 and num_contrib > 0 with o = 0 among them


def test_the_clamp_min_tie_passes_the_gradient():
    """torch's clamp_min passes the gradient at self >= min: at o = float32(1e-5) d(raw / o.clamp_min(1e-5)) / do = -raw / o^2 in the
    reference's fp32, and in the fp64 oracle with the threshold rounded where the reference rounds it (float32(1e-5) < double 1e-5:
    unrounded, the oracle would clamp there and return 0)."""
    raw = np.float32(0.37e-5)
    for dtype in (torch.float32, torch.float64):
        o = torch.tensor([[[float(ic.OPMIN)]]], dtype=dtype, requires_grad=True)
        f = torch.zeros(4, 1, 1, dtype=dtype)
        vf = torch.zeros(13, 1, 1, dtype=dtype)
        vf[6] = float(raw)                                   # a normal plane: passed through as x = raw / o
        res = eo.unpack_svgss_torch(o, f, vf, torch.zeros(3, dtype=dtype), True)
        res["normal"][0].sum().backward()
        want = -float(raw) / float(ic.OPMIN) ** 2
        assert float(o.grad) == pytest.approx(want, rel=1e-6) and abs(want) > 3e4, (dtype, float(o.grad))
        r = eo.unpack_rgss_torch(torch.ones(1, 1, dtype=torch.int32), o, torch.ones(1, 1, 1, dtype=dtype), vf[4:9])
        g, = torch.autograd.grad(r["feature_normal"].sum(), o)
        assert float(g) == pytest.approx(want, rel=1e-6)
    below = torch.tensor([[[float(np.nextafter(ic.OPMIN, np.float32(0)))]]], dtype=torch.float64, requires_grad=True)
    eo.unpack_svgss_torch(below, f.double(), vf.double(), torch.zeros(3, dtype=torch.float64), True)["normal"][0].sum().backward()
    assert float(below.grad) == 0.0
    assert eo.unpack_svgss(np.full((1, 1, 1), ic.OPMIN), f.numpy(), vf.numpy(), np.zeros(3), True)["normal"][0, 0, 0] == float(raw) / float(ic.OPMIN)


def test_nonfinite_values_propagate_through_the_restatements():
    """torch.clamp / clamp_min propagate NaN: a NaN plane or opacity is a NaN result, never a valid-looking pixel."""
    run = next(r for r in SVGSS_RUNS if r["case"] == "nonfinite" and r["mode"] == "eval" and r["H"] == 37)
    d = ic.build_unpack(run)
    bg = ic.BACKGROUNDS[run["bg"]]
    ref = eo.unpack_svgss(d["opacity"], d["feature"], d["vfeature"], bg, False)
    tt = eo.unpack_svgss_torch(_t(d["opacity"]), _t(d["feature"]), _t(d["vfeature"]), _t(bg), False)
    nan_op = np.isnan(d["opacity"][0])
    for k in [g[0] for g in ic.GROUPS["eval"]]:
        a, b = np.broadcast_to(ref[k], tt[k].shape), tt[k].numpy()
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), k
        np.testing.assert_allclose(a, b, rtol=1e-13, atol=0, err_msg=k)
        assert np.isnan(ref[k][:, nan_op]).all(), k
    assert np.isnan(ref["lights"][1][np.isnan(d["feature"][1])]).all()
    assert np.array_equal(ref["lights"][1][np.isposinf(d["feature"][1])], (d["opacity"][0].astype(np.float64) + (1 - d["opacity"][0].astype(np.float64)) * bg[1])[np.isposinf(d["feature"][1])])


# ---- depth2normal ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ic.D2N_RUNS, ids=_id)
def test_depth2normal_runs_stay_inside_the_degenerate_cap(run):
    depth, mask, n, gd, excl = ic.d2n_reference(run)
    H, W = run["H"], run["W"]
    assert depth.shape == mask.shape == (1, H, W) and depth.dtype == mask.dtype == np.float32
    n_np = eo.depth2normal(depth, mask, ic.FOVX, ic.FOVY, run["prcp"])               # torch and numpy restatements agree
    assert np.abs(n - n_np).max() <= 1e-12 and np.array_equal(n == 0, n_np == 0)
    assert np.isfinite(n).all() and np.isfinite(gd).all()
    all_degenerate = min(H, W) == 1 or run["mask"] == "zeros"
    print(f"{run['id']}: excluded {excl.mean():.3f}, masked out {1 - mask.mean():.3f}, depth-0 pixels {(depth == 0).sum()}")
    if all_degenerate:
        assert not n.any()                       # one row / one column: two of the four differences vanish everywhere
        if H * W == 1 or run["mask"] == "zeros":
            assert not gd.any()
    elif run["grad"]:
        assert excl.mean() <= ic.MAX_DEGENERATE_SHARE
        assert (np.abs(n).sum(0) > 0)[mask[0] != 0].mean() > 0.9
    else:
        assert run["mask"] == "checker" and excl.all()
    if run["depth"] == "holes" and H * W > 1:
        assert (depth == 0).sum() >= 1
    if H * W > 1:
        want = {"ones": mask.all(), "zeros": not mask.any(), "checker": abs(mask.mean() - 0.5) < 0.02}
        assert want.get(run["mask"], 0 < (mask == 0).sum() < mask.size)


def test_depth2normal_table_covers_the_sizes_scales_and_masks():
    runs = ic.D2N_RUNS
    assert {(r["H"], r["W"]) for r in runs} == set(ic.D2N_SIZES) and {r["prcp"] for r in runs} == set(ic.PRCP)
    big = [r for r in runs if (r["H"], r["W"]) == (37, 29)]
    assert {r["mask"] for r in big} == set(ic.MASKS) and {r["depth"] for r in big} == {"plane1", "plane1e-3", "plane1e4", "holes"}
    assert ic.FOVX != ic.FOVY and 37 * 29 % ic.BLOCK and 37 * 29 > ic.BLOCK
    _, mask = ic.build_d2n(next(r for r in big if r["mask"] == "border_holes"))
    m = mask[0]
    assert not (m[0, 0] or m[-1, -1] or m[0, -2] or m[-2, 0]) and m[0, -1] and m[-1, 0] and (m[0, 1:-1] == 0).any() \
        and (m[-1, 1:-1] == 0).any() and (m[1:-1, 0] == 0).any() and (m[1:-1, -1] == 0).any()
    run = next(r for r in big if r["mask"] == "border_holes")
    deg, _ = ic.d2n_excluded(ic.d2n_reference(run)[2], mask)
    assert deg[0, -1] and deg[-1, 0] and run["grad"]        # the 1 / eps branch of the adjoint is reached, beside compared pixels
    _, mask = ic.build_d2n(next(r for r in big if r["mask"] == "isolated"))
    z = np.argwhere(mask[0] == 0)
    assert len(z) >= 3 and all(0 < y < 36 and 0 < x < 28 for y, x in z)


# ---- L1 + SSIM ---------------------------------------------------------------------------------------------------------------------
def test_ssim_table_covers_the_shapes_and_contents():
    assert {(r["C"], r["H"], r["W"]) for r in ic.SSIM_RUNS} == set(ic.SSIM_SHAPES) and {r["content"] for r in ic.SSIM_RUNS} == set(ic.SSIM_CONTENTS)
    assert max(ic.partials(r) for r in ic.SSIM_RUNS) == 330 > 256        # the reduce kernel's loop strides
    assert sum(1 for r in ic.SSIM_RUNS if max(r["H"], r["W"]) <= 11) >= 3   # the image is smaller than the window
    assert {r["C"] for r in ic.SSIM_RUNS} == {1, 2, 3}


@pytest.mark.parametrize("run", ic.SSIM_RUNS, ids=_id)
def test_ssim_cases_and_the_fp32_loss_of_the_reference_arithmetic(run):
    img, gt = ic.build_ssim(run)
    assert img.dtype == gt.dtype == torch.float32 and tuple(img.shape) == (run["C"], run["H"], run["W"])
    fin = img[torch.isfinite(img)]
    assert 0 <= float(fin.min()) and float(fin.max()) <= 1 and 0 <= float(gt.min()) and float(gt.max()) <= 1
    r64, r32 = ic.ssim_reference(run), ic.ssim_reference(run, torch.float32)
    c = run["content"]
    if c == "nan":
        assert int(torch.isnan(img).sum()) == 1
        assert all(np.isnan(r[k]) for r in (r64, r32) for k in ("l1", "ssim"))
        return
    if c == "flat":
        assert len(torch.unique(gt)) == 1 and len(torch.unique(img)) == 2
    if c == "sat":
        assert set(torch.unique(gt).tolist()) == {0.0, 1.0} and float((img != gt).float().mean()) > 0.1
        assert float((img == 0).float().mean()) > 0.2 and float((img == 1).float().mean()) > 0.2
    if c == "equal":
        same = (img == gt)
        assert 0.4 < float(same.float().mean()) < 0.9 and not r64["d_l1"][same.numpy()].any()
    assert all(np.isfinite(r[k]).all() for r in (r64, r32) for k in r)
    ev, eg, lv, lg = ic.ssim_e32(r64, r32)
    print(f"{run['id']}: E32 ssim {ev:.2e} grad {eg:.2e} | l1 {lv:.2e} grad {lg:.2e} | ssim {r64['ssim']:.6f}")
    cv, cg = ic.SSIM_CEILING[c]
    assert ev <= cv and eg <= cg, (ev, eg)
    assert lv <= 1e-7 and lg <= 1e-6
