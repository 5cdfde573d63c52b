"""LPIPS on the GPU (csrc/lpips.hip through svgir_harness/metrics.py and the drop-in lpipsPyTorch) against the fp64 oracle of
tests/lpips_cases.py, with the seeded weights of that module (unpinned by the published weights).

Bounds, eps32 = 2^-23; E32_k / EM_k = what torch's own two fp32 orders (contiguous, channels_last) lose against fp64 over the whole table,
measured from the restatements and never from a kernel (tests/test_lpips_edge_inputs.py prints them):
  tap_k    4 max(E32_k, 8 eps32) |oracle tap_k|; the score: the sum of the five bounds.  4: the project's standing margin over the reference's
           own fp32 deviation; the floor covers taps where one fp32 sample happened to land close to fp64.
  tap maps 4 max(EM_k, 8 eps32) max|map_k| per element, through the `tap_maps` output.
There are no threshold elements (ReLU and max are continuous): every element of every case is compared.  Exact zeros, symmetry, NaN,
batch independence, plane operands and repeatability are compared bit for bit.  Every output is poisoned by the binding layer, the workspace
is NaN-filled there as well (SVGIR_POISON)."""
import numpy as np
import pytest
import torch

import lpips_cases as lc

pytestmark = pytest.mark.gpu
_id = lambda c: c["id"]  # noqa: E731


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="session")
def nets(built):
    """The three seeded networks, built and packed once."""
    from svgir_harness import metrics
    out = {v: metrics.LPIPS(*lc.weights(v)) for v in ("base", "dead5", "signed")}
    for net in out.values():
        net.packed(_dev())
    return out


def _plane(o, dev):
    from svgir_harness import metrics
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    return metrics.plane(t(o["src"]), mask=t(o["mask"]), bg=o["bg"], fill=t(o["fill"]), scale=o["scale"], offset=o["offset"], srgb=o["srgb"])


def _pair(case, dev):
    return _plane(case["a"], dev), _plane(case["b"], dev)


def _run(nets, cids, maps=False):
    from svgir_harness import metrics
    dev = _dev()
    cases = [lc.BY_ID[c] for c in cids]
    res = metrics.lpips_terms(nets[cases[0]["variant"]], [_pair(c, dev) for c in cases], with_taps=True, tap_maps=maps)
    torch.cuda.synchronize()
    out = [res[0].cpu().numpy(), res[1].cpu().numpy()]
    if maps:
        out.append([m.cpu().numpy() for m in res[2]])
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_taps(cid, score, taps):
    ref = lc.oracle(cid)
    tol, tol_score = lc.tap_bounds(cid)
    err = np.abs(taps.astype(np.float64) - ref["taps"])
    print(cid, "taps", taps, "oracle", ref["taps"], "err / tol", err / np.maximum(tol, 1e-300), "score", score, float(ref["score"]),
          abs(float(score) - float(ref["score"])) / max(tol_score, 1e-300))
    assert np.all(err <= tol), (cid, err, tol)
    assert abs(float(score) - float(ref["score"])) <= tol_score, (cid, score, ref["score"], tol_score)


@pytest.mark.parametrize("case", [c for c in lc.CASES if c["expect"] != "nan"], ids=_id)
def test_taps_score_and_tap_maps_against_fp64(nets, case):
    cid = case["id"]
    score, taps, maps = _run(nets, [cid], maps=True)
    ref = lc.oracle(cid)
    for k, (got, want, tol) in enumerate(zip(maps, ref["maps"], lc.map_bounds(cid))):
        assert got.shape == want.shape, (k, got.shape, want.shape)
        err = float(np.abs(got.astype(np.float64) - want).max()) if np.isfinite(got).all() else float("inf")
        print(cid, "map", k, "max err", err, "tol", tol, "ratio", err / max(tol, 1e-300))
        assert err <= tol, (cid, k, err, tol)
    _check_taps(cid, score[0], taps[0])
    if case["expect"] == "zero":
        assert not _bits(taps).any() and not _bits(score).any()        # +0.0 in every tap
    if case["expect"] == "zero5":
        assert not maps[4].any() and _bits(taps[0, 4:5])[0] == 0 and np.all(taps[0, :4] > 0.0)


def test_the_same_tensor_twice_gives_exact_zeros(nets):
    from svgir_harness import metrics
    x = torch.from_numpy(lc.operands(lc.BY_ID["size_33x47"])[0].numpy()).to(_dev())
    score, taps = metrics.lpips_terms(nets["base"], [(x, x)], with_taps=True)
    assert not _bits(taps.cpu().numpy()).any() and not _bits(score.cpu().numpy()).any()
    out = nets["base"](x, x)
    assert tuple(out.shape) == (1, 1, 1, 1) and out.dtype == torch.float32 and out.device.type == "cuda" and float(out) == 0.0


def test_swapped_operands_give_the_same_bits(nets):
    a, b = _run(nets, ["size_33x47"]), _run(nets, ["swapped_33x47"])
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert np.all(a[1] > 0.0)


@pytest.mark.parametrize("cid", ("nan_pixel_33x47", "inf_pixel_33x47"))
def test_a_non_finite_pixel_gives_a_nan_score(nets, cid):
    score, taps = _run(nets, [cid])
    ref = lc.oracle(cid)
    print(cid, score, taps, ref["taps"])
    assert np.isnan(score[0])
    assert np.array_equal(np.isnan(taps[0]), np.isnan(ref["taps"]))
    fin = ~np.isnan(ref["taps"])
    tol, _ = lc.tap_bounds(cid)
    assert np.all(np.abs(taps[0][fin].astype(np.float64) - ref["taps"][fin]) <= tol[fin])


@pytest.mark.parametrize("batch", lc.BATCHES, ids=lambda b: f"{len(b)}_pairs")
def test_pairs_per_call_and_batch_independence(nets, batch):
    """1, 2 and 4 pairs: every pair against the oracle, and bit for bit what the same pair gives alone."""
    score, taps = _run(nets, list(batch))
    assert score.shape == (len(batch),) and taps.shape == (len(batch), 5)
    for i, cid in enumerate(batch):
        _check_taps(cid, score[i], taps[i])
        alone = _run(nets, [cid])
        assert np.array_equal(_bits(alone[0][0]), _bits(score[i])) and np.array_equal(_bits(alone[1][0]), _bits(taps[i])), cid
    if len(batch) == 4:   # and the same pair at another position, among other neighbours
        again = _run(nets, list(batch[::-1]))
        assert np.array_equal(_bits(again[1][::-1]), _bits(taps)) and np.array_equal(_bits(again[0][::-1]), _bits(score))


@pytest.mark.parametrize("case", [c for c in lc.CASES if c["id"].startswith("plane_")], ids=_id)
def test_plane_operands_against_materialised_planes(nets, case):
    """An operand composed on load has torch's bits unless it goes through sRGB (powf differs from torch's pow by ulps): bit for bit
    there, within the tap bound with sRGB."""
    from svgir_harness import metrics
    dev = _dev()
    x, y = (t.to(dev) for t in lc.operands(case))
    want = metrics.lpips_terms(nets["base"], [(x, y)], with_taps=True)
    got = metrics.lpips_terms(nets["base"], [_pair(case, dev)], with_taps=True)
    s, t = got[0].cpu().numpy(), got[1].cpu().numpy()
    _check_taps(case["id"], s[0], t[0])
    _check_taps(case["id"], want[0].cpu().numpy()[0], want[1].cpu().numpy()[0])
    if case["id"] not in lc.SRGB_CASES:
        assert np.array_equal(_bits(s), _bits(want[0].cpu().numpy())) and np.array_equal(_bits(t), _bits(want[1].cpu().numpy()))


def test_second_run_is_bit_identical_with_a_poisoned_workspace(nets):
    """The binding layer NaN-fills the workspace and the outputs before every call (SVGIR_POISON): a result that depended on the
    workspace's previous contents, or an element left unwritten, would be NaN; `out=` writes the caller's row only."""
    from gaussian_renderer import _native as N
    from svgir_harness import metrics
    assert N.POISON
    dev = _dev()
    cids = ["size_150x161", "size_150x161"]
    a = _run(nets, cids, maps=True)
    torch.full((1 << 22,), float("nan"), device=dev)   # (dirty the allocator's pool some more)
    b = _run(nets, cids, maps=True)
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all() and all(np.isfinite(m).all() for m in a[2])
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a[2], b[2]))
    assert np.array_equal(_bits(a[1][0]), _bits(a[1][1]))
    table = torch.full((3, 2), float("nan"), device=dev)
    metrics.lpips_terms(nets["base"], [_pair(lc.BY_ID[c], dev) for c in cids], out=table[1])
    t = table.cpu().numpy()
    assert np.array_equal(_bits(t[1]), _bits(a[0])) and np.isnan(t[0]).all() and np.isnan(t[2]).all()


def test_drop_in_equals_metrics_lpips(nets):
    import lpipsPyTorch
    dev = _dev()
    x, y = (t.to(dev) for t in lc.operands(lc.BY_ID["size_33x47"]))
    want = nets["base"](x, y)
    lpipsPyTorch.set_weights(*lc.weights("base"))
    try:
        got = lpipsPyTorch.lpips(x, y, net_type="vgg")
        got4 = lpipsPyTorch.lpips(x[None], y[None], net_type="vgg")
        assert lpipsPyTorch._network() is lpipsPyTorch._network()          # built once, not per call
        assert len(lpipsPyTorch._network()._packed) == 1                   # packed once per device
    finally:
        lpipsPyTorch.set_weights()
    assert tuple(got.shape) == (1, 1, 1, 1) and got.dtype == torch.float32 and got.device == want.device
    assert torch.equal(got, want) and torch.equal(got4, want)
    _check_taps("size_33x47", float(got), _run(nets, ["size_33x47"])[1][0])


def test_too_small_images_are_refused(nets):
    from svgir_harness import metrics
    x = torch.rand(3, 15, 40, device=_dev())
    with pytest.raises(ValueError, match="smaller than 16 x 16"):
        metrics.lpips_terms(nets["base"], [(x, x)])
    with pytest.raises(ValueError, match="one image size"):
        metrics.lpips_terms(nets["base"], [(torch.rand(3, 16, 16, device=_dev()), torch.rand(3, 16, 17, device=_dev()))])
