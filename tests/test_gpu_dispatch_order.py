"""The dispatch order the cull publishes for the composite forward (csrc/common.hpp DISP_NCLS): size-class buckets filled with atomics,
gradient rows and state slots allocated in the order the cull's workgroups finish, the empty sub-tiles written by the waves behind the
non-empty count -- at the smallest shapes where such a queue can go wrong.  Helpers and budgets are tests/test_gpu_parity.py's, unchanged;
each scene's size claims are shown on the oracle by tests/test_binning_scenes.py and tests/test_edge_scenes.py.  SVGIR_POISON is on
(tests/conftest.py): a pixel no wave writes is NaN and fails the comparison."""
import numpy as np
import pytest
import torch

import test_gpu_parity as gp
from oracle import oracle as orc
from svgir_harness import runner, scenes

pytestmark = pytest.mark.gpu
SCOPE0 = 7600       # workload scopes of this file
# (variant, S, VS): the specialised widths of the two rasterizers (svgss: gradient rows) and one run-time width each
WIDTHS = [("svgss", 3, 8), ("rgss", 5, 0)]
RUNTIME = [("svgss", 2, 0), ("rgss", 7, 0)]
IDS = lambda ws: [f"{v}_S{S}_VS{VS}" for v, S, VS in ws]


def _check(sc, variant, backward=True, seed=7):
    """Forward images, integer state and (fp64-anchored) gradients of one view against the oracle."""
    grads = scenes.upstream_grads(sc, variant, seed=seed) if backward else None
    out, leaves, o, R = gp._run_both(sc, variant, grads)
    gp._check_forward(out, o, R, variant)          # (not finite = a pixel nobody wrote)
    gp._check_binning(sc, variant, o, R)
    if backward:
        gp._check_backward(leaves, o, variant, exact=gp._exact_grads(sc, variant, grads, R))
    return out, leaves, o, R


@pytest.mark.parametrize("variant,S,VS", WIDTHS + RUNTIME, ids=IDS(WIDTHS + RUNTIME))
def test_mostly_empty_image(built, variant, S, VS):
    """A twentieth of the tiles hold everything: the other pixels are the background, written by waves without a sub-tile of their own."""
    sc = scenes.binning_scene(variant, gx=5, gy=3, layout="skewed", P=3000, S=S, VS=VS)
    assert len(np.unique(sc["plan"]["tile"])) <= 2
    out, _, o, _ = _check(sc, variant)
    bgpix = o.get("n_contrib").reshape(sc["H"], sc["W"]) == 0
    assert bgpix.mean() > 0.8
    assert np.array_equal(out["color"].detach().cpu().numpy()[:, bgpix], o.images()["color"][:, bgpix])


@pytest.mark.parametrize("variant,S,VS", WIDTHS, ids=IDS(WIDTHS))
def test_one_list_beyond_the_top_class(built, variant, S, VS):
    """3000 candidates in one tile (the class every count above 1008 shares), nothing anywhere else."""
    sc = scenes.binning_scene(variant, layout="one", P=3000, S=S, VS=VS)
    _check(sc, variant)


@pytest.mark.parametrize("variant,S,VS", WIDTHS, ids=IDS(WIDTHS))
def test_all_subtiles_in_one_class(built, variant, S, VS):
    """Every tile of the 8 x 6 grid holds 1 .. 16 surfels: all 192 sub-tiles fall into the last class, spread over its eight shards."""
    sc = scenes.binning_scene(variant, gx=8, gy=6, layout="uniform", P=288, seed=0, S=S, VS=VS)
    cnt = np.bincount(sc["plan"]["tile"], minlength=48)
    assert cnt.min() >= 1 and cnt.max() <= 16, (cnt.min(), cnt.max())
    _check(sc, variant)


@pytest.mark.parametrize("variant,S,VS", WIDTHS + RUNTIME[:1], ids=IDS(WIDTHS + RUNTIME[:1]))
def test_image_not_a_multiple_of_the_tile(built, variant, S, VS):
    """200 x 136: the last tile column is half inside, the last tile row too -- sub-tiles partly and wholly outside the image."""
    sc = scenes.random_cloud(P=10000, W=200, H=136, variant=variant, S=S, VS=VS)
    _check(sc, variant)


@pytest.mark.parametrize("terminate", [False, True], ids=["all_blend", "terminate"])
@pytest.mark.parametrize("variant,S,VS", WIDTHS, ids=IDS(WIDTHS))
def test_slot_and_row_bases_of_multi_segment_stacks(built, variant, S, VS, terminate):
    """Lists of 1 .. 193 candidates: up to four state slots per sub-tile, rows and slots wherever the cull's allocation put them."""
    _check(scenes.stack_scene(variant, terminate=terminate, S=S, VS=VS), variant)


@pytest.mark.parametrize("variant,S,VS", WIDTHS, ids=IDS(WIDTHS))
def test_slot_and_row_bases_of_a_random_cloud(built, variant, S, VS):
    sc = scenes.random_cloud(P=10000, W=256, H=256, variant=variant, S=S, VS=VS)
    _check(sc, variant)


@pytest.mark.parametrize("variant", ["svgss", "rgss"])
def test_fully_culled_view_between_two_others(built, variant):
    """Nothing non-empty: no dispatch entry, no allocation, totals of zero -- and the workload's history continues behind it."""
    from gaussian_renderer import _native
    kw = dict(P=3000, seed=3, gx=8, gy=6)
    full = scenes.binning_scene(variant, **kw)
    none = scenes.binning_scene(variant, n_culled=3000, **kw)
    scope = SCOPE0 + (0 if variant == "svgss" else 1)
    _native.reset_workload_history(scope)
    before = _native.speculation_stats()
    with _native.workload_scope(scope):
        for sc in (full, none, full):
            o = orc.OracleRun(sc, orc.SVGSS if variant == "svgss" else orc.RGSS)
            R = o.forward()
            raw = runner.forward_raw(runner.to_torch(sc, gp._dev()), variant)
            torch.cuda.synchronize()
            gp._check_forward(raw, o, R, variant)
            gp._check_binning_raw(raw, o, R)
            if sc is none:
                assert R == 0 and not raw["ranges"].any() and not raw["n_contrib"].any()
                assert np.array_equal(raw["color"].cpu().numpy(), o.images()["color"])
            else:
                assert R == 3000
    assert _native.speculation_stats()["rerun_capacity"] == before["rerun_capacity"]


@pytest.mark.parametrize("variant,S,VS", WIDTHS, ids=IDS(WIDTHS))
def test_placement_does_not_leak_into_values(built, variant, S, VS):
    """The same view twice, into fresh blobs: rows and slots may land elsewhere, images and n_contrib are bit-identical, and so are the
    svgss gradients (grad_reduce sums a Gaussian's rows in emit order); rgss gradients and out_weights are sums of unordered float
    atomics and stay within the budgets of every other test here."""
    sc = scenes.random_cloud(P=10000, W=200, H=136, variant=variant, S=S, VS=VS, seed=5)
    grads = scenes.upstream_grads(sc, variant, seed=3)
    sct = runner.to_torch(sc, gp._dev())
    runs = []
    for _ in range(2):
        out, leaves = runner.render(sct, variant, requires_grad=True)
        runner.backward(out, grads, variant)
        raw = runner.forward_raw(sct, variant)
        torch.cuda.synchronize()
        runs.append(({k: out[k].detach().clone() for k in ("color", "normal", "depth", "opacity", "feature", "vfeature") if k in out},
                     raw["n_contrib"].copy(),
                     {k: v.grad.clone() for k, v in leaves.items() if v.grad is not None}))
    for k in runs[0][0]:
        assert torch.equal(runs[0][0][k], runs[1][0][k]), k
    assert np.array_equal(runs[0][1], runs[1][1])
    assert set(runs[0][2]) == set(runs[1][2]) and len(runs[0][2]) >= 5
    if variant == "svgss":
        for k in runs[0][2]:
            assert torch.equal(runs[0][2][k], runs[1][2][k]), k


def test_slot_capacity_miss_redumps_through_the_lookup(built):
    """small -> large -> small in one scope: the stacked view needs far more state slots than its speculative capacity, its backward
    replays the composite for the states alone -- the same dispatch lookup, the same slot bases -- and all gradients match the oracle."""
    from gaussian_renderer import _native
    spread = scenes.surface_scene(P=9000, W=512, H=512, seed=91, sh_degree=1, variant="svgss", S=4, VS=52, scale_lo=0.003, scale_hi=0.004)
    stacked = dict(spread)
    rng = np.random.default_rng(92)
    stacked["means3D"] = (0.004 * rng.normal(size=spread["means3D"].shape)).astype(np.float32)
    stacked["opacities"] = (spread["opacities"] * 0.02).astype(np.float32)   # translucent: the lists are consumed to the end
    campos = np.asarray(spread["campos"], dtype=np.float64)
    behind = campos + 2.0 * campos / np.linalg.norm(campos)                   # every second surfel behind the camera: the instance capacity holds
    stacked["means3D"][1::2] = (behind + 0.01 * rng.normal(size=stacked["means3D"][1::2].shape)).astype(np.float32)
    # (the default scope: the autograd thread that runs a view's backward, where its slot total enters the history, carries no other)
    _native.reset_workload_history(0)
    before = _native.speculation_stats()
    for sc in (spread, spread, stacked, spread):
        grads = scenes.upstream_grads(sc, "svgss", seed=5)
        out, leaves, o, R = gp._run_both(sc, "svgss", grads)
        gp._check_forward(out, o, R, "svgss")
        gp._check_backward(leaves, o, "svgss")
        # State slots: a sub-tile with n >= 64 candidates owns n // 64 + 1.  No TILE list of the spread views reaches 64, so they own none
        # and the stacked view gets the floor capacity of 64; its ~2200 surfels per centre tile leave lists of more than a thousand
        # candidates in at least the four sub-tiles around the image centre (that it did exceed the capacity: rerun_slots below).
        rg = o.get("ranges").reshape(-1, 2).astype(np.int64)
        assert (int((rg[:, 1] - rg[:, 0]).max()) < 64) == (sc is not stacked)
    after = _native.speculation_stats()
    assert after["rerun_capacity"] == before["rerun_capacity"]
    assert after["rerun_slots"] == before["rerun_slots"] + 1
