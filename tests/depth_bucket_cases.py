"""The case table of the depth sort's bucket plan (csrc/depth_sort_plan.hpp, csrc/binning.hip launch_depth_bucket_sort): under a speculated
common top byte and up to 2^19 keys, ONE global pass puts the visible keys into the 256 buckets of key bits 16..23, and one workgroup per
bucket finishes it on bits 0..15 -- inside LDS up to CAP keys, chunk by chunk through global memory above, or not at all where the low
bits of an oversize bucket are all equal.

A case = keyword arguments of svgir_harness.scenes.binning_scene on the 8 x 6 grid (rgss, four views on a workload of its own: the
fourth is sorted under the speculated byte) + optionally `narrow`, which moves every surfel along its own view ray -- its pixel stays --
to a view depth inside ONE bucket, [3.0005, 3.015] (fp32 keys 0x4040 0831 .. 0x4040 f5c3), drawn uniformly or from a few `levels` (ties)
-- + what the visible keys must amount to:
  visible   number of visible surfels
  buckets   non-empty buckets (exact, or a (lo, hi) range where the depths are random)
  largest   size of the largest bucket (the same)
  low       "equal" | "differ": the low 16 key bits of the largest bucket
  one_byte  the visible keys share their top byte (False: the workload never speculates; the LSD passes sort it)
tests/test_depth_bucket_scenes.py proves these on the host; tests/test_gpu_depth_buckets.py runs CASES through the HIP binning with the
capacity as built, and FORCED in child processes under SVGIR_DEPTH_BUCKET_CAP=256 / SVGIR_DEPTH_SORT=lsd (scripts/depth_bucket_paths.py)."""
import numpy as np

CAP = 8192            # csrc/depth_sort_plan.hpp DEPTH_BUCKET_CAP
FORCED_CAP = 256      # SVGIR_DEPTH_BUCKET_CAP of the forced-path child process
MAX_P = 1 << 19       # DEPTH_BUCKET_MAX_P
GRID = dict(gx=8, gy=6)
NARROW = (3.0005, 3.015)

CASES, FORCED = {}, {}


def _case(table, name, visible, buckets, largest, low, one_byte=True, narrow=None, **kw):
    assert name not in CASES and name not in FORCED
    table[name] = dict(kw=dict(kw, **GRID), visible=visible, buckets=buckets, largest=largest, low=low, one_byte=one_byte, narrow=narrow, views=4)


# ---- the capacity as built ----
for _P in (1, 63, 64, 65):          # wave edges of the global pass and of the in-LDS passes
    _case(CASES, f"size_P{_P}", _P, (1, 64), (1, _P), "differ" if _P > 1 else "equal", P=_P, edge_frac=0.5, depth="binade", seed=150 + _P)
for _P in (1023, 1024, 1025):       # block edges of the global pass; weights 0, 1 and 2
    _case(CASES, f"size_P{_P}", _P - 300, (48, 64), (2, 64), "differ", P=_P, n_culled=300, edge_frac=0.5, depth="binade", seed=150 + _P)
_case(CASES, "one_visible", 1, 1, 1, "equal", P=1025, n_culled=1024, depth="binade", seed=161)
# whole-grid splats at depth 0.5-0.7 break the common byte: this workload stays on the LSD passes
_case(CASES, "near_breaks_byte", 1017 - 200 + 8, (49, 80), (2, 64), "differ", one_byte=False, P=1017, n_near=8, n_culled=200, edge_frac=0.3,
      depth="binade", seed=162)
for _n, _tag in ((CAP - 1, "cap_minus_1"), (CAP, "cap"), (CAP + 1, "cap_plus_1")):     # one bucket of equal keys around the capacity
    _case(CASES, f"same_{_tag}", _n, 1, _n, "equal", P=_n + 1000, n_culled=1000, edge_frac=0.5, depth="same", seed=163)
_case(CASES, "differ_cap_plus_1", CAP + 1, 1, CAP + 1, "differ", narrow=dict(seed=1), P=CAP + 1 + 900, n_culled=900, edge_frac=0.5, depth="same", seed=164)
_case(CASES, "differ_2cap_plus_1", 2 * CAP + 1, 1, 2 * CAP + 1, "differ", narrow=dict(seed=2), P=2 * CAP + 1 + 900, n_culled=900, edge_frac=0.5,
      depth="same", seed=165)
# five depths only: runs of ~3 400 equal keys, in index order across both chunk boundaries of both passes
_case(CASES, "ties_straddle_chunks", 2 * CAP + 700, 1, 2 * CAP + 700, "differ", narrow=dict(seed=3, levels=5), P=2 * CAP + 700 + 500, n_culled=500,
      edge_frac=0.5, depth="same", seed=166)

# ---- SVGIR_DEPTH_BUCKET_CAP = 256: every path of the bucket kernel with a few hundred keys ----
_case(FORCED, "f_same_cap_minus_1", 255, 1, 255, "equal", P=255 + 150, n_culled=150, edge_frac=0.5, depth="same", seed=170)
_case(FORCED, "f_same_cap", 256, 1, 256, "equal", P=256 + 150, n_culled=150, edge_frac=0.5, depth="same", seed=171)
_case(FORCED, "f_same_cap_plus_1", 257, 1, 257, "equal", P=257 + 150, n_culled=150, edge_frac=0.5, depth="same", seed=172)
_case(FORCED, "f_differ_cap", 256, 1, 256, "differ", narrow=dict(seed=4), P=256 + 150, n_culled=150, edge_frac=0.5, depth="same", seed=173)
_case(FORCED, "f_differ_cap_plus_1", 257, 1, 257, "differ", narrow=dict(seed=5), P=257 + 150, n_culled=150, edge_frac=0.5, depth="same", seed=174)
_case(FORCED, "f_differ_2cap_plus_1", 513, 1, 513, "differ", narrow=dict(seed=6), P=513 + 87, n_culled=87, edge_frac=0.5, depth="same", seed=175)
_case(FORCED, "f_ties_straddle_chunks", 600, 1, 600, "differ", narrow=dict(seed=7, levels=3), P=600 + 100, n_culled=100, edge_frac=0.5, depth="same",
      seed=176)
_case(FORCED, "f_many_small", 1025 - 300, (48, 64), (2, 64), "differ", P=1025, n_culled=300, edge_frac=0.5, depth="binade", seed=177)

# all culled (span 0, R = 0) between full views of a workload that speculates by then
EMPTY_BETWEEN = dict(P=2049, edge_frac=0.5, depth="binade", seed=178, **GRID)
# svgss with backward under the speculated byte: tests/depth_offsets_cases.py SVGSS with depths that share their top byte
SVGSS = dict(P=20000, gx=16, gy=16, edge_frac=0.3, n_culled=2000, depth="binade", seed=179, S=3, VS=8, sh_degree=1, opacity=(0.5, 0.95))


def build(case, variant="rgss"):
    """The case's scene; `narrow` applied."""
    from svgir_harness import scenes
    sc = scenes.binning_scene(variant, **case["kw"])
    if case["narrow"]:
        _narrow(sc, **case["narrow"])
    return sc


def _narrow(sc, seed, levels=None):
    """Every surfel along the ray from the eye through it -- the projection keeps its pixel -- to a view depth in NARROW (culled ones behind
    the camera: to minus that).  The camera looks down the world z axis from BINNING_EYE: view depth = eye_z - z_world in one fp32 rounding."""
    from svgir_harness import scenes
    rng = np.random.default_rng(seed)
    pl = sc["plan"]
    assert pl["n_near"] == 0
    eye = np.array(scenes.BINNING_EYE, dtype=np.float64)
    p = sc["means3D"].astype(np.float64)
    lo, hi = NARROW
    target = rng.uniform(lo, hi, size=len(p)) if levels is None else np.linspace(lo, hi, levels)[rng.integers(0, levels, size=len(p))]
    f = target / np.abs(eye[2] - p[:, 2])
    sc["means3D"] = (eye[None] + (p - eye[None]) * f[:, None]).astype(np.float32)
    pl["depth"] = np.float32(eye[2]) - sc["means3D"][:, 2]


def visible_keys(sc):
    """fp32 depth keys of the visible surfels, whole-grid splats included, by index."""
    pl = sc["plan"]
    vis = np.concatenate([pl["visible"], np.ones(pl["n_near"], dtype=bool)])
    return np.ascontiguousarray(pl["depth"]).view(np.uint32)[vis]


def bucket_facts(sc):
    """What the visible keys amount to: visible, buckets, largest, low ("equal" | "differ" in the largest bucket), one_byte."""
    k = visible_keys(sc)
    cnt = np.bincount((k >> 16) & 255, minlength=256)
    big = k[((k >> 16) & 255) == int(cnt.argmax())]
    return dict(visible=len(k), buckets=int((cnt > 0).sum()), largest=int(cnt.max()),
                low="equal" if len(np.unique(big & 0xffff)) <= 1 else "differ", one_byte=len(np.unique(k >> 24)) == 1)
