"""The case table of the ROWS of the depth sort's bucket plan (csrc/depth_sort_plan.hpp DepthRows): under that plan every preprocess
workgroup leaves its row of K = DEPTH_ROW consecutive surfels grouped by key bits 16..23 (csrc/preprocess.hip), and the workgroup of a
bucket gathers its keys row by row (csrc/binning.hip depth_bucket_sort_kernel).  tests/depth_bucket_cases.py covers the buckets -- sizes
around the capacity, the oversize paths; this table covers what is new with the rows: their edges, empty rows, rows of one digit next to
rows of many, ties across and inside rows, the last surfel of the last row, the largest number of rows, and oversize buckets that are
gathered from several rows.

A case = keyword arguments of svgir_harness.scenes.binning_scene on the 8 x 6 grid (rgss, every surfel visible and inside the binade
[2.5, 3.5): one top byte), four views on a workload of its own -- the fourth is sorted under the speculated byte -- + `shape`, a function
of (index array, rng) that returns which surfels stay visible and their view depths (None: as the scene has them); the others go behind
the camera.  Every surfel moves along its own view ray: its pixel, and so its tiles, stay.  `facts` names what the case must amount to;
tests/test_depth_gather_scenes.py proves it on the host, tests/test_gpu_depth_gather.py runs CASES with the capacity as built and FORCED
in a child process under SVGIR_DEPTH_BUCKET_CAP=256 (scripts/depth_gather_paths.py), both against the oracle and the LSD passes."""
import numpy as np

K = 1024              # csrc/depth_sort_plan.hpp DEPTH_ROW
MAX_P = 1 << 19       # DEPTH_BUCKET_MAX_P
FORCED_CAP = 256      # SVGIR_DEPTH_BUCKET_CAP of the forced-path child process
GRID = dict(gx=8, gy=6)
NARROW = (3.0005, 3.015)     # fp32 keys 0x4040 0831 .. 0x4040 f5c3: one value of bits 16..23
BINADE = (2.5, 3.5)          # 0x4020 0000 .. 0x405f ffff: 64 values of them

CASES, FORCED = {}, {}


def _case(table, name, shape=None, views=4, **facts_and_kw):
    facts = {k: facts_and_kw.pop(k) for k in list(facts_and_kw) if k in ("visible", "rows", "last_row", "empty_rows", "one_digit_rows", "spread_rows",
                                                                        "ties", "largest", "low", "largest_rows")}
    assert name not in CASES and name not in FORCED
    table[name] = dict(kw=dict(facts_and_kw, depth="binade", **GRID), shape=shape, facts=facts, views=views)


# ---- row edges: a partial last row, a full one, a last row of one surfel, two rows and one surfel ----
def _thirds(idx, rng):
    return (idx % 3) != 1, None


for _P in (K - 1, K, K + 1, 2 * K + 1):
    _case(CASES, f"rows_P{_P}", _thirds, P=_P, edge_frac=0.5, seed=300 + _P % 7, rows=(_P + K - 1) // K, last_row=_P - (_P - 1) // K * K,
          visible=_P - (_P + 1) // 3)


# ---- a row without a visible key between two rows that have some ----
def _middle_row_empty(idx, rng):
    return ((idx // K) != 1) & ((idx % 4) != 2), None


_case(CASES, "empty_row_between", _middle_row_empty, P=3 * K, edge_frac=0.5, seed=311, rows=3, empty_rows=[1], visible=2 * K - 2 * K // 4)


# ---- a row whose visible keys all carry one digit, next to rows that spread over >= 48 ----
def _middle_row_one_digit(idx, rng):
    d = rng.uniform(*BINADE, size=len(idx))
    mid = (idx // K) == 1
    d[mid] = rng.uniform(*NARROW, size=int(mid.sum()))
    return (idx % 5) != 3, d


_case(CASES, "one_digit_row", _middle_row_one_digit, P=3 * K, edge_frac=0.5, seed=312, rows=3, one_digit_rows=[1], spread_rows=[0, 2],
      visible=3 * K - (3 * K + 1) // 5)


# ---- ties: seven depths only -- every key in both rows and many times inside each, ending up in index order ----
def _seven_levels(idx, rng):
    return (idx % 6) != 0, np.linspace(2.6, 3.4, 7)[rng.integers(0, 7, size=len(idx))]


_case(CASES, "ties_across_rows", _seven_levels, P=2 * K + 100, edge_frac=0.5, seed=313, rows=3, ties=7, visible=2 * K + 100 - (2 * K + 100 + 5) // 6)


# ---- the only visible surfel is the last index of the last row ----
def _last_only(idx, rng):
    return idx == idx[-1], None


_case(CASES, "last_surfel_only", _last_only, P=2 * K + 7, edge_frac=0.0, seed=314, rows=3, last_row=7, visible=1)

# ---- the most rows the plan can see: P = 2^19, a quarter visible in every row (the row prefix at its largest) ----
_case(CASES, "max_rows", lambda idx, rng: ((idx % 4) == 1, None), P=MAX_P, edge_frac=0.25, seed=315, rows=MAX_P // K, visible=MAX_P // 4)


# ---- SVGIR_DEPTH_BUCKET_CAP = 256: one oversize bucket gathered from four rows ----
def _sparse_narrow(idx, rng):
    return (idx % 8) == 5, rng.uniform(*NARROW, size=len(idx))


def _sparse_same(idx, rng):
    return (idx % 8) == 5, np.full(len(idx), 3.0078125)


_case(FORCED, "f_oversize_differ_4_rows", _sparse_narrow, P=3 * K + 100, edge_frac=0.5, seed=320, rows=4, visible=(3 * K + 100 + 2) // 8, largest=(3 * K + 100 + 2) // 8,
      low="differ", largest_rows=4)
_case(FORCED, "f_oversize_equal_4_rows", _sparse_same, P=3 * K + 100, edge_frac=0.5, seed=321, rows=4, visible=(3 * K + 100 + 2) // 8, largest=(3 * K + 100 + 2) // 8,
      low="equal", largest_rows=4)
# (in LDS under the lowered capacity: the same rows, every 16th surfel)
_case(FORCED, "f_in_lds_4_rows", lambda idx, rng: ((idx % 16) == 5, rng.uniform(*NARROW, size=len(idx))), P=3 * K + 100, edge_frac=0.5, seed=322, rows=4,
      visible=(3 * K + 100 + 10) // 16, largest=(3 * K + 100 + 10) // 16, low="differ", largest_rows=4)

# svgss with the fused shading under the speculated byte: a few hundred culled surfels whose rows the shading must clear -- it finds them
# at the back of the depth order, which the bucket kernel assembles from the rows' tails
SVGSS = dict(P=2000, n_culled=300, edge_frac=0.3, depth="binade", seed=330, S=4, VS=52, sh_degree=1, opacity=(0.5, 0.95), **GRID)


def build(case, variant="rgss"):
    """The case's scene; `shape` applied."""
    from svgir_harness import scenes
    sc = scenes.binning_scene(variant, **case["kw"])
    if case["shape"]:
        P = sc["means3D"].shape[0]
        vis, depth = case["shape"](np.arange(P), np.random.default_rng(case["kw"]["seed"] + 1000))
        _move(sc, np.asarray(vis, dtype=bool), depth)
    return sc


def _move(sc, visible, depth):
    """Every surfel along the ray from the eye through it -- the projection keeps its pixel -- to view depth `depth` (None: its own), the
    ones that are not `visible` to minus that: behind the camera.  The camera looks down the world z axis from BINNING_EYE: view depth =
    eye_z - z_world in one fp32 rounding, so equal targets give bit-identical keys."""
    from svgir_harness import scenes
    pl = sc["plan"]
    assert pl["n_near"] == 0 and pl["visible"].all()
    eye = np.array(scenes.BINNING_EYE, dtype=np.float64)
    p = sc["means3D"].astype(np.float64)
    own = eye[2] - p[:, 2]
    target = own if depth is None else np.asarray(depth, dtype=np.float64)
    f = np.where(visible, target, -target) / own
    sc["means3D"] = (eye[None] + (p - eye[None]) * f[:, None]).astype(np.float32)
    pl["depth"] = np.float32(eye[2]) - sc["means3D"][:, 2]
    pl["visible"] = visible.copy()
    pl["R"] = int(visible.sum() + (pl["tile2"][visible] >= 0).sum())


def row_facts(sc):
    """What the rows of the scene amount to, from the fp32 view depths of sc["plan"]."""
    pl = sc["plan"]
    vis = pl["visible"]
    key = np.ascontiguousarray(pl["depth"]).view(np.uint32)
    P = len(vis)
    rows = (P + K - 1) // K
    row = np.arange(P) // K
    digit = (key >> 16) & 255
    per_row = [np.unique(digit[vis & (row == b)]) for b in range(rows)]
    vk, vr = key[vis], row[vis]
    cnt = np.bincount(digit[vis], minlength=256)
    big = int(cnt.argmax())
    in_big = vis & (digit == big)
    # ties: keys that occur in two different rows AND at least twice inside one row (counted where the scene has few distinct keys)
    tied = 0
    for k in (np.unique(vk) if len(np.unique(vk)) <= 64 else ()):
        r = vr[vk == k]
        if len(np.unique(r)) >= 2 and np.bincount(r).max() >= 2:
            tied += 1
    return dict(visible=int(vis.sum()), rows=rows, last_row=P - (rows - 1) * K, empty_rows=[b for b in range(rows) if len(per_row[b]) == 0],
                digits_per_row=[len(d) for d in per_row], ties=tied, distinct_keys=len(np.unique(vk)), one_byte=len(np.unique(vk >> 24)) == 1,
                largest=int(cnt.max()), low="equal" if len(np.unique(key[in_big] & 0xffff)) <= 1 else "differ",
                largest_rows=len(np.unique(row[in_big])))
