"""The case table of the depth-offsets tests: the last pass of the geometry depth sort (csrc/binning.hip, the weighted radix pass) also
sums the surfels' tile counts, and the instance offsets, the instance count R and the visible span come out of it.  The depth cases
of tests/binning_cases.py all weigh 1 (R = P); these mix the weights 0 (culled, interleaved by index), 1, 2 (`edge_frac`: a surfel on
a tile's right edge) and T (`n_near`: a splat whose rectangle is the whole grid) across the places where that pass changes behaviour:
1024 keys per block, 32 blocks per group, 64 keys per wave, 2^20 keys (16 keys per thread above).

A case = keyword arguments of svgir_harness.scenes.binning_scene on the 8 x 6 grid (T = 48), rgss, + what it must amount to:
  keys     surfels, whole-grid splats included (the depth sort's key count)
  R        instances = the sum of the weights
  views    forwards on one workload (four: the fourth view sorts in three passes where the visible keys share their top byte)
tests/test_depth_offsets_scenes.py proves these on the host; tests/test_gpu_depth_offsets.py runs them through the HIP binning."""
M = 1 << 20
GRID = dict(gx=8, gy=6)
T = GRID["gx"] * GRID["gy"]

CASES = {}


def _case(name, keys, R, views=1, **kw):
    assert name not in CASES
    CASES[name] = dict(kw=dict(kw, **GRID), keys=keys, R=R, views=views)


_case("block_edge_below", 1023, 1027, P=1023, n_culled=300, edge_frac=0.5, depth="binade", seed=41)
_case("block_edge_above", 1025, 1041, P=1025, n_culled=300, edge_frac=0.5, depth="binade", seed=42)
_case("group_edge", 32769, 34250, views=4, P=32769, n_culled=9000, edge_frac=0.5, depth="binade", seed=43)
_case("heavy_small", 1025, 1414, P=1017, n_near=8, n_culled=200, edge_frac=0.3, depth="spread", seed=44)
_case("heavy_group_edge", 32769, 35412, views=4, P=32761, n_near=8, n_culled=5000, edge_frac=0.3, depth="spread", seed=45)
_case("ties", 2049, 1958, P=2049, n_culled=700, edge_frac=0.5, depth="same", seed=46)
_case("one_visible", 1025, 1, P=1025, n_culled=1024, depth="binade", seed=47)
for _P in (1, 63, 64, 65):      # (R: whatever the plan says -- the sizes are the point)
    _case(f"wave_edge_P{_P}", _P, None, P=_P, edge_frac=0.5, depth="binade", seed=50 + _P)
# the only large case: 16 keys per thread
_case("large", M + 1, 819466, views=4, P=M + 1 - 8, n_near=8, n_culled=400000, edge_frac=0.3, depth="binade", seed=48)

# all culled (R = 0) between two non-empty views of one workload
EMPTY_BETWEEN = dict(P=2049, edge_frac=0.5, depth="binade", seed=49, **GRID)
# svgss with backward: the order_svgss_* recipe of tests/binning_cases.py, with weights 0 and 2
SVGSS = dict(P=20000, gx=16, gy=16, edge_frac=0.3, n_culled=2000, seed=46, S=3, VS=8, sh_degree=1, opacity=(0.5, 0.95))
# three views whose visible keys share their top byte, then one of the same size whose keys do not
BROKEN_SPECULATION = (dict(P=1025, n_culled=300, edge_frac=0.5, depth="binade", seed=42, **GRID),
                      dict(P=1025, n_culled=300, edge_frac=0.5, depth="spread", seed=42, **GRID))


def weights(sc):
    """Tile count of every surfel that sc["plan"] implies: 0 culled, 1, 2 on a right edge (not in the last column), T whole-grid."""
    import numpy as np
    pl = sc["plan"]
    w = np.where(pl["visible"], 1 + (pl["tile2"] >= 0), 0)
    return np.concatenate([w, np.full(pl["n_near"], pl["T"])]).astype(np.int64)


def top_bytes(sc):
    """The distinct top bytes of the visible depth keys (1: the three-pass depth sort from the fourth view on)."""
    import numpy as np
    pl = sc["plan"]
    vis = np.concatenate([pl["visible"], np.ones(pl["n_near"], dtype=bool)])
    return np.unique(np.ascontiguousarray(pl["depth"]).view(np.uint32)[vis] >> 24)
