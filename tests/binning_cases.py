"""The case matrix of the binning tests: one table for tests/test_binning_scenes.py (the CPU oracle against the numpy construction, and
the proof that every case sits on the threshold it is named for) and tests/test_gpu_binning.py / scripts/binning_paths.py (the HIP
binning against the oracle).  A case = keyword arguments of svgir_harness.scenes.binning_scene + what the case must amount to:

  P        surfels (the depth sort's key count; the offsets kernels' input size), whole-grid splats included
  R        instances (the tile sort's key count); None: whatever the plan says (surfels on a tile's right edge count twice, except in
           the last column) -- the case then does not sit on a threshold of R
  T        tiles; `bits` = bits of the tile id, `passes` = radix passes of the tile sort when the single 12-bit counting pass is not used
  top      number of distinct top bytes among the visible depth keys (1: the three-pass depth sort from the fourth view on)
  visible  surfels that survive the cull (the span of the depth order that the emit walks, 64 per wave)

The thresholds (csrc/binning.hip, csrc/common.hpp tile_sort_plan, csrc/api.hip):
  depth sort / two-pass tile sort: 4 keys per thread up to 2^20 keys, 16 above; cursor rows per 1024 (4096) keys, group totals per
      32 768 (131 072) keys.  For the tile sort the launch is sized by the CAPACITY: exact on a workload's first view, R + R/8 + 1024
      rounded up to 4096 on later ones
  single-pass tile sort (T <= 4096): bins = T rounded up to 256, 2048 keys per workgroup, column scan in 16 row segments with an 8-way
      unrolled body (more than 16 * 8 rows: R > 262 144)
  offsets scan: 2048 surfels per block, more than 256 blocks from P > 524 288
  emit: one wave per 64 surfels of the visible span; rectangle width in 12 bits (1023 tiles)
  sub-tile order: counts in registers up to 4 T = 12 288 (T = 3072); per-XCD lists: eighths of the prefix at 4 T = 1024 / 8192
No list of any case is longer than 2^20 / 8 = 131 072 (csrc/common.hpp SEG_K_BITS: a consumed sub-tile list ends at 2^20 candidates).
"""
M = 1 << 20
GRID = dict(gx=8, gy=6)      # the small grid of the depth-sort cases: T = 48, 6 bits
MAX_LIST = M // 8

CASES = {}


def _bits(T):
    b = 1
    while (1 << b) < T:
        b += 1
    return b


def _case(name, expect, variant="rgss", views=1, backward=False, **kw):
    T = kw.get("gx", 8) * kw.get("gy", 6)
    expect = dict(expect)
    expect.setdefault("T", T)
    expect.setdefault("bits", _bits(T))
    expect.setdefault("visible", kw["P"] - kw.get("n_culled", 0))
    expect.setdefault("P", kw["P"] + kw.get("n_near", 0))
    if variant == "svgss":
        kw.update(S=3, VS=8, sh_degree=1, opacity=(0.5, 0.95))    # opaque enough for the gradients to carry signal
    assert name not in CASES
    CASES[name] = dict(variant=variant, views=views, backward=backward, kw=kw, expect=expect)


# ---- depth sort size: rgss, S = 0, the 8 x 6 grid; R = P.  From P = 32 767 on: four views of one workload ----
for _P in (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 32767, 32768, 32769):
    _v = 4 if _P >= 32767 else 1
    _case(f"depth_P{_P}_one_same", dict(R=_P, top=1), P=_P, layout="one", depth="same", seed=_P, views=_v, **GRID)
    _case(f"depth_P{_P}_uniform_same", dict(R=_P, top=1), P=_P, layout="uniform", depth="same", seed=_P + 1, views=_v, **GRID)
    _case(f"depth_P{_P}_uniform_spread", dict(R=_P, top=3 if _P >= 63 else 1), P=_P, layout="uniform", depth="spread", seed=_P + 2, views=_v, **GRID)
# (the eight-tile layout keeps every list at or below 2^20 / 8: the visible surfels are dealt to the tiles in equal shares, and eight
# of the P are culled -- the depth sort still sorts all P keys)
for _P, _n in ((M - 1, "2p20m1"), (M, "2p20"), (M + 1, "2p20p1")):
    for _d, _top in (("spread", 3), ("binade", 1), ("same", 1)):
        _case(f"depth_P{_n}_uniform_{_d}", dict(R=_P, top=_top), P=_P, layout="uniform", depth=_d, seed=7, views=4, **GRID)
        _case(f"depth_P{_n}_eight_{_d}", dict(R=_P - 8, top=_top), P=_P, layout="eight", depth=_d, n_culled=8, seed=8, views=4, **GRID)

# ---- visible span of the depth order on a wave boundary (the culled surfels interleaved by index) ----
for _vis in (63, 64, 65):
    _case(f"emit_visible{_vis}", dict(R=_vis, top=3), P=_vis + 64, n_culled=64, seed=_vis, **GRID)
_case("emit_culled_third", dict(R=None, top=3), P=5000, n_culled=1500, edge_frac=0.1, seed=5, **GRID)

# ---- tile sort plan: grid sizes at the plan's thresholds, R at the counting sort's and the radix sort's ----
_case("tiles_T1", dict(R=3000, top=3, bits=1, passes=1), P=3000, gx=1, gy=1, seed=11)
_case("tiles_T255_wide_R2047", dict(R=2047, top=3, bits=8, passes=1), P=2047, gx=255, gy=1, seed=12)
_case("tiles_T256_tall_R2048", dict(R=2048, top=3, bits=8, passes=1), P=2048, gx=1, gy=256, seed=13)
_case("tiles_T257_wide_R2049", dict(R=2049, top=3, bits=9, passes=2), P=2049, gx=257, gy=1, seed=14)
_case("tiles_T3072_edges", dict(R=None, top=3, bits=12, passes=2), P=20000, gx=64, gy=48, edge_frac=0.1, seed=15)
_case("tiles_T3074_skewed", dict(R=20000, top=3, bits=12, passes=2), P=20000, gx=58, gy=53, layout="skewed", seed=16)
_case("tiles_T4095_edges", dict(R=None, top=3, bits=12, passes=2), P=20000, gx=65, gy=63, edge_frac=0.1, seed=17)
_case("tiles_T4096_R300000", dict(R=300000, top=3, bits=12, passes=2), P=300000, gx=64, gy=64, seed=18, views=4)
_case("tiles_T4097_R2p20m1", dict(R=M - 1, top=3, bits=13, passes=2), P=M - 1, gx=17, gy=241, seed=19, views=4)
_case("tiles_T4097_R2p20p1", dict(R=M + 1, top=1, bits=13, passes=2), P=M + 1, gx=17, gy=241, depth="binade", seed=20, views=4)
# 14 bits; R < 2^20 <= R + R/8 + 1024: the first view sorts 4 keys per thread, the later ones 16 with the count read on the device
_case("tiles_T10000_R940000", dict(R=940000, top=3, bits=14, passes=2), P=940000, gx=100, gy=100, seed=21, views=4)
# 16 bits, the widest accepted grid; three near splats whose rectangle is the whole grid (width 1023: all 10 bits of the packed width)
_case("tiles_T33759_whole_grid_splats", dict(R=None, top=3, bits=16, passes=2), P=20000, gx=1023, gy=33, edge_frac=0.1,
      n_near=3, seed=22)

# ---- sub-tile order and gradient-row prefixes: svgss S = 3, VS = 8 with backward ----
for _gx, _gy in ((64, 48), (58, 53), (16, 16), (257, 1), (64, 32), (683, 3)):
    _T = _gx * _gy
    _case(f"order_svgss_T{_T}", dict(R=20000, top=3), variant="svgss", backward=True, P=20000, gx=_gx, gy=_gy, seed=30 + _gx)

# what the forced-path child processes run (scripts/binning_paths.py)
FORCED = {
    # SVGIR_TILE_SORT12=0: the radix passes at 1 ... 12 tile bits (one pass up to 8 bits, two from 9)
    "radix": [n for n, c in CASES.items() if n.startswith("tiles_") and c["expect"]["T"] <= 4096] + ["depth_P2049_uniform_spread", "emit_culled_third"],
    # SVGIR_FWD_FILL=1 SVGIR_FWD_XCD=1: one dispatch list per XCD, 4 T = 1024 / 1028 / 8192 / 8196 / 12 296
    "xcd": ["order_svgss_T256", "order_svgss_T257", "order_svgss_T2048", "order_svgss_T2049", "order_svgss_T3074"],
}
