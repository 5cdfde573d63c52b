"""The case matrix of the tile-sort tests on the single-pass plan (csrc/binning.hip launch_tile_sort12: the kernels are launched for an
instance CAPACITY and bound their work by the count they read on the device -- a key block past ceil(count / 4096) writes no histogram
row, the column scan walks the written rows only, a scatter block past the count returns; the sorted tile ids are not stored).  One table
for tests/test_tile_bin_scenes.py (the CPU proof that every case has the property it is named for) and tests/test_gpu_tile_bin.py (the HIP
binning against the oracle).  A case = keyword arguments of svgir_harness.scenes.binning_scene + what it must amount to (as in
tests/binning_cases.py):

  R        instances; None: whatever the plan says (surfels on a tile's right edge count twice)
  T        tiles (all <= 4096: the single-pass plan)
  visible  surfels that survive the cull (the span of the depth order that the emit walks, 64 per wave)
"""
KEYS = 4096          # csrc/binning.hip TS12K: instance positions per key block (a workgroup of 512 threads; 2048 in the 256-thread build)

CASES = {}


def _case(name, expect, variant="rgss", backward=False, **kw):
    T = kw.get("gx", 8) * kw.get("gy", 6)
    expect = dict(expect)
    expect.setdefault("T", T)
    expect.setdefault("visible", kw["P"] - kw.get("n_culled", 0) + kw.get("n_near", 0))
    if variant == "svgss":
        kw.update(S=3, VS=8, sh_degree=1, opacity=(0.5, 0.95))
    assert name not in CASES and T <= 4096
    CASES[name] = dict(variant=variant, backward=backward, kw=kw, expect=expect)


# ---- R on a block boundary (of 2048 and of 4096 keys): uniform layout, no edge surfels, R = P ----
for _R in (2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193):
    _case(f"block_R{_R}", dict(R=_R), P=_R, gx=20, gy=13, seed=100 + _R % 97)

# ---- a surfel whose two instances lie on either side of a block boundary (the seed was moved until one does) ----
_case("run_straddles_boundary", dict(R=None, straddle=True), P=3000, edge_frac=0.5, seed=1, gx=8, gy=6)

# ---- one surfel longer than a block: the whole-grid splats (depth 0.5 .. 0.7) sort in front of the rest (one binade, 2.5 .. 3.5), so the
# first instances belong to them alone: three runs of 3072 (two boundaries of runs inside the first three blocks), and one run that is
# exactly block 0 ----
_case("run_longer_than_block_T3072", dict(R=2000 + 3 * 3072, long_runs=3), P=2000, gx=64, gy=48, n_near=3, depth="binade", seed=41)
_case("run_longer_than_block_T4096_span2", dict(R=4097, whole_blocks=1, visible=2), P=1, gx=64, gy=64, n_near=1, depth="binade", seed=42)

# ---- short visible spans (the culled surfels interleaved by index) ----
for _vis in (1, 63, 64, 65, 255, 256, 257):
    _case(f"visible{_vis}", dict(R=_vis), P=_vis + 64, n_culled=64, seed=200 + _vis, gx=8, gy=6)

# ---- the largest single-pass grid, a fifth of the surfels on tile edges; one tile ----
_case("tiles_T4096_edges_R70000", dict(R=None, R_about=70000), P=58400, gx=64, gy=64, edge_frac=0.2, seed=51)
_case("tiles_T1", dict(R=5000), P=5000, gx=1, gy=1, seed=52)

# ---- svgss with backward: a wrong first-instance record puts gradient rows on the wrong surfels ----
_case("svgss_T3072_backward", dict(R=20000), variant="svgss", backward=True, P=20000, gx=64, gy=48, seed=61)

# the capacity re-run (tests/test_gpu_tile_bin.py): equal surfel counts, the second view's instance count beyond the capacity guessed from the first
RERUN = (dict(P=3003, gx=64, gy=48, seed=71), dict(P=3000, gx=64, gy=48, n_near=3, seed=72))
