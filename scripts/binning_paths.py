"""Child process of tests/test_gpu_binning.py::test_forced_paths_in_a_child_process: runs the cases of tests/binning_cases.py FORCED[which]
against the oracle under switches that the library reads once per process --
  radix: SVGIR_TILE_SORT12=0 (the two-kernel radix passes sort the tiles of grids the single counting pass would take);
  xcd:   SVGIR_FWD_FILL=1 SVGIR_FWD_XCD=1 (one longest-first dispatch list per XCD), svgss forward + backward.
Prints one line per case and `failed: N`; the exit status is 1 if any case failed."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svg-ir_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import binning_cases as bc
import test_gpu_binning as G

which = sys.argv[1]
want = {"radix": dict(SVGIR_TILE_SORT12="0"), "xcd": dict(SVGIR_FWD_FILL="1", SVGIR_FWD_XCD="1")}[which]
assert all(os.environ.get(k) == v for k, v in want.items()), f"{which} needs {want} in the environment"
n_bad = 0
for name in bc.FORCED[which]:
    try:
        G.check_case(name)
    except AssertionError as e:
        n_bad += 1
        print("FAIL", name, "::", str(e)[:400], flush=True)
        continue
    print("ok", name, flush=True)
print("cases:", len(bc.FORCED[which]), "failed:", n_bad)
sys.exit(1 if n_bad else 0)
