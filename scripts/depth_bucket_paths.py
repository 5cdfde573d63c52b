"""Child process of tests/test_gpu_depth_buckets.py::test_forced_paths_in_a_child_process: runs the FORCED cases of
tests/depth_bucket_cases.py against the oracle under switches that the library reads once per process --
  cap: SVGIR_DEPTH_BUCKET_CAP=256 (the bucket kernel's oversize paths with a few hundred keys);
  lsd: SVGIR_DEPTH_SORT=lsd (the LSD passes sort every view: the control).
argv[2]: a directory that receives <case>.npz = the fourth view's point_list and ranges.
Prints one line per case and `failed: N`; the exit status is 1 if any case failed."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svg-ir_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import depth_bucket_cases as bk
import test_gpu_depth_buckets as G

which, outdir = sys.argv[1], sys.argv[2]
want = {"cap": dict(SVGIR_DEPTH_BUCKET_CAP=str(bk.FORCED_CAP)), "lsd": dict(SVGIR_DEPTH_SORT="lsd")}[which]
assert all(os.environ.get(k) == v for k, v in want.items()), f"{which} needs {want} in the environment"
table = dict(bk.FORCED) if which == "cap" else dict(bk.CASES, **bk.FORCED)      # (the control sorts every case)
n_bad = 0
for name, case in table.items():
    try:
        raw = G.check_case(case, G.SCOPE0 + 200 + list(table).index(name))
        np.savez(os.path.join(outdir, name + ".npz"), point_list=raw["point_list"], ranges=raw["ranges"])
    except AssertionError as e:
        n_bad += 1
        print("FAIL", name, "::", str(e)[:400], flush=True)
        continue
    print("ok", name, flush=True)
print("cases:", len(table), "failed:", n_bad)
sys.exit(1 if n_bad else 0)
