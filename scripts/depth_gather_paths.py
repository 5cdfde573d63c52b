"""Child process of tests/test_gpu_depth_gather.py: runs cases of tests/depth_gather_cases.py against the oracle under switches that the
library reads once per process --
  cap: SVGIR_DEPTH_BUCKET_CAP=256 (the FORCED cases: oversize buckets gathered from several rows);
  lsd: SVGIR_DEPTH_SORT=lsd (the LSD passes sort every view of every case: the control).
argv[2]: a directory that receives <case>.npz = the fourth view's point_list and ranges.
Prints one line per case and `failed: N`; the exit status is 1 if any case failed."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svg-ir_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import depth_gather_cases as gc
import test_gpu_depth_gather as T

which, outdir = sys.argv[1], sys.argv[2]
want = {"cap": dict(SVGIR_DEPTH_BUCKET_CAP=str(gc.FORCED_CAP)), "lsd": dict(SVGIR_DEPTH_SORT="lsd")}[which]
assert all(os.environ.get(k) == v for k, v in want.items()), f"{which} needs {want} in the environment"
table = dict(gc.FORCED) if which == "cap" else dict(gc.CASES, **gc.FORCED)      # (the control sorts every case)
n_bad = 0
for name, case in table.items():
    try:
        raw = T.check_case(case, T.SCOPE0 + 200 + list(table).index(name))
        np.savez(os.path.join(outdir, name + ".npz"), point_list=raw["point_list"], ranges=raw["ranges"])
    except AssertionError as e:
        n_bad += 1
        print("FAIL", name, "::", str(e)[:400], flush=True)
        continue
    print("ok", name, flush=True)
print("cases:", len(table), "failed:", n_bad)
sys.exit(1 if n_bad else 0)
