"""Runs the value tests of tests/test_gpu_composite_edges.py on the GPU and writes the measured worst ratios per case and kernel --
error / bound of the axis pixel's colour, of dL_dcolors and of dL_dopacity, the list position of the worst candidate, and the fp32
reference's own E32 / E32c -- to profiles/composite_edges.json.  A ratio above 1 is a failing test; the record keeps it.
usage: python scripts/composite_edges_profile.py [out.json]"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = {"svgss_S3_VS8": "render_fwd.hip / render_bwd.hip", "rgss_S5": "render_fwd.hip / render_bwd_plain.hip",
          "rgss_S0": "render_fwd.hip / render_bwd_plain.hip", "svgss_S0_VS0": "render_fwd.hip / render_bwd_plain.hip",
          "svgss_S9_VS72": "render_generic.hip", "rgss_S7": "render_generic.hip"}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "composite_edges.json")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    rc = pytest.main([os.path.join(ROOT, "tests", "test_gpu_composite_edges.py"), "-q", "-m", "gpu", "-p", "no:cacheprovider",
                      "-k", "axis_colour or per_candidate"])
    import test_gpu_composite_edges as T
    rec = {"source": "tests/test_gpu_composite_edges.py (value tests)", "eps32": 2.0 ** -24, "pytest_exit": int(rc),
           "cases": [dict(case=c, width=w, kernels=KERNEL[w], **{k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
                     for (c, w), r in sorted(T.RATIOS.items())]}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"{len(rec['cases'])} records -> {out}")


if __name__ == "__main__":
    main()
