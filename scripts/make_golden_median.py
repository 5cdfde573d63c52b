"""Reference-run fixture for the exact median's two consumers (tests/golden/median.npz).  Runs only in the authoring container, with the
machinery of scripts/make_golden_view.py: the REFERENCE's own Python is imported and executed on the CPU; the committed fixture is data
(the reference's results on inputs that tests/median_cases.py rebuilds from its seeds), no reference source.

What is executed, unmodified, from the reference: `srgb_to_rgb` (utils/graphics_utils.py:218-229), on a ladder around its knee and inside
the albedo lines.  eval_relighting_tensoIR.py:227-237 and gaussian_renderer/render.py:218-219 stand inside a script's main loop and inside
`calculate_loss`, so they are restated literally (median_cases.albedo_lines around the reference's own srgb_to_rgb, with the
`.median(dim=0).values` of :237 taken here; median_cases.loss_lines), in fp32 and in fp64; the loss gradient is torch autograd's through
those lines in fp64, upstream median_cases.UPSTREAM.

    python scripts/make_golden_median.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_view as mgv  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "svg-ir_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import median_cases as mc  # noqa: E402  (before the reference's packages go on the path: it imports this project's gaussian_renderer)


def median_fixtures():
    from utils.graphics_utils import srgb_to_rgb
    out = {}
    lad = torch.from_numpy(np.resize(mc.knee_ladder(), 3 * 2 * 6).reshape(3, 2, 6))
    out["knee_ladder_32"] = srgb_to_rgb(lad).numpy()
    out["knee_ladder_64"] = srgb_to_rgb(lad.double()).numpy()
    for cid in mc.GOLDEN_ALBEDO:
        case = next(c for c in mc.ALBEDO_CASES if c["id"] == cid)
        r, g = mc.build_albedo(case)
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            q, m = mc.albedo_lines(torch.from_numpy(r.copy()).to(dt), torch.from_numpy(g.copy()).to(dt), case["srgb"], srgb_to_rgb)
            out[f"albedo.{cid}.scale{tag}"] = q.median(dim=0).values.numpy()
            out[f"albedo.{cid}.count{tag}"] = np.int64(int(m.sum()))
    for cid in mc.GOLDEN_LOSS:
        case = next(c for c in mc.LOSS_CASES if c["id"] == cid)
        x = mc.build_loss(case)
        with torch.no_grad():
            out[f"loss.{cid}.loss32"] = mc.loss_lines(torch.from_numpy(x.copy())).numpy()
        x64 = torch.from_numpy(x.copy()).double().requires_grad_(True)
        loss = mc.loss_lines(x64)
        (loss * mc.UPSTREAM).backward()
        out[f"loss.{cid}.loss64"] = loss.detach().numpy()
        out[f"loss.{cid}.grad64"] = x64.grad.numpy()
    np.savez_compressed(os.path.join(mgv.OUT, "median.npz"), **out)
    print("wrote median.npz", len(out), "arrays")


if __name__ == "__main__":
    mgv.setup_reference()
    median_fixtures()
