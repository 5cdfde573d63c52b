"""Reference-run fixture for the eval view's tail (tests/golden/view_metrics.npz).  Runs only in the authoring container, with the
machinery of scripts/make_golden_view.py: the REFERENCE's own Python is imported and executed on the CPU; the committed fixture is data
(the reference's results on inputs that tests/metrics_cases.py rebuilds from its seeds), no reference source.

What is executed, unmodified, from the reference: `mse` and `psnr` (utils/image_utils.py:32-37), `ssim` (utils/loss_utils.py:33-64) and
`rgb_to_srgb` (utils/graphics_utils.py:198-215), in fp32 and in fp64, on the composed operands of metrics_cases.GOLDEN_CASES; and the
albedo-scale lines of eval_relighting_tensoIR.py:285-294 -- they stand inside that script's main loop, so they are restated literally
(metrics_cases.albedo_lines) around the reference's own rgb_to_srgb -- on metrics_cases.GOLDEN_ALBEDO.

    python scripts/make_golden_metrics.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_view as mgv  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def metrics_fixtures():
    import metrics_cases as mc
    from utils.graphics_utils import rgb_to_srgb
    from utils.image_utils import mse, psnr
    from utils.loss_utils import ssim
    out = {}
    lad = torch.from_numpy(np.resize(mc.srgb_ladder(), 3 * 4 * 4).reshape(3, 4, 4))
    out["srgb_ladder_32"] = rgb_to_srgb(lad).numpy()
    out["srgb_ladder_64"] = rgb_to_srgb(lad.double()).numpy()
    with torch.no_grad():
        for cid in mc.GOLDEN_CASES:
            oa, ob = mc.build(mc.BY_ID[cid])
            for tag, dt in (("32", torch.float32), ("64", torch.float64)):
                # the operands as torch holds them (fp32 planes); the reference's sRGB in the dtype of the evaluation
                a, b = (mc.compose(o, with_srgb=False).to(dt) for o in (oa, ob))
                a, b = (rgb_to_srgb(x) if o["srgb"] else x for x, o in ((a, oa), (b, ob)))
                out[f"{cid}.mse{tag}"] = mse(a, b).numpy()
                out[f"{cid}.psnr{tag}"] = psnr(a, b).numpy()
                out[f"{cid}.ssim{tag}"] = ssim(a, b).numpy()
        for cid in mc.GOLDEN_ALBEDO:
            case = next(c for c in mc.ALBEDO_CASES if c["id"] == cid)
            r, g = mc.build_albedo(case)
            for tag, dt in (("32", torch.float32), ("64", torch.float64)):
                s, m = mc.albedo_lines(torch.from_numpy(r).to(dt), torch.from_numpy(g).to(dt), case["srgb"], rgb_to_srgb)
                out[f"albedo.{cid}.scale{tag}"] = s.numpy()
                out[f"albedo.{cid}.count{tag}"] = np.int64(int(m.sum()))
    np.savez_compressed(os.path.join(mgv.OUT, "view_metrics.npz"), **out)
    print("wrote view_metrics.npz", len(out), "arrays")


if __name__ == "__main__":
    mgv.setup_reference()
    metrics_fixtures()
