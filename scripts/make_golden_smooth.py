"""Generates tests/golden/smooth_losses.npz: the REFERENCE's own `first_order_edge_aware_loss`, `second_order_edge_aware_loss` and `tv_loss`
(utils/loss_utils.py:101-117) run in the authoring container with autograd, in fp64 and in fp32, on a handful of the cases of
tests/smooth_cases.py.  The reference takes its image derivative from kornia, which is not installed here: `kornia.filters` is stubbed and
the stub's `spatial_gradient` is THIS script's statement of the contract (normalized Sobel kernels built as outer products, replicate
padding, (x, y) / (xx, xy, yy) order; the xy plane it returns is NaN, so a composition that touched it would show).  What the fixture pins is
therefore the composition by the reference's own lines -- broadcasting, `[:, [0, 2]]`, `.sum(1).mean()`, the factor 10, and `tv_loss`
entirely --, not kornia's kernels.  Data only: losses and gradients; the inputs are rebuilt from the seeded builders.

A masked term is recorded the way the reference calls it (svgss.py:368): on the fp32 products data * mask and img * mask, with the gradients
w.r.t. those products.

    python scripts/make_golden_smooth.py
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_view as mgv       # noqa: E402
import smooth_cases as sc            # noqa: E402

RECORDED = ("sizes-1x7", "sizes-5x5", "sizes-9x33", "four-7x31", "shared-9x33", "light-9x33", "stage2-21x70", "envmap-16x32")


def spatial_gradient(input, mode="sobel", order=1, normalized=True):
    """[B,C,H,W] -> [B,C,2,H,W] (order 1: x, y) or [B,C,3,H,W] (order 2: xx, xy, yy with xy = NaN)."""
    assert mode == "sobel" and normalized and order in (1, 2)
    if order == 1:
        smooth, deriv, norm = [1.0, 2.0, 1.0], [-1.0, 0.0, 1.0], 8.0
    else:
        smooth, deriv, norm = [1.0, 4.0, 6.0, 4.0, 1.0], [-1.0, 0.0, 2.0, 0.0, -1.0], 64.0
    kx = torch.tensor(np.outer(smooth, deriv) / norm, dtype=input.dtype)
    B, C, H, W = input.shape
    padded = F.pad(input.reshape(B * C, 1, H, W), (order, order, order, order), mode="replicate")
    dx = F.conv2d(padded, kx[None, None]).reshape(B, C, H, W)
    dy = F.conv2d(padded, kx.t()[None, None]).reshape(B, C, H, W)
    if order == 1:
        return torch.stack([dx, dy], dim=2)
    return torch.stack([dx, torch.full_like(dx, float("nan")), dy], dim=2)


def main():
    mgv.setup_reference()
    filters = types.ModuleType("kornia.filters")
    filters.spatial_gradient = spatial_gradient
    filters.laplacian = None
    sys.modules["kornia.filters"] = filters
    from utils import loss_utils as lu
    fns = {"first": lu.first_order_edge_aware_loss, "second": lu.second_order_edge_aware_loss}
    out = {"recorded": np.array(RECORDED)}
    cases = {c["id"]: c for c in sc.CASES}
    for cid in RECORDED:
        for k, term in enumerate(sc.build(cases[cid])):
            prod = lambda a, m: a if m is None else a * m   # noqa: E731   (fp32, one rounding)
            D = prod(term["data"], term["data_mask"])
            I = None if term["img"] is None else prod(term["img"], term["img_mask"])   # noqa: E741
            for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
                d = torch.from_numpy(D).to(dt).requires_grad_(True)
                if term["kind"] == "tv":
                    loss = lu.tv_loss(d)
                    grads = torch.autograd.grad(loss, d)
                else:
                    i = torch.from_numpy(I).to(dt).requires_grad_(True)
                    loss = fns[term["kind"]](d, i)
                    grads = torch.autograd.grad(loss, (d, i))
                out[f"{cid}.{k}.{tag}.loss"] = np.float64(loss.detach())
                if dt == torch.float64:
                    out[f"{cid}.{k}.f64.d_data"] = grads[0].numpy()
                    if len(grads) > 1:
                        out[f"{cid}.{k}.f64.d_img"] = grads[1].numpy()
            print(cid, k, term["kind"], float(out[f"{cid}.{k}.f64.loss"]), float(out[f"{cid}.{k}.f32.loss"]))
    path = os.path.join(ROOT, "tests", "golden", "smooth_losses.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
