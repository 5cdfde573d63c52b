"""Generates tests/golden/geom_losses.npz: the REFERENCE's own `cos_loss` (utils/loss_utils.py:119-121) and `depth2normal`
(utils/image_utils.py:61-125) run in the authoring container with autograd, in fp64 and in fp32, on four seeded inputs (two at 37 x 29, two at
17 x 33) -- the surface term cos_loss(normal, depth2normal(depth, mask, cam)), the mono-normal term cos_loss(normal, target, weight=mask) --
plus the literal torch lines of the pooled-mask and mask-entropy terms (gaussian_renderer/render.py:157-159, 184-186).  Data only: inputs,
losses, selection counts and fp64 gradients.

    python scripts/make_golden_geom_loss.py
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import make_golden as mg             # noqa: E402
import make_golden_view as mgv       # noqa: E402

INPUTS = ((37, 29, 5), (37, 29, 6), (17, 33, 7), (17, 33, 8))   # H, W, seed


def make_input(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    depth = (3.0 + 0.01 * xx - 0.02 * yy + 0.3 * torch.sin(xx * 0.3) * torch.cos(yy * 0.2) + 0.05 * torch.rand(H, W, generator=g))[None]
    mask = ((yy - 0.5 * H) ** 2 + (xx - 0.45 * W) ** 2 <= (0.45 * min(H, W)) ** 2)[None] & (torch.rand(1, H, W, generator=g) > 0.05)
    noise = 0.05 * torch.randn(3, H, W, generator=g)
    target = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0)
    opacity = torch.rand(1, H, W, generator=g)
    ends = torch.tensor([1e-6, 1 - 1e-6, 0.0, 1.0, 5e-7, 1 - 5e-7], dtype=torch.float32)
    pick = torch.rand(H, W, generator=g) < 0.2
    opacity[0][pick] = ends[torch.randint(0, len(ends), (int(pick.sum()),), generator=g)]
    return depth, mask.float(), noise, target, opacity, (0.47 + 0.01 * seed, 0.55 - 0.01 * seed)


def main():
    mgv.setup_reference()
    import torch.utils.cpp_extension as cpp
    cpp.load = lambda *a, **k: mg._Stub("_C")
    from utils.image_utils import depth2normal
    from utils.loss_utils import cos_loss
    out = {"n_inputs": np.int32(len(INPUTS))}
    for k, (H, W, seed) in enumerate(INPUTS):
        depth, mask, noise, target, opacity, prcp = make_input(H, W, seed)
        cam = types.SimpleNamespace(prcppoint=torch.tensor(prcp), image_width=W, image_height=H, FoVx=0.69, FoVy=0.52)
        normal = torch.nn.functional.normalize(depth2normal(depth, mask, cam) + noise, dim=0)   # the rendered normal: near the pseudo normal
        g = torch.Generator().manual_seed(100 + seed)
        long_ = torch.rand(H, W, generator=g) < 0.15                 # 15 % of the rendered normals are 1.3 long: cos > 1 inside the mask, not selected
        normal = torch.where(long_[None], 1.3 * normal, normal)
        along = torch.rand(H, W, generator=g) < 0.25                 # a quarter of the targets lie along the rendered normal with cos = 1.3
        target = torch.where(along[None], 1.3 * normal / normal.square().sum(0, keepdim=True).clamp_min(1e-12), target)
        target = target * mask
        out.update({f"{k}.depth": depth.numpy(), f"{k}.mask": mask.numpy(), f"{k}.normal": normal.numpy(), f"{k}.target": target.numpy(),
                    f"{k}.opacity": opacity.numpy(), f"{k}.prcppoint": np.asarray(prcp, dtype=np.float32), f"{k}.fovx": np.float64(cam.FoVx),
                    f"{k}.fovy": np.float64(cam.FoVy)})
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            cam_d = types.SimpleNamespace(prcppoint=cam.prcppoint.to(dt), image_width=W, image_height=H, FoVx=cam.FoVx, FoVy=cam.FoVy)
            n, d, o = (t.to(dt).clone().requires_grad_(True) for t in (normal, depth, opacity))
            image_mask = mask.to(dt)
            d2n = depth2normal(d, image_mask, cam_d)
            loss_surface = cos_loss(n, d2n)
            gn, gd = torch.autograd.grad(loss_surface, (n, d))
            loss_mono = cos_loss(n, target.to(dt), weight=image_mask)
            gmono, = torch.autograd.grad(loss_mono, n)
            pool = torch.nn.MaxPool2d(9, stride=1, padding=4)
            loss_mask = (o * (1 - pool(image_mask))).mean()
            gmask, = torch.autograd.grad(loss_mask, o)
            oc = o.clamp(1e-6, 1 - 1e-6)
            loss_mask_entropy = -(image_mask * torch.log(oc) + (1 - image_mask) * torch.log(1 - oc)).mean()
            gent, = torch.autograd.grad(loss_mask_entropy, o)
            with torch.no_grad():
                c_surface = int((torch.sum(n * d2n * 1, 0) < np.cos(0)).sum())
                c_mono = int((torch.sum(n * target.to(dt) * image_mask, 0) < np.cos(0)).sum())
            out.update({f"{k}.{tag}.losses": np.array([float(loss_surface), float(loss_mono), float(loss_mask), float(loss_mask_entropy)], dtype=np.float64),
                        f"{k}.{tag}.counts": np.array([c_surface, c_mono], dtype=np.int64)})
            if dt == torch.float64:
                # (depth2normal builds the pixel grid and the intrinsics in fp32 whatever the depth's dtype: its "fp64" run rounds the
                # camera-space x, y to fp32.  The pseudo normal it returned is recorded, so that cos_loss itself is pinned to fp64 accuracy.)
                out.update({f"{k}.f64.d2n": d2n.detach().numpy(), f"{k}.f64.d_normal_surface": gn.numpy(), f"{k}.f64.d_depth": gd.numpy(), f"{k}.f64.d_normal_mono": gmono.numpy(),
                            f"{k}.f64.d_opacity_mask": gmask.numpy(), f"{k}.f64.d_opacity_entropy": gent.numpy()})
        print(k, H, W, out[f"{k}.f64.losses"], out[f"{k}.f64.counts"], out[f"{k}.f32.counts"])
    path = os.path.join(ROOT, "tests", "golden", "geom_losses.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
