"""tests/golden/sg_paths.npz: the REFERENCE's spherical-Gaussian light (scene/direct_light_sg.py) on the three paths around the shading --
its gradient, the eval view's backdrop and the light of the radiance-consistency loss -- on seeded inputs, in fp64 and in fp32 (`_f32`).

  (i)   `grad_*`: autograd through render_envmap_sg w.r.t. lgtSGs [32,7] and viewdirs [257,3] under a recorded upstream `grad_up`
        (the gradient of sum(L * up)); a quarter of the directions look into a lobe, |lambda| in the hundreds.
  (ii)  `view_*`: the three images of gaussian_renderer/svgss.py:256-260 on a 17 x 13 view: Camera.get_world_directions
        (scene/cameras.py:96-108, called on a stand-in that carries intrinsics / c2w in the run's precision), the light's direct_light
        = render_envmap_sg along them, and the reference's rgb_to_srgb in the three compositions; the pbr plane is the rasterizer's
        vfeature / opacity.clamp_min(1e-5) (:188-189).  The lobes are wide (|lambda| ~ 8) and dim so that the backdrop is neither black nor all clipped.
  (iii) `block_*`: direct_light(dirs) * areas for a 9 x 8 block of samples, the `envmap` of GaussianModel.get_radiance_loss
        (scene/gaussian_model.py:560).

Runs where the reference is checked out (authoring container), on the CPU, through make_golden_view's stubs and device redirection.
The file holds data only.
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_view as mgv  # noqa: E402

H, W = 13, 17


def _f32(t):
    return t.float().double()


def main():
    mgv.setup_reference()
    from scene.cameras import Camera
    from scene.direct_light_sg import render_envmap_sg
    from utils.graphics_utils import rgb_to_srgb
    out = {}
    g = torch.Generator().manual_seed(77)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    unit = lambda v: v / v.norm(dim=-1, keepdim=True)  # noqa: E731
    DT = ((torch.float64, ""), (torch.float32, "_f32"))

    # (i) the gradient of the bare light
    lobes = rnd(32, 7)
    lobes[:, 3] *= 100.0   # DirectLightSG.__init__
    lobes[::2, 3] *= 0.2
    dirs = unit(rnd(257, 3))
    dirs[:64] = unit(lobes[torch.arange(64) % 32, :3] / lobes[torch.arange(64) % 32, :3].norm(dim=-1, keepdim=True) + 0.05 * rnd(64, 3))
    lobes, dirs, up = _f32(lobes), _f32(dirs), _f32(rnd(257, 3))
    out["grad_lgtSGs"], out["grad_dirs"], out["grad_up"] = lobes.numpy(), dirs.numpy(), up.numpy()
    with mgv.cpu_reference():
        for dt, sfx in DT:
            lb, dr = lobes.to(dt).requires_grad_(True), dirs.to(dt).requires_grad_(True)
            L = render_envmap_sg(lb, dr)
            gl, gd = torch.autograd.grad((L * up.to(dt)).sum(), [lb, dr])
            out["grad_light" + sfx], out["grad_d_lgtSGs" + sfx], out["grad_d_dirs" + sfx] = L.detach().numpy(), gl.numpy(), gd.numpy()

        # (ii) the eval view's backdrop
        vl = rnd(32, 7)
        vl[:, 3] *= 8.0
        vl[:, 4:] *= 0.1
        vl = _f32(vl)
        Q, _ = np.linalg.qr(rnd(3, 3).numpy())
        if np.linalg.det(Q) < 0:
            Q[:, 0] *= -1
        c2w = np.eye(4)
        c2w[:3, :3] = Q
        K = np.array([[21.5, 0, 6.25], [0, 17.75, 8.5], [0, 0, 1]])
        c2w, K = _f32(torch.from_numpy(c2w)), _f32(torch.from_numpy(K))
        image, opacity, vfeature = (_f32(torch.rand(*s, generator=g, dtype=torch.float64)) for s in ((3, H, W), (1, H, W), (3, H, W)))
        opacity[0, 0, :4] = 0.0
        opacity[0, 1, :4] = 1.0
        out.update(view_lgtSGs=vl.numpy(), view_intrinsics=K.numpy(), view_c2w=c2w.numpy(), view_image=image.numpy(),
                   view_opacity=opacity.numpy(), view_vfeature=vfeature.numpy())
        for dt, sfx in DT:
            cam = types.SimpleNamespace(image_height=H, image_width=W, intrinsics=K.to(dt), c2w=c2w.to(dt))
            directions = Camera.get_world_directions(cam)
            light = types.SimpleNamespace(direct_light=lambda d, transform=None: render_envmap_sg(vl.to(dt), d))
            rendered_image, rendered_opacity = image.to(dt), opacity.to(dt)
            pbr = vfeature.to(dt) / rendered_opacity.clamp_min(1e-5)                                        # svgss.py:189
            direct_env = light.direct_light(directions.permute(1, 2, 0)).permute(2, 0, 1)                   # svgss.py:256-260
            out["view_render_env" + sfx] = (rendered_image + (1 - rendered_opacity) * rgb_to_srgb(direct_env)).numpy()
            out["view_pbr_env" + sfx] = rgb_to_srgb(pbr * rendered_opacity + (1 - rendered_opacity) * direct_env).numpy()
            out["view_env_only" + sfx] = rgb_to_srgb(direct_env).numpy()
            out["view_directions" + sfx] = directions.numpy()

        # (iii) the light of a block of the radiance-consistency loss
        bl = rnd(5, 7)
        bl[:, 3] *= 20.0
        bl, bd = _f32(bl), _f32(unit(rnd(9, 8, 3)))
        areas = _f32(torch.rand(9, 8, 1, generator=g, dtype=torch.float64) * 0.2 + 0.7)
        out.update(block_lgtSGs=bl.numpy(), block_dirs=bd.numpy(), block_areas=areas.numpy())
        for dt, sfx in DT:
            out["block_envmap" + sfx] = (render_envmap_sg(bl.to(dt), bd.to(dt)) * areas.to(dt)).numpy()
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    path = os.path.join(mgv.OUT, "sg_paths.npz")
    np.savez_compressed(path, **out)
    print("wrote sg_paths.npz", len(out), "arrays,", os.path.getsize(path), "bytes; env_only range %.3g .. %.3g" %
          (out["view_env_only"].min(), out["view_env_only"].max()))


if __name__ == "__main__":
    main()
