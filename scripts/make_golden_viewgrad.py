"""tests/golden/shading_viewgrad.npz: the view-direction gradient of the REFERENCE's own rendering_equation4 (gaussian_renderer/svgss.py:
537-631) on the inputs already stored in tests/golden/shading.npz (sets a, b, c), under the same loss and upstream weights as
make_golden.shading_fixtures(), with `viewdirs` a leaf -- in fp64 (`shade_{a,b,c}_g_viewdirs`) and in fp32 (`shade_{a,b,c}_f32_g_viewdirs`).

Only the new arrays are written; shading.npz is read, never rewritten.  The reference is imported through make_golden's stubs (its
rasterizer modules build themselves on import and its env-map module fetches a file at import: never import it without them).
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402


class EnvStandIn:
    """The light of make_golden.shading_fixtures(): softplus + F.grid_sample at the lat-long coordinates, x2."""

    def __init__(self, env):
        self.env = env

    def direct_light(self, dirs):
        shape = dirs.shape
        dirs = dirs.reshape(-1, 3)
        envir_map = F.softplus(self.env).permute(0, 3, 1, 2)
        phi = torch.arccos(dirs[:, 2]).reshape(-1) - 1e-6
        theta = torch.atan2(dirs[:, 1], dirs[:, 0]).reshape(-1)
        grid = torch.stack((-theta / np.pi, (phi / np.pi) * 2 - 1)).permute(1, 0).unsqueeze(0).unsqueeze(0)
        light_rgbs = F.grid_sample(envir_map, grid, align_corners=True).squeeze().permute(1, 0).reshape(-1, 3)
        return light_rgbs.reshape(*shape) * 2.0


def main():
    sys.meta_path.insert(0, mg._Finder())
    sys.path.insert(0, mg.REF)
    import torch.utils.cpp_extension as cpp
    cpp.load = lambda *a, **k: mg._Stub("_C")
    from gaussian_renderer.svgss import rendering_equation4

    gold = np.load(os.path.join(mg.OUT, "shading.npz"))
    out = {}
    for tag in ("a", "b", "c"):
        pre = "shade_" + tag + "_"
        d = {k[len(pre):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(pre) and "_f32_" not in k}
        for dtype, key in ((torch.float64, "g_viewdirs"), (torch.float32, "f32_g_viewdirs")):
            cv = lambda t: t.to(dtype)  # noqa: E731
            viewdirs = cv(d["viewdirs"]).clone().requires_grad_(True)
            pbr, ex = rendering_equation4(cv(d["base"]), cv(d["rough"]), cv(d["normals"]), viewdirs, cv(d["radiance"]),
                                          EnvStandIn(cv(d["env"])), visibility_precompute=cv(d["vis"]),
                                          incident_dirs_precompute=cv(d["dirs"]), incident_areas_precompute=cv(d["areas"]))
            loss = (pbr * cv(d["w_pbr"])).sum() + sum((ex[k] * cv(d["w_" + k])).sum() for k in ("diffuse_light", "specular", "direct", "indirect")) \
                + (ex["incident_lights"].mean(-2) * cv(d["w_inc"])).sum() + (ex["global_incident_lights"].mean(-2) * cv(d["w_glob"])).sum()
            (g,) = torch.autograd.grad(loss, [viewdirs])
            assert g.dtype == dtype and bool(torch.isfinite(g).all())
            out[pre + key] = g.numpy()
            print(pre + key, tuple(g.shape), "max |g| = %.4g" % float(g.abs().max()))
    np.savez_compressed(os.path.join(mg.OUT, "shading_viewgrad.npz"), **out)
    print("wrote shading_viewgrad.npz", len(out), "arrays")


if __name__ == "__main__":
    main()
