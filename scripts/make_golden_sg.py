"""tests/golden/sg_light.npz: the REFERENCE's spherical-Gaussian direct light (scene/direct_light_sg.py) and its own rendering_equation4
(gaussian_renderer/svgss.py:537-631) with that light, on seeded inputs, in fp32 (the reference's precision, suffix `_f32`) and in fp64.

Stored: render_envmap_sg on random directions, compute_envmap at 8 x 16, and per set (`a`: n = 9, Ns = 8, M = 32; `b`: n = 5, Ns = 64,
M = 128) the inputs, every tensor rendering_equation4 returns that the drop-in reproduces, and the autograd gradients of pbr.sum() (`gs_*`)
and of a seeded weighted sum of all returned tensors (`gw_*`) w.r.t. lgtSGs, base_color, roughness and normals.

Runs where the reference is checked out (authoring container), on the CPU.  The reference is imported through make_golden's stubs (its
rasterizer modules build themselves on import and its env-map module fetches a file at import: never import it without them).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402

SETS = {"a": dict(n=9, Ns=8, M=32, seed=41), "b": dict(n=5, Ns=64, M=128, seed=43)}
EXTRA = ("diffuse_light", "specular", "direct", "indirect")
LEAVES = ("lgtSGs", "base", "rough", "normals")


def inputs(n, Ns, M, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    unit = lambda v: v / v.norm(dim=-1, keepdim=True)  # noqa: E731
    geo = unit(rnd(n, 3))
    lobes = rnd(M, 7)
    lobes[:, 3] *= 100.0   # DirectLightSG.__init__
    d = {
        "lgtSGs": lobes,
        "base": torch.sigmoid(rnd(n, 12)) * 0.77 + 0.03, "rough": torch.sigmoid(rnd(n, 4)) * 0.9 + 0.09,
        "normals": unit(geo[:, None] + 0.1 * rnd(n, 4, 3)), "viewdirs": unit(geo + 0.5 * rnd(n, 3)),
        "radiance": (0.2 * rnd(n, Ns, 3)).abs(), "vis": (torch.rand(n, Ns, 1, generator=g, dtype=torch.float64) > 0.3).double(),
        "dirs": unit(geo[:, None] + 0.9 * rnd(n, Ns, 3)), "areas": torch.full((n, Ns, 1), 2 * np.pi, dtype=torch.float64),
    }
    # every second direction of the first rows looks straight into a lobe (|lambda| in the hundreds: the light is ~0 elsewhere)
    k = min(M, Ns)
    d["dirs"][0, :k:2] = unit(lobes[:k:2, :3] + 0.02 * rnd(len(range(0, k, 2)), 3))
    w = {"w_pbr": rnd(n, 12), "w_inc": rnd(n, 3), "w_glob": rnd(n, 3)}
    w.update({"w_" + k_: rnd(n, 12) for k_ in EXTRA})
    # fp32-representable: the fp32 and the fp64 run see the same numbers
    return {k_: v.float().double() for k_, v in {**d, **w}.items()}


def main():
    sys.meta_path.insert(0, mg._Finder())
    sys.path.insert(0, mg.REF)
    import torch.utils.cpp_extension as cpp
    cpp.load = lambda *a, **k: mg._Stub("_C")
    from gaussian_renderer.svgss import rendering_equation4
    from scene.direct_light_sg import compute_envmap, render_envmap_sg

    class SGStandIn:   # DirectLightSG without its .cuda() constructor: direct_light is render_envmap_sg, `transform` ignored
        def __init__(self, lgtSGs):
            self.lgtSGs = lgtSGs

        def direct_light(self, dirs, transform=None):
            return render_envmap_sg(self.lgtSGs, dirs)

    out = {}
    g = torch.Generator().manual_seed(7)
    lobes = torch.randn(32, 7, generator=g, dtype=torch.float64)
    lobes[:, 3] *= 100.0
    lobes = lobes.float().double()
    dirs = torch.randn(257, 3, generator=g, dtype=torch.float64)
    dirs = (dirs / dirs.norm(dim=-1, keepdim=True)).float().double()
    dirs[:32] = (lobes[:, :3] / lobes[:, :3].norm(dim=-1, keepdim=True)).float().double()   # (into the lobes)
    out["eval_lgtSGs"], out["eval_dirs"] = lobes.numpy(), dirs.numpy()
    for dtype, sfx in ((torch.float64, ""), (torch.float32, "_f32")):
        out["eval_light" + sfx] = render_envmap_sg(lobes.to(dtype), dirs.to(dtype)).numpy()
        out["envmap_8x16" + sfx] = compute_envmap(lobes.to(dtype), 8, 16).numpy()

    for tag, cfg in SETS.items():
        d = inputs(**cfg)
        pre = "shade_" + tag + "_"
        for k, v in d.items():
            out[pre + k] = v.numpy()
        for dtype, sfx in ((torch.float64, ""), (torch.float32, "_f32")):
            cv = lambda t: t.to(dtype)  # noqa: E731
            for loss_tag in ("gs", "gw"):
                lv = {k: cv(d[k]).clone().requires_grad_(True) for k in LEAVES}
                pbr, ex = rendering_equation4(lv["base"], lv["rough"], lv["normals"], cv(d["viewdirs"]), cv(d["radiance"]),
                                              SGStandIn(lv["lgtSGs"]), visibility_precompute=cv(d["vis"]),
                                              incident_dirs_precompute=cv(d["dirs"]), incident_areas_precompute=cv(d["areas"]))
                res = {"pbr": pbr, "inc": ex["incident_lights"].mean(-2), "glob": ex["global_incident_lights"].mean(-2)}
                res.update({k: ex[k] for k in EXTRA})
                if loss_tag == "gs":
                    loss = pbr.sum()
                    for k, v in res.items():
                        out[pre + "out_" + k + sfx] = v.detach().numpy()
                    out[pre + "light" + sfx] = render_envmap_sg(cv(d["lgtSGs"]), cv(d["dirs"])).numpy()
                else:
                    loss = sum((res[k] * cv(d["w_" + k])).sum() for k in res)
                gr = torch.autograd.grad(loss, [lv[k] for k in LEAVES])
                for k, gv in zip(LEAVES, gr):
                    assert gv.dtype == dtype and bool(torch.isfinite(gv).all())
                    out[pre + loss_tag + "_" + k + sfx] = gv.numpy()
        L = torch.from_numpy(out[pre + "light"])
        print(pre, "max L = %.4g (no sample near the clamp at 64: %s); fp32 light vs fp64: %.3g relative" %
              (float(L.max()), bool(((L - 64).abs() > 64e-3).all()),
               float((torch.from_numpy(out[pre + "light_f32"]).double() - L).abs().max() / L.abs().max())))
    np.savez_compressed(os.path.join(mg.OUT, "sg_light.npz"), **out)
    print("wrote sg_light.npz", len(out), "arrays")


if __name__ == "__main__":
    main()
