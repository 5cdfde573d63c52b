"""Generates tests/golden/activations.npz by running the REFERENCE's own `GaussianModel` getters (scene/gaussian_model.py:270-355:
get_scaling, get_rotation, get_opacity, get_geo_normal, get_shading_normal, get_base_color, get_albedo, get_roughness) and torch's
autograd on a GaussianModel created with __new__ and filled with seeded tensors, on the CPU, in the authoring container
(make_golden_view.setup_reference / cpu_reference, as make_golden_densify.py does).  The two lines that are not getters -- `viewdirs =
F.normalize(camera_center - means3D, dim=-1)` (gaussian_renderer/svgss.py:109) and `F.mse_loss(_normal, zeros)` (:316) -- sit inside
render_view and are evaluated here on the same tensors.

Two scenes of P <= 64: the edge rows of tests/activation_cases.py (`edge_rows`) followed by seeded ordinary rows, once with the model's
default base_color_scale of ones and once with (1, 0.5, 2) and without the NaN-offset row (a finite normal_reg).  The fixture is data only: the raw inputs, the camera centre, the upstream
gradients, every output, and the raw gradients autograd returns (NaN where torch gives NaN).

    python scripts/make_golden_activations.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden as mg             # noqa: E402
import make_golden_view as mgv       # noqa: E402
import activation_cases as ac        # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
ATTR = {"xyz": "_xyz", "scaling": "_scaling", "rotation": "_rotation", "opacity": "_opacity", "normal": "_normal",
        "base_color": "_base_color", "roughness": "_roughness"}
P_TOTAL = 64


def main(fname="activations.npz"):
    mgv.setup_reference()
    import torch.utils.cpp_extension as cpp
    cpp.load = lambda *a, **k: mg._Stub("_C")
    from scene.gaussian_model import GaussianModel
    out = {}
    for tag, scale in (("ones", None), ("scaled", (1.0, 0.5, 2.0))):
        er, labels = ac.edge_rows(nan_offset=scale is None)     # (the scaled scene keeps normal_reg finite)
        E = labels.shape[0]
        assert E <= P_TOTAL
        g = torch.Generator().manual_seed(31337 if scale is None else 31338)
        rnd = ac._random_rows(P_TOTAL - E, g)
        raw = {k: torch.cat([er[k], rnd[k]]) for k in ac.RAW}
        campos = torch.tensor(ac.CAMPOS)
        with mgv.cpu_reference():
            gm = GaussianModel.__new__(GaussianModel)
            gm.use_pbr = True
            gm.vertex_num = 4
            gm.setup_functions()
            gm.base_color_scale = torch.ones(3) if scale is None else torch.tensor(scale)
            for k in ac.RAW:
                setattr(gm, ATTR[k], torch.nn.Parameter(raw[k].clone().requires_grad_(True)))
            res = {"scales": gm.get_scaling, "rotations": gm.get_rotation, "opacities": gm.get_opacity, "geo_normal": gm.get_geo_normal,
                   "shading_normal": gm.get_shading_normal, "base_color": gm.get_base_color, "albedo": gm.get_albedo,
                   "roughness": gm.get_roughness,
                   "viewdirs": torch.nn.functional.normalize(campos - gm.get_xyz, dim=-1),
                   "normal_reg": torch.nn.functional.mse_loss(gm._normal, torch.zeros_like(gm._normal))}
            assert torch.equal(torch.nan_to_num(res["albedo"], nan=7.0), torch.nan_to_num(res["base_color"], nan=7.0))
            del res["albedo"]
            up = {k: torch.randn(v.shape, generator=g) for k, v in res.items() if k != "normal_reg"}
            g_reg = 0.1
            loss = sum((res[k] * up[k]).sum() for k in up) + g_reg * res["normal_reg"]
            loss.backward()
            for k in ac.RAW:
                out[f"{tag}/raw_{k}"] = raw[k].numpy()
                out[f"{tag}/grad_{k}"] = getattr(gm, ATTR[k]).grad.numpy().copy()
            for k, v in res.items():
                out[f"{tag}/out_{k}"] = v.detach().numpy().copy()
            for k, v in up.items():
                out[f"{tag}/up_{k}"] = v.numpy()
            out[f"{tag}/labels"] = np.concatenate([labels, np.array(["ordinary"] * (P_TOTAL - E))])
            out[f"{tag}/g_reg"] = np.array(g_reg)
            out[f"{tag}/campos"] = campos.numpy()
            out[f"{tag}/base_color_scale"] = gm.base_color_scale.numpy().copy()
        nn = {k: int(np.isnan(out[f"{tag}/grad_{k}"]).sum()) for k in ac.RAW}
        print(tag, "P", P_TOTAL, "NaN gradient elements:", nn)
    np.savez_compressed(os.path.join(OUT, fname), **out)
    print("wrote", fname, os.path.getsize(os.path.join(OUT, fname)), "bytes")


if __name__ == "__main__":
    main()
