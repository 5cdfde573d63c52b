"""Reference-run fixture for the eval view's environment backdrop (tests/golden/backdrop.npz).  Runs only in the authoring
container, with the machinery of scripts/make_golden_view.py: the REFERENCE's own Python is imported and executed on the CPU
(CUDA device arguments redirected), its CUDA rasterizer replaced by the recording stub; the committed fixture is data (inputs +
the reference's outputs), no reference source.

What is executed, unmodified, from the reference: the whole eval branch of gaussian_renderer/svgss.py `render_view`, i.e. its tail
:255-260 -- `Camera.get_world_directions` (scene/cameras.py:96-108) of a real `scene.cameras.Camera`, the light's `direct_light`
(`DirectLightMap`, scene/direct_light_map.py:70-83; `EnvLight`, scene/envmap.py:54-73, with and without `.transform`) and the three
images `render_env`, `pbr_env`, `env_only` -- on seeded synthetic rasterizer buffers.

Unlike render_view.npz (whose softplus(env) * 2 >= 1 saturates the sRGB clip: its env_only is 1.0 everywhere) the maps here keep the
backdrop inside (0, 1): a DirectLightMap with raw texels in [-6, 0] and an HDR EnvLight map in [0, 2].

    python scripts/make_golden_backdrop.py
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_view as mgv  # noqa: E402

H, W = 40, 56


def _rotation(g):
    Q, _ = np.linalg.qr(torch.randn(3, 3, generator=g).double().numpy())
    if np.linalg.det(Q) < 0:
        Q[:, 0] *= -1
    return Q


def backdrop_fixtures():
    import gaussian_renderer.svgss as ref_svgss
    from scene.cameras import Camera
    from scene.direct_light_map import DirectLightMap
    from scene.envmap import EnvLight
    ref_svgss.GaussianRasterizer = mgv.RecordingRasterizer
    np32 = mgv.np32
    out = {}
    n, Ns = 12, 6
    g = torch.Generator().manual_seed(2607)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    unif = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    geo_n = torch.nn.functional.normalize(rnd(n, 3), dim=-1)
    # (a handful of surfels: the shading in front of the stub rasterizer has to run, its results do not reach the backdrop)
    pc = types.SimpleNamespace(
        get_xyz=0.6 * rnd(n, 3), get_opacity=unif(n, 1), get_scaling=0.02 + 0.05 * unif(n, 3),
        get_rotation=torch.nn.functional.normalize(rnd(n, 4), dim=-1), get_shs=0.3 * rnd(n, 16, 3),
        active_sh_degree=3, max_sh_degree=3, config=[1.0, 1.0, 1.0],
        get_base_color=torch.sigmoid(rnd(n, 12)) * 0.77 + 0.03, get_roughness=torch.sigmoid(rnd(n, 4)) * 0.9 + 0.09,
        get_shading_normal=torch.nn.functional.normalize(geo_n[:, None] + 0.1 * rnd(n, 4, 3), dim=-1),
        get_radiances=(0.2 * rnd(n, Ns, 3)).abs(), _visibility_tracing=(unif(n, Ns, 1) > 0.3).float(),
        _incident_dirs=torch.nn.functional.normalize(geo_n[:, None] + 0.9 * rnd(n, Ns, 3), dim=-1),
        _incident_areas=torch.full((n, Ns, 1), 2 * np.pi))
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, compute_SHs_python=False)
    bg = torch.tensor([1.0, 1.0, 1.0])
    with mgv.cpu_reference():
        cams = {
            # focal lengths from the fields of view, principal point at the image centre (scene/cameras.py:117-123)
            "fov": Camera(colmap_id=0, R=_rotation(g), T=np.array([0.1, -0.2, 3.5]), FoVx=0.69, FoVy=0.52, fx=None, fy=None, cx=None,
                          cy=None, image=None, image_name="x", uid=0, data_device="cpu", height=H, width=W),
            # explicit intrinsics: fx != fy, principal point off-centre (:125-127)
            "pin": Camera(colmap_id=1, R=_rotation(g), T=np.array([-0.3, 0.1, 2.5]), FoVx=0.9, FoVy=0.7, fx=61.5, fy=48.25, cx=19.75,
                          cy=26.5, image=None, image_name="y", uid=1, data_device="cpu", height=H, width=W)}
        for cam in cams.values():
            cam.random_patch = lambda *a, **k: torch.tensor([0.0, 0.0, float(H), float(W)])
            cam.image_mask = torch.ones(1, H, W)
        dlm = DirectLightMap(H=8, light_init=3.0)
        dlm.env = torch.nn.Parameter(-6.0 * unif(1, 8, 16, 3))                    # 2 softplus(.) in (0.005, 1.39), mostly below 1
        el = EnvLight.__new__(EnvLight)
        torch.nn.Module.__init__(el)
        el.envmap = 2.0 * unif(48, 96, 3) ** 2                                     # HDR-like in [0, 2], not 32x64: the resample runs
        el.transform = None
        elt = EnvLight.__new__(EnvLight)
        torch.nn.Module.__init__(elt)
        elt.envmap = el.envmap
        elt.transform = torch.tensor(_rotation(g), dtype=torch.float32)
        out["dlm_env"], out["el_envmap"], out["elt_transform"] = np32(dlm.env), np32(el.envmap), np32(elt.transform)
        for cname, cam in cams.items():
            out[f"{cname}_intrinsics"], out[f"{cname}_c2w"] = np32(cam.intrinsics), np32(cam.c2w)
        opacity = unif(1, H, W)
        opacity[0, 0, :8] = 0.0
        opacity[0, 1, :8] = 1.0
        mgv.RecordingRasterizer.outputs = dict(
            num_rendered=77, image=unif(3, H, W), normal=rnd(3, H, W), opacity=opacity, depth=2.0 + unif(1, H, W),
            feature=unif(7, H, W), vfeature=1.2 * unif(16, H, W), weights=unif(n, 1), radii=(unif(n) * 9).int())
        for k in ("image", "opacity", "vfeature"):
            out["raster_" + k] = np32(mgv.RecordingRasterizer.outputs[k])[:3]      # (the first three vfeature planes: the pbr)
        for cname, lname, light in (("fov", "dlm", dlm), ("pin", "el", el), ("pin", "elt", elt), ("fov", "elt", elt)):
            res = ref_svgss.render_view(cams[cname], pc, pipe, bg, scaling_modifier=1.0, override_color=None, is_training=False,
                                        dict_params={"env_light": light})
            for k in ("env_only", "render_env", "pbr_env"):
                out[f"{cname}_{lname}_{k}"] = np32(res[k])
    np.savez_compressed(os.path.join(mgv.OUT, "backdrop.npz"), **out)
    print("wrote backdrop.npz", len(out), "arrays")


if __name__ == "__main__":
    mgv.setup_reference()
    backdrop_fixtures()
