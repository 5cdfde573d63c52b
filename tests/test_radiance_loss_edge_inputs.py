"""CPU checks of the fused radiance-consistency loss's case table and oracle (tests/radiance_loss_cases.py) and of its new surface: the
lookup is the reference's own (the recorded outputs of DirectLightMap.direct_light / EnvLight.direct_light, tests/golden/lights.npz and
render_view.npz), the selection and the L1 are the reference's literal lines in fp64 torch, the lookup's adjoint is autograd of
F.grid_sample, the whole loss agrees with central differences in env, albedos and ratio, every case holds what it is named for, the two
measured constants cover the table, threshold rows are rare, and the header, `_native.EXPORTS` and the library agree on the new symbols.
No GPU work is launched."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import shading_oracle as so
from tests import radiance_cases as rc
from tests import radiance_loss_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("svgir_radiance_loss_work_bytes", "svgir_radiance_loss_forward", "svgir_radiance_loss_backward")
NAMES = sorted(lc.CASES)


# ---- the oracle is pinned -----------------------------------------------------------------------------------------------------------
def _light_of(env, dirs, softplus, scale, transform=None):
    c = dict(env=np.asarray(env, np.float64).reshape(env.shape[-3:]), ray_d=np.asarray(dirs, np.float64), softplus=softplus, scale=scale,
             transform=transform)
    return lc.light64(c)[0]


def test_lookup_is_the_reference_classes_own():
    g = np.load(os.path.join(GOLD, "lights.npz"))
    np.testing.assert_allclose(_light_of(g["dlm_env"], g["dirs"], True, 2.0), g["dlm_light"], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(_light_of(g["el_resampled"], g["dirs"], False, 1.0), g["el_light"], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(_light_of(g["el_resampled"], g["dirs"], False, 1.0, g["el_transform"]), g["el_light_transformed"], rtol=2e-5,
                               atol=2e-6)
    # and the shading oracle's restatement of the same lines, on every case of the table (fp64 both)
    for name in NAMES:
        c = lc.case(name)
        want = so.env_lookup(torch.from_numpy(c["env"].astype(np.float64)), torch.from_numpy(lc.lookup_dirs(c)), c["softplus"], c["scale"]).numpy()
        got = lc.light64(c)[0]
        fin = np.isfinite(want)
        assert (np.isfinite(got) == fin).all(), name
        np.testing.assert_allclose(got[fin], want[fin], rtol=1e-12, atol=1e-13, err_msg=name)


def test_render_view_fixture_lookup():
    """the incident light the reference's shading recorded is its direct_light * nothing else: pin the lookup on the view fixture's env too"""
    rv = np.load(os.path.join(GOLD, "render_view.npz"))
    dirs, env = rv["pc_incident_dirs"], rv["env"]
    want = so.env_lookup(torch.from_numpy(env.astype(np.float64)), torch.from_numpy(dirs.astype(np.float64)), True, 2.0).numpy()
    np.testing.assert_allclose(_light_of(env, dirs, True, 2.0), want, rtol=1e-12, atol=1e-13)


def _reference_lines(c, dtype=torch.float64, env=None, albedos=None, ratio=None):
    """get_radiance_loss's lines (scene/gaussian_model.py:544-575) with the kernel replaced by the irradiance oracle's rows: returns
    (max_idx, target [N,3])"""
    t = lambda k: torch.from_numpy(np.ascontiguousarray(c[k]).copy()).to(dtype)
    view_dirs = t("xyz") - t("camera_center")
    view_dirs = F.normalize(view_dirs, dim=-1)
    geo_normal = t("geo_normal")
    view_reflect = 2 * torch.sum(geo_normal * view_dirs, dim=-1, keepdim=True) * geo_normal + view_dirs
    n_d_i = torch.sum(t("ray_d") * view_reflect[:, None], dim=-1)
    occlusion = 1 - t("visibility")[..., None]
    n_d_i = n_d_i * occlusion.squeeze(-1)
    max_idx = torch.argmax(n_d_i, dim=-1).unsqueeze(-1).int()
    # (get_radiances; the contract keeps +-inf where torch.nan_to_num's defaults would clamp them to the largest finite number)
    get_radiances = torch.nan_to_num(t("radiances") * t("radiance_ratio"), nan=0.0, posinf=math.inf, neginf=-math.inf)
    sample_indices_expanded = max_idx.unsqueeze(-1).expand(-1, -1, 3)
    return max_idx, get_radiances.gather(1, sample_indices_expanded.long()).squeeze(-2)


@pytest.mark.parametrize("name", NAMES)
def test_selection_target_and_l1_are_the_reference_lines(name):
    c, o = lc.case(name), lc.oracle(name)
    max_idx, target = _reference_lines(c)
    assert np.array_equal(max_idx.reshape(-1).numpy(), o["sel"])
    assert np.array_equal(target.numpy(), o["target"])
    loss = F.l1_loss(torch.from_numpy(np.array(o["out"])), target)
    if o["bad"].any():
        assert not np.isfinite(float(loss)) and np.isnan(o["loss"])
    else:
        assert abs(float(loss) - o["loss"]) <= 1e-14 * max(1.0, abs(o["loss"]))


def test_lookup_adjoint_is_autograd_of_grid_sample():
    for name in ("map_2x4", "map_32x64", "poles_and_seam", "envlight_transform", "softplus_linear"):
        c = lc.case(name)
        env = torch.from_numpy(c["env"].astype(np.float64)).requires_grad_(True)
        d = torch.from_numpy(lc.lookup_dirs(c)).reshape(-1, 3)
        envir_map = (F.softplus(env) if c["softplus"] else env).permute(2, 0, 1)[None]
        phi = torch.arccos(d[:, 2]).reshape(-1) - 1e-6
        theta = torch.atan2(d[:, 1], d[:, 0]).reshape(-1)
        grid = torch.stack((-theta / np.pi, (phi / np.pi) * 2 - 1)).permute(1, 0).unsqueeze(0).unsqueeze(0)
        light = F.grid_sample(envir_map, grid, align_corners=True).squeeze().permute(1, 0).reshape(-1, 3) * c["scale"]
        np.testing.assert_allclose(light.detach().numpy(), lc.light64(c)[0].reshape(-1, 3), rtol=1e-10, atol=1e-12, err_msg=name)
        g = np.random.default_rng(5).normal(size=light.shape)
        light.backward(torch.from_numpy(g))
        np.testing.assert_allclose(lc.lookup_adjoint(c, g) * lc.df_env(c), env.grad.numpy(), rtol=1e-9, atol=1e-12, err_msg=name)


def _loss_of(c, sel):
    return lc.oracle_at(c, sel)["loss"]


def test_whole_loss_against_central_differences():
    """d_env, d_albedos and d_ratio of the oracle against central differences of its own loss under the fixed selection (elements away from
    the L1's kinks: the step is far below every |R - T| gap that is not `unsafe`)"""
    name = "random_9x65"
    c, o = lc.case(name), lc.oracle(name)
    assert not o["unsafe"].any() and o["gap"][o["out_abs"] > 0].min() > 1e-4
    rng = np.random.default_rng(3)
    h = 1e-6
    k = o["kernel"]
    checked = 0
    for key, grad in (("env", o["d_env"]), ("albedos", k["d_albedos"]), ("radiance_ratio", np.asarray(o["d_ratio"]))):
        nz = np.argwhere(grad != 0) if grad.ndim else np.zeros((1, 0), int)
        for pos in nz[rng.permutation(len(nz))[:6]]:
            pos = tuple(pos)
            vals = []
            for s in (+1, -1):
                x = c[key].astype(np.float64).copy()
                x[pos] += s * h
                vals.append(_loss_of(dict(c, **{key: x}), o["sel"]))
            fd = (vals[0] - vals[1]) / (2 * h)
            want = float(grad[pos])
            assert abs(fd - want) <= 1e-6 * max(abs(want), 1e-3), (key, pos, fd, want)
            checked += 1
    assert checked >= 13


# ---- the table holds what it is named for ---------------------------------------------------------------------------------------------
def test_constants_mirror_the_kernel_file():
    src = open(os.path.join(ROOT, "svg-ir_amd", "csrc", "irradiance.hip")).read()
    assert re.search(r"IRR_WAVE = (\d+)", src).group(1) == str(lc.WAVE)
    assert "IRR_WAVES = BLOCK / IRR_WAVE" in src and 256 // lc.WAVE == lc.ROWS
    assert re.search(r"RLB_WAVES = (\d+)", src).group(1) == str(lc.BWD_ROWS)
    assert re.search(r"RL_LDS_BYTES = (\d+) \* 1024", src).group(1) == str(lc.LDS_BYTES // 1024)
    assert "lds + (size_t)a.ntex3 * 8 <= RL_LDS_BYTES" in src and lc.LDS_TEXELS == 6824


def test_sizes_passes_and_maps():
    for S in (63, 64, 65, 129, 300):
        c = lc.case("random_5x%d" % S)
        assert (c["N"], c["S"]) == (5, S) and c["N"] == lc.ROWS + 1
    assert [-(-S // lc.WAVE) for S in (63, 64, 65, 129, 300)] == [1, 1, 2, 3, 5]
    assert lc.case("random_9x65")["N"] == lc.BWD_ROWS + 1 and lc.case("self_hit_1x1")["hit"].tolist() == [[0]]
    shapes = {n: lc.case(n)["env"].shape[:2] for n in NAMES}
    assert shapes["map_1x2"] == (1, 2) and shapes["map_2x4"] == (2, 4) and shapes["map_32x64"] == (32, 64) and shapes["map_128x256"] == (128, 256)
    a, b = shapes["map_lds_last"], shapes["map_lds_first_global"]
    assert a[0] * a[1] == lc.LDS_TEXELS and b[0] * b[1] == lc.LDS_TEXELS + 1      # the last LDS table, the first global one
    assert 32 * 64 <= lc.LDS_TEXELS < 128 * 256
    for n in NAMES:
        c = lc.case(n)
        assert np.abs(c["ray_d"][..., 2]).max() <= 1.0, n                          # every direction has a latitude
        assert c["visibility"].shape == (c["N"], c["S"]) and c["areas"].shape == (c["N"], c["S"])
        if n not in ("all_primaries_miss", "self_hit_1x1"):
            assert len(lc.oracle(n)["kernel"]["rows"]) > 0 and (lc.oracle(n)["d_env"] != 0).any(), n


def test_selection_cases():
    o = lc.oracle("max_positions")
    assert o["sel"][:3].tolist() == [63, 64, 128] and lc.case("max_positions")["S"] == 129
    o, c = lc.oracle("tie_3_70"), lc.case("tie_3_70")
    assert o["sel"][:3].tolist() == [3, 3, 3] and (o["margin"][:3] == 0).all()
    assert (o["score"][:3, 3] == o["score"][:3, 70]).all() and (o["score"][:3, 3] == o["score"][:3].max(1)).all()
    s32 = lc.scores_torch(c, torch.float32).numpy()
    assert (s32[:3, 3] == s32[:3, 70]).all() and (s32[:3].argmax(1) == 3).all()     # a tie in fp32 as well
    o = lc.oracle("all_visible")
    assert (o["score"] == 0).all() and (o["sel"] == 0).all() and np.signbit(o["score"]).any() and not np.signbit(o["score"]).all()
    o = lc.oracle("all_negative")
    assert (o["score"] < 0).all()
    o, c = lc.oracle("at_camera"), lc.case("at_camera")
    assert (c["xyz"][[0, 3]] == c["camera_center"]).all() and (o["score"][[0, 3]] == 0).all() and o["sel"][[0, 3]].tolist() == [0, 0]
    o = lc.oracle("nan_scores")
    assert np.flatnonzero(np.isnan(o["score"][0])).tolist() == [17] and np.flatnonzero(np.isnan(o["score"][1])).tolist() == [40, 100]
    assert o["sel"][:2].tolist() == [17, 40] and np.nanargmax(o["score"][1]) == 5
    c = lc.case("dyadic")
    assert np.array_equal(lc.scores_torch(c, torch.float32).numpy().astype(np.float64), lc.scores_torch(c, torch.float64).numpy())
    assert lc.measure("dyadic")[0] == 0.0


def test_light_cases():
    c = lc.case("poles_and_seam")
    He, We = c["env"].shape[:2]
    for h, z in ((0, 1.0), (1, -1.0)):
        idx, w, ok = lc.taps(c["ray_d"][h, :3], He, We)
        assert (c["hit"][h, :3] == -1).all() and c["ray_d"][h, 0].tolist() == [0.0, 0.0, z]
        if z > 0:
            assert not ok[0, :2].any() and ok[0, 2:].all()                       # the north pole: the taps of row -1 lie outside
        else:
            assert ok[0].all()
        assert ok[1].all() and idx[1, 0] % We == 0                               # theta = +pi: x = 0
        assert idx[2, 0] % We == We - 1 and not ok[2, 1] and not ok[2, 3]         # theta = -pi: the tap at We lies outside
    assert lc.case("envlight")["transform"] is None and not lc.case("envlight")["softplus"] and lc.case("envlight")["scale"] == 1.0
    T = lc.case("envlight_transform")["transform"]
    assert T.shape == (3, 3) and np.allclose(T @ T.T, np.eye(3), atol=1e-6) and not np.allclose(T, np.eye(3))
    assert lc.case("envlight")["env"].shape == (32, 64, 3)
    assert np.ptp(lc.case("flat_map")["env"]) == 0
    e = lc.case("softplus_linear")["env"]
    assert (e[..., 0] > 20).all() and (e[..., 1:] < 20).all()


def test_structure_cases():
    c, o = lc.case("contention"), lc.oracle("contention")
    assert c["N"] == 300 and (o["kernel"]["hits"] == 0).all() and len(o["kernel"]["rows"]) == 299
    assert len(lc.oracle("all_primaries_miss")["kernel"]["rows"]) == 0 and (lc.oracle("all_primaries_miss")["out"] == 0).all()
    c, o = lc.case("hits_out_of_range"), lc.oracle("hits_out_of_range")
    assert [int(c["hit"][i, o["sel"][i]]) for i in range(5)] == [-2, 20, 25, -100, 5] and c["N"] == 20
    assert not np.isin(np.arange(4), o["kernel"]["rows"]).any() and 4 in o["kernel"]["rows"]
    assert set(np.unique(c["hit"][5])) == {-2, -1, 20}
    c, o = lc.case("non_finite"), lc.oracle("non_finite")
    assert np.isnan(c["env"]).sum() == 3 and np.isnan(o["out"][0]).all() and np.isposinf(o["target"][2]).all() and np.isnan(o["loss"])
    assert o["dead"][[0, 2]].all() and (o["bad"].any(1) == o["dead"]).all() and 2 <= o["dead"].sum() < c["N"] // 2
    for k in ("d_env", "d_env_abs"):
        assert np.isfinite(o[k]).all()
    assert np.isfinite(o["kernel"]["d_albedos"]).all() and np.isfinite(o["d_ratio"]) and (o["d_env"] != 0).any()
    with np.errstate(invalid="ignore"):
        g = np.where(o["bad"], 0.0, np.sign(o["out"] - o["target"])) / (3 * c["N"])
    without = rc.oracle_of(lc.kernel_case(c, np.where(o["dead"], -1, o["sel"]), g, clean=True))     # the same with those rows as misses
    for key in ("d_albedos", "d_roughnesses", "d_envmap"):
        assert np.array_equal(without[key], o["kernel"][key]), key
    c, o = lc.case("non_finite_channels"), lc.oracle("non_finite_channels")
    k = o["kernel"]
    assert np.isnan(c["env"]).sum() == 1 and np.isposinf(c["env"]).sum() == 1
    assert o["bad"][0].tolist() == [False, True, False] and np.isnan(o["out"][0, 1])                 # NaN light, green only
    assert o["bad"][2].tolist() == [False, False, True] and not np.isfinite(o["out"][2, 2])           # inf light, blue only
    assert o["bad"][4].tolist() == [True, False, False] and np.isfinite(o["out"][4]).all() and np.isposinf(o["target"][4, 0])
    assert not o["dead"].any() and {0, 2, 4} <= set(k["rows"].tolist()) and np.isnan(o["loss"])
    hit_of = dict(zip(k["rows"].tolist(), k["hits"].tolist()))
    assert (hit_of[0], hit_of[2], hit_of[4]) == (1, 3, 7)
    for key in ("d_albedos", "d_roughnesses", "d_envmap"):
        assert np.isfinite(k[key]).all(), key
    assert np.isfinite(o["d_env"]).all() and np.isfinite(o["d_ratio"])
    # the finite channels of those rows still feed their hit surfels: [channel * 4 + corner]
    alb = k["d_albedos_abs"].reshape(-1, 3, 4)
    only = lambda h: [i for i, hh in hit_of.items() if hh == h]
    for h, ch in ((1, 1), (3, 2), (7, 0)):
        rows = only(h)
        fed = [k3 for k3 in range(3) if not o["bad"][rows, k3].all()]
        assert (alb[h, fed] > 0).all() and all((alb[h, k3] == 0).all() for k3 in range(3) if k3 not in fed), (h, rows)
    assert o["bad"][only(1), 1].all() and o["bad"][only(3), 2].all()       # every row that sums the NaN / inf light is non-finite there
    assert (alb[1, 1] == 0).all() and (alb[3, 2] == 0).all() and (alb[1, [0, 2]] > 0).all() and (alb[3, [0, 1]] > 0).all()
    c, o = lc.case("ratio_zero"), lc.oracle("ratio_zero")
    assert float(c["radiance_ratio"].reshape(-1)[0]) == 0.0 and (o["target"] == 0).all() and o["d_ratio"] != 0
    c = lc.case("physical")
    assert (c["N"], c["S"]) == (2000, 16) and np.allclose(c["areas"], 2 * math.pi)


# ---- the constants of the tolerances ---------------------------------------------------------------------------------------------
def test_the_measured_constants_cover_every_case():
    worst = {"E_SEL": (0.0, None), "E_ENV": (0.0, None)}
    for name in NAMES:
        e_sel, e_env = lc.measure(name)
        print(f"{name:24s} E_SEL {e_sel:.3e}  E_ENV {e_env:.3e}")
        for k, v in (("E_SEL", e_sel), ("E_ENV", e_env)):
            if v > worst[k][0]:
                worst[k] = (v, name)
    for k, stated in (("E_SEL", lc.E_SEL), ("E_ENV", lc.E_ENV)):
        v, name = worst[k]
        print(f"{k} measured {v:.4g} ({name}); stated {stated:.4g}")
        assert v <= stated <= 1.5 * v, (k, name, v)


def test_brdf_terms_stay_within_the_irradiance_tables_e_term():
    """the table's own directions and lights: one fp32 term of every kind deviates from fp64 by no more than radiance_cases.E_TERM, plus
    the two roundings of the upstream g = sign / 3N (fp32(3N) and the quotient: 2^-23), which the irradiance table's fp32 grad_out does not
    have and which is far below the E_ENV the bound adds"""
    for name in NAMES:
        c, o = lc.case(name), lc.oracle(name)
        with np.errstate(invalid="ignore"):
            g = np.where(o["bad"], 0.0, np.sign(o["out"] - o["target"])) / (3 * c["N"])
        dev = rc.term_deviation_of(lc.kernel_case(c, o["sel"], g, clean=True), False)
        for k in ("out", "d_envmap", "d_albedos", "d_roughnesses"):
            assert dev[k] <= rc.E_TERM[k] + 2.0 ** -23, (name, k, dev[k])


def test_threshold_rows_are_rare_and_absent_from_the_selection_cases():
    for name in NAMES:
        o = lc.oracle(name)
        assert o["threshold"].sum() <= 0.01 * len(o["sel"]), name
        if name in lc.SELECTION_CASES:
            assert not o["threshold"].any(), name
        total = o["d_env"].size + o["kernel"]["d_albedos"].size + o["kernel"]["d_roughnesses"].size
        assert o["kernel"]["thr"].sum() <= 0.01 * total, name
        assert o["unsafe"].sum() <= max(1, 0.01 * len(o["sel"])), name


# ---- the surface ----------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_library_agree_on_the_new_symbols(built):
    from gaussian_renderer import _native
    hdr = open(os.path.join(ROOT, "include", "svgir_raster.h")).read()
    lib = C.CDLL(_native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _native.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define SVGIR_ABI_VERSION (\d+)", hdr).group(1) == "14" and _native.ABI_VERSION == 14
    # the ctypes block mirrors the header's struct, field for field
    body = re.search(r"typedef struct svgir_radiance_loss_params \{(.*?)\} svgir_radiance_loss_params;", hdr, re.S).group(1)
    fields = [f.strip().lstrip("*") for decl in body.split(";") if decl.strip() for f in decl.strip().split(" ", 2 if decl.strip().startswith("const") else 1)[-1].split(",")]
    assert fields == [f[0] for f in _native.RadianceLossParams._fields_], fields


def test_argument_checks_come_before_any_hip_call_and_the_work_size_is_consistent(built):
    from gaussian_renderer import _native
    lib = _native.lib
    wb = lib.svgir_radiance_loss_work_bytes
    assert wb(-1, 32, 64) == 0 and wb(5, 0, 64) == 0 and wb(5, 32, 0) == 0 and wb(5, 1 << 14, 1 << 14) == 0
    # table (16 B per texel) + gradient table (12 B per texel, padded to 16) + one double per forward workgroup, 1 024 at least
    for N, He, We in ((0, 1, 2), (5, 32, 64), (200000, 128, 256), (4097, 5, 1365)):
        tex = He * We
        assert wb(N, He, We) == tex * 16 + ((tex * 12 + 15) // 16) * 16 + max(-(-N // lc.ROWS), 1024) * 8, (N, He, We)
    assert wb(6, 32, 64) >= wb(5, 32, 64) and wb(5, 33, 64) > wb(5, 32, 64)
    p = _native.RadianceLossParams()
    buf = (C.c_float * 64)()                       # host memory: never dereferenced, every call below fails its checks first
    host = C.cast(buf, C.c_void_p).value
    fwd = lambda: lib.svgir_radiance_loss_forward(p, host, host, host, host, None)
    bwd = lambda: lib.svgir_radiance_loss_backward(p, host, host, host, host, host, host, host, None)
    p.N, p.S, p.env_h, p.env_w = 0, 4, 32, 64
    assert fwd() == 0 and bwd() == 0               # N = 0 is accepted and launches nothing
    assert lib.svgir_radiance_loss_forward(None, host, host, host, host, None) == -1
    for N, S, He, We in ((-1, 4, 32, 64), (5, 0, 32, 64), (5, 4, 0, 64), (5, 4, 32, 0), (1 << 20, 1 << 12, 32, 64), (0, 4, 1 << 14, 1 << 14)):
        p.N, p.S, p.env_h, p.env_w = N, S, He, We
        assert fwd() == -1 and bwd() == -1, (N, S, He, We)
    p.N, p.S, p.env_h, p.env_w = 5, 4, 32, 64      # N > 0 without its pointers
    assert fwd() == -1 and bwd() == -1


def test_python_surface(built):
    import inspect
    from pbgi.renderer import Renderer
    from svgir_harness import losses
    sig = inspect.signature(losses.fused_radiance_loss)
    assert list(sig.parameters) == ["renderer", "xyz", "camera_center", "geo_normal", "incident_dirs", "incident_areas", "visibility", "light",
                                    "normals12", "albedos", "roughnesses", "radiances", "radiance_ratio", "with_rows"]
    assert sig.parameters["with_rows"].default is False and hasattr(Renderer, "radiance_consistency")
    z = torch.zeros(2, 3, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r = Renderer()
        r.hemi_index_buffers, r.uv_buffers = torch.zeros(2, 3, 1, dtype=torch.int32), torch.zeros(2, 3, 2)
        r.radiance_consistency(torch.zeros(2, 3), torch.zeros(3), torch.zeros(2, 3), z, torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(4, 8, 3),
                               True, 2.0, None, torch.zeros(2, 12), torch.zeros(2, 12), torch.zeros(2, 4), z, torch.ones(()))
