"""CPU suite of the spherical-Gaussian light's three paths around the shading (tests/sg_paths_cases.py): the oracles are pinned by the
reference's own recordings (tests/golden/sg_paths.npz, scripts/make_golden_sg_paths.py), the closed-form direction gradient is checked
against autograd and central differences, every case is proven to hold what it is named for, what fp32 loses is measured and printed
(E32 / G32 per case, E_SG over the table), the exclusion cap of the loss's cases is asserted on the oracle alone, and the new entry points'
argument checks -- all made before any HIP call -- are exercised without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import backdrop_cases as bc
import sg_light_cases as sg
import sg_paths_cases as sp
import shading_cases as sc
from tests import radiance_loss_cases as lc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sg_paths.npz")
T = torch.from_numpy


# ---- the oracles against the reference's recordings -----------------------------------------------------------------------------
def test_gradient_oracles_match_the_reference_autograd():
    g = np.load(GOLD)
    lobes, dirs, up = T(g["grad_lgtSGs"]), T(g["grad_dirs"]), T(g["grad_up"])
    assert lobes.shape == (32, 7) and dirs.shape == (257, 3)
    np.testing.assert_allclose(sg.sg_light(lobes, dirs).numpy(), g["grad_light"], rtol=1e-12, atol=1e-300)
    d_lobes, d_dirs = sp.eval_oracle(lobes, dirs, up)
    for got, key in ((d_lobes, "grad_d_lgtSGs"), (d_dirs, "grad_d_dirs")):
        e = sc.row_err(got, T(g[key]))
        assert float(e.max()) < 1e-11, (key, float(e.max()))
        # the reference's own fp32 run loses what the fp32 restatement loses, within a factor
        ref32 = float(sc.row_err(T(g[key + "_f32"]), T(g[key])).max())
        own32 = float(sc.row_err(sp.eval_oracle(lobes, dirs, up, torch.float32)[key != "grad_d_lgtSGs"], T(g[key])).max())
        print(f"{key}: fp32 reference {ref32:.2e}, fp32 restatement {own32:.2e}")
        assert own32 <= 4 * ref32 + 1e-6 and ref32 <= 4 * own32 + 1e-6
    assert float(T(g["grad_d_lgtSGs"]).abs().max()) > 0 and float(T(g["grad_d_dirs"]).abs().max()) > 0


def test_backdrop_oracle_matches_the_reference_view():
    g = np.load(GOLD)
    H, W = g["view_image"].shape[-2:]
    assert (H, W) == (13, 17)
    case = dict(name="fixture", H=H, W=W, K=g["view_intrinsics"].astype(np.float32), R=g["view_c2w"][:3, :3].astype(np.float32), T=None,
                lobes=g["view_lgtSGs"], image=g["view_image"].astype(np.float32), opacity=g["view_opacity"].astype(np.float32),
                vfeature=g["view_vfeature"].astype(np.float32))
    np.testing.assert_allclose(bc.directions64(case).transpose(2, 0, 1), g["view_directions"], rtol=0, atol=1e-14)
    o64, r32 = sp.view_oracle64(case), sp.view_reference32(case)
    for k in bc.OUTPUTS:
        np.testing.assert_allclose(o64[k], g["view_" + k], rtol=0, atol=1e-12, err_msg=k)
        np.testing.assert_allclose(r32[k], g["view_" + k + "_f32"], rtol=0, atol=4e-6, err_msg=k)
    e = g["view_env_only"]
    assert ((e > 0) & (e < 1)).all() and e.max() - e.min() > 0.05       # (neither black nor clipped)


def test_loss_light_matches_the_reference_block():
    g = np.load(GOLD)
    env = sg.sg_light(T(g["block_lgtSGs"]), T(g["block_dirs"])) * T(g["block_areas"])
    assert env.shape == (9, 8, 3)
    np.testing.assert_allclose(env.numpy(), g["block_envmap"], rtol=1e-12, atol=1e-300)
    c = dict(lobes=g["block_lgtSGs"].astype(np.float32), ray_d=g["block_dirs"].astype(np.float32))
    np.testing.assert_allclose(sp.rl_light64(c)[0] * g["block_areas"], g["block_envmap"], rtol=1e-12, atol=1e-300)


# ---- A ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", ["n63-M5", "signs-and-zeros", "unnormalised-dirs"])
def test_direction_gradient_against_autograd_and_central_differences(id):
    lobes, dirs, up = sp.eval_build(id)
    d = dirs.clone().requires_grad_(True)
    lb = lobes.clone().requires_grad_(True)
    (sg.sg_light(lb, d) * up).sum().backward()
    closed_l, closed_d = sp.eval_oracle(lobes, dirs, up)
    assert float(sc.row_err(closed_d, d.grad).max()) < 1e-11 and float(sc.row_err(closed_l, lb.grad).max()) < 1e-11
    h = 1e-6
    f = lambda x: (sg.sg_light(lobes, x) * up).sum(-1)  # noqa: E731
    for j in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[j] = h
        fd = (f(dirs + e) - f(dirs - e)) / (2 * h)
        scale = float(closed_d.abs().max())
        assert float((fd - closed_d[:, j]).abs().max()) <= 1e-5 * scale + 1e-9, (id, j)


def test_eval_cases_hold_what_they_are_named_for():
    ns, Ms = {c["n"] for c in sp.EVAL_CASES}, {c["M"] for c in sp.EVAL_CASES}
    assert {1, 63, 64, 65, 257, 1200} <= ns and {1, 5, 32, 33, 128} <= Ms
    lb, d, up = sp.eval_build("signs-and-zeros")
    assert lb[0, 3] < 0 and (lb[0, 4:] < 0).all() and lb[1, 3] == 0 and lb[2, 5] == 0 and (lb[3, 4:] == 0).all()
    assert lb[4, 4] == 0 and np.signbit(lb[4, 4].item())
    gl, _ = sp.eval_oracle(lb, d, up)
    assert gl[1, 3] == 0 and gl[2, 5] == 0 and (gl[3, 4:] == 0).all() and gl[4, 4] == 0       # sign(0) = 0
    assert float(gl[0].abs().min()) > 0
    lb, d, up = sp.eval_build("sharp-on-axis")
    L = sg.sg_light(lb[:2], d[:4])
    assert abs(lb[0, 3]) == 1000 and abs(lb[1, 3]) == 1000
    assert torch.allclose(L[0], lb[0, 4:].abs()) and float(sg.sg_light(lb[:1], d[1:2]).abs().max()) == 0.0   # e = 1, exp(-2000) = 0
    assert torch.allclose(sg.sg_light(lb[1:2], d[2:3])[0], lb[1, 4:].abs()) and float(sg.sg_light(lb[1:2], d[3:4]).abs().max()) == 0.0
    lb, d, up = sp.eval_build("unnormalised-dirs")
    nrm = d.norm(dim=-1)
    assert float(nrm.min()) < 0.6 and float(nrm.max()) > 1.4
    assert float(sp.eval_build("zero-upstream")[2].abs().max()) == 0.0
    for c in sp.EVAL_CASES:
        lb, d, up = sp.eval_build(c["id"])
        assert lb.shape == (c["M"], 7) and d.shape == (c["n"], 3)
        for t in (lb, d, up):
            assert torch.equal(t.float().double(), t)          # fp32-representable


def test_eval_cases_fp32_loss_is_measured():
    for c in sp.EVAL_CASES:
        l64, d64, G = sp.eval_g32(c["id"])
        assert torch.isfinite(l64).all() and torch.isfinite(d64).all()
        print(f"{c['id']:20s} G32 d_lobes {G['d_lobes']:.2e}  d_dirs {G['d_dirs']:.2e}")
        assert G["d_lobes"] < 1e-2 and G["d_dirs"] < 1e-2


# ---- B ------------------------------------------------------------------------------------------------------------------------
def test_views_hold_what_they_are_named_for():
    v = {c["name"]: c for c in sp.views()}
    assert {(c["H"], c["W"]) for c in sp.views()} >= {(1, 1), (13, 17), (48, 64)}
    assert {c["lobes"].shape[0] for c in sp.views()} >= {1, 32, 128}
    K = v["17x13_M32_off_centre_fx_ne_fy"]["K"]
    assert K[0, 0] != K[1, 1] and K[0, 2] != 17 / 2 and K[1, 2] != 13 / 2
    K = v["64x48_M128_principal_point_outside"]["K"]
    assert K[0, 2] < 0 and K[1, 2] > 48
    for name in ("17x13_M32_opacity_edges_and_knee", "64x48_M1_above_one"):
        op = v[name]["opacity"]
        assert (op == 0).any() and (op == 1).any() and ((op > 0) & (op < 1e-5)).any() and np.isnan(op).any()
    env = sp.view_light64(v["17x13_M32_opacity_edges_and_knee"])
    assert (env < sp.SRGB_KNEE).any() and (env > sp.SRGB_KNEE).any()          # both sides of the knee
    env = sp.view_light64(v["64x48_M1_above_one"])
    assert (env > 1).any() and (env < 1).any()                                # the clip
    for c in sp.views():
        o64, r32, e32, bound, thr = sp.view_tables(c["name"])
        for k in bc.OUTPUTS:
            frac = float(thr[k].mean())
            print(f"{c['name']:40s} {k:10s} E32 {e32[k]:.2e} bound {bound[k]:.2e} threshold pixels {frac:.3%}")
            assert frac <= 0.05 and e32[k] < 1e-4


# ---- C ------------------------------------------------------------------------------------------------------------------------
def test_loss_cases_cover_every_geometry_and_lobe_count_once():
    geo = [s["geometry"] for s in sp.RL_CASES.values()]
    assert {"max_positions", "tie_3_70", "contention", "all_primaries_miss", "hits_out_of_range", "ratio_zero", "at_camera", "physical",
            "random_9x65"} <= set(geo)
    assert {s["M"] for s in sp.RL_CASES.values()} == {1, 32, 33, 128}
    c = sp.rl_case("random_9x65-M128")
    assert (c["N"], c["S"]) == (9, 65)
    assert sp.rl_case("physical-M32")["N"] == 2000
    for name in sp.RL_NAMES:
        c, g = sp.rl_case(name), lc.case(sp.RL_CASES[name]["geometry"])
        for k in (() if sp.RL_CASES[name]["geometry"] == "physical" else ("ray_d",)) + ("hit", "uvs", "xyz", "geo_normal", "visibility", "areas", "normals", "albedos", "roughnesses"):
            assert np.array_equal(c[k], g[k], equal_nan=True), (name, k)        # the geometry, untouched
        assert c["lobes"].dtype == np.float32 and c["lobes"].shape == (sp.RL_CASES[name]["M"], 7) and np.isfinite(c["lobes"]).all()


def test_non_finite_case_is_non_finite_where_it_says():
    c, o = sp.rl_case("non_finite-M32"), sp.rl_oracle("non_finite-M32")
    L, raw = sp.rl_light64(c)
    assert np.isinf(L[..., 1]).all() and np.isfinite(raw).all() and np.isfinite(L[..., 0]).all() and np.isfinite(L[..., 2]).all()
    hit_rows = np.abs(o["out_abs"][:, 0]) > 0
    assert hit_rows.sum() > 20 and o["bad"][hit_rows, 1].all() and np.isnan(o["loss"])
    assert o["bad"][2].all() and not o["bad"][4, 0] and o["bad"][6, 2]
    assert (~o["bad"]).sum() > 40                                    # red and blue of most rows keep their gradients
    d = o["d_lobes"]
    assert np.isfinite(d).all() and (d[:, 5] == 0).all() and np.abs(d[:, 4]).max() > 0 and np.abs(d[:, 6]).max() > 0


def test_e_sg_covers_the_table_and_fp32_loss_is_measured():
    worst = 0.0
    for name in sp.RL_NAMES:
        e = sp.rl_measure(name)
        o = sp.rl_oracle(name)
        print(f"{name:28s} E_SG {e:.2e}  G32 d_lobes {o['G32']:.2e}  loss {o['loss']:.6g}")
        worst = max(worst, e)
    print(f"E_SG over the table: {worst:.3e} (constant {sp.E_SG:.1e})")
    assert worst <= sp.E_SG <= 4 * worst


def test_exclusions_stay_within_the_cap_on_the_oracle():
    for name in sp.RL_NAMES:
        o = sp.rl_oracle(name)
        rows = float((o["threshold"] | o["unsafe"]).mean())
        lobes = float(o["unsafe_lobes"].mean())
        print(f"{name:28s} excluded rows {rows:.3%} lobes {lobes:.3%}")
        assert rows <= sp.MAX_EXCLUDED and lobes <= sp.MAX_EXCLUDED, name


# ---- the ABI surface, without a GPU ---------------------------------------------------------------------------------------------
NEW = ("svgir_sg_eval_backward", "svgir_env_backdrop_sg", "svgir_radiance_loss_sg_work_bytes", "svgir_radiance_loss_forward_sg",
       "svgir_radiance_loss_backward_sg")


def test_new_symbols_exist_and_the_abi_stays_14(built):
    from gaussian_renderer import _native as N
    lib = C.CDLL(N.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name) and name in N.EXPORTS, name
    assert lib.svgir_abi_version() == N.ABI_VERSION == 14
    wb = N.lib.svgir_radiance_loss_sg_work_bytes
    assert wb(10, 32) >= 8 * 32 * 4 + 8 * 3 and wb(10, 32) % 8 == 0 and wb(0, 1) > 0
    assert wb(-1, 32) == 0 and wb(10, 0) == 0 and wb(10, 129) == 0 and wb(10, -4) == 0
    assert N.lib.svgir_sg_grad_work_bytes(0) == 0 and N.lib.svgir_sg_grad_work_bytes(-1) == 0


def test_invalid_arguments_are_rejected_before_any_hip_call(built):
    """host memory stands in for device memory: a rejected call dereferences nothing"""
    from gaussian_renderer import _native as N
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    base += -base % 16
    lb, wk, a, b, c_, gw = base, base + 1024, base + 2048, base + 4096, base + 6144, base + 8192

    def light(count=4, lobes=lb, work=wk):
        lt = N.SgLight()
        lt.count, lt.lobes, lt.work = count, lobes, work
        return lt

    def bwd(lt=None, n=5, dirs=a, up=b, d_lobes=c_, d_dirs=None, work=gw):
        return N.lib.svgir_sg_eval_backward(lt or light(), n, dirs, up, d_lobes, d_dirs, work, None)

    for kw, word in ((dict(lt=light(count=0)), "count"), (dict(lt=light(count=129)), "count"), (dict(lt=light(lobes=None)), "NULL"),
                     (dict(lt=light(work=None)), "NULL"), (dict(lt=light(work=wk + 4)), "aligned"), (dict(work=None), "grad_work"),
                     (dict(n=-1), "bad n"), (dict(d_lobes=None, d_dirs=None), "both NULL"), (dict(dirs=None), "NULL dirs"),
                     (dict(up=None), "dL_dout")):
        assert bwd(**kw) == -1 and word in N.last_error(), (kw, N.last_error())
    # the backdrop: its own argument checks and the light's
    intr, rot = (C.c_float * 4)(20, 20, 8, 6), (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)

    def bd(W=4, H=4, intr=intr, rot=rot, lt=None, image=a, out=c_):
        return N.lib.svgir_env_backdrop_sg(W, H, intr, rot, lt or light(), image, a, a, out, None)

    for kw, word in ((dict(W=0), "image size"), (dict(lt=light(count=200)), "count"), (dict(lt=light(work=wk + 8)), "aligned"),
                     (dict(intr=None), "intrinsics"), (dict(image=None), "must be provided"), (dict(out=None), "must be provided"),
                     (dict(intr=(C.c_float * 4)(0, 20, 8, 6)), "focal")):
        assert bd(**kw) == -1 and word in N.last_error(), (kw, N.last_error())
    # the loss: the light's checks first, then the parameter block's
    p = N.RadianceLossParams()
    p.N, p.S = 4, 8
    for k in ("xyz", "camera_center", "geo_normal", "ray_d", "areas", "visibility", "normals", "albedos", "roughnesses", "hit_indices", "uvs",
              "radiances", "radiance_ratio", "work"):
        setattr(p, k, a)

    def fwd(p=p, lt=None, idx=b):
        return N.lib.svgir_radiance_loss_forward_sg(p, lt or light(), idx, b, b, b, None)

    def back(p=p, lt=None, d_alb=b):
        return N.lib.svgir_radiance_loss_backward_sg(p, lt or light(), b, b, b, c_, d_alb, b, None, None)

    for call in (fwd, back):
        assert call(lt=light(count=0)) == -1 and "count" in N.last_error()
        assert call(lt=light(work=wk + 4)) == -1 and "aligned" in N.last_error()
        for field, value in (("S", 0), ("N", -1), ("ray_d", None), ("work", None), ("work", a + 8)):
            q = N.RadianceLossParams()
            C.memmove(C.addressof(q), C.addressof(p), C.sizeof(p))
            setattr(q, field, value)
            assert call(p=q) == -1 and "radiance_loss" in N.last_error(), (field, N.last_error())
    assert fwd(idx=None) == -1 and back(d_alb=None) == -1
    with pytest.raises(RuntimeError, match="failed"):
        N.check(fwd(idx=None), "radiance_loss_forward_sg")
