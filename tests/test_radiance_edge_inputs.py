"""CPU checks of the irradiance case table and its oracle (tests/radiance_cases.py), and of the new surface: every case holds what it is
named for, the oracle's specular term is the shading oracle's GGX, its gradients are the autograd of an independently written torch fp64
forward and agree with central finite differences, the measured term deviations E_TERM[kind] are the ones the module states, no case spends more
than 1 % of its gradient elements on threshold terms, and the header, `_native.EXPORTS` and the library agree on the three new symbols.
No GPU work is launched."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import radiance_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = np.float64
NEW_SYMBOLS = ("svgir_pbgi_irradiance_sample", "svgir_pbgi_irradiance_sample_backward", "svgir_pbgi_irradiance")
K = {k: float(v) for k, v in rc._C.items()}     # the contract's constants (fp32 values)


# ---- the table ------------------------------------------------------------------------------------------------------------------

def test_table_lists_the_sizes_and_forms():
    for N in (1, 2, 65, 300):
        for S in (1, 3, 63, 64, 65, 128, 384):
            name = "random_%dx%d" % (N, S)
            if S == 384 and N > 65:
                assert name not in rc.CASES
                continue
            c = rc.case(name)
            assert (c["N"], c["S"]) == (N, S) and rc.has_full(name) == (S <= 128)
            assert c["ray_d"].shape == (N, S, 3) and c["envmap"].shape == (N, S, 3) and c["uvs"].shape == (N, S, 2)
            assert c["normals"].shape == (N, 12) and c["albedos"].shape == (N, 12) and c["roughnesses"].shape == (N, 4)
            assert c["hit"].shape == (N, S) and c["hit"].dtype == np.int32 and c["sample"].shape == (N,) and c["sample"].dtype == np.int32
            assert all(c[k].dtype == np.float32 and not c[k].flags.writeable for k in ("ray_d", "envmap", "normals", "albedos", "roughnesses", "uvs"))
    src = open(os.path.join(ROOT, "svg-ir_amd", "csrc", "irradiance.hip")).read()
    assert re.search(r"IRR_WAVE = (\d+)", src).group(1) == str(rc.WAVE)          # 63 / 64 / 65 and 128 / 384 straddle the pass
    assert "IRR_WAVES = BLOCK / IRR_WAVE" in src and rc.ROWS == 256 // rc.WAVE   # N = 1, 2, 65, 300: a part block, whole blocks + 1


def test_random_tables_keep_the_half_vector_away_from_zero():
    for name in ("random_65x64", "random_300x128", "random_2x384"):
        c = rc.case(name)
        unit = c["ray_d"].astype(F64) / np.linalg.norm(c["ray_d"].astype(F64), axis=-1, keepdims=True)
        worst = 2.0
        for i, p, h in rc.full_chunks(c):
            worst = min(worst, np.linalg.norm(-unit[i, p][:, None] + unit[h], axis=-1).min())
        assert worst >= 0.2 - 1e-6, name


def test_self_hit_and_miss_cases_are_zero():
    c, o = rc.case("self_hit_1x1"), rc.oracle("self_hit_1x1")
    assert c["hit"].tolist() == [[0]] and len(o["rows"]) == 1 and not o["out"].any() and not o["d_envmap"].any()
    c, o = rc.case("all_primaries_miss"), rc.oracle("all_primaries_miss")
    assert (c["hit"] == -1).all() and len(o["rows"]) == 0
    assert not rc.oracle_full("all_primaries_miss")["out"].any()
    c, o = rc.case("all_secondaries_occluded"), rc.oracle("all_secondaries_occluded")
    assert (c["hit"] >= 0).all() and len(o["rows"]) == 65 and not o["out_abs"].any() and not o["d_roughnesses_abs"].any()
    for name in ("self_hit_1x1", "all_primaries_miss", "all_secondaries_occluded"):
        o = rc.oracle(name)
        assert not any(o[k].any() for k in ("out", "d_albedos", "d_envmap", "d_roughnesses"))


def test_contention_case_sends_every_row_to_surfel_0():
    c, o = rc.case("contention"), rc.oracle("contention")
    assert len(o["rows"]) == 300 and (o["hits"] == 0).all()
    free = int((c["hit"][0] == -1).sum())
    assert free == 63 and (o["d_albedos_cnt"][0] == 300 * free).all() and not o["d_albedos_cnt"][1:].any()
    assert o["d_roughnesses_cnt"][0, 0] == 300 * free and set(np.unique(o["d_envmap_cnt"][0])) == {0.0, 300.0}


def test_uv_corner_case_sits_on_the_clamps():
    c = rc.case("uv_corners")
    assert set(np.unique(c["uvs"])) == {np.float32(0.001), np.float32(0.999)}
    pairs = {tuple(x) for x in c["uvs"][0].round(3).tolist()}
    assert len(pairs) == 4


def test_backfacing_case_clamps_every_dot():
    c = rc.case("backfacing")
    rows, p, h = rc.valid_rows(c)
    assert len(rows) == 33 and (rows & 1).all() and not (h & 1).any()
    n = c["normals"][h].astype(F64).reshape(-1, 3, 4).transpose(0, 2, 1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    V = -c["ray_d"][rows, p].astype(F64)
    V /= np.linalg.norm(V, axis=-1, keepdims=True)
    L = c["ray_d"][h].astype(F64)
    L /= np.linalg.norm(L, axis=-1, keepdims=True)
    H = V[:, None] + L
    H /= np.linalg.norm(H, axis=-1, keepdims=True)
    assert (np.einsum("ekc,ec->ek", n, V) < 0).all() and (np.einsum("ekc,esc->esk", n, L) < 0).all() and (np.einsum("ekc,esc->esk", n, H) < 0).all()
    assert np.abs(rc.oracle("backfacing")["out"][rows]).min() > 0      # (the diffuse part and the clamped specular remain)


def test_denominator_clamp_case_is_deep_inside_and_outside():
    c = rc.case("denominator_clamp")
    rows, p, h = rc.valid_rows(c)
    assert set(np.unique(c["roughnesses"])) == {np.float32(0.09), np.float32(0.99)}
    r = np.repeat(c["roughnesses"][h][:, :1].astype(F64), 4, 1)
    n = c["normals"][h].astype(F64).reshape(-1, 3, 4).transpose(0, 2, 1)
    _, _, _, raw = rc.specular(F64, -c["ray_d"][rows, p].astype(F64), c["ray_d"][h].astype(F64), n, r, grad=True)
    low, high = r[:, 0] < 0.5, r[:, 0] > 0.5
    assert low.any() and high.any()
    assert raw[low].max() < 1e-6 / 10 and raw[high].min() > 1.0          # clamped by a factor >= 10; inside
    V = -c["ray_d"][rows, p].astype(F64)
    H = V / np.linalg.norm(V, axis=-1, keepdims=True)
    L = c["ray_d"][h].astype(F64)
    H = H[:, None] + L / np.linalg.norm(L, axis=-1, keepdims=True)
    H /= np.linalg.norm(H, axis=-1, keepdims=True)
    noh = np.einsum("ekc,esc->esk", n / np.linalg.norm(n, axis=-1, keepdims=True), H)
    assert noh.min() > 1 - 1e-4


def test_out_of_range_indices_are_misses():
    c, o = rc.case("indices_out_of_range"), rc.oracle("indices_out_of_range")
    N, S = c["N"], c["S"]
    assert c["sample"][0] == -1 and c["sample"][1] == S and c["hit"][2, c["sample"][2]] == -2 and c["hit"][3, c["sample"][3]] == N
    assert not set(o["rows"].tolist()) & {0, 1, 2, 3} and not o["out"][:4].any()
    assert 4 in o["rows"] and o["hits"][o["rows"].tolist().index(4)] == 5
    assert sorted(np.unique(c["hit"][5]).tolist()) == [-2, -1, N]
    # of surfel 5's samples only the exact -1 escape
    assert (o["d_envmap_cnt"][5, :, 0] > 0).tolist() == (c["hit"][5] == -1).tolist()
    full = rc.oracle_full("indices_out_of_range")
    assert not full["out_abs"][2, c["sample"][2]].any() and not full["out_abs"][3, c["sample"][3]].any()


def test_physical_case_is_a_real_mix(built):
    c = rc.case("physical")
    assert c["N"] == 2000 and c["S"] == 16
    hit = c["hit"]
    assert (hit == -1).mean() >= 0.05 and (hit >= 0).mean() >= 0.05
    rows, p, h = rc.valid_rows(c)
    occluded = (hit[h] != -1).mean()
    assert occluded >= 0.05 and 1 - occluded >= 0.05 and len(rows) >= 0.05 * c["N"] and c["N"] - len(rows) >= 0.05 * c["N"]
    assert hit.min() >= -1 and hit.max() < c["N"] and c["uvs"].min() >= 0 and c["uvs"].max() <= 1
    lo = rc.loss_oracle()
    # the selection of radiance_loss is either clear of fp32 rounding or an exact tie (the first index wins in numpy and torch alike)
    assert ((lo["margin"] == 0) | (lo["margin"] > 1e-5)).all() and len(np.unique(lo["sel"])) == c["S"]
    assert lo["unsafe"].mean() <= 0.01


# ---- the oracle -----------------------------------------------------------------------------------------------------------------

def test_specular_term_is_the_shading_oracles_ggx():
    """oracle/shading_oracle.py's `ggx` is pinned against the reference; it flips the normal toward the viewer and shading_brdf_simple
    does not, so the inputs have n.v > 0."""
    from oracle import shading_oracle as so
    rng = np.random.default_rng(5)
    E, S = 200, 24
    base = rc._unit(rng, (E,))
    n = base[:, None] + 0.2 * rng.normal(size=(E, 4, 3))
    V = base + 0.5 * rng.normal(size=(E, 3))
    L = rc._unit(rng, (E, S)) * rng.uniform(0.5, 2.0, size=(E, S, 1))
    r = rng.uniform(0.09, 0.99, size=(E, 4))
    keep = ((n / np.linalg.norm(n, axis=-1, keepdims=True)) @ V[:, :, None])[..., 0].min(1) > 0.05
    assert keep.sum() > 100
    n, V, L, r = n[keep], V[keep], L[keep], r[keep]
    mine = rc.specular(F64, V, L, n, r)
    t = lambda a: torch.from_numpy(a)
    theirs = so.ggx(t(n), t(V), t(L), t(r)).numpy()
    assert mine.shape == theirs.shape == (keep.sum(), S, 4)
    assert np.abs(mine - theirs).max() <= 1e-6 * np.abs(theirs).max() and (np.abs(mine - theirs) <= 1e-6 * np.abs(theirs) + 1e-12).all()


def _torch_forward(c, env, alb, rough):
    """The sample form written independently, vectorised, in torch fp64 (the reference's own form of n0)."""
    N, S = c["N"], c["S"]
    t = lambda k: torch.from_numpy(c[k].copy()).double()
    hit, ar = torch.from_numpy(c["hit"].copy()).long(), torch.arange(N)
    p = torch.from_numpy(c["sample"].copy()).long()
    h = hit[ar, p.clamp(0, S - 1)]
    ok = (p >= 0) & (p < S) & (h >= 0) & (h < N)
    hh, nz = h.clamp(0, N - 1), torch.nn.functional.normalize
    V = nz(-t("ray_d")[ar, p.clamp(0, S - 1)], dim=-1)
    L = nz(t("ray_d")[hh], dim=-1)
    H = nz(V[:, None] + L, dim=-1)
    n = nz(t("normals")[hh].view(N, 3, 4).transpose(1, 2), dim=-1)
    cl = lambda x: x.clamp(K["eps"], 1.0)
    NoL, NoH = cl(torch.einsum("nkc,nsc->nsk", n, L)), cl(torch.einsum("nkc,nsc->nsk", n, H))
    NoV, VoH = cl(torch.einsum("nkc,nc->nk", n, V))[:, None], cl((V[:, None] * H).sum(-1))[..., None]
    r = rough[hh][:, 0][:, None, None]
    a2 = r ** 4
    k = (r * r + 2 * r + 1) / 8
    fres = K["f0"] + K["f1"] * torch.pow(torch.tensor(2.0, dtype=torch.float64), (K["ea"] * VoH - K["eb"]) * VoH)
    den = (K["pi4"] * (NoH * NoH * (a2 - 1) + 1) ** 2 * (NoV * (1 - k) + k) * (NoL * (1 - k) + k)).clamp(K["eps"], K["pi4"])
    brdf = (fres * a2 / den)[:, :, None, :] + alb[hh].view(N, 1, 3, 4) * K["ipi"]
    u, v = t("uvs")[hh][..., 0], t("uvs")[hh][..., 1]
    w = torch.stack([(1 - u) * (1 - v), u * (1 - v), (1 - u) * v, u * v], -1)
    free = (hit[hh] == -1) & ok[:, None]
    return ((brdf * w[:, :, None, :]).sum(-1) * env[hh] * free[..., None]).sum(1) / S


GRAD_CASES = ("random_2x3", "random_65x3", "random_65x65", "random_300x64", "contention", "uv_corners", "backfacing", "denominator_clamp",
              "indices_out_of_range", "physical")


@pytest.mark.parametrize("name", GRAD_CASES)
def test_oracle_equals_autograd_of_an_independent_forward(built, name):
    c, o = rc.case(name), rc.oracle(name)
    leaves = [torch.from_numpy(c[k].astype(F64)).requires_grad_(True) for k in ("envmap", "albedos", "roughnesses")]
    out = _torch_forward(c, *leaves)
    scale = max(np.abs(o["out"]).max(), 1e-30)
    assert np.abs(out.detach().numpy() - o["out"]).max() <= 1e-9 * scale
    out.backward(torch.from_numpy(c["grad_out"].astype(F64)))
    for leaf, k in zip(leaves, ("d_envmap", "d_albedos", "d_roughnesses")):
        got, want = leaf.grad.numpy(), o[k]
        if k == "d_roughnesses":
            assert not want[:, 1:].any()
            keep = ~o["thr"]
            got, want, mag = got[keep], want[keep], o[k + "_abs"][keep]
        else:
            mag = o[k + "_abs"]
        assert (np.abs(got - want) <= 1e-8 * mag + 1e-300).all(), k


def _torch_full_forward(c):
    """The full form written independently from intersect_test.slang:901-1138, vectorised over (i, p, s, corner) in torch fp64: per-corner
    roughness (:1042-1045), the reference's own form of n0, and each corner's brdf times clamp(dot(stored normal, normalised secondary
    direction), 1e-6, 1) (:1063-1066) before the uv blend."""
    N, S = c["N"], c["S"]
    t = lambda k: torch.from_numpy(c[k].copy()).double()
    nz = torch.nn.functional.normalize
    hit = torch.from_numpy(c["hit"].copy()).long()                    # [N,S]
    ok = (hit >= 0) & (hit < N)
    h = hit.clamp(0, N - 1)                                           # [N,P]
    V = nz(-t("ray_d"), dim=-1)[:, :, None, None, :]                  # [N,P,1,1,3]
    L = nz(t("ray_d"), dim=-1)[h][:, :, :, None, :]                   # [N,P,S,1,3]
    H = nz(V + L, dim=-1)
    nraw = t("normals").view(N, 3, 4).transpose(1, 2)[h][:, :, None]  # [N,P,1,4,3]
    n = nz(nraw, dim=-1)
    cl = lambda x: x.clamp(K["eps"], 1.0)
    NoL, NoV, NoH, VoH = cl((n * L).sum(-1)), cl((n * V).sum(-1)), cl((n * H).sum(-1)), cl((V * H).sum(-1))
    r = t("roughnesses")[h][:, :, None, :]                            # [N,P,1,4]
    a2 = r ** 4
    k = (r * r + 2 * r + 1) / 8
    fres = K["f0"] + K["f1"] * torch.pow(torch.tensor(2.0, dtype=torch.float64), (K["ea"] * VoH - K["eb"]) * VoH)
    den = (K["pi4"] * (NoH * NoH * (a2 - 1) + 1) ** 2 * (NoV * (1 - k) + k) * (NoL * (1 - k) + k)).clamp(K["eps"], K["pi4"])
    spec = fres * a2 / den                                            # [N,P,S,4]
    alb = t("albedos").view(N, 3, 4)[h][:, :, None]                   # [N,P,1,3,4]
    cosn = cl((nraw * L).sum(-1))                                     # [N,P,S,4]
    corner = (spec[:, :, :, None, :] + alb * K["ipi"]) * cosn[:, :, :, None, :]          # [N,P,S,3,4]
    uv = t("uvs")[h]                                                  # [N,P,S,2]
    u, v = uv[..., 0], uv[..., 1]
    w = torch.stack([(1 - u) * (1 - v), u * (1 - v), (1 - u) * v, u * v], -1)
    free = (hit[h] == -1) & ok[:, :, None]                            # [N,P,S]
    return ((corner * w[:, :, :, None, :]).sum(-1) * t("envmap")[h] * free[..., None]).sum(2) / S


@pytest.mark.parametrize("name", ["random_2x3", "random_65x3", "random_65x65", "uv_corners", "backfacing", "indices_out_of_range"])
def test_full_form_oracle_equals_an_independent_forward(name):
    c, o = rc.case(name), rc.oracle_full(name)
    got = _torch_full_forward(c).numpy()
    assert got.shape == o["out"].shape
    assert (np.abs(got - o["out"]) <= 1e-9 * o["out_abs"] + 1e-300).all()
    if name != "indices_out_of_range":
        assert o["out_abs"].any()
    # per-corner roughness and the cosine are what tell the two forms apart: the sample form's arithmetic must NOT reproduce this
    rows, p, h = rc.valid_rows(c)
    free_rows = [j for j in range(len(rows)) if (c["hit"][h[j]] == -1).any()]
    if free_rows:
        s_out = rc.oracle(name)["out"][rows[free_rows]]
        f_out = o["out"][rows[free_rows], p[free_rows]]
        assert (np.abs(s_out - f_out) > 1e-3 * np.abs(s_out)).any()


def test_oracle_gradients_agree_with_central_differences():
    name = "random_65x3"
    c, o = rc.case(name), rc.oracle(name)
    g = c["grad_out"].astype(F64)

    def value(**over):
        c2 = dict(c, **over)
        rows, _, _, t = rc.sample_terms(F64, c2, g=False)
        return (t["t_out"].sum(1) * g[rows]).sum()

    hits = np.unique(o["hits"])[:6]
    eps = 1e-6
    for key, grad, cols in (("roughnesses", "d_roughnesses", (0,)), ("albedos", "d_albedos", (0, 5, 11)), ("envmap", "d_envmap", (0,))):
        for h in hits:
            for col in cols:
                idx = (h, col) if key != "envmap" else (h, col, 1)
                if key == "envmap" and c["hit"][h, col] != -1:
                    continue
                base = c[key].astype(F64)
                up, dn = base.copy(), base.copy()
                up[idx] += eps
                dn[idx] -= eps
                fd = (value(**{key: up}) - value(**{key: dn})) / (2 * eps)
                assert abs(fd - o[grad][idx]) <= 1e-6 * o[grad + "_abs"][idx] + 1e-9, (key, idx, fd, o[grad][idx])


def test_term_deviations_are_the_stated_constants_and_thresholds_stay_under_the_cap(built):
    """E_TERM[kind] of the module are the measured values (the GPU test's tolerance is 4 E_TERM[kind] next to the summation bound), kind
    by kind: not smaller than what the table and radiance_loss's case give today and at most a tenth larger.  Threshold terms exclude
    at most 1 % of a case's gradient elements."""
    worst = {k: (0.0, "") for k in rc.KINDS}
    measured = {name: rc.term_deviation(name) for name in rc.CASES}
    measured["radiance_loss"] = rc.term_deviation_of(rc.loss_oracle()["case"], False)
    for name, dev in measured.items():
        for k, v in dev.items():
            if v > worst[k][0]:
                worst[k] = (v, name)
    for name in rc.CASES:
        o = rc.oracle(name)
        total = o["d_envmap"].size + o["d_albedos"].size + o["d_roughnesses"].size
        assert o["thr"].sum() <= 0.01 * total, name
    k2 = rc.loss_oracle()["kernel"]
    assert k2["thr"].sum() <= 0.01 * (k2["d_envmap"].size + k2["d_albedos"].size + k2["d_roughnesses"].size)
    assert set(rc.E_TERM) == set(rc.KINDS)
    for k, (v, name) in worst.items():
        print("E_TERM[%s] measured %.4g (%s); stated %.4g" % (k, v, name, rc.E_TERM[k]))
        assert v <= rc.E_TERM[k] <= 1.1 * v, (k, name, v)
    # what the split buys: the sample form, which has no cosine factor, is not held to the full form's grazing cosines
    assert max(rc.E_TERM[k] for k in rc.KINDS if k != "full") < rc.E_TERM["full"] / 20


# ---- the surface ----------------------------------------------------------------------------------------------------------------

def test_header_exports_and_library_agree_on_the_new_symbols(built):
    from gaussian_renderer import _native
    hdr = open(os.path.join(ROOT, "include", "svgir_raster.h")).read()
    lib = C.CDLL(_native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _native.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define SVGIR_ABI_VERSION (\d+)", hdr).group(1) == "14" and _native.ABI_VERSION == 14
    # argument checks come before any HIP call; N = 0 launches nothing
    nargs = {"svgir_pbgi_irradiance_sample": 10, "svgir_pbgi_irradiance_sample_backward": 13, "svgir_pbgi_irradiance": 9}
    for name, n in nargs.items():
        fn = getattr(lib, name)
        fn.argtypes = [C.c_int32, C.c_int32] + [C.c_void_p] * n
        assert fn(-1, 4, *[None] * n) == -1 and fn(5, 4, *[None] * n) == -1 and fn(5, 0, *[None] * n) == -1
        assert fn(0, 4, *[None] * n) == 0
        assert fn(1 << 20, 1 << 12, *[None] * n) == -1      # N * S beyond int32


def test_renderer_offers_the_references_signatures(built):
    from pbgi.renderer import Renderer
    from svgir_harness import losses
    assert list(inspect.signature(Renderer.render_irradiance).parameters) == [
        "self", "N", "S", "envmap", "ray_directions", "centers", "scales", "rotates", "normals", "albedos", "roughnesses", "metallics", "opacities",
        "SHs"]
    assert list(inspect.signature(Renderer.render_irradiance_sample).parameters) == [
        "self", "N", "S", "sample_indices", "envmap", "ray_directions", "centers", "scales", "rotates", "normals", "albedos", "roughnesses",
        "metallics", "opacities", "SHs"]
    assert list(inspect.signature(losses.radiance_loss).parameters) == [
        "renderer", "xyz", "camera_center", "geo_normal", "incident_dirs", "visibility", "envmap", "normals12", "albedos", "roughnesses",
        "radiances", "radiance_ratio"]
    assert "forward only" in Renderer.render_irradiance.__doc__.lower()
    r = Renderer()
    x = torch.zeros(2, 3, 3)
    with pytest.raises(RuntimeError, match="are not set"):
        r.render_irradiance(2, 3, x, x, None, None, None, torch.zeros(2, 12), torch.zeros(2, 12), torch.zeros(2, 4), None, None, None)
    r.hemi_index_buffers, r.uv_buffers = torch.zeros(2, 3, 1, dtype=torch.int32), torch.zeros(2, 3, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.render_irradiance_sample(2, 3, torch.zeros(2, 1, dtype=torch.int32), x, x, None, None, None, torch.zeros(2, 12), torch.zeros(2, 12),
                                   torch.zeros(2, 4), None, None, None)
