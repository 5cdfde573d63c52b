"""Generates tests/golden/densify.npz, densify_nan.npz and densify_edges.npz by running the REFERENCE's own GaussianModel methods (scene/gaussian_model.py) in the
authoring container on the CPU: `step()` (replace_nangrad_to_zero + torch.optim.Adam.step + zero_grad, :775-813) and
`densify_and_prune` (-> densify_and_clone, densify_and_split, densification_postfix, cat_tensors_to_optimizer, prune_points,
_prune_optimizer, :1020-1268) on a GaussianModel created with __new__ and filled with seeded tensors.  CUDA device arguments
are redirected to the CPU, `torch.normal(mean, std)` is replaced by mean + std * Z with recorded draws Z (the product is fed the
same Z).  The fixture is data only: inputs, the gradients, and the tensors the reference ended up with.

densify_edges.npz (`edges()`): a list of small scenes (P <= 64), each run through the reference's `densify_and_prune` (or
`prune`) and one more `step()`: nothing / everything cloned, split or pruned, P = 1 and P = 0, exact threshold ties, 0 / 0 and
x / 0 mean gradients, negative accumulators, and densification before any Adam state exists.  Keys are `<scene>/<block>`; a
block that holds one tensor per parameter group is stored as one flat fp32 vector, the groups in SPEC order, next to
`<block>_has` (which groups are present: a group without a gradient or without Adam state contributes nothing); the row count
is the vector's length over the present groups' row widths (tests/optim_cases.py `unpack_block`).

    python scripts/make_golden_densify.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import make_golden as mg             # noqa: E402
import make_golden_view as mgv       # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
# group name, per-Gaussian shape, learning rate (scene/gaussian_model.py:745-768 with the default OptimizationParams scale)
SPEC = [("xyz", (3,), 1.6e-4), ("normal", (12,), 1e-3), ("rotation", (4,), 1e-3), ("scaling", (3,), 5e-3), ("opacity", (1,), 5e-2),
        ("f_dc", (1, 3), 2.5e-3), ("f_rest", (15, 3), 1.25e-4), ("base_color", (12,), 1e-2), ("roughness", (4,), 1e-2),
        ("incidents_dc", (1, 3), 2e-3), ("incidents_rest", (15, 3), 1e-4), ("visibility_dc", (1, 1), 2.5e-3),
        ("visibility_rest", (15, 1), 1.25e-4)]
ATTR = {"xyz": "_xyz", "normal": "_normal", "rotation": "_rotation", "scaling": "_scaling", "opacity": "_opacity", "f_dc": "_shs_dc",
        "f_rest": "_shs_rest", "base_color": "_base_color", "roughness": "_roughness", "incidents_dc": "_incidents_dc",
        "incidents_rest": "_incidents_rest", "visibility_dc": "_visibility_dc", "visibility_rest": "_visibility_rest"}


POISON_ROWS = {5: (float("nan"),) * 3, 6: (float("nan"), None, None), 7: (100.0,) * 3, 8: (None, 100.0, None),
               9: (float("nan"), float("nan"), None), 10: (None, None, float("nan"))}   # row -> per-axis override of the log-scale


def main(fname="densify.npz", poison=False):
    """`poison`: a second fixture (densify_nan.npz) whose `_scaling` has NaN / overflowing rows -- the case the reference's
    get_scaling = nan_to_num(exp(.), nan=1e-6) exists for (scene/gaussian_model.py:270-272) -- all of them selected for
    densification."""
    mgv.setup_reference()
    import torch.utils.cpp_extension as cpp
    cpp.load = lambda *a, **k: mg._Stub("_C")
    from scene.gaussian_model import GaussianModel
    g = torch.Generator().manual_seed(4242)
    P = 300
    out = {}
    with mgv.cpu_reference():
        gm = GaussianModel.__new__(GaussianModel)
        gm.use_pbr = True
        gm.percent_dense = 0.01
        gm.setup_functions()
        init = {}
        for name, shp, lr in SPEC:
            t = torch.randn((P,) + shp, generator=g)
            if name == "scaling":   # log-scales around the clone / split limit percent_dense * extent = 0.05
                t = torch.log(torch.exp(torch.empty(P, 3).uniform_(np.log(0.01), np.log(0.2), generator=g)))
            if name == "scaling" and poison:
                for r, ov in POISON_ROWS.items():
                    for ax, v in enumerate(ov):
                        if v is not None:
                            t[r, ax] = v
            if name == "opacity" and poison:
                t[sorted(POISON_ROWS)] = 2.0
            if name == "xyz":
                t = t * 0.8
            init[name] = t.clone()
            setattr(gm, ATTR[name], torch.nn.Parameter(t.clone().requires_grad_(True)))
            out["init_" + name] = t.numpy()
        groups = [{"params": [getattr(gm, ATTR[n])], "lr": lr, "name": n} for n, _, lr in SPEC]
        gm.optimizer = torch.optim.Adam(groups, lr=1e-4, eps=1e-15)
        # ---- three optimisation steps with NaN-poisoned gradients ----
        for it in range(3):
            for name, shp, lr in SPEC:
                gr = torch.randn((P,) + shp, generator=g) * 1e-2
                bad = torch.rand((P,) + shp, generator=g) < 0.01
                gr[bad] = float("nan")
                if it == 1 and name == "incidents_rest":
                    gr = None            # a group without a gradient this iteration
                getattr(gm, ATTR[name]).grad = gr
                out[f"grad{it}_{name}"] = gr.numpy() if gr is not None else np.zeros(0, np.float32)
            gm.step()
        for name, _, _ in SPEC:
            p = getattr(gm, ATTR[name])
            st = gm.optimizer.state[p]
            out["step_" + name] = p.detach().numpy().copy()
            out["step_m_" + name] = st["exp_avg"].numpy().copy()
            out["step_v_" + name] = st["exp_avg_sq"].numpy().copy()
            assert p.grad is None      # zero_grad(set_to_none=True)
        # ---- densify_and_prune ----
        gm.weights_accum = torch.rand(P, 1, generator=g) * 2e-5          # some below the 1e-5 threshold
        gm.xyz_gradient_accum = torch.rand(P, 1, generator=g) * 6e-4
        gm.normal_gradient_accum = torch.rand(P, 1, generator=g) * 2e-4
        gm.denom = torch.randint(0, 3, (P, 1), generator=g).float()     # zeros -> NaN / inf grads
        gm.max_radii2D = torch.rand(P, generator=g) * 30
        if poison:   # the poisoned rows pass the gradient test and survive the weight / screen-size pruning (their opacity: set at init)
            rows = sorted(POISON_ROWS)
            gm.xyz_gradient_accum[rows] = 1e-3
            gm.denom[rows] = 1.0
            gm.weights_accum[rows] = 2e-5
            gm.max_radii2D[rows] = 1.0
        for k in ("weights_accum", "xyz_gradient_accum", "normal_gradient_accum", "denom", "max_radii2D"):
            out["stat_" + k] = getattr(gm, k).numpy().copy()
        Z = []
        real_normal = torch.normal

        def fake_normal(mean, std, **kw):
            z = torch.randn(std.shape, generator=g)
            Z.append(z)
            return mean + std * z
        torch.normal = fake_normal
        try:
            args = dict(max_grad=2e-4, min_opacity=0.05, extent=5.0, max_screen_size=20, max_grad_normal=1.5e-4)
            gm.densify_and_prune(**args)
        finally:
            torch.normal = real_normal
        out["densify_args"] = np.array([args["max_grad"], args["min_opacity"], args["extent"], args["max_screen_size"], args["max_grad_normal"]])
        out["split_z"] = torch.cat(Z, 0).numpy() if Z else np.zeros((0, 3), np.float32)
        for name, _, _ in SPEC:
            p = getattr(gm, ATTR[name])
            st = gm.optimizer.state[p]
            out["dens_" + name] = p.detach().numpy().copy()
            out["dens_m_" + name] = st["exp_avg"].numpy().copy()
            out["dens_v_" + name] = st["exp_avg_sq"].numpy().copy()
        for k in ("weights_accum", "xyz_gradient_accum", "normal_gradient_accum", "denom", "max_radii2D"):
            out["dens_" + k] = getattr(gm, k).numpy().copy()
    np.savez_compressed(os.path.join(OUT, fname), **out)
    print("wrote", fname, ": P", P, "->", out["dens_xyz"].shape[0], "split draws", out["split_z"].shape,
          "NaN scaling entries after densify:", int(np.isnan(out["dens_scaling"]).sum()))


# ---- densify_edges.npz -------------------------------------------------------------------------------------------------------
ARGS = dict(max_grad=2e-4, min_opacity=0.05, extent=5.0, max_screen_size=20, max_grad_normal=1.5e-4)
# row kind -> overrides of the quiet default row (accum 1e-5 / denom 1: not selected; log-scale -4: 0.018 <= 0.05, small;
# opacity >= 0: kept; weights_accum 2e-5, max_radii2D 1: kept).  `ls`: the three log-scales.
KINDS = {
    "idle": {},
    "clone": dict(accum=1e-3),
    "split": dict(accum=1e-3, denom=2.0, ls=(-2.0, -3.0, -2.5)),
    "neg_big": dict(accum=-1e-3, ls=(-2.0, -3.0, -2.5)),            # |g| selects, g does not: the reference leaves it alone
    "neg_small": dict(accum=-1e-3),                                   # cloned on the norm
    "nneg_big": dict(naccum=-1e-3, ls=(-3.0, -2.0, -2.5)),           # the same on the normal accumulator
    "nneg_small": dict(naccum=-1e-3),
    "n_split": dict(accum=0.0, naccum=1e-3, ls=(-2.5, -3.0, -2.0)),
    "n_clone": dict(accum=0.0, naccum=1e-3),
    "tie_size": dict(accum=1e-3, ls=(0.0, -1.0, -0.5)),              # exp(0) = 1 = 0.01 * 100 exactly: <= holds, cloned
    "nan_scale": dict(accum=1e-3, ls=(float("nan"),) * 3),           # get_scaling 1e-6 = fp32(0.01 * 1e-4): cloned
    "tie_grad": dict(accum=3e-4),                                     # == max_grad 3e-4 in fp32: selected
    "tie_ngrad": dict(accum=0.0, naccum=2.5e-4),                      # == max_grad_normal 2.5e-4
    "inf_grad": dict(accum=1e-3, denom=0.0),                          # x / 0 = inf: selected
    "inf_split": dict(accum=1e-3, denom=0.0, ls=(-2.0, -3.0, -2.5)),
    "ninf_big": dict(accum=-1e-3, denom=0.0, ls=(-2.0, -3.0, -2.5)),  # -inf: norm selects, sign does not, and it is big
    "nan_grad": dict(accum=0.0, denom=0.0),                           # 0 / 0 = NaN -> 0: not selected
    "zero_quat": dict(accum=1e-3, ls=(-2.0, -3.0, -2.5), quat=(0.0, 0.0, 0.0, 0.0)),
    "flat": dict(accum=1e-3, ls=(-2.0, -2.5, -1e10)),                 # a split row that is the child of an earlier split
    "low_opacity": dict(opacity=-5.0),
    "low_weight": dict(weight=1e-6),
    "big_screen": dict(radii=30.0),
    "big_world": dict(ls=(-0.5, -3.0, -3.0)),                         # 0.61 > 0.1 * 5: pruned when max_screen_size is set
    "clone_low_opacity": dict(accum=1e-3, opacity=-5.0),              # cloned, then both copies pruned
}
MIXED = ["idle", "clone", "split", "neg_big", "neg_small", "nneg_big", "nneg_small", "n_split", "n_clone", "inf_grad", "inf_split",
         "ninf_big", "nan_grad", "zero_quat", "flat", "low_opacity", "low_weight", "big_screen", "big_world", "clone_low_opacity",
         "split", "idle", "clone"]


def edge_scenes():
    """(name, row kinds, densify arguments, options).  Options: pre = optimisation steps before (0: no Adam state at all),
    skip = a group that never receives a gradient before the densification, op = the method called, hold = the scaling group
    receives a zero gradient in the steps before (exact log-scales stay exact)."""
    S = []
    for tag, n in (("p1", 1), ("p5", 5)):
        S += [(f"nothing_{tag}", ["clone"] * n, dict(ARGS, max_grad=1e9, max_grad_normal=1e9), {}),
              (f"all_clone_{tag}", ["clone"] * n, ARGS, {}),
              (f"all_clone_thr0_{tag}", ["idle"] * n, dict(ARGS, max_grad=0.0, max_grad_normal=0.0), {}),
              (f"all_split_{tag}", ["split"] * n, ARGS, {}),
              (f"all_split_noscreen_{tag}", ["split"] * n, dict(ARGS, max_screen_size=None), {}),
              (f"all_split_thr0_{tag}", ["split"] * n, dict(ARGS, max_grad=0.0, max_grad_normal=0.0), {}),
              (f"all_pruned_{tag}", ["clone"] * n, dict(ARGS, min_opacity=2.0), {}),
              (f"all_split_all_pruned_{tag}", ["split"] * n, dict(ARGS, min_opacity=2.0), {})]
    S += [("empty", [], ARGS, {}),
          ("empty_prune", [], ARGS, dict(op="prune")),
          ("negative_accum", ["neg_big"] * 12, ARGS, {}),
          ("negative_normal_accum", ["nneg_big"] * 3 + ["ninf_big"] * 2, ARGS, {}),
          ("tie_size", ["tie_size", "idle", "tie_size"], dict(ARGS, extent=100.0), dict(hold=True)),
          ("nan_scale_at_limit", ["nan_scale", "clone", "nan_scale"], dict(ARGS, extent=1e-4, max_screen_size=None), dict(hold=True)),
          ("tie_grad", ["tie_grad", "idle", "tie_ngrad", "tie_grad"], dict(ARGS, max_grad=3e-4, max_grad_normal=2.5e-4), {}),
          ("denom0_positive", ["inf_grad", "idle", "inf_split"], ARGS, {}),
          ("denom0_zero", ["nan_grad"] * 3, ARGS, {}),
          ("no_state", ["clone"] * 50, ARGS, dict(pre=0)),
          ("one_group_no_state", ["clone"] * 50, ARGS, dict(skip="incidents_rest")),
          ("mixed", MIXED, ARGS, {}),
          ("mixed_noscreen", MIXED, dict(ARGS, max_screen_size=None), {}),
          ("mixed_no_state", MIXED, ARGS, dict(pre=0)),
          ("mixed_two_steps_one_group_skipped", MIXED, ARGS, dict(pre=2, skip="visibility_rest")),
          ("prune_mixed", MIXED, ARGS, dict(op="prune")),
          ("prune_all", ["idle"] * 4, dict(ARGS, min_opacity=2.0), dict(op="prune")),
          ("prune_p1", ["low_weight"], ARGS, dict(op="prune"))]
    return S


def _coarse(g, shape, scale, levels=8):
    """seeded values on a coarse grid (multiples of scale / levels, up to 2 scale): exact in fp32, and the fixture compresses"""
    return torch.randint(-2 * levels, 2 * levels + 1, shape, generator=g).float() * (scale / levels)


def edges(fname="densify_edges.npz"):
    mgv.setup_reference()
    import torch.utils.cpp_extension as cpp
    cpp.load = lambda *a, **k: mg._Stub("_C")
    from scene.gaussian_model import GaussianModel
    out = {"scenes": np.array([s[0] for s in edge_scenes()])}
    for si, (scene, kinds, args, opt) in enumerate(edge_scenes()):
        g = torch.Generator().manual_seed(7000 + si)
        P = len(kinds)
        rows = [KINDS[k] for k in kinds]
        put = lambda k, v: out.__setitem__(f"{scene}/{k}", v)

        def put_block(k, tensors):
            """tensors: one per SPEC group, or None"""
            has = np.array([t is not None for t in tensors])
            put(k, np.concatenate([t.detach().numpy().astype(np.float32).reshape(-1) for t in tensors if t is not None] or [np.zeros(0, np.float32)]))
            put(k + "_has", has)
        with mgv.cpu_reference():
            gm = GaussianModel.__new__(GaussianModel)
            gm.use_pbr, gm.percent_dense = True, 0.01
            gm.setup_functions()
            init = []
            for name, shp, lr in SPEC:
                t = _coarse(g, (P,) + shp, 1.0, 32)
                for r, row in enumerate(rows):
                    if name == "scaling":
                        t[r] = torch.tensor(row.get("ls", (-4.0, -4.5, -5.0)))
                    if name == "opacity":
                        t[r] = row.get("opacity", float(t[r].abs()))
                    if name == "rotation":
                        t[r] = torch.tensor(row["quat"]) if "quat" in row else t[r] + torch.tensor([3.0, 0.0, 0.0, 0.0])
                setattr(gm, ATTR[name], torch.nn.Parameter(t.clone().requires_grad_(True)))
                init.append(t.clone())
            put_block("init", init)
            put("rows", np.array(P))
            gm.optimizer = torch.optim.Adam([{"params": [getattr(gm, ATTR[n])], "lr": lr, "name": n} for n, _, lr in SPEC], lr=1e-4, eps=1e-15)
            pre = opt.get("pre", 1)
            put("pre", np.array(pre))
            for it in range(pre):
                grads = []
                for name, shp, lr in SPEC:
                    gr = _coarse(g, (P,) + shp, 1e-2)
                    gr[torch.rand((P,) + shp, generator=g) < 0.02] = float("nan")
                    if name == "scaling" and opt.get("hold"):
                        gr = torch.zeros((P,) + shp)
                    if name == "rotation":       # a zero quaternion stays one: a zero gradient leaves its row untouched
                        gr[[r for r, row in enumerate(rows) if "quat" in row]] = 0.0
                    if name == opt.get("skip"):
                        gr = None
                    getattr(gm, ATTR[name]).grad = gr
                    grads.append(None if gr is None else gr.clone())
                put_block(f"grad{it}", grads)
                gm.step()
            col = lambda key, default: torch.tensor([row.get(key, default) for row in rows], dtype=torch.float32).reshape(P, 1)
            gm.weights_accum = col("weight", 2e-5)
            gm.xyz_gradient_accum = col("accum", 1e-5)
            gm.normal_gradient_accum = col("naccum", 0.0)
            gm.denom = col("denom", 1.0)
            gm.max_radii2D = col("radii", 1.0).reshape(P)
            stat = lambda: np.stack([getattr(gm, k).numpy().reshape(-1) for k in
                                     ("weights_accum", "xyz_gradient_accum", "normal_gradient_accum", "denom", "max_radii2D")])
            put("stat", stat())          # [5, P]
            Z = []
            real_normal = torch.normal

            def fake_normal(mean, std, **kw):
                z = _coarse(g, tuple(std.shape), 2.0)
                Z.append(z)
                return mean + std * z
            torch.normal = fake_normal
            op = opt.get("op", "densify_and_prune")
            try:
                if op == "prune":
                    gm.prune(args["min_opacity"], args["extent"], args["max_screen_size"], weights_threshold=1e-5)
                else:
                    gm.densify_and_prune(**args)
            finally:
                torch.normal = real_normal
            put("op", np.array(op))
            put("args", np.array([args["max_grad"], args["min_opacity"], args["extent"],
                                  float("nan") if args["max_screen_size"] is None else args["max_screen_size"], args["max_grad_normal"]]))
            put("split_z", torch.cat(Z, 0).numpy() if Z else np.zeros((0, 3), np.float32))

            def record(tag):
                ps = [getattr(gm, ATTR[name]) for name, _, _ in SPEC]
                sts = [gm.optimizer.state.get(p, None) for p in ps]
                put_block(tag, ps)
                put_block(tag + "_m", [st["exp_avg"] if st else None for st in sts])      # (no Adam state: absent, step -1)
                put_block(tag + "_v", [st["exp_avg_sq"] if st else None for st in sts])
                put(tag + "_t", np.array([float(st["step"]) if st else -1.0 for st in sts]))
                put(tag + "_stat", stat())
                put(tag + "_rows", np.array(ps[0].shape[0]))
            record("dens")
            # ---- one more step() on the new block ----
            grads = []
            for name, shp, lr in SPEC:
                p = getattr(gm, ATTR[name])
                gr = _coarse(g, tuple(p.shape), 1e-2)
                if p.shape[0]:
                    gr[0].view(-1)[0] = float("nan")
                p.grad = gr
                grads.append(gr.clone())
            put_block("post_grad", grads)
            gm.step()
            record("post")
        print(f"{scene}: P {P} -> {int(out[scene + '/dens_rows'])}, split draws {out[scene + '/split_z'].shape[0]}")
    np.savez_compressed(os.path.join(OUT, fname), **out)
    print("wrote", fname, os.path.getsize(os.path.join(OUT, fname)), "bytes")


if __name__ == "__main__":
    main()
    main("densify_nan.npz", poison=True)
    edges()
