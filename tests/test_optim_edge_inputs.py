"""The optimizer case table (tests/optim_cases.py) proved on the CPU oracle alone (oracle/optim_oracle.py): every case reaches the edge
it is named for, no mask comparison sits undecidably close to its threshold, and the oracle is pinned from outside the project -- by
the reference's own methods (tests/golden/densify.npz, densify_nan.npz, densify_edges.npz) and by torch.optim.Adam on the CPU.
Run with -s for the figures.

Nothing here is built to fault: P = 0, empty tensors and NaN / inf values only change floats and counts; no loop of csrc/optim.hip has
a trip count that depends on a float, and every index is bounded by a row count the host computed.
"""
import numpy as np
import pytest
import torch

from oracle import optim_oracle as oo
from tests import optim_cases as oc

F32 = np.float32


# ---- the oracle against the reference's methods ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", ["densify.npz", "densify_nan.npz"])
def test_oracle_reproduces_the_reference_fixture(fixture):
    """three step()s with NaN-poisoned gradients (one group without a gradient once), then densify_and_prune, as the reference ran them"""
    g = oc.gold(fixture)
    m = oo.Model({n: g["init_" + n] for n in oc.NAMES}, oc.LRS, eps=oc.EPS)
    for it in range(3):
        m.step({n: (g[f"grad{it}_{n}"] if g[f"grad{it}_{n}"].size else None) for n in oc.NAMES})
    for n in oc.NAMES:
        oc.same(m.params[n], g["step_" + n], "step " + n)
        oc.same(m.state[n]["exp_avg"], g["step_m_" + n], "step m " + n)
        oc.same(m.state[n]["exp_avg_sq"], g["step_v_" + n], "step v " + n, oc.TOL_EXP_AVG_SQ)
    for k in oc.BOOK:
        setattr(m, k, np.array(g["stat_" + k], dtype=np.float64))
    max_grad, min_opacity, extent, max_screen, max_grad_normal = [float(x) for x in g["densify_args"]]
    m.densify_and_prune(max_grad, min_opacity, extent, max_screen, max_grad_normal, z=g["split_z"])
    for n in oc.NAMES:
        (oc.same_scaling if n == "scaling" else oc.same_xyz if n == "xyz" else oc.same)(m.params[n], g["dens_" + n], "densify " + n, oc.TOL_DENSIFIED)
        oc.same(m.state[n]["exp_avg"], g["dens_m_" + n], "densify m " + n)
        oc.same(m.state[n]["exp_avg_sq"], g["dens_v_" + n], "densify v " + n, oc.TOL_EXP_AVG_SQ)
    for k in oc.BOOK:
        oc.same(getattr(m, k), g["dens_" + k], "densify " + k)
    print(f"{fixture}: {g['init_xyz'].shape[0]} -> {m.P} rows, {len(oc.near_threshold(m.compared, False))} comparisons near a threshold")


@pytest.mark.parametrize("scene", oc.scene_names())
def test_oracle_reproduces_the_reference_scene(scene):
    e = oc.scene_expected(scene)
    for tag in ("dens", "post"):
        oc.compare_snapshot(e[tag], oc.scene_reference(scene, tag), f"{scene} {tag}")


EXPECTED_ROWS = {"nothing": 1.0, "all_clone": 2.0, "all_clone_thr0": 2.0, "all_split": 2.0, "all_split_noscreen": 2.0, "all_split_thr0": 2.0,
                 "all_pruned": 0.0, "all_split_all_pruned": 0.0}


@pytest.mark.parametrize("scene", oc.scene_names())
def test_scene_reaches_its_edge(scene):
    c, e = oc.scene_inputs(scene), oc.scene_expected(scene)
    P, Pd = c["init"]["xyz"].shape[0], e["dens"]["params"]["xyz"].shape[0]
    clone, split, pruned = e["clone"], e["split"], e["pruned"]
    print(f"{scene}: {P} -> {Pd} rows; clone {None if clone is None else int(clone.sum())}, split {None if split is None else int(split.sum())}, "
          f"pruned {int(pruned.sum())}")
    # ---- the threshold-row condition: a tie by construction or clear of the threshold ----
    assert oc.near_threshold(e["compared"], scene in oc.TIE_SCENES) == []
    base = scene.rsplit("_p", 1)[0]
    if base in EXPECTED_ROWS:
        assert Pd == EXPECTED_ROWS[base] * P and P in (1, 5)
        if "split" in base:
            assert split.all() and not clone.any()
        elif "clone" in base:
            assert clone.all() and not split.any()
        elif base == "nothing":
            assert not clone.any() and not split.any() and not pruned.any()
    st = c["stat"]
    if scene.startswith("empty"):
        assert P == 0 and Pd == 0 and e["post"]["params"]["f_rest"].shape == (0, 15, 3)
    if scene in ("negative_accum", "negative_normal_accum"):
        # the selection on the norm passes, the row is big, the signed test fails: untouched (|g| for both would split every row)
        acc = st["xyz_gradient_accum"] if scene == "negative_accum" else st["normal_gradient_accum"]
        assert (acc[:, 0] < 0).any() and Pd == P and not clone.any() and not split.any() and not pruned.any()
        fabs_rule = oo.selection_masks(np.abs(st["xyz_gradient_accum"]), np.abs(st["normal_gradient_accum"]), np.abs(st["denom"]),
                                       c["init"]["scaling"], c["args"]["max_grad"], c["args"]["max_grad_normal"], 0.01 * c["args"]["extent"])[1]
        assert fabs_rule.all()
    if scene == "tie_size":
        s, lim = oo.max_scale32(e["dens"]["params"]["scaling"][:P]), F32(0.01 * c["args"]["extent"])
        assert (s == lim).sum() == 2 and lim == 1.0 and clone[s == lim].all() and not split.any()
    if scene == "nan_scale_at_limit":
        nan = np.isnan(c["init"]["scaling"]).all(axis=1)
        assert nan.sum() == 2 and F32(0.01 * c["args"]["extent"]) == F32(1e-6) and clone[nan].all() and split[~nan].all()
    if scene == "tie_grad":
        g, gn = oo.mean_grads(st["xyz_gradient_accum"], st["denom"]), oo.mean_grads(st["normal_gradient_accum"], st["denom"])
        assert (g == F32(c["args"]["max_grad"])).sum() == 2 and (gn == F32(c["args"]["max_grad_normal"])).sum() == 1 and clone.sum() == 3
    if scene == "denom0_positive":
        assert np.isinf(oo.mean_grads(st["xyz_gradient_accum"], st["denom"])).sum() == 2 and clone.sum() == 1 and split.sum() == 1
    if scene == "denom0_zero":
        with np.errstate(all="ignore"):
            assert np.isnan(st["xyz_gradient_accum"] / st["denom"]).all() and not clone.any() and not split.any()
    if scene in ("no_state", "mixed_no_state"):
        assert all(t == -1 for t in e["dens"]["t"].values()) and all(t == 1 for t in e["post"]["t"].values()) and Pd > P
    if scene == "one_group_no_state":
        assert e["dens"]["t"]["incidents_rest"] == -1 and e["dens"]["t"]["xyz"] == 1 and e["post"]["t"]["incidents_rest"] == 1 and Pd == 2 * P
    if scene == "mixed_two_steps_one_group_skipped":
        assert e["dens"]["t"]["visibility_rest"] == -1 and e["dens"]["t"]["xyz"] == 2
    if scene.startswith("mixed"):
        # a few rows of each kind: cloned, split, pruned and left alone; a zero quaternion and a flat row among the split ones
        assert clone.sum() >= 5 and split.sum() >= 5 and pruned.sum() >= 3 and (~clone & ~split).sum() >= 5
        assert (np.abs(c["init"]["rotation"][split]).sum(axis=1) == 0).sum() == 1 and (c["init"]["scaling"][split, 2] == F32(-1e10)).sum() == 1
        d = e["dens"]
        assert d["child"].sum() >= 8 and np.isnan(d["params"]["xyz"][d["child"]]).any() and d["fresh"].sum() > d["child"].sum()
    if scene.startswith("prune"):
        assert clone is None and Pd < P


def test_the_table_names_every_scene_of_the_issue():
    names = set(oc.scene_names())
    for base in EXPECTED_ROWS:
        assert {base + "_p1", base + "_p5"} <= names
    assert {"empty", "negative_accum", "tie_size", "nan_scale_at_limit", "tie_grad", "denom0_positive", "denom0_zero", "no_state",
            "one_group_no_state", "mixed"} <= names


# ---- Adam --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oc.ADAM))
def test_adam_case_and_oracle_against_torch(name):
    """values: torch.optim.Adam in fp64 on the CPU; finiteness class of every element: the same optimizer in fp32"""
    c, e = oc.ADAM[name](), oc.adam_expected(name)
    t64, t32 = oc.adam_torch(name, torch.float64), oc.adam_torch(name, torch.float32)
    chunks, launches = oc.adam_geometry(c)
    print(f"{name}: {len(c['sizes'])} tensors, chunks {chunks[:12]}, launches {max(launches) + 1}; {c['edge']}")
    assert e["t"] == t64["t"] == t32["t"]
    for i in range(len(c["sizes"])):
        for k, tol in (("p", oc.TOL), ("m", oc.TOL), ("v", oc.TOL_EXP_AVG_SQ)):
            assert np.array_equal(oc.finiteness_class(e[k][i]), oc.finiteness_class(t32[k][i])), (name, i, k)
            if c["arbiter"] == "torch32":     # (fp64 torch keeps finite what overflows fp32, and goes another way from there)
                oc.same(e[k][i], t32[k][i].astype(np.float64), f"{name} {k}[{i}] oracle vs fp32 torch", tol)
            else:
                oc.same(e[k][i], t64[k][i], f"{name} {k}[{i}] oracle vs fp64 torch", 1e-12)
    # ---- the edge the case is named for ----
    if name == "chunk_sizes":
        assert tuple(c["sizes"]) == oc.ADAM_SIZES and sorted(set(chunks)) == [1, 2, 4] and chunks[c["sizes"].index(4096)] == 1 and \
            chunks[c["sizes"].index(4097)] == 2 and chunks[c["sizes"].index(8192)] == 2 and min(c["sizes"]) < 256
    if name == "table_of_32":
        assert len(c["sizes"]) == oo.MAX_TENSORS and max(launches) == 0 and c["sizes"].count(1) >= 3 and c["sizes"][-1] == 1
    if name == "table_of_40":
        assert len(c["sizes"]) == 40 and launches.count(0) == 32 and launches.count(1) == 8 and 1 in c["sizes"][32:] and 1 in c["sizes"][:32]
    if name == "empty_tensor_between":
        assert c["sizes"][1] == 0 and e["t"] == [2, 2, 2]
    if name == "step_counts":
        assert e["t"][:4] == [1, 2, 1000, 100000] and c["lrs"][4] == 0.0 and np.array_equal(e["p"][4], c["params"][4].astype(np.float64))
    if name == "gradient_magnitudes":
        g = c["grads"][0][0][:len(oc.MAGNITUDES)]
        v = e["v"][0][:len(oc.MAGNITUDES)]
        at = lambda x: int(np.flatnonzero(g == F32(x))[0])
        assert np.isfinite(v[at(1e20)]) and abs(v[at(1e20)] / 1.999e37 - 1) < 1e-3 and v[at(5e20)] == np.inf and v[at(1e21)] == np.inf
        with np.errstate(all="ignore"):
            assert np.isinf(F32(0.001) * (F32(1e20) * F32(1e20))) and np.isfinite((F32(0.001) * F32(1e20)) * F32(1e20))
        assert sorted(set(oc.finiteness_class(e["p"][0]))) == [0, 3] and sorted(set(oc.finiteness_class(e["v"][0]))) == [0, 1, 3]
        assert sorted(set(oc.finiteness_class(e["m"][0]))) == [0, 3]      # (an infinite gradient: inf after one step, inf - inf after two)
    if name.startswith("scrub"):
        nan_in = [np.isnan(g) for g in c["grads"][-1]]
        assert all(n.any() for n in nan_in)
        assert np.isnan(e["p"][1]).any() and not np.isnan(e["p"][0]).any() and not np.isnan(e["p"][2]).any()     # group b is not scrubbed
        if c["zero_grad"] == "fill":
            assert all((gl == 0).all() for gl in e["grad_left"])
        else:
            assert (e["grad_left"][0][nan_in[0]] == 0.375).all() and (e["grad_left"][2][nan_in[2]] == 0.0).all() and np.isnan(e["grad_left"][1]).any()
        # a wrong table column (another group's replacement, or 0) moves the result by more than the bound
        wrong = oo.adam_step(c["params"][0], c["grads"][0][0], np.zeros(300), np.zeros(300), 1, c["lrs"][0], eps=oc.EPS, nan_value=0.0)
        right = oo.adam_step(c["params"][0], c["grads"][0][0], np.zeros(300), np.zeros(300), 1, c["lrs"][0], eps=oc.EPS, nan_value=0.375)
        assert np.abs(wrong[1] - right[1]).max() > 100 * oc.TOL * np.abs(right[1]).max()


# ---- mask scan, compaction, append -------------------------------------------------------------------------------------------------------
def test_mask_sizes_reach_the_scan_edges():
    blocks = {P: oc.scan_blocks(P) for P in oc.MASK_P}
    trips = {P: oc.block_sum_trips(P) for P in oc.MASK_P}
    print("blocks", blocks, "block-sum trips", trips)
    assert [blocks[P] for P in (2047, 2048, 2049, 4096, 6145)] == [1, 1, 2, 2, 4]
    assert blocks[526337] == 258 and blocks[528389] == 259 and trips[526337] == 2 and trips[528389] == 2 and trips[6145] == 1
    assert max(blocks.values()) > oo.SCAN_BLOCK      # the strided loop takes its second trip
    for P in oc.MASK_P:
        for shape in oc.MASK_SHAPES:
            m = oc.mask(P, shape)
            assert m.shape == (P,) and m.dtype == bool
        assert oc.mask(P, "all").all() and not oc.mask(P, "none").any()
        assert oc.mask(P, "first").sum() == 1 and oc.mask(P, "first")[0] and oc.mask(P, "last").sum() == 1 and oc.mask(P, "last")[-1]
        if blocks[P] >= 2:
            assert np.flatnonzero(oc.mask(P, "block_edge")).tolist() == [2047, 2048]
            per_block = np.add.reduceat(oc.mask(P, "one_block").astype(int), np.arange(0, P, 2048))
            assert (per_block > 0).sum() == 1 and per_block[1] == min(2048, P - 2048)
            per_block = np.add.reduceat(oc.mask(P, "one_empty_block").astype(int), np.arange(0, P, 2048))
            assert (per_block == 0).sum() == 1 and per_block[1] == 0
            assert oc.mask(P, "every_2048").sum() == P // 2048
    widths = sorted({int(np.prod(a.shape[1:])) for _, a in oc.row_tensors(2049)})
    assert widths == [1, 3, 4, 12, 45] and any(a.dtype == np.int32 and a.ndim == 1 for _, a in oc.row_tensors(2049))
    assert any(not a.flags["C_CONTIGUOUS"] for _, a in oc.row_tensors(2049))
    assert len(oc.row_tensors(oc.MANY_TENSORS_P, many=True)) > oo.MAX_TENSORS
    assert max(a.nbytes for P in oc.MASK_P for _, a in oc.row_tensors(P)) < 8 << 20       # the big sizes carry narrow tensors only


def test_append_cases_reach_their_edges():
    new = [(P, int(oc.append_selection(P, sel).sum()) * r) for P, sel, r in oc.APPEND]
    print("(rows, new rows):", new)
    assert {r for _, _, r in oc.APPEND} == {1, 2, 3}
    for edge in (256, 2048):
        assert {P for P, _ in new} >= {edge - 1, edge, edge + 1}
        assert any(n < edge for _, n in new) and any(n == edge for _, n in new) and any(n > edge for _, n in new)
        assert {edge - 1, edge, edge + 1} & {n for _, n in new} >= {edge}
    assert {255, 256, 258} <= {n for _, n in new} and {2047, 2048, 2049} <= {n for _, n in new}
    assert any(P == 0 for P, _ in new) and any(n == 0 and P > 0 for P, n in new) and any(n == r for (P, n), (_, _, r) in zip(new, oc.APPEND) if P > 1)
    assert any(sel == "last" for _, sel, _ in oc.APPEND) and any(sel == "all" and r == 3 for _, sel, r in oc.APPEND)
    words = [w for _, w, _, _ in oc.APPEND_TENSORS]
    assert 45 in words and 1 in words and any(z and w == 45 for _, w, _, z in oc.APPEND_TENSORS) and any(z and w == 1 for _, w, _, z in oc.APPEND_TENSORS)
    # the order of Tensor.repeat: the whole selection, then the whole selection again
    t = torch.arange(12.0).reshape(4, 3)
    sel = np.array([True, False, True, True])
    for r in (1, 2, 3):
        assert np.array_equal(oo.append_rows(t.numpy(), sel, r), torch.cat((t, t[torch.from_numpy(sel)].repeat(r, 1))).numpy())


# ---- statistics --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", oc.STATS, ids=lambda c: f"P{c[0]}-stride{c[1]}-{'w' if c[2] else 'now'}-{c[3]}")
def test_stats_oracle_against_the_reference_statements(case):
    c = oc.stats_case(*case)
    wa, ga, dn = (torch.from_numpy(a.copy()) for a in c["accum"])
    vg, flt = torch.from_numpy(c["vgrad"]), torch.from_numpy(c["filter"])
    if c["weights"] is not None:
        wa += torch.from_numpy(c["weights"])
    ga[flt] += torch.norm(vg[flt, :2], dim=-1, keepdim=True)
    dn[flt] += 1
    got = oo.add_densification_stats(c["vgrad"], c["filter"], c["weights"], *c["accum"])
    for a, b in zip(got, (wa, ga, dn)):
        assert np.isfinite(a).all() and np.allclose(a, b.numpy().astype(np.float64), rtol=2e-7, atol=0)
    out = ~c["filter"]
    assert np.array_equal(got[1][out], c["accum"][1][out].astype(np.float64)) and np.array_equal(got[2][out], c["accum"][2][out].astype(np.float64))
    if case[3] != "all" and case[0] > 1:
        assert np.isnan(c["vgrad"][out, :2]).any()
    assert {s for _, s, _, _ in oc.STATS} == {2, 3, 4} and {P for P, _, _, _ in oc.STATS} == {1, 255, 256, 257, 513}


# ---- split transform ---------------------------------------------------------------------------------------------------------------------
def _reference_split_fp32(c):
    """the reference's statements for the new points (scene/gaussian_model.py:1152-1160), in torch fp32 on the CPU"""
    t = {n: torch.from_numpy(a) for n, a in c["params"].items()}
    sel, N = torch.from_numpy(c["sel"]), c["N"]
    act = lambda x: torch.nan_to_num(torch.exp(x), nan=1e-6)
    stds = act(t["scaling"])[sel].repeat(N, 1)
    samples = stds * torch.from_numpy(c["z"])
    q = t["rotation"][sel]
    q = q / torch.sqrt((q * q).sum(dim=1, keepdim=True))
    r, x, y, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + w * w), 2 * (x * y - r * w), 2 * (x * w + r * y), 2 * (x * y + r * w), 1 - 2 * (x * x + w * w),
                     2 * (y * w - r * x), 2 * (x * w - r * y), 2 * (y * w + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3).repeat(N, 1, 1)
    xyz = torch.bmm(R, samples.unsqueeze(-1)).squeeze(-1) + t["xyz"][sel].repeat(N, 1)
    sc = torch.log(stds / (0.8 * N))
    sc[:, -1] = -1e10
    return xyz.numpy(), sc.numpy()


@pytest.mark.parametrize("case", oc.SPLIT, ids=lambda c: f"{c[0]}x{c[1]}")
def test_split_transform_fp32_error(case):
    """The error of the reference's own fp32 arithmetic against the fp64 oracle on the split cases (extreme scales included): the
    figure behind `no new bound is needed` in tests/optim_cases.py.  4 x it must fit the bound the GPU test uses."""
    c, e = oc.split_case(*case), oc.split_expected(*case)
    n_new = case[0] * case[1]
    assert int(e["child"].sum()) == n_new and e["params"]["xyz"].shape[0] == oc.SPLIT_P - case[0] + n_new
    xyz, sc = _reference_split_fp32(c)
    ex = oc.same_xyz(xyz, e["params"]["xyz"][e["child"]], "xyz of the new points", oc.TOL_DENSIFIED / 4)
    es = oc.same_scaling(sc, e["params"]["scaling"][e["child"]], "scaling of the new points", oc.TOL_DENSIFIED / 4)
    print(f"split {case}: fp32 reference vs fp64 oracle, relative to the tensor's scale: xyz {ex:.2e}, scaling {es:.2e}")
    if case[0] >= 5:
        ch = e["params"]
        assert np.isnan(ch["xyz"][e["child"]]).any() and np.isinf(ch["xyz"][e["child"]]).any()
        assert len(c["special"]) == 5 and (c["params"]["scaling"][c["sel"], 2] == F32(-1e10)).sum() == 1
    # the rows that are not new are moved, not computed
    keep = ~c["sel"]
    assert np.array_equal(e["params"]["xyz"][~e["child"]], c["params"]["xyz"][keep].astype(np.float64))
