"""csrc/optim.hip through svgir_harness/optim.py (`FusedAdam`, `add_densification_stats`, `prune_rows`, `_scan`, `append_rows`,
`DensifyState._masks` / `densify_and_split` / `densify_and_prune` / `prune`) held to the optimizer case table (tests/optim_cases.py;
tests/test_optim_edge_inputs.py proves the table and pins the oracle on the CPU).

The rule, case for case: row movement, masks, kept lists, counts and step counts are compared on raw bits; arithmetic outputs with
the bounds of tests/test_gpu_optim.py (`optim_cases.same`: NaN / inf pattern exact, 2e-6 / 3e-6 / 4e-6 of the tensor's scale).  No
mask row is excused: the table holds no comparison that is undecidably close to its threshold (the host test asserts it).  The suite
runs with SVGIR_POISON=1, so every gathered / appended tensor, both masks, the kept list and the count start as NaN / -7: a word the
kernels forget shows.  Entries of the kept list beyond the count are not promised and not compared.
"""
import numpy as np
import pytest
import torch

from oracle import optim_oracle as oo
from tests import optim_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(x):
    """raw words of a tensor or array (NaNs compare by their bits, -0 differs from +0)"""
    a = x.detach().contiguous().cpu().numpy() if hasattr(x, "detach") else np.ascontiguousarray(x)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, exp, what):
    g, e = bits(got), bits(exp)
    assert g.shape == e.shape, (what, g.shape, e.shape)
    assert np.array_equal(g, e), f"{what}: {int((g != e).sum())} of {g.size} words differ, first at {np.argwhere(g != e)[:4].tolist()}"


def test_outputs_are_poisoned(built):
    from gaussian_renderer import _native as N
    assert N.POISON and float(N.out_tensor(1, torch.uint8, DEV)[0]) == 249 and int(N.out_tensor(1, torch.int32, DEV)[0]) == -7


# ---- Adam --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oc.ADAM))
def test_adam_case(built, name):
    from svgir_harness.optim import FusedAdam
    c = oc.ADAM[name]()
    e = oc.adam_expected(name)
    # the magnitude classes are arbitrated by torch's own fp32 Adam on the CPU (the oracle agrees with it: host test)
    arb = oc.adam_torch(name, torch.float32) if c["arbiter"] == "torch32" else e
    ps = [torch.nn.Parameter(t(a)) for a in c["params"]]
    opt = FusedAdam([{"params": [p], "lr": lr, "name": n} for p, lr, n in zip(ps, c["lrs"], c["names"])], lr=1e-4, eps=oc.EPS)
    for p, s in zip(ps, c["state"]):
        if s is not None:
            opt.state[p] = {"step": torch.tensor(float(s[0])), "exp_avg": t(s[1]), "exp_avg_sq": t(s[2])}
    held = None
    for gs in c["grads"]:
        for p, g in zip(ps, gs):
            p.grad = t(g)
        held = [p.grad for p in ps]
        opt.step(nan_values=c["nan_values"], zero_grad=c["zero_grad"])
    for i, p in enumerate(ps):
        what = f"{name} tensor {i} (n = {c['sizes'][i]})"
        assert float(opt.state[p]["step"]) == arb["t"][i] == e["t"][i], what
        oc.same(p, arb["p"][i], what + " param")
        oc.same(opt.state[p]["exp_avg"], arb["m"][i], what + " exp_avg")
        oc.same(opt.state[p]["exp_avg_sq"], arb["v"][i], what + " exp_avg_sq", oc.TOL_EXP_AVG_SQ)
        # the gradient tensor as the step leaves it: zeros (fill), the scrubbed values (scrub), or untouched
        assert p.grad is held[i]
        same_bits(held[i], oo.f32(e["grad_left"][i]), what + " gradient left behind")
        if c["lrs"][i] == 0.0:
            same_bits(p, c["params"][i], what + " lr = 0")


# ---- mask scan and compaction ------------------------------------------------------------------------------------------------------------
def _upload_rows(rows):
    out = []
    for what, a in rows:
        if a.flags["C_CONTIGUOUS"]:
            out.append(t(a))
        else:       # the same values behind a stride: every second column of a twice as wide tensor
            d = t(np.repeat(np.ascontiguousarray(a), 2, axis=1))[:, ::2]
            assert not d.is_contiguous() and np.array_equal(d.cpu().numpy(), a)
            out.append(d)
    return out


@pytest.mark.parametrize("P", oc.MASK_P)
def test_mask_scan_and_compaction(built, P):
    from svgir_harness import optim as O
    rows = oc.row_tensors(P)
    dev = _upload_rows(rows)
    for shape in oc.MASK_SHAPES:
        m = oc.mask(P, shape)
        keep = t(m)
        kept, count, n = O._scan(keep)
        exp = np.flatnonzero(m).astype(np.int32)                       # torch.nonzero
        assert n == exp.size and int(count.item()) == exp.size, (P, shape, n, exp.size)
        same_bits(kept[:n], exp, f"P = {P} {shape}: kept list")
        outs = O.prune_rows(dev, keep)
        for (what, a), o in zip(rows, outs):
            assert o.dtype == torch.from_numpy(a[:0].copy()).dtype and o.is_contiguous()
            same_bits(o, a[m], f"P = {P} {shape}: {what}")                 # t[mask]


def test_compaction_of_more_tensors_than_one_launch_takes(built):
    from svgir_harness import optim as O
    P = oc.MANY_TENSORS_P
    rows = oc.row_tensors(P, many=True)
    assert len(rows) > O.MAX_TENSORS
    for shape in ("random_0.5", "block_edge", "all"):
        m = oc.mask(P, shape)
        for (what, a), o in zip(rows, O.prune_rows([t(a) for _, a in rows], t(m))):
            same_bits(o, a[m], f"{shape}: {what}")


def test_rows_that_are_no_multiple_of_4_bytes_are_refused(built):
    from svgir_harness import optim as O
    P = 9
    keep = t(oc.mask(P, "alternating"))
    for bad in (torch.zeros(P, 1, dtype=torch.float16, device=DEV), torch.zeros(P, dtype=torch.uint8, device=DEV),
                torch.zeros(P, 3, dtype=torch.float16, device=DEV)):
        with pytest.raises(ValueError):
            O.prune_rows([torch.zeros(P, 3, device=DEV), bad], keep)
        lst, cnt, n = O._scan(keep)
        with pytest.raises(ValueError):
            O.append_rows([bad], lst, cnt, n)
    assert O.prune_rows([torch.zeros(P, 2, dtype=torch.float16, device=DEV)], keep)[0].shape == (4, 2)      # 4 bytes a row: accepted


# ---- append ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,sel,repeat", oc.APPEND, ids=lambda v: str(v))
def test_append_case(built, P, sel, repeat):
    from svgir_harness import optim as O
    m = oc.append_selection(P, sel)
    tensors = oc.append_tensors(P)
    lst, cnt, n = O._scan(t(m))
    assert n == int(m.sum())
    outs = O.append_rows([t(a) for _, a, _ in tensors], lst, cnt, n, repeat=repeat, zero_new={i for i, x in enumerate(tensors) if x[2]})
    ms = torch.from_numpy(m)
    for (what, a, zero_new), o in zip(tensors, outs):
        ta = torch.from_numpy(a)
        new = ta[ms].repeat(repeat, *([1] * (ta.dim() - 1)))                  # the arbiter: Tensor.repeat's order
        exp = torch.cat((ta, torch.zeros_like(new) if zero_new else new))
        same_bits(o, exp.numpy(), f"P = {P}, {sel} x {repeat}: {what}")
        same_bits(o, oo.append_rows(a, m, repeat, zero_new), f"P = {P}, {sel} x {repeat}: {what} (oracle)")


# ---- statistics --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", oc.STATS, ids=lambda c: f"P{c[0]}-stride{c[1]}-{'w' if c[2] else 'now'}-{c[3]}")
def test_stats_case(built, case):
    from svgir_harness.optim import add_densification_stats
    c = oc.stats_case(*case)
    exp = oo.add_densification_stats(c["vgrad"], c["filter"], c["weights"], *c["accum"])
    acc = [t(a) for a in c["accum"]]
    add_densification_stats(t(c["vgrad"]), t(c["filter"]), None if c["weights"] is None else t(c["weights"]), *acc)
    out = ~c["filter"]
    for a, b, a0, what in zip(acc, exp, c["accum"], ("weights_accum", "xyz_gradient_accum", "denom")):
        a = a.cpu().numpy()
        assert np.isfinite(a).all() and np.allclose(a.astype(np.float64), b, rtol=2e-7, atol=0), (case, what)
        if what != "weights_accum":       # a row outside the filter is untouched, whatever its gradient holds
            same_bits(a[out], a0[out], f"{case} {what} outside the filter")
        elif c["weights"] is None:
            same_bits(a, a0, f"{case} weights_accum without weights")


# ---- split transform ---------------------------------------------------------------------------------------------------------------------
def _state(params, spec, use_pbr):
    from svgir_harness.optim import DensifyState, FusedAdam
    ps = {n: torch.nn.Parameter(t(params[n])) for n, _, _ in spec}
    opt = FusedAdam([{"params": [ps[n]], "lr": lr, "name": n} for n, _, lr in spec], lr=1e-4, eps=oc.EPS)
    return DensifyState(ps, opt, percent_dense=0.01, use_pbr=use_pbr)


def _snapshot(st, names):
    s = dict(params={}, m={}, v={}, t={}, book={k: getattr(st, k) for k in oc.BOOK})
    for n in names:
        p = st.params[n]
        state = st.optimizer.state.get(p, None)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and st.optimizer.param_groups[names.index(n)]["params"][0] is p
        s["params"][n] = p
        s["m"][n], s["v"][n] = (state["exp_avg"], state["exp_avg_sq"]) if state else (None, None)
        s["t"][n] = int(state["step"]) if state else -1
    return s


def _moved_exactly(before, got, e, names, what):
    """every row that densification only MOVED holds the bits it held before: parameters (but the computed xyz / scaling of split
    children), both moments (zero for new rows)"""
    origin, fresh, child = e["origin"], e["fresh"], e["child"]
    for n in names:
        rows = ~child if n in ("xyz", "scaling") else np.ones(origin.size, dtype=bool)
        same_bits(got["params"][n].detach().cpu().numpy()[rows], before["params"][n][origin[rows]], f"{what}: moved rows of {n}")
        for k in ("m", "v"):
            if before[k][n] is not None:
                exp = before[k][n][origin]
                exp[fresh] = 0.0
                same_bits(got[k][n], exp, f"{what}: {k} of {n}")


def _host(s):
    return {k: {n: (None if x is None else x.detach().cpu().numpy().copy()) for n, x in s[k].items()} for k in ("params", "m", "v")}


@pytest.mark.parametrize("case", oc.SPLIT, ids=lambda c: f"{c[0]}x{c[1]}")
def test_split_case(built, case):
    c, e = oc.split_case(*case), oc.split_expected(*case)
    names = [n for n, _, _ in oc.SPLIT_SPEC]
    st = _state(c["params"], oc.SPLIT_SPEC, False)
    before = _host(_snapshot(st, names))
    n = st.densify_and_split(t(c["sel"]), c["N"], z=t(c["z"]))
    assert n == case[0]
    got = _snapshot(st, names)
    oc.same_xyz(got["params"]["xyz"], e["params"]["xyz"], f"split {case} xyz", oc.TOL_DENSIFIED)
    oc.same_scaling(got["params"]["scaling"], e["params"]["scaling"], f"split {case} scaling", oc.TOL_DENSIFIED)
    _moved_exactly(before, got, e, names, f"split {case}")
    for k in oc.BOOK:
        oc.same(got["book"][k], e["book"][k], f"split {case} {k}")


# ---- the densification sequence, scene by scene ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", oc.scene_names())
def test_densify_scene(built, scene):
    c, e = oc.scene_inputs(scene), oc.scene_expected(scene)
    st = _state(c["init"], oc.SPEC, True)
    for gr in c["grads"]:
        for n in oc.NAMES:
            st.params[n].grad = None if gr[n] is None else t(gr[n])
        st.step()
        assert all(st.params[n].grad is None for n in oc.NAMES)
    for k in oc.BOOK:
        setattr(st, k, t(c["stat"][k]))
    before = _host(_snapshot(st, oc.NAMES))
    a = c["args"]
    if c["op"] == "prune":
        st.prune(a["min_opacity"], a["extent"], a["max_screen_size"], weights_threshold=1e-5)
    else:
        clone, split = st._masks(a["max_grad"], a["extent"], a["max_grad_normal"], raw=True)
        assert clone.dtype == torch.uint8 and split.dtype == torch.uint8
        same_bits(clone, e["clone"].astype(np.uint8), f"{scene}: clone mask")
        same_bits(split, e["split"].astype(np.uint8), f"{scene}: split mask")
        st.densify_and_prune(a["max_grad"], a["min_opacity"], a["extent"], a["max_screen_size"], a["max_grad_normal"], z=t(c["z"]))
    got = _snapshot(st, oc.NAMES)
    oc.compare_snapshot(got, e["dens"], f"{scene} after {c['op']}")
    _moved_exactly(before, got, e["dens"], oc.NAMES, scene)
    # ---- one more step() on the new block (P = 0 included) ----
    for n in oc.NAMES:
        st.params[n].grad = t(c["post_grad"][n])
    st.step()
    oc.compare_snapshot(_snapshot(st, oc.NAMES), e["post"], f"{scene} after the next step", densified=True)
