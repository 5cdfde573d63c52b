"""The fused smoothness losses (csrc/smooth_loss.hip through svgir_harness.losses) on the cases of tests/smooth_cases.py against the fp64 oracle.

Losses: the kernels' sum / count (doubles, from `stats`) within 4 x E32 + n 2^-53 A of the oracle (E32 = |the reference's operation order in
fp32 - the oracle|, n elements of absolute sum A); the returned fp32 scalar is exactly float32(sum / count) (tv: of the sum of its two means);
where the bound is 0 -- the flat and masked-out cases -- the loss is exactly 0.  Counts: Cb H W; tv C (H-1) W and C H (W-1).  Gradients: per
element |kernel - oracle| <= 4 G32 eps32 max(Aabs, AABS_FLOOR) outside the threshold elements, finite inside them (smooth_cases.py holds the
definitions and the measured G32).  Every output buffer is NaN-filled first (tests/conftest.py sets SVGIR_POISON; the direct-ABI tests fill
their own), so an element the kernels forget shows."""
import numpy as np
import pytest
import torch

import smooth_cases as sc

pytestmark = pytest.mark.gpu
_id = lambda c: c["id"] if isinstance(c, dict) else str(c)   # noqa: E731
CASES = {c["id"]: c for c in sc.CASES}
UPSTREAM = (-1.7, 0.6, 2.0, 0.25)                            # per term of a launch: a negative one among them
FUSED = ("stage2-21x70", "sizes-150x161", "sizes-9x33", "sizes-1x1", "four-7x31", "flat-21x70")
_refs = {}


def _dev():
    return torch.device("cuda:0")


def refs(cid):
    """(terms, [oracle], [E32]) of a case, computed once and left unchanged."""
    if cid not in _refs:
        terms = sc.build(CASES[cid])
        o = [sc.oracle(t) for t in terms]
        e32 = [abs(sc.torch_eval(t, torch.float32)["loss"] - r["loss"]) for t, r in zip(terms, o)]
        _refs[cid] = (terms, o, e32)
    return _refs[cid]


def _leaves(terms, dev):
    """The terms as dicts of device tensors for smoothness_losses; arrays shared between terms become ONE tensor.  data always requires
    grad, an img where the case says so."""
    made = {}

    def put(a, grad):
        if a is None:
            return None
        if id(a) not in made:
            made[id(a)] = torch.from_numpy(a).to(dev)
        if grad:
            made[id(a)].requires_grad_(True)
        return made[id(a)]

    return [dict(kind=t["kind"], data=put(t["data"], True), img=put(t["img"], t["img_grad"]), data_mask=put(t["data_mask"], False),
                 img_mask=put(t["img_mask"], False)) for t in terms]


def _check_loss(name, scalar, st, kind, o, e32):
    with np.errstate(invalid="ignore", divide="ignore"):
        got = float(np.float64(st[0]) / np.float64(st[1]) + (np.float64(st[2]) / np.float64(st[3]) if kind == "tv" else 0.0))
    if np.isnan(o["loss"]):
        assert np.isnan(got) and np.isnan(scalar), name
        return
    tol = sc.loss_bound(o, e32)
    print(f"{name}: kernel {got!r}, oracle {o['loss']!r}, |difference| {abs(got - o['loss']):.3e}, E32 {e32:.3e}, bound {tol:.3e}")
    assert abs(got - o["loss"]) <= tol, (name, got, o["loss"], tol)
    assert np.float32(scalar) == np.float32(got), (name, scalar, got)


def _check_grad(name, got, ref, aabs, thr):
    got = got.detach().double().cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all(), name          # complete writes: no NaN of the poison is left, threshold elements included
    bound = 4 * sc.G32 * sc.EPS32 * np.maximum(aabs, sc.AABS_FLOOR)
    err = np.abs(got - ref)
    keep = ~thr
    worst = float((err[keep] / (sc.EPS32 * np.maximum(aabs[keep], sc.AABS_FLOOR))).max()) if keep.any() else 0.0
    print(f"{name}: max |difference| {err[keep].max() if keep.any() else 0.0:.3e}, max |oracle| {np.abs(ref).max():.3e}, worst error {worst:.2f} eps32 Aabs "
          f"(allowed {4 * sc.G32:.0f}), threshold elements {int(thr.sum())}")
    assert (err[keep] <= bound[keep]).all(), (name, worst)
    assert not got[(aabs == 0) & keep].any(), name                           # nothing contributes: exactly 0


@pytest.mark.parametrize("case", sc.CASES, ids=_id)
def test_losses_counts_and_gradients(built, case):
    from svgir_harness import losses
    dev = _dev()
    terms, o, e32 = refs(case["id"])
    lv = _leaves(terms, dev)
    out, stats = losses.smoothness_losses(lv, with_stats=True)
    assert out.shape == (len(terms),) and stats.shape == (len(terms), 4) and stats.dtype == torch.float64
    st = stats.cpu().numpy()
    for k, t in enumerate(terms):
        ca, cb = sc.counts(t)
        assert st[k, 1] == ca and st[k, 3] == cb and (t["kind"] == "tv" or st[k, 2] == 0), (k, st[k])
        _check_loss(f"{case['id']} term {k} {t['kind']}", float(out[k].detach()), st[k], t["kind"], o[k], e32[k])
    # backward: the upstream scalars are a device tensor; gradients of a shared img add up
    up = torch.tensor(UPSTREAM[:len(terms)], device=dev)
    (up * out).sum().backward()
    acc = {}
    for k, (t, l) in enumerate(zip(terms, lv)):
        for nm, leaf in (("data", l["data"]), ("img", l["img"] if t["img_grad"] else None)):
            if leaf is None:
                continue
            a = acc.setdefault(id(leaf), dict(leaf=leaf, ref=0.0, aabs=0.0, thr=False, name=f"{case['id']} d_{nm} of term {k}"))
            a["ref"] = a["ref"] + UPSTREAM[k] * o[k]["d_" + nm]
            a["aabs"] = a["aabs"] + abs(UPSTREAM[k]) * o[k]["aabs_" + nm]
            a["thr"] = a["thr"] | o[k]["thr_" + nm]
    for a in acc.values():
        _check_grad(a["name"], a["leaf"].grad, a["ref"], a["aabs"], a["thr"])
    for t, l in zip(terms, lv):
        if not t["img_grad"] and l["img"] is not None:
            assert l["img"].grad is None
    if case["id"].split("-")[0] in sc.NONFINITE:                               # the NaN is in the loss and in no gradient
        assert torch.isnan(out).all() and all(torch.isfinite(a["leaf"].grad).all() for a in acc.values())
    if case["id"].startswith("flat"):
        assert not out[:3].any() and not st[:3, 0].any()                      # exactly 0


def _raw_call(N, dev, terms, lv, W, H):
    """One forward + backward through the C ABI with every output NaN-filled; returns the buffers."""
    n = len(terms)
    nan = lambda shape, dtype=torch.float32: torch.full(shape, float("nan"), dtype=dtype, device=dev)   # noqa: E731
    partial, stats, lo = nan((N.lib.svgir_smooth_loss_partials(W, H, n), 2), torch.float64), nan((n, 4), torch.float64), nan((n,))
    grads = [(nan(tuple(l["data"].shape)), None if l["img"] is None else nan(tuple(l["img"].shape))) for l in lv]
    arr = (N.SmoothTerm * n)()
    for k, (t, l) in enumerate(zip(terms, lv)):
        d = arr[k]
        d.kind, d.C, d.Ci = sc.KINDS[t["kind"]], l["data"].shape[0], 0 if l["img"] is None else l["img"].shape[0]
        d.data, d.img, d.data_mask, d.img_mask = (None if l[nm] is None else l[nm].data_ptr() for nm in ("data", "img", "data_mask", "img_mask"))
    N.check(N.lib.svgir_smooth_loss_forward(W, H, n, arr, partial.data_ptr(), stats.data_ptr(), lo.data_ptr(), N.stream_ptr(dev)), "forward")
    for k, (gd, gi) in enumerate(grads):
        arr[k].d_data, arr[k].d_img = gd.data_ptr(), None if gi is None else gi.data_ptr()
    g = torch.tensor(UPSTREAM[:n], device=dev)
    N.check(N.lib.svgir_smooth_loss_backward(W, H, n, arr, stats.data_ptr(), g.data_ptr(), N.stream_ptr(dev)), "backward")
    return [partial, stats, lo] + [x for pair in grads for x in pair if x is not None]


@pytest.mark.parametrize("cid", FUSED)
def test_every_element_is_written_and_two_runs_give_the_same_bits(built, cid):
    from gaussian_renderer import _native as N
    dev = _dev()
    terms, o, _ = refs(cid)
    lv = _leaves(terms, dev)
    a = _raw_call(N, dev, terms, lv, CASES[cid]["W"], CASES[cid]["H"])
    b = _raw_call(N, dev, terms, lv, CASES[cid]["W"], CASES[cid]["H"])
    empty_tv = any(np.isnan(r["loss"]) for r in o)                              # (1 x 1: the tv means are empty, NaN by contract)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (cid, i)
        if i >= 3 or i == 0 or not empty_tv:
            assert not torch.isnan(x).any(), (cid, i)                           # every record, every gradient element: written


@pytest.mark.parametrize("cid", FUSED)
def test_fused_launch_equals_the_single_term_calls(built, cid):
    from svgir_harness import losses
    dev = _dev()
    terms, _, _ = refs(cid)
    up = torch.tensor(UPSTREAM[:len(terms)], device=dev)
    fl = _leaves(terms, dev)
    fused = losses.smoothness_losses(fl)
    sl = _leaves(terms, dev)
    single = torch.stack([losses.smoothness_losses([t])[0] for t in sl])
    assert torch.equal(fused.detach().view(torch.int32), single.detach().view(torch.int32))
    uniq = lambda lv: list({id(x): x for l in lv for x in (l["data"], l["img"]) if x is not None and x.requires_grad}.values())   # noqa: E731
    gf = torch.autograd.grad((up * fused).sum(), uniq(fl))
    gs = torch.autograd.grad((up * single).sum(), uniq(sl))
    assert len(gf) == len(gs) >= len(terms)
    for x, y in zip(gf, gs):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_drop_ins_against_the_fused_form(built):
    """A caller that multiplied by the mask itself (the reference's call form): the same losses within the bound -- the products are the
    same fp32 numbers -- and the gradients, which now pass through autograd's own mask product, within the gradient bound."""
    from svgir_harness import losses
    dev = _dev()
    terms, o, e32 = refs("mask_border-21x70")
    for k, (t, l) in enumerate(zip(terms, _leaves(terms, dev))):
        fn = losses.first_order_edge_aware_loss if t["kind"] == "first" else losses.second_order_edge_aware_loss
        data, img = l["data"], l["img"]
        loss = fn(data * l["data_mask"], img if l["img_mask"] is None else img * l["img_mask"])
        assert abs(float(loss.detach()) - o[k]["loss"]) <= sc.loss_bound(o[k], e32[k]) + 0.5 * float(np.spacing(np.float32(o[k]["loss"])))
        (UPSTREAM[k] * loss).backward()
        _check_grad(f"drop-in {k} d_data", data.grad, UPSTREAM[k] * o[k]["d_data"], abs(UPSTREAM[k]) * o[k]["aabs_data"], o[k]["thr_data"])
        if t["img_grad"]:
            _check_grad(f"drop-in {k} d_img", img.grad, UPSTREAM[k] * o[k]["d_img"], abs(UPSTREAM[k]) * o[k]["aabs_img"], o[k]["thr_img"])
    # tv_loss: [C,H,W], [H,W], and the reference's call form on a permuted environment map [H,W,3] (svgss.py:390-391)
    terms, o, e32 = refs("envmap-16x32")
    env = torch.from_numpy(terms[0]["data"]).to(dev)
    hw3 = env.permute(1, 2, 0).contiguous().requires_grad_(True)
    loss = losses.tv_loss(hw3.permute(2, 0, 1))
    assert loss.shape == () and abs(float(loss.detach()) - o[0]["loss"]) <= sc.loss_bound(o[0], e32[0]) + 0.5 * float(np.spacing(np.float32(o[0]["loss"])))
    loss.backward()
    _check_grad("tv d_env", hw3.grad.permute(2, 0, 1), o[0]["d_data"], o[0]["aabs_data"], o[0]["thr_data"])
    one = losses.tv_loss(env[0])
    assert torch.equal(one, losses.tv_loss(env[:1]))
    assert torch.isnan(losses.tv_loss(env[:, :1])) and torch.isnan(losses.tv_loss(env[0, :, :1]))


def test_gradients_reach_the_leaves_behind_other_torch_ops(built):
    from svgir_harness import losses
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    p = torch.randn(3, 21, 70, generator=g).to(dev).requires_grad_(True)
    q = torch.randn(3, 21, 70, generator=g).to(dev).requires_grad_(True)
    mask = (torch.rand(1, 21, 70, generator=g) > 0.3).float().to(dev)
    data, img = torch.sigmoid(p), torch.nn.functional.normalize(q, dim=0)
    term = dict(kind="first", data=data, img=img, data_mask=mask)
    loss = 0.3 * losses.smoothness_losses([term, dict(kind="tv", data=data)]).sum() + 0.1 * data.mean()
    loss.backward()
    assert torch.isfinite(p.grad).all() and torch.isfinite(q.grad).all() and p.grad.any() and q.grad.any()
    # the same through detached leaves and an explicit chain
    d0, i0 = data.detach().requires_grad_(True), img.detach().requires_grad_(True)
    (0.3 * losses.smoothness_losses([dict(term, data=d0, img=i0), dict(kind="tv", data=d0)]).sum() + 0.1 * d0.mean()).backward()
    gp, = torch.autograd.grad(torch.sigmoid(p), p, d0.grad)
    gq, = torch.autograd.grad(torch.nn.functional.normalize(q, dim=0), q, i0.grad)
    assert torch.allclose(p.grad, gp, rtol=1e-6, atol=1e-12) and torch.allclose(q.grad, gq, rtol=1e-6, atol=1e-12)
    # an img that does not require grad gets none, and costs no gradient buffer
    d1 = data.detach().requires_grad_(True)
    losses.first_order_edge_aware_loss(d1, img.detach()).backward()
    assert d1.grad is not None and torch.isfinite(d1.grad).all()
    with pytest.raises(RuntimeError, match="gets no gradient"):
        losses.smoothness_losses([dict(term, data_mask=mask.clone().requires_grad_(True))])
