"""CPU restatement of the optimizer stage (csrc/optim.hip + svgir_harness/optim.py), test infrastructure only: plain NumPy,
fp64 for values, fp32 for everything a comparison decides.

What it restates (scene/gaussian_model.py of the reference, by method name):
  adam_step                -- torch.optim.Adam's single-tensor update (amsgrad = False, no weight decay) behind
                              replace_nangrad_to_zero and in front of zero_grad, bias corrections in double
  add_densification_stats  -- the three statements of the method
  Model                    -- step, densify_and_clone, densify_and_split, densification_postfix / cat_tensors_to_optimizer,
                              prune_points / _prune_optimizer, densify_and_prune, prune
  masked_rows / kept_list / append_rows -- `t[mask]`, `nonzero(mask)`, `cat((t, t[sel].repeat(r, 1...)))`

Values are carried in fp64 but stay inside the fp32 RANGE: after every statement a magnitude that fp32 would round to
infinity becomes infinity (`_r`), so the NaN / inf pattern is the fp32 one.  Mask comparisons are made on fp32 values:
`accum / denom` is one correctly rounded fp32 division, thresholds are rounded to fp32 (torch compares an fp32 tensor with a
Python float that way: torch.tensor([0.1]) > 0.1 is False), exp of a log-scale is rounded to fp32 before it meets the limit.

The oracle is pinned by tests/test_optim_edge_inputs.py: the reference's own methods (tests/golden/densify*.npz) and
torch.optim.Adam on the CPU.
"""
import numpy as np

F32_MAX = float(np.finfo(np.float32).max)
NANGRAD_VALUES = {"xyz": 0.0, "f_dc": 0.0, "f_rest": 0.0, "scaling": 1e-6, "rotation": 1e-6, "opacity": 0.0}
NANGRAD_VALUES_PBR = {"roughness": 1e-6, "base_color": 0.0, "normal": 0.0}
BOOK = ("weights_accum", "xyz_gradient_accum", "normal_gradient_accum", "denom", "max_radii2D")
SCAN_ELEMS, SCAN_BLOCK, ADAM_CHUNK, MAX_TENSORS = 2048, 256, 4096, 32   # the launch geometry the case table is built around


def f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32)


def _r(x):
    """fp64 value, fp32 range: what fp32 rounds to +-inf is +-inf."""
    x = np.asarray(x, dtype=np.float64)
    y = f32(x)
    return np.where(np.isinf(y), y.astype(np.float64), x)


# ---- Adam ------------------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, nan_value=None, fill=False):
    """One update of one tensor; `step` is the count AFTER the increment (>= 1).  `nan_value`: NaN gradient entries become
    fp32(nan_value) first (in the gradient tensor too); `fill`: the gradient tensor reads zero afterwards.
    Returns (param, exp_avg, exp_avg_sq, gradient tensor as left behind)."""
    b1, b2 = betas
    p, g, m, v = (np.array(a, dtype=np.float64) for a in (p, g, m, v))
    if nan_value is not None:
        g = np.where(np.isnan(g), float(np.float32(nan_value)), g)
    with np.errstate(all="ignore"):
        m = _r(m + _r((1.0 - b1) * _r(g - m)))                    # exp_avg.lerp_(grad, 1 - beta1)
        v = _r(_r(v * b2) + _r(_r((1.0 - b2) * g) * g))           # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        denom = _r(_r(np.sqrt(v) / np.sqrt(bc2)) + eps)
        p = _r(p + _r((-(lr / bc1)) * _r(m / denom)))             # param.addcdiv_(exp_avg, denom, value = -step_size)
    return p, m, v, (np.zeros_like(g) if fill else g)


# ---- statistics ------------------------------------------------------------------------------------------------------------
def add_densification_stats(vgrad, update_filter, weights, weights_accum, xyz_gradient_accum, denom):
    """Returns the three arrays [P,1] after the method; rows outside the filter are untouched whatever their gradient holds."""
    flt = np.asarray(update_filter, dtype=bool)
    wa, ga, dn = (np.array(a, dtype=np.float64) for a in (weights_accum, xyz_gradient_accum, denom))
    if weights is not None:
        wa = wa + np.asarray(weights, dtype=np.float64)
    vg = np.asarray(vgrad, dtype=np.float64)[:, :2]
    with np.errstate(all="ignore"):
        nrm = _r(np.sqrt(_r(_r(vg[:, 0] * vg[:, 0]) + _r(vg[:, 1] * vg[:, 1]))))
        ga[flt, 0] = _r(ga[flt, 0] + nrm[flt])
    dn[flt, 0] += 1.0
    return wa, ga, dn


# ---- rows ------------------------------------------------------------------------------------------------------------------
def kept_list(mask):
    return np.flatnonzero(np.asarray(mask, dtype=bool)).astype(np.int32)


def masked_rows(t, mask):
    return np.asarray(t)[np.asarray(mask, dtype=bool)]


def append_rows(t, sel, repeat=1, zero_new=False):
    """cat((t, t[sel].repeat(repeat, 1...))): the whole selection once, then again (Tensor.repeat), not row by row."""
    t = np.asarray(t)
    new = np.concatenate([t[np.asarray(sel, dtype=bool)]] * repeat, axis=0) if repeat else t[:0]
    return np.concatenate([t, np.zeros_like(new) if zero_new else new], axis=0)


# ---- activations and selections --------------------------------------------------------------------------------------------
def get_scaling(raw):
    """nan_to_num(exp(_scaling), nan = 1e-6) with fp32 range (+inf -> FLT_MAX), fp64 values of the fp32 inputs."""
    with np.errstate(all="ignore"):
        e = _r(np.exp(np.asarray(f32(raw), dtype=np.float64)))
    e = np.where(np.isnan(e), float(np.float32(1e-6)), e)
    return np.where(e == np.inf, F32_MAX, e)


def mean_grads(accum, denom):
    """densify_and_prune's grads: one fp32 division, NaN -> 0.  [P] fp32."""
    with np.errstate(all="ignore"):
        g = f32(accum).reshape(-1) / f32(denom).reshape(-1)
    g[np.isnan(g)] = 0.0
    return g


def max_scale32(raw):
    return f32(get_scaling(raw).max(axis=1)) if np.asarray(raw).shape[0] else np.zeros(0, np.float32)


def selection_masks(xyz_accum, normal_accum, denom, scaling_raw, max_grad, max_grad_normal, size_limit):
    """(clone, split) over the rows the statistics cover: densify_and_clone tests the NORM of the mean gradient (|.| of its one
    component), densify_and_split the SIGNED value; the scale test is <= / > the limit."""
    g, gn = mean_grads(xyz_accum, denom), mean_grads(normal_accum, denom)
    tg, tn, lim = np.float32(max_grad), np.float32(max_grad_normal), np.float32(size_limit)
    s = max_scale32(scaling_raw)
    clone = ((np.abs(g) >= tg) | (np.abs(gn) >= tn)) & (s <= lim)
    split = ((g >= tg) | (gn >= tn)) & (s > lim)
    return clone, split


def split_transform(xyz, scaling_raw, rotation, z, N):
    """The new points of densify_and_split for already repeated rows: (xyz, scaling)."""
    s = get_scaling(scaling_raw)
    q = np.asarray(rotation, dtype=np.float64)
    with np.errstate(all="ignore"):
        q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
        r, x, y, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = np.stack([1 - 2 * (y * y + w * w), 2 * (x * y - r * w), 2 * (x * w + r * y),
                      2 * (x * y + r * w), 1 - 2 * (x * x + w * w), 2 * (y * w - r * x),
                      2 * (x * w - r * y), 2 * (y * w + r * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
        samples = _r(s * np.asarray(z, dtype=np.float64))
        # (bmm sums the three products of a row: a NaN / inf entry reaches the sum even when its factor is zero)
        new_xyz = _r(_r((R * samples[:, None, :]).sum(axis=2)) + np.asarray(xyz, dtype=np.float64))
        new_scaling = np.log(_r(s / (0.8 * N)))      # (FLT_MAX / 0.8 overflows in fp32: N = 1)
    new_scaling[:, -1] = -1e10
    return new_xyz, new_scaling


# ---- the model -------------------------------------------------------------------------------------------------------------
class Model:
    """GaussianModel's optimisation / densification half.  `params`: {name: array [P, ...]} in optimizer-group order, `lrs`:
    {name: lr}.  state[name] is None until the group's first step, then {"step", "exp_avg", "exp_avg_sq"}."""

    def __init__(self, params, lrs, percent_dense=0.01, use_pbr=True, betas=(0.9, 0.999), eps=1e-15):
        self.params = {n: np.array(a, dtype=np.float64) for n, a in params.items()}
        self.lrs, self.percent_dense, self.use_pbr, self.betas, self.eps = dict(lrs), percent_dense, use_pbr, betas, eps
        self.state = {n: None for n in self.params}
        P = self.P
        self.weights_accum, self.xyz_gradient_accum, self.normal_gradient_accum, self.denom = (np.zeros((P, 1)) for _ in range(4))
        self.max_radii2D = np.zeros(P)
        # where every current row came from (row of the block at `mark()`), whether densification created it since (its moments are
        # zero) and whether it is a split child (its xyz / scaling were computed, not moved): the row movement, for exact checks
        self.mark()
        self.compared = []     # (kind, fp32 values, fp32 threshold) of every mask comparison made, for the threshold-row check

    def mark(self):
        self.origin, self.fresh, self.child = np.arange(self.P), np.zeros(self.P, dtype=bool), np.zeros(self.P, dtype=bool)

    @property
    def P(self):
        return self.params["xyz"].shape[0]

    def step(self, grads):
        """GaussianModel.step(): grads {name: array or None}; a group without a gradient is skipped, count and all."""
        nv = dict(NANGRAD_VALUES)
        if self.use_pbr:
            nv.update(NANGRAD_VALUES_PBR)
        for n, p in self.params.items():
            g = grads.get(n)
            if g is None:
                continue
            st = self.state[n]
            if st is None:
                st = self.state[n] = {"step": 0, "exp_avg": np.zeros_like(p), "exp_avg_sq": np.zeros_like(p)}
            st["step"] += 1
            self.params[n], st["exp_avg"], st["exp_avg_sq"], _ = adam_step(
                p, g, st["exp_avg"], st["exp_avg_sq"], st["step"], self.lrs[n], self.betas, self.eps, nan_value=nv.get(n))

    def _rows(self, fn, moments, new=None, child=False):
        """`new`: None for a compaction, else the number of rows `fn` appends"""
        self.origin = fn(self.origin)
        if new is None:
            self.fresh, self.child = fn(self.fresh), fn(self.child)
        else:
            self.fresh = np.concatenate([self.fresh, np.ones(new, dtype=bool)])
            self.child = np.concatenate([self.child, np.full(new, child)])
        for n in self.params:
            self.params[n] = fn(self.params[n])
            st = self.state[n]
            if st is not None:
                st["exp_avg"], st["exp_avg_sq"] = moments(st["exp_avg"]), moments(st["exp_avg_sq"])

    def _postfix(self, n_new):
        """densification_postfix's bookkeeping: ones for the new weights, every other statistic restarts for ALL rows."""
        self.weights_accum = np.concatenate([self.weights_accum, np.ones((n_new, 1))], axis=0)
        P = self.P
        self.xyz_gradient_accum, self.normal_gradient_accum, self.denom = np.zeros((P, 1)), np.zeros((P, 1)), np.zeros((P, 1))
        self.max_radii2D = np.zeros(P)

    def densify_and_clone(self, g, gn, max_grad, max_grad_normal, extent):
        lim = np.float32(self.percent_dense * extent)
        s = max_scale32(self.params["scaling"])
        self.compared += [("grad", np.abs(g), np.float32(max_grad)), ("grad", np.abs(gn), np.float32(max_grad_normal)), ("scale", s, lim)]
        sel = ((np.abs(g) >= np.float32(max_grad)) | (np.abs(gn) >= np.float32(max_grad_normal))) & (s <= lim)
        self._rows(lambda t: append_rows(t, sel, 1), lambda t: append_rows(t, sel, 1, zero_new=True), new=int(sel.sum()))
        self._postfix(int(sel.sum()))
        return sel

    def densify_and_split(self, g, gn, max_grad, max_grad_normal, extent, z, N=2):
        P = self.P
        pg, pgn = np.zeros(P, np.float32), np.zeros(P, np.float32)     # padded_grad: zero for rows cloned since the statistics
        pg[:g.shape[0]], pgn[:gn.shape[0]] = g, gn
        lim = np.float32(self.percent_dense * extent)
        s = max_scale32(self.params["scaling"])
        self.compared += [("grad", pg, np.float32(max_grad)), ("grad", pgn, np.float32(max_grad_normal)), ("scale", s, lim)]
        sel = ((pg >= np.float32(max_grad)) | (pgn >= np.float32(max_grad_normal))) & (s > lim)
        n_new = int(sel.sum()) * N
        self._rows(lambda t: append_rows(t, sel, N), lambda t: append_rows(t, sel, N, zero_new=True), new=n_new, child=True)
        if n_new:
            z = np.asarray(z, dtype=np.float64).reshape(-1, 3)[:n_new]
            xyz, sc = split_transform(self.params["xyz"][P:], self.params["scaling"][P:], self.params["rotation"][P:], z, N)
            self.params["xyz"][P:], self.params["scaling"][P:] = xyz, sc
        self._postfix(n_new)
        self.prune_points(np.concatenate([sel, np.zeros(n_new, dtype=bool)]))
        return sel

    def prune_points(self, mask):
        keep = ~np.asarray(mask, dtype=bool)
        self._rows(lambda t: t[keep], lambda t: t[keep])
        for k in BOOK:
            setattr(self, k, getattr(self, k)[keep])

    def prune_mask(self, min_opacity, extent, max_screen_size, weights_threshold):
        with np.errstate(all="ignore"):
            opacity = f32(1.0 / (1.0 + np.exp(-np.asarray(f32(self.params["opacity"]), dtype=np.float64)))).reshape(-1)
        mask = (opacity < np.float32(min_opacity)) | (f32(self.weights_accum[:, 0]) < np.float32(weights_threshold))
        self.compared += [("value", opacity, np.float32(min_opacity)), ("value", f32(self.weights_accum[:, 0]), np.float32(weights_threshold))]
        if max_screen_size:
            s = max_scale32(self.params["scaling"])
            mask = mask | (f32(self.max_radii2D) > np.float32(max_screen_size)) | (s > np.float32(0.1 * extent))
            self.compared += [("value", f32(self.max_radii2D), np.float32(max_screen_size)), ("scale", s, np.float32(0.1 * extent))]
        return mask

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, max_grad_normal, weights_threshold=1e-5, z=None):
        g = mean_grads(self.xyz_gradient_accum, self.denom)
        gn = mean_grads(self.normal_gradient_accum, self.denom)
        clone = self.densify_and_clone(g, gn, max_grad, max_grad_normal, extent)
        split = self.densify_and_split(g, gn, max_grad, max_grad_normal, extent, z)
        pruned = self.prune_mask(min_opacity, extent, max_screen_size, weights_threshold)
        self.prune_points(pruned)
        self.weights_accum[:] = 0.0
        return clone, split[:clone.shape[0]], pruned

    def prune(self, min_opacity, extent, max_screen_size, weights_threshold=1e-4):
        pruned = self.prune_mask(min_opacity, extent, max_screen_size, weights_threshold)
        self.prune_points(pruned)
        self.weights_accum[:] = 0.0
        return pruned
