"""A plain oracle of the fused optimizer step (``csrc/optim.hip``: ``clip_grad_norm_`` -> Adam / AdamW; ``k_soap_adam`` of
``csrc/soap_train.hip``), the bars the device is held to, and the data the tests feed it. No GPU import.

Two things compute the step:

``formula_step``  the documented formulas written out on a parameter list (``{key: 1-D tensor}``), in the dtype handed in:
    norm = sqrt(sum over the live parameters of sum g^2); coef = min(1, max_norm / (norm + 1e-6)) (``max_norm <= 0``: 1);
    g' = coef g; AdamW: w <- w (1 - lr wd); m <- b1 m + (1 - b1) g'; v <- b2 v + (1 - b2) g'^2;
    w <- w - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), bc_i = 1 - b_i^t with t the parameter's OWN step count.
    In fp32 it rounds where the kernel rounds (norm accumulated in fp64 and rounded once, every later operation in fp32, no
    fused multiply-add: the device may contract and then rounds less often). ``mutation`` names one deliberate error of the
    sensitivity list (``MUTATIONS``).
``TorchRun``  ``torch.optim.Adam`` / ``AdamW`` and ``torch.nn.utils.clip_grad_norm_`` themselves in fp64 on leaf tensors: a tied
    parameter once, an idle (frozen) parameter with ``.grad = None``.

Hyperparameters reach the device as ``float``; the oracle gets those fp32 values widened (``Hypers.widened``) and, as the code
does, forms bc1 and sqrt(bc2) in fp64 from the widened betas and rounds them to fp32 (``round_bc``).

Bars (``bars``), elementwise against ``formula_step`` in fp64, u = 2^-24 the unit roundoff of fp32; each constant counts the
fp32 roundings between the inputs and the quantity (first order; one spare unit covers the second-order terms and the
constant 1e-6f):

norm          K_NORM = 2, relative: fp64 accumulation (its error is 1e-16 relative) and ONE rounding of sqrt to fp32.
g' = coef g   K_G = 6 u |ref|: norm (1), norm + 1e-6f (1), the division (1), 1e-6f against 1e-6 (at most 1 for norm >= 1e-6),
              the product (1), and the sum g_a + g_b of a tied parameter's two slots (1). Exact where coef == 1 and no tie.
exp_avg       K_M = 9 u (|b1 m| + |(1 - b1) g'|): the g' term carries K_G, its product 1 and the sum 1 (8); the m term 2;
              1 - b1 is exact (b1 >= 0.5). Against the SUM of the magnitudes: the terms cancel.
exp_avg_sq    K_V = 16 u ref: g'^2 carries 2 K_G, two products, the sum (15); all terms are positive.
weight        c_w u |w| + (lr / bc1) [K_U u |m / denom| + bar_m / denom + |m / denom| (bar_v / (2 v)) s / denom],
              s = sqrt(v) / sqrt(bc2), denom = s + eps. c_w = 1 (the final subtraction) without decay and 4 with it
              (lr wd, 1 - lr wd, the product, the subtraction); K_U = 7: lr / bc1, sqrt, / sqrt(bc2), + eps, m / denom, the
              product, one spare. The last two terms are the errors of m and v carried through the quotient.
An element with g = m = v = 0 has update exactly 0: the weight must equal fl(w (1 - lr wd)) -- w itself under Adam.

``test_optim_cpu.py`` shows that the formulas in fp32 on the host stay inside every bar and that every mutation leaves one."""
import collections
import math

import torch

U = 2.0 ** -24
K_NORM, K_G, K_M, K_V, K_U = 2.0, 6.0, 9.0, 16.0, 7.0
NORM_BLOCKS = 256   # optim.hip

MUTATIONS = ("eps_inside_sqrt", "eps_before_bc2", "coupled_decay", "decay_after_update", "decay_under_adam", "no_1e-6_in_clip",
             "coef_not_clamped", "tied_counted_twice", "norm_includes_frozen", "bias_correction_step_minus_1",
             "global_step_after_sitting_out", "grad_left_unscaled")


def f32(x):
    """``x`` rounded to fp32, as a Python double."""
    return float(torch.tensor(float(x), dtype=torch.float32))


class Hypers(collections.namedtuple("Hypers", "lr b1 b2 eps wd max_norm")):
    """``wd = None``: Adam (no decay); a number: AdamW. ``max_norm <= 0``: no clipping."""

    def widened(self):
        return Hypers(f32(self.lr), f32(self.b1), f32(self.b2), f32(self.eps), None if self.wd is None else f32(self.wd),
                      f32(self.max_norm))


def hypers(lr=1e-2, wd=None, max_norm=0.0, b1=0.9, b2=0.999, eps=1e-8):
    return Hypers(lr, b1, b2, eps, wd, max_norm)


def bias_corrections(hp, t, round_bc=True):
    """(bc1, sqrt(bc2)) of step ``t`` in fp64, rounded to fp32 as ``adam_step`` hands them to the kernel."""
    bc1, bc2s = 1.0 - hp.b1 ** t, math.sqrt(1.0 - hp.b2 ** t)
    return (f32(bc1), f32(bc2s)) if round_bc else (bc1, bc2s)


def total_norm(g, live, dtype, tied=(), mutation=None, idle=()):
    """The norm over the parameter list (fp64 accumulation), and its value in ``dtype``."""
    s = 0.0
    for k in g:
        if k in live or (mutation == "norm_includes_frozen" and k in idle):
            s2 = float((g[k].double() ** 2).sum())
            s += 2.0 * s2 if (mutation == "tied_counted_twice" and k in tied) else s2
    return float(torch.tensor(math.sqrt(s), dtype=dtype))


def clip_coefficient(norm, hp, dtype, mutation=None):
    if not hp.max_norm > 0.0:
        return 1.0
    one = torch.tensor(1.0, dtype=dtype)
    small = torch.tensor(0.0 if mutation == "no_1e-6_in_clip" else 1e-6, dtype=dtype)
    coef = torch.tensor(hp.max_norm, dtype=dtype) / (torch.tensor(norm, dtype=dtype) + small)
    if mutation != "coef_not_clamped":
        coef = torch.minimum(coef, one)
    return float(coef)


def formula_step(w, m, v, g, steps, hp, dtype, idle=(), tied=(), mutation=None, round_bc=True, global_step=None, soap=False):
    """One step of the written-out formulas in ``dtype``. ``w, m, v, g``: ``{key: 1-D tensor}`` (any dtype; converted);
    ``steps[key]``: the parameter's own step count INCLUDING this step (torch's ``state["step"]`` after the increment);
    ``idle``: keys without a gradient in this step (untouched, outside the norm). ``global_step`` feeds the mutation
    ``global_step_after_sitting_out``. ``soap``: the denominator as ``k_soap_adam`` writes it, ``sqrt(v / bc2) + eps`` with
    bc1 and bc2 (not its root) rounded to fp32. Returns ``(w, m, v, g', norm, coef)``; ``g'`` is what ``.grad`` holds after."""
    live = [k for k in w if k not in idle]
    norm = total_norm(g, live, dtype, tied, mutation, idle)
    coef = clip_coefficient(norm, hp, dtype, mutation)
    c = lambda x: torch.tensor(x, dtype=dtype)   # noqa: E731
    wn, mn, vn, gn = {}, {}, {}, {}
    for k in w:
        w0, m0, v0, g0 = (x[k].to(dtype) for x in (w, m, v, g))
        if k in idle:
            wn[k], mn[k], vn[k], gn[k] = w0.clone(), m0.clone(), v0.clone(), g0.clone()
            continue
        t = steps[k]
        if mutation == "bias_correction_step_minus_1":
            t -= 1
        if mutation == "global_step_after_sitting_out":
            t = global_step
        if soap:
            bc1, bc2 = 1.0 - hp.b1 ** t, 1.0 - hp.b2 ** t
            if round_bc:
                bc1, bc2 = f32(bc1), f32(bc2)
        else:
            bc1, bc2s = bias_corrections(hp, t, round_bc) if t > 0 else (0.0, 0.0)
        gs = g0 * c(coef)
        gn[k] = g0.clone() if mutation == "grad_left_unscaled" else gs
        ww = w0
        decay = hp.wd is not None or mutation == "decay_under_adam"
        wd = hp.wd if hp.wd is not None else -1.0   # the kernel's "none" is a negative number
        if mutation == "coupled_decay" and decay:
            gs = gs + c(wd) * ww
        elif decay and mutation != "decay_after_update":
            ww = ww * (c(1.0) - c(hp.lr) * c(wd))
        m1 = c(hp.b1) * m0 + (c(1.0) - c(hp.b1)) * gs
        v1 = c(hp.b2) * v0 + (c(1.0) - c(hp.b2)) * gs * gs
        if soap:
            ww = ww - c(hp.lr) * (m1 / c(bc1)) / (torch.sqrt(v1 / c(bc2)) + c(hp.eps))
        else:
            if mutation == "eps_inside_sqrt":
                denom = torch.sqrt(v1 / (c(bc2s) * c(bc2s)) + c(hp.eps))
            elif mutation == "eps_before_bc2":
                denom = (torch.sqrt(v1) + c(hp.eps)) / c(bc2s)
            else:
                denom = torch.sqrt(v1) / c(bc2s) + c(hp.eps)
            ww = ww - (c(hp.lr) / c(bc1)) * (m1 / denom)
        if decay and mutation == "decay_after_update":
            ww = ww * (c(1.0) - c(hp.lr) * c(wd))
        wn[k], mn[k], vn[k] = ww, m1, v1
    return wn, mn, vn, gn, norm, coef


class TorchRun:
    """``torch.optim.Adam`` (``wd is None``) / ``AdamW`` and ``clip_grad_norm_`` in fp64 on leaf tensors; moments and per
    parameter step counts may be preset (a loaded optimizer state)."""

    def __init__(self, w, hp, m=None, v=None, steps=None):
        self.hp = hp
        self.p = {k: t.double().clone().requires_grad_(True) for k, t in w.items()}
        if hp.wd is None:
            self.opt = torch.optim.Adam(list(self.p.values()), lr=hp.lr, betas=(hp.b1, hp.b2), eps=hp.eps, weight_decay=0.0)
        else:
            self.opt = torch.optim.AdamW(list(self.p.values()), lr=hp.lr, betas=(hp.b1, hp.b2), eps=hp.eps, weight_decay=hp.wd)
        for k, p in self.p.items():
            if steps is not None and steps.get(k, 0) > 0:
                self.opt.state[p] = {"step": torch.tensor(float(steps[k])), "exp_avg": m[k].double().clone(),
                                     "exp_avg_sq": v[k].double().clone()}

    def step(self, g, idle=(), lr=None):
        """One step with gradients ``g``; returns the pre-clip norm. ``idle`` keys get ``.grad = None``."""
        for k, p in self.p.items():
            p.grad = None if k in idle else g[k].double().clone()
        if lr is not None:
            for group in self.opt.param_groups:
                group["lr"] = lr
        norm = None
        if self.hp.max_norm > 0.0:
            norm = float(torch.nn.utils.clip_grad_norm_(list(self.p.values()), self.hp.max_norm))
        self.opt.step()
        return norm

    def weights(self):
        return {k: p.detach().clone() for k, p in self.p.items()}

    def grads(self):
        return {k: (None if p.grad is None else p.grad.clone()) for k, p in self.p.items()}

    def moments(self):
        zero = lambda p: torch.zeros_like(p)   # noqa: E731
        return ({k: self.opt.state[p]["exp_avg"].clone() if p in self.opt.state else zero(p.detach()) for k, p in self.p.items()},
                {k: self.opt.state[p]["exp_avg_sq"].clone() if p in self.opt.state else zero(p.detach()) for k, p in self.p.items()})

    def step_counts(self):
        return {k: int(self.opt.state[p]["step"]) if p in self.opt.state else 0 for k, p in self.p.items()}


# ---- bars --------------------------------------------------------------------------------------------------------------------
def bars(ref_in, ref_out, steps, hp, idle=(), soap=False, carried=None):
    """Elementwise bars ``{quantity: {key: tensor}}`` and the norm's relative bar, from the fp64 reference: ``ref_in`` =
    ``(w, m, v, g)`` before the step, ``ref_out`` = ``formula_step``'s result in fp64 (module docstring). ``carried``: the bars
    of the step before, where the reference's moments rather than the device's start this step (no moment accessor): b1
    times the old bar of exp_avg and b2 times the old bar of exp_avg_sq enter the new ones."""
    w0, m0, v0, _ = ref_in
    w1, m1, v1, g1, _, coef = ref_out
    out = {"grad": {}, "exp_avg": {}, "exp_avg_sq": {}, "weight": {}}
    c_w = 1.0 if hp.wd is None else 4.0
    for k in w0:
        if k in idle:   # bit-unchanged
            for q in out:
                out[q][k] = torch.zeros_like(w0[k], dtype=torch.float64)
            continue
        out["grad"][k] = K_G * U * g1[k].abs()
        out["exp_avg"][k] = K_M * U * ((hp.b1 * m0[k].double()).abs() + ((1.0 - hp.b1) * g1[k]).abs())
        out["exp_avg_sq"][k] = K_V * U * v1[k]
        if carried is not None:
            out["exp_avg"][k] = out["exp_avg"][k] + hp.b1 * carried["exp_avg"][k]
            out["exp_avg_sq"][k] = out["exp_avg_sq"][k] + hp.b2 * carried["exp_avg_sq"][k]
        if soap:
            bc1, bc2 = f32(1.0 - hp.b1 ** steps[k]), f32(1.0 - hp.b2 ** steps[k])
            bc2s = math.sqrt(bc2)
        else:
            bc1, bc2s = bias_corrections(hp, steps[k])
        s = torch.sqrt(v1[k]) / bc2s
        denom = s + hp.eps
        q = (m1[k] / denom).abs()
        out["weight"][k] = c_w * U * w1[k].abs() + (hp.lr / bc1) * (
            K_U * U * q + out["exp_avg"][k] / denom + q * (0.5 * out["exp_avg_sq"][k] / v1[k].clamp_min(1e-300)) * s / denom)
    return out, K_NORM * U


def worst(got, ref, bar, skip=()):
    """max over the elements of ``|got - ref| / bar`` for dicts of tensors; an element whose bar is 0 must be met exactly
    (ratio 0 if it is, inf if not). ``skip``: keys left out (idle parameters: the caller holds them to bit-equality)."""
    ratio = 0.0
    for k in ref:
        if k in skip:
            continue
        err = (got[k].double() - ref[k].double()).abs()
        b = bar[k].double()
        r = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
        if r.numel():
            ratio = max(ratio, float(r.max()))
    return ratio


def report(case, rows):
    """The table ``(case, quantity, max err / bar)`` a test prints before it asserts."""
    for quantity, ratio in rows:
        print(f"[optim] {case:<44s} {quantity:<12s} max err / bar = {ratio:.3f}")


def compare(case, got, ref_in, ref_out, steps, hp, idle=(), soap=False, quantities=("grad", "exp_avg", "exp_avg_sq", "weight")):
    """``got = (w, m, v, g', norm)`` against the fp64 reference: the table rows ``[(quantity, max err / bar)]``."""
    b, norm_bar = bars(ref_in, ref_out, steps, hp, idle, soap)
    w1, m1, v1, g1, norm, _ = ref_out
    ref = {"weight": w1, "exp_avg": m1, "exp_avg_sq": v1, "grad": g1}
    idx = {"weight": 0, "exp_avg": 1, "exp_avg_sq": 2, "grad": 3}
    rows = [(q, worst(got[idx[q]], ref[q], b[q], idle)) for q in quantities]
    if got[4] is not None:
        rows.append(("norm", abs(got[4] - norm) / (norm_bar * norm) if norm > 0 else float(got[4] != 0.0)))
    report(case, rows)
    return rows


# ---- the flat layout of the device and the parameter list of the reference -------------------------------------------------
def expected_layout(params, hypers_):
    """What ``HipModel.flat_layout()`` returns for a state dict: upload order, the integer table left out, a tied ``w_in``
    (activation = "SiLU") with twice its elements."""
    out = []
    for k, t in params.items():
        if k == "species_to_species_index":
            continue
        tied = hypers_["activation"] == "SiLU" and ".w_in." in k
        out.append((k, int(t.numel()) * (2 if tied else 1)))
    return out


def tied_keys(params, hypers_):
    return {k for k in params if hypers_["activation"] == "SiLU" and ".w_in." in k and k != "species_to_species_index"}


def split(flat, layout):
    """The flat buffer as ``{key: segment}`` (views)."""
    out, off = {}, 0
    for k, n in layout:
        out[k] = flat[off:off + n]
        off += n
    assert off == flat.numel()
    return out


def join(segs, layout):
    return torch.cat([segs[k].reshape(-1) for k, _ in layout])


def untie(segs, tied, how):
    """Device segments -> the reference's parameter list: of a tied segment ``[a; b]`` the first half (``how = "first"``) or
    the sum of the halves in fp64 (``"sum"``: the gradient of W used twice)."""
    out = {}
    for k, t in segs.items():
        if k in tied:
            h = t.numel() // 2
            out[k] = t[:h].clone() if how == "first" else t[:h].double() + t[h:].double()
        else:
            out[k] = t.clone()
    return out


def retie(plist, tied):
    """The reference's parameter list -> device segments: a tied parameter stacked on itself."""
    return {k: (torch.cat([t, t]) if k in tied else t) for k, t in plist.items()}


# ---- data ---------------------------------------------------------------------------------------------------------------------
def log_uniform(n, lo, hi, gen):
    mag = torch.exp(torch.rand(n, generator=gen, dtype=torch.float64) * (math.log(hi) - math.log(lo)) + math.log(lo))
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float()


def edge_data(layout, seed=0, unit_norm=False, tied=()):
    """Seeded fp32 buffers in the flat layout: ``w`` U(-1, 1); gradient magnitudes log-uniform over 1e-10 .. 1e2 with random
    signs, so that sqrt(v_hat) lies below, near and above eps = 1e-8; loaded moments ``m = h U(-1, 1)``, ``v = h^2`` with ``h``
    drawn like the gradient (|m| <= sqrt(v), as moments are). In every segment of at least four elements the element after the
    first is an exact zero of g, m and v (update exactly 0), and the first and last element of every segment carry a value
    unique to the segment, ``+-(1 + s / 64)`` (x 2^-3 in the gradient), so that a slip of the segment table lands on a visibly wrong
    weight. ``unit_norm``: the gradient is scaled by a power of two to a norm in [0.5, 1): the 1e-6 of ``clip_grad_norm_`` is
    then 17 u of the coefficient and more than an ulp of the fp32 norm -- at the unscaled norm of about 1e3 fp32 itself loses
    it. A tied segment's second half repeats the first in ``w``, ``m`` and ``v`` (the copies are equal), not in ``g``."""
    gen = torch.Generator().manual_seed(1000 + seed)
    n = sum(c for _, c in layout)
    w = (torch.rand(n, generator=gen, dtype=torch.float64) * 2.0 - 1.0).float()
    g = log_uniform(n, 1e-10, 1e2, gen)
    h = log_uniform(n, 1e-10, 1e2, gen).abs()
    m = (h.double() * (torch.rand(n, generator=gen, dtype=torch.float64) * 2.0 - 1.0)).float()
    v = h * h
    off, zeros = 0, []
    for s, (k, c) in enumerate(layout):
        mark = 1.0 + s / 64.0
        w[off], w[off + c - 1] = mark, -mark
        g[off], g[off + c - 1] = -mark / 8.0, mark / 8.0
        if c >= 4:
            zeros.append(off + 1)
            g[off + 1] = m[off + 1] = v[off + 1] = 0.0
        if k in tied:
            h2 = c // 2
            for t in (w, m, v):
                t[off + h2:off + c] = t[off:off + h2]
            if c >= 8:   # zero in both halves: the summed gradient is zero too
                g[off + h2 + 1] = 0.0
        off += c
    if unit_norm:
        norm = float(g.double().norm())
        g = g * 2.0 ** -(math.floor(math.log2(norm)) + 1)
        assert 0.5 <= float(g.double().norm()) < 1.0
    return {"w": w, "g": g, "m": m, "v": v, "zeros": torch.tensor(zeros, dtype=torch.long)}


# ---- the cases, and one checker for whatever takes the step ---------------------------------------------------------------------
Case = collections.namedtuple("Case", "name model moments wd clip step frozen")
LR = 1e-2   # large enough that lr^2 wd (decay after the update) stands clear of u |w|


def _cases():
    out = []
    for moments in ("zero", "loaded"):
        for opt, wd in (("adam", None), ("adamw0", 0.0), ("adamw", 0.1)):
            for clip in ("off", "below", "above", "equal"):
                out.append(Case(f"{moments}-{opt}-clip_{clip}", "plain", moments, wd, clip, 1 if moments == "zero" else 2, False))
    out += [Case(f"step_{t}", "plain", "loaded", 0.1, "off", t, False) for t in (1, 2, 1000, 10 ** 6)]
    out += [Case("tied-clip_below", "tied", "loaded", 0.1, "below", 2, False), Case("tied-clip_off", "tied", "zero", None, "off", 1, False),
            Case("frozen-clip_below", "plain", "loaded", 0.1, "below", 2, True), Case("frozen-clip_off", "plain", "zero", None, "off", 1, True),
            Case("tied-frozen-clip_below", "tied", "loaded", 0.1, "below", 2, True)]
    return out


CASES = _cases()
CASE = {c.name: c for c in CASES}
FAILS_ON = {   # mutation -> the case whose bars it must leave
    "eps_inside_sqrt": "zero-adam-clip_off", "eps_before_bc2": "zero-adam-clip_off", "coupled_decay": "loaded-adamw-clip_off",
    "decay_after_update": "loaded-adamw-clip_off", "decay_under_adam": "zero-adam-clip_off", "no_1e-6_in_clip": "zero-adam-clip_below",
    "coef_not_clamped": "loaded-adamw-clip_above", "tied_counted_twice": "tied-clip_below",
    "norm_includes_frozen": "frozen-clip_below", "bias_correction_step_minus_1": "step_2", "grad_left_unscaled": "zero-adamw0-clip_below",
}


def model_case(tag):
    """(hypers, atomic types, state dict) of the smallest PET model of ``gen_shapes.py``; ``"tied"``: activation = "SiLU"."""
    import gen_shapes as gs
    from oracle import pet as opet

    hy = dict(opet.DEFAULT_HYPERS, **gs.CASES["hd3"])
    if tag == "tied":
        hy["activation"] = "SiLU"
    return hy, list(gs.TYPES), opet.synthetic_params(hy, gs.TYPES, {"energy": 1}, 0, torch.float32)


def frozen_subset(layout, tied):
    """Every third key, the first tied key among them and the second tied key not."""
    keys = [k for k, _ in layout]
    sub = set(keys[1::3])
    t = [k for k in keys if k in tied]
    if t:
        sub.add(t[0])
        sub.discard(t[1])
    return sub


def head_keys(layout):
    return [k for k, _ in layout if k.split(".")[0] in ("node_heads", "edge_heads", "node_last_layers", "edge_last_layers")]


class Checker:
    """Drives an engine -- ``load(w, m, v)`` (flat fp32 buffers; ``m = None``: fresh moments), ``set_frozen(keys)``,
    ``step(g, hp, t, idle) -> (w, m, v, g', norm)`` flat fp32 buffers and a float -- and holds every step to ``formula_step`` in
    fp64 started from the state the engine itself had before that step. It keeps the per-parameter step counts the way torch
    does: a parameter that is frozen or idle in a step does not count it."""

    def __init__(self, engine, layout, tied):
        self.e, self.layout, self.tied = engine, layout, set(tied)
        self.frozen, self.lag = set(), {k: 0 for k, _ in layout}

    def load(self, w, m=None, v=None):
        self.state = (w.clone(), torch.zeros_like(w) if m is None else m.clone(), torch.zeros_like(w) if v is None else v.clone())
        self.e.load(w, m, v)
        self.lag = {k: 0 for k in self.lag}

    def set_frozen(self, keys):
        self.frozen = set(keys)
        self.e.set_frozen(self.frozen)

    def reference(self, g, hp, t, idle, **kw):
        """fp64 formulas from the engine's pre-step state: ``(ref_in, ref_out, steps, idle)`` on the parameter list."""
        w, m, v = (untie(split(x, self.layout), self.tied, "first") for x in self.state)
        gp = untie(split(g, self.layout), self.tied, "sum")
        out_of_step = self.frozen | set(idle)
        steps = {k: t - self.lag[k] - (1 if k in out_of_step else 0) for k in self.lag}
        ref_in = (w, m, v, gp)
        return ref_in, formula_step(w, m, v, gp, steps, hp.widened(), torch.float64, idle=out_of_step, tied=self.tied, **kw), steps, out_of_step

    def step(self, name, g, hp, t, idle=(), strict=True):
        """One step of the engine against the reference. ``strict``: every exact property is asserted here and the rows are
        left to the caller; otherwise (a mutated engine) a broken exact property becomes a row of its own with ratio inf."""
        ref_in, ref_out, steps, out = self.reference(g, hp, t, idle)
        w, m, v, g1, norm = self.e.step(g, hp, t, idle)
        broken = []

        def require(ok, *what):
            if strict:
                assert ok, (name,) + what
            elif not ok:
                broken.append(("exact", math.inf))

        names = ("weight", "exp_avg", "exp_avg_sq", "grad")
        segs = [split(x, self.layout) for x in (w, m, v, g1)]
        for k in self.tied - out:   # both copies / both slots hold the same bits
            for q, s in zip(names, segs):
                h = s[k].numel() // 2
                require(torch.equal(s[k][:h], s[k][h:]), q, k, "the two halves of a tied parameter differ")
        got = tuple(untie(s, self.tied, "first") for s in segs) + (norm,)
        rows = compare(name, got, ref_in, ref_out, steps, hp.widened(), out)
        pre = [split(x, self.layout) for x in self.state + (g,)]
        for k in out:   # bit-unchanged: value, both moments, the gradient slot
            for q, s, p in zip(names, segs, pre):
                require(torch.equal(s[k], p[k]), q, k, "a frozen / idle parameter changed")
        self._exact(require, hp, ref_in, ref_out, got, out)
        for k in out:
            self.lag[k] += 1
        self.state = (w.clone(), m.clone(), v.clone())
        return rows + broken, (w, m, v, g1, norm), ref_out

    def _exact(self, require, hp, ref_in, ref_out, got, out):
        """An element with g = m = v = 0 gets exactly the decay (either rounding of 1 - lr wd: with or without a fused
        multiply-add) and nothing else; with coefficient 1 an untied gradient is bit-unchanged."""
        w0, m0, v0, g0 = ref_in
        hw = hp.widened()
        for k in w0:
            if k in out:
                continue
            z = (g0[k] == 0) & (m0[k] == 0) & (v0[k] == 0)
            if bool(z.any()):
                require(bool((got[1][k][z] == 0).all() and (got[2][k][z] == 0).all() and (got[3][k][z] == 0).all()), k,
                        "moments or gradient of a zero element moved")
                before, after = w0[k][z].float(), got[0][k][z].float()
                if hp.wd is None:
                    require(torch.equal(after, before), k, "a zero-gradient element moved under Adam")
                else:
                    lr, wd = torch.tensor(hw.lr, dtype=torch.float32), torch.tensor(hw.wd, dtype=torch.float32)
                    two = before * (1.0 - lr * wd)
                    one = before * (1.0 - lr.double() * wd.double()).float()
                    require(bool(((after == two) | (after == one)).all()), k, "a zero-gradient element got more than the decay")
            if ref_out[5] == 1.0 and k not in self.tied:
                require(torch.equal(got[3][k].float(), g0[k].float()), k, "coefficient 1 changed the gradient")


def case_setup(case):
    """(layout, tied keys, data, frozen keys, hypers) of a case of ``CASES``. ``max_norm`` is 0 (off) or 0.3 x, 2 x, 1 x the
    fp64 norm of the live parameter list, rounded to fp32."""
    hy, _, params = model_case(case.model)
    layout, tied = expected_layout(params, hy), tied_keys(params, hy)
    d = edge_data(layout, seed=0, unit_norm=case.clip != "off", tied=tied)
    frozen = frozen_subset(layout, tied) if case.frozen else set()
    norm = total_norm(untie(split(d["g"], layout), tied, "sum"), [k for k, _ in layout if k not in frozen], torch.float64)
    factor = {"off": 0.0, "below": 0.3, "above": 2.0, "equal": 1.0}[case.clip]
    return layout, tied, d, frozen, hypers(lr=LR, wd=case.wd, max_norm=f32(factor * norm))


def run_case(engine, case, strict=True):
    """One case of ``CASES`` on a fresh engine: the table rows, asserted if ``strict``."""
    layout, tied, d, frozen, hp = case_setup(case)
    ck = Checker(engine, layout, tied)
    ck.load(d["w"], *((d["m"], d["v"]) if case.moments == "loaded" else (None, None)))
    ck.set_frozen(frozen)
    rows, got, ref_out = ck.step(case.name, d["g"], hp, case.step, strict=strict)
    coef = ref_out[5]
    if case.clip in ("off", "above"):
        assert coef == 1.0, (case.name, coef)
    else:   # the oracle's side of 1: "equal" is a hair under it by the 1e-6
        assert coef < 1.0, (case.name, coef)
        if strict:   # and the engine's: the largest untied live gradient element shrank
            live = torch.cat([torch.full((n,), float(k not in frozen and k not in tied)) for k, n in layout])
            i = int((d["g"].abs() * live).argmax())
            assert abs(float(got[3][i])) < abs(float(d["g"][i])), (case.name, "the coefficient is not under 1")
    if strict:
        for q, r in rows:
            assert r <= 1.0, (case.name, q, r)
    return rows


def run_sitting_out(engine, strict=True, with_set_trainable=False):
    """Three steps from fresh moments with the head keys idle in step 2 only (``frozen_for_step``): torch gives them the
    bias correction of THEIR second step in step 3. ``with_set_trainable``: instead, the head keys are frozen by
    ``set_trainable`` for steps 1 and 2, turned back on, and take steps 3 and 4 -- torch's steps 1 and 2 for them. Returns
    the rows of the steps after the idle ones."""
    case = CASE["zero-adamw-clip_below"]
    layout, tied, d, _, hp = case_setup(case)
    ck = Checker(engine, layout, tied)
    ck.load(d["w"])
    heads = head_keys(layout)
    assert heads
    grads = [d["g"]] + [edge_data(layout, seed=s, unit_norm=True, tied=tied)["g"] for s in (1, 2, 3)]
    rows = []
    if with_set_trainable:
        ck.set_frozen(heads)
        for t in (1, 2):
            ck.step(f"set_trainable off, step {t}", grads[t - 1], hp, t, strict=strict)
        ck.set_frozen(())
        for t in (3, 4):
            rows += ck.step(f"set_trainable back on, step {t}", grads[t - 1], hp, t, strict=strict)[0]
    else:
        ck.step("sitting out, step 1", grads[0], hp, 1, strict=strict)
        ck.step("sitting out, step 2 (heads idle)", grads[1], hp, 2, idle=heads, strict=strict)
        rows += ck.step("sitting out, step 3", grads[2], hp, 3, strict=strict)[0]
    if strict:
        for q, r in rows:
            assert r <= 1.0, (q, r)
    return rows


class HostEngine:
    """The written-out formulas in fp32 on the flat layout, rounding where the device rounds (the tied slots are summed in
    fp32); ``mutation`` makes it one of the wrong optimizers of ``MUTATIONS``. It counts a parameter's steps as torch does."""

    def __init__(self, layout, tied, mutation=None):
        self.layout, self.tied, self.mutation, self.frozen = layout, set(tied), mutation, set()

    def load(self, w, m, v):
        self.w = w.clone()
        self.m = torch.zeros_like(w) if m is None else m.clone()
        self.v = torch.zeros_like(w) if v is None else v.clone()
        self.lag = {k: 0 for k, _ in self.layout}

    def set_frozen(self, keys):
        self.frozen = set(keys)

    def step(self, g, hp, t, idle=()):
        out = self.frozen | set(idle)
        gs = split(g.clone(), self.layout)
        gp = {}
        for k, s in gs.items():
            h = s.numel() // 2
            gp[k] = (s[:h] + s[h:]) if (k in self.tied and k not in out) else s
        w, m, v = (untie(split(x, self.layout), self.tied - out, "first") for x in (self.w, self.m, self.v))
        steps = {k: t - self.lag[k] for k in self.lag}
        wn, mn, vn, gn, norm, _ = formula_step(w, m, v, gp, steps, hp.widened(), torch.float32, idle=out, tied=self.tied,
                                               mutation=self.mutation, global_step=t)
        for k in out:
            self.lag[k] += 1
        live_tied = self.tied - out
        self.w, self.m, self.v = (join(retie(x, live_tied), self.layout) for x in (wn, mn, vn))
        return self.w.clone(), self.m.clone(), self.v.clone(), join(retie(gn, live_tied), self.layout), norm
