"""The premises of ``test_gpu_optim.py``, with no GPU (``_optim_oracle.py`` holds the formulas, the bars and the cases):

* the written-out formulas equal ``torch.optim.Adam`` / ``AdamW`` + ``clip_grad_norm_`` in fp64 to a few ulp, over several
  steps, idle steps included -- which licenses the formulas as the reference;
* the formulas evaluated in fp32 on the host stay inside every bar, on every case the device runs (no bar is tighter than
  fp32 allows);
* every mutation of the sensitivity list leaves a bar on its case, in fp32 on the host (no bar is looser than the errors it
  exists to catch);
* what the fp32 rounding of the hyperparameters and of the bias corrections costs, against the nominal doubles;
* the learning-rate schedules of ``TrainStep`` and ``SoapTrainStep`` against ``LambdaLR``, the pairing of rate and bias
  correction, and their resumption.

None of these looks at device output."""
import math

import pytest
import torch

import _optim_oracle as oo

ULP64 = 2.0 ** -52


def _layout(tag):
    hy, _, params = oo.model_case(tag)
    return oo.expected_layout(params, hy), oo.tied_keys(params, hy)


def test_the_models_reach_the_edges_of_the_launch_geometry():
    """``num_params`` is a multiple neither of the 256-thread block of ``k_adam`` nor of ``NORM_BLOCKS``, so the last block of
    both kernels is partly filled and ``k_sumsq_partial`` has empty trailing blocks; there are one-element segments (first
    = last element), many segments for the binary search, and the tied model has tied keys the plain one lacks."""
    for tag in ("plain", "tied"):
        layout, tied = _layout(tag)
        n = sum(c for _, c in layout)
        assert n % 256 != 0 and n % oo.NORM_BLOCKS != 0, n
        per = -(-n // oo.NORM_BLOCKS)
        assert per * (oo.NORM_BLOCKS - 1) > n, "no empty trailing block in the norm's grid"
        assert n > 256 * 2 and len(layout) > 64 and min(c for _, c in layout) == 1
        assert bool(tied) == (tag == "tied")
        assert len(oo.head_keys(layout)) >= 4
        if tied:
            assert len(tied) >= 2 and all(dict(layout)[k] % 2 == 0 for k in tied)
            frozen = oo.frozen_subset(layout, tied)
            assert tied & frozen and tied - frozen
    assert sum(c for _, c in _layout("plain")[0]) < 10 ** 6


def test_the_data_reaches_the_edges_of_the_formula():
    layout, tied = _layout("tied")
    for unit in (False, True):
        d = oo.edge_data(layout, 0, unit_norm=unit, tied=tied)
        g = d["g"].double().abs()
        nz = g[g > 0]
        assert float(nz.min()) < 1e-9 * float(nz.max())   # ten decades
        root = nz * math.sqrt(1e-3) / math.sqrt(1.0 - 0.999)   # sqrt(v_hat) of a first step
        assert bool((root < 1e-9).any() and ((root > 3e-9) & (root < 3e-8)).any() and (root > 1e-6).any())
        z = d["zeros"]
        assert len(z) > 10 and bool((d["g"][z] == 0).all() and (d["m"][z] == 0).all() and (d["v"][z] == 0).all())
        firsts = []
        off = 0
        for k, c in layout:
            firsts.append(float(d["w"][off]))
            off += c
        assert len(set(firsts)) == len(layout)
        if unit:   # the 1e-6 of the clip is above the bar of the coefficient and above an ulp of the fp32 norm
            norm = float(d["g"].double().norm())
            assert 0.5 <= norm < 1.0 and 1e-6 / norm > oo.K_G * oo.U and 1e-6 > 8 * oo.U * norm


# ---- the formulas are torch's --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd,max_norm_factor", [(None, 0.0), (0.0, 0.3), (0.1, 0.3), (0.1, 2.0)])
def test_formulas_equal_torch_in_fp64_over_steps_with_idle_ones(wd, max_norm_factor):
    """Five steps on the parameter list of the tied model (W once), the head keys idle in steps 2 and 4, nominal doubles and
    unrounded bias corrections on both sides, each step of the formulas started from torch's state before it: weights, moments, clipped gradients and norms agree to 16 ulp of fp64 (torch
    forms exp_avg by lerp and the update by addcdiv: other roundings of the same formula). Measured against the magnitudes
    the terms have, since they cancel."""
    layout, tied = _layout("tied")
    data = [oo.edge_data(layout, s, unit_norm=True, tied=tied) for s in range(5)]
    heads = set(oo.head_keys(layout))
    w = oo.untie(oo.split(data[0]["w"], layout), tied, "first")
    w = {k: t.double() for k, t in w.items()}
    m = {k: torch.zeros_like(t) for k, t in w.items()}
    v = {k: torch.zeros_like(t) for k, t in w.items()}
    norm0 = float(torch.cat([t for t in oo.untie(oo.split(data[0]["g"], layout), tied, "sum").values()]).norm())
    hp = oo.hypers(lr=oo.LR, wd=wd, max_norm=max_norm_factor * norm0)
    run = oo.TorchRun(w, hp)
    steps = {k: 0 for k in w}
    worst = 0.0
    for t in range(1, 6):
        g = oo.untie(oo.split(data[t - 1]["g"], layout), tied, "sum")
        idle = heads if t in (2, 4) else set()
        for k in w:
            steps[k] += k not in idle
        tw0, (tm0, tv0) = run.weights(), run.moments()
        w0, m0, v = tw0, tm0, tv0   # every step starts from torch's own state: an error carried over from an earlier step
        w, m = w0, m0               # has no scale in this one (the terms of exp_avg cancel)
        w, m, v, g1, norm, coef = oo.formula_step(w, m, v, g, steps, hp, torch.float64, idle=idle, round_bc=False)
        tnorm = run.step(g, idle)
        assert run.step_counts() == steps
        if tnorm is not None:
            assert abs(tnorm - norm) <= 4 * ULP64 * norm
        tw, (tm, tv), tg = run.weights(), run.moments(), run.grads()
        for k in w:
            if k in idle:
                assert tg[k] is None and torch.equal(tw[k], tw0[k]) and torch.equal(tm[k], tm0[k])
                assert torch.equal(w[k], w0[k]) and torch.equal(m[k], m0[k])
                continue
            scale_m = (hp.b1 * m0[k]).abs() + ((1 - hp.b1) * g1[k]).abs()
            bc1, bc2s = oo.bias_corrections(hp, steps[k], round_bc=False)
            upd = (hp.lr / bc1) * (scale_m / (v[k].sqrt() / bc2s + hp.eps))
            for got, ref, scale in ((tg[k], g1[k], g1[k].abs()), (tm[k], m[k], scale_m), (tv[k], v[k], v[k]),
                                    (tw[k], w[k], w[k].abs() + upd)):
                err = (got - ref).abs()
                assert bool((err[scale == 0] == 0).all())
                if bool((scale > 0).any()):
                    worst = max(worst, float((err[scale > 0] / scale[scale > 0]).max()))
    print(f"[optim] formulas against torch (wd {wd}, clip {max_norm_factor}): worst {worst / ULP64:.1f} ulp of fp64")
    assert worst <= 16 * ULP64


def test_torch_counts_the_steps_of_a_parameter_that_sat_out_per_parameter():
    """The premise of the sitting-out case: after three steps with one parameter idle in step 2, torch's ``state["step"]`` is
    2 for it and 3 for the rest (``test_every_mutation_leaves_a_bar`` shows what a global step costs instead)."""
    w = {"a": torch.ones(3, dtype=torch.float64), "b": torch.ones(3, dtype=torch.float64)}
    run = oo.TorchRun(w, oo.hypers())
    g = {k: torch.full((3,), 0.5, dtype=torch.float64) for k in w}
    for t in (1, 2, 3):
        run.step(g, idle={"b"} if t == 2 else ())
    assert run.step_counts() == {"a": 3, "b": 2}


# ---- the bars: not tighter than fp32, not looser than the errors ----------------------------------------------------------------
@pytest.mark.parametrize("case", oo.CASES, ids=lambda c: c.name)
def test_fp32_formulas_on_the_host_stay_inside_every_bar(case):
    layout, tied = _layout(case.model)
    oo.run_case(oo.HostEngine(layout, tied), case)


@pytest.mark.parametrize("trainable", [False, True], ids=["frozen_for_step", "set_trainable"])
def test_fp32_formulas_on_the_host_stay_inside_the_bars_after_sitting_out(trainable):
    layout, tied = _layout("plain")
    oo.run_sitting_out(oo.HostEngine(layout, tied), with_set_trainable=trainable)


@pytest.mark.parametrize("mutation", oo.MUTATIONS)
def test_every_mutation_leaves_a_bar(mutation):
    if mutation == "global_step_after_sitting_out":
        layout, tied = _layout("plain")
        rows = oo.run_sitting_out(oo.HostEngine(layout, tied, mutation), strict=False)
        rows += oo.run_sitting_out(oo.HostEngine(layout, tied, mutation), strict=False, with_set_trainable=True)
    else:
        case = oo.CASE[oo.FAILS_ON[mutation]]
        layout, tied = _layout(case.model)
        rows = oo.run_case(oo.HostEngine(layout, tied, mutation), case, strict=False)
    worst = max(r for _, r in rows)
    print(f"[optim] mutation {mutation}: worst max err / bar = {worst:.3g}")
    assert worst > 1.0, (mutation, rows)


def test_what_the_fp32_hyperparameters_cost():
    """The device takes lr, beta1, beta2, eps and weight_decay as ``float`` and bc1, sqrt(bc2) rounded to fp32; the oracle
    is given the same numbers. Against the nominal doubles (0.9, 0.999, 1e-8) with unrounded bias corrections the UPDATED
    WEIGHT differs, between the two fp64 oracle runs, by at most

        |dw| <= 1.1 { |w| d(lr wd) + step [ r_lr + r_bc1 + (|m0| + |g'|) |db1| / |m1| + r_bc2s + d_eps / denom
                                            + (v0 + g'^2) |db2| / (2 v1) ] },    step = (lr / bc1) |m1| / denom,

    the first-order sensitivities of the update to each number (r_x: relative, d_x: absolute change of x; 1.1 for the second
    order). The beta2 term dominates: 1 - beta2 changes by 1.3e-5 relative. Checked at step 2 with loaded moments."""
    layout, tied = _layout("plain")
    d = oo.edge_data(layout, 0)
    w, m, v, g = (oo.split(d[q].double(), layout) for q in ("w", "m", "v", "g"))
    hp = oo.hypers(lr=oo.LR, wd=0.1)
    hw = hp.widened()
    t = 2
    steps = {k: t for k in w}
    a = oo.formula_step(w, m, v, g, steps, hw, torch.float64)
    b = oo.formula_step(w, m, v, g, steps, hp, torch.float64, round_bc=False)
    (bc1, bc2s), (bc1n, bc2sn) = oo.bias_corrections(hw, t), oo.bias_corrections(hp, t, round_bc=False)
    rel = lambda x, y: abs(x - y) / abs(y)   # noqa: E731
    worst = 0.0
    for k in w:
        m1, v1 = b[1][k], b[2][k]
        denom = v1.sqrt() / bc2sn + hp.eps
        step = (hp.lr / bc1n) * m1.abs() / denom
        sens = (rel(hw.lr, hp.lr) + rel(bc1, bc1n) + rel(bc2s, bc2sn) + abs(hw.eps - hp.eps) / denom
                + (v[k] + g[k] ** 2) * abs(hw.b2 - hp.b2) / (2 * v1).clamp_min(1e-300))
        bound = 1.1 * (w[k].abs() * abs(hw.lr * hw.wd - hp.lr * hp.wd) + step * sens
                       + (hp.lr / bc1n) * (m[k].abs() + g[k].abs()) * abs(hw.b1 - hp.b1) / denom)
        err = (a[0][k] - b[0][k]).abs()
        assert bool((err[bound == 0] == 0).all())
        ok = bound > 0
        if bool(ok.any()):
            worst = max(worst, float((err[ok] / bound[ok]).max()))
    print(f"[optim] fp32 hyperparameters against the nominal doubles: worst |dw| / bound = {worst:.3f}")
    assert worst <= 1.0


# ---- schedules -------------------------------------------------------------------------------------------------------------------
def _documented_lambda(total_steps, warmup_fraction):
    """Linear warm-up over ``int(warmup_fraction * total_steps)`` steps, then a cosine to zero over the rest."""
    warmup = int(warmup_fraction * total_steps)

    def f(step):
        if step < warmup:
            return float(step) / float(max(1, warmup))
        progress = (step - warmup) / float(max(1, total_steps - warmup))
        return 0.5 * (1.0 + math.cos(math.pi * progress))

    return f, warmup


class _StubModel:
    """Stands in for ``HipModel`` where ``TrainStep`` only schedules: records what reaches ``adam_step``."""

    target = None
    hypers = {}

    def __init__(self):
        self.calls = []
        self.state = {"exp_avg": torch.zeros(3), "exp_avg_sq": torch.zeros(3), "layout": [("a", 3)]}

    def head_keys(self):
        return {}

    def flat_grad(self):
        return torch.zeros(3)

    def set_flat_grad(self, flat):
        pass

    def frozen_for_step(self, keys):
        import contextlib

        return contextlib.nullcontext()

    def adam_step(self, lr, step, weight_decay=None, max_grad_norm=0.0):
        self.calls.append((lr, step))
        return torch.zeros(1)

    def optimizer_state(self):
        return dict(self.state)

    def load_optimizer_state(self, state):
        self.state = dict(state)


def _lambda_lr_rates(lr, fn, n):
    """The rate ``LambdaLR`` gives optimizer step 1 .. n (``scheduler.step()`` after each ``optimizer.step()``)."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=lr)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, fn)
    out = []
    for _ in range(n):
        out.append(opt.param_groups[0]["lr"])
        p.grad = torch.zeros(1)
        opt.step()
        sched.step()
    return out


SCHEDULES = [(total, wf) for total in (1, 7, 100) for wf in (0.0, 0.1, 0.5, 1.0)]


def _close(a, b):
    return a == b or abs(a - b) <= ULP64 * max(abs(a), abs(b))


@pytest.mark.parametrize("total,wf", SCHEDULES)
@pytest.mark.parametrize("split", [(1, None), (None, 1)], ids=["epochs", "steps_per_epoch"])
def test_pet_schedule_is_lambda_lr_over_a_whole_run(total, wf, split):
    """``TrainStep.current_lr()`` of every step of a run of ``total`` steps and one step past its end against ``LambdaLR`` on a
    dummy Adam: exact or within 1 ulp of fp64. The run includes the step where warm-up ends and the last step. The n-th
    optimizer step takes the rate of ``step_index = n - 1`` and the bias correction of step n."""
    from metatrain_amd.pet.trainer import TrainStep

    epochs, per = (total, 1) if split[0] == 1 else (1, total)
    lr = 3e-4
    model = _StubModel()
    ts = TrainStep(model, {"learning_rate": lr, "num_epochs": epochs, "warmup_fraction": wf}, steps_per_epoch=per)
    assert ts.total_steps == total
    fn, warmup = _documented_lambda(total, wf)
    ref = _lambda_lr_rates(lr, fn, total + 2)
    got = []
    for n in range(1, total + 3):
        assert ts.step_index == n - 1
        got.append(ts.current_lr())
        ts._finish()
        assert model.calls[-1] == (got[-1], n)
    for n, (a, b) in enumerate(zip(got, ref)):
        assert _close(a, b), (n, a, b)
    assert warmup <= total
    if 0 < warmup:
        assert got[0] == 0.0 and (warmup >= len(got) or got[warmup] == lr)   # the step where warm-up ends runs at the peak
    if warmup < total:
        assert abs(got[total]) <= lr * 1e-30 + 4e-33 or _close(got[total], ref[total])   # the cosine's end
    assert _close(got[total + 1], ref[total + 1])   # one step past the end


def test_pet_schedule_and_step_count_resume_from_a_state_dict():
    from metatrain_amd.pet.trainer import TrainStep

    hy = {"learning_rate": 1e-3, "num_epochs": 7, "warmup_fraction": 0.5}
    a = TrainStep(_StubModel(), hy, steps_per_epoch=3)
    for _ in range(5):
        a._finish()
    state = a.state_dict()
    b = TrainStep(_StubModel(), {"learning_rate": 9.0, "num_epochs": 1, "warmup_fraction": 0.0})
    b.load_state_dict(state)
    assert (b.step_index, b.total_steps) == (5, 21) and b.current_lr() == a.current_lr()
    for _ in range(3):
        a._finish()
        b._finish()
        assert a.model.calls[-1] == b.model.calls[-1]
    assert b.model.calls[-1][1] == 8 and b.state_dict()["step_index"] == 8


class _StubSoap:
    """Stands in for ``SoapBpnnHip`` in an energy-only step: one system of two atoms; records what reaches ``adam_step``."""

    def __init__(self):
        self.calls = []

    def system_of_atom(self):   # (the stub is its own graph)
        return torch.zeros(2, dtype=torch.long)

    def zero_grad(self):
        pass

    def forward(self, g):
        return torch.zeros(2)

    def sum_over_atoms(self, g, atomic):
        return atomic.sum().reshape(1)

    def train_gradients(self, g, seeds, u, u_cell):
        return None

    def adam_step(self, lr, step):
        self.calls.append((lr, step))


@pytest.mark.parametrize("total,wf", SCHEDULES)
def test_soap_schedule_is_lambda_lr_and_resumes(total, wf):
    """``SoapTrainStep.current_lr()`` against ``LambdaLR`` over a whole run and one step past it; the n-th step pairs the rate of
    ``step_index = n - 1`` with the bias correction of step n, read off what an energy-only ``__call__`` on a stub model hands
    to ``adam_step``; ``state_dict`` resumes both."""
    from metatrain_amd.soap_bpnn import SoapTrainStep

    lr = 1e-3
    ts = SoapTrainStep(_StubSoap(), {"learning_rate": lr, "num_epochs": total, "warmup_fraction": wf}, steps_per_epoch=1)
    fn, _ = _documented_lambda(total, wf)
    ref = _lambda_lr_rates(lr, fn, total + 2)
    for n in range(1, total + 3):
        assert ts.step_index == n - 1 and _close(ts.current_lr(), ref[n - 1]), (n, ts.current_lr(), ref[n - 1])
        if n == max(1, total // 2):
            other = SoapTrainStep(_StubSoap(), {"learning_rate": 5.0, "num_epochs": 3, "warmup_fraction": 0.0})
            other.load_state_dict(ts.state_dict())
            assert (other.step_index, other.total_steps, other.current_lr()) == (ts.step_index, ts.total_steps, ts.current_lr())
        out = ts(ts.model, torch.zeros(1), torch.full((1,), 2.0))
        assert ts.model.calls[-1] == (out["lr"], n) and _close(out["lr"], ref[n - 1])


def test_soap_formula_in_fp32_stays_inside_the_bars_over_two_steps():
    """``k_soap_adam``'s form of the update, ``lr (m / c1) / (sqrtf(v / c2) + eps)``, in fp32 on the host against fp64, as
    ``test_gpu_optim.py`` holds the device to it: step 1 from zero moments, step 2 from the fp32 weights and the fp64 moments
    with the first step's bars carried over (SOAP has no moment accessor). c1 and c2 formed in fp32 -- ``1 - powf(b2, 2)`` is off
    by up to 1.5e-5 relative, half an ulp of b2^2 against 1 - b2^2 -- leave the bar of step 2."""
    layout = [("a", 700), ("b", 1), ("c", 333)]
    d = oo.edge_data(layout, 0)
    w0, g = oo.split(d["w"], layout), oo.split(d["g"], layout)
    zeros = {k: torch.zeros_like(t, dtype=torch.float64) for k, t in w0.items()}
    hp = oo.hypers(lr=1e-3).widened()
    one, two = {k: 1 for k in w0}, {k: 2 for k in w0}
    ref1 = oo.formula_step(w0, zeros, zeros, g, one, hp, torch.float64, soap=True)
    got1 = oo.formula_step(w0, zeros, zeros, g, one, hp, torch.float32, soap=True)
    bar1, _ = oo.bars((w0, zeros, zeros, g), ref1, one, hp, soap=True)
    ref_in2 = (got1[0], ref1[1], ref1[2], g)
    ref2 = oo.formula_step(*ref_in2, two, hp, torch.float64, soap=True)
    bar2, _ = oo.bars(ref_in2, ref2, two, hp, soap=True, carried=bar1)
    got2 = oo.formula_step(got1[0], got1[1], got1[2], g, two, hp, torch.float32, soap=True)
    rows = [("step 1", oo.worst(got1[0], ref1[0], bar1["weight"])), ("step 2", oo.worst(got2[0], ref2[0], bar2["weight"]))]
    oo.report("soap formula, fp32 host", rows)
    assert all(r <= 1.0 for _, r in rows), rows
    # the fp32 bias corrections: the worst rounding of b2^2 to fp32, half an ulp off, carried into c2
    b2sq = oo.f32(hp.b2 ** 2)
    half_ulp = 2.0 ** -25   # of a number in [0.5, 1)
    c2_bad = oo.f32(1.0 - (b2sq + half_ulp))
    bad = {k: got1[0][k].double() - hp.lr * (ref2[1][k] / oo.f32(1.0 - hp.b1 ** 2)) / (torch.sqrt(ref2[2][k] / c2_bad) + hp.eps)
           for k in w0}
    worst_bad = oo.worst(bad, ref2[0], bar2["weight"])
    print(f"[optim] soap step 2 with b2^2 half an fp32 ulp off: max err / bar = {worst_bad:.2f}")
    assert worst_bad > 1.0
