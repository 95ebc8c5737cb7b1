"""The fused optimizer step on the device (``csrc/optim.hip``: ``k_tie_grads`` -> ``k_sumsq_partial`` -> ``k_clip_coef`` ->
``k_adam``; ``k_soap_adam`` of ``csrc/soap_train.hip``) given a KNOWN gradient, against the written-out formulas in fp64
(``_optim_oracle.py``) started from the state the device had before the step, at bars counted from the fp32 roundings of the
formula. ``test_optim_cpu.py`` holds the premises: the formulas are torch's optimizers, fp32 on the host stays inside every bar,
every error of the sensitivity list leaves one.

Parameters, moments and the gradient go in through ``HipModel.load``, ``load_optimizer_state``, ``zero_grad`` +
``set_flat_grad``; the results come back through ``param_as_uploaded``, ``optimizer_state``, ``flat_grad`` and the returned norm.
No graph, no forward pass: a handful of elementwise launches over 5 590 floats per test. Each test prints the table
``(case, quantity, max err / bar)`` before it asserts."""
import pytest
import torch

import _optim_oracle as oo

pytestmark = pytest.mark.gpu


class DeviceEngine:
    """``HipModel`` behind the engine interface of ``_optim_oracle.Checker``; a fresh model per ``load``."""

    def __init__(self, tag):
        self.hy, self.types, self.params = oo.model_case(tag)
        self.layout, self.tied = oo.expected_layout(self.params, self.hy), oo.tied_keys(self.params, self.hy)
        self.dev = torch.device("cuda:0")

    def load(self, w, m, v):
        from metatrain_amd import runtime as rt

        segs = oo.untie(oo.split(w, self.layout), self.tied, "first")
        state = {k: (t if k not in segs else segs[k].reshape(t.shape)).to(self.dev) for k, t in self.params.items()}
        self.model = rt.HipModel(self.hy, self.types)
        self.model.load(state, "energy")
        assert self.model.flat_layout() == self.layout and self.model.num_params == w.numel()
        self.model.zero_grad()
        if m is not None:
            self.model.load_optimizer_state({"exp_avg": m, "exp_avg_sq": v, "layout": self.layout})

    def set_frozen(self, keys):
        self.model.set_trainable({k: k not in keys for k, _ in self.layout})

    def read(self):
        st = self.model.optimizer_state()
        w = torch.cat([self.model.param_as_uploaded(k).reshape(-1) for k, _ in self.layout])
        return w.cpu(), st["exp_avg"].cpu(), st["exp_avg_sq"].cpu()

    def step(self, g, hp, t, idle=()):
        self.model.zero_grad()
        self.model.set_flat_grad(g.to(self.dev))
        with self.model.frozen_for_step(list(idle)):
            norm = self.model.adam_step(hp.lr, t, betas=(hp.b1, hp.b2), eps=hp.eps, weight_decay=hp.wd, max_grad_norm=hp.max_norm)
        w, m, v = self.read()
        return w, m, v, self.model.flat_grad().cpu(), float(norm)


@pytest.mark.parametrize("case", oo.CASES, ids=lambda c: c.name)
def test_one_step_against_the_formulas(case):
    """One step from zero and from loaded moments under Adam, AdamW with weight_decay 0.0 and 0.1, with ``max_grad_norm`` off,
    below the norm, above it (the coefficient clamps to exactly 1 and the gradient keeps its bits) and the norm itself (a hair
    under 1 by the 1e-6, on the oracle's side and on the device's); ``step`` 1, 2, 1000 and 10^6 (fp32 bc1 = sqrt(bc2) = 1);
    the tied model (both copies bit-equal, W once in the norm, both halves of the moments equal, each gradient slot the
    clipped sum of the two); a frozen subset alone and with the tie (out of the norm; value, moments and gradient slot
    bit-unchanged). Elements with g = m = v = 0 get exactly the decay, nothing under Adam."""
    oo.run_case(DeviceEngine(case.model), case)


def test_a_head_that_sat_out_a_step_takes_its_own_bias_correction():
    """Three steps with the head keys frozen in step 2 only (``frozen_for_step``, as ``TrainStep._finish`` does for the heads of
    targets absent from a step): step 3 against torch's per-parameter step count -- 2 for the heads, 3 for the rest."""
    oo.run_sitting_out(DeviceEngine("plain"))


def test_a_parameter_turned_back_on_starts_its_own_count():
    """The head keys frozen by ``set_trainable`` for steps 1 and 2, then trainable: steps 3 and 4 are their steps 1 and 2."""
    oo.run_sitting_out(DeviceEngine("plain"), with_set_trainable=True)


def _state_after_two_steps(tag="tied"):
    """An engine two steps in (the head keys idle in the second), its case data, and what a third step needs."""
    case = oo.CASE["tied-clip_below"]
    layout, tied, d, _, hp = oo.case_setup(case)
    e = DeviceEngine(tag)
    e.load(d["w"], d["m"], d["v"])
    e.step(d["g"], hp, 5)
    e.step(oo.edge_data(layout, 1, unit_norm=True, tied=tied)["g"], hp, 6, idle=oo.head_keys(layout))
    return e, layout, tied, oo.edge_data(layout, 2, unit_norm=True, tied=tied)["g"], hp


def test_two_identical_calls_give_the_same_bits():
    outs = []
    for _ in range(2):
        e, layout, tied, g, hp = _state_after_two_steps()
        outs.append(e.step(g, hp, 7))
    for a, b in zip(*outs):
        assert torch.equal(torch.as_tensor(a), torch.as_tensor(b))


def test_optimizer_state_round_trip_reproduces_the_next_step():
    """``optimizer_state()`` -> a new model -> ``load_optimizer_state()``: step n + 1 from the edge data is bit-identical to the
    one the original model takes, the bias correction of the heads that sat out a step included."""
    e, layout, tied, g, hp = _state_after_two_steps()
    state = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in e.model.optimizer_state().items()}
    w = e.read()[0]
    f = DeviceEngine("tied")
    f.load(w, None, None)
    f.model.load_optimizer_state(state)
    for a, b in zip(e.read(), f.read()):
        assert torch.equal(a, b)
    for a, b in zip(e.step(g, hp, 7), f.step(g, hp, 7)):
        assert torch.equal(torch.as_tensor(a), torch.as_tensor(b))


# ---- SOAP-BPNN ---------------------------------------------------------------------------------------------------------------
def test_soap_adam_step_against_the_formulas():
    """``soap_adam_step`` on the smallest model of ``soap_cases.py`` (one atomic type) and its graph: one real backward pass,
    ``grads()`` and ``params()`` read back, one step, the weights against the formulas run on the gradients read back -- the
    denominator as ``k_soap_adam`` writes it, ``sqrtf(v / c2) + eps``, no clipping, no decay. A second step from the same
    gradients checks that the moments carry over: its reference starts from the fp64 moments of the first. SOAP has no moment
    accessor, so only the weights are compared, the second step with the first step's bars of the moments carried into its
    own (``bars(..., carried=...)``)."""
    import soap_cases as sc
    from metatrain_amd.pet.trainer import energy_loss_and_seeds, force_loss_and_seeds
    from metatrain_amd.soap_bpnn import SoapBpnnHip

    dev = torch.device("cuda:0")
    name = "legacy_types_1"
    c, b = sc.case(name), sc.batch(name)
    m = SoapBpnnHip(c.hypers, c.types)
    m.load({k: v.to(dev) for k, v in sc.params(name).items()})
    g = m.graph(b["positions"].float().to(dev), b["cells"].float().to(dev), b["centers"].to(dev), b["neighbors"].to(dev),
                b["cell_shifts"].to(dev), b["species"].to(dev), b["system_indices"].int().to(dev))
    te, tg = sc.training_targets(name)
    n_atoms = torch.bincount(b["system_indices"], minlength=len(te)).float().to(dev)
    m.zero_grad()
    atomic = m.forward(g)
    loss, seeds = energy_loss_and_seeds(m.sum_over_atoms(g, atomic), te.float().to(dev), n_atoms, g.system_of_atom())
    _, u = force_loss_and_seeds(m.backward(g, torch.ones_like(atomic)), tg.float().to(dev))
    m.train_gradients(g, seeds, u)
    flat = lambda d: {k: t.detach().cpu().reshape(-1) for k, t in d.items()}   # noqa: E731
    grads, w0 = flat(m.grads()), flat(m.params())
    assert set(grads) == set(w0) and any(float(t.abs().max()) > 0 for t in grads.values())
    hp = oo.hypers(lr=1e-3)
    zeros = {k: torch.zeros_like(t, dtype=torch.float64) for k, t in w0.items()}
    ref_in = (w0, zeros, zeros, grads)
    steps = {k: 1 for k in w0}
    ref1 = oo.formula_step(*ref_in, steps, hp.widened(), torch.float64, soap=True)
    m.adam_step(hp.lr, 1)
    w1 = flat(m.params())
    rows = oo.compare("soap step 1", (w1, None, None, None, None), ref_in, ref1, steps, hp.widened(), soap=True, quantities=("weight",))
    # second step: the device's weights, the reference's moments
    steps = {k: 2 for k in w0}
    ref_in2 = (w1, ref1[1], ref1[2], grads)
    ref2 = oo.formula_step(*ref_in2, steps, hp.widened(), torch.float64, soap=True)
    m.adam_step(hp.lr, 2)
    w2 = flat(m.params())
    bar1, _ = oo.bars(ref_in, ref1, {k: 1 for k in w0}, hp.widened(), soap=True)
    bar2, _ = oo.bars(ref_in2, ref2, steps, hp.widened(), soap=True, carried=bar1)
    rows2 = [("weight", oo.worst(w2, ref2[0], bar2["weight"]))]
    oo.report("soap step 2 (moments carried over)", rows2)
    for q, r in rows + rows2:
        assert r <= 1.0, (q, r)
    moved = max(float((w2[k].double() - w1[k].double()).abs().max()) for k in w0)
    assert moved > 0.5 * hp.lr   # (Adam's step is about lr wherever the gradient is not tiny)
