"""GPU tests of the long-range PET's training sweep with a CELL tangent and of the stress term of ``LongRangeTrainStep``
(``pet_backward_train2_long_range_cell``; ``LongRangeFeaturizerHip(..., cell_tangents=True)``), by Ewald
summation and through P3M, against ``_long_range_cell_oracle.evaluate_cell``.

Bar (``gen_shapes.bar``): ``relmax = max|got - ref| / max|ref| <= max(1e-5, 2 y)`` with ``y`` the relmax of the fp32 oracle
against its fp64 self, an input counting only if ``y <= 1e-3``; per parameter tensor, and per SYSTEM for the per-atom tangents
(``ewald_cases.check_per_system``: the same bar in absolute form over each system's rows). A tensor whose reference is
identically zero comes back identically zero. Every test prints its figures before it asserts. Without the
feature ``cell_tangents`` is not a keyword of the featuriser: every test here fails."""
import functools

import pytest
import torch

import _long_range_cell_oracle as co
import _long_range_train_oracle as lo
import _p3m_second_oracle as so2
import ewald_cases as ec
import gen_shapes as gs
from test_gpu_long_range_train import LR_KEYS, _check_rows, _check_tensors

pytestmark = pytest.mark.gpu

NODES = 5
METHODS = ["ewald", "p3m"]
CASES = [("odd33", "two_cells"), ("odd33", "model_batch"), ("residual", "box"), ("default", "box")]


def _setup(tag, which, method, cell_tangents=True):
    from metatrain_amd import long_range as lr
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    hypers, params = lo.model_case(tag)
    batch = co.batch_of(which)
    model = rt.HipModel(hypers, lo.eo.TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    graph = rt.HipGraph(model, batch["positions"].float().to(dev), batch["cells"].float().to(dev), batch["centers"].to(dev),
                        batch["neighbors"].to(dev), batch["cell_shifts"].to(dev), batch["species"].to(dev),
                        batch["system_indices"].int().to(dev))
    kw = dict(method="p3m", second_order=True) if method == "p3m" else {}
    feat = lr.LongRangeFeaturizerHip.from_state_dict(hypers, params, device=dev, cell_tangents=cell_tangents, **kw)
    return lr, dev, batch, model, graph, feat


def _check_tangents(label, batch, tan, ref, f32):
    """``tangent_atomic`` per system (an error confined to one system cannot hide under another's scale), each system's fp32
    yardstick under the cap; then the batch-wide figure, whose bar is returned for the sum."""
    for s in range(len(batch["first_atom"]) - 1):
        _, scale, e32, _ = ec.system_bar(ref["tangent"], f32["tangent"], ec.system_rows(batch, "atom", s))
        assert scale == 0.0 or e32 / scale <= gs.Y_CAP, (label, s, e32, scale)
    ec.check_per_system(label, batch, ["tangent_atomic"], ["atom"], [tan], [ref["tangent"]], [f32["tangent"]])
    return _check_rows(label, tan, ref["tangent"], f32["tangent"], "tangent_atomic")


def _reference(tag, which, method, with_u=True, with_cell=True):
    return co.reference_model(tag, which, NODES if method == "p3m" else 0, with_u, with_cell)


def _sweep(tag, which, method, with_u=True, with_cell=True, setup=None):
    lr, dev, batch, model, graph, feat = setup or _setup(tag, which, method)
    nu, u, uc = co.seeds(which)
    fw = lr.LongRangeForward(model, feat, graph, batch["pbcs"])
    model.zero_grad()
    tan = fw.backward_train2(torch.ones(len(nu), device=dev), nu.float().to(dev), u.float().to(dev) if with_u else None,
                             want_tangent=True, u_cell=uc.float().to(dev) if with_cell else None)
    return lr, dev, batch, model, graph, feat, fw, tan


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("tag,which", CASES)
def test_gradients_and_tangents_along_positions_and_cells(tag, which, method):
    """dJ/dtheta of ``J = <nu, e> + <u, dE/dR> + <u_cell, dE/dcell>`` per tensor, the six featuriser tensors among them, the
    per-atom tangents and their sum. ``two_cells``: two different cells around an open system (a per-system U indexed wrongly
    cannot pass it); ``model_batch``: an open cluster, a periodic box with an atom at a face, a QM9 frame."""
    ref, f32 = _reference(tag, which, method)
    lr, dev, batch, model, graph, feat, fw, tan = _sweep(tag, which, method)
    label = f"{method} {tag} {which} (u, u_cell)"
    _check_tensors(label, model.grads(), ref["grads"], f32["grads"])
    bar = _check_tangents(label, batch, tan, ref, f32)
    _, u, uc = co.seeds(which)
    n, scale = ref["tangent"].numel(), float(ref["tangent"].abs().max())
    total, want = float(tan.double().sum()), float((u * ref["grad"]).sum() + (uc * ref["cell_grad"]).sum())
    print(f"({label}, sum tangent, {total:.6e}, <u, dE/dR> + <u_cell, dE/dcell> {want:.6e})")
    assert abs(total - want) <= bar * n * scale


@pytest.mark.parametrize("method", METHODS)
def test_cell_direction_alone(method):
    """``d_u = NULL`` with ``d_u_cell`` given."""
    tag, which = "odd33", "two_cells"
    ref, f32 = _reference(tag, which, method, with_u=False)
    lr, dev, batch, model, graph, feat, fw, tan = _sweep(tag, which, method, with_u=False)
    label = f"{method} {tag} {which} (u_cell alone)"
    _check_tensors(label, model.grads(), ref["grads"], f32["grads"])
    _check_tangents(label, batch, tan, ref, f32)


@pytest.mark.parametrize("method", METHODS)
def test_without_a_cell_direction_and_without_a_periodic_system_nothing_changes(method):
    """``d_u_cell = NULL`` on the new C entry: the bits of ``pet_backward_train2_long_range`` (``backward_train2`` without
    ``u_cell``, which calls the entry that has no such argument) on the same handle and model. ``qm9_three`` (no
    periodic system) with a non-zero ``u_cell``: the bits of the run without it. Twice: the same bits."""
    tag, which = "odd33", "two_cells"
    nu, u, uc = co.seeds(which)
    setup = _setup(tag, which, method)
    lr, dev, batch, model, graph, feat = setup
    ones, nud, ud = torch.ones(len(nu), device=dev), nu.float().to(dev), u.float().to(dev)
    *_, fw, tan = _sweep(tag, which, method, setup=setup)
    flat = model.flat_grad().clone()
    *_, tan2 = _sweep(tag, which, method, setup=setup)
    assert torch.equal(flat, model.flat_grad()) and torch.equal(tan, tan2)
    # the C entry with d_u_cell = NULL against the entry that has no such argument
    from metatrain_amd import runtime as rt

    fw._plan()
    op = feat.ewald
    pos = graph._pos.detach().float().contiguous()
    need = int(model.lib.pet_train2_long_range_cell_workspace_bytes(model.handle, graph.handle, op.handle))
    assert need >= int(model.lib.pet_train2_long_range_workspace_bytes(model.handle, graph.handle, op.handle)) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    t_new = torch.empty(len(nu), device=dev)
    model.zero_grad()
    op._with_hook(ws, lambda: model.lib.pet_backward_train2_long_range_cell(
        model.handle, graph.handle, op.handle, rt._ptr(pos), rt._ptr(ws), ws.numel(), rt._ptr(ones), rt._ptr(nud), rt._ptr(ud), None,
        rt._ptr(t_new), rt._stream()))
    new = model.flat_grad().clone()
    model.zero_grad()
    t_old = fw.backward_train2(ones, nud, ud, want_tangent=True)
    assert torch.equal(new, model.flat_grad()) and torch.equal(t_new, t_old)
    # no periodic system: the cell direction has nothing to act on
    which = "qm9_three"
    nu, u, _ = co.seeds(which)
    setup = _setup(tag, which, method)
    lr, dev, batch, model, graph, feat = setup
    fw = lr.LongRangeForward(model, feat, graph, batch["pbcs"])
    ones, nud, ud = torch.ones(len(nu), device=dev), nu.float().to(dev), u.float().to(dev)
    model.zero_grad()
    t0 = fw.backward_train2(ones, nud, ud, want_tangent=True)
    g0 = model.flat_grad().clone()
    model.zero_grad()
    any_cells = torch.randn(graph.n_systems, 3, 3, generator=torch.Generator().manual_seed(9)).to(dev)
    t1 = fw.backward_train2(ones, nud, ud, want_tangent=True, u_cell=any_cells)
    assert torch.equal(g0, model.flat_grad()) and torch.equal(t0, t1)


# ---- the training step with a stress term -----------------------------------------------------------------------------------
TRAIN = ("odd33", "two_cells")


@functools.lru_cache(maxsize=None)
def _targets(method):
    """Energy, dE/dR and dE/d(strain) targets: the fp64 oracle's own values plus seeded offsets."""
    tag, which = TRAIN
    ref, _ = _reference(tag, which, method)
    b = co.batch_of(which)
    s = b["system_indices"].long()
    n_sys = len(b["first_atom"]) - 1
    n_atoms = torch.bincount(s, minlength=n_sys).double()
    e = torch.zeros(n_sys, dtype=torch.float64).index_add(0, s, ref["atomic"])
    gen = torch.Generator().manual_seed(99)
    pos, cells = b["positions"].double(), b["cells"].double()
    virial = torch.zeros(n_sys, 3, 3, dtype=torch.float64).index_add(0, s, pos[:, :, None] * ref["grad"][:, None, :])
    virial = virial + cells.transpose(1, 2) @ ref["cell_grad"]
    return (s, n_atoms, e + n_atoms * torch.tensor([0.04, -0.3, 0.2], dtype=torch.float64),
            ref["grad"] + 0.1 * torch.randn(ref["grad"].shape, generator=gen, dtype=torch.float64),
            virial + 0.5 * torch.randn(virial.shape, generator=gen, dtype=torch.float64))


def _loss(p, hypers, b, targets, dtype, huber_delta=None):
    """Energy per atom + dE/dR + dE/d(strain), the strain derivative formed the reference's way (``positions @ strain``,
    ``cell @ strain``); MSE each, or with ``huber_delta`` a Huber term on the strain gradients."""
    s, n_atoms, te, tg, ts = targets
    n_sys = len(n_atoms)
    strain = torch.eye(3, dtype=dtype).repeat(n_sys, 1, 1).requires_grad_(True)
    pos0 = b["positions"].to(dtype).clone().requires_grad_(True)
    pos = torch.einsum("na,nab->nb", pos0, strain[s])
    atomic = lo.atomic_energies(p, hypers, b, pos, b["cells"].to(dtype) @ strain)
    e = torch.zeros(n_sys, dtype=dtype).index_add(0, s, atomic)
    g, virial = torch.autograd.grad(e.sum(), [pos0, strain], create_graph=True)
    r = (e - te.to(dtype)) / n_atoms.to(dtype)
    d = virial - ts.to(dtype)
    stress = (d ** 2).mean() if huber_delta is None else torch.nn.functional.huber_loss(d, torch.zeros_like(d), delta=huber_delta)
    return (r ** 2).mean() + ((g - tg.to(dtype)) ** 2).mean() + stress


@functools.lru_cache(maxsize=None)
def _reference_steps(method, dtype, rate):
    """Three steps of clip_grad_norm_(1.0) + torch.optim.Adam on the oracle in ``dtype``: the losses before each step."""
    tag, which = TRAIN
    hypers, params = lo.model_case(tag)
    b = co.batch_of(which)

    def run():
        p = lo.leaves_of(params, dtype)
        leaves = [v for k, v in p.items() if k != "species_to_species_index"]
        opt = torch.optim.Adam(leaves, lr=rate)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = _loss(p, hypers, b, _targets(method), dtype)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(leaves, 1.0)
            opt.step()
            losses.append(float(loss.detach()))
        return losses

    if method == "p3m":
        with so2.mesh_operator(NODES):
            return run()
    return run()


@pytest.mark.parametrize("method", METHODS)
def test_training_steps_with_a_stress_term_follow_torch_adam_on_the_oracle(method):
    """Three steps of energy-per-atom + force + strain MSE against the same steps on the fp64 oracle at rate 3e-6, judged by
    the rule of ``test_training_steps_follow_torch_adam_on_the_oracle``; then one step under the ``loss`` hyper with a Huber
    stress term, whose featuriser gradients meet the bar; then frozen featuriser tensors stay bit-equal."""
    tag, which = TRAIN
    _targets(method)   # (the Ewald / mesh reference is formed outside the operator swap of the steps)
    lr, dev, batch, model, graph, feat = _setup(tag, which, method)
    hypers, _ = lo.model_case(tag)
    targets = _targets(method)
    s, n_atoms, te, tg, ts = targets
    rate = 3e-6
    ref_losses = _reference_steps(method, torch.float64, rate)
    f32_losses = _reference_steps(method, torch.float32, rate)
    step = lr.LongRangeTrainStep(model, feat, {"learning_rate": rate, "warmup_fraction": 0.0, "num_epochs": 10**9})
    fw = lr.LongRangeForward(model, feat, graph, batch["pbcs"])
    args = (graph, fw, te.float().to(dev), n_atoms.float().to(dev), tg.float().to(dev))
    kw = dict(target_strain_gradients=ts.float().to(dev), positions=batch["positions"].float().to(dev),
              cells=batch["cells"].float().to(dev))
    losses = []
    for _ in range(3):
        losses.append(float(step(*args, **kw)["loss"]))
        sd, fd = model.state_dict(), feat.state_dict()
        assert all(torch.equal(sd[k], fd[k]) for k in LR_KEYS)
    y = max(abs(a - b) / abs(b) for a, b in zip(f32_losses, ref_losses))
    err = max(abs(a - b) / abs(b) for a, b in zip(losses, ref_losses))
    print(f"({method} {tag} {which}, losses {losses}, oracle {ref_losses}, y {y:.2e}, relative deviation {err:.2e})")
    assert err <= max(5e-5, 2.0 * y)
    assert losses[-1] < losses[0] and ref_losses[-1] < ref_losses[0]
    # one more step under the `loss` hyper, Huber on the stress: the oracle's gradient of the same loss at the current state
    delta = 0.1
    state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    state["species_to_species_index"] = lo.model_case(tag)[1]["species_to_species_index"]
    b = co.batch_of(which)

    def want_of(dtype):
        p = lo.leaves_of(state, dtype)
        return [w.double() for w in torch.autograd.grad(_loss(p, hypers, b, targets, dtype, delta), [p[k] for k in LR_KEYS])]

    if method == "p3m":
        with so2.mesh_operator(NODES):
            want, want32 = want_of(torch.float64), want_of(torch.float32)
    else:
        want, want32 = want_of(torch.float64), want_of(torch.float32)
    term = {"type": "mse", "weight": 1.0}
    huber = lr.LongRangeTrainStep(model, feat, {
        "learning_rate": rate, "warmup_fraction": 0.0, "num_epochs": 10**9, "grad_clip_norm": 0.0,
        "loss": {"energy": {"type": "mse", "weight": 1.0,
                            "gradients": {"positions": term, "strain": {"type": "huber", "delta": delta, "weight": 1.0}}}}})
    out = huber(*args, **kw)
    assert torch.isfinite(torch.as_tensor(float(out["loss"])))
    got = {k: model.grad(k) for k in LR_KEYS}
    _check_tensors(f"{method} {tag} {which} huber stress", got, dict(zip(LR_KEYS, want)), dict(zip(LR_KEYS, want32)))
    # frozen featuriser tensors: no gradient, and a step leaves their bits alone
    model.set_trainable({k: False for k in LR_KEYS})
    before = model.state_dict()
    step(*args, **kw)
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in LR_KEYS)
    assert any(not torch.equal(before[k], after[k]) for k in before if k not in LR_KEYS)


def test_without_the_opt_in_the_stress_term_is_refused_as_before():
    from metatrain_amd._lib import PetHipError

    tag, which = TRAIN
    lr, dev, batch, model, graph, feat = _setup(tag, which, "ewald", cell_tangents=False)
    s, n_atoms, te, tg, ts = _targets("ewald")
    step = lr.LongRangeTrainStep(model, feat, {"learning_rate": 1e-6, "warmup_fraction": 0.0, "num_epochs": 10**9})
    fw = lr.LongRangeForward(model, feat, graph, batch["pbcs"])
    with pytest.raises(PetHipError, match="target_strain_gradients"):
        step(graph, fw, te.float().to(dev), n_atoms.float().to(dev), tg.float().to(dev),
             target_strain_gradients=ts.float().to(dev), positions=batch["positions"].float().to(dev),
             cells=batch["cells"].float().to(dev))
    with pytest.raises(PetHipError, match="u_cell"):
        fw.backward_train2(torch.ones(len(s), device=dev), None, None, u_cell=torch.zeros(3, 3, 3, device=dev))
