"""GPU tests of the long-range PET's force-loss training sweep and Hessian-vector product THROUGH THE MESH OPERATOR
(``pet_backward_train2_long_range`` / ``pet_hessian_vector_long_range`` on a P3M-mode handle with a transform hook;
``LongRangeFeaturizerHip(..., method="p3m", second_order=True)``) against
``_long_range_train_oracle.evaluate`` under the operator swap of ``_p3m_oracle.model_reference`` (the P3M definition in place
of the Ewald one; ``evaluate``, not the cached ``reference``, which holds the Ewald results).

Bar (``gen_shapes.bar``): ``relmax = max|got - ref| / max|ref| <= max(1e-5, 2 y)`` with ``y`` the relmax of the fp32 oracle
against its fp64 self, an input counting only if ``y <= 1e-3``; per parameter tensor, and per system for position-shaped
results. A tensor whose reference is identically zero comes back identically zero. Every test prints its figures before it
asserts; the measured table is in DESIGN.md section 22."""
import functools

import pytest
import torch

import _long_range_train_oracle as lo
import _p3m_second_oracle as so2
import ewald_cases as ec
import gen_shapes as gs
from test_gpu_long_range_train import LR_KEYS, _check_rows, _check_tensors, _loss, _targets

pytestmark = pytest.mark.gpu

NODES = 5  # interpolation_nodes of the hypers of _long_range_train_oracle.model_case
CASES = [("odd33", "model_batch"), ("residual", "box"), ("default", "box")]


@functools.lru_cache(maxsize=None)
def _reference(tag, which, second_order=True):
    """(fp64, fp32) ``evaluate`` of a case on the mesh operator, computed once."""
    hypers, params = lo.model_case(tag)
    nu, u, _ = lo.seeds(which)
    b = lo.batch_of(which)
    d = u if second_order else None
    with so2.mesh_operator(NODES):
        return lo.evaluate(params, hypers, b, nu, d, torch.float64), lo.evaluate(params, hypers, b, nu, d, torch.float32)


def _check_hvp(label, batch, hu, ref, f32):
    """H u per system against the double backward. (A mesh breaks translation invariance, so unlike the Ewald sum's the rows
    of H u of a periodic system do not add up to zero; the oracle's do not either.)"""
    assert gs.relmax(f32["hvp"], ref["hvp"]) <= gs.Y_CAP
    ec.check_per_system(label, batch, ["hvp"], ["atom"], [hu], [ref["hvp"]], [f32["hvp"]])


def _setup(tag, which):
    from metatrain_amd import long_range as lr
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    hypers, params = lo.model_case(tag)
    assert int(hypers["long_range"]["interpolation_nodes"]) == NODES
    batch = lo.batch_of(which)
    model = rt.HipModel(hypers, lo.eo.TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    graph = rt.HipGraph(model, batch["positions"].float().to(dev), batch["cells"].float().to(dev), batch["centers"].to(dev),
                        batch["neighbors"].to(dev), batch["cell_shifts"].to(dev), batch["species"].to(dev),
                        batch["system_indices"].int().to(dev))
    feat = lr.LongRangeFeaturizerHip.from_state_dict(hypers, params, device=dev, method="p3m", second_order=True)
    assert isinstance(feat.ewald, lr.P3MHip)
    return lr, dev, batch, model, graph, feat


def _sweep2(tag, which):
    lr, dev, batch, model, graph, feat = _setup(tag, which)
    nu, u, _ = lo.seeds(which)
    fw = lr.LongRangeForward(model, feat, graph, batch["pbcs"])
    model.zero_grad()
    tan = fw.backward_train2(torch.ones(len(nu), device=dev), nu.float().to(dev), u.float().to(dev), want_tangent=True)
    return lr, dev, batch, model, graph, feat, fw, tan


@pytest.mark.parametrize("tag,which", CASES)
def test_second_order_gradients_tangents_and_hessian_vector_product(tag, which):
    """dJ/dtheta of J = <nu, e> + <u, dE/dR> per tensor (the six featuriser tensors among them), the tangents e' and H u per
    system. ``model_batch``: an open cluster, the 64-atom periodic box and a QM9 frame in one batch; ``box``: three periodic
    boxes. The hook runs inside both entry points: a sweep without a mesh would leave it uncalled."""
    ref, f32 = _reference(tag, which)
    lr, dev, batch, model, graph, feat, fw, tan = _sweep2(tag, which)
    assert feat.ewald.transform_calls > 0
    label = f"p3m {tag} {which}"
    _check_tensors(label, model.grads(), ref["grads"], f32["grads"])
    bar = _check_rows(label, tan, ref["tangent"], f32["tangent"], "tangent_atomic")
    n, scale = ref["tangent"].numel(), float(ref["tangent"].abs().max())
    total, want = float(tan.double().sum()), float((lo.seeds(which)[1] * ref["grad"]).sum())
    print(f"({label}, sum tangent, {total:.6e}, <u, dE/dR> {want:.6e})")
    assert abs(total - want) <= bar * n * scale
    u = lo.seeds(which)[1].float().to(dev)
    hu, tan2 = lr.hessian_vector_product(model, feat, graph, batch["pbcs"], u, want_tangent=True, replan=False)
    _check_hvp(label, batch, hu, ref, f32)
    _check_rows(label, tan2, ref["tangent"], f32["tangent"], "tangent_atomic (hvp)")
    # the first-order pair of the same featuriser is the operator the sweep differentiated
    atomic, _, gpos = lr.energy_and_gradient(model, feat, graph, batch["pbcs"], replan=False)
    _check_rows(label, atomic, ref["atomic"], f32["atomic"], "atomic")
    _check_rows(label, gpos, ref["grad"], f32["grad"], "grad")


def test_energy_only_gradients():
    """``u = NULL``: the first-order gradients of <nu, e>."""
    tag, which = "odd33", "model_batch"
    ref, f32 = _reference(tag, which, second_order=False)
    lr, dev, batch, model, graph, feat = _setup(tag, which)
    fw = lr.LongRangeForward(model, feat, graph, batch["pbcs"])
    model.zero_grad()
    fw.backward_train(lo.seeds(which)[0].float().to(dev))
    _check_tensors(f"p3m {tag} {which} energy only", model.grads(), ref["grads"], f32["grads"])


@pytest.mark.parametrize("which", ["qm9_three", "three"])
def test_small_open_batches_on_a_p3m_featuriser(which):
    """Edge-free rows in a batch, and a batch without any edge: open systems have no mesh, so the P3M handle serves them with
    the all-pairs kernels alone and the hook is never called."""
    tag = "odd33"
    ref, f32 = _reference(tag, which)
    lr, dev, batch, model, graph, feat, fw, tan = _sweep2(tag, which)
    label = f"p3m {tag} {which}"
    _check_tensors(label, model.grads(), ref["grads"], f32["grads"])
    _check_rows(label, tan, ref["tangent"], f32["tangent"], "tangent_atomic")
    hu = lr.hessian_vector_product(model, feat, graph, batch["pbcs"], lo.seeds(which)[1].float().to(dev), replan=False)
    _check_hvp(label, batch, hu, ref, f32)
    assert feat.ewald.transform_calls == 0
    assert float(hu.abs().max()) > 1e-5


@functools.lru_cache(maxsize=None)
def _reference_steps(tag, which, dtype, rate):
    """Three steps of clip_grad_norm_(1.0) + torch.optim.Adam on the mesh-operator oracle in ``dtype``: the losses before
    each step (``test_gpu_long_range_train._reference_steps`` under the operator swap)."""
    hypers, params = lo.model_case(tag)
    b = lo.batch_of(which)
    s, n_atoms, te, tg = _targets(which)   # (targets: the Ewald oracle's values plus offsets; any target would do)
    p = lo.leaves_of(params, dtype)
    leaves = [v for k, v in p.items() if k != "species_to_species_index"]
    opt = torch.optim.Adam(leaves, lr=rate)
    losses = []
    with so2.mesh_operator(NODES):
        for _ in range(3):
            opt.zero_grad()
            loss = _loss(p, hypers, b, s, n_atoms, te, tg, dtype)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(leaves, 1.0)
            opt.step()
            losses.append(float(loss.detach()))
    return losses


def test_training_steps_follow_torch_adam_on_the_oracle():
    """Three steps of energy-per-atom + force MSE through the mesh operator (zero_grad, forward, dE/dR, second-order sweep,
    clip, Adam) against the same steps on the oracle; the featuriser's copies follow the model's tensors."""
    tag, which = "odd33", "model_batch"
    lr, dev, batch, model, graph, feat = _setup(tag, which)
    s, n_atoms, te, tg = _targets(which)
    rate = 3e-6
    ref_losses = _reference_steps(tag, which, torch.float64, rate)
    f32_losses = _reference_steps(tag, which, torch.float32, rate)
    step = lr.LongRangeTrainStep(model, feat, {"learning_rate": rate, "warmup_fraction": 0.0, "num_epochs": 10**9})
    fw = lr.LongRangeForward(model, feat, graph, batch["pbcs"])
    args = (graph, fw, te.float().to(dev), n_atoms.float().to(dev), tg.float().to(dev))
    losses = []
    for _ in range(3):
        before = feat.state_dict()
        losses.append(float(step(*args)["loss"]))
        sd, fd = model.state_dict(), feat.state_dict()
        assert all(torch.equal(sd[k], fd[k]) for k in LR_KEYS)
        assert any(not torch.equal(before[k], fd[k]) for k in LR_KEYS)
    y = max(abs(a - b) / abs(b) for a, b in zip(f32_losses, ref_losses))
    err = max(abs(a - b) / abs(b) for a, b in zip(losses, ref_losses))
    print(f"(p3m {tag} {which}, losses {losses}, oracle {ref_losses}, y {y:.2e}, relative deviation {err:.2e})")
    assert err <= gs.bar(y)
    assert losses[-1] < losses[0] and ref_losses[-1] < ref_losses[0]


def test_frozen_featurizer():
    """``set_trainable`` turns the six keys off: every other tensor gets the same gradient bits, the six none."""
    tag, which = "odd33", "model_batch"
    lr, dev, batch, model, graph, feat, fw, tan = _sweep2(tag, which)
    free = model.grads()
    model.set_trainable({k: False for k in LR_KEYS})
    nu, u, _ = lo.seeds(which)
    model.zero_grad()
    fw.backward_train2(torch.ones(len(nu), device=dev), nu.float().to(dev), u.float().to(dev))
    frozen = model.grads()
    for k in free:
        if k in LR_KEYS:
            assert float(free[k].abs().max()) > 0.0 and float(frozen[k].abs().max()) == 0.0, k
        else:
            assert torch.equal(free[k], frozen[k]), k


def test_same_bits_run_to_run_and_alone_as_in_a_batch():
    tag, which = "odd33", "model_batch"
    lr, dev, batch, model, graph, feat, fw, tan = _sweep2(tag, which)
    flat = model.flat_grad().clone()
    nu, u, _ = lo.seeds(which)
    model.zero_grad()
    tan2 = fw.backward_train2(torch.ones(len(nu), device=dev), nu.float().to(dev), u.float().to(dev), want_tangent=True)
    assert torch.equal(flat, model.flat_grad()) and torch.equal(tan, tan2)
    ud = u.float().to(dev)
    hu = lr.hessian_vector_product(model, feat, graph, batch["pbcs"], ud, replan=False)
    assert torch.equal(hu, lr.hessian_vector_product(model, feat, graph, batch["pbcs"], ud, replan=False))
    # the periodic box alone: the same rows of H u as inside the batch
    a0, a1 = batch["first_atom"][1], batch["first_atom"][2]
    lr1, dev1, alone, model1, graph1, feat1 = _setup(tag, "box_alone")
    assert torch.equal(alone["positions"], batch["positions"][a0:a1])
    hu1 = lr1.hessian_vector_product(model1, feat1, graph1, alone["pbcs"], ud[a0:a1].contiguous())
    assert torch.equal(hu[a0:a1], hu1)


def test_a_handle_without_a_hook_is_still_refused():
    """The same featuriser without ``second_order=True``: Python refuses by name, and the library's workspace functions
    return -1 with the handle's mode in the message."""
    from metatrain_amd import long_range as lr

    tag, which = "odd33", "model_batch"
    _, dev, batch, model, graph, _ = _setup(tag, which)
    hypers, params = lo.model_case(tag)
    plain = lr.LongRangeFeaturizerHip.from_state_dict(hypers, params, device=dev, method="p3m")
    for build in (lambda: lr.LongRangeTrainStep(model, plain), lambda: lr.LongRangeForward(model, plain, graph, batch["pbcs"]),
                  lambda: lr.hessian_vector_product(model, plain, graph, batch["pbcs"], torch.zeros(graph.n_nodes, 3, device=dev))):
        with pytest.raises(lr.PetHipError, match="P3M featuriser.*second_order=True"):
            build()
    plain.plan(batch["cells"], batch["pbcs"], batch["first_atom"])
    for name in ("pet_train2_long_range_workspace_bytes", "pet_hvp_long_range_workspace_bytes"):
        assert getattr(model.lib, name)(model.handle, graph.handle, plain.ewald.handle) == -1
        assert "P3M-mode handle" in model.lib.pet_last_error().decode()
