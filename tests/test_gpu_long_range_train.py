"""GPU tests of the long-range PET's force-loss training sweep and Hessian-vector product
(``pet_backward_train2_long_range``, ``pet_hessian_vector_long_range``; ``metatrain_amd.long_range.LongRangeForward`` /
``LongRangeTrainStep`` / ``hessian_vector_product``) against the CPU oracle ``tests/_long_range_train_oracle.py``.

Bar (the fp32-floor rule of ``test_gpu_hvp.py``): ``relmax = max|got - ref| / max|ref| <= max(1e-5, 2 y)`` with ``y`` the
relmax of the fp32 oracle against its fp64 self, an input counting only if ``y <= 1e-3``; per parameter tensor, and per
system for position-shaped results (``ewald_cases.check_per_system``). A tensor whose reference is identically zero must
come back identically zero. Every test prints its figures before it asserts; the measured table is in DESIGN.md section 21.

On the parent commit the entry points do not exist and ``TrainStep`` raises for a long-range model: every test here fails."""
import functools
import math

import pytest
import torch

import _ewald_oracle as eo
import _long_range_train_oracle as lo
import ewald_cases as ec
import gen_shapes as gs

pytestmark = pytest.mark.gpu

CASES = [("odd33", "box"), ("odd33", "qm9"), ("odd33", "model_batch"), ("residual", "box"), ("residual", "qm9"), ("default", "box")]
LR_KEYS = tuple(lo.PRE + k for k in ("charges_map.weight", "charges_map.bias", "out_projection.0.weight", "out_projection.0.bias",
                                     "out_projection.2.weight", "out_projection.2.bias"))


def _setup(tag, which, params=None, hypers=None):
    from metatrain_amd import long_range as lr
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    h, p = lo.model_case(tag)
    hypers = hypers or h
    params = params or p
    batch = lo.batch_of(which)
    model = rt.HipModel(hypers, eo.TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    graph = rt.HipGraph(model, batch["positions"].float().to(dev), batch["cells"].float().to(dev), batch["centers"].to(dev),
                        batch["neighbors"].to(dev), batch["cell_shifts"].to(dev), batch["species"].to(dev),
                        batch["system_indices"].int().to(dev))
    feat = lr.LongRangeFeaturizerHip.from_state_dict(h, p, device=dev)
    return lr, rt, dev, batch, model, graph, feat


def _check_tensors(label, got, ref, f32):
    """The bar per parameter tensor; identically zero where the reference is."""
    bad, worst, worst_lr = [], (0.0, 0.0, ""), (0.0, 0.0, "")
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))
    for k, r in ref.items():
        g = got[k].detach().cpu().double()
        if float(r.abs().max()) == 0.0:
            if float(g.abs().max()) != 0.0:
                bad.append((k, "reference is zero", float(g.abs().max())))
            continue
        y, err = gs.tensor_err(f32[k], r), gs.tensor_err(g, r)
        if err > worst[0]:
            worst = (err, y, k)
        if k in LR_KEYS and err > worst_lr[0]:
            worst_lr = (err, y, k)
        if not err <= gs.bar(y):
            bad.append((k, err, y))
    print(f"[worst] {label} | parameter gradients | relmax {worst[0]:.1e} | y {worst[1]:.1e} | {worst[2]}")
    print(f"[worst] {label} | featuriser gradients | relmax {worst_lr[0]:.1e} | y {worst_lr[1]:.1e} | {worst_lr[2]}")
    assert not bad, (label, bad[:6])


def _check_rows(label, got, ref, f32, name):
    y, err = gs.relmax(f32, ref), gs.relmax(got, ref)
    print(f"({label}, {name}, {y:.2e}, {err:.2e})")
    assert err <= gs.bar(y), (label, name, err, y)
    return gs.bar(y)


def _sweep2(tag, which):
    lr, rt, dev, batch, model, graph, feat = _setup(tag, which)
    nu, u, _ = lo.seeds(which)
    fw = lr.LongRangeForward(model, feat, graph, batch["pbcs"])
    model.zero_grad()
    tan = fw.backward_train2(torch.ones(len(nu), device=dev), nu.float().to(dev), u.float().to(dev), want_tangent=True)
    return lr, dev, batch, model, graph, feat, fw, tan


@pytest.mark.parametrize("tag,which", CASES)
def test_second_order_gradients(tag, which):
    """dJ/dtheta of J = <nu, e> + <u, dE/dR> for every parameter tensor, the six featuriser tensors among them, the per-atom
    tangents e' and their sum <u, dE/dR>."""
    ref, f32 = lo.reference(tag, which)
    lr, dev, batch, model, graph, feat, fw, tan = _sweep2(tag, which)
    label = f"{tag} {which}"
    _check_tensors(label, model.grads(), ref["grads"], f32["grads"])
    bar = _check_rows(label, tan, ref["tangent"], f32["tangent"], "tangent_atomic")
    n, scale = ref["tangent"].numel(), float(ref["tangent"].abs().max())
    total, want = float(tan.double().sum()), float((lo.seeds(which)[1] * ref["grad"]).sum())
    print(f"({label}, sum tangent, {total:.6e}, <u, dE/dR> {want:.6e})")
    assert abs(total - want) <= bar * n * scale


def test_energy_only_gradients():
    """``u = NULL``: the first-order gradients of <nu, e>."""
    tag, which = "odd33", "model_batch"
    ref, f32 = lo.reference(tag, which, second_order=False)
    lr, rt, dev, batch, model, graph, feat = _setup(tag, which)
    fw = lr.LongRangeForward(model, feat, graph, batch["pbcs"])
    model.zero_grad()
    fw.backward_train(lo.seeds(which)[0].float().to(dev))
    _check_tensors(f"{tag} {which} energy only", model.grads(), ref["grads"], f32["grads"])


def _hvp(tag, which, direction="u"):
    lr, rt, dev, batch, model, graph, feat = _setup(tag, which)
    _, u, v = lo.seeds(which)
    d = (u if direction == "u" else v).float().to(dev)
    return lr, model, feat, graph, batch, d, lr.hessian_vector_product(model, feat, graph, batch["pbcs"], d, want_tangent=True)


def _check_hvp(label, batch, hu, ref, f32):
    """Per system against the double backward; sum_i (H u)_i = 0 per system within bar x N x max|H u|."""
    assert gs.relmax(f32["hvp"], ref["hvp"]) <= gs.Y_CAP
    ec.check_per_system(label, batch, ["hvp"], ["atom"], [hu], [ref["hvp"]], [f32["hvp"]])
    for s in range(len(batch["first_atom"]) - 1):
        rows = ec.system_rows(batch, "atom", s)
        bar, scale, _, _ = ec.system_bar(ref["hvp"], f32["hvp"], rows)   # (bar is absolute: max(1e-5 scale, 2 e32))
        total = hu[rows].detach().cpu().double().sum(0).abs().max()
        print(f"({label}, {s}, sum H u, {float(total):.2e}, allowed {bar * (rows.stop - rows.start):.2e})")
        assert float(total) <= bar * (rows.stop - rows.start)


@pytest.mark.parametrize("tag,which", CASES)
def test_hessian_vector_product(tag, which):
    """H u against the oracle's double backward, per system; translation invariance; <v, H u> = <u, H v>."""
    ref, f32 = lo.reference(tag, which)
    ref_v, f32_v = lo.reference(tag, which, direction="v")
    lr, model, feat, graph, batch, u, (hu, tan) = _hvp(tag, which)
    label = f"{tag} {which}"
    _check_hvp(label, batch, hu, ref, f32)
    _check_rows(label, tan, ref["tangent"], f32["tangent"], "tangent_atomic")
    _, _, v = lo.seeds(which)
    hv = lr.hessian_vector_product(model, feat, graph, batch["pbcs"], v.float().to(u.device), replan=False)
    bar_u, bar_v = gs.bar(gs.relmax(f32["hvp"], ref["hvp"])), gs.bar(gs.relmax(f32_v["hvp"], ref_v["hvp"]))
    # every component of H u is within bar_u max|H u| of the reference, whose Hessian is symmetric: the two products differ
    # by at most the sum of |v_i| (|u_i|) times those errors
    allowed = (bar_u * float(ref["hvp"].abs().max()) * float(v.abs().sum())
               + bar_v * float(ref_v["hvp"].abs().max()) * float(u.double().abs().sum()))
    a = float((v.to(hu.device) * hu.double()).sum())
    b = float((u.double() * hv.double()).sum())
    print(f"({label}, <v, H u> {a:.8e}, <u, H v> {b:.8e}, allowed {allowed:.2e})")
    assert abs(a - b) <= allowed


def test_edge_free_rows_in_a_batch():
    """The first QM9 frame and three open atoms about 6 A apart in one batch (N = 8, E = 20): the three atoms have no edge
    and still forces, a Hessian and a share in every gradient through K(d) = (1 - f) / d beyond the cutoff."""
    tag, which = "odd33", "qm9_three"
    batch = lo.batch_of(which)
    assert batch["positions"].shape[0] == 8 and len(batch["centers"]) == 20 and int(batch["centers"].max()) < 5
    ref, f32 = lo.reference(tag, which)
    lr, dev, batch, model, graph, feat, fw, tan = _sweep2(tag, which)
    _check_tensors(f"{tag} {which}", model.grads(), ref["grads"], f32["grads"])
    hu = lr.hessian_vector_product(model, feat, graph, batch["pbcs"], lo.seeds(which)[1].float().to(dev), replan=False)
    _check_hvp(f"{tag} {which}", batch, hu, ref, f32)
    assert float(ref["hvp"][5:].abs().max()) > 1e-5


def test_a_batch_without_any_edge():
    """The three atoms alone (E = 0) through the two new entry points: H u and the featuriser gradients are non-zero and
    within the bar (the dual pass' and the Hessian-vector product's edge-free exits are wrong with the long-range term)."""
    tag, which = "odd33", "three"
    assert len(lo.batch_of(which)["centers"]) == 0
    ref, f32 = lo.reference(tag, which)
    lr, dev, batch, model, graph, feat, fw, tan = _sweep2(tag, which)
    assert graph.n_edges == 0
    grads = model.grads()
    _check_tensors(f"{tag} {which}", grads, ref["grads"], f32["grads"])
    for k in LR_KEYS:
        assert float(ref["grads"][k].abs().max()) > 0.0 and float(grads[k].abs().max()) > 0.0, k
    _check_rows(f"{tag} {which}", tan, ref["tangent"], f32["tangent"], "tangent_atomic")
    hu = lr.hessian_vector_product(model, feat, graph, batch["pbcs"], lo.seeds(which)[1].float().to(dev), replan=False)
    _check_hvp(f"{tag} {which}", batch, hu, ref, f32)
    print(f"(three atoms, max|dE/dR| {float(ref['grad'].abs().max()):.2e}, max|H u| {float(ref['hvp'].abs().max()):.2e})")
    assert float(hu.abs().max()) > 1e-5


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
    # the periodic box alone: the same rows of H u as inside the batch (a direction is per atom, systems do not interact)
    a0, a1 = batch["first_atom"][1], batch["first_atom"][2]
    lr1, rt1, dev1, alone, model1, graph1, feat1 = _setup(tag, "box_alone")
    assert torch.equal(alone["positions"], batch["positions"][a0:a1])
    hu1 = lr1.hessian_vector_product(model1, feat1, graph1, alone["pbcs"], ud[a0:a1].contiguous())
    assert torch.equal(hu[a0:a1], hu1)


# ---- the training step ------------------------------------------------------------------------------------------------------
def _targets(which):
    """Energy and dE/dR targets: the fp64 oracle's own values plus seeded offsets (so the loss has something to reduce)."""
    ref, _ = lo.reference("odd33" if which == "model_batch" else "residual", which)
    b = lo.batch_of(which)
    s = b["system_indices"].long()
    n_sys = len(b["first_atom"]) - 1
    n_atoms = torch.bincount(s, minlength=n_sys).double()
    e = torch.zeros(n_sys, dtype=torch.float64).index_add(0, s, ref["atomic"])
    off = torch.tensor([0.04, -0.3, 0.2], dtype=torch.float64)[:n_sys]
    gen = torch.Generator().manual_seed(99)
    return s, n_atoms, e + n_atoms * off, ref["grad"] + 0.1 * torch.randn(ref["grad"].shape, generator=gen, dtype=torch.float64)


def _loss(p, hypers, b, s, n_atoms, te, tg, dtype, huber_delta=None):
    pos = b["positions"].to(dtype).clone().requires_grad_(True)
    atomic = lo.atomic_energies(p, hypers, b, pos, b["cells"].to(dtype))
    e = torch.zeros(len(n_atoms), dtype=dtype).index_add(0, s, atomic)
    (g,) = torch.autograd.grad(e.sum(), pos, create_graph=True)
    r = (e - te.to(dtype)) / n_atoms.to(dtype)
    if huber_delta is None:
        term = (r ** 2).mean()
    else:
        term = torch.nn.functional.huber_loss(r, torch.zeros_like(r), delta=huber_delta)
    return term + ((g - tg.to(dtype)) ** 2).mean()


@functools.lru_cache(maxsize=None)
def _reference_steps(tag, which, dtype, lr_rate):
    """Three steps of clip_grad_norm_(1.0) + torch.optim.Adam on the oracle in ``dtype``: the losses before each step."""
    hypers, params = lo.model_case(tag)
    b = lo.batch_of(which)
    s, n_atoms, te, tg = _targets(which)
    p = lo.leaves_of(params, dtype)
    leaves = [v for k, v in p.items() if k != "species_to_species_index"]
    opt = torch.optim.Adam(leaves, lr=lr_rate)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = _loss(p, hypers, b, s, n_atoms, te, tg, dtype)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(leaves, 1.0)
        opt.step()
        losses.append(float(loss.detach()))
    return losses


@pytest.mark.parametrize("tag,which", [("odd33", "model_batch"), ("residual", "box")])
def test_training_steps_follow_torch_adam_on_the_oracle(tag, which):
    """Three steps of energy-per-atom + force MSE (zero_grad, forward, dE/dR, second-order sweep, clip, Adam) against the
    same steps on the fp64 oracle; then one step under a Huber energy loss whose featuriser gradients meet the bar."""
    lr, rt, dev, batch, model, graph, feat = _setup(tag, which)
    hypers, _ = lo.model_case(tag)
    s, n_atoms, te, tg = _targets(which)
    rate = 3e-6   # (Adam's first steps move every parameter by the rate: at 1e-4 the oracle's own loss rises on these inputs)
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
    print(f"({tag} {which}, losses {losses}, oracle {ref_losses}, y {y:.2e}, relative deviation {err:.2e})")
    assert err <= max(5e-5, 2.0 * y)
    assert losses[-1] < losses[0] and ref_losses[-1] < ref_losses[0]
    # energy_and_gradient after the steps reads the updated tensors: it agrees with the oracle at the model's current state
    state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    state["species_to_species_index"] = lo.model_case(tag)[1]["species_to_species_index"]   # (not a parameter: the model keeps no copy)
    now = lo.evaluate(state, hypers, lo.batch_of(which), lo.seeds(which)[0], None, torch.float64)
    now32 = lo.evaluate(state, hypers, lo.batch_of(which), lo.seeds(which)[0], None, torch.float32)
    atomic, _, gpos = lr.energy_and_gradient(model, feat, graph, batch["pbcs"])
    start, _ = lo.reference(tag, which)
    for name, got in (("atomic", atomic), ("grad", gpos)):
        bar = gs.bar(gs.relmax(now32[name], now[name]))
        moved, off = gs.relmax(start[name], now[name]), gs.relmax(got, now[name])
        print(f"({tag} {which}, {name} moved by {moved:.2e} in three steps, now off by {off:.2e}, bar {bar:.1e})")
        assert off <= bar
        assert moved >= 10.0 * bar   # (the steps moved the model by far more than the bar: stale tensors would show)
    # one more step, Huber on the energy: the reference is the oracle's gradient of the same loss at the current state
    delta = 0.1
    p = lo.leaves_of(state, torch.float64)
    p32 = lo.leaves_of(state, torch.float32)
    b = lo.batch_of(which)
    want = torch.autograd.grad(_loss(p, hypers, b, s, n_atoms, te, tg, torch.float64, delta), [p[k] for k in LR_KEYS])
    want32 = torch.autograd.grad(_loss(p32, hypers, b, s, n_atoms, te, tg, torch.float32, delta), [p32[k] for k in LR_KEYS])
    huber = lr.LongRangeTrainStep(model, feat, {"learning_rate": rate, "warmup_fraction": 0.0, "num_epochs": 10**9,
                                                "grad_clip_norm": 0.0,
                                                "loss": {"energy": {"type": "huber", "delta": delta, "weight": 1.0,
                                                                    "gradients": {"positions": {"type": "mse", "weight": 1.0}}}}})
    out = huber(*args)
    assert math.isfinite(float(out["loss"]))
    got = {k: model.grad(k) for k in LR_KEYS}
    _check_tensors(f"{tag} {which} huber", got, dict(zip(LR_KEYS, (w.double() for w in want))),
                   dict(zip(LR_KEYS, (w.double() for w in want32))))


def test_frozen_featurizer():
    """``set_trainable`` turns the six keys off: every other tensor gets the same gradient bits, the six none, and a step
    leaves their bits alone."""
    tag, which = "odd33", "qm9"
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
    s, n_atoms, te, tg = _targets(which)
    step = lr.LongRangeTrainStep(model, feat, {"learning_rate": 1e-3, "warmup_fraction": 0.0, "num_epochs": 10**9})
    before = model.state_dict()
    step(graph, fw, te.float().to(dev), n_atoms.float().to(dev), tg.float().to(dev))
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in LR_KEYS)
    assert any(not torch.equal(before[k], after[k]) for k in before if k not in LR_KEYS)
    assert all(torch.equal(after[k], feat.state_dict()[k]) for k in LR_KEYS)


def test_refusals_on_the_device():
    tag, which = "odd33", "qm9"
    lr, rt, dev, batch, model, graph, feat = _setup(tag, which)
    hypers, params = lo.model_case(tag)
    s, n_atoms, te, tg = _targets(which)
    fw = lr.LongRangeForward(model, feat, graph, batch["pbcs"])
    args = (graph, fw, te.float().to(dev), n_atoms.float().to(dev), tg.float().to(dev))
    p3m = lr.LongRangeFeaturizerHip.from_state_dict(hypers, params, device=dev, method="p3m")
    with pytest.raises(lr.PetHipError, match="P3M featuriser"):
        lr.LongRangeTrainStep(model, p3m)
    p3m.plan(batch["cells"], batch["pbcs"], batch["first_atom"])
    assert model.lib.pet_train2_long_range_workspace_bytes(model.handle, graph.handle, p3m.ewald.handle) == -1
    assert "P3M-mode handle" in model.lib.pet_last_error().decode()
    step = lr.LongRangeTrainStep(model, feat)
    with pytest.raises(lr.PetHipError, match="target_strain_gradients"):
        step(*args, target_strain_gradients=torch.zeros(3, 3, 3, device=dev))
    with pytest.raises(lr.PetHipError, match="extra_targets"):
        step(*args, extra_targets={"non_conservative_forces": {"values": torch.zeros(12, 3, device=dev)}})
    with pytest.raises(lr.PetHipError, match="u_cell"):
        fw.backward_train2(torch.ones(12, device=dev), None, torch.zeros(12, 3, device=dev), u_cell=torch.zeros(3, 3, 3))
    with pytest.raises(lr.PetHipError, match="seed_features"):
        fw.backward_train(torch.ones(12, device=dev), seed_features=(None, None))
    # a handle planned for another batch
    other = lr.LongRangeFeaturizerHip.from_state_dict(hypers, params, device=dev)
    b2 = lo.batch_of("box")
    other.plan(b2["cells"], b2["pbcs"], b2["first_atom"])
    assert model.lib.pet_hvp_long_range_workspace_bytes(model.handle, graph.handle, other.ewald.handle) == -1
    assert "the plan" in model.lib.pet_last_error().decode()
    # a model loaded without the six tensors: by key, in Python and in the library
    bare = {k: v for k, v in params.items() if not k.startswith(lo.PRE)}
    lr2, rt2, dev2, batch2, model2, graph2, feat2 = _setup(tag, which, params=bare)
    with pytest.raises(lr.PetHipError, match="long_range_featurizer.charges_map.weight"):
        lr.LongRangeTrainStep(model2, feat2)
    model2.zero_grad()
    with pytest.raises(lr.PetHipError, match="long_range_featurizer.charges_map.weight"):
        lr.LongRangeForward(model2, feat2, graph2, batch["pbcs"]).backward_train(torch.ones(12, device=dev))
    with pytest.raises(lr.PetHipError, match="long_range_featurizer.charges_map.weight"):
        lr.hessian_vector_product(model2, feat2, graph2, batch["pbcs"], torch.zeros(12, 3, device=dev))
    # an adaptive-cutoff model
    adaptive = dict(hypers, num_neighbors_adaptive=8.0)
    lr3, rt3, dev3, batch3, model3, graph3, feat3 = _setup(tag, which, hypers=adaptive)
    with pytest.raises(lr.PetHipError, match="num_neighbors_adaptive"):
        lr.LongRangeTrainStep(model3, feat3)
    feat3.plan(batch["cells"], batch["pbcs"], batch["first_atom"])
    assert model3.lib.pet_train2_long_range_workspace_bytes(model3.handle, graph3.handle, feat3.ewald.handle) == -1
    assert "adaptive cutoff" in model3.lib.pet_last_error().decode()
    # the ordinary entry points keep refusing a long-range model
    from metatrain_amd.pet.trainer import TrainStep

    with pytest.raises(lr.PetHipError, match=r"training \(TrainStep\) of a long-range model"):
        TrainStep(model)
    with pytest.raises(lr.PetHipError, match="Hessian-vector product of a long-range model"):
        rt.hessian_vector_product(model, graph, torch.zeros(12, 3, device=dev))
