"""GPU tests for training further targets beside the energy on the native step (``TrainStep(extra_targets=...)``):
non-conservative forces ``[N, 3]``, non-conservative stress (per structure, ``process_non_conservative_stress``) and a
two-block per-atom target, through ``pet_train_predict`` / ``pet_train_predict_backward`` and ONE seeded backbone sweep.

Bar: every parameter's gradient within 1e-5 relative (max|d| / max|ref| per tensor) of torch's (double) backward through
the fp64 CPU oracle -- the bar of ``test_gpu_train.py``.
"""
import os

import numpy as np
import pytest
import torch

from oracle import pet as opet

from _memo import memo_oracle

pytestmark = pytest.mark.gpu

TOL = 1e-5
TYPES = [1, 6, 7, 8]
TARGETS = {"energy": 1, "non_conservative_forces": 3, "non_conservative_stress": 9, "multi": {"a": 3, "b": 6}}
WEIGHTS = {"energy": 1.0, "forces": 0.7, "non_conservative_forces": 0.6, "non_conservative_stress": 2.5, "multi": 0.3}
PER_STRUCTURE = ["non_conservative_stress"]


def _inputs(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "batch_two_systems.npz")))
    return {k[3:]: torch.tensor(v) for k, v in g.items() if k.startswith("in_")}


def _targets(inp):
    gen = torch.Generator().manual_seed(11)
    s = inp["system_indices"].long()
    n, n_sys = s.numel(), int(s.max()) + 1
    n_atoms = torch.bincount(s, minlength=n_sys).double()
    t = {
        "energy": torch.randn(n_sys, generator=gen, dtype=torch.float64) * n_atoms * 0.1,
        "forces": torch.randn((n, 3), generator=gen, dtype=torch.float64) * 0.1,
        "ncf": torch.randn((n, 3), generator=gen, dtype=torch.float64) * 0.1,
        "ncs": torch.randn((n_sys, 3, 3, 1), generator=gen, dtype=torch.float64) * 1e-3,
        "a": torch.randn((n, 3), generator=gen, dtype=torch.float64),
        "b": torch.randn((n, 3, 2), generator=gen, dtype=torch.float64),
    }
    t["ncs"][-1, 0, 1, 0] = float("nan")  # NaN entries are dropped from the loss
    t["b"][0] = float("nan")
    return t, n_atoms


def _nc_stress(p, cells, sys):  # backend.py process_non_conservative_stress, restated
    t = p.reshape(-1, 3, 3, p.shape[1] // 9)
    vol = torch.abs(torch.det(cells))
    vol[vol == 0.0] = torch.inf
    t = t / vol[sys][:, None, None, None]
    return ((t + t.transpose(1, 2)) / 2.0).reshape(p.shape[0], -1)


def _masked_mse(pred, target):
    pred, target = pred.reshape(-1), target.reshape(-1)
    m = ~torch.isnan(target)
    return ((pred[m] - target[m]) ** 2).mean()


@memo_oracle
def _oracle_grads(params, hypers, inp, with_energy, weights, per_structure=tuple(PER_STRUCTURE)):
    """The reference's loss: MSE(E / n) + MSE(dE/dR) + the three further targets, backward through the fp64 oracle."""
    p64 = {k: (v if k == "species_to_species_index" else v.double().clone().requires_grad_(True)) for k, v in params.items()}
    t, n_atoms = _targets(inp)
    s = inp["system_indices"].long()
    cells = inp["cells"].double()
    pos = inp["positions"].double().clone().requires_grad_(True)

    def run(target, block=None):
        return opet.pet_atomic_energies(p64, hypers, pos, cells, inp["centers"], inp["neighbors"], inp["cell_shifts"],
                                        inp["species"], s, target, block)

    loss = torch.zeros((), dtype=torch.float64)
    if with_energy:
        e = torch.zeros(len(n_atoms), dtype=torch.float64).index_add(0, s, run("energy")[:, 0])
        loss = loss + weights["energy"] * (((e - t["energy"]) / n_atoms) ** 2).mean()
        (g_r,) = torch.autograd.grad(e.sum(), pos, create_graph=True)
        loss = loss + weights["forces"] * ((g_r - t["forces"]) ** 2).mean()
    loss = loss + weights["non_conservative_forces"] * _masked_mse(run("non_conservative_forces"), t["ncf"])
    ncs = torch.zeros((len(n_atoms), 9), dtype=torch.float64).index_add(0, s, _nc_stress(run("non_conservative_stress"), cells, s))
    t_ncs = t["ncs"].reshape(len(n_atoms), 9)
    if "non_conservative_stress" not in per_structure:  # average_by_num_atoms: predictions and targets
        ncs, t_ncs = ncs / n_atoms[:, None], t_ncs / n_atoms[:, None]
    loss = loss + weights["non_conservative_stress"] * _masked_mse(ncs, t_ncs)
    pa, pb = run("multi", "a"), run("multi", "b")
    both_p, both_t = torch.cat([pa.reshape(-1), pb.reshape(-1)]), torch.cat([t["a"].reshape(-1), t["b"].reshape(-1)])
    loss = loss + weights["multi"] * _masked_mse(both_p, both_t)
    keys = [k for k in p64 if k != "species_to_species_index"]
    grads = torch.autograd.grad(loss, [p64[k] for k in keys], allow_unused=True)
    return float(loss.detach()), {k: (torch.zeros_like(p64[k]) if g is None else g) for k, g in zip(keys, grads)}


def _setup(golden_dir, target="energy", hypers_extra=None):
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    hypers = dict(opet.DEFAULT_HYPERS, **(hypers_extra or {}))
    targets = dict(TARGETS) if target == "energy" else {k: v for k, v in TARGETS.items() if k != "energy"}
    params = opet.synthetic_params(hypers, TYPES, targets, 0, torch.float32)
    inp = _inputs(golden_dir)
    model = rt.HipModel(hypers, TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, target)
    graph = rt.HipGraph(model, inp["positions"].float().to(dev), inp["cells"].float().to(dev), inp["centers"].to(dev),
                        inp["neighbors"].to(dev), inp["cell_shifts"].to(dev), inp["species"].to(dev),
                        inp["system_indices"].int().to(dev))
    fw = rt.HipForward(model, graph, train=True)
    return hypers, params, inp, model, graph, fw


def _extra(inp, dev, weights=WEIGHTS):
    t, _ = _targets(inp)
    f = {k: v.float().to(dev) for k, v in t.items()}
    return {
        "non_conservative_forces": {"values": f["ncf"], "weight": weights["non_conservative_forces"]},
        "non_conservative_stress": {"values": f["ncs"], "per_atom": False, "weight": weights["non_conservative_stress"]},
        "multi": {"values": {"a": f["a"], "b": f["b"]}, "weight": weights["multi"]},
    }


def _step(model, graph, fw, inp, with_energy=True, weights=WEIGHTS, per_structure=PER_STRUCTURE, **kw):
    from metatrain_amd.pet.trainer import TrainStep

    dev = torch.device("cuda:0")
    t, n_atoms = _targets(inp)
    step = TrainStep(model, {"loss_weights": dict(weights), "per_structure_targets": list(per_structure), "grad_clip_norm": 0.0,
                             "learning_rate": 0.0}, **kw)
    args = dict(graph=graph, fw=fw, n_atoms=n_atoms.float().to(dev), cells=inp["cells"].float().to(dev),
                extra_targets=_extra(inp, dev, weights))
    if with_energy:
        args.update(target_energies=t["energy"].float().to(dev), target_gradients=t["forces"].float().to(dev))
    else:
        args.update(target_energies=None)
    return step, args


def _compare(got, ref):
    assert set(got) == set(ref), set(got) ^ set(ref)
    worst = {}
    for k, r in ref.items():
        r = r.numpy()
        g = got[k].cpu().numpy().astype(np.float64)
        assert g.shape == r.shape, k
        scale = np.abs(r).max()
        err = np.abs(g - r).max()
        worst[k] = err / scale if scale > 1e-12 else err
    for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:10]:
        print(f"{v:.3e}  {k}")
    bad = {k: v for k, v in worst.items() if not v < TOL}
    assert not bad, f"parameter gradients off: {bad}"


@pytest.mark.parametrize("per_structure", [PER_STRUCTURE, []], ids=["stress_per_structure", "stress_averaged"])
def test_energy_forces_and_further_targets_match_oracle(golden_dir, per_structure):
    hypers, params, inp, model, graph, fw = _setup(golden_dir)
    step, args = _step(model, graph, fw, inp, per_structure=per_structure)
    out = step(**args)
    ref_loss, ref = _oracle_grads(params, hypers, inp, True, WEIGHTS, tuple(per_structure))
    assert abs(float(out["loss"]) - ref_loss) <= 1e-5 * abs(ref_loss)
    _compare(model.grads(), ref)


def test_further_targets_without_a_fused_target(golden_dir):
    """A model whose only targets are NC forces, NC stress and a two-block target (``load(..., target=None)``) trains
    through the first-order pass."""
    hypers, params, inp, model, graph, fw = _setup(golden_dir, target=None)
    step, args = _step(model, graph, fw, inp, with_energy=False)
    out = step(**args)
    assert out["energies"] is None
    ref_loss, ref = _oracle_grads(params, hypers, inp, False, WEIGHTS)
    assert abs(float(out["loss"]) - ref_loss) <= 1e-5 * abs(ref_loss)
    _compare(model.grads(), ref)


def test_zero_weight_extras_leave_backbone_bitwise_and_one_sweep(golden_dir):
    """Weight-0 further targets: every backbone gradient is bitwise the energy + forces step's, and the multi-target
    step launches the backbone's reverse stages exactly as often as the energy + forces step."""
    from metatrain_amd import runtime as rt

    hypers, params, inp, model, graph, fw = _setup(golden_dir)
    zero = dict(WEIGHTS, non_conservative_forces=0.0, non_conservative_stress=0.0, multi=0.0)
    rt.profile(True)
    step, args = _step(model, graph, fw, inp, weights=zero)
    step(**args)
    torch.cuda.synchronize()
    calls_multi = {r["name"]: r["calls"] for r in rt.profile_report()}
    g_multi = model.grads()
    rt.profile(True)
    del args["extra_targets"]
    step(**args)
    torch.cuda.synchronize()
    calls_plain = {r["name"]: r["calls"] for r in rt.profile_report()}
    rt.profile(False)
    g_plain = model.grads()
    heads = ("node_heads.", "edge_heads.", "node_last_layers.", "edge_last_layers.")
    for k, v in g_plain.items():
        if not k.startswith(heads) or ".energy." in k:
            assert torch.equal(v, g_multi[k]), k
    for name, c in calls_plain.items():  # (the further heads' own weight-gradient GEMMs are "wgrad" launches as well)
        if name != "wgrad":
            assert calls_multi.get(name) == c, (name, c, calls_multi.get(name))
    assert calls_multi["wgrad"] > calls_plain["wgrad"]


def test_two_identical_steps_are_bitwise_equal(golden_dir):
    hypers, params, inp, model, graph, fw = _setup(golden_dir)
    step, args = _step(model, graph, fw, inp)
    step(**args)
    first = {k: v.clone() for k, v in model.grads().items()}
    step(**args)  # learning rate 0: the parameters did not move
    for k, v in model.grads().items():
        assert torch.equal(v, first[k]), k


def test_microbatched_and_begin_end_match_one_batch(golden_dir):
    hypers, params, inp, model, graph, fw = _setup(golden_dir)
    step, args = _step(model, graph, fw, inp)
    step(**args)
    one = {k: v.clone() for k, v in model.grads().items()}
    step.begin(**args)
    step.end()
    for k, v in model.grads().items():
        assert torch.equal(v, one[k]), k
    # two micro-batches, one structure each: the whole step's shares and NaN-aware denominators
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    sys = inp["system_indices"].long()
    assert bool((sys[1:] >= sys[:-1]).all())
    batches = []
    for si in range(int(sys.max()) + 1):
        atoms = torch.nonzero(sys == si).squeeze(1)
        a0 = int(atoms[0])
        keep = (sys[inp["centers"].long()] == si)
        g_s = rt.HipGraph(model, inp["positions"][atoms].float().to(dev), inp["cells"][si:si + 1].float().to(dev),
                          (inp["centers"][keep] - a0).to(dev), (inp["neighbors"][keep] - a0).to(dev),
                          inp["cell_shifts"][keep].to(dev), inp["species"][atoms].to(dev),
                          torch.zeros(len(atoms), dtype=torch.int32, device=dev))
        sub = dict(graph=g_s, fw=rt.HipForward(model, g_s, train=True), n_atoms=args["n_atoms"][si:si + 1],
                   cells=args["cells"][si:si + 1], target_energies=args["target_energies"][si:si + 1],
                   target_gradients=args["target_gradients"][atoms.to(dev)])
        ex = args["extra_targets"]
        sub["extra_targets"] = {
            "non_conservative_forces": dict(ex["non_conservative_forces"], values=ex["non_conservative_forces"]["values"][atoms.to(dev)]),
            "non_conservative_stress": dict(ex["non_conservative_stress"], values=ex["non_conservative_stress"]["values"][si:si + 1]),
            "multi": dict(ex["multi"], values={b: v[atoms.to(dev)] for b, v in ex["multi"]["values"].items()}),
        }
        batches.append(sub)
    out = step.microbatched(batches)
    for k, v in model.grads().items():
        ref = one[k].cpu().numpy()
        np.testing.assert_allclose(v.cpu().numpy(), ref, rtol=0, atol=1e-5 * max(float(np.abs(ref).max()), 1e-12),
                                   err_msg=k)


def test_position_gradient_with_feature_seeds_is_refused(golden_dir):
    """The seeds carry no cutoff-factor adjoint: dL/dR of a loss with further targets is refused, not returned wrong."""
    from metatrain_amd._lib import PetHipError

    hypers, params, inp, model, graph, fw = _setup(golden_dir)
    model.zero_grad()
    fw.forward()
    ga = torch.ones((graph.n_nodes, 3), device="cuda:0")
    seeds = fw.train_predict_backward("non_conservative_forces", {"non_conservative_forces": ga})
    with pytest.raises(PetHipError, match="cutoff-factor"):
        fw.backward_train(None, want_position_grad=True, seed_features=seeds)


def test_heads_of_targets_absent_from_the_step_do_not_move(golden_dir):
    """torch's optimizer skips a parameter whose .grad is None: under AdamW, the heads of targets left out of a step's
    loss keep their values, while those in the loss move."""
    hypers, params, inp, model, graph, fw = _setup(golden_dir)
    step, args = _step(model, graph, fw, inp)
    step.hypers.update(learning_rate=1e-3, weight_decay=0.1, warmup_fraction=0.0)
    step(**args)  # every target: moments of every head become non-zero
    before = {k: model.param(k).clone() for k in model.head_keys()}
    args["extra_targets"] = {"non_conservative_forces": args["extra_targets"]["non_conservative_forces"]}
    step(**args)
    for k, (t, _) in model.head_keys().items():
        moved = not torch.equal(model.param(k), before[k])
        assert moved == (t in ("energy", "non_conservative_forces")), k
