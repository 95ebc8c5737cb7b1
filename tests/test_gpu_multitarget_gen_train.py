"""GPU tests for training further targets (non-conservative forces and stress, a two-block target) on the SIZE-GENERIC
training pass (``csrc/gen_train.hip``): every model the tuned pass does not serve -- other sizes, PostLN layers, the residual
featuriser with its several readout layers -- and default-size models on a graph with a dense atom or without any edge.
Same recipe and bar as ``test_gpu_multitarget_train.py``: one step at learning rate 0, the loss and every parameter gradient
against torch's (double) backward through the fp64 oracle, 1e-5 relative (max|d| / max|ref| per tensor)."""
import numpy as np
import pytest
import torch

from oracle import pet as opet

from test_gpu_gen_train import CASES, LOOSE
from test_gpu_gen_train import _compare as _compare_folded
from test_gpu_multitarget_train import TARGETS, TOL, TYPES, WEIGHTS, _inputs, _oracle_grads, _step

pytestmark = pytest.mark.gpu

HEADS = ("node_heads.", "edge_heads.", "node_last_layers.", "edge_last_layers.")


def _setup(tag, inp, target="energy"):
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    hypers = dict(opet.DEFAULT_HYPERS, **({} if tag == "default" else CASES[tag]))
    targets = dict(TARGETS) if target == "energy" else {k: v for k, v in TARGETS.items() if k != "energy"}
    params = opet.synthetic_params(hypers, TYPES, targets, 0, torch.float32)
    model = rt.HipModel(hypers, TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, target)
    graph = rt.HipGraph(model, inp["positions"].float().to(dev), inp["cells"].float().to(dev), inp["centers"].to(dev),
                        inp["neighbors"].to(dev), inp["cell_shifts"].to(dev), inp["species"].to(dev),
                        inp["system_indices"].int().to(dev))
    return hypers, params, model, graph, rt.HipForward(model, graph, train=True)


def _compare(got, ref, what, tol=TOL):
    """Per tensor max|d| / max|ref| < tol; activation = "SiLU" holds w_in as [W; W], whose halves' gradients are summed
    (``test_gpu_gen_train._compare``)."""
    assert set(got) == set(ref), set(got) ^ set(ref)
    return _compare_folded(got, ref, None, what, tol)


def _check_step(tag, inp, with_energy=True, tol=TOL):
    hypers, params, model, graph, fw = _setup(tag, inp, "energy" if with_energy else None)
    step, args = _step(model, graph, fw, inp, with_energy=with_energy)
    # the gradients are read between the step's two halves: the optimizer half leaves the SUM of a tied projection's two
    # halves (activation = "SiLU") in both of them, which model.grads() would fold a second time
    step.begin(**args)
    got = model.grads()
    out = step.end()
    ref_loss, ref = _oracle_grads(params, hypers, inp, with_energy, WEIGHTS)
    print(f"{tag}: loss {float(out['loss']):.9e} oracle {ref_loss:.9e} rel {abs(float(out['loss']) - ref_loss) / abs(ref_loss):.2e}")
    _compare(got, ref, f"{tag} energy={with_energy}", tol)
    assert abs(float(out["loss"]) - ref_loss) <= 1e-5 * abs(ref_loss)
    return out, got, ref


@pytest.mark.parametrize("tag", ["flat32", "s64", "flat32_legacy", "default_postln", "default_residual", "s64_adaptive"])
def test_energy_forces_and_further_targets_match_oracle(golden_dir, tag):
    """Other sizes (d_node == d_pet included), PostLN, the residual featuriser (two readout layers: the prediction is the sum
    of the layers' heads, one dL/d(prediction) seeds both), LayerNorm + SiLU's tied halves, an adaptive cutoff."""
    _check_step(tag, _inputs(golden_dir))


def test_further_targets_without_a_fused_target(golden_dir):
    """``load(..., target=None)``: no fused head to run or to require; the sweep starts from the further targets' seeds."""
    out, _, _ = _check_step("flat32_legacy", _inputs(golden_dir), with_energy=False)
    assert out["energies"] is None


def test_minimal_model(golden_dir):
    """d_pet = 1: the degenerate model of ``test_gpu_gen_train.LOOSE`` (2e-3, from the reference's own fp32 arithmetic)."""
    _check_step("minimal", _inputs(golden_dir), tol=LOOSE["minimal"])


def _dense_inputs(cutoff):
    from oracle import nl as onl

    gen = torch.Generator().manual_seed(4)
    n = 132
    pos = torch.rand(n, 3, generator=gen, dtype=torch.float64) * 2.4   # the cube's diagonal, 4.16 A, is inside the cutoff
    cell = torch.eye(3, dtype=torch.float64) * 30.0
    z = torch.tensor(TYPES)[torch.randint(0, 4, (n,), generator=gen)]
    i, j, s, _ = onl.neighbor_list(pos.numpy(), cell.numpy(), [False] * 3, cutoff)
    assert np.bincount(i, minlength=n).max() > 127
    return {"positions": pos, "cells": cell[None], "centers": torch.tensor(i).long(), "neighbors": torch.tensor(j).long(),
            "cell_shifts": torch.tensor(s).long(), "species": z, "system_indices": torch.zeros(n, dtype=torch.long)}


def test_default_size_on_a_graph_with_more_than_127_neighbours():
    """132 atoms, each with 131 neighbours: the smallest graph that leaves the tuned pass at the default size."""
    _check_step("default", _dense_inputs(opet.DEFAULT_HYPERS["cutoff"]))


@pytest.mark.parametrize("tag", ["s64", "default"])
def test_batch_without_any_edge(tag):
    """The five isolated atoms of ``test_training_on_a_batch_of_isolated_atoms``: the node path alone carries gradients,
    every edge-side parameter -- the further targets' edge heads and last layers included -- gets exactly zero."""
    e0 = torch.zeros(0, dtype=torch.long)
    inp = {"positions": torch.tensor([[0.0, 0, 0], [40.0, 0, 0], [0, 40.0, 0], [0, 0, 40.0], [40.0, 40.0, 0]]),
           "cells": torch.zeros(3, 3, 3), "centers": e0, "neighbors": e0, "cell_shifts": torch.zeros((0, 3), dtype=torch.long),
           "species": torch.tensor([1, 6, 7, 8, 6]), "system_indices": torch.tensor([0, 0, 1, 2, 2])}
    _, got, ref = _check_step(tag, inp)
    zero_keys = [k for k in ref if float(ref[k].abs().max()) == 0.0]   # (the stress heads too: a zero cell counts as infinite)
    for t in ("energy", "multi", "non_conservative_forces"):
        assert any(k.startswith(f"edge_heads.{t}.") for k in zero_keys) and any(k.startswith(f"edge_last_layers.{t}.") for k in zero_keys)
    assert all(k in zero_keys for k in ref if k.startswith(("edge_heads.", "edge_last_layers.", "edge_embedder.")))
    assert all(float(got[k].abs().max()) == 0.0 for k in zero_keys)
    for t in ("energy", "multi", "non_conservative_forces"):
        assert all(float(got[k].abs().max()) > 0.0 for k in ref if k.startswith((f"node_heads.{t}.", f"node_last_layers.{t}.")))


def test_zero_weight_extras_leave_backbone_bitwise(golden_dir):
    """Weight-0 further targets against no further targets on the two-readout-layer model: every gradient outside the
    further targets' heads is bitwise equal (their seeds are zeros added to the adjoints the one sweep starts from). The
    size-generic pass has no profile scopes, so the stage counts of the tuned test have nothing to read here: bitwise
    equality is the whole assertion."""
    inp = _inputs(golden_dir)
    hypers, params, model, graph, fw = _setup("flat32_legacy", inp)
    zero = dict(WEIGHTS, non_conservative_forces=0.0, non_conservative_stress=0.0, multi=0.0)
    step, args = _step(model, graph, fw, inp, weights=zero)
    step(**args)
    g_multi = model.grads()
    del args["extra_targets"]
    step(**args)
    g_plain = model.grads()
    checked = 0
    for k, v in g_plain.items():
        if not k.startswith(HEADS) or ".energy." in k:
            assert torch.equal(v, g_multi[k]), k
            checked += 1
            assert float(v.abs().max()) > 0.0, k
    assert checked > 40


def test_two_identical_steps_are_bitwise_equal(golden_dir):
    inp = _inputs(golden_dir)
    hypers, params, model, graph, fw = _setup("default_residual", inp)
    step, args = _step(model, graph, fw, inp)
    step(**args)
    first = model.flat_grad().clone()
    step(**args)  # learning rate 0: the parameters did not move
    assert torch.equal(model.flat_grad(), first)
    assert float(first.abs().max()) > 0.0


def test_microbatched_matches_one_batch(golden_dir):
    """One structure per micro-batch: the whole step's shares and NaN-aware denominators, equal up to summation order."""
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    inp = _inputs(golden_dir)
    hypers, params, model, graph, fw = _setup("s64", inp)
    step, args = _step(model, graph, fw, inp)
    step(**args)
    one = {k: v.clone() for k, v in model.grads().items()}
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
        ex = args["extra_targets"]
        at = atoms.to(dev)
        batches.append(dict(
            graph=g_s, fw=rt.HipForward(model, g_s, train=True), n_atoms=args["n_atoms"][si:si + 1],
            cells=args["cells"][si:si + 1], target_energies=args["target_energies"][si:si + 1],
            target_gradients=args["target_gradients"][at],
            extra_targets={
                "non_conservative_forces": dict(ex["non_conservative_forces"], values=ex["non_conservative_forces"]["values"][at]),
                "non_conservative_stress": dict(ex["non_conservative_stress"], values=ex["non_conservative_stress"]["values"][si:si + 1]),
                "multi": dict(ex["multi"], values={b: v[at] for b, v in ex["multi"]["values"].items()}),
            }))
    step.microbatched(batches)
    for k, v in model.grads().items():
        ref = one[k].cpu().numpy()
        np.testing.assert_allclose(v.cpu().numpy(), ref, rtol=0, atol=1e-5 * max(float(np.abs(ref).max()), 1e-12), err_msg=k)


def test_refusals_are_kept(golden_dir):
    """The seeds carry no cutoff-factor adjoint, so dL/dR of a loss with further targets is refused on this pass too; a seed
    list that is not one pair per readout layer is refused."""
    from metatrain_amd._lib import PetHipError

    inp = _inputs(golden_dir)
    hypers, params, model, graph, fw = _setup("s64", inp)
    model.zero_grad()
    fw.forward()
    ga = torch.ones((graph.n_nodes, 3), device="cuda:0")
    seeds = fw.train_predict_backward("non_conservative_forces", {"non_conservative_forces": ga})
    with pytest.raises(PetHipError, match="cutoff-factor"):
        fw.backward_train(None, want_position_grad=True, seed_features=seeds)
    node, edge = seeds
    with pytest.raises(PetHipError, match="one seed pair per readout layer"):
        fw.backward_train(None, seed_features=([node, node], [edge, edge]))
    with pytest.raises(PetHipError):
        fw.train_predict("non_conservative_forces", readout_layer=1)


def test_idle_and_frozen_heads(golden_dir):
    """AdamW: heads of targets left out of a step do not move (torch skips a parameter without .grad); with the ``multi``
    heads frozen their gradients are exactly zero and every other gradient is bitwise what it was."""
    inp = _inputs(golden_dir)
    hypers, params, model, graph, fw = _setup("s64", inp)
    step, args = _step(model, graph, fw, inp)
    step(**args)  # learning rate 0
    free = {k: v.clone() for k, v in model.grads().items()}
    multi = [k for k, (t, _) in model.head_keys().items() if t == "multi"]
    assert any(k.startswith("edge_last_layers.") for k in multi) and any(k.startswith("node_heads.") for k in multi)
    model.set_trainable({k: False for k in multi})
    step(**args)
    for k, v in model.grads().items():
        if k in multi:
            assert float(v.abs().max()) == 0.0 and float(free[k].abs().max()) > 0.0, k
        else:
            assert torch.equal(v, free[k]), k
    model.set_trainable({k: True for k in multi})
    step.hypers.update(learning_rate=1e-3, weight_decay=0.1, warmup_fraction=0.0)
    step(**args)  # every target: moments of every head become non-zero
    before = {k: model.param(k).clone() for k in model.head_keys()}
    args["extra_targets"] = {"non_conservative_forces": args["extra_targets"]["non_conservative_forces"]}
    step(**args)
    for k, (t, _) in model.head_keys().items():
        moved = not torch.equal(model.param(k), before[k])
        assert moved == (t in ("energy", "non_conservative_forces")), k
