"""GPU tests of the size-generic PET pass (``csrc/gen_common.h``, ``gen.hip``, ``gen_train.hip``) at the widths its
kernels tile by: the cases, inputs and the one fp64 / fp32 oracle evaluation per (case, input) are ``tests/gen_shapes.py``
(each case is there for a named boundary: a head-dimension bucket of ``attn_dispatch``, a partial feature slice, the
scalar / 16-byte paths and the K / output tails of ``k_gen_lin`` and ``k_gt_wgrad``, the partly filled last block of the
row kernels, the multi-pass and 64-lane chunk loops of the attention kernels). Through ``metatrain_amd.runtime`` and the
C ABI.

Bar: ``relmax = max|got - ref| / max|ref| <= max(1e-5, 2 y)`` against the fp64 oracle, ``y`` the relmax of the fp32 oracle
against the fp64 oracle for the same quantity and input (per parameter tensor for parameter gradients; tensors without
signal absolutely); ``y <= 1e-3`` is asserted. No per-case constant. Every test prints ``(case, input, quantity, y,
relmax)``; the measured table is in DESIGN.md."""
import pytest
import torch

import gen_shapes as gs

pytestmark = pytest.mark.gpu


def _setup(tag, which):
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    hypers, params, inp, nu, u, w = gs.case(tag, which)
    model = rt.HipModel(hypers, gs.TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    graph = rt.HipGraph(model, inp["positions"].float().to(dev), inp["cells"].float().to(dev), inp["centers"].to(dev),
                        inp["neighbors"].to(dev), inp["cell_shifts"].to(dev), inp["species"].to(dev),
                        inp["system_indices"].int().to(dev))
    if "charge" in inp:
        graph.set_conditioning(inp["charge"].to(dev), inp["spin_multiplicity"].to(dev), inp["system_indices"].to(dev))
    ref, ys = gs.reference(tag, which)
    return rt, dev, hypers, model, graph, ref, ys, nu.to(dev), u.to(dev), w.to(dev)


def _check(tag, which, what, got, ref, y):
    e = gs.relmax(got, ref)
    print(f"({tag}, {which}, {what}, {y:.2e}, {e:.2e})")
    assert e <= gs.bar(y), (tag, which, what, e, y)


def _check_grads(tag, which, what, got, ref, ys):
    errs = {k: gs.tensor_err(got[k], r) for k, r in ref.items()}
    print(f"({tag}, {which}, {what}, {gs.worst(ys):.2e}, {max(errs.values()):.2e})")
    bad = {k: (e, ys[k]) for k, e in errs.items() if not e <= gs.bar(ys[k])}
    assert not bad, f"{tag} {which} {what}: parameter gradients off (relmax, y): {bad}"


def _staged(rt, model, graph, want_cell_grad):
    """calculate_features -> predict summed over read-out layers, and dE/dR (dE/dcell) through the adjoints of the three
    calls (``test_gpu_sizes._staged``)."""
    fw = rt.HipForward(model, graph)
    nfs, efs = fw.features_layers()
    atomic = sum(rt.predict(model, graph, nfs[l], efs[l], "energy", readout_layer=l) for l in range(len(nfs)))
    ones = torch.ones_like(atomic)
    g_nf, g_ef, g_fc = [], [], None
    for l in range(len(nfs)):
        a, b, c = rt.predict_backward(model, graph, nfs[l], efs[l], ones, "energy", readout_layer=l)
        g_nf.append(a)
        g_ef.append(b)
        g_fc = c if g_fc is None else g_fc + c
    geo, gfc = fw.backward_features_layers(g_nf, g_ef)
    out = fw.backward_geometry(geo, gfc + g_fc, want_cell_grad=want_cell_grad)
    return (atomic.reshape(-1),) + (tuple(out) if want_cell_grad else (out,))


@pytest.mark.parametrize("tag,which", gs.PAIRS)
def test_inference(tag, which):
    """Per-atom energies, dE/dR and (periodic input) dE/dcell through the staged calls and through the fused entry points."""
    rt, dev, hypers, model, graph, ref, ys, nu, u, w = _setup(tag, which)
    cell = which == "a"
    names = ("atomic", "grad") + (("cell_grad",) if cell else ())
    for q, got in zip(names, _staged(rt, model, graph, cell)):
        _check(tag, which, f"staged {q}", got, ref[q], ys[q])
    if hypers["featurizer_type"] != "residual":
        fw = rt.HipForward(model, graph)
        atomic = fw.forward()
        back = fw.backward(torch.ones_like(atomic), want_cell_grad=cell)
        for q, got in zip(names, (atomic,) + (tuple(back) if cell else (back,))):
            _check(tag, which, f"fused {q}", got, ref[q], ys[q])
        assert torch.equal(fw.forward(), atomic)


@pytest.mark.parametrize("tag,which", gs.PAIRS)
def test_energy_term_parameter_gradients(tag, which):
    rt, dev, hypers, model, graph, ref, ys, nu, u, w = _setup(tag, which)
    fw = rt.HipForward(model, graph, train=True)
    model.zero_grad()
    fw.forward()
    fw.backward_train(w)
    _check_grads(tag, which, "energy-term parameter gradients", model.grads(), ref["energy_grads"], ys["energy_grads"])


@pytest.mark.parametrize("tag,which", gs.PAIRS)
def test_force_loss_parameter_gradients(tag, which):
    rt, dev, hypers, model, graph, ref, ys, nu, u, w = _setup(tag, which)
    fw = rt.HipForward(model, graph, train=True)
    ones = torch.ones(graph.n_nodes, device=dev)
    flats = []
    for _ in range(2):
        model.zero_grad()
        fw.forward()
        gpos = fw.backward(ones)
        fw.backward_train2(ones, nu, u)
        flats.append(model.flat_grad().clone())
    _check(tag, which, "training-pass grad", gpos, ref["grad"], ys["grad"])
    _check_grads(tag, which, "force-loss parameter gradients", model.grads(), ref["force_grads"], ys["force_grads"])
    assert torch.equal(flats[0], flats[1])   # fixed summation orders, no float atomics


@pytest.mark.parametrize("tag,which", gs.PAIRS)
def test_hessian_vector_product(tag, which):
    rt, dev, hypers, model, graph, ref, ys, nu, u, w = _setup(tag, which)
    hp = rt.hessian_vector_product(model, graph, u)
    _check(tag, which, "hvp", hp, ref["hvp"], ys["hvp"])
    hp2, tan = rt.hessian_vector_product(model, graph, u, want_tangent=True)
    _check(tag, which, "hvp tangent", tan, ref["tangent"], ys["tangent"])
    assert torch.equal(hp2, hp)
    hp3, tan3 = rt.hessian_vector_product(model, graph, u, want_tangent=True)
    assert torch.equal(hp3, hp) and torch.equal(tan3, tan)
