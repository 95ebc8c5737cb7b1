"""GPU tests of the long-range (Ewald) operator (``csrc/ewald.hip``) and of the whole long-range PET
(``metatrain_amd.long_range``) against the fp64 oracle of the definition (``tests/_ewald_oracle.py``).

Bar, per quantity: ``relmax = max|got - oracle| / max|oracle| <= max(1e-5, 2 e32)`` with ``e32`` the relmax of the same
oracle evaluated in fp32 on the host against its fp64 self (the factor 2 is the margin of DESIGN.md section 13: the kernels
sum in another order than torch's fp32). Every test prints ``(case, quantity, e32, relmax)`` before it asserts; the measured
table is in DESIGN.md section 18."""
import functools

import pytest
import torch

import _ewald_oracle as eo
import ewald_cases as ec
import gen_shapes as gs
from _memo import memo_oracle
from oracle import pet as opet

pytestmark = pytest.mark.gpu

SMEARING, RESOLUTION, CUTOFF = 1.4, 1.33, 4.5
QUANTITIES = ("potential", "grad_charges", "grad_positions", "grad_cells")


def _bar(e32):
    return max(1e-5, 2.0 * e32)


def _check(case, names, got, ref, f32):
    bad = []
    for name, g, r, y in zip(names, got, ref, f32):
        e32, err = eo.relmax(y, r), eo.relmax(g, r)
        print(f"({case}, {name}, {e32:.2e}, {err:.2e})")
        if not err <= _bar(e32):
            bad.append((name, err, e32))
    assert not bad, (case, bad)


def _lr_hypers(**extra):
    return ec.lr_hypers(SMEARING, RESOLUTION, **extra)


@functools.lru_cache(maxsize=None)
def _batch(name):
    return eo.collate(eo.mixed_batch(CUTOFF) if name == "mixed" else eo.small_cell(), CUTOFF)


@functools.lru_cache(maxsize=None)
def _charges(name, channels):
    g = torch.Generator().manual_seed(17 + channels)
    n = _batch(name)["positions"].shape[0]
    return torch.randn(n, channels, generator=g, dtype=torch.float64), torch.randn(n, channels, generator=g, dtype=torch.float64)


@memo_oracle
def _reference(batch, q, gv, dtype):
    return eo.operator_reference(batch, q, gv, SMEARING, RESOLUTION, CUTOFF, dtype)


# the model's graph of a batch, the planned operator on it and one run of it: shared with test_gpu_long_range_edges.py
_graph, _operator, _run = ec.graph, ec.operator, ec.run


@pytest.mark.parametrize("channels", [1, 24, 256])
def test_operator_on_a_mixed_batch(channels):
    """One batch of a 1-atom periodic cell, a triclinic 43-atom cell, a 130-atom cubic cell of L = 20 A and a 17-atom open
    cluster: potential and the three adjoints for a random dL/dV, at C = 1 (scalar loads), 24 and 256."""
    dev = torch.device("cuda:0")
    batch = _batch("mixed")
    q, gv = _charges("mixed", channels)
    model, graph, ew = _operator(batch, dev)
    assert ew.num_kvectors(2) > 4000 and ew.num_kvectors(3) == 0 and ew.num_kvectors(1) == len(eo.kvectors(batch["cells"][1], RESOLUTION))
    got = _run(ew, graph, batch, q, gv, dev)
    _check(f"mixed C={channels}", QUANTITIES, got, _reference(batch, q, gv, torch.float64), _reference(batch, q, gv, torch.float32))


def test_operator_on_a_cell_smaller_than_the_cutoff():
    """3 atoms, L = 4.0 A < R = 4.5 A: edges from an atom to its own images count in the potential and in dL/dcell and not
    in dL/dR."""
    dev = torch.device("cuda:0")
    batch = _batch("small")
    assert int((batch["centers"] == batch["neighbors"]).sum()) >= 18  # six nearest images per atom at least
    q, gv = _charges("small", 24)
    model, graph, ew = _operator(batch, dev)
    got = _run(ew, graph, batch, q, gv, dev)
    _check("small cell C=24", QUANTITIES, got, _reference(batch, q, gv, torch.float64), _reference(batch, q, gv, torch.float32))


def test_operator_is_deterministic_and_batch_independent():
    """The same call twice, and the 43-atom system alone against inside the batch: the same bits."""
    dev = torch.device("cuda:0")
    batch = _batch("mixed")
    q, gv = _charges("mixed", 24)
    model, graph, ew = _operator(batch, dev)
    a = _run(ew, graph, batch, q, gv, dev)
    b = _run(ew, graph, batch, q, gv, dev)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a0, a1 = batch["first_atom"][1], batch["first_atom"][2]
    alone = eo.collate([eo.mixed_batch(CUTOFF)[1]], CUTOFF)
    assert torch.equal(alone["positions"], batch["positions"][a0:a1])
    model1, graph1, ew1 = _operator(alone, dev)
    c = _run(ew1, graph1, alone, q[a0:a1], gv[a0:a1], dev)
    for name, x, y in zip(QUANTITIES[:3], a, c):
        assert torch.equal(x[a0:a1], y), name
    assert torch.equal(a[3][1], c[3][0])


def test_operator_refuses_graphs_it_cannot_serve():
    from metatrain_amd import long_range as lr
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    batch = _batch("small")
    q, _ = _charges("small", 24)
    pos = batch["positions"].float().to(dev)
    ew = lr.EwaldHip(SMEARING, RESOLUTION, CUTOFF).plan(batch["cells"], batch["pbcs"], batch["first_atom"])
    _, loose = _graph(batch, dev, hypers=dict(opet.DEFAULT_HYPERS))
    with pytest.raises(lr.PetHipError, match="nl_is_strict"):
        ew.potential(loose, pos, q.float().to(dev))
    model, strict = _graph(batch, dev)
    from_batch = rt.HipGraph.from_batch(model, strict.export_batch())
    with pytest.raises(lr.PetHipError, match="pet_graph_build handle"):
        ew.potential(from_batch, pos, q.float().to(dev))
    _, adaptive = _graph(batch, dev, hypers=_lr_hypers(num_neighbors_adaptive=8.0))
    with pytest.raises(lr.PetHipError, match="adaptive cutoff"):
        ew.potential(adaptive, pos, q.float().to(dev))


# ---- the whole model --------------------------------------------------------------------------------------------------------
MODELS = {
    "default": {},
    "odd33": gs.CASES["odd33"],
    "residual": dict(featurizer_type="residual"),
}


@functools.lru_cache(maxsize=None)
def _model_case(tag):
    hypers = _lr_hypers(**MODELS[tag])
    params = opet.synthetic_params(hypers, eo.TYPES, {"energy": 1}, 0, torch.float32)
    return hypers, params, eo.featurizer_params(hypers["d_node"], 0)


@functools.lru_cache(maxsize=None)
def _model_batch(which):
    return eo.periodic_box_batch(64, 3, CUTOFF) if which == "box" else eo.qm9_batch(3, CUTOFF)


@memo_oracle
def _model_reference(params, lr_params, hypers, batch, dtype):
    return eo.model_reference(params, lr_params, hypers, batch, dtype)


@pytest.mark.parametrize("which", ["box", "qm9"])
@pytest.mark.parametrize("tag", list(MODELS))
def test_long_range_model(tag, which):
    """Per-atom and per-system energies, dE/dR and dE/dcell of a long-range PET on a 64-atom periodic box and on the first
    QM9 frames: the default size (tuned path), a size-generic case and the residual featuriser (two readout layers)."""
    from metatrain_amd import long_range as lr
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    hypers, params, lr_params = _model_case(tag)
    batch = _model_batch(which)
    model = rt.HipModel(hypers, eo.TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    assert model.num_readout_layers() == (2 if tag == "residual" else 1)
    graph = rt.HipGraph(model, batch["positions"].float().to(dev), batch["cells"].float().to(dev), batch["centers"].to(dev),
                        batch["neighbors"].to(dev), batch["cell_shifts"].to(dev), batch["species"].to(dev),
                        batch["system_indices"].int().to(dev))
    feat = lr.LongRangeFeaturizerHip.from_state_dict(hypers, lr_params, device=dev)
    got = lr.energy_and_gradient(model, feat, graph, batch["pbcs"], want_cell_grad=True)
    ref = _model_reference(params, lr_params, hypers, batch, torch.float64)
    f32 = _model_reference(params, lr_params, hypers, batch, torch.float32)
    print(f"({tag} {which}: max|sum_l h_l| {ref[4][0]:.2e}, max|long-range features| {ref[4][1]:.2e})")
    names = ("atomic", "energies", "grad", "cell_grad")
    n = 4 if which == "box" else 3  # open systems: dE/dcell is zero, checked absolutely below
    _check(f"{tag} {which}", names[:n], got[:n], ref[:n], f32[:n])
    if which == "qm9":
        assert float(got[3].abs().max()) == 0.0
    again = lr.energy_and_gradient(model, feat, graph, batch["pbcs"], want_cell_grad=True, replan=False)
    assert all(torch.equal(x, y) for x, y in zip(got, again))


def test_models_without_long_range_are_untouched():
    """A model without ``long_range.enable`` through the old entry points: the fused and the staged path give the bits they
    gave (the staged composition of test_gpu_gen_shapes), and the long-range entry point refuses it."""
    from metatrain_amd import long_range as lr
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    hypers = dict(opet.DEFAULT_HYPERS)
    params = opet.synthetic_params(hypers, eo.TYPES, {"energy": 1}, 0, torch.float32)
    batch = _model_batch("box")
    model = rt.HipModel(hypers, eo.TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    graph = rt.HipGraph(model, batch["positions"].float().to(dev), batch["cells"].float().to(dev), batch["centers"].to(dev),
                        batch["neighbors"].to(dev), batch["cell_shifts"].to(dev), batch["species"].to(dev),
                        batch["system_indices"].int().to(dev))
    fw = rt.HipForward(model, graph)
    atomic = fw.forward()
    grad = fw.backward(torch.ones_like(atomic))
    p64 = {k: (v.double() if v.is_floating_point() else v) for k, v in params.items()}
    e_ref, g_ref, _ = opet.energy_and_gradient(p64, hypers, batch["positions"], batch["cells"], batch["centers"],
                                               batch["neighbors"], batch["cell_shifts"], batch["species"],
                                               batch["system_indices"])
    assert abs(float(atomic.double().sum()) - float(e_ref)) <= 1e-5 * abs(float(e_ref))
    assert eo.relmax(grad, g_ref) <= 1e-5
    fw2 = rt.HipForward(model, graph)
    assert torch.equal(fw2.forward(), atomic) and torch.equal(fw2.backward(torch.ones_like(atomic)), grad)
    with pytest.raises(lr.PetHipError, match="no long_range.enable"):
        lr.energy_and_gradient(model, None, graph, batch["pbcs"])
