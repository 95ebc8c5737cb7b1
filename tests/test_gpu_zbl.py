"""ZBL additive model on the GPU (csrc/zbl.hip, metatrain_amd/zbl.py, the exported wrappers) against the fp64 fixtures
``tests/golden/zbl_*.npz`` made from the reference's ``get_pairwise_zbl`` (``make_golden_zbl.py``) and against the fp64
restatement ``tests/zbl_ref.py``. The bar is the project's: relmax = max|a - b| / max|b| < 1e-5."""
import io
import os

import numpy as np
import pytest
import torch

import zbl_ref

pytestmark = pytest.mark.gpu
TOL = 1e-5
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["box_a", "box_a_sheared", "box_b", "one_atom", "qm9_compressed"]


def relmax(a, b, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = np.abs(b).max() if b.size else 0.0
    err = np.abs(a - b).max() if b.size else 0.0
    out = err / scale if scale > 0 else err  # an all-zero reference must be met exactly
    print(f"    relmax {what}: {out:.3e} (scale {scale:.4g})")
    return out


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from metatrain_amd import data, runtime
    from metatrain_amd.pet import default_hypers
    from metatrain_amd.zbl import ZBLHip

    class Env:
        dev = torch.device("cuda:0")
        rt = runtime
        _models = {}

        def graph_model(self, types, **delta):
            """A default-size PET model that only builds graphs (species table, no weights)."""
            key = (tuple(types), tuple(sorted(delta.items())))
            if key not in self._models:
                m = runtime.HipModel(dict(default_hypers(), **delta), list(types))
                m.load_species_table()
                self._models[key] = m
            return self._models[key]

        def fixture(self, name):
            return dict(np.load(os.path.join(GOLD, f"zbl_{name}.npz")))

        def systems(self, f, which=None):
            out = []
            for s in range(f["cells"].shape[0]) if which is None else which:
                sel = f["system_indices"] == s
                out.append((torch.tensor(f["positions"][sel], dtype=torch.float32).to(self.dev),
                            torch.tensor(f["numbers"][sel]).to(self.dev), torch.tensor(f["cells"][s], dtype=torch.float32),
                            tuple(bool(p) for p in f["pbc"][s])))
            return out

        def graph(self, model, systems):
            return data.graph_of(model, data.collate(systems, float(model.hypers["cutoff"])))

        def zbl(self, f):
            types = [int(z) for z in f["atomic_types"]]
            return ZBLHip(types, covalent_radii=dict(zip(types, f["radii"].tolist())))

    return Env()


def check_against_fixture(z, g, f):
    atomic = z.forward(g)
    gpos, gcell, gstrain = z.backward(g, want_cell_grad=True, want_strain=True)
    assert relmax(atomic.cpu(), f["atomic"], "atomic") < TOL
    assert relmax(gpos.cpu(), f["grad_positions"], "dE/dR") < TOL
    assert relmax(gcell.cpu(), f["grad_cells"], "dE/dcell") < TOL
    assert relmax(gstrain.cpu(), f["grad_strain"], "dE/deps") < TOL
    assert relmax(z.energies(g).cpu(), np.bincount(f["system_indices"], weights=f["atomic"]), "energies") < TOL
    return atomic, gpos, gcell, gstrain


@pytest.mark.parametrize("name", CASES)
def test_forward_and_backward_match_the_reference_fixture(env, name):
    """1. Per-atom energies, dE/dR, dE/dcell and the direct strain gradient on the graph of a default PET model (cutoff 4.5)."""
    f = env.fixture(name)
    z = env.zbl(f)
    g = env.graph(env.graph_model(z.atomic_types), env.systems(f))
    assert z.graph_for(g) is g  # the model's own graph serves
    atomic, gpos, gcell, gstrain = check_against_fixture(z, g, f)
    if name == "one_atom":  # six self-image edges: their two directions cancel exactly in dE/dR, add in the cell terms
        assert torch.equal(gpos, torch.zeros_like(gpos))
        assert float(gstrain.abs().max()) > 0.1 and float(gcell.abs().max()) > 0.1


def test_weighted_backward(env):
    """2. A random dL/d(atomic) on the sheared box against fp64 autograd of sum_i w_i a_i."""
    f = env.fixture("box_a_sheared")
    z = env.zbl(f)
    g = env.graph(env.graph_model(z.atomic_types), env.systems(f))
    w = torch.rand(f["positions"].shape[0], generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 2 - 0.5
    pos = torch.tensor(f["positions"], requires_grad=True)
    cells = torch.tensor(f["cells"], requires_grad=True)
    a = zbl_ref.atomic_energies(pos, cells, torch.tensor(f["system_indices"]).long(), torch.tensor(f["numbers"]).long(),
                                torch.tensor(f["radii_table"]), torch.tensor(f["pairs"]))
    rp, rc = torch.autograd.grad((w * a).sum(), [pos, cells])
    gpos, gcell = z.backward(g, w.float().to(env.dev), want_cell_grad=True)
    assert relmax(gpos.cpu(), rp, "weighted dL/dR") < TOL
    assert relmax(gcell.cpu(), rc, "weighted dL/dcell") < TOL
    with pytest.raises(env.rt.PetHipError, match="strain"):
        z.backward(g, w.float().to(env.dev), want_strain=True)


def _cluster(n, radius, dmin, seed):
    gen = torch.Generator().manual_seed(seed)
    pts = [torch.zeros(3, dtype=torch.float64)]
    while len(pts) < n:
        p = (torch.rand(3, generator=gen, dtype=torch.float64) * 2 - 1) * radius
        if float(p.norm()) < radius and float((torch.stack(pts) - p).norm(dim=1).min()) >= dmin:
            pts.append(p)
    return torch.stack(pts)


def test_rows_of_every_length(env):
    """3. One atom with more than 130 neighbours inside the ZBL cutoff (rows of more than 64 and more than 128 edges, the
    queue flushed several times inside one row), an atom with no edge, and a batch with no edge at all."""
    from metatrain_amd.zbl import ZBLHip

    radii = {1: 2.0, 6: 2.1}  # ZBL cutoff 4.2 inside the model's 4.5
    pos = torch.cat([_cluster(141, 4.1, 0.9, seed=2), torch.tensor([[50.0, 50.0, 50.0]], dtype=torch.float64)])
    numbers = torch.tensor([1, 6])[torch.randint(0, 2, (142,), generator=torch.Generator().manual_seed(4))]
    z = ZBLHip([1, 6], covalent_radii=radii)
    model = env.graph_model([1, 6])
    g = env.graph(model, [(pos.float().to(env.dev), numbers.to(env.dev), torch.zeros(3, 3), (False,) * 3)])
    rows = g.csr()["rowptr"].cpu()
    assert int(rows[1] - rows[0]) > 130 and int(rows[142] - rows[141]) == 0
    radii_of = torch.zeros(7, dtype=torch.float64)
    radii_of[1], radii_of[6] = 2.0, 2.1
    pairs = zbl_ref.brute_force_pairs(pos, torch.zeros(3, 3, dtype=torch.float64), 4.5, periodic=False)
    r = (pos[pairs[:, 1]] - pos[pairs[:, 0]]).norm(dim=1)
    inside_row0 = int(((pairs[:, 0] == 0) & (r <= radii_of[numbers[0]] + radii_of[numbers[pairs[:, 1]]])).sum())
    assert inside_row0 > 130, inside_row0
    p64 = pos.clone().requires_grad_(True)
    sysidx = torch.zeros(142, dtype=torch.long)
    a = zbl_ref.atomic_energies(p64, torch.zeros(1, 3, 3, dtype=torch.float64), sysidx, numbers, radii_of, pairs)
    (rp,) = torch.autograd.grad(a.sum(), [p64])
    strain = torch.eye(3, dtype=torch.float64)[None].clone().requires_grad_(True)
    a2 = zbl_ref.atomic_energies(pos, torch.zeros(1, 3, 3, dtype=torch.float64), sysidx, numbers, radii_of, pairs, strain)
    (rs,) = torch.autograd.grad(a2.sum(), [strain])
    atomic = z.forward(g)
    gpos, gcell, gstrain = z.backward(g, want_cell_grad=True, want_strain=True)
    assert relmax(atomic.cpu(), a.detach(), "cluster atomic") < TOL
    assert relmax(gpos.cpu(), rp, "cluster dE/dR") < TOL
    assert relmax(gstrain.cpu(), rs, "cluster dE/deps") < TOL
    assert float(atomic[141]) == 0.0 and torch.equal(gpos[141], torch.zeros(3, device=env.dev))
    assert torch.equal(gcell, torch.zeros_like(gcell))  # no periodic image: no cell term
    # no edge at all: zeros, nothing launched on an empty array
    far = torch.tensor([[0.0, 0.0, 0.0], [20.0, 0.0, 0.0]])
    g0 = env.graph(model, [(far.to(env.dev), torch.tensor([1, 6]).to(env.dev), torch.zeros(3, 3), (False,) * 3)])
    assert g0.n_edges == 0
    outs = [z.forward(g0), *z.backward(g0, want_cell_grad=True, want_strain=True),
            *z.backward(g0, torch.ones(2, device=env.dev), want_cell_grad=True)]
    assert [tuple(o.shape) for o in outs] == [(2,), (2, 3), (1, 3, 3), (1, 3, 3), (2, 3), (1, 3, 3)]
    assert all(torch.equal(o, torch.zeros_like(o)) for o in outs)


def test_two_systems_land_in_their_slots_bitwise(env):
    """4. A periodic system and one with a zero cell in one batch: every output equals, bit for bit, the system alone."""
    f = env.fixture("box_b")
    z = env.zbl(f)
    model = env.graph_model(z.atomic_types)
    periodic = env.systems(f)[0]
    molecule = (periodic[0][:9].clone(), periodic[1][:9].clone(), torch.zeros(3, 3), (False,) * 3)
    w = torch.rand(33, generator=torch.Generator().manual_seed(8)).to(env.dev)
    both = env.graph(model, [periodic, molecule])
    alone = [env.graph(model, [periodic]), env.graph(model, [molecule])]
    a = z.forward(both)
    gpos, gcell, gstrain = z.backward(both, want_cell_grad=True, want_strain=True)
    wpos, wcell = z.backward(both, w, want_cell_grad=True)
    for s, (lo, hi) in enumerate([(0, 24), (24, 33)]):
        assert torch.equal(a[lo:hi], z.forward(alone[s]))
        p1, c1, s1 = z.backward(alone[s], want_cell_grad=True, want_strain=True)
        assert torch.equal(gpos[lo:hi], p1) and torch.equal(gcell[s], c1[0]) and torch.equal(gstrain[s], s1[0])
        p2, c2 = z.backward(alone[s], w[lo:hi], want_cell_grad=True)
        assert torch.equal(wpos[lo:hi], p2) and torch.equal(wcell[s], c2[0])
    assert relmax(gstrain[0].cpu(), f["grad_strain"][0], "strain, periodic slot") < TOL
    assert torch.equal(gcell[1], torch.zeros(3, 3, device=env.dev)) and float(gstrain[1].abs().max()) > 0.1
    assert float(gcell[0].abs().max()) > 0.1


def test_outputs_repeat_bitwise(env):
    """5. No atomics, fixed summation orders: two calls give the same bits."""
    f = env.fixture("box_a_sheared")
    z = env.zbl(f)
    g = env.graph(env.graph_model(z.atomic_types), env.systems(f))
    w = torch.rand(48, generator=torch.Generator().manual_seed(5)).to(env.dev)
    first = [z.forward(g), *z.backward(g, want_cell_grad=True, want_strain=True), *z.backward(g, w, want_cell_grad=True)]
    for _ in range(3):
        again = [z.forward(g), *z.backward(g, want_cell_grad=True, want_strain=True), *z.backward(g, w, want_cell_grad=True)]
        assert all(torch.equal(x, y) for x, y in zip(first, again))


def test_stand_alone_graph_and_refusals(env):
    """6. A model at cutoff 2.0 with Cu present (ZBL needs 2.64), and an adaptive-cutoff model: ``graph_for`` builds a graph
    of its own at the ZBL cutoff; the model graphs themselves are refused."""
    f = env.fixture("box_a")
    z = env.zbl(f)
    short = env.graph(env.graph_model(z.atomic_types, cutoff=2.0, cutoff_width=0.4), env.systems(f))
    adaptive = env.graph(env.graph_model(z.atomic_types, num_neighbors_adaptive=8.0), env.systems(f))
    for g, message in ((short, "below the ZBL cutoff"), (adaptive, "adaptive")):
        with pytest.raises(env.rt.PetHipError, match=message):
            z.forward(g)
        with pytest.raises(env.rt.PetHipError, match=message):
            z.backward(g)
        with pytest.raises(env.rt.PetHipError, match="pbcs"):  # a HipGraph records no pbc, and a box is no evidence of one
            z.graph_for(g)
        own = z.graph_for(g, pbcs=[[True, True, True]])
        assert own is not g and float(own.model.hypers["cutoff"]) == pytest.approx(2.64)
        check_against_fixture(z, own, f)
    # the same from a plain batch
    s = env.systems(f)[0]
    own = z.graph_for({"positions": s[0], "cells": s[2][None], "species": s[1],
                       "system_indices": torch.zeros(48, dtype=torch.int32, device=env.dev), "pbcs": [s[3]]})
    check_against_fixture(z, own, f)
    # the same box declared non-periodic: no image pairs, so fewer edges than the periodic list
    open_box = z.graph_for(short, pbcs=[[False, False, False]])
    assert 0 < open_box.n_edges < own.n_edges


def _exported_inputs(env, f, cutoff=4.5):
    from metatrain_amd import data

    b = data.collate(env.systems(f), cutoff)
    return (b["positions"], b["cells"], b["centers"], b["neighbors"], b["cell_shifts"], b["species"], b["system_indices"])


@pytest.mark.parametrize("scripted", [False, True])
def test_exported_energy_model_with_zbl(env, scripted):
    """7. energies, forces, stress and per-atom energies = the same model without ZBL + the fixture's ZBL terms, with a scaler
    factor of 2 that must leave the ZBL term alone; selected_atoms; torch.jit.save / load.

    One graph per call: the graph build has no profile stage of its own, so what is pinned here is that a call runs ONE
    PET forward (``head_node``) and ONE ZBL launch each way (``zbl_fwd``, ``zbl_bwd``) -- the two terms are evaluated
    together, once. What is NOT pinned is the number of graph builds as such: a second build that launched none of these
    three stages would pass. That the two terms share one graph is a property of the code (the energy node of
    csrc/torch_ops.cpp hands its one ``GraphHolder`` to both), not of this count."""
    from metatrain_amd.pet import default_hypers, script
    from metatrain_amd.synthetic import synthetic_params

    f = env.fixture("box_a")
    types = [int(t) for t in f["atomic_types"]]
    hypers = default_hypers()
    params = synthetic_params(hypers, types, {"energy": 1}, 0, torch.float32)
    comp = torch.zeros(30)
    comp[types] = torch.tensor([-0.5, -37.8, -75.1, -16.4])
    plain = script.ExportedEnergyModel(script.make_core(hypers, types, params, "energy"), 2.0, comp)
    parts = script.make_core_and_zbl(dict(hypers, zbl=True), types, params, "energy")
    with_zbl = script.ExportedEnergyModel(parts.core, 2.0, comp, zbl=parts.zbl)
    if scripted:
        plain, with_zbl = torch.jit.script(plain), torch.jit.script(with_zbl)
    plain, with_zbl = plain.to(env.dev), with_zbl.to(env.dev)
    args = _exported_inputs(env, f)
    keep = (torch.arange(48) % 3 != 0).to(env.dev)
    e0, f0, s0, a0 = plain(*args, None, True)
    env.rt.profile(True)
    try:
        e1, f1, s1, a1 = with_zbl(*args, None, True)
        torch.cuda.synchronize()
        calls = {r["name"]: r["calls"] for r in env.rt.profile_report()}
    finally:
        env.rt.profile(False)
    assert calls["zbl_fwd"] == 1 and calls["zbl_bwd"] == 1 and calls["head_node"] == 1, calls
    vol = abs(np.linalg.det(f["cells"][0]))
    assert relmax(e1.cpu(), e0.cpu().double().numpy() + f["atomic"].sum(), "energy") < TOL
    assert relmax(a1.cpu(), a0.cpu().double().numpy() + f["atomic"], "per atom") < TOL
    assert relmax(f1.cpu(), f0.cpu().double().numpy() - f["grad_positions"], "forces") < TOL
    assert relmax(s1.cpu(), s0.cpu().double().numpy() + f["grad_strain"] / vol, "stress") < TOL
    # (a0 carries the scaler's factor 2 on the PET term only: had the ZBL term been scaled too, a1 would be off by 58 eV)
    # selected atoms: the mask applies to the ZBL per-atom energies as to the rest
    e2, f2, _, a2 = with_zbl(*args, keep, False)
    e3, f3, _, a3 = plain(*args, keep, False)
    k = keep.cpu().numpy()
    assert a2.shape[0] == int(k.sum())
    assert relmax(e2.cpu(), e3.cpu().double().numpy() + f["atomic"][k].sum(), "selected energy") < TOL
    assert relmax(a2.cpu(), a3.cpu().double().numpy() + f["atomic"][k], "selected per atom") < TOL
    pos = torch.tensor(f["positions"], requires_grad=True)
    a = zbl_ref.atomic_energies(pos, torch.tensor(f["cells"]), torch.zeros(48, dtype=torch.long),
                                torch.tensor(f["numbers"]).long(), torch.tensor(f["radii_table"]), torch.tensor(f["pairs"]))
    (g_sel,) = torch.autograd.grad(a[torch.tensor(k)].sum(), [pos])
    assert relmax(f2.cpu(), f3.cpu().double() - g_sel, "selected forces") < TOL
    if scripted:
        buf = io.BytesIO()
        torch.jit.save(with_zbl, buf)
        buf.seek(0)
        back = torch.jit.load(buf).to(env.dev)
        e4, f4, s4, a4 = back(*args, None, True)
        assert torch.equal(f4, f1) and torch.equal(a4, a1)  # what the library returns: the same bits
        # (energies and stress go through torch's index_add, whose float atomics may add in another order)
        assert relmax(e4.cpu(), e1.cpu(), "reloaded energy") < TOL and relmax(s4.cpu(), s1.cpu(), "reloaded stress") < TOL


def test_exported_llpr_model_mean_includes_zbl(env):
    """The LLPR wrapper: energies (the mean the ensemble is centred on) include ZBL; sigma and the ensemble's spread do not
    change (sigma: the same bits; the ensemble is the same rows re-centred on the new mean)."""
    from metatrain_amd.pet import default_hypers, script
    from metatrain_amd.synthetic import synthetic_params

    f = env.fixture("box_b")
    types = [int(t) for t in f["atomic_types"]]
    hypers = default_hypers()
    params = synthetic_params(hypers, types, {"energy": 1}, 0, torch.float32)
    F = 2 * hypers["d_head"]
    gen = torch.Generator().manual_seed(1)
    state = {"covariance_energy_uncertainty": torch.eye(F, dtype=torch.float64),
             "cholesky_energy_uncertainty": torch.eye(F, dtype=torch.float64) * 2.0,
             "multiplier_energy_uncertainty": torch.tensor([1.5], dtype=torch.float64),
             "llpr_ensemble_layers.energy.weight": torch.rand((8, F), generator=gen) * 0.01}
    plain = script.ExportedLLPRModel(script.make_core(hypers, types, params, "energy"), state).to(env.dev)
    parts = script.make_core_and_zbl(dict(hypers, zbl=True), types, params, "energy")
    with_zbl = torch.jit.script(script.ExportedLLPRModel(parts.core, state, zbl=parts.zbl)).to(env.dev)
    args = _exported_inputs(env, f)
    o0, o1 = plain(*args), with_zbl(*args)
    assert relmax(o1[0].cpu(), o0[0].cpu().double().numpy() + f["atomic"].sum(), "LLPR energy") < TOL
    assert relmax(o1[1].cpu(), o0[1].cpu().double().numpy() - f["grad_positions"], "LLPR forces") < TOL
    assert torch.equal(o1[4], o0[4])  # sigma
    assert relmax(o1[6].mean(1).cpu(), o1[0].cpu(), "ensemble mean") < TOL
    assert o1[6].shape == (1, 8)


def test_remove_from_targets_and_training_on_them(env):
    """8. The five compressed QM9 frames: targets - fixture; and one TrainStep on the removed targets equals, bit for bit, a
    TrainStep on targets from which the same numbers were subtracted by hand (the training path itself is untouched)."""
    from metatrain_amd.pet import default_hypers
    from metatrain_amd.pet.trainer import TrainStep
    from metatrain_amd.synthetic import synthetic_params

    f = env.fixture("qm9_compressed")
    z = env.zbl(f)
    types, hypers = z.atomic_types, default_hypers()
    params = {k: v.to(env.dev) for k, v in synthetic_params(hypers, types, {"energy": 1}, 0, torch.float32).items()}
    gen = torch.Generator().manual_seed(11)
    n = f["positions"].shape[0]
    energies = (torch.randn(5, generator=gen) * 3).to(env.dev)
    gradients = torch.randn((n, 3), generator=gen).to(env.dev)
    strain = torch.randn((5, 3, 3), generator=gen).to(env.dev)
    n_atoms = torch.tensor(np.bincount(f["system_indices"]), dtype=torch.float32).to(env.dev)

    def fresh():
        model = env.rt.HipModel(hypers, types)
        model.load(params, "energy")
        g = env.graph(model, env.systems(f))
        return model, g, env.rt.HipForward(model, g, train=True), TrainStep(
            model, {"learning_rate": 1e-3, "warmup_fraction": 0.0, "num_epochs": 10**9})

    model_a, g_a, fw_a, step_a = fresh()
    pos, cells = g_a._pos, g_a._cells
    e_r, g_r, s_r = z.remove_from_targets(g_a, pos, cells, energies, gradients, strain)
    assert relmax((energies - e_r).cpu(), np.bincount(f["system_indices"], weights=f["atomic"]), "removed energies") < TOL
    assert relmax((gradients - g_r).cpu(), f["grad_positions"], "removed dE/dR") < TOL
    assert relmax((strain - s_r).cpu(), f["grad_strain"], "removed dE/deps") < TOL
    assert z.remove_from_targets(g_a, pos, cells, energies)[1:] == (None, None)
    out_a = step_a(g_a, fw_a, e_r, n_atoms, g_r)
    model_b, g_b, fw_b, step_b = fresh()
    hand_e = energies - z.energies(g_b)
    hand_g = gradients - z.backward(g_b)
    out_b = step_b(g_b, fw_b, hand_e, n_atoms, hand_g)
    assert float(out_a["loss"]) == float(out_b["loss"])
    sa, sb = model_a.state_dict(), model_b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert any(not torch.equal(sa[k], params[k]) for k in sa if k != "species_to_species_index")  # a step was taken


def test_soap_bpnn_with_zbl(env):
    """9. SoapBpnnHip.evaluate on Box B: energies and dE/dR = the network's + the fixture's ZBL terms."""
    from oracle import soap as osoap

    from metatrain_amd.soap_bpnn import SoapBpnnHip

    f = env.fixture("box_b")
    types = [int(t) for t in f["atomic_types"]]
    hypers = dict(osoap.DEFAULT_HYPERS)
    params = {k: v.to(env.dev) for k, v in
              osoap.synthetic_params(hypers, len(types), osoap.basis(hypers)[0], 0, torch.float32).items()}
    plain, with_zbl = SoapBpnnHip(hypers, types), SoapBpnnHip(dict(hypers, zbl=True), types)
    for m in (plain, with_zbl):
        m.load(params)
    args = _exported_inputs(env, f, cutoff=float(hypers["soap"]["cutoff"]["radius"]))
    g = with_zbl.graph(*args)
    a0, p0, c0 = plain.evaluate(plain.graph(*args), want_cell_grad=True)
    a1, p1, c1 = with_zbl.evaluate(g, want_cell_grad=True)
    assert torch.equal(with_zbl.forward(g), a0)  # forward / backward stay the network alone: that is what trains
    assert relmax(a1.cpu(), a0.cpu().double().numpy() + f["atomic"], "SOAP-BPNN + ZBL atomic") < TOL
    assert relmax(p1.cpu(), p0.cpu().double().numpy() + f["grad_positions"], "SOAP-BPNN + ZBL dE/dR") < TOL
    assert relmax(c1.cpu(), c0.cpu().double().numpy() + f["grad_cells"], "SOAP-BPNN + ZBL dE/dcell") < TOL
