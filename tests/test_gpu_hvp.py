"""GPU tests of the Hessian-vector product of the PET energy (``pet_hessian_vector``, ``csrc/gen_train.hip``;
``runtime.hessian_vector_product``, ``pet/hessian.py``, the differentiable backward of the exported energy op) against
torch's double backward through the fp64 oracle: ``grad(E_w, [R, cells], create_graph=True)`` then
``grad(<g_R, u> + <g_cell, u_cell>, [R, cells])`` with ``E_w = sum_i w_i e_i``.

Bar (the fp32-floor rule of ``tests/test_gpu_fp32_floor.py``): ``relmax = max|got - ref| / max|ref| <= max(1e-5, 2 y)``
where ``y`` is the relmax of the SAME oracle evaluated by torch in fp32 on the same inputs, computed here, per quantity;
an input only pins something if ``y <= 1e-3``. Measured ``(case, y, relmax)``: DESIGN.md, profiles/hvp_bench.json."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import nl as onl
from oracle import pet as opet
from test_gpu_gen_train import CASES
from test_gpu_train import _inputs

from _memo import memo_oracle

pytestmark = pytest.mark.gpu
TYPES = [1, 6, 7, 8]
HYPERS = {
    "default": {},
    "s64": CASES["s64"],
    "flat32_legacy": CASES["flat32_legacy"],
    "flat32_cosine": dict(CASES["flat32"], cutoff_function="Cosine"),
    "flat32_conditioned": dict(CASES["flat32"], system_conditioning=True),
}


def relmax(got, ref):
    ref = ref.double()
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def bar(y):
    assert y <= 1e-3, f"fp32 yardstick {y:.2e}: this input pins nothing"
    return max(1e-5, 2.0 * y)


@memo_oracle
def _oracle_hvp(params, hypers, inp, u, u_cell, weights, dtype):
    """(hvp_positions, hvp_cells, tangent_atomic) of the oracle in ``dtype``; tangent_i = d/dw_i of the contracted gradient."""
    p = {k: (v if k == "species_to_species_index" else v.to(dtype)) for k, v in params.items()}
    pos = inp["positions"].to(dtype).clone().requires_grad_(True)
    cells = inp["cells"].to(dtype).clone().requires_grad_(True)
    w = weights.to(dtype).clone().requires_grad_(True)
    kw = {k: inp[k] for k in ("charge", "spin_multiplicity") if k in inp}
    atomic = opet.pet_atomic_energies(p, hypers, pos, cells, inp["centers"], inp["neighbors"], inp["cell_shifts"],
                                      inp["species"], inp["system_indices"].long(), "energy", **kw)[:, 0]
    g_pos, g_cell = torch.autograd.grad((w * atomic).sum(), [pos, cells], create_graph=True)
    phi = (g_pos * u.to(dtype)).sum() + (g_cell * u_cell.to(dtype)).sum()
    hp, hc, tan = torch.autograd.grad(phi, [pos, cells, w])
    return hp.double(), hc.double(), tan.double()


def _reference(params, hypers, inp, u, u_cell, weights):
    """fp64 reference and the fp32 yardsticks (one per quantity)."""
    ref = _oracle_hvp(params, hypers, inp, u, u_cell, weights, torch.float64)
    f32 = _oracle_hvp(params, hypers, inp, u, u_cell, weights, torch.float32)
    return ref, [relmax(a, b) for a, b in zip(f32, ref)]


def _model_graph(hypers, params, inp, dev):
    from metatrain_amd import runtime as rt

    model = rt.HipModel(hypers, TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    graph = rt.HipGraph(model, inp["positions"].float().to(dev), inp["cells"].float().to(dev), inp["centers"].to(dev),
                        inp["neighbors"].to(dev), inp["cell_shifts"].to(dev), inp["species"].to(dev),
                        inp["system_indices"].int().to(dev))
    if "charge" in inp:
        graph.set_conditioning(inp["charge"].to(dev), inp["spin_multiplicity"].to(dev), inp["system_indices"].to(dev))
    return rt, model, graph


def _case(golden_dir, tag):
    hypers = dict(opet.DEFAULT_HYPERS, **HYPERS[tag])
    params = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    inp = _inputs(golden_dir, "batch_two_systems.npz")
    if hypers.get("system_conditioning"):
        inp["charge"], inp["spin_multiplicity"] = torch.tensor([-2, 3]), torch.tensor([1, 4])
    n, s = inp["positions"].shape[0], inp["cells"].shape[0]
    gen = torch.Generator().manual_seed(1)
    u = torch.randn(n, 3, generator=gen)
    u_cell = torch.randn(s, 3, 3, generator=gen) * 0.1
    weights = torch.rand(n, generator=gen) + 0.5
    return hypers, params, inp, u, u_cell, weights


@pytest.mark.parametrize("tag", list(HYPERS))
def test_hvp_matches_the_oracle_double_backward(golden_dir, tag):
    """hvp_positions, hvp_cells and tangent_atomic for a non-zero cell direction and non-uniform weights."""
    dev = torch.device("cuda:0")
    hypers, params, inp, u, u_cell, weights = _case(golden_dir, tag)
    ref, ys = _reference(params, hypers, inp, u, u_cell, weights)
    rt, model, graph = _model_graph(hypers, params, inp, dev)
    got = rt.hessian_vector_product(model, graph, u.to(dev), u_cell.to(dev), weights.to(dev), want_cells=True, want_tangent=True)
    errs = [relmax(g, r) for g, r in zip(got, ref)]
    print(f"hvp {tag}: (y, relmax) positions ({ys[0]:.2e}, {errs[0]:.2e}) cells ({ys[1]:.2e}, {errs[1]:.2e}) "
          f"tangent ({ys[2]:.2e}, {errs[2]:.2e})")
    for what, e, y in zip(("positions", "cells", "tangent"), errs, ys):
        assert e <= bar(y), (tag, what, e, y)
    # weights = None is ones, u_cell = None is a zero cell direction
    one = rt.hessian_vector_product(model, graph, u.to(dev))
    same = rt.hessian_vector_product(model, graph, u.to(dev), torch.zeros_like(u_cell).to(dev), torch.ones(len(weights), device=dev))
    assert torch.equal(one, same)


def dense_cluster(n_atoms=72, spacing=1.5, jitter=0.3, seed=3):
    """``n_atoms`` sites of a cubic lattice nearest to the origin, each moved by at most ``jitter`` per axis: the minimum
    distance is at least ``spacing - 2 sqrt(3) jitter`` = 0.46 A by construction and 0.8 A for this seed (asserted), and the
    whole cluster lies within one default cutoff (4.5 A) of its central atom, which therefore has ``n_atoms - 1`` neighbours."""
    k = np.arange(-4, 5)
    grid = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    order = np.lexsort((grid[:, 2], grid[:, 1], grid[:, 0], (grid ** 2).sum(1)))
    sites = grid[order[:n_atoms]] * spacing
    gen = torch.Generator().manual_seed(seed)
    pos = torch.tensor(sites) + (torch.rand(n_atoms, 3, generator=gen, dtype=torch.float64) * 2 - 1) * jitter
    pos[0] = 0.0
    z = torch.tensor(TYPES)[torch.randint(0, 4, (n_atoms,), generator=gen)]
    return pos, z


def test_an_atom_with_more_than_63_neighbours(golden_dir):
    """T > 64 tokens in the central rows: the 64-lane chunk loop of the attention adjoint, whose bias adjoints must be the
    complete sums over the queries of every chunk. Default size, non-periodic 72-atom cluster."""
    dev = torch.device("cuda:0")
    hypers = dict(opet.DEFAULT_HYPERS)
    params = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    pos, z = dense_cluster()
    n = len(z)
    i, j, s, _ = onl.neighbor_list(pos.numpy(), np.zeros((3, 3)), [False] * 3, hypers["cutoff"])
    d = np.linalg.norm(pos.numpy()[i] - pos.numpy()[j], axis=1)
    assert d.min() >= 0.8 and np.bincount(i, minlength=n).max() > 63 and np.bincount(i, minlength=n)[0] == n - 1
    inp = {"positions": pos, "cells": torch.zeros(1, 3, 3, dtype=torch.float64), "centers": torch.tensor(i).long(),
           "neighbors": torch.tensor(j).long(), "cell_shifts": torch.tensor(s).long(), "species": z,
           "system_indices": torch.zeros(n, dtype=torch.long)}
    gen = torch.Generator().manual_seed(1)
    u = torch.randn(n, 3, generator=gen)
    weights = torch.rand(n, generator=gen) + 0.5
    ref, ys = _reference(params, hypers, inp, u, torch.zeros(1, 3, 3), weights)
    rt, model, graph = _model_graph(hypers, params, inp, dev)
    assert graph.max_neighbors > 63
    hp, tan = rt.hessian_vector_product(model, graph, u.to(dev), None, weights.to(dev), want_tangent=True)
    errs = [relmax(hp, ref[0]), relmax(tan, ref[2])]
    print(f"hvp dense cluster: (y, relmax) positions ({ys[0]:.2e}, {errs[0]:.2e}) tangent ({ys[2]:.2e}, {errs[1]:.2e})")
    assert errs[0] <= bar(ys[0]) and errs[1] <= bar(ys[2]), (errs, ys)


def test_translation_invariance(golden_dir):
    """One direction for all atoms of a system: every edge tangent is exactly zero, and so is the result. Any direction:
    the forces' sum per system does not move, sum_i (H u)_i = 0 to rounding -- within the bar times N max|H u|."""
    dev = torch.device("cuda:0")
    hypers, params, inp, u, u_cell, weights = _case(golden_dir, "s64")
    rt, model, graph = _model_graph(hypers, params, inp, dev)
    sysidx = inp["system_indices"].long()
    rigid = torch.tensor([[0.3, -1.2, 0.7], [-2.0, 0.1, 0.4]])[sysidx]
    hp, tan = rt.hessian_vector_product(model, graph, rigid.to(dev), want_tangent=True)
    assert float(hp.abs().max()) == 0.0 and float(tan.abs().max()) == 0.0
    ones = torch.ones_like(weights)
    zero_cell = torch.zeros_like(u_cell)
    ref, ys = _reference(params, hypers, inp, u, zero_cell, ones)
    hu = rt.hessian_vector_product(model, graph, u.to(dev)).cpu().double()
    assert relmax(hu, ref[0]) <= bar(ys[0])
    for s in range(int(sysidx.max()) + 1):
        rows = hu[sysidx == s]
        assert float(rows.sum(0).abs().max()) <= bar(ys[0]) * len(rows) * float(hu.abs().max())


def test_degenerate_batches_and_refusals(golden_dir):
    from metatrain_amd import _lib

    dev = torch.device("cuda:0")
    hypers, params, inp, u, u_cell, weights = _case(golden_dir, "s64")
    rt, model, graph = _model_graph(hypers, params, inp, dev)
    # isolated atoms (no edge at all) and a system without atoms: zeros
    pos = torch.tensor([[0.0, 0, 0], [40.0, 0, 0], [0, 40.0, 0], [0, 0, 40.0], [40.0, 40.0, 0]])
    e0 = torch.zeros(0, dtype=torch.long)
    iso = rt.HipGraph(model, pos.to(dev), torch.zeros(4, 3, 3, device=dev), e0.to(dev), e0.to(dev),
                      torch.zeros((0, 3), dtype=torch.long, device=dev), torch.tensor([1, 6, 7, 8, 6]).to(dev),
                      torch.tensor([0, 0, 1, 3, 3]).int().to(dev))
    assert iso.n_edges == 0
    hp, hc, tan = rt.hessian_vector_product(model, iso, torch.randn(5, 3).to(dev), torch.randn(4, 3, 3).to(dev), None, True, True)
    assert hp.shape == (5, 3) and hc.shape == (4, 3, 3) and tan.shape == (5,)
    assert float(hp.abs().max()) == 0.0 and float(hc.abs().max()) == 0.0 and float(tan.abs().max()) == 0.0
    # the same bits run to run (fixed summation orders, no float atomics)
    a = rt.hessian_vector_product(model, graph, u.to(dev), u_cell.to(dev), weights.to(dev), True, True)
    b = rt.hessian_vector_product(model, graph, u.to(dev), u_cell.to(dev), weights.to(dev), True, True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # no gradient slot is needed (none of the calls above followed a zero_grad) or touched: cleared slots stay cleared
    model.zero_grad()
    rt.hessian_vector_product(model, graph, u.to(dev), u_cell.to(dev), weights.to(dev), True, True)
    assert float(model.flat_grad().abs().max()) == 0.0
    # a per-layer exchange on the graph: refused
    keep = _lib.EXCHANGE_FN(lambda user, direction, layer: 0)
    _lib.check(model.lib.pet_graph_set_exchange(graph.handle, None, 0, None, 0, None, None, keep, None))
    with pytest.raises(_lib.PetHipError, match=f"error {_lib.PET_ERR_UNSUPPORTED}: .*exchange"):
        rt.hessian_vector_product(model, graph, u.to(dev))
    # adaptive cutoffs: refused
    ah = dict(opet.DEFAULT_HYPERS, **CASES["s64_adaptive"])
    ap = opet.synthetic_params(ah, TYPES, {"energy": 1}, 0, torch.float32)
    _, amodel, agraph = _model_graph(ah, ap, inp, dev)
    with pytest.raises(_lib.PetHipError, match=f"error {_lib.PET_ERR_UNSUPPORTED}: .*adaptive"):
        rt.hessian_vector_product(amodel, agraph, u.to(dev))


def _methane(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "qm9_first5.npz")))
    return torch.tensor(g["pos0"]), torch.tensor(g["z0"])


@memo_oracle
def _oracle_hessian(params, hypers, pos, z, dtype):
    p = {k: (v if k == "species_to_species_index" else v.to(dtype)) for k, v in params.items()}
    n = len(z)
    i, j, s, _ = onl.neighbor_list(pos.numpy(), np.zeros((3, 3)), [False] * 3, hypers["cutoff"])
    i, j, s = torch.tensor(i).long(), torch.tensor(j).long(), torch.tensor(s).long()

    def energy(flat):
        return opet.pet_atomic_energies(p, hypers, flat.reshape(n, 3), torch.zeros(1, 3, 3, dtype=dtype), i, j, s, z,
                                        torch.zeros(n, dtype=torch.long), "energy")[:, 0].sum()

    return torch.autograd.functional.hessian(energy, pos.to(dtype).reshape(-1)).double()


def test_dense_hessian_of_a_molecule(golden_dir):
    """``hessian()`` on the first QM9 molecule, one column per launch and four replicas per launch: equal to each other,
    to ``torch.autograd.functional.hessian`` of the fp64 oracle, and symmetric -- all within the bar (of max|H|)."""
    from metatrain_amd.pet.hessian import hessian

    dev = torch.device("cuda:0")
    hypers = dict(opet.DEFAULT_HYPERS)
    params = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    pos, z = _methane(golden_dir)
    n = len(z)
    ref = _oracle_hessian(params, hypers, pos, z, torch.float64)
    y = relmax(_oracle_hessian(params, hypers, pos, z, torch.float32), ref)
    from metatrain_amd import runtime as rt

    model = rt.HipModel(hypers, TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    system = (pos.float().to(dev), z.to(dev), torch.eye(3) * 30.0, [False] * 3)   # (non-periodic: the cell is not used)
    h1 = hessian(model, system, hypers["cutoff"], columns_per_launch=1).cpu().double()
    h4 = hessian(model, system, hypers["cutoff"], columns_per_launch=4).cpu().double()
    assert h1.shape == (3 * n, 3 * n) == h4.shape
    scale = float(ref.abs().max())
    e1, e4 = relmax(h1, ref), relmax(h4, ref)
    print(f"dense Hessian: y {y:.2e}, relmax K=1 {e1:.2e}, K=4 {e4:.2e}, asymmetry {float((h4 - h4.T).abs().max()) / scale:.2e}")
    for col in range(3 * n):
        assert float((h1[col] - h4[col]).abs().max()) <= bar(y) * scale, col
    assert e1 <= bar(y) and e4 <= bar(y)
    assert float((h4 - h4.T).abs().max()) <= bar(y) * scale
    sub = hessian(model, system, hypers["cutoff"], atoms=[3, 1], columns_per_launch=4).cpu().double()
    assert torch.equal(sub, h4[[9, 10, 11, 3, 4, 5]])


def test_scripted_exported_model_differentiates_twice(golden_dir, tmp_path):
    """``torch.autograd.grad(<dE/dR, u> + <dE/dcell, u_cell>, [positions, cells])`` through the backbone of a scripted,
    saved and re-loaded ``ExportedEnergyModel`` is the C-ABI Hessian-vector product (the same kernels: the same bits, in
    fp32; 1e-6 allows for torch's reduction of the contracted gradient), eagerly too, and with the weights as
    ``grad_outputs`` the derivative w.r.t. them is the tangent. ``torch.autograd.functional.hvp`` works on it."""
    from metatrain_amd.pet import script

    dev = torch.device("cuda:0")
    hypers, params, inp, u, u_cell, weights = _case(golden_dir, "default")
    rt, model, graph = _model_graph(hypers, params, inp, dev)
    want = rt.hessian_vector_product(model, graph, u.to(dev), u_cell.to(dev), weights.to(dev), True, True)
    eager = script.ExportedEnergyModel(script.make_core(hypers, TYPES, {k: v.cpu() for k, v in params.items()}, "energy"))
    path = str(tmp_path / "energy.pt")
    torch.jit.save(torch.jit.script(eager), path)
    loaded = torch.jit.load(path)
    idx = [inp[k].to(dev) for k in ("centers", "neighbors", "cell_shifts", "species", "system_indices")]
    for mod in (loaded.pet, eager.pet):
        pos = inp["positions"].float().to(dev).requires_grad_(True)
        cells = inp["cells"].float().to(dev).requires_grad_(True)
        w = weights.to(dev).requires_grad_(True)
        atomic = mod(pos, cells, *idx)[:, 0]
        g_pos, g_cell = torch.autograd.grad((w * atomic).sum(), [pos, cells], create_graph=True)
        phi = (g_pos * u.to(dev)).sum() + (g_cell * u_cell.to(dev)).sum()
        got = torch.autograd.grad(phi, [pos, cells, w])
        for a, b in zip(got, want):
            assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())
    pos0, cells0 = inp["positions"].float().to(dev), inp["cells"].float().to(dev)
    _, hv = torch.autograd.functional.hvp(lambda p: loaded.pet(p, cells0, *idx).sum(), pos0, u.to(dev))
    ones = rt.hessian_vector_product(model, graph, u.to(dev))
    assert float((hv - ones).abs().max()) <= 1e-6 * float(ones.abs().max())


def test_training_pass_gradients_keep_their_bits(golden_dir):
    """The force-loss pass of the size-generic training path shares its sweep with the Hessian-vector mode: its flat
    parameter gradient (s64, batch_two_systems, the inputs of test_gpu_gen_train's force-loss test) still has the SHA-256
    recorded from a build of the commit before the Hessian-vector product was added. The pass is atomics-free."""
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    want = json.load(open(os.path.join(golden_dir, "gen_train_parent_digest.json")))
    hypers = dict(opet.DEFAULT_HYPERS, **CASES["s64"])
    params = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    inp = _inputs(golden_dir, "batch_two_systems.npz")
    _, model, graph = _model_graph(hypers, params, inp, dev)
    n = inp["positions"].shape[0]
    gen = torch.Generator().manual_seed(11)
    nu = torch.rand(n, generator=gen) - 0.5
    u = torch.randn(n, 3, generator=gen)
    fw = rt.HipForward(model, graph, train=True)
    model.zero_grad()
    fw.forward()
    ones = torch.ones(n, device=dev)
    fw.backward(ones)
    fw.backward_train2(ones, nu.to(dev), u.to(dev))
    flat = np.ascontiguousarray(model.flat_grad().cpu().numpy())
    assert flat.size == want["numel"]
    assert hashlib.sha256(flat.tobytes()).hexdigest() == want["sha256"]
