"""LLPR on the MI355X: the last-layer features of every readout layer against the reference (``pet_llpr.npz``), the four
kernels of csrc/llpr.hip against fp64 oracles, and ``LLPRUncertainty`` end to end."""
import os

import numpy as np
import pytest
import torch

from oracle import nl as onl
from oracle import pet as opet

pytestmark = pytest.mark.gpu
TYPES = [1, 6, 7, 8]
TOL = 1e-5


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from metatrain_amd import runtime

    return runtime


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / np.abs(b).max()


def _setup(rt, dev, golden_dir, fname, hypers, targets=None):
    from metatrain_amd.pet import llpr

    targets = targets or {"energy": 1}
    g = dict(np.load(os.path.join(golden_dir, fname)))
    params = {k: v.to(dev) for k, v in opet.synthetic_params(hypers, TYPES, targets, 0, torch.float32).items()}
    m = rt.HipModel(hypers, TYPES)
    m.load(params, "energy")
    t = lambda k, dt=None: torch.tensor(g[k]).to(dev) if dt is None else torch.tensor(g[k]).to(dev, dt)  # noqa: E731
    graph = rt.HipGraph(m, t("in_positions", torch.float32), t("in_cells", torch.float32), t("in_centers"),
                        t("in_neighbors"), t("in_cell_shifts"), t("in_species"), t("in_system_indices", torch.int32))
    u = llpr.LLPRUncertainty(m, params, {k: "system" for k in targets})
    return m, graph, u, params


@pytest.mark.parametrize("case,fname,delta", [
    ("two_systems", "batch_two_systems.npz", {}),
    ("box64", "pet_default_box64.npz", {}),
    ("residual_box64", "pet_variant_residual_box64.npz", {"featurizer_type": "residual"}),
])
def test_full_last_layer_features_match_the_reference(rt, dev, golden_dir, case, fname, delta):
    ref = np.load(os.path.join(golden_dir, "pet_llpr.npz"))
    hypers = dict(opet.DEFAULT_HYPERS, **delta)
    _, graph, u, _ = _setup(rt, dev, golden_dir, fname, hypers)
    atomic, llf = u.features(graph, targets=["energy"])["energy"]
    assert llf.shape == ref[f"llf_{case}"].shape == (graph.n_nodes, u.F)
    assert u.F == (512 if delta else 256)
    assert relmax(llf.cpu().numpy(), ref[f"llf_{case}"]) < TOL
    assert relmax(atomic.cpu().numpy(), ref[f"atomic_{case}"]) < TOL
    # layer 0 of the full LLF is what pet_aux_outputs returns for one readout layer
    if not delta:
        fw = rt.HipForward(u.model, graph)
        _, nf, ef = fw.forward(want_features=True)
        _, one = fw.aux_outputs(nf, ef, feature=False)
        assert relmax(llf.cpu().numpy(), one.cpu().numpy()) < TOL


def test_full_last_layer_features_size_generic_path(rt, dev):
    from metatrain_amd.pet import llpr

    hypers = dict(opet.DEFAULT_HYPERS, d_head=64, d_pet=64, d_node=128, d_feedforward=128, num_heads=4)
    params = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    pos, z, cell = opet.random_box(97, 23)
    i, j, s, _ = onl.neighbor_list(pos.numpy(), cell.numpy(), [True] * 3, hypers["cutoff"])
    i, j, s = torch.tensor(i), torch.tensor(j), torch.tensor(s)
    sysidx = torch.zeros(len(pos), dtype=torch.int32)
    m = rt.HipModel(hypers, TYPES)
    m.load({k: v.to(dev) for k, v in params.items()}, "energy")
    graph = rt.HipGraph(m, pos.to(dev), cell[None].to(dev), i.to(dev), j.to(dev), s.to(dev), z.to(dev), sysidx.to(dev))
    u = llpr.LLPRUncertainty(m, {k: v.to(dev) for k, v in params.items()}, {"energy": "system"})
    assert u.F == 128
    _, llf = u.features(graph, targets=["energy"])["energy"]
    p64 = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float64)
    _, _, llf64 = opet.pet_atomic_energies(p64, hypers, pos.double(), cell[None].double(), i, j, s.long(), z,
                                           sysidx.long(), return_aux=True)
    assert relmax(llf.cpu().numpy(), llf64.numpy()) < TOL


def _rows(n, F, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, F, generator=g, dtype=torch.float64) * 0.5 + torch.rand(F, generator=g, dtype=torch.float64)
    return x.to(dev, torch.float32)


@pytest.mark.parametrize("R,featurizer", [(8, "feedforward"), (10000, "feedforward"), (3001, "residual")])
def test_covariance_matches_fp64_and_is_reproducible(rt, dev, R, featurizer):
    from metatrain_amd.pet import llpr

    hypers = dict(opet.DEFAULT_HYPERS, featurizer_type=featurizer)
    m = rt.HipModel(hypers, TYPES)
    u = llpr.LLPRUncertainty.__new__(llpr.LLPRUncertainty)
    u.model, u.lib, u.dev = m, m.lib, dev
    u.F = int(m.lib.pet_llpr_feature_size(m.handle))
    x = _rows(R, u.F, 1, dev)
    C = torch.zeros((u.F, u.F), dtype=torch.float64, device=dev)
    u.accumulate(x, C)
    u.finalize(C)
    x64 = x.double()
    C64 = x64.T @ x64
    err = float((C - C64).abs().max() / C64.abs().max())
    err_t = float(((x.T @ x).double() - C64).abs().max() / C64.abs().max())
    assert err < TOL and err <= 2 * err_t + 2.0 ** -23, (err, err_t)  # (fp32 epsilon: both exact-ish on 8 rows)
    assert torch.equal(C, C.T)
    C2 = torch.zeros_like(C)
    u.accumulate(x, C2)
    u.finalize(C2)
    assert torch.equal(C, C2)  # the same bits on a repeat
    C3 = torch.zeros_like(C)
    for lo in range(0, R, 777):  # micro-batches
        u.accumulate(x[lo:lo + 777], C3)
    u.finalize(C3)
    assert float((C3 - C).abs().max() / C.abs().max()) < 1e-6


@pytest.mark.parametrize("R", [8, 10000])
def test_variance_matches_fp64(rt, dev, R):
    from metatrain_amd.pet import llpr

    m = rt.HipModel(dict(opet.DEFAULT_HYPERS), TYPES)
    u = llpr.LLPRUncertainty.__new__(llpr.LLPRUncertainty)
    u.model, u.lib, u.dev = m, m.lib, dev
    u.F = F = 256
    train = _rows(20000, F, 2, dev).double().cpu()
    cov = train.T @ train
    x = _rows(R, F, 3, dev)
    x64 = x.double().cpu()
    for reg in (1e-3 * float(cov.diagonal().mean()), None):
        L, r = llpr.cholesky_ladder(cov, reg)
        M = torch.tril(torch.linalg.solve_triangular(L, torch.eye(F, dtype=torch.float64), upper=False))
        want = torch.sqrt(((M @ x64.T) ** 2).sum(0)) * 0.75
        got = u.sigma(x, M.to(dev, torch.float32), 0.75).double().cpu()
        err = float(((got - want).abs() / want).max())
        if reg is not None:
            assert err < TOL, err
        else:  # the reference's own fp32 evaluation: solve_triangular on the fp32 factor
            v = torch.linalg.solve_triangular(L.float().to(dev), x.T, upper=False)
            ref32 = (torch.sqrt((v ** 2).sum(0)) * 0.75).double().cpu()
            err_ref = float(((ref32 - want).abs() / want).max())
            assert err <= 2 * err_ref + 1e-7, (err, err_ref, r)
    again = u.sigma(x, M.to(dev, torch.float32), 0.75)
    assert torch.equal(again, u.sigma(x, M.to(dev, torch.float32), 0.75))


@pytest.mark.parametrize("R,K,P", [(8, 128, 1), (5000, 64, 3), (300, 1024, 1), (16, 4096, 1)])
def test_ensemble_matches_fp64_and_recentres(rt, dev, R, K, P):
    from metatrain_amd.pet import llpr

    m = rt.HipModel(dict(opet.DEFAULT_HYPERS), TYPES)
    u = llpr.LLPRUncertainty.__new__(llpr.LLPRUncertainty)
    u.model, u.lib, u.dev = m, m.lib, dev
    u.F = F = 256
    x = _rows(R, F, 4, dev)
    g = torch.Generator().manual_seed(9)
    W = (torch.randn(K * P, F, generator=g) * 0.1).to(dev)
    pred = torch.randn(R, P, generator=g).to(dev)
    raw = u.ensemble(x, W, K, None).double()
    want = x.double() @ W.double().T
    assert float((raw - want).abs().max() / want.abs().max()) < TOL
    y = u.ensemble(x, W, K, pred).double().reshape(R, K, P)
    w3 = want.reshape(R, K, P)
    want_c = w3 - w3.mean(1, keepdim=True) + pred.double()[:, None, :]
    assert float((y - want_c).abs().max() / want_c.abs().max()) < TOL
    assert float((y.mean(1) - pred.double()).abs().max()) < 1e-6 * max(1.0, float(want.abs().max()))
    assert torch.equal(u.ensemble(x, W, K, pred), u.ensemble(x, W, K, pred))


def test_ensemble_spread_matches_sigma(rt, dev):
    """Members drawn as w + L^-T z: their spread at a row x is sqrt(x^T (L L^T)^-1 x) = sigma (K = 4096)."""
    from metatrain_amd.pet import llpr

    m = rt.HipModel(dict(opet.DEFAULT_HYPERS), TYPES)
    u = llpr.LLPRUncertainty.__new__(llpr.LLPRUncertainty)
    u.model, u.lib, u.dev = m, m.lib, dev
    u.F = F = 256
    train = _rows(4000, F, 5, dev).double().cpu()
    L, _ = llpr.cholesky_ladder(train.T @ train, 1e-6)
    K = 4096
    g = torch.Generator().manual_seed(13)
    w = torch.randn(1, F, generator=g, dtype=torch.float64) * 0.05
    W = llpr.ensemble_weights(w, L, torch.ones(1, dtype=torch.float64), [torch.randn(F, K, generator=g, dtype=torch.float64)])
    x = _rows(6, F, 6, dev)
    y = u.ensemble(x, W.to(dev, torch.float32), K, torch.zeros(6, 1, device=dev))
    M = torch.tril(torch.linalg.solve_triangular(L, torch.eye(F, dtype=torch.float64), upper=False))
    sigma = u.sigma(x, M.to(dev, torch.float32))
    ratio = (y.double().std(1) / sigma.double()).cpu()
    assert float((ratio - 1).abs().max()) < 0.05, ratio


def test_llpr_end_to_end_energy(rt, dev, golden_dir):
    """compute_covariance -> Cholesky -> calibrate -> ensemble -> forward on the two-system batch: energies equal
    pet_forward's bitwise, sigma and the ensemble against fp64 oracles on the reference LLF."""
    ref = np.load(os.path.join(golden_dir, "pet_llpr.npz"))
    hypers = dict(opet.DEFAULT_HYPERS)
    m, graph, _, params = _setup(rt, dev, golden_dir, "batch_two_systems.npz", hypers)
    from metatrain_amd.pet import llpr

    u = llpr.LLPRUncertainty(m, params, {"energy": "system"}, num_ensemble_members={"energy": 128})
    u.compute_covariance([graph])
    cov = u.buffers["covariance_energy_uncertainty"]
    _, llf = u.features(graph, targets=["energy"])["energy"]
    assert relmax(llf.cpu(), ref["llf_two_systems"]) < TOL
    llf64 = llf.double().cpu()  # the oracles below start from the kernels' own LLF (pinned to the reference just above)
    sysl = graph.system_of_atom().long().cpu()
    n_at = torch.bincount(sysl).double()
    rows64 = torch.zeros(2, u.F, dtype=torch.float64).index_add(0, sysl, llf64)
    x64 = rows64 / n_at[:, None]
    assert float((cov.cpu() - x64.T @ x64).abs().max() / (x64.T @ x64).abs().max()) < TOL
    u.compute_cholesky_decomposition(regularizer=1e-4)
    labels = {"energy": torch.tensor([[1.0], [-2.0]], device=dev)}
    u.calibrate([(graph, labels)], "squared_residuals")
    alpha = float(u.buffers["multiplier_energy_uncertainty"][0])
    u.generate_ensemble(torch.Generator().manual_seed(0))
    out = u.forward(graph, {"energy": "system", "energy_uncertainty": "system", "energy_ensemble": "system"})
    fw = rt.HipForward(m, graph)
    e = fw.sum_over_atoms(fw.forward())
    assert torch.equal(u.forward(graph, {"energy": "atom"})["energy"][:, 0], fw.forward())  # the fused head's bits
    assert relmax(out["energy"][:, 0].cpu(), e.cpu()) < 1e-6
    L = u.buffers["cholesky_energy_uncertainty"].cpu()
    s64 = alpha * torch.sqrt((torch.linalg.solve_triangular(L, rows64.T, upper=False) ** 2).sum(0))
    assert out["energy_uncertainty"].shape == (2, 1)
    assert relmax(out["energy_uncertainty"][:, 0].cpu(), s64) < 1e-4
    res = (out["energy"] - labels["energy"]).double().cpu()
    sig1 = out["energy_uncertainty"].double().cpu() / alpha
    assert abs(alpha - float(torch.sqrt((res ** 2 / sig1 ** 2).mean()))) < 1e-4 * alpha
    ens = out["energy_ensemble"]
    assert ens.shape == (2, 128)
    assert float((ens.double().mean(1) - out["energy"][:, 0].double()).abs().max()) < 1e-6 * float(ens.abs().max())
    W = u.buffers["llpr_ensemble_layers.energy.weight"].double().cpu()
    y = rows64 @ W.T
    want = y - y.mean(1, keepdim=True) + out["energy"].double().cpu()
    # the members cancel a large common part (small regularizer): bound the error by torch's own fp32 evaluation as well
    x32 = u.rows(graph, llf, mean=False)
    y32 = x32 @ u.buffers["llpr_ensemble_layers.energy.weight"].T
    t32 = (y32 - y32.mean(1, keepdim=True) + out["energy"]).double().cpu()
    assert relmax(ens.cpu(), want) <= max(TOL, 2 * relmax(t32, want))
    # per-atom outputs and selected atoms
    per_atom = u.forward(graph, {"energy_uncertainty": "atom"})["energy_uncertainty"]
    s_atom = alpha * torch.sqrt((torch.linalg.solve_triangular(L, llf64.T, upper=False) ** 2).sum(0))
    assert relmax(per_atom[:, 0].cpu(), s_atom) < 1e-4
    sel = torch.zeros(graph.n_nodes, dtype=torch.bool)
    sel[::3] = True
    got = u.forward(graph, {"energy": "system", "energy_uncertainty": "system"}, selected_atoms=sel.to(dev))
    rows_sel = torch.zeros(2, u.F, dtype=torch.float64).index_add(0, sysl[sel], llf64[sel])
    s_sel = alpha * torch.sqrt((torch.linalg.solve_triangular(L, rows_sel.T, upper=False) ** 2).sum(0))
    assert relmax(got["energy_uncertainty"][:, 0].cpu(), s_sel) < 1e-4
    assert not torch.allclose(got["energy_uncertainty"], out["energy_uncertainty"])
    a = fw.forward().cpu()
    e_sel = torch.zeros(2).index_add(0, sysl[sel], a[sel])
    assert relmax(got["energy"][:, 0].cpu(), e_sel) < 1e-6
    idx = u.forward(graph, {"energy_uncertainty": "system"}, selected_atoms=torch.nonzero(sel)[:, 0].to(dev))
    assert torch.equal(idx["energy_uncertainty"], got["energy_uncertainty"])
    # forces next to the uncertainty: the fused head's adjoint
    fo = u.forward(graph, {"energy": "system"}, explicit_gradients={"energy": ["positions"]})
    assert torch.equal(fo["energy/positions"], fw.backward(torch.ones(graph.n_nodes, device=dev)))
    with pytest.raises(NotImplementedError, match="energy_ensemble"):
        u.forward(graph, {"energy_ensemble": "system"}, explicit_gradients={"energy_ensemble": ["positions"]})
    # state dict round trip
    u2 = llpr.LLPRUncertainty(m, params, {"energy": "system"}, num_ensemble_members={"energy": 128})
    u2.load_state_dict(u.state_dict())
    o2 = u2.forward(graph, {"energy_uncertainty": "system", "energy_ensemble": "system"})
    assert torch.equal(o2["energy_uncertainty"], out["energy_uncertainty"])
    assert torch.equal(o2["energy_ensemble"], out["energy_ensemble"])


def test_llpr_several_targets_with_several_properties(rt, dev, golden_dir):
    from metatrain_amd.pet import llpr

    hypers = dict(opet.DEFAULT_HYPERS)
    targets = {"energy": 1, "multi_a": 3, "multi_b": 6}
    m, graph, _, params = _setup(rt, dev, golden_dir, "pet_multitarget_box50.npz", hypers, targets)
    u = llpr.LLPRUncertainty(m, params, {"energy": "system", "multi_a": "atom", "multi_b": "atom"},
                             num_ensemble_members={"multi_a": 16, "multi_b": 8})
    u.compute_covariance([graph])
    u.compute_cholesky_decomposition()
    for t in ("multi_a", "multi_b"):
        assert u.regularizers[f"mtt::aux::{t}_uncertainty"] >= 1e-20
    u.generate_ensemble(torch.Generator().manual_seed(1))
    out = u.forward(graph, {"multi_a": "atom", "mtt::aux::multi_a_uncertainty": "atom", "mtt::aux::multi_a_ensemble": "atom",
                            "multi_b": "atom", "mtt::aux::multi_b_ensemble": "atom"})
    for t, P, K in (("multi_a", 3, 16), ("multi_b", 6, 8)):
        pred = out[t]
        ref = rt.predict(m, graph, *rt.HipForward(m, graph).forward(want_features=True)[1:], t)
        assert pred.shape == (graph.n_nodes, P) and relmax(pred.cpu(), ref.cpu()) < 1e-6
        ens = out[f"mtt::aux::{t}_ensemble"].reshape(graph.n_nodes, K, P).double()
        assert float((ens.mean(1) - pred.double()).abs().max()) < 1e-5 * float(ens.abs().max())
    s = out["mtt::aux::multi_a_uncertainty"]
    assert s.shape == (graph.n_nodes, 3) and torch.equal(s[:, 0], s[:, 1])  # broadcast over the properties


def _inputs(golden_dir, fname, dev):
    g = dict(np.load(os.path.join(golden_dir, fname)))
    t = lambda k, dt=None: torch.tensor(g[k]).to(dev) if dt is None else torch.tensor(g[k]).to(dev, dt)  # noqa: E731
    return (t("in_positions", torch.float32), t("in_cells", torch.float32), t("in_centers"), t("in_neighbors"),
            t("in_cell_shifts"), t("in_species"), t("in_system_indices"))


def test_exported_llpr_model_scripts_saves_and_matches(rt, dev, golden_dir, tmp_path):
    """ExportedLLPRModel: scripted, saved and reloaded, equals eager within 1e-6; its energies, forces and per-atom
    energies are the bits of ExportedEnergyModel's; sigma and the ensemble equal LLPRUncertainty.forward's."""
    from metatrain_amd.pet import llpr, script

    hypers = dict(opet.DEFAULT_HYPERS)
    m, graph, _, params = _setup(rt, dev, golden_dir, "batch_two_systems.npz", hypers)
    u = llpr.LLPRUncertainty(m, params, {"energy": "system"}, num_ensemble_members={"energy": 16})
    u.compute_covariance([graph])
    u.compute_cholesky_decomposition(regularizer=1e-4)
    u.calibrate([(graph, {"energy": torch.tensor([[1.0], [-2.0]], device=dev)})], "absolute_residuals")
    u.generate_ensemble(torch.Generator().manual_seed(2))
    cpu_params = {k: v.cpu() for k, v in params.items()}
    eager = script.ExportedLLPRModel(script.make_core(hypers, TYPES, cpu_params, "energy"), u.state_dict())
    plain = script.ExportedEnergyModel(script.make_core(hypers, TYPES, cpu_params, "energy"))
    path = str(tmp_path / "llpr.pt")
    torch.jit.save(torch.jit.script(eager), path)
    loaded = torch.jit.load(path)
    assert torch.equal(loaded.multiplier_energy_uncertainty, u.buffers["multiplier_energy_uncertainty"].cpu())
    assert torch.equal(loaded.llpr_ensemble_layers_energy_weight.cpu(), u.buffers["llpr_ensemble_layers.energy.weight"].cpu())
    args = _inputs(golden_dir, "batch_two_systems.npz", dev)
    for sel in (None, torch.arange(0, args[0].shape[0], 3, device=dev)):
        want = eager(*args, selected_atoms=sel, with_stress=True, per_atom_uncertainty=True)
        got = loaded(*args, selected_atoms=sel, with_stress=True, per_atom_uncertainty=True)
        ref = plain(*args, selected_atoms=sel, with_stress=True)
        for a, b in zip(got, want):
            assert a.shape == b.shape
            if a.numel():
                assert float((a - b).abs().max()) <= 1e-6 * max(1.0, float(b.abs().max()))
        # forces and per-atom energies: the same bits as ExportedEnergyModel's (one pet_forward / pet_backward each);
        # energies and stress are torch index_add sums of those bits, whose order of additions on the device is not fixed
        assert torch.equal(got[1], ref[1]) and torch.equal(got[3], ref[3])
        for k in (0, 2):
            assert float((got[k] - ref[k]).abs().max()) <= 1e-6 * max(1.0, float(ref[k].abs().max())), k
        out = u.forward(graph, {"energy_uncertainty": "system", "energy_ensemble": "system"}, selected_atoms=sel)
        assert got[4].shape == (2,) and got[6].shape == (2, 16)
        assert relmax(got[4].cpu(), out["energy_uncertainty"][:, 0].cpu()) < 1e-6
        assert relmax(got[6].cpu(), out["energy_ensemble"].cpu()) < 1e-6
        per_atom = u.forward(graph, {"energy_uncertainty": "atom"}, selected_atoms=sel)["energy_uncertainty"]
        assert relmax(got[5].cpu(), per_atom[:, 0].cpu()) < 1e-6


def test_forces_next_to_llpr_outputs_need_the_fused_head(rt, dev, golden_dir):
    """The residual featuriser has no fused energy head: energy/positions next to LLPR outputs is refused, named."""
    from metatrain_amd._lib import PetHipError

    hypers = dict(opet.DEFAULT_HYPERS, featurizer_type="residual")
    _, graph, u, _ = _setup(rt, dev, golden_dir, "pet_variant_residual_box64.npz", hypers)
    u.compute_covariance([graph])
    u.compute_cholesky_decomposition(regularizer=1e-4)
    out = u.forward(graph, {"energy": "system", "energy_uncertainty": "system"})
    assert out["energy_uncertainty"].shape == (1, 1)
    with pytest.raises(PetHipError, match="residual featuriser"):
        u.forward(graph, {"energy": "system", "energy_uncertainty": "system"}, explicit_gradients={"energy": ["positions"]})


def test_energy_alone_takes_no_llf_pass(rt, dev, golden_dir):
    """Only the target requested: the plain fused forward, bit for bit, and no last-layer feature pass."""
    hypers = dict(opet.DEFAULT_HYPERS)
    m, graph, u, _ = _setup(rt, dev, golden_dir, "batch_two_systems.npz", hypers)
    calls = []
    orig = u.features
    u.features = lambda *a, **k: calls.append(1) or orig(*a, **k)
    out = u.forward(graph, {"energy": "atom"}, explicit_gradients={"energy": ["positions"]})
    assert not calls
    fw = rt.HipForward(m, graph)
    assert torch.equal(out["energy"][:, 0], fw.forward())
    assert torch.equal(out["energy/positions"], fw.backward(torch.ones(graph.n_nodes, device=dev)))
