"""SOAP-BPNN last-layer features, LLPR uncertainties and ensembles on the MI355X (``csrc/soap_llpr.hip``,
``metatrain_amd/soap_bpnn/llpr.py``) against the fp64 restatement ``_soap_llpr_oracle.py``; ``test_soap_llpr_cpu.py`` holds
the premises.

Bar of the features, the rows and the end-to-end chain: the fp32-floor rule, ``relmax <= max(1e-5, 2 y)`` with ``y`` the
relmax of the SAME oracle evaluated by torch in fp32. Bars of the four shared kernels: those of ``test_gpu_llpr.py``,
``err < 1e-5 and err <= 2 err_t + 2^-23`` with ``err_t`` the error of fp32 torch. Measured figures: DESIGN §28."""
import pytest
import torch

import _soap_llpr_oracle as lo
import soap_cases as sc
from test_soap_llpr_cpu import REGULARIZER

pytestmark = pytest.mark.gpu
TOL = 1e-5
EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


def bar(y):
    assert y <= 1e-3, f"fp32 yardstick {y:.2e}: this input pins nothing"
    return max(TOL, 2.0 * y)


_MODELS = {}


def _model(c, dev, zbl=None):
    """One model per (hypers, types): the row and bucket cases share the four-type legacy model."""
    key = (repr(c.hypers), tuple(c.types), zbl)
    if key not in _MODELS:
        from metatrain_amd.soap_bpnn import SoapBpnnHip

        m = SoapBpnnHip(c.hypers, c.types, zbl=zbl)
        m.load({k: v.to(dev) for k, v in lo.params_of(c).items()})
        _MODELS[key] = m
    return _MODELS[key]


def _graph(m, b, dev):
    return m.graph(b["positions"].float().to(dev), b["cells"].float().to(dev), b["centers"].to(dev), b["neighbors"].to(dev),
                   b["cell_shifts"].to(dev), b["species"].to(dev), b["system_indices"].int().to(dev))


def _v(base, tag, **kw):
    heads = kw.pop("heads", None)
    return lambda: lo.variant(base, tag, bpnn=kw, heads=heads)


FEATURE_CASES = {
    # tail forms and widths, H = 32
    **{n: (lambda n=n: sc.case(n)) for n in ("legacy_types_1", "legacy_types_3", "legacy_types_8", "legacy_types_9",
                                             "alchemical_types_1", "alchemical_types_9")},
    # widths the MFMA tails do not serve
    **{f"{base}+h{H}": _v(base, f"h{H}", num_neurons_per_layer=H)
       for base in ("legacy_types_3", "alchemical_types_1") for H in (1, 31, 33, 64)},
    # depth
    **{f"legacy_types_3+nh{k}": _v("legacy_types_3", f"nh{k}", num_hidden_layers=k) for k in (1, 2, 3, 8)},
    "alchemical_types_1+nh3": _v("alchemical_types_1", "nh3", num_hidden_layers=3),
    "legacy_types_3+mlp": _v("legacy_types_3", "mlp", num_hidden_layers=2, heads={"energy": "mlp"}),
    "alchemical_types_1+mlp": _v("alchemical_types_1", "mlp", num_hidden_layers=2, heads={"energy": "mlp"}),
    "legacy_types_3+noln": _v("legacy_types_3", "noln", layernorm=False),
    # rows and buckets
    **{n: (lambda n=n: sc.case(n)) for n in ("small_1", "small_5", "holes", "mixed", "bucket_70_0_1_0", "bucket_0_0_0_130",
                                             "bucket_64_65_63_1", "chunks")},
}


@pytest.mark.parametrize("name", list(FEATURE_CASES))
def test_last_layer_features_against_the_oracle(name, dev):
    """LLF and ``feature`` against the fp64 oracle at the fp32-floor bar; shape and F; off-block columns exactly zero; the same
    bits on a second call and behind a packed and a full feature buffer; ``LLF @ w.T`` (host fp64) within ``H 2^-23`` of the
    forward's per-atom energies relative to ``max_i sum_j |w_j x_ij|``."""
    from metatrain_amd.soap_bpnn import last_layer_weights

    c = FEATURE_CASES[name]()
    b = sc.batch(name.split("+")[0])
    m = _model(c, dev)
    g = _graph(m, b, dev)
    H, ns = c.hypers["bpnn"]["num_neurons_per_layer"], len(c.types)
    F = H * ns if c.hypers["legacy"] else H
    n = b["positions"].shape[0]
    assert m.llpr_feature_size == F
    atomic = m.forward(g)
    llf = m.last_layer_features(g)
    feature = m.features(g)
    assert llf.shape == feature.shape == (n, F) and llf.dtype == torch.float32
    a64, llf64, feat64 = lo.features(c, b)
    _, llf32, feat32 = lo.features(c, b, torch.float32)
    for what, got, ref, ref32 in (("llf", llf, llf64, llf32), ("feature", feature, feat64, feat32)):
        y, err = lo.relmax(ref32, ref), lo.relmax(got, ref)
        print(f"[{name}] {what}: relmax {err:.2e} (fp32 oracle {y:.2e})")
        assert err <= bar(y), (name, what, err, y)
    mlp = (c.hypers.get("heads") or {}).get("energy") == "mlp"
    assert torch.equal(llf, feature) != mlp
    if c.hypers["legacy"]:
        sp = torch.tensor([c.types.index(int(z)) for z in b["species"]], dtype=torch.long)
        own = (torch.arange(F)[None, :] // H) == sp[:, None]
        assert bool((llf.cpu()[~own] == 0.0).all()) and bool((feature.cpu()[~own] == 0.0).all())
    # the same bits again
    assert torch.equal(m.last_layer_features(g), llf)
    # behind the full-layout feature buffer (the forward above was packed where the model allows): the entry point reads the
    # workspace of that forward as it is -- the oracle at the same bar; its first Linear sums in another order than the packed
    # one's, so the last bits may differ -- and the model's method gives the bits of the inference forward again
    from metatrain_amd import runtime as rt
    from metatrain_amd._lib import check

    m.forward(g, want_features=True)
    ws, full = m._workspace(g), torch.empty_like(llf)
    check(m.lib.soap_llpr_features(m._handle, g.handle, rt._ptr(ws), ws.numel(), 0, rt._ptr(full), rt._stream()))
    err = lo.relmax(full, llf64)
    print(f"[{name}] llf behind the full layout: relmax {err:.2e}; against the packed forward's {lo.relmax(full, llf):.2e}")
    assert err <= bar(lo.relmax(llf32, llf64)), (name, err)
    assert torch.equal(m.last_layer_features(g), llf)
    # consistency with the forward's energies: the same H fp32 products, summed in another order
    w = last_layer_weights(lo.params_of(c), c.hypers, ns).double()
    x = llf.double().cpu()
    scale = float((x.abs() * w.abs()).sum(1).max())
    err = float(((x @ w.T)[:, 0] - atomic.double().cpu()).abs().max()) / scale
    print(f"[{name}] LLF @ w against the forward's energies: {err:.2e} of {H * EPS:.2e}")
    assert err <= H * EPS, (name, err)
    assert lo.relmax(atomic, a64) <= 1e-4  # (the forward itself is pinned by test_gpu_soap_edges.py)


def test_mixed_rows_and_the_empty_system(dev):
    """Per-system rows of ``mixed`` (a dense system, an EMPTY one, a dilute one, an isolated atom) for ``mean`` 0 and 1 against
    the oracle; the empty system's row is exactly zero."""
    from metatrain_amd.soap_bpnn import SoapLLPRUncertainty

    c, b = sc.case("mixed"), sc.batch("mixed")
    m = _model(c, dev)
    g = _graph(m, b, dev)
    u = SoapLLPRUncertainty(m, {k: v.to(dev) for k, v in lo.params_of(c).items()})
    llf = m.last_layer_features(g)
    _, llf64, _ = lo.features(c, b)
    _, llf32, _ = lo.features(c, b, torch.float32)
    sysidx, n_sys = b["system_indices"].long(), b["cells"].shape[0]
    assert n_sys == 4 and int((sysidx == 1).sum()) == 0
    for mean in (False, True):
        got = u.rows(g, llf, mean=mean)
        ref = lo.system_rows(llf64, sysidx, n_sys, mean)
        y = lo.relmax(lo.system_rows(llf32, sysidx, n_sys, mean), ref)
        err = lo.relmax(got, ref)
        print(f"[mixed] rows mean={mean}: relmax {err:.2e} (fp32 oracle {y:.2e})")
        assert got.shape == (4, u.F) and err <= bar(y)
        assert float(got[1].abs().max()) == 0.0
        assert torch.equal(got, u.rows(g, llf, mean=mean))


def test_a_batch_without_atoms(dev):
    c = sc.case("small_1")
    m = _model(c, dev)
    e0 = torch.zeros(0, dtype=torch.long, device=dev)
    g = m.graph(torch.zeros((0, 3), device=dev), torch.zeros(1, 3, 3, device=dev), e0, e0,
                torch.zeros((0, 3), dtype=torch.long, device=dev), e0, torch.zeros(0, dtype=torch.int32, device=dev))
    assert m.last_layer_features(g).shape == (0, 128) and m.features(g).shape == (0, 128)


def test_a_system_alone_gives_the_bits_it_has_inside_a_batch(dev):
    """``sheared_batch``: every system's LLF rows and per-system row, evaluated alone, equal those inside the batch."""
    from metatrain_amd.soap_bpnn import SoapLLPRUncertainty

    c, b = sc.case("sheared_batch"), sc.batch("sheared_batch")
    m = _model(c, dev)
    u = SoapLLPRUncertainty(m, {k: v.to(dev) for k, v in lo.params_of(c).items()})
    g = _graph(m, b, dev)
    llf = m.last_layer_features(g).clone()
    rows = u.rows(g, llf, mean=True)
    first = b["first_atom"]
    for s in range(3):
        lo_, hi = first[s], first[s + 1]
        pairs = (b["centers"] >= lo_) & (b["centers"] < hi)
        one = {"positions": b["positions"][lo_:hi], "cells": b["cells"][s:s + 1], "centers": b["centers"][pairs] - lo_,
               "neighbors": b["neighbors"][pairs] - lo_, "cell_shifts": b["cell_shifts"][pairs],
               "species": b["species"][lo_:hi], "system_indices": torch.zeros(hi - lo_, dtype=torch.long)}
        g1 = _graph(m, one, dev)
        llf1 = m.last_layer_features(g1)
        assert torch.equal(llf1, llf[lo_:hi]), s
        assert torch.equal(u.rows(g1, llf1, mean=True)[0], rows[s]), s


# ---- the four shared kernels at SOAP widths ------------------------------------------------------------------------------------
def _width_model(F, dev):
    """A model whose last-layer feature size is F: F <= 64 alchemical with H = F, else legacy with F / 32 species of H = 32 (or
    H = 64 for 512). Only its handle is used (the F check); no parameters are loaded."""
    from metatrain_amd.soap_bpnn import SoapBpnnHip, SoapLLPRUncertainty

    key = ("width", F)
    if key not in _MODELS:
        if F <= 64:
            hypers, types = dict(sc.ALCHEMICAL, bpnn=dict(sc.ALCHEMICAL["bpnn"], num_neurons_per_layer=F)), sc.TYPES4
        else:
            H = 32 if F // 32 <= 9 else 64
            hypers, types = dict(sc.LEGACY, bpnn=dict(sc.LEGACY["bpnn"], num_neurons_per_layer=H)), sc.TYPES11[:F // H]
        _MODELS[key] = SoapBpnnHip(hypers, types)
    m = _MODELS[key]
    u = SoapLLPRUncertainty.__new__(SoapLLPRUncertainty)
    u.model, u.lib, u.dev, u.F = m, m.lib, dev, F
    assert m.llpr_feature_size == F
    return u


def _rows(n, F, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, F, generator=g, dtype=torch.float64) * 0.5 + torch.rand(F, generator=g, dtype=torch.float64)
    return x.to(dev, torch.float32)


@pytest.mark.parametrize("R", [1, 8, 3001])
@pytest.mark.parametrize("F", [1, 3, 31, 33, 288, 512])
def test_shared_kernels_at_soap_widths(F, R, dev):
    """Covariance (symmetric, reproducible), variance and ensemble (recentred) of ``csrc/llpr.hip`` behind the ``soap_llpr_*``
    entries at widths below, across and off the 64-column tiles, with the bars of ``test_gpu_llpr.py``."""
    u = _width_model(F, dev)
    x = _rows(R, F, 1 + F + R, dev)
    x64 = x.double()
    # covariance
    C = torch.zeros((F, F), dtype=torch.float64, device=dev)
    u.accumulate(x, C)
    u.finalize(C)
    C64 = x64.T @ x64
    err = float((C - C64).abs().max() / C64.abs().max())
    err_t = float(((x.T @ x).double() - C64).abs().max() / C64.abs().max())
    assert err < TOL and err <= 2 * err_t + EPS, ("covariance", err, err_t)
    assert torch.equal(C, C.T)
    C2 = torch.zeros_like(C)
    u.accumulate(x, C2)
    u.finalize(C2)
    assert torch.equal(C, C2)
    # variance, on a well-conditioned factor of this width
    train = _rows(4 * F + 64, F, 2, dev).double().cpu()
    cov = train.T @ train
    L = torch.linalg.cholesky(cov + 1e-3 * float(cov.diagonal().mean()) * torch.eye(F, dtype=torch.float64))
    M = torch.tril(torch.linalg.solve_triangular(L, torch.eye(F, dtype=torch.float64), upper=False))
    M32 = M.to(dev, torch.float32)
    want = torch.sqrt(((M32.double().cpu() @ x64.cpu().T) ** 2).sum(0)) * 0.75
    got = u.sigma(x, M32, 0.75)
    t32 = torch.sqrt(((M32 @ x.T) ** 2).sum(0)) * 0.75
    err = float(((got.double().cpu() - want).abs() / want).max())
    err_t = float(((t32.double().cpu() - want).abs() / want).max())
    assert err < TOL and err <= 2 * err_t + EPS, ("variance", err, err_t)
    assert torch.equal(got, u.sigma(x, M32, 0.75))
    # ensemble
    K = 16
    g = torch.Generator().manual_seed(9)
    W = (torch.randn(K, F, generator=g) * 0.1).to(dev)
    pred = torch.randn(R, 1, generator=g).to(dev)
    raw = u.ensemble(x, W, K, None).double()
    want = x64 @ W.double().T
    scale = float(want.abs().max())
    err = float((raw - want).abs().max()) / scale
    err_t = float(((x @ W.T).double() - want).abs().max()) / scale
    assert err < TOL and err <= 2 * err_t + EPS, ("ensemble", err, err_t)
    y = u.ensemble(x, W, K, pred)
    want_c = want - want.mean(1, keepdim=True) + pred.double()
    assert float((y.double() - want_c).abs().max() / want_c.abs().max()) < TOL
    assert float((y.double().mean(1, keepdim=True) - pred.double()).abs().max()) < 1e-6 * max(1.0, scale)
    assert torch.equal(y, u.ensemble(x, W, K, pred))


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lo.END_TO_END))
def test_llpr_end_to_end(name, dev):
    """compute_covariance -> Cholesky -> calibrate (three methods) -> ensemble (K = 16) -> forward, every quantity against the
    oracle chain in fp64 at ``max(1e-5, 2 y)``, ``y`` from the fp32 chain, per quantity. ``sheared_batch`` trains on per-system
    labels, ``legacy_types_5`` on per-atom labels. The regularizer is passed explicitly: ``REGULARIZER = 1e-5``, the smallest
    power of ten at which ``test_soap_llpr_cpu.py`` finds ``y <= 1e-4`` in every quantity of both cases (measured there:
    sheared_batch 7.1e-6, legacy_types_5 8.2e-5; at 1e-6 legacy_types_5 has 2.9e-4). A ``state_dict`` round trip reproduces every
    output bit for bit; the ensemble's mean is the prediction."""
    from metatrain_amd.soap_bpnn import SoapLLPRUncertainty

    c, b = sc.case(name), sc.batch(name)
    kind = lo.END_TO_END[name]
    labels, z, selected = lo.end_to_end_inputs(name)
    ref, y = lo.chain_yardstick(name, REGULARIZER)
    m = _model(c, dev)
    g = _graph(m, b, dev)
    params = {k: v.to(dev) for k, v in lo.params_of(c).items()}
    u = SoapLLPRUncertainty(m, params, sample_kind=kind, num_ensemble_members=lo.K_MEMBERS)
    u.compute_covariance([g])
    u.compute_cholesky_decomposition(regularizer=REGULARIZER)
    got = {"covariance": u.buffers["covariance_energy_uncertainty"], "cholesky": u.buffers["cholesky_energy_uncertainty"]}
    assert torch.equal(got["covariance"], got["covariance"].T)
    got["sigma_system"] = u.forward(g, {"energy_uncertainty": "system"})["energy_uncertainty"][:, 0]
    got["sigma_atom"] = u.forward(g, {"energy_uncertainty": "atom"})["energy_uncertainty"][:, 0]
    sel = u.forward(g, {"energy_uncertainty": "system"}, selected_atoms=selected.to(dev))["energy_uncertainty"]
    got["sigma_selected"] = sel[:, 0]
    idx = u.forward(g, {"energy_uncertainty": "system"}, selected_atoms=torch.nonzero(selected)[:, 0].to(dev))
    assert torch.equal(idx["energy_uncertainty"], sel)
    lab = {"energy": labels.to(dev).reshape(-1, 1)}
    for method in reversed(lo.CALIBRATION_METHODS):  # squared_residuals last: the ensemble is drawn with its multiplier
        u.calibrate([(g, lab)], method)
        got[f"alpha_{method}"] = u.buffers["multiplier_energy_uncertainty"][0].clone()
    u.generate_ensemble(torch.Generator().manual_seed(lo.DRAW_SEED))  # draws the oracle's z [F, K]
    assert u.buffers["llpr_ensemble_layers.energy.weight"].shape == (lo.K_MEMBERS, u.F) and z.shape == (u.F, lo.K_MEMBERS)
    # (the weights themselves are not pinned: along directions the training rows do not span they are z / sqrt(regularizer),
    # which no evaluation row sees; the ensemble below is)
    print(f"[{name}] ensemble weights: relmax {lo.relmax(u.buffers['llpr_ensemble_layers.energy.weight'], ref['ensemble_weights']):.2e}")
    out = u.forward(g, {"energy": "system", "energy_uncertainty": "system", "energy_ensemble": "system"})
    got["ensemble"] = out["energy_ensemble"]
    for k in lo.CHAIN_KEYS:
        err = lo.relmax(got[k], ref[k])
        print(f"[{name}] {k}: relmax {err:.2e} (fp32 chain {y[k]:.2e})")
    for k in lo.CHAIN_KEYS:
        assert lo.relmax(got[k], ref[k]) <= bar(y[k]), (name, k, lo.relmax(got[k], ref[k]), y[k])
    # the calibrated sigma is alpha times the uncalibrated one; predictions are the forward's
    alpha = float(got["alpha_squared_residuals"])
    assert lo.relmax(out["energy_uncertainty"][:, 0], alpha * ref["sigma_system"]) <= bar(max(y["sigma_system"],
                                                                                           y["alpha_squared_residuals"]))
    assert torch.equal(out["energy"][:, 0], m.sum_over_atoms(g, m.forward(g)))
    assert torch.equal(u.forward(g, {"energy": "atom"})["energy"][:, 0], m.forward(g))
    ens = out["energy_ensemble"].double()
    assert ens.shape == (b["cells"].shape[0], lo.K_MEMBERS)
    assert float((ens.mean(1) - out["energy"][:, 0].double()).abs().max()) < 1e-6 * float(ens.abs().max())
    fo = u.forward(g, {"energy": "system"}, explicit_gradients={"energy": ["positions"]})
    assert torch.equal(fo["energy/positions"], m.backward(g, torch.ones(g.n_nodes, device=dev)))
    # state dict round trip, under the reference's buffer names
    state = u.state_dict()
    assert sorted(state) == ["cholesky_energy_uncertainty", "covariance_energy_uncertainty",
                             "llpr_ensemble_layers.energy.weight", "multiplier_energy_uncertainty"]
    u2 = SoapLLPRUncertainty(m, params, sample_kind=kind, num_ensemble_members=lo.K_MEMBERS)
    u2.load_state_dict(state)
    req = {"energy": "system", "energy_uncertainty": "system", "energy_ensemble": "system"}
    o2 = u2.forward(g, req)
    assert all(torch.equal(o2[k], out[k]) for k in req)
    a1, a2 = u.forward(g, {"energy_uncertainty": "atom", "energy_ensemble": "atom"}), u2.forward(
        g, {"energy_uncertainty": "atom", "energy_ensemble": "atom"})
    assert all(torch.equal(a1[k], a2[k]) for k in a1) and a1["energy_ensemble"].shape == (g.n_nodes, lo.K_MEMBERS)


def test_a_zbl_model_predicts_what_evaluate_does_and_keeps_the_network_covariance(dev):
    """``zbl=True``: predictions and the ensemble's centre include the ZBL term as ``evaluate`` does; covariance and sigma are
    those of the model without it. ``dense_lattice``: sites 1.2 A apart, inside the ZBL range of every pair of these types."""
    from metatrain_amd.soap_bpnn import SoapLLPRUncertainty

    name = "dense_lattice"
    c, b = sc.case(name), sc.batch(name)
    params = {k: v.to(dev) for k, v in lo.params_of(c).items()}
    plain, withz = _model(c, dev), _model(c, dev, zbl=True)
    gp, gz = _graph(plain, b, dev), _graph(withz, b, dev)
    up = SoapLLPRUncertainty(plain, params, num_ensemble_members=4)
    uz = SoapLLPRUncertainty(withz, params, num_ensemble_members=4)
    for u, g in ((up, gp), (uz, gz)):
        u.compute_covariance([g])
        u.compute_cholesky_decomposition(regularizer=REGULARIZER)
        u.generate_ensemble(torch.Generator().manual_seed(5))
    assert all(torch.equal(up.buffers[k], uz.buffers[k]) for k in up.buffers)
    req = {"energy": "atom", "energy_uncertainty": "atom", "energy_ensemble": "atom"}
    op, oz = up.forward(gp, req), uz.forward(gz, req, explicit_gradients={"energy": ["positions"]})
    atomic, gpos = withz.evaluate(gz)
    assert torch.equal(oz["energy"][:, 0], atomic) and torch.equal(oz["energy/positions"], gpos)
    assert not torch.equal(oz["energy"], op["energy"])
    assert torch.equal(oz["energy_uncertainty"], op["energy_uncertainty"])
    ens = oz["energy_ensemble"].double()
    assert float((ens.mean(1) - atomic.double()).abs().max()) < 1e-6 * float(ens.abs().max())


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name(dev):
    from metatrain_amd import runtime as rt
    from metatrain_amd._lib import PET_LLPR_MAX_ENSEMBLE, PetHipError
    from metatrain_amd.soap_bpnn import SoapLLPRUncertainty

    c, b = sc.case("small_5"), sc.batch("small_5")
    m = _model(c, dev)
    g = _graph(m, b, dev)
    params = {k: v.to(dev) for k, v in lo.params_of(c).items()}
    F = m.llpr_feature_size
    llf = torch.empty((g.n_nodes, F), device=dev)
    # no forward record: a workspace of the right size that no forward has written
    ws = torch.empty(int(m.lib.soap_workspace_bytes(m._handle, g.n_nodes, g.n_edges)), dtype=torch.uint8, device=dev)
    rc = m.lib.soap_llpr_features(m._handle, g.handle, rt._ptr(ws), ws.numel(), 0, rt._ptr(llf), rt._stream())
    assert rc != 0 and "no soap_forward of this graph into this workspace" in m.lib.pet_last_error().decode()
    m.forward(g)
    own = m._workspace(g)
    rc = m.lib.soap_llpr_features(m._handle, g.handle, rt._ptr(own), 16, 0, rt._ptr(llf), rt._stream())
    assert rc != 0 and "workspace too small" in m.lib.pet_last_error().decode()
    rc = m.lib.soap_llpr_features(m._handle, g.handle, rt._ptr(own), own.numel(), 2, rt._ptr(llf), rt._stream())
    assert rc != 0 and "layer = 2" in m.lib.pet_last_error().decode()
    # a wrong F at each of the five shared entries
    u = SoapLLPRUncertainty(m, params, num_ensemble_members=4)
    u.F = F + 1
    x = torch.zeros((3, F + 1), device=dev)
    for call in (lambda: u.rows(g, torch.zeros((g.n_nodes, F + 1), device=dev), mean=True),
                 lambda: u.accumulate(x, torch.zeros((F + 1, F + 1), dtype=torch.float64, device=dev)),
                 lambda: u.finalize(torch.zeros((F + 1, F + 1), dtype=torch.float64, device=dev)),
                 lambda: u.sigma(x, torch.eye(F + 1, device=dev)),
                 lambda: u.ensemble(x, torch.zeros((4, F + 1), device=dev), 4, None)):
        with pytest.raises(PetHipError, match="not this model's last-layer feature size"):
            call()
    u.F = F
    with pytest.raises(NotImplementedError, match="energy_ensemble"):
        u.forward(g, {"energy_ensemble": "system"}, explicit_gradients={"energy_ensemble": ["positions"]})
    with pytest.raises(ValueError, match="unknown LLPR output"):
        u.forward(g, {"mtt::aux::dipole_uncertainty": "system"})
    with pytest.raises(ValueError, match="no ensemble was configured"):
        SoapLLPRUncertainty(m, params).forward(g, {"energy_ensemble": "system"})
    with pytest.raises(ValueError, match=f"exceed {PET_LLPR_MAX_ENSEMBLE}"):
        SoapLLPRUncertainty(m, params, num_ensemble_members=PET_LLPR_MAX_ENSEMBLE + 1)
    with pytest.raises(PetHipError, match="MI355X only"):
        SoapLLPRUncertainty(m, lo.params_of(c))
    with pytest.raises(PetHipError, match="MI355X only"):
        u.sigma(torch.zeros(3, F), torch.eye(F))
    with pytest.raises(RuntimeError, match="no Cholesky factor yet"):
        u.forward(g, {"energy_uncertainty": "system"})
