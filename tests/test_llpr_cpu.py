"""LLPR host side (metatrain_amd/pet/llpr.py) and the argument checks of the pet_llpr_* entry points, without a GPU."""
import ctypes
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import pet as opet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pet_llpr.npz")
TYPES = [1, 6, 7, 8]


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))


def _feed(cal, res, sig, lo=0, hi=400):
    for s in range(lo, hi, 100):
        cal.update("u", torch.tensor(res[s:s + 100]), torch.tensor(sig[s:s + 100]))
    return cal.finalize()["u"].numpy()


@pytest.mark.parametrize("method", ["squared_residuals", "absolute_residuals", "crps"])
def test_calibrators_match_the_reference_multipliers(method):
    from metatrain_amd.pet import llpr

    g = np.load(GOLDEN)
    got = _feed(llpr.make_calibrator(method), g["cal_residuals"], g["cal_sigma"])
    assert _rel(got, g[f"cal_{method}"]) < 1e-9, (got, g[f"cal_{method}"])


def test_unknown_calibration_method_is_refused():
    from metatrain_amd.pet import llpr

    with pytest.raises(ValueError, match="Unknown calibration method"):
        llpr.make_calibrator("nll")


def _reference_ladder(cov):
    """The procedure of llpr/model.py:950-977, written out: r from 1e-20, times 10 while cholesky raises and r < 1e16."""
    sym = 0.5 * (cov + cov.T)
    r = 1e-20
    while r < 1e16:
        try:
            torch.linalg.cholesky(sym + r * torch.eye(cov.shape[0], dtype=torch.float64))
            return r
        except RuntimeError:
            r *= 10.0
    return None


def test_cholesky_ladder_picks_the_reference_regularizer():
    from metatrain_amd.pet import llpr

    gen = torch.Generator().manual_seed(3)
    x = torch.randn(40, 96, generator=gen, dtype=torch.float64)  # rank 40 < 96: singular
    cov = x.T @ x
    cov[0, 1] += 1e-9  # not exactly symmetric: the ladder symmetrises first
    L, r = llpr.cholesky_ladder(cov)
    assert r == _reference_ladder(cov) and r > 1e-20
    sym = 0.5 * (cov + cov.T) + r * torch.eye(96, dtype=torch.float64)
    assert torch.allclose(L @ L.T, sym, rtol=1e-10, atol=1e-8 * float(sym.abs().max()))
    L2, r2 = llpr.cholesky_ladder(cov, regularizer=1e-3)
    assert r2 == 1e-3 and torch.allclose(L2 @ L2.T, 0.5 * (cov + cov.T) + 1e-3 * torch.eye(96, dtype=torch.float64))
    full = torch.randn(200, 16, generator=gen, dtype=torch.float64)
    assert llpr.cholesky_ladder(full.T @ full)[1] == 1e-20  # positive definite: the first rung
    with pytest.raises(RuntimeError, match="1e16"):
        llpr.cholesky_ladder(-1e17 * torch.eye(8, dtype=torch.float64))
    assert _reference_ladder(-1e17 * torch.eye(8, dtype=torch.float64)) is None


def test_ensemble_weights_are_w_plus_alpha_inverse_cholesky_transpose_z():
    from metatrain_amd.pet import llpr

    gen = torch.Generator().manual_seed(5)
    F, K, P = 24, 7, 3
    x = torch.randn(60, F, generator=gen, dtype=torch.float64)
    L = torch.linalg.cholesky(x.T @ x + 0.1 * torch.eye(F, dtype=torch.float64))
    w = torch.randn(P, F, generator=gen, dtype=torch.float64)
    z = [torch.randn(F, K, generator=gen, dtype=torch.float64) for _ in range(P)]
    for mult in (torch.tensor([0.7], dtype=torch.float64), torch.tensor([0.5, 1.5, 2.0], dtype=torch.float64)):
        W = llpr.ensemble_weights(w, L, mult, z)
        assert W.shape == (K * P, F)
        Linv_T = torch.linalg.inv(L).T
        for k in range(K):
            for p in range(P):
                alpha = float(mult[p] if mult.numel() > 1 else mult[0])
                want = w[p] + alpha * (Linv_T @ z[p][:, k])
                assert torch.allclose(W[k * P + p], want, rtol=1e-10, atol=1e-12)


def _model(hypers):
    from metatrain_amd import runtime as rt

    return rt.HipModel(hypers, TYPES)


@pytest.mark.parametrize("featurizer", ["feedforward", "residual"])
def test_state_dict_names_and_shapes_match_the_reference(featurizer):
    from metatrain_amd.pet import llpr

    hypers = dict(opet.DEFAULT_HYPERS, featurizer_type=featurizer)
    params = opet.synthetic_params(hypers, TYPES, {"energy": 1, "multi_a": 3}, 0, torch.float32)
    u = llpr.LLPRUncertainty(_model(hypers), params, {"energy": "system", "multi_a": "atom"},
                             num_ensemble_members={"energy": 16, "multi_a": 4})
    L = hypers["num_gnn_layers"] if featurizer == "residual" else 1
    F = 2 * L * hypers["d_head"]  # pet/model.py:118-120
    assert u.F == F
    want = {}
    for t, un in (("energy", "energy_uncertainty"), ("multi_a", "mtt::aux::multi_a_uncertainty")):
        want[f"covariance_{un}"] = (F, F)
        want[f"cholesky_{un}"] = (F, F)
        want[f"multiplier_{un}"] = (1,)
    want["llpr_ensemble_layers.energy.weight"] = (16, F)
    want["llpr_ensemble_layers.multi_a.weight"] = (4 * 3, F)
    sd = u.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    # the mean weights are the concatenation of last_layer_parameter_names: node0 | edge0 | node1 | edge1 ...
    parts = [params[f"{s}_last_layers.multi_a.{layer}.multi_a.weight"] for layer in range(L) for s in ("node", "edge")]
    assert torch.equal(u.weights["multi_a"], torch.cat(parts, dim=1))
    sd["multiplier_energy_uncertainty"].fill_(3.0)
    u.load_state_dict(sd)
    assert float(u.buffers["multiplier_energy_uncertainty"][0]) == 3.0
    with pytest.raises(KeyError):
        u.load_state_dict({k: v for k, v in sd.items() if "cholesky" not in k})
    with pytest.raises(ValueError, match="not supported"):
        llpr.LLPRUncertainty(_model(hypers), params, {"energy": "system"}, num_ensemble_members={"multi_a": 4})


def test_output_names():
    from metatrain_amd.pet import llpr

    assert llpr.uncertainty_name("energy") == "energy_uncertainty"
    assert llpr.uncertainty_name("mtt::dipole") == "mtt::aux::dipole_uncertainty"
    assert llpr.ensemble_name("energy") == "energy_ensemble"
    assert llpr.ensemble_name("multi_a") == "mtt::aux::multi_a_ensemble"


def test_llpr_entry_points_refuse_bad_arguments_without_a_gpu():
    from metatrain_amd import _lib

    lib = _lib.load()
    m = _model(dict(opet.DEFAULT_HYPERS))
    h = m.handle
    ERR = _lib.PET_ERR_ARGUMENT
    F = int(lib.pet_llpr_feature_size(h))
    assert F == 256 and lib.pet_llpr_feature_size(None) == -1
    assert int(lib.pet_llpr_feature_size(_model(dict(opet.DEFAULT_HYPERS, featurizer_type="residual")).handle)) == 512
    buf = ctypes.c_void_p(0x1000)  # never dereferenced: every call below fails its host-side checks first
    null = ctypes.c_void_p(0)
    # wrong F, R <= 0, NULL buffers, K P above the maximum, NULL model
    assert lib.pet_llpr_covariance_accumulate(h, F + 1, buf, 10, buf, null) == ERR
    assert lib.pet_llpr_covariance_accumulate(h, F, buf, 0, buf, null) == ERR
    assert lib.pet_llpr_covariance_accumulate(h, F, null, 10, buf, null) == ERR
    assert lib.pet_llpr_covariance_accumulate(h, F, buf, 10, null, null) == ERR
    assert lib.pet_llpr_covariance_accumulate(None, F, buf, 10, buf, null) == ERR
    assert lib.pet_llpr_covariance_finalize(h, 128, buf, null) == ERR
    assert lib.pet_llpr_covariance_finalize(h, F, null, null) == ERR
    assert lib.pet_llpr_variance(h, F, buf, -1, buf, 1.0, buf, null) == ERR
    assert lib.pet_llpr_variance(h, F, buf, 5, null, 1.0, buf, null) == ERR
    assert lib.pet_llpr_variance(h, 2 * F, buf, 5, buf, 1.0, buf, null) == ERR
    assert lib.pet_llpr_ensemble(h, F, buf, 5, buf, _lib.PET_LLPR_MAX_ENSEMBLE + 1, 1, null, buf, null) == ERR
    assert lib.pet_llpr_ensemble(h, F, buf, 5, buf, 1024, 17, null, buf, null) == ERR
    assert lib.pet_llpr_ensemble(h, F, buf, 5, buf, 0, 1, null, buf, null) == ERR
    assert lib.pet_llpr_ensemble(h, F, buf, 5, null, 8, 1, null, buf, null) == ERR
    assert lib.pet_llpr_ensemble(h, F, buf, 0, buf, 8, 1, null, buf, null) == ERR
    assert lib.pet_llpr_rows(h, F - 1, buf, 10, buf, 2, null, 0, buf, null) == ERR
    assert lib.pet_llpr_rows(h, F, buf, 10, buf, 0, null, 0, buf, null) == ERR
    assert lib.pet_llpr_rows(h, F, null, 10, buf, 2, null, 0, buf, null) == ERR
    assert lib.pet_llpr_rows(h, F, buf, 10, buf, 2, null, 0, null, null) == ERR
    arr = (ctypes.c_void_p * 1)(buf)
    assert lib.pet_llpr_features(h, None, b"@", b"@", arr, arr, 1, null, buf, null) == ERR
    assert b"F = 257" in (lib.pet_llpr_covariance_accumulate(h, F + 1, buf, 10, buf, null) and lib.pet_last_error())


# ---- two ranks (gloo): the covariance reduction and the calibration sums ------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    from metatrain_amd.pet import llpr

    gen = torch.Generator().manual_seed(11)
    x = torch.randn(64, 32, generator=gen, dtype=torch.float64)
    half = x[rank * 32:(rank + 1) * 32]
    cov = llpr.all_reduce_sum(half.T @ half)
    g = np.load(GOLDEN)
    mult = {}
    for method in ("squared_residuals", "absolute_residuals", "crps"):
        mult[method] = _feed(llpr.make_calibrator(method), g["cal_residuals"], g["cal_sigma"], rank * 200, rank * 200 + 200)
    out.put((rank, cov.numpy(), mult))
    torch.distributed.destroy_process_group()


def test_two_rank_covariance_and_calibration_equal_one_rank():
    from metatrain_amd.pet import llpr

    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((out.get(timeout=120) for _ in range(2)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    x = torch.randn(64, 32, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    one = (x[:32].T @ x[:32] + x[32:].T @ x[32:]).numpy()
    g = np.load(GOLDEN)
    for rank, cov, mult in res:
        assert np.array_equal(cov, one)
        for method, got in mult.items():
            single = _feed(llpr.make_calibrator(method), g["cal_residuals"], g["cal_sigma"])
            assert _rel(got, single) < 1e-12, (method, got, single)
            assert _rel(got, g[f"cal_{method}"]) < 1e-9
    assert math.isfinite(float(res[0][2]["crps"][0]))


def test_per_property_multipliers_survive_a_state_dict_round_trip():
    """Calibrating a target with P > 1 gives one multiplier per property; a fresh wrapper takes that state back."""
    from metatrain_amd.pet import llpr

    hypers = dict(opet.DEFAULT_HYPERS)
    params = opet.synthetic_params(hypers, TYPES, {"energy": 1, "multi_a": 3}, 0, torch.float32)
    targets = {"energy": "system", "multi_a": "atom"}
    u = llpr.LLPRUncertainty(_model(hypers), params, targets)
    u.buffers["multiplier_mtt::aux::multi_a_uncertainty"] = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)
    sd = u.state_dict()
    assert tuple(sd["multiplier_energy_uncertainty"].shape) == (1,)
    fresh = llpr.LLPRUncertainty(_model(hypers), params, targets)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.buffers["multiplier_mtt::aux::multi_a_uncertainty"], sd["multiplier_mtt::aux::multi_a_uncertainty"])
    fresh.load_state_dict(llpr.LLPRUncertainty(_model(hypers), params, targets).state_dict())  # back to the reference's [1]
    assert tuple(fresh.buffers["multiplier_mtt::aux::multi_a_uncertainty"].shape) == (1,)
    bad = dict(sd)
    bad["multiplier_mtt::aux::multi_a_uncertainty"] = torch.ones(2, dtype=torch.float64)
    with pytest.raises(ValueError, match="multiplier"):
        fresh.load_state_dict(bad)


def test_exported_llpr_model_scripts_pickles_its_buffers_and_refuses_host_tensors(tmp_path):
    from metatrain_amd.pet import llpr, script

    hypers = dict(opet.DEFAULT_HYPERS)
    params = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    F = 256
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(300, F, generator=gen, dtype=torch.float64)
    cov = x.T @ x
    L, _ = llpr.cholesky_ladder(cov)
    state = {"covariance_energy_uncertainty": cov, "cholesky_energy_uncertainty": L,
             "multiplier_energy_uncertainty": torch.tensor([1.5], dtype=torch.float64),
             "llpr_ensemble_layers.energy.weight": torch.randn(8, F, generator=gen)}
    m = script.ExportedLLPRModel(script.make_core(hypers, TYPES, params, "energy"), state)
    path = str(tmp_path / "m.pt")
    torch.jit.save(torch.jit.script(m), path)
    r = torch.jit.load(path)
    assert torch.equal(r.cholesky_energy_uncertainty, L) and torch.equal(r.covariance_energy_uncertainty, cov)
    assert torch.equal(r.llpr_ensemble_layers_energy_weight, state["llpr_ensemble_layers.energy.weight"])
    inv = torch.linalg.inv(L)
    assert torch.allclose(r.inverse_cholesky.double(), torch.tril(inv), rtol=1e-5, atol=1e-6 * float(inv.abs().max()))
    assert r.num_ensemble_members == 8
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.pet.core.llpr_variance(torch.zeros(2, F), r.inverse_cholesky, 1.0)
    u = llpr.LLPRUncertainty(_model(hypers), params, {"energy": "system"})
    with pytest.raises(Exception, match="no CPU path"):
        u.sigma(torch.zeros(2, F), torch.zeros(F, F))
