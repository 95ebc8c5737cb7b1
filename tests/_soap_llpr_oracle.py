"""Torch restatement (fp64, or fp32 as the yardstick) of the SOAP-BPNN last-layer features and of the LLPR chain behind them,
built on ``oracle.soap`` (``spherical_expansion``, ``power_spectrum``, ``basis``). TEST INFRASTRUCTURE ONLY; no GPU import.

Definition. ``H = num_neurons_per_layer``; the tail is ``num_hidden_layers`` x [Linear, SiLU], then for
``heads: {energy: mlp}`` one more [Linear(H, H), SiLU], then the bias-free last layer.

* last-layer features of atom i: the input of ``last_layers.energy.<s>.weight`` -- the head's output;
* ``feature``: the BPNN's output before the head (equal to the former for a linear head);
* layout: ``legacy = False``: ``[N, H]``; ``legacy = True``: ``[N, n_species H]``, the atom's H values in the columns of its
  centre species' index in ``atomic_types``, exact zeros elsewhere;
* weights ``[1, F]``: ``last_layers.energy.<s>.weight`` concatenated over s, so ``llf @ w.T`` is the atomic energy.

The chain: ``cov = X^T X`` (X: per-system ``sum_i LLF_i / n_atoms`` or the per-atom LLF), the Cholesky factor of
``sym(cov) + r I``, ``sigma = alpha |L^-1 x|`` on the evaluation rows (per-system sums, or per atom), the calibration
multipliers and the ensemble ``x W^T - mean_k + prediction`` with ``W = w + alpha L^-T z``. In fp32 the chain mirrors what
the device holds in fp32 (features, rows, the products) and keeps in fp64 what the device keeps in fp64 (the covariance
buffer, the factorisation and the draw on the host)."""
import math

import torch

import soap_cases as sc
from _memo import memo_oracle
from oracle import soap as osoap

CALIBRATION_METHODS = ("squared_residuals", "absolute_residuals", "crps")


# ---- cases -------------------------------------------------------------------------------------------------------------------
def variant(base, tag, bpnn=None, heads=None):
    """``base`` of ``soap_cases`` with other ``bpnn`` hypers and / or a head, as a case of its own (``<base>+<tag>``)."""
    c = sc.case(base)
    h = dict(c.hypers, bpnn=dict(c.hypers["bpnn"], **(bpnn or {})))
    if heads:
        h["heads"] = dict(heads)
    return sc._make(f"{base}+{tag}", c.reason, c.systems, h, c.types)


_PARAMS = {}


def params_of(c, seed=1):
    """``soap_cases.params`` for any case (variants included): fp32, LayerNorm weights and biases perturbed."""
    key = (c.name, seed)
    if key not in _PARAMS:
        p = osoap.synthetic_params(c.hypers, len(c.types), osoap.basis(c.hypers)[0], seed, torch.float32)
        g = torch.Generator().manual_seed(3)
        for k in p:
            if k.startswith("layernorm."):
                p[k] = p[k] + 0.3 * torch.randn(p[k].shape, generator=g)
        _PARAMS[key] = p
    return _PARAMS[key]


def feature_size(hypers, n_species):
    return hypers["bpnn"]["num_neurons_per_layer"] * (n_species if hypers["legacy"] else 1)


def weights(p, hypers, n_species):
    """``[1, F]`` straight from the definition (not through ``last_layer_weights``)."""
    n_sets = n_species if hypers["legacy"] else 1
    return torch.cat([p[f"last_layers.energy.{s}.weight"] for s in range(n_sets)], dim=1)


# ---- features ----------------------------------------------------------------------------------------------------------------
@memo_oracle
def _features(p, hypers, types, b, dtype):
    p = {k: v.to(dtype) for k, v in p.items()}
    legacy, ns = bool(hypers["legacy"]), len(types)
    H, nh = hypers["bpnn"]["num_neurons_per_layer"], hypers["bpnn"]["num_hidden_layers"]
    mlp = (hypers.get("heads") or {}).get("energy") == "mlp"
    pos, cells = b["positions"].to(dtype), b["cells"].to(dtype)
    n = pos.shape[0]
    table = torch.full((max(types) + 1,), -1, dtype=torch.long)
    table[torch.tensor(types)] = torch.arange(ns)
    sp = table[b["species"].long()]
    ctr, nbr = b["centers"].long(), b["neighbors"].long()
    v = pos[nbr] - pos[ctr] + torch.einsum("ab,abc->ac", b["cell_shifts"].to(dtype), cells[b["system_indices"].long()[ctr]])
    spw = torch.eye(ns, dtype=dtype) if legacy else p["species_embedding.weight"]
    feats = osoap.power_spectrum(osoap.spherical_expansion(v, ctr, sp[nbr], n, hypers, spw))
    if not legacy:
        feats = feats * p["center_encoding.weight"][sp]
    F = feature_size(hypers, ns)
    atomic = torch.zeros(n, dtype=dtype)
    llf, feature = torch.zeros(n, F, dtype=dtype), torch.zeros(n, F, dtype=dtype)
    for s in range(ns if legacy else 1):
        idx = torch.nonzero(sp == s).squeeze(-1) if legacy else torch.arange(n)
        if len(idx) == 0:
            continue
        x = feats[idx]
        if hypers["bpnn"]["layernorm"]:
            x = torch.nn.functional.layer_norm(x, (x.shape[1],), p[f"layernorm.{s}.weight"], p[f"layernorm.{s}.bias"], 1e-5)
        for k in range(nh):
            x = torch.nn.functional.silu(x @ p[f"bpnn.{s}.{2 * k}.weight"].T)
        feature[idx, s * H:(s + 1) * H] = x
        if mlp:
            x = torch.nn.functional.silu(x @ p[f"heads.energy.{s}.0.weight"].T)
        llf[idx, s * H:(s + 1) * H] = x
        atomic[idx] = (x @ p[f"last_layers.energy.{s}.weight"].T)[:, 0]
    return atomic, llf, feature


def features(c, b, dtype=torch.float64):
    """``(atomic [N], llf [N, F], feature [N, F])`` of case ``c`` on batch ``b`` (of ``soap_cases.batch``), in ``dtype``."""
    return _features(params_of(c), c.hypers, c.types, b, dtype)


def relmax(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    if b.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


# ---- the chain ---------------------------------------------------------------------------------------------------------------
def system_rows(llf, sysidx, n_sys, mean, mask=None):
    x = llf if mask is None else torch.where(mask[:, None], llf, torch.zeros_like(llf))
    rows = torch.zeros(n_sys, llf.shape[1], dtype=llf.dtype).index_add(0, sysidx, x)
    if mean:
        n = torch.bincount(sysidx, minlength=n_sys).to(llf.dtype)
        rows = torch.where(n[:, None] > 0, rows / n.clamp_min(1)[:, None], torch.zeros_like(rows))
    return rows


def cholesky(cov, regularizer):
    c = cov.double()
    return torch.linalg.cholesky(0.5 * (c + c.T) + regularizer * torch.eye(c.shape[0], dtype=torch.float64))


def sigma(L, x, alpha=1.0):
    """``alpha |L^-1 x|`` per row, in the precision of ``x`` (the factor rounded to it, as the device's ``L^-1`` is)."""
    if x.shape[0] == 0:
        return x.new_zeros(0)
    v = torch.linalg.solve_triangular(L.to(x.dtype), x.T, upper=False)
    return alpha * torch.sqrt((v * v).sum(0))


def calibration(method, residuals, sigmas):
    """The multiplier of ``llpr/calibration.py`` for one property, fp64."""
    r, s = residuals.double().reshape(-1), sigmas.double().reshape(-1)
    if method == "squared_residuals":
        return float(torch.sqrt((r * r / (s * s)).mean()))
    if method == "absolute_residuals":
        return float((r.abs() / s).mean() * math.sqrt(math.pi / 2.0))
    assert method == "crps"

    def lhs(alpha):  # d/d alpha of sum_i CRPS(N(mu_i, (alpha s_i)^2); y_i), up to a positive factor
        u = r / (alpha * s)
        phi = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
        cdf = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))
        g = 1.0 / math.sqrt(math.pi) - 2.0 * phi - u * (2.0 * cdf - 1.0)
        return float((s * (g - u * (1.0 - 2.0 * cdf))).sum())

    lo, hi = 1e-8, 1e8
    assert lhs(lo) * lhs(hi) < 0.0
    for _ in range(400):
        mid = math.sqrt(lo * hi) if hi / lo > 4.0 else 0.5 * (lo + hi)
        if not lo < mid < hi:
            break
        if lhs(lo) * lhs(mid) <= 0.0:
            hi = mid
        else:
            lo = mid
    return 0.5 * (lo + hi)


def ensemble_weights(w, L, alpha, z):
    """``[K, F]``: ``w + alpha L^-T z`` with ``z [F, K]``, fp64."""
    return (w.double().reshape(-1, 1) + alpha * torch.linalg.solve_triangular(L.double().T, z.double(), upper=True)).T.contiguous()


def ensemble(x, W, pred):
    y = x @ W.to(x.dtype).T
    return y - y.mean(1, keepdim=True) + pred.to(x.dtype).reshape(-1, 1)


def chain(c, b, sample_kind, regularizer, z, labels, selected, dtype=torch.float64):
    """Every quantity of the end-to-end test for case ``c``: covariance, factor, per-system / per-atom / selected-atom sigma
    (multiplier 1), the three calibration multipliers against ``labels`` (per ``sample_kind``), and the ensemble on the
    per-system rows with the ``squared_residuals`` multiplier and the draw ``z [F, K]``. ``dtype``: the precision of the
    features and of the products; the covariance buffer and what follows on the host are fp64 either way."""
    atomic, llf, _ = features(c, b, dtype)
    sysidx, n_sys = b["system_indices"].long(), b["cells"].shape[0]
    w = weights(params_of(c), c.hypers, len(c.types))
    X = system_rows(llf, sysidx, n_sys, True) if sample_kind == "system" else llf
    cov = (X.T @ X).double()
    L = cholesky(cov, regularizer)
    rows = system_rows(llf, sysidx, n_sys, False)
    out = {"covariance": cov, "cholesky": L, "sigma_system": sigma(L, rows), "sigma_atom": sigma(L, llf),
           "sigma_selected": sigma(L, system_rows(llf, sysidx, n_sys, False, selected))}
    energies = torch.zeros(n_sys, dtype=dtype).index_add(0, sysidx, atomic)
    pred, s1 = (energies, out["sigma_system"]) if sample_kind == "system" else (atomic, out["sigma_atom"])
    for method in CALIBRATION_METHODS:
        out[f"alpha_{method}"] = torch.tensor(calibration(method, pred.double() - labels.double(), s1))
    alpha = float(out["alpha_squared_residuals"])
    out["ensemble_weights"] = ensemble_weights(w, L, alpha, z)
    out["ensemble"] = ensemble(rows, out["ensemble_weights"], energies)
    out["energies"] = energies
    return out


CHAIN_KEYS = ("covariance", "cholesky", "sigma_system", "sigma_atom", "sigma_selected", "alpha_squared_residuals",
              "alpha_absolute_residuals", "alpha_crps", "ensemble")

# ---- the end-to-end cases: inputs shared by the CPU premise and the GPU test ---------------------------------------------------
END_TO_END = {"sheared_batch": "system", "legacy_types_5": "atom"}  # case -> sample kind of the training labels
K_MEMBERS = 16
DRAW_SEED = 23  # generate_ensemble(torch.Generator().manual_seed(DRAW_SEED)) draws the z of end_to_end_inputs


def end_to_end_inputs(name):
    """Seeded labels (per ``END_TO_END[name]``), the ensemble draw ``z [F, K]`` and the selected-atom mask of a case. The labels
    are the oracle's energies plus noise of half their largest magnitude: a residual ``prediction - label`` carries the
    prediction's fp32 error divided by ``|residual| / |prediction|``, and the multipliers -- most of all the CRPS root over
    three systems -- amplify it further, so residuals of a few per cent of the energies would let the comparison measure the
    conditioning of the calibration problem and not the code."""
    c, b = sc.case(name), sc.batch(name)
    g = torch.Generator().manual_seed(17)
    n, n_sys = b["positions"].shape[0], b["cells"].shape[0]
    atomic, _, _ = features(c, b)
    energies = torch.zeros(n_sys, dtype=torch.float64).index_add(0, b["system_indices"].long(), atomic)
    base = energies if END_TO_END[name] == "system" else atomic
    labels = base + 0.5 * float(base.abs().max()) * torch.randn(base.shape, generator=g, dtype=torch.float64)
    z = torch.randn((feature_size(c.hypers, len(c.types)), K_MEMBERS), generator=torch.Generator().manual_seed(DRAW_SEED),
                    dtype=torch.float64)
    selected = torch.zeros(n, dtype=torch.bool)
    selected[::3] = True
    return labels, z, selected


def chain_yardstick(name, regularizer):
    """``(fp64 chain, {key: relmax of the fp32 chain against it})`` of an end-to-end case."""
    c, b = sc.case(name), sc.batch(name)
    labels, z, selected = end_to_end_inputs(name)
    c64 = chain(c, b, END_TO_END[name], regularizer, z, labels, selected, torch.float64)
    c32 = chain(c, b, END_TO_END[name], regularizer, z, labels, selected, torch.float32)
    return c64, {k: relmax(c32[k], c64[k]) for k in CHAIN_KEYS}
