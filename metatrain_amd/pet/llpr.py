"""Last-layer prediction rigidity (LLPR, ``metatrain/llpr``) on the native PET path.

``LLPRUncertainty`` wraps a :class:`~metatrain_amd.runtime.HipModel` and adds what a PET-MAD-style model ships:
``energy_uncertainty`` / ``energy_ensemble`` for the energy target and ``mtt::aux::<t>_uncertainty`` /
``mtt::aux::<t>_ensemble`` for the others (``llpr/model.py:362-670``). The per-atom last-layer features of every readout
layer (``pet_llpr_features``), the per-system rows, the covariance ``X^T X``, the variance ``|L^-1 x|^2`` and the ensemble
``X W^T`` run in the HIP kernels of ``csrc/llpr.hip``; the Cholesky factorisation, the ensemble draw and the calibration are
host fp64, as in the reference (``compute_cholesky_decomposition`` :924, ``generate_ensemble`` :1075, ``calibrate`` :979,
``llpr/calibration.py``).

Explicit gradients of ensemble members (positions, strain) would cost one full adjoint per member: they are not served.
"""
import math
from ctypes import c_void_p
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from .. import runtime as rt
from .._lib import PET_LLPR_MAX_ENSEMBLE, PetHipError, check
from ..runtime import _ptr, _require_cuda, _stream

CALIBRATION_METHODS = ("squared_residuals", "absolute_residuals", "crps")


def uncertainty_name(target: str) -> str:
    """``_get_uncertainty_name`` (llpr/model.py:1326)."""
    return "energy_uncertainty" if target == "energy" else f"mtt::aux::{target.replace('mtt::', '')}_uncertainty"


def ensemble_name(target: str) -> str:
    return "energy_ensemble" if target == "energy" else f"mtt::aux::{target.replace('mtt::', '')}_ensemble"


def _dist() -> bool:
    return torch.distributed.is_available() and torch.distributed.is_initialized()


def all_reduce_sum(t: torch.Tensor) -> torch.Tensor:
    """In-place SUM over the ranks when ``torch.distributed`` is initialised (through host memory for gloo)."""
    if not _dist():
        return t
    if t.is_cuda and torch.distributed.get_backend() == "gloo":
        host = t.cpu()
        torch.distributed.all_reduce(host)
        t.copy_(host)
    else:
        torch.distributed.all_reduce(t)
    return t


# ---- calibration (llpr/calibration.py) ------------------------------------------------------------------------------
class RatioCalibrator:
    """``squared_residuals``: alpha = sqrt(mean r^2 / s^2); ``absolute_residuals``: alpha = mean |r| / s * sqrt(pi / 2).
    Sums and counts are fp64 and reduced over the ranks once, in :meth:`finalize`."""

    def __init__(self, method: str):
        if method not in ("squared_residuals", "absolute_residuals"):
            raise ValueError(f"unknown ratio calibration method '{method}'")
        self.method = method
        self.sums: Dict[str, torch.Tensor] = {}
        self.counts: Dict[str, torch.Tensor] = {}

    def update(self, name: str, residuals: torch.Tensor, uncertainties: torch.Tensor) -> None:
        r = residuals.detach().to(torch.float64).cpu()
        s = uncertainties.detach().to(torch.float64).cpu()
        ratios = r.abs() / s if self.method == "absolute_residuals" else r ** 2 / s ** 2
        total = ratios.sum(dim=0)
        n = torch.tensor(float(ratios.shape[0]), dtype=torch.float64)
        if name in self.sums:
            self.sums[name] += total
            self.counts[name] += n
        else:
            self.sums[name], self.counts[name] = total, n

    def finalize(self) -> Dict[str, torch.Tensor]:
        out = {}
        for k in self.sums:
            all_reduce_sum(self.sums[k])
            all_reduce_sum(self.counts[k])
            mean = self.sums[k] / self.counts[k]
            out[k] = mean * math.sqrt(math.pi / 2.0) if self.method == "absolute_residuals" else torch.sqrt(mean)
        return out


def _crps_lhs(alpha: float, r: torch.Tensor, s: torch.Tensor) -> float:
    """Optimality condition of sum_i CRPS(N(mu_i, (alpha s_i)^2); y_i) in alpha: sum_i s_i [G(u_i) - u_i (1 - 2 Phi(u_i))]
    with u = r / (alpha s), G(u) = 1/sqrt(pi) - 2 phi(u) - u (2 Phi(u) - 1); fp64, summed over the ranks."""
    alpha = max(float(alpha), 1e-20)
    u = r / (alpha * s)
    phi = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    cdf = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))
    g = 1.0 / math.sqrt(math.pi) - 2.0 * phi - u * (2.0 * cdf - 1.0)
    lhs = (s * (g - u * (1.0 - 2.0 * cdf))).sum().reshape(1)
    return float(all_reduce_sum(lhs)[0])


def _solve_crps(r: torch.Tensor, s: torch.Tensor) -> float:
    f = lambda a: _crps_lhs(a, r, s)  # noqa: E731
    lo, hi = 1e-10, 50.0
    f_lo, f_hi = f(lo), f(hi)
    if abs(f_lo) <= 1e-12:  # flat at the lower end: move it up until the condition is informative
        for _ in range(8):
            lo *= 10.0
            f_lo = f(lo)
            if abs(f_lo) > 1e-12:
                break
        else:
            raise RuntimeError("CRPS calibration: the optimality condition vanishes at the lower bound")
    if f_lo * f_hi > 0.0:
        for _ in range(12):
            hi *= 10.0
            f_hi = f(hi)
            if f_lo * f_hi <= 0.0:
                break
        else:
            raise RuntimeError("CRPS calibration: no sign change of the optimality condition")
    # bisection to convergence: every rank takes the same steps (each evaluation is a collective)
    for _ in range(400):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        f_mid = f(mid)
        if f_mid == 0.0:
            return mid
        if f_lo * f_mid < 0.0:
            hi, f_hi = mid, f_mid
        else:
            lo, f_lo = mid, f_mid
    return 0.5 * (lo + hi)


class CRPSCalibrator:
    """Gaussian CRPS: per property, the alpha at which the CRPS derivative vanishes (uncertainties clamped at 1e-12)."""

    def __init__(self, eps: float = 1e-12):
        self.eps = eps
        self.res: Dict[str, List[torch.Tensor]] = {}
        self.unc: Dict[str, List[torch.Tensor]] = {}

    def update(self, name: str, residuals: torch.Tensor, uncertainties: torch.Tensor) -> None:
        r = residuals.detach().to(torch.float64).cpu()
        s = uncertainties.detach().to(torch.float64).cpu().clamp_min(self.eps)
        self.res.setdefault(name, []).append(r.reshape(r.shape[0], -1))
        self.unc.setdefault(name, []).append(s.reshape(s.shape[0], -1))

    def finalize(self) -> Dict[str, torch.Tensor]:
        out = {}
        for k in self.res:
            r, s = torch.cat(self.res[k]), torch.cat(self.unc[k])
            out[k] = torch.tensor([_solve_crps(r[:, m], s[:, m]) for m in range(r.shape[1])], dtype=torch.float64)
        return out


def make_calibrator(method: str):
    if method in ("squared_residuals", "absolute_residuals"):
        return RatioCalibrator(method)
    if method == "crps":
        return CRPSCalibrator()
    raise ValueError(f"Unknown calibration method '{method}'! Supported methods are {', '.join(CALIBRATION_METHODS)}.")


# ---- host fp64 linear algebra ---------------------------------------------------------------------------------------
def cholesky_ladder(covariance: torch.Tensor, regularizer: Optional[float] = None) -> Tuple[torch.Tensor, float]:
    """Cholesky factor of the symmetrised covariance + r I (fp64). No regularizer: r = 1e-20, 1e-19, ... (times 10) while
    the factorisation fails and r < 1e16 (llpr/model.py:924-977); raises when none works. Returns (L, r)."""
    c = covariance.detach().to(torch.float64).cpu()
    sym = 0.5 * (c + c.T)
    eye = torch.eye(c.shape[0], dtype=torch.float64)
    if regularizer is not None:
        return torch.linalg.cholesky(sym + regularizer * eye), float(regularizer)
    r = 1e-20
    while r < 1e16:
        L, info = torch.linalg.cholesky_ex(sym + r * eye)
        if int(info) == 0:
            return L, r
        r *= 10.0
    raise RuntimeError("Could not compute the Cholesky decomposition of the LLPR covariance up to a regularizer of 1e16")


def ensemble_weights(weights: torch.Tensor, cholesky: torch.Tensor, multiplier: torch.Tensor,
                     z: Sequence[torch.Tensor]) -> torch.Tensor:
    """Ensemble weights ``[K P, F]`` (member-major, index k P + p): for property p, ``w_p + alpha_p L^-T z_p`` with
    ``z_p [F, K]`` (llpr/model.py:1075-1138)."""
    L = cholesky.detach().to(torch.float64).cpu()
    w = weights.detach().to(torch.float64).cpu()
    m = multiplier.detach().to(torch.float64).cpu().reshape(-1)
    cols = []
    for p in range(w.shape[0]):
        alpha = float(m[p] if m.numel() > 1 else m[0])
        disp = torch.linalg.solve_triangular(L.T, z[p].to(torch.float64).cpu(), upper=True) * alpha
        cols.append(w[p].unsqueeze(1) + disp)  # [F, K]
    return torch.stack(cols, dim=-1).reshape(w.shape[1], -1).T.contiguous()


# ---- the wrapper ----------------------------------------------------------------------------------------------------
class LLPRUncertainty:
    """LLPR over a loaded :class:`HipModel`.

    :param model: the model (its state dict uploaded with :meth:`HipModel.load`).
    :param params: that state dict (reference schema): the last-layer weights the ensembles are drawn around.
    :param targets: target name -> sample kind of its training labels (``"system"`` or ``"atom"``): per-system targets
        use LLF / n_atoms rows in the covariance, per-atom targets the per-atom rows.
    :param num_ensemble_members: target name -> K (``hypers["num_ensemble_members"]``).
    """

    def __init__(self, model: rt.HipModel, params: Dict[str, torch.Tensor], targets: Dict[str, str],
                 num_ensemble_members: Optional[Dict[str, int]] = None):
        rt.refuse_long_range(getattr(model, "hypers", None) or {}, "LLPR")
        self.model = model
        self.lib = model.lib
        self.F = int(self.lib.pet_llpr_feature_size(model.handle))
        self.L = int(self.lib.pet_model_num_readout_layers(model.handle))
        self.dev = next(v for v in params.values() if torch.is_tensor(v)).device
        self.targets = dict(targets)
        self.num_ensemble_members = dict(num_ensemble_members or {})
        for t in self.num_ensemble_members:
            if t not in self.targets:
                raise ValueError(f"Output '{t}' in ensembles section is not supported by the model")
        self.weights: Dict[str, torch.Tensor] = {}
        self.buffers: Dict[str, torch.Tensor] = {}
        for t, kind in self.targets.items():
            if kind not in ("system", "atom"):
                raise ValueError(f"sample kind of '{t}' must be 'system' or 'atom', not '{kind}'")
            parts = []
            for layer in range(self.L):
                for side in ("node", "edge"):
                    key = f"{side}_last_layers.{t}.{layer}.{t}.weight"
                    if key not in params:
                        raise PetHipError(f"target '{t}': '{key}' is not in the state dict")
                    parts.append(params[key].detach())
            self.weights[t] = torch.cat(parts, dim=-1).to(self.dev, torch.float32)  # [P, F]: last_layer_parameter_names
            u = uncertainty_name(t)
            self.buffers[f"covariance_{u}"] = torch.zeros((self.F, self.F), dtype=torch.float64, device=self.dev)
            self.buffers[f"cholesky_{u}"] = torch.zeros((self.F, self.F), dtype=torch.float64, device=self.dev)
            self.buffers[f"multiplier_{u}"] = torch.ones(1, dtype=torch.float64, device=self.dev)
        for t, k in self.num_ensemble_members.items():
            P = self.weights[t].shape[0]
            if k * P > PET_LLPR_MAX_ENSEMBLE:
                raise ValueError(f"'{t}': {k} members x {P} properties exceed {PET_LLPR_MAX_ENSEMBLE}")
            self.buffers[f"llpr_ensemble_layers.{t}.weight"] = torch.zeros((k * P, self.F), dtype=torch.float32,
                                                                            device=self.dev)
        self.regularizers: Dict[str, float] = {}
        self._inv: Dict[str, torch.Tensor] = {}

    # ---- state ------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {k: v.clone() for k, v in self.buffers.items()}

    def load_state_dict(self, state: Dict[str, torch.Tensor]) -> None:
        missing = sorted(set(self.buffers) - set(state))
        unexpected = sorted(set(state) - set(self.buffers))
        if missing or unexpected:
            raise KeyError(f"LLPR state dict: missing {missing}, unexpected {unexpected}")
        for k, v in state.items():
            if k.startswith("multiplier_"):
                # the reference's [1], or one multiplier per property after calibrating a target with P > 1
                t = next(t for t in self.targets if k == f"multiplier_{uncertainty_name(t)}")
                if v.dim() != 1 or v.numel() not in (1, self.weights[t].shape[0]):
                    raise ValueError(f"'{k}': shape {tuple(v.shape)}, expected (1,) or ({self.weights[t].shape[0]},)")
                self.buffers[k] = v.detach().to(self.dev, torch.float64).clone()
                continue
            if tuple(v.shape) != tuple(self.buffers[k].shape):
                raise ValueError(f"'{k}': shape {tuple(v.shape)}, expected {tuple(self.buffers[k].shape)}")
            self.buffers[k].copy_(v)
        self._inv.clear()

    def _names(self, t: str) -> Tuple[bytes, bytes]:
        return rt._head_names(self.model, t, t, readout_zero=self.L == 1)

    def _inverse_cholesky(self, t: str) -> torch.Tensor:
        u = uncertainty_name(t)
        if u not in self._inv:
            L = self.buffers[f"cholesky_{u}"].cpu()
            if not bool(L.diagonal().ne(0).all()):
                raise RuntimeError(f"'{u}': no Cholesky factor yet (compute_cholesky_decomposition)")
            M = torch.linalg.solve_triangular(L, torch.eye(self.F, dtype=torch.float64), upper=False)
            self._inv[u] = torch.tril(M).to(self.dev, torch.float32).contiguous()  # uploaded once per factor
        return self._inv[u]

    # ---- kernels ----------------------------------------------------------------------------------------------------
    def features(self, graph: rt.HipGraph, fw: Optional[rt.HipForward] = None, targets: Iterable[str] = (),
                 feats=None):
        """Per-atom predictions ``[N, P]`` and LLF ``[N, F]`` of every target, from one backbone forward."""
        fw = fw or rt.HipForward(self.model, graph)
        if feats is None:
            if self.L == 1:
                _, nf, ef = fw.forward(want_features=True)
                feats = ([nf], [ef])
            else:
                feats = fw.features_layers()
        pn = (c_void_p * self.L)(*[t.data_ptr() for t in feats[0]])
        pe = (c_void_p * self.L)(*[t.data_ptr() for t in feats[1]])
        out = {}
        for t in targets:
            tn, bn = self._names(t)
            P = self.weights[t].shape[0]
            atomic = torch.empty((graph.n_nodes, P), dtype=torch.float32, device=self.dev)
            llf = torch.empty((graph.n_nodes, self.F), dtype=torch.float32, device=self.dev)
            check(self.lib.pet_llpr_features(self.model.handle, graph.handle, tn, bn, pn, pe, self.L, _ptr(atomic),
                                             _ptr(llf), _stream()))
            out[t] = (atomic, llf)
        return out

    def rows(self, graph: rt.HipGraph, llf: torch.Tensor, mean: bool, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        _require_cuda(llf)
        rows = torch.empty((graph.n_systems, self.F), dtype=torch.float32, device=self.dev)
        sysidx = graph.system_of_atom().to(torch.int32).contiguous()
        m = mask.to(torch.uint8).contiguous() if mask is not None else None
        check(self.lib.pet_llpr_rows(self.model.handle, self.F, _ptr(llf), graph.n_nodes, _ptr(sysidx), graph.n_systems,
                                     _ptr(m), int(mean), _ptr(rows), _stream()))
        return rows

    def accumulate(self, x: torch.Tensor, cov: torch.Tensor) -> None:
        _require_cuda(x, cov)
        x = x.contiguous()
        if x.shape[0] > 0:
            check(self.lib.pet_llpr_covariance_accumulate(self.model.handle, self.F, _ptr(x), x.shape[0], _ptr(cov),
                                                          _stream()))

    def finalize(self, cov: torch.Tensor) -> None:
        _require_cuda(cov)
        check(self.lib.pet_llpr_covariance_finalize(self.model.handle, self.F, _ptr(cov), _stream()))

    def sigma(self, x: torch.Tensor, inv_cholesky: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
        _require_cuda(x, inv_cholesky)
        x = x.contiguous()
        out = torch.empty(x.shape[0], dtype=torch.float32, device=self.dev)
        if x.shape[0] > 0:
            check(self.lib.pet_llpr_variance(self.model.handle, self.F, _ptr(x), x.shape[0], _ptr(inv_cholesky),
                                             float(alpha), _ptr(out), _stream()))
        return out

    def ensemble(self, x: torch.Tensor, weights: torch.Tensor, K: int, prediction: Optional[torch.Tensor]) -> torch.Tensor:
        _require_cuda(x, weights)
        x = x.contiguous()
        P = weights.shape[0] // K
        out = torch.empty((x.shape[0], K * P), dtype=torch.float32, device=self.dev)
        if prediction is not None:
            _require_cuda(prediction)
        pred = prediction.to(torch.float32).contiguous() if prediction is not None else None
        if x.shape[0] > 0:
            check(self.lib.pet_llpr_ensemble(self.model.handle, self.F, _ptr(x), x.shape[0], _ptr(weights.contiguous()),
                                             K, P, _ptr(pred), _ptr(out), _stream()))
        return out

    # ---- llpr/model.py procedures -----------------------------------------------------------------------------------
    def compute_covariance(self, batches: Iterable[rt.HipGraph]) -> None:
        """covariance += X^T X over the batches (per-system targets: LLF summed per system / n_atoms; per-atom
        targets: per-atom LLF), all-reduced when ``torch.distributed`` is initialised."""
        inc = {t: torch.zeros((self.F, self.F), dtype=torch.float64, device=self.dev) for t in self.targets}
        for graph in batches:
            feats = self.features(graph, targets=list(self.targets))
            for t, (_, llf) in feats.items():
                x = self.rows(graph, llf, mean=True) if self.targets[t] == "system" else llf
                self.accumulate(x, inc[t])
        for t in self.targets:  # only this call's increment is reduced: a second call adds to the covariance once
            self.finalize(inc[t])
            all_reduce_sum(inc[t])
            self.buffers[f"covariance_{uncertainty_name(t)}"] += inc[t]

    def compute_cholesky_decomposition(self, regularizer: Optional[float] = None) -> None:
        for t in self.targets:
            u = uncertainty_name(t)
            L, r = cholesky_ladder(self.buffers[f"covariance_{u}"], regularizer)
            self.buffers[f"cholesky_{u}"].copy_(L)
            self.regularizers[u] = r
            self._inv.pop(u, None)

    def calibrate(self, batches: Iterable[Tuple[rt.HipGraph, Dict[str, torch.Tensor]]], method: str) -> None:
        """Multipliers from (prediction - label, uncalibrated sigma) over the batches: ``squared_residuals``,
        ``absolute_residuals`` or ``crps`` (fp64 sums, all-reduced when distributed)."""
        cal = make_calibrator(method)
        saved = {u: self.buffers[f"multiplier_{uncertainty_name(u)}"].clone() for u in self.targets}
        for t in self.targets:
            self.buffers[f"multiplier_{uncertainty_name(t)}"].fill_(1.0)
        try:
            for graph, labels in batches:
                req = {}
                for t in labels:
                    req[t] = self.targets[t]
                    req[uncertainty_name(t)] = self.targets[t]
                out = self.forward(graph, req)
                for t, y in labels.items():
                    pred = out[t].reshape(y.shape[0], -1)
                    cal.update(uncertainty_name(t), pred - y.reshape(y.shape[0], -1).to(pred),
                               out[uncertainty_name(t)].reshape(y.shape[0], -1))
            mult = cal.finalize()
        except Exception:
            for t, v in saved.items():
                self.buffers[f"multiplier_{uncertainty_name(t)}"].copy_(v)
            raise
        for u, alpha in mult.items():
            buf = self.buffers[f"multiplier_{u}"]
            if alpha.numel() != buf.numel():  # several properties: one multiplier each
                self.buffers[f"multiplier_{u}"] = alpha.to(self.dev, torch.float64)
            else:
                buf.copy_(alpha.reshape(buf.shape))

    def generate_ensemble(self, generator: Optional[torch.Generator] = None) -> None:
        """Weights ``w + alpha L^-T z``, z standard normal ``[F, K]``, one draw per property (host fp64)."""
        for t, K in self.num_ensemble_members.items():
            u = uncertainty_name(t)
            w = self.weights[t]
            z = [torch.randn((self.F, K), generator=generator, dtype=torch.float64) for _ in range(w.shape[0])]
            W = ensemble_weights(w, self.buffers[f"cholesky_{u}"], self.buffers[f"multiplier_{u}"], z)
            self.buffers[f"llpr_ensemble_layers.{t}.weight"].copy_(W)

    def forward(self, graph: rt.HipGraph, outputs: Dict[str, str], selected_atoms: Optional[torch.Tensor] = None,
                explicit_gradients: Optional[Dict[str, List[str]]] = None) -> Dict[str, torch.Tensor]:
        """``outputs``: name -> sample kind (``"system"`` or ``"atom"``). Names: a target (its prediction, summed over the
        selected atoms per system, or per selected atom), its uncertainty (sigma broadcast over the P properties) and its
        ensemble (``[samples, K P]``, member-major). ``selected_atoms``: bool mask or indices of the atoms that count.
        ``explicit_gradients`` of an ensemble output raise ``NotImplementedError``; ``{"energy": ["positions"]}`` adds
        ``"energy/positions"`` (dE/dR of the per-system energies' sum, fused energy head)."""
        explicit_gradients = explicit_gradients or {}
        if self.model.hypers.get("zbl", False):
            # predictions (and the mean an ensemble is centred on) would lack the additive ZBL term of pet/model.py:616-660
            raise PetHipError("this wrapper evaluates the network alone, and the model has `zbl: true`: evaluate through "
                              "ExportedLLPRModel(..., zbl=...), which adds the ZBL term (covariance, Cholesky factor, "
                              "calibration and ensemble weights of this object do not depend on it)")
        for name, grads in explicit_gradients.items():
            if name.endswith("_ensemble") and grads:
                raise NotImplementedError(f"explicit gradients ({', '.join(grads)}) of '{name}' are not implemented: each "
                                          "ensemble member would need its own adjoint pass")
        wanted: Dict[str, str] = {}
        for name, kind in outputs.items():
            t = self._target_of(name)
            if name.endswith("_ensemble") and t not in self.num_ensemble_members:
                raise ValueError(f"'{name}': no ensemble was configured for '{t}'")
            wanted.setdefault(t, kind)
        mask = None
        if selected_atoms is not None:
            sa = selected_atoms.to(self.dev)
            mask = sa if sa.dtype == torch.bool else torch.zeros(graph.n_nodes, dtype=torch.bool,
                                                                 device=self.dev).index_fill(0, sa.long(), True)
        fw = rt.HipForward(self.model, graph)
        want_forces = "positions" in explicit_gradients.get("energy", [])
        fused = self.model.target == "energy" and self.L == 1 and "energy" in wanted
        need_llf = {self._target_of(n) for n in outputs if n.endswith("_uncertainty") or n.endswith("_ensemble")}
        # the fused energy head needs no LLF pass: only targets with an LLPR output or without a fused head go through
        # pet_llpr_features (which recomputes the heads)
        kernel_targets = [t for t in wanted if t in need_llf or not (t == "energy" and fused)]
        fused_atomic = None
        per_target = {}
        if kernel_targets:
            feats = None
            if self.L == 1:
                a, nf, ef = fw.forward(want_features=True)
                fused_atomic = a if fused else None
                feats = ([nf], [ef])
            per_target = self.features(graph, fw, kernel_targets, feats=feats)
        else:  # only the fused energy: the plain forward
            fused_atomic = fw.forward()
        sysl = graph.system_of_atom().long()
        keep = mask if mask is not None else torch.ones(graph.n_nodes, dtype=torch.bool, device=self.dev)
        preds: Dict[Tuple[str, str], torch.Tensor] = {}
        rows: Dict[Tuple[str, str], torch.Tensor] = {}  # evaluation rows, shared by a target's uncertainty and ensemble
        res: Dict[str, torch.Tensor] = {}
        for name, kind in outputs.items():
            t = self._target_of(name)
            if (t, kind) not in preds:
                atomic = fused_atomic.unsqueeze(1) if (t == "energy" and fused) else per_target[t][0]
                if kind == "system":
                    preds[(t, kind)] = torch.zeros((graph.n_systems, atomic.shape[1]), dtype=torch.float32,
                                                   device=self.dev).index_add(
                        0, sysl, torch.where(keep[:, None], atomic, torch.zeros_like(atomic)))
                else:
                    preds[(t, kind)] = atomic[keep]
            pred = preds[(t, kind)]
            if name == t:
                res[name] = pred
                continue
            if (t, kind) not in rows:
                llf = per_target[t][1]
                rows[(t, kind)] = self.rows(graph, llf, mean=False, mask=mask) if kind == "system" else llf[keep]
            x = rows[(t, kind)]
            u = uncertainty_name(t)
            if name.endswith("_uncertainty"):
                mult = self.buffers[f"multiplier_{u}"]
                alpha = float(mult[0]) if mult.numel() == 1 else 1.0
                s = self.sigma(x, self._inverse_cholesky(t), alpha)
                s = s[:, None].expand(-1, pred.shape[1])
                res[name] = s * mult.to(torch.float32)[None, :] if mult.numel() > 1 else s.contiguous()
            else:
                K = self.num_ensemble_members[t]
                res[name] = self.ensemble(x, self.buffers[f"llpr_ensemble_layers.{t}.weight"], K, pred)
        if want_forces:
            if not fused:
                raise PetHipError("forces next to LLPR outputs need the fused energy head: HipModel.load(params, 'energy') "
                                  "and one readout layer (not the residual featuriser)")
            res["energy/positions"] = fw.backward(torch.where(
                mask, 1.0, 0.0).to(torch.float32) if mask is not None else torch.ones(graph.n_nodes, device=self.dev))
        return res

    def _target_of(self, name: str) -> str:
        base = name
        for suf in ("_uncertainty", "_ensemble"):
            if name.endswith(suf):
                base = name[: -len(suf)]
                if base.startswith("mtt::aux::"):
                    base = base[len("mtt::aux::"):]
                    if base not in self.targets and f"mtt::{base}" in self.targets:
                        base = f"mtt::{base}"
        if base not in self.targets:
            raise ValueError(f"'{name}': unknown LLPR target '{base}' (targets: {sorted(self.targets)})")
        return base

