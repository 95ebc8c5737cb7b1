"""Last-layer prediction rigidity (LLPR, ``metatrain/llpr``) on the native SOAP-BPNN path.

``llpr/model.py`` asks two things of the model it wraps: an ``mtt::aux::<target>_last_layer_features`` output and the names
of the last-layer parameters. :meth:`SoapBpnnHip.last_layer_features` (``soap_llpr_features``, ``csrc/soap_llpr.hip``) is the
first and :func:`last_layer_weights` the second; ``SoapLLPRUncertainty`` has the surface of
:class:`metatrain_amd.pet.llpr.LLPRUncertainty` for the single target ``energy``. Rows, covariance, variance and ensemble
are the kernels of ``csrc/llpr.hip`` behind their ``soap_llpr_*`` entries; the Cholesky ladder, the ensemble draw and the
calibrators are the host fp64 procedures of ``metatrain_amd.pet.llpr``.

Explicit gradients of ensemble members would cost one full adjoint per member: they are not served.
"""
from typing import Dict, Iterable, List, Optional, Tuple

import torch

from .._lib import PET_LLPR_MAX_ENSEMBLE, PetHipError, check
from ..runtime import _ptr, _require_cuda, _stream
from ..pet.llpr import (all_reduce_sum, cholesky_ladder, ensemble_name, ensemble_weights, make_calibrator,  # noqa: F401
                        uncertainty_name)

TARGET = "energy"


def last_layer_weights(params: Dict[str, torch.Tensor], hypers: dict, n_species: int) -> torch.Tensor:
    """``[1, F]``: ``last_layers.energy.<s>.weight`` ``[1, H]`` concatenated over the networks ``s`` along the last axis --
    one per species for ``legacy`` models, else one (``last_layer_parameter_names``, ``llpr/model.py:1087-1091``) -- so that
    ``LLF_i . w`` is the atomic energy of the network. CPU or GPU tensors; touches no library."""
    n_sets = int(n_species) if bool(hypers["legacy"]) else 1
    H = int(hypers["bpnn"]["num_neurons_per_layer"])
    parts = []
    for s in range(n_sets):
        key = f"last_layers.energy.{s}.weight"
        if key not in params:
            raise KeyError(f"'{key}' is not in the state dict")
        w = params[key].detach()
        if tuple(w.shape) != (1, H):
            raise ValueError(f"'{key}': shape {tuple(w.shape)}, expected (1, {H})")
        parts.append(w)
    return torch.cat(parts, dim=-1)


def feature_size(hypers: dict, n_species: int) -> int:
    """``F`` (``soap_bpnn/model.py:347-351``)."""
    return int(hypers["bpnn"]["num_neurons_per_layer"]) * (int(n_species) if bool(hypers["legacy"]) else 1)


class SoapLLPRUncertainty:
    """LLPR over a loaded :class:`SoapBpnnHip`.

    :param model: the model (its state dict uploaded with :meth:`SoapBpnnHip.load`).
    :param params: that state dict: the last-layer weights the ensemble is drawn around.
    :param sample_kind: ``"system"`` (covariance rows are ``sum_i LLF_i / n_atoms``) or ``"atom"`` (the per-atom LLF), the
        kind of the training labels.
    :param num_ensemble_members: K, or None for no ensemble.

    For a model with ``zbl``, predictions and the ensemble's centre include the ZBL term as :meth:`SoapBpnnHip.evaluate`
    does; covariance, factor, multiplier and ensemble weights are the network's and do not depend on it.
    """

    def __init__(self, model, params: Dict[str, torch.Tensor], sample_kind: str = "system",
                 num_ensemble_members: Optional[int] = None):
        if sample_kind not in ("system", "atom"):
            raise ValueError(f"sample kind of '{TARGET}' must be 'system' or 'atom', not '{sample_kind}'")
        self.model = model
        self.lib = model.lib
        self.sample_kind = sample_kind
        self.F = int(model.llpr_feature_size)
        w = last_layer_weights(params, model.hypers, len(model.atomic_types))
        _require_cuda(w)
        self.dev = w.device
        self.weights = w.to(torch.float32).contiguous()  # [1, F]
        if self.weights.shape[1] != self.F:
            raise PetHipError(f"the last-layer weights are {self.weights.shape[1]} wide, the model's features {self.F}")
        self.num_ensemble_members = None if num_ensemble_members is None else int(num_ensemble_members)
        u = uncertainty_name(TARGET)
        self.buffers: Dict[str, torch.Tensor] = {
            f"covariance_{u}": torch.zeros((self.F, self.F), dtype=torch.float64, device=self.dev),
            f"cholesky_{u}": torch.zeros((self.F, self.F), dtype=torch.float64, device=self.dev),
            f"multiplier_{u}": torch.ones(1, dtype=torch.float64, device=self.dev),
        }
        if self.num_ensemble_members is not None:
            K = self.num_ensemble_members
            if K < 1 or K * 1 > PET_LLPR_MAX_ENSEMBLE:
                raise ValueError(f"'{TARGET}': {K} members x 1 properties exceed {PET_LLPR_MAX_ENSEMBLE}" if K >= 1 else
                                 f"'{TARGET}': {K} ensemble members")
            self.buffers[f"llpr_ensemble_layers.{TARGET}.weight"] = torch.zeros((K, self.F), dtype=torch.float32,
                                                                                 device=self.dev)
        self.regularizer: Optional[float] = None
        self._inv: Optional[torch.Tensor] = None

    # ---- state ------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {k: v.clone() for k, v in self.buffers.items()}

    def load_state_dict(self, state: Dict[str, torch.Tensor]) -> None:
        missing = sorted(set(self.buffers) - set(state))
        unexpected = sorted(set(state) - set(self.buffers))
        if missing or unexpected:
            raise KeyError(f"LLPR state dict: missing {missing}, unexpected {unexpected}")
        for k, v in state.items():
            if tuple(v.shape) != tuple(self.buffers[k].shape):
                raise ValueError(f"'{k}': shape {tuple(v.shape)}, expected {tuple(self.buffers[k].shape)}")
            self.buffers[k].copy_(v)
        self._inv = None

    def _inverse_cholesky(self) -> torch.Tensor:
        if self._inv is None:
            L = self.buffers[f"cholesky_{uncertainty_name(TARGET)}"].cpu()
            if not bool(L.diagonal().ne(0).all()):
                raise RuntimeError(f"'{uncertainty_name(TARGET)}': no Cholesky factor yet (compute_cholesky_decomposition)")
            M = torch.linalg.solve_triangular(L, torch.eye(self.F, dtype=torch.float64), upper=False)
            self._inv = torch.tril(M).to(self.dev, torch.float32).contiguous()  # uploaded once per factor
        return self._inv

    # ---- kernels ----------------------------------------------------------------------------------------------------
    def features(self, graph) -> Tuple[torch.Tensor, torch.Tensor]:
        """Per-atom energies of the network ``[N]`` and LLF ``[N, F]``, from one forward."""
        atomic = self.model.forward(graph)
        return atomic, self.model.last_layer_features(graph)

    def rows(self, graph, llf: torch.Tensor, mean: bool, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        _require_cuda(llf)
        llf = llf.contiguous()
        rows = torch.empty((graph.n_systems, self.F), dtype=torch.float32, device=self.dev)
        sysidx = graph.system_of_atom().to(torch.int32).contiguous()
        m = mask.to(torch.uint8).contiguous() if mask is not None else None
        check(self.lib.soap_llpr_rows(self.model._handle, self.F, _ptr(llf), graph.n_nodes, _ptr(sysidx), graph.n_systems,
                                      _ptr(m), int(mean), _ptr(rows), _stream()))
        return rows

    def accumulate(self, x: torch.Tensor, cov: torch.Tensor) -> None:
        _require_cuda(x, cov)
        x = x.contiguous()
        if x.shape[0] > 0:
            check(self.lib.soap_llpr_covariance_accumulate(self.model._handle, self.F, _ptr(x), x.shape[0], _ptr(cov),
                                                           _stream()))

    def finalize(self, cov: torch.Tensor) -> None:
        _require_cuda(cov)
        check(self.lib.soap_llpr_covariance_finalize(self.model._handle, self.F, _ptr(cov), _stream()))

    def sigma(self, x: torch.Tensor, inv_cholesky: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
        _require_cuda(x, inv_cholesky)
        x = x.contiguous()
        out = torch.empty(x.shape[0], dtype=torch.float32, device=self.dev)
        if x.shape[0] > 0:
            check(self.lib.soap_llpr_variance(self.model._handle, self.F, _ptr(x), x.shape[0], _ptr(inv_cholesky.contiguous()),
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
            check(self.lib.soap_llpr_ensemble(self.model._handle, self.F, _ptr(x), x.shape[0], _ptr(weights.contiguous()),
                                              K, P, _ptr(pred), _ptr(out), _stream()))
        return out

    # ---- llpr/model.py procedures -----------------------------------------------------------------------------------
    def compute_covariance(self, batches: Iterable) -> None:
        """covariance += X^T X over the batches (``sample_kind`` ``"system"``: LLF summed per system / n_atoms;
        ``"atom"``: the per-atom LLF), all-reduced when ``torch.distributed`` is initialised."""
        inc = torch.zeros((self.F, self.F), dtype=torch.float64, device=self.dev)
        for graph in batches:
            llf = self.model.last_layer_features(graph)
            self.accumulate(self.rows(graph, llf, mean=True) if self.sample_kind == "system" else llf, inc)
        self.finalize(inc)  # only this call's increment is reduced: a second call adds to the covariance once
        all_reduce_sum(inc)
        self.buffers[f"covariance_{uncertainty_name(TARGET)}"] += inc

    def compute_cholesky_decomposition(self, regularizer: Optional[float] = None) -> None:
        u = uncertainty_name(TARGET)
        L, r = cholesky_ladder(self.buffers[f"covariance_{u}"], regularizer)
        self.buffers[f"cholesky_{u}"].copy_(L)
        self.regularizer = r
        self._inv = None

    def calibrate(self, batches: Iterable[Tuple[object, Dict[str, torch.Tensor]]], method: str) -> None:
        """The multiplier from (prediction - label, uncalibrated sigma) over the batches of ``(graph, {"energy": labels})``:
        ``squared_residuals``, ``absolute_residuals`` or ``crps`` (fp64 sums, all-reduced when distributed)."""
        cal = make_calibrator(method)
        u = uncertainty_name(TARGET)
        mult = self.buffers[f"multiplier_{u}"]
        saved = mult.clone()
        mult.fill_(1.0)
        try:
            for graph, labels in batches:
                y = labels[TARGET]
                out = self.forward(graph, {TARGET: self.sample_kind, u: self.sample_kind})
                pred = out[TARGET].reshape(y.shape[0], -1)
                cal.update(u, pred - y.reshape(y.shape[0], -1).to(pred), out[u].reshape(y.shape[0], -1))
            alpha = cal.finalize()[u]
        except Exception:
            mult.copy_(saved)
            raise
        mult.copy_(alpha.reshape(mult.shape))

    def generate_ensemble(self, generator: Optional[torch.Generator] = None) -> None:
        """Weights ``w + alpha L^-T z``, z standard normal ``[F, K]`` (host fp64)."""
        if self.num_ensemble_members is None:
            raise ValueError(f"'{ensemble_name(TARGET)}': no ensemble was configured for '{TARGET}'")
        u = uncertainty_name(TARGET)
        z = [torch.randn((self.F, self.num_ensemble_members), generator=generator, dtype=torch.float64)]
        W = ensemble_weights(self.weights, self.buffers[f"cholesky_{u}"], self.buffers[f"multiplier_{u}"], z)
        self.buffers[f"llpr_ensemble_layers.{TARGET}.weight"].copy_(W)

    def forward(self, graph, outputs: Dict[str, str], selected_atoms: Optional[torch.Tensor] = None,
                explicit_gradients: Optional[Dict[str, List[str]]] = None, pbcs=None) -> Dict[str, torch.Tensor]:
        """``outputs``: name -> sample kind (``"system"`` or ``"atom"``). Names: ``energy`` (summed over the selected atoms
        per system, or per selected atom; ``[samples, 1]``), ``energy_uncertainty`` and ``energy_ensemble``
        (``[samples, K]``). ``selected_atoms``: bool mask or indices of the atoms that count. ``explicit_gradients`` of the
        ensemble raise ``NotImplementedError``; ``{"energy": ["positions"]}`` adds ``"energy/positions"`` (dE/dR of the
        per-system energies' sum). ``pbcs``: as in :meth:`SoapBpnnHip.evaluate`, for a ``zbl`` model on a short graph."""
        explicit_gradients = explicit_gradients or {}
        u, e = uncertainty_name(TARGET), ensemble_name(TARGET)
        for name, grads in explicit_gradients.items():
            if name.endswith("_ensemble") and grads:
                raise NotImplementedError(f"explicit gradients ({', '.join(grads)}) of '{name}' are not implemented: each "
                                          "ensemble member would need its own adjoint pass")
        for name, kind in outputs.items():
            if name not in (TARGET, u, e):
                raise ValueError(f"'{name}': unknown LLPR output (outputs: {[TARGET, u, e]}; one SOAP-BPNN target, '{TARGET}')")
            if kind not in ("system", "atom"):
                raise ValueError(f"'{name}': sample kind must be 'system' or 'atom', not '{kind}'")
            if name == e and self.num_ensemble_members is None:
                raise ValueError(f"'{name}': no ensemble was configured for '{TARGET}'")
        for name in explicit_gradients:
            if name != e and name != TARGET:
                raise ValueError(f"'{name}': explicit gradients are served for '{TARGET}' only")
        m = self.model
        mask = None
        if selected_atoms is not None:
            sa = selected_atoms.to(self.dev)
            mask = sa if sa.dtype == torch.bool else torch.zeros(graph.n_nodes, dtype=torch.bool,
                                                                 device=self.dev).index_fill(0, sa.long(), True)
        atomic = m.forward(graph)
        zg = None
        if m.zbl is not None:
            zg = m.zbl.graph_for(graph, pbcs)
            atomic = atomic + m.zbl.forward(zg)
        llf = m.last_layer_features(graph) if (u in outputs or e in outputs) else None
        preds: Dict[str, torch.Tensor] = {}
        rows: Dict[str, torch.Tensor] = {}  # evaluation rows, shared by the uncertainty and the ensemble
        res: Dict[str, torch.Tensor] = {}
        for name, kind in outputs.items():
            if kind not in preds:
                if kind == "system":
                    a = atomic if mask is None else torch.where(mask, atomic, torch.zeros_like(atomic))
                    preds[kind] = m.sum_over_atoms(graph, a)[:, None]
                else:
                    preds[kind] = (atomic if mask is None else atomic[mask])[:, None]
            pred = preds[kind]
            if name == TARGET:
                res[name] = pred
                continue
            if kind not in rows:
                rows[kind] = self.rows(graph, llf, mean=False, mask=mask) if kind == "system" else (
                    llf if mask is None else llf[mask])
            x = rows[kind]
            if name == u:
                alpha = float(self.buffers[f"multiplier_{u}"][0])
                res[name] = self.sigma(x, self._inverse_cholesky(), alpha)[:, None]
            else:
                res[name] = self.ensemble(x, self.buffers[f"llpr_ensemble_layers.{TARGET}.weight"],
                                          self.num_ensemble_members, pred)
        if "positions" in explicit_gradients.get(TARGET, []):
            seeds = torch.ones(graph.n_nodes, dtype=torch.float32, device=self.dev) if mask is None else mask.to(torch.float32)
            gpos = m.backward(graph, seeds)
            if zg is not None:
                gpos = gpos + m.zbl.backward(zg, seeds)
            res[f"{TARGET}/positions"] = gpos
        return res
