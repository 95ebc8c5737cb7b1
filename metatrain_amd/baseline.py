"""Composition baselines and target scales, fitted and removed on the device (``composition/_base_composition.py``,
``composition/trainer.py``, ``scaler/_base_scaler.py``, ``scaler/trainer.py:160-200``, ``utils/additive/remove.py``): the two
steps the reference runs by default (``atomic_baseline``, ``scale_targets: true``) before the first optimizer step.

:class:`CompositionHip` and :class:`ScalerHip` work on collated batches, the dicts of :func:`metatrain_amd.data.collate`, with
the raw targets among their entries -- float64 for raw DFT energies: an energy of -1e5 eV has a float32 ulp of 8e-3 eV, and
the kernels (``csrc/baseline.hip``) widen every input to fp64 before the first operation and round once at the end. A target
entry is a tensor ``[S or N, ...]`` or, for a target of several blocks, ``{block: tensor}``. ``accumulate`` is the device
part (fixed-order fp64 / integer sums into accumulators that are ``+=`` across calls, bitwise reproducible); ``fit`` is a
handful of fp64 operations on the host. Accumulators are plain torch tensors and may live on either device; only
``accumulate`` and :class:`TargetTransform` need the GPU.

    comp = CompositionHip(types, {"energy": {"per_atom": False, "shape": [1]}})
    scaler = ScalerHip(types, {"energy": {"per_atom": False, "shape": [1]}})
    for batch in training_batches: comp.accumulate(batch)
    comp.all_reduce(); comp.fit()
    for batch in training_batches: scaler.accumulate(batch, composition=comp)
    scaler.all_reduce(); scaler.fit()
    transform = TargetTransform(comp, scaler)
    t = transform(batch, {"energies": "energy", "gradients": "dE_dR"})      # once per cached batch, before O3Augmenter
    step(graph, fw, n_atoms=t["n_atoms"], target_energies=t["target_energies"], target_gradients=t["target_gradients"])
    exported = ExportedEnergyModel(core, scaler.scale("energy"), comp.table("energy"))

Not served, each refused with a message that names it: atomic-basis (``atom_type``-keyed) and atom-pair targets, the
trace-only fit of ``o3_lambda_1`` rank-2 targets, per-type per-property scales of per-atom targets (``TrainStep`` cannot
apply them), the reference's TensorMap checkpoint buffers.
"""
from typing import Dict, Iterable, List, Optional, Union

import torch

from . import _lib
from . import runtime as rt
from ._lib import PetHipError, check

BATCH_KEYS = ("species", "system_indices")
UNSUPPORTED_SPEC = {
    "atom_type": "atomic-basis (atom_type-keyed) targets are not served",
    "atomic_basis": "atomic-basis (atom_type-keyed) targets are not served",
    "atom_pair": "atom-pair targets are not served",
    "o3_lambda_1": "the trace-only fit of o3_lambda_1 rank-2 targets is not served",
}


def _normalise_targets(targets: Dict[str, dict]) -> Dict[str, dict]:
    out = {}
    for name, spec in targets.items():
        if not isinstance(spec, dict) or "shape" not in spec:
            raise ValueError(f"target '{name}': expected {{'per_atom': bool, 'shape': [...]}}, got {spec!r}")
        for key, why in UNSUPPORTED_SPEC.items():
            if spec.get(key) or spec.get("sample_kind") == key:
                raise ValueError(f"target '{name}': {why}")
        unknown = set(spec) - {"per_atom", "shape", "sample_kind"} - set(UNSUPPORTED_SPEC)
        if unknown:
            raise ValueError(f"target '{name}': unknown entries {sorted(unknown)}")
        if spec.get("sample_kind") not in (None, "per_atom", "per_structure"):
            raise ValueError(f"target '{name}': unknown sample kind '{spec['sample_kind']}'")
        shape = spec["shape"]
        blocks = {str(b): [int(d) for d in s] for b, s in shape.items()} if isinstance(shape, dict) else {name: [int(d) for d in shape]}
        for b, s in blocks.items():
            if any(d < 1 for d in s):
                raise ValueError(f"target '{name}', block '{b}': empty dimension in the shape {s}")
        per_atom = bool(spec.get("per_atom", spec.get("sample_kind") == "per_atom"))
        out[name] = {"per_atom": per_atom, "blocks": blocks}
    return out


def _width(shape: List[int]) -> int:
    w = 1
    for d in shape:
        w *= d
    return w


def _n_properties(shape: List[int]) -> int:
    return shape[-1] if shape else 1


class _Fitted:
    """What the two classes share: the atomic types' lookup table, the device error flag, the blocks of a batch entry."""

    def __init__(self, atomic_types: Iterable[int], targets: Dict[str, dict]):
        self.atomic_types = [int(z) for z in atomic_types]
        if not self.atomic_types or len(set(self.atomic_types)) != len(self.atomic_types) or min(self.atomic_types) < 0:
            raise ValueError(f"atomic_types must be distinct non-negative atomic numbers, got {self.atomic_types}")
        self.max_z = max(self.atomic_types)
        self.targets = _normalise_targets(targets)
        self._tables: Dict[torch.device, torch.Tensor] = {}

    @property
    def n_types(self) -> int:
        return len(self.atomic_types)

    def type_index(self, device) -> torch.Tensor:
        """``[max_Z + 1]`` int32 on ``device``: the position of an atomic number in ``atomic_types``, -1 for the others."""
        device = torch.device(device)
        if device not in self._tables:
            t = torch.full((self.max_z + 1,), -1, dtype=torch.int32)
            t[torch.tensor(self.atomic_types, dtype=torch.long)] = torch.arange(self.n_types, dtype=torch.int32)
            self._tables[device] = t.to(device)
        return self._tables[device]

    def _geometry(self, batch):
        for k in BATCH_KEYS:
            if k not in batch:
                raise ValueError(f"not a collated batch: '{k}' is missing")
        species, sysidx = batch["species"], batch["system_indices"]
        rt._require_cuda(species, sysidx)
        if species.dtype != torch.int32 or sysidx.dtype != torch.int32 or species.shape != sysidx.shape or species.dim() != 1:
            raise ValueError("species and system_indices must be int32 [N] (as collate makes them)")
        n_sys = int(batch["cells"].shape[0]) if "cells" in batch else int(sysidx[-1]) + 1
        return species.contiguous(), sysidx.contiguous(), n_sys

    def _blocks(self, name: str, entry, per_atom: bool, n_atoms: int, n_sys: int) -> Dict[str, torch.Tensor]:
        """The blocks of a batch entry as contiguous ``[rows, width]`` fp32 / fp64 device tensors."""
        spec = self.targets[name]["blocks"]
        entry = entry if isinstance(entry, dict) else {name: entry}
        if set(entry) != set(spec):
            raise ValueError(f"target '{name}': the batch holds the blocks {sorted(entry)}, the target was declared with {sorted(spec)}")
        rows = n_atoms if per_atom else n_sys
        out = {}
        for b, v in entry.items():
            rt._require_cuda(v)
            if v.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"target '{name}', block '{b}': float32 or float64 values, got {v.dtype}")
            w = _width(spec[b])
            if v.dim() < 1 or int(v.shape[0]) != rows or v.numel() != rows * w:
                raise ValueError(f"target '{name}', block '{b}': expected [{rows}, {spec[b]}] values "
                                 f"({'per atom' if per_atom else 'per structure'}), got the shape {tuple(v.shape)}")
            out[b] = v.detach().reshape(rows, w).contiguous()
        return out

    @staticmethod
    def _raise_on(flag: torch.Tensor, atomic_types, species: torch.Tensor) -> None:
        code = int(flag.item())
        if code & 1:
            found = sorted(set(torch.unique(species).cpu().tolist()))
            raise PetHipError(f"system contains unexpected atom types. Expected atomic types: {list(atomic_types)}, found: {found}")
        if code & 2:
            raise PetHipError("system_indices leave [0, n_systems): not a collated batch")


def species_counts(species: torch.Tensor, system_indices: torch.Tensor, n_systems: int, type_index: torch.Tensor,
                   n_types: int, error: Optional[torch.Tensor] = None):
    """``counts [S, T]`` int32 (the atoms of every type in every system, ``_compute_X_per_structure``) and ``n_atoms [S]``
    int32 (``pet_species_counts``). ``error``: an int32 device scalar the kernel ORs its flags into (see ``pet_hip.h``); the
    caller reads it."""
    rt._require_cuda(species, system_indices, type_index)
    dev = species.device
    counts = torch.empty((int(n_systems), int(n_types)), dtype=torch.int32, device=dev)
    n_atoms = torch.empty((int(n_systems),), dtype=torch.int32, device=dev)
    error = torch.zeros((), dtype=torch.int32, device=dev) if error is None else error
    with torch.cuda.device(dev):
        check(_lib.load().pet_species_counts(rt._ptr(species), rt._ptr(system_indices), int(species.numel()), int(n_systems),
                                             rt._ptr(type_index), int(type_index.numel()) - 1, int(n_types), rt._ptr(counts),
                                             rt._ptr(n_atoms), rt._ptr(error), rt._stream()))
    return counts, n_atoms, error


def _workspace(rows: int, n_types: int, width: int, device) -> torch.Tensor:
    return torch.empty(int(_lib.load().pet_baseline_workspace_bytes(int(rows), int(n_types), int(width))), dtype=torch.uint8,
                       device=device)


def _all_reduce(tensors: List[torch.Tensor], group) -> None:
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()):
        raise PetHipError("all_reduce needs an initialised torch.distributed process group")
    for t in tensors:
        dist.all_reduce(t, group=group)  # SUM, as composition/trainer.py:199-205 and scaler/trainer.py:186-198


class CompositionHip(_Fitted):
    """Least-squares per-species baselines (``atomic_baseline``): ``CompositionModel`` of the reference.

    ``targets``: ``{name: {"per_atom": bool, "shape": [components..., properties]}}`` (``"shape": {block: [...]}`` for a
    target of several blocks). Per-structure targets ``Y [S, ...]`` are fitted against the systems' type counts, per-atom
    targets ``Y [N, ...]`` get the mean of every type (a NaN stays inside its own type)."""

    def __init__(self, atomic_types: Iterable[int], targets: Dict[str, dict]):
        super().__init__(atomic_types, targets)
        t = self.n_types
        self.XTX = {n: {b: torch.zeros((t, t), dtype=torch.int64) for b in s["blocks"]} for n, s in self.targets.items()}
        self.XTY = {n: {b: torch.zeros((t, _width(sh)), dtype=torch.float64) for b, sh in s["blocks"].items()}
                    for n, s in self.targets.items()}
        self._weights: Dict[str, Dict[str, torch.Tensor]] = {}

    def _accumulators(self) -> List[torch.Tensor]:
        return [t for d in (self.XTX, self.XTY) for n in sorted(d) for _, t in sorted(d[n].items())]

    def _move(self, device) -> None:
        for d in (self.XTX, self.XTY):
            for n in d:
                d[n] = {b: t.to(device) for b, t in d[n].items()}

    def accumulate(self, batch: Dict[str, object], names: Optional[Iterable[str]] = None) -> None:
        """``XTX += X^T X``, ``XTY += X^T Y`` for every declared target (or ``names``) of a collated batch
        (``_base_composition.py:229-322``). One read-back, of the error flag: an atom of an undeclared type raises."""
        names = list(self.targets) if names is None else list(names)
        species, sysidx, n_sys = self._geometry(batch)
        dev = species.device
        self._move(dev)
        tix = self.type_index(dev)
        counts, _, flag = species_counts(species, sysidx, n_sys, tix, self.n_types)
        self._raise_on(flag, self.atomic_types, species)  # before anything is added: a refused batch leaves no trace
        lib = _lib.load()
        for name in names:
            if name not in self.targets:
                raise ValueError(f"target '{name}' was not declared; declared: {sorted(self.targets)}")
            if name not in batch:
                raise ValueError(f"the batch holds no '{name}'")
            per_atom = self.targets[name]["per_atom"]
            for b, y in self._blocks(name, batch[name], per_atom, int(species.numel()), n_sys).items():
                rows, width = int(y.shape[0]), int(y.shape[1])
                ws = _workspace(rows, self.n_types, width, dev)
                with torch.cuda.device(dev):
                    check(lib.pet_composition_accumulate(int(per_atom), rt._ptr(y), int(y.dtype == torch.float64), rows, width,
                                                         rt._ptr(counts), rt._ptr(species), rt._ptr(tix), self.max_z, self.n_types,
                                                         rt._ptr(self.XTX[name][b]), rt._ptr(self.XTY[name][b]), rt._ptr(flag),
                                                         rt._ptr(ws), ws.numel(), rt._stream()))

    def all_reduce(self, group=None) -> None:
        """Sum the accumulators over the ranks (``composition/trainer.py:199-205``); every rank then fits the same weights."""
        _all_reduce(self._accumulators(), group)

    def _fixed(self, fixed_weights) -> Dict[str, Dict[int, float]]:
        out = {}
        for name, w in (fixed_weights or {}).items():
            if name not in self.targets:
                continue  # (the reference warns and goes on, :345-350)
            if isinstance(w, float):
                w = {z: float(w) for z in self.atomic_types}
            else:
                missing = set(self.atomic_types) - set(w)
                if missing:
                    raise ValueError(f"Fixed weights for target '{name}' are missing the following atomic types: {missing}")
            out[name] = w
        return out

    def fit(self, fixed_weights: Optional[Dict[str, Union[float, Dict[int, float]]]] = None) -> None:
        """Weights from the accumulators, on the host in fp64 (``fit`` :369-467 and ``_solve_linear_system`` :713-742):
        ``(XTX + 1e-14 mean|diag XTX| I) W = XTY`` for per-structure targets, ``XTY / counts`` (0 where the count is 0) for
        per-atom ones, zeros when ``XTX`` is all zero, ``fixed_weights`` (a float or ``{Z: float}`` per target) as given."""
        fixed = self._fixed(fixed_weights)
        for name, spec in self.targets.items():
            self._weights[name] = {}
            for b in spec["blocks"]:
                xtx = self.XTX[name][b].detach().cpu().to(torch.float64)
                xty = self.XTY[name][b].detach().cpu().to(torch.float64)
                if name in fixed:
                    w = torch.tensor([fixed[name][z] for z in self.atomic_types], dtype=torch.float64)[:, None].expand_as(xty).clone()
                elif bool((xtx == 0).all()):
                    w = torch.zeros_like(xty)
                elif not spec["per_atom"]:
                    reg = 1e-14 * float(torch.diag(xtx).abs().mean())
                    w = torch.linalg.solve(xtx + reg * torch.eye(self.n_types, dtype=torch.float64), xty)
                else:
                    n = torch.diag(xtx).unsqueeze(1)
                    w = torch.where(n == 0, torch.zeros_like(xty), xty / n)
                if not bool(torch.isfinite(w).all()):
                    raise PetHipError(f"composition weights of target '{name}' (block '{b}') are not finite: NaN or infinite "
                                      "targets in the training set, or a singular fit")
                self._weights[name][b] = w

    def weights(self, name: str, block: Optional[str] = None) -> torch.Tensor:
        """``[T, P]`` fp64 host tensor, ``P`` = components x properties flattened, rows in the order of ``atomic_types``."""
        if name not in self._weights:
            raise PetHipError(f"no composition weights for '{name}': call fit() first")
        w = self._weights[name]
        if block is None:
            if len(w) != 1:
                raise ValueError(f"target '{name}' has the blocks {sorted(w)}: name one")
            block = next(iter(w))
        return w[block]

    def table(self, name: str) -> torch.Tensor:
        """``[max_Z + 1]`` fp32 per-species values indexed by atomic number (0 for the others): the ``composition`` argument
        of ``ExportedEnergyModel`` and ``ExportedLLPRModel``. Scalar targets only."""
        w = self.weights(name)
        if w.shape[1] != 1:
            raise ValueError(f"target '{name}' has {w.shape[1]} values per sample: the exported classes take a scalar table")
        out = torch.zeros(self.max_z + 1, dtype=torch.float64)
        out[torch.tensor(self.atomic_types, dtype=torch.long)] = w[:, 0]
        return out.to(torch.float32)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        out = {"atomic_types": torch.tensor(self.atomic_types, dtype=torch.int32)}
        for name, spec in self.targets.items():
            for b in spec["blocks"]:
                out[f"{name}/{b}/XTX"] = self.XTX[name][b].detach().cpu().clone()
                out[f"{name}/{b}/XTY"] = self.XTY[name][b].detach().cpu().clone()
                if name in self._weights:
                    out[f"{name}/{b}/weights"] = self._weights[name][b].clone()
        return out

    def load_state_dict(self, state: Dict[str, torch.Tensor]) -> None:
        if "atomic_types" not in state or any(not torch.is_tensor(v) for v in state.values()):
            raise PetHipError("not a CompositionHip state (the reference's TensorMap checkpoint buffers are not read)")
        if state["atomic_types"].tolist() != self.atomic_types:
            raise ValueError(f"the state was fitted for the atomic types {state['atomic_types'].tolist()}, not {self.atomic_types}")
        self._weights = {}
        for name, spec in self.targets.items():
            for b in spec["blocks"]:
                self.XTX[name][b] = state[f"{name}/{b}/XTX"].to(torch.int64).clone()
                self.XTY[name][b] = state[f"{name}/{b}/XTY"].to(torch.float64).clone()
                if f"{name}/{b}/weights" in state:
                    self._weights.setdefault(name, {})[b] = state[f"{name}/{b}/weights"].to(torch.float64).clone()


class ScalerHip(_Fitted):
    """Uncentred RMS target scales (``scale_targets: true``): ``Scaler`` of the reference.

    One scale per per-structure target, one per atomic type for a per-atom target, from ``N`` (non-NaN entries) and
    ``Y2 = sum r^2`` of the residual ``r``: the target with the baseline removed and -- per-structure targets not named in
    ``per_structure_targets`` -- divided by the atom count (``scaler/trainer.py:174-186``). Targets of several blocks or
    properties get per-block per-property scales on top (:meth:`accumulate_per_property`, :meth:`fit_per_property`;
    ``_base_scaler.py:207-213``), in the form ``TrainStep``'s ``spec["scales"]`` takes. A per-atom target of several
    properties is refused: its per-property scales are per type, which ``TrainStep`` cannot apply."""

    def __init__(self, atomic_types: Iterable[int], targets: Dict[str, dict], per_structure_targets: Iterable[str] = ()):
        super().__init__(atomic_types, targets)
        self.per_structure_targets = [str(n) for n in per_structure_targets]
        self.multi_property = []
        for name, spec in self.targets.items():
            multi = len(spec["blocks"]) > 1 or any(_n_properties(s) > 1 for s in spec["blocks"].values())
            if multi and spec["per_atom"]:
                raise ValueError(f"target '{name}' is per atom and has several blocks or properties: its per-property scales "
                                 "would be per atomic type, which TrainStep cannot apply (not served)")
            if multi:
                self.multi_property.append(name)
        rows = {n: (self.n_types if s["per_atom"] else 1) for n, s in self.targets.items()}
        self.N = {n: torch.zeros(rows[n], dtype=torch.int64) for n in self.targets}
        self.Y2 = {n: torch.zeros(rows[n], dtype=torch.float64) for n in self.targets}
        self.per_property_N = {n: {b: torch.zeros((1, _n_properties(s)), dtype=torch.int64)
                                   for b, s in self.targets[n]["blocks"].items()} for n in self.multi_property}
        self.per_property_Y2 = {n: {b: torch.zeros((1, _n_properties(s)), dtype=torch.float64)
                                    for b, s in self.targets[n]["blocks"].items()} for n in self.multi_property}
        self._scales: Dict[str, torch.Tensor] = {}
        self._property_scales: Dict[str, Dict[str, torch.Tensor]] = {}
        self._full_scales: Dict[str, Dict[str, torch.Tensor]] = {}
        self.zbl_removed: Optional[bool] = None  # what the accumulated batches declared (all of them the same)

    def _accumulators(self) -> List[torch.Tensor]:
        out = [d[n] for d in (self.N, self.Y2) for n in sorted(d)]
        return out + [t for d in (self.per_property_N, self.per_property_Y2) for n in sorted(d) for _, t in sorted(d[n].items())]

    def _move(self, device) -> None:
        for d in (self.N, self.Y2):
            for n in d:
                d[n] = d[n].to(device)
        for d in (self.per_property_N, self.per_property_Y2):
            for n in d:
                d[n] = {b: t.to(device) for b, t in d[n].items()}

    def _declare_zbl(self, zbl_removed: bool) -> None:
        if self.zbl_removed is not None and self.zbl_removed != bool(zbl_removed):
            raise PetHipError("some batches were accumulated with the ZBL term removed from their targets and some without")
        self.zbl_removed = bool(zbl_removed)

    def _moments(self, batch, composition, names, per_property: bool) -> None:
        species, sysidx, n_sys = self._geometry(batch)
        dev = species.device
        self._move(dev)
        if composition is not None and composition.atomic_types != self.atomic_types:
            raise ValueError("the composition model was built for other atomic types")
        tix = self.type_index(dev)
        counts, n_atoms, flag = species_counts(species, sysidx, n_sys, tix, self.n_types)
        self._raise_on(flag, self.atomic_types, species)
        lib = _lib.load()
        for name in names:
            if name not in self.targets:
                raise ValueError(f"target '{name}' was not declared; declared: {sorted(self.targets)}")
            if name not in batch:
                raise ValueError(f"the batch holds no '{name}'")
            per_atom = self.targets[name]["per_atom"]
            scale = None
            if per_property:
                if name not in self._scales:
                    raise PetHipError(f"per-property scales of '{name}' are fitted on top of its per-target scale: call fit() first")
                scale = self._scales[name].to(dev)
            for b, y in self._blocks(name, batch[name], per_atom, int(species.numel()), n_sys).items():
                rows, width = int(y.shape[0]), int(y.shape[1])
                w = None
                if composition is not None and name in composition.targets:
                    if composition.targets[name] != self.targets[name]:
                        raise ValueError(f"target '{name}' is declared differently in the composition model and in the scaler")
                    w = composition.weights(name, b).to(dev).contiguous()
                n_out = _n_properties(self.targets[name]["blocks"][b]) if per_property else 1
                acc_n = self.per_property_N[name][b] if per_property else self.N[name]
                acc_y2 = self.per_property_Y2[name][b] if per_property else self.Y2[name]
                ws = _workspace(rows, self.n_types, width, dev)
                with torch.cuda.device(dev):
                    check(lib.pet_target_moments(int(per_atom), rt._ptr(y), int(y.dtype == torch.float64), rows, width, n_out,
                                                 rt._ptr(counts), rt._ptr(n_atoms), int(name not in self.per_structure_targets),
                                                 rt._ptr(species), rt._ptr(tix), self.max_z, self.n_types, rt._ptr(w),
                                                 rt._ptr(scale), rt._ptr(acc_n), rt._ptr(acc_y2), rt._ptr(flag), rt._ptr(ws),
                                                 ws.numel(), rt._stream()))

    def accumulate(self, batch: Dict[str, object], composition: Optional[CompositionHip] = None, zbl_removed: bool = False,
                   names: Optional[Iterable[str]] = None) -> None:
        """``N`` and ``Y2`` of every declared target (or ``names``) of a collated batch, pooled over a target's blocks
        (``accumulate`` :372-429), on the residual formed on the fly from ``composition``'s fitted weights (None: no
        baseline). ``zbl_removed``: the batch's energies were passed through ``ZBLHip.remove_from_targets`` first -- the
        reference removes every additive model before it scales --; recorded, so that :class:`TargetTransform` can refuse
        a scaler fitted the other way."""
        self._declare_zbl(zbl_removed)
        self._moments(batch, composition, list(self.targets) if names is None else list(names), per_property=False)

    def accumulate_per_property(self, batch: Dict[str, object], composition: Optional[CompositionHip] = None,
                                zbl_removed: bool = False) -> None:
        """Per-block per-property ``N`` and ``Y2`` of the multi-property targets, on the residual divided by the fitted
        per-target scale (``accumulate_per_property`` :431-491). Single-property targets are skipped, as there."""
        self._declare_zbl(zbl_removed)
        self._moments(batch, composition, [n for n in self.multi_property if n in batch], per_property=True)

    def all_reduce(self, group=None) -> None:
        """Sum the accumulators over the ranks (``scaler/trainer.py:186-198``)."""
        _all_reduce(self._accumulators(), group)

    def fit(self, fixed_weights: Optional[Dict[str, Union[float, Dict[int, float]]]] = None) -> None:
        """``scale = sqrt(Y2 / N)``, NaN (no samples) -> 1.0 (``fit`` :493-538); ``fixed_weights``: a float, or ``{Z: float}``
        for a per-atom target (``_set_fixed_weights`` :841-916)."""
        fixed_weights = fixed_weights or {}
        for name, spec in self.targets.items():
            if name in fixed_weights:
                w = fixed_weights[name]
                if name in self.multi_property:
                    raise NotImplementedError(f"Multiple blocks or properties are not supported for fixed weights of target '{name}'")
                if isinstance(w, dict):
                    if not spec["per_atom"]:
                        raise ValueError(f"Fixed weights as a dict are not supported for per-structure target '{name}'")
                    missing = [z for z in self.atomic_types if z not in w]
                    if missing:
                        raise ValueError(f"Atomic type {missing[0]} is missing from the fixed scaling weights for target '{name}'")
                    s = torch.tensor([float(w[z]) for z in self.atomic_types], dtype=torch.float64)
                elif isinstance(w, float):
                    s = torch.full((self.N[name].numel(),), w, dtype=torch.float64)
                else:
                    raise ValueError(f"weights for '{name}' must be either a float or a dict of int to float.")
            else:
                s = (self.Y2[name].detach().cpu() / self.N[name].detach().cpu()) ** 0.5
            self._scales[name] = torch.nan_to_num(s, nan=1.0)

    def fit_per_property(self) -> None:
        """``sqrt(Y2 / N)`` per block and property, NaN -> 1.0; the full scale of a property is the per-target scale times
        this (``fit_per_property`` :540-617)."""
        for name in self.multi_property:
            if name not in self._scales:
                raise PetHipError(f"per-property scales of '{name}' multiply its per-target scale: call fit() first")
            self._property_scales[name] = {}
            for b in self.targets[name]["blocks"]:
                s = torch.sqrt(self.per_property_Y2[name][b].detach().cpu() / self.per_property_N[name][b].detach().cpu())[0]
                # the product is formed before the NaNs are replaced (:599-607): a property without samples has the FULL
                # scale 1.0, not the per-target scale
                self._full_scales.setdefault(name, {})[b] = torch.nan_to_num(self._scales[name][0] * s, nan=1.0)
                self._property_scales[name][b] = torch.nan_to_num(s, nan=1.0)

    def scale(self, name: str):
        """The per-target scale: a float, or ``[T]`` fp64 (rows in the order of ``atomic_types``) for a per-atom target."""
        if name not in self._scales:
            raise PetHipError(f"no scale for '{name}': call fit() first")
        s = self._scales[name]
        return s.clone() if self.targets[name]["per_atom"] else float(s[0])

    def property_scales(self, name: str) -> Dict[str, torch.Tensor]:
        """``{block: [n_properties]}`` fp64, what ``TrainStep``'s ``spec["scales"]`` takes; ones for a target without fitted
        per-property scales (a single-property target has none by definition)."""
        if name not in self.targets:
            raise ValueError(f"target '{name}' was not declared")
        if name in self._property_scales:
            return {b: s.clone() for b, s in self._property_scales[name].items()}
        if name in self.multi_property:
            raise PetHipError(f"no per-property scales for '{name}': call accumulate_per_property() and fit_per_property() first")
        return {b: torch.ones(_n_properties(s), dtype=torch.float64) for b, s in self.targets[name]["blocks"].items()}

    def full_scales(self, name: str) -> Dict[str, torch.Tensor]:
        """Per-target times per-property scales (``_base_scaler.py:599-601``), ``{block: [n_properties]}``, NaN -> 1.0."""
        if self.targets[name]["per_atom"]:
            raise ValueError(f"target '{name}' is per atom: its scale is per type, see scale()")
        if name in self._full_scales:
            return {b: s.clone() for b, s in self._full_scales[name].items()}
        return {b: torch.nan_to_num(self.scale(name) * s, nan=1.0) for b, s in self.property_scales(name).items()}

    def state_dict(self) -> Dict[str, torch.Tensor]:
        out = {"atomic_types": torch.tensor(self.atomic_types, dtype=torch.int32),
               "zbl_removed": torch.tensor(-1 if self.zbl_removed is None else int(self.zbl_removed), dtype=torch.int32)}
        for name in self.targets:
            out[f"{name}/N"] = self.N[name].detach().cpu().clone()
            out[f"{name}/Y2"] = self.Y2[name].detach().cpu().clone()
            if name in self._scales:
                out[f"{name}/scale"] = self._scales[name].clone()
            for b in self.per_property_N.get(name, {}):
                out[f"{name}/{b}/per_property_N"] = self.per_property_N[name][b].detach().cpu().clone()
                out[f"{name}/{b}/per_property_Y2"] = self.per_property_Y2[name][b].detach().cpu().clone()
                if name in self._property_scales:
                    out[f"{name}/{b}/per_property_scale"] = self._property_scales[name][b].clone()
                    out[f"{name}/{b}/full_scale"] = self._full_scales[name][b].clone()
        return out

    def load_state_dict(self, state: Dict[str, torch.Tensor]) -> None:
        if "atomic_types" not in state or any(not torch.is_tensor(v) for v in state.values()):
            raise PetHipError("not a ScalerHip state (the reference's TensorMap checkpoint buffers are not read)")
        if state["atomic_types"].tolist() != self.atomic_types:
            raise ValueError(f"the state was fitted for the atomic types {state['atomic_types'].tolist()}, not {self.atomic_types}")
        z = int(state["zbl_removed"])
        self.zbl_removed = None if z < 0 else bool(z)
        self._scales, self._property_scales, self._full_scales = {}, {}, {}
        for name in self.targets:
            self.N[name] = state[f"{name}/N"].to(torch.int64).clone()
            self.Y2[name] = state[f"{name}/Y2"].to(torch.float64).clone()
            if f"{name}/scale" in state:
                self._scales[name] = state[f"{name}/scale"].to(torch.float64).clone()
            for b in self.per_property_N.get(name, {}):
                self.per_property_N[name][b] = state[f"{name}/{b}/per_property_N"].to(torch.int64).clone()
                self.per_property_Y2[name][b] = state[f"{name}/{b}/per_property_Y2"].to(torch.float64).clone()
                if f"{name}/{b}/per_property_scale" in state:
                    self._property_scales.setdefault(name, {})[b] = state[f"{name}/{b}/per_property_scale"].to(torch.float64).clone()
                    self._full_scales.setdefault(name, {})[b] = state[f"{name}/{b}/full_scale"].to(torch.float64).clone()


def targets_remove(per_atom: bool, values: torch.Tensor, gradient_arrays: Iterable[torch.Tensor], counts: Optional[torch.Tensor],
                   species: torch.Tensor, type_index: torch.Tensor, n_types: int, weights: Optional[torch.Tensor],
                   scale: Optional[torch.Tensor], error: torch.Tensor) -> List[torch.Tensor]:
    """``pet_targets_remove``: fresh fp32 tensors ``[(values - baseline) / scale, gradient arrays / scale ...]`` in one
    launch; fp32 or fp64 in, fp64 arithmetic, one rounding. ``values [rows, width]``; ``weights [T, width]`` and ``scale``
    (``[1]``, or ``[T]`` per atom) fp64 device tensors or None."""
    arrays = [values] + list(gradient_arrays)
    if len(arrays) > _lib.PET_TARGET_MAX_ARRAYS:
        raise ValueError(f"at most {_lib.PET_TARGET_MAX_ARRAYS - 1} gradient arrays go with a target")
    rt._require_cuda(*arrays, species, type_index, error, *[t for t in (counts, weights, scale) if t is not None])
    descs, outs, keep = [], [], []
    for k, a in enumerate(arrays):
        if a.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"float32 or float64 values, got {a.dtype}")
        x = a.detach().contiguous()
        x = x.reshape(x.shape[0], -1) if k == 0 else x.reshape(-1, 1)  # a gradient array is scaled entry by entry
        out = torch.empty(a.shape, dtype=torch.float32, device=a.device)
        keep.append(x)
        outs.append(out)
        descs.append(_lib.TargetArray(x.data_ptr(), out.data_ptr(), int(x.shape[0]), int(x.shape[1]), int(x.dtype == torch.float64)))
    if weights is not None and (weights.dtype != torch.float64 or tuple(weights.shape) != (n_types, descs[0].width)):
        raise ValueError(f"weights must be float64 [{n_types}, {descs[0].width}], got {weights.dtype} {tuple(weights.shape)}")
    if scale is not None and (scale.dtype != torch.float64 or scale.numel() != (n_types if per_atom else 1)):
        raise ValueError(f"scale must be float64 [{n_types if per_atom else 1}], got {scale.dtype} {tuple(scale.shape)}")
    with torch.cuda.device(values.device):
        check(_lib.load().pet_targets_remove(int(per_atom), len(descs), (_lib.TargetArray * len(descs))(*descs), rt._ptr(counts),
                                             rt._ptr(species), rt._ptr(type_index), int(type_index.numel()) - 1, int(n_types),
                                             rt._ptr(weights), rt._ptr(scale), rt._ptr(error), rt._stream()))
    return outs


class TargetTransform:
    """The per-step target transform of the reference's training loop (``get_remove_additive_transform`` for every additive
    model, then the scaler's ``remove=True`` with per-target scales), on a collated batch: composition removed, ZBL removed
    through ``ZBLHip.remove_from_targets`` when ``zbl`` is given, scale removed. fp64 raw targets go in, fp32 residuals come
    out.

    ``__call__(batch, names, graph=None)`` with ``names = {"energies": key, "gradients": key, "strain_gradients": key,
    "extra": [keys]}`` (every entry optional; the values are the batch's keys and the targets' declared names) returns a new
    dict with the keyword arguments of ``TrainStep.__call__`` / ``SoapTrainStep.__call__``: ``target_energies [S]``,
    ``target_gradients [N,3]``, ``target_strain_gradients [S,3,3]`` (each only when named), ``extra_targets = {name:
    {"values", "per_atom", "scales"}}`` with the scaler's per-property scales, and ``n_atoms [S]`` fp32. The batch is left alone.

    The composition baseline of a scalar is a scalar, and a per-target scale is one number (per type): both commute with a
    rotation of scalar, vector and rank-2 targets. So the transform is applied ONCE to a cached collated batch, before
    ``O3Augmenter``, and serves every epoch; gradient arrays only lose the scale (the baseline does not depend on
    positions). ``composition`` or ``scaler`` may be None (that step is skipped)."""

    def __init__(self, composition: Optional[CompositionHip], scaler: Optional[ScalerHip], zbl=None):
        if composition is None and scaler is None:
            raise ValueError("TargetTransform needs a composition model or a scaler")
        if composition is not None and scaler is not None and composition.atomic_types != scaler.atomic_types:
            raise ValueError("the composition model and the scaler were built for different atomic types")
        if scaler is not None and scaler.zbl_removed is not None and scaler.zbl_removed != (zbl is not None):
            raise PetHipError("the scaler was fitted on targets " + ("with" if scaler.zbl_removed else "without") +
                              " the ZBL term removed, the transform is set up the other way")
        self.composition, self.scaler, self.zbl = composition, scaler, zbl
        self._types = composition if composition is not None else scaler

    def _declared(self, name: str):
        for m in (self.scaler, self.composition):
            if m is not None and name in m.targets:
                return m, m.targets[name]
        raise ValueError(f"target '{name}' was declared neither in the composition model nor in the scaler")

    def _parts(self, name: str, block: str, per_atom: bool, dev):
        w = s = None
        if self.composition is not None and name in self.composition.targets:
            w = self.composition.weights(name, block).to(dev).contiguous()
        if self.scaler is not None and name in self.scaler.targets:
            s = self.scaler._scales.get(name)
            if s is None:
                raise PetHipError(f"no scale for '{name}': call fit() first")
            s = s.to(dev).contiguous()
        return w, s

    def __call__(self, batch: Dict[str, object], names: Dict[str, object], graph=None) -> Dict[str, object]:
        unknown = set(names) - {"energies", "gradients", "strain_gradients", "extra"}
        if unknown:
            raise ValueError(f"unknown roles {sorted(unknown)}: expected 'energies', 'gradients', 'strain_gradients', 'extra'")
        ty = self._types
        species, sysidx, n_sys = ty._geometry(batch)
        dev = species.device
        tix = ty.type_index(dev)
        counts, n_atoms, flag = species_counts(species, sysidx, n_sys, tix, ty.n_types)
        out: Dict[str, object] = {}
        e_key, g_key, s_key = names.get("energies"), names.get("gradients"), names.get("strain_gradients")
        if e_key is None and (g_key is not None or s_key is not None):
            raise ValueError("gradients and strain gradients go with an energy target: name it under 'energies'")
        if e_key is not None:
            holder, decl = self._declared(e_key)
            if decl["per_atom"] or [_width(s) for s in decl["blocks"].values()] != [1] or isinstance(batch[e_key], dict):
                raise ValueError(f"'{e_key}' must be a per-structure scalar target of one block")
            w, s = self._parts(e_key, e_key, False, dev)
            e = holder._blocks(e_key, batch[e_key], False, int(species.numel()), n_sys)[e_key]
            grads = [batch[k] for k in (g_key, s_key) if k is not None]
            if g_key is not None and tuple(batch[g_key].shape) != (int(species.numel()), 3):
                raise ValueError(f"'{g_key}' must be dE/dR [N,3], got {tuple(batch[g_key].shape)}")
            if s_key is not None and tuple(batch[s_key].shape) != (n_sys, 3, 3):
                raise ValueError(f"'{s_key}' must be dE/d(strain) [S,3,3], got {tuple(batch[s_key].shape)}")
            if self.zbl is None:
                res = targets_remove(False, e, grads, counts, species, tix, ty.n_types, w, s, flag)
            else:
                # the reference's order: composition, then ZBL, then the scale. The composition comes off in fp64 and the
                # residual -- a few eV, not 1e5 -- is rounded to fp32, the precision of the ZBL energies themselves; a
                # second launch divides by the scale.
                if graph is None:
                    graph = {k: batch[k] for k in ("positions", "cells", "species", "system_indices")}
                    if "pbcs" in batch:
                        graph["pbcs"] = batch["pbcs"]
                e32 = targets_remove(False, e, [], counts, species, tix, ty.n_types, w, None, flag)[0]
                ze, zg, zs = self.zbl.remove_from_targets(graph, batch["positions"], batch["cells"], e32.reshape(n_sys),
                                                          None if g_key is None else batch[g_key],
                                                          None if s_key is None else batch[s_key])
                res = targets_remove(False, ze.reshape(n_sys, 1), [t for t in (zg, zs) if t is not None], counts, species, tix,
                                     ty.n_types, None, s, flag)
            out["target_energies"] = res[0].reshape(n_sys)
            rest = res[1:]
            if g_key is not None:
                out["target_gradients"], rest = rest[0], rest[1:]
            if s_key is not None:
                out["target_strain_gradients"] = rest[0]
        extra = {}
        for name in names.get("extra") or []:
            holder, decl = self._declared(name)
            per_atom = decl["per_atom"]
            values = {}
            for b, y in holder._blocks(name, batch[name], per_atom, int(species.numel()), n_sys).items():
                w, s = self._parts(name, b, per_atom, dev)
                src = batch[name][b] if isinstance(batch[name], dict) else batch[name]
                values[b] = targets_remove(per_atom, y, [], counts, species, tix, ty.n_types, w, s, flag)[0].reshape(src.shape)
            spec = {"values": values if isinstance(batch[name], dict) else values[name], "per_atom": per_atom}
            if self.scaler is not None and name in self.scaler.multi_property:
                spec["scales"] = self.scaler.property_scales(name)
            extra[name] = spec
        if extra:
            out["extra_targets"] = extra
        ty._raise_on(flag, ty.atomic_types, species)  # one read-back for the whole batch
        out["n_atoms"] = n_atoms.to(torch.float32)
        return out
