"""TorchScript surface of the PET hot path: ``torch.classes.pet_hip.PetHipModule`` from
``lib/libpet_hip_torch.so`` (csrc/torch_ops.cpp) wrapped in a scriptable ``torch.nn.Module``.

An exported model (``mtt export`` -> ``torch.jit.save``, ``cli/export.py:235-266``) needs every op reachable from
``forward`` to be TorchScript-visible; this module is what ``PET.forward`` (``pet/model.py:416-537``) would hold in
place of the eager ``PETBackend`` when it is scripted: per-atom energies that are differentiable w.r.t. positions and
cells inside TorchScript, weights pickled with the module. MD engines load it after
``torch.ops.load_library("libpet_hip_torch.so")``.
"""
import os
from typing import Dict, List, NamedTuple, Optional

import torch

from ..build import TORCH_LIB
from ..runtime import hypers_struct, refuse_long_range
from .._lib import PetHipError

_loaded = False


def load_ops() -> None:
    """Register ``torch.classes.pet_hip.*`` (idempotent). Raises if the library has not been built."""
    global _loaded
    if _loaded:
        return
    if not os.path.exists(TORCH_LIB):
        raise PetHipError(f"{TORCH_LIB} not found: build it with `python -m metatrain_amd.build`")
    from .. import _lib

    _lib.load()  # libpet_hip.so first (and torch before both): one HIP runtime
    torch.ops.load_library(TORCH_LIB)
    _loaded = True


def make_zbl(hypers: dict, atomic_types: List[int], zbl=None):
    """``torch.classes.pet_hip.ZblTable`` of a model, or None when it has no ZBL term. ``zbl``: a
    :class:`~metatrain_amd.zbl.ZBLHip` (e.g. ``ZBLHip.from_state_dict`` of the checkpoint's ``additive_models`` buffers),
    ``True`` (the default radii table) or None (``hypers["zbl"]`` decides). The exported model evaluates ZBL on the model's
    own neighbour list (one graph per call), so a model whose list does not hold every ZBL pair is refused."""
    from ..zbl import ZBLHip

    if zbl is None or zbl is False:
        if not hypers.get("zbl", False) or zbl is False:
            return None
        zbl = True
    if zbl is True:
        zbl = ZBLHip(atomic_types)
    if list(zbl.atomic_types) != [int(z) for z in atomic_types]:
        raise PetHipError("the ZBL model and the PET model list different atomic types")
    if hypers.get("num_neighbors_adaptive"):
        raise PetHipError("zbl with num_neighbors_adaptive: the adaptive cutoff drops edges inside the ZBL range, so the "
                          "exported model cannot share its neighbour list; evaluate ZBLHip on its own graph "
                          "(ZBLHip.graph_for)")
    if float(hypers["cutoff"]) + 1e-6 < zbl.cutoff:
        raise PetHipError(f"zbl needs a neighbour list of {zbl.cutoff:.2f} A (twice the largest covalent radius) but the "
                          f"model's cutoff is {float(hypers['cutoff']):.2f} A: the exported model cannot share its "
                          "neighbour list; evaluate ZBLHip on its own graph (ZBLHip.graph_for)")
    load_ops()
    return torch.classes.pet_hip.ZblTable([int(z) for z in zbl.atomic_types], [float(r) for r in zbl.covalent_radii])


class CoreAndZbl(NamedTuple):
    """What :func:`make_core_and_zbl` returns: the ``PetHipModule`` and the model's ``ZblTable`` (None without ZBL)."""
    core: object
    zbl: object


def make_core_and_zbl(hypers: dict, atomic_types: List[int], state_dict: Dict[str, torch.Tensor], target: str,
                      block: Optional[str] = None, zbl=None) -> CoreAndZbl:
    """The two parts of an exported model, whatever ``hypers["zbl"]`` says: ``(core, zbl)`` with ``zbl`` the ``ZblTable``
    of :func:`make_zbl` or None. ``ExportedEnergyModel(parts.core, scale, composition, zbl=parts.zbl)``."""
    table = make_zbl(hypers, atomic_types, zbl)
    return CoreAndZbl(make_core(hypers, atomic_types, state_dict, target, block, zbl=table if table is not None else False),
                      table)


def make_core(hypers: dict, atomic_types: List[int], state_dict: Dict[str, torch.Tensor], target: str,
              block: Optional[str] = None, zbl=None):
    """``torch.classes.pet_hip.PetHipModule`` for one target of a reference-schema state dict: the network alone, always.
    For a model with ``hypers["zbl"]`` set the caller must say what becomes of the ZBL term, since the core does not hold
    it: ``zbl`` is the ``ZblTable`` of :func:`make_zbl` that goes to :class:`ExportedEnergyModel` /
    :class:`ExportedLLPRModel` ``(..., zbl=table)`` with this core (:func:`make_core_and_zbl` does both), or ``False`` for
    the bare network (training-side comparisons). Leaving it None for such a model raises."""
    if hypers.get("zbl", False) and zbl is None:
        raise PetHipError("this model has `zbl: true` and the core evaluates the network alone: build both parts with "
                          "make_core_and_zbl(...) and pass its table as ExportedEnergyModel(core, ..., zbl=table), or "
                          "pass zbl=False for the bare network")
    refuse_long_range(hypers, "the scripted model (ExportedEnergyModel, csrc/torch_ops.cpp)")
    load_ops()
    block = block or target
    h = hypers_struct(hypers, atomic_types)
    numbers = [float(getattr(h, name)) for name, _ in h._fields_]
    keys, tensors = [], []
    for key, t in state_dict.items():
        parts = key.split(".")
        if parts[0] in ("node_heads", "edge_heads", "node_last_layers", "edge_last_layers"):
            if parts[1] != target:
                continue
            parts[1] = "@"
            if parts[0].endswith("last_layers"):
                if parts[3] != block:
                    continue
                parts[3] = "@"
        keys.append(".".join(parts))
        t = t.detach().cpu()
        if hypers["activation"] == "SiLU" and ".w_in." in key:
            t = torch.cat([t, t], dim=0)  # silu(W x + b) on the SwiGLU stage: value half = gate half (runtime.py)
        tensors.append(t.contiguous())
    return torch.classes.pet_hip.PetHipModule(numbers, [int(z) for z in atomic_types], keys, tensors)


class PETScriptModule(torch.nn.Module):
    """Scriptable: ``forward(positions, cells, centers, neighbors, cell_shifts, species, system_indices)`` ->
    per-atom predictions ``[N, 1]`` of one target (sum them per system for energies; autograd for forces)."""

    def __init__(self, core):
        super().__init__()
        self.core = core

    def forward(self, positions: torch.Tensor, cells: torch.Tensor, centers: torch.Tensor, neighbors: torch.Tensor,
                cell_shifts: torch.Tensor, species: torch.Tensor, system_indices: torch.Tensor) -> torch.Tensor:
        return self.core.atomic_energies(positions, cells, centers, neighbors, cell_shifts, species, system_indices)

    @torch.jit.export
    def energies_and_llf(self, positions: torch.Tensor, cells: torch.Tensor, centers: torch.Tensor,
                         neighbors: torch.Tensor, cell_shifts: torch.Tensor, species: torch.Tensor,
                         system_indices: torch.Tensor):
        return self.core.atomic_energies_and_llf(positions, cells, centers, neighbors, cell_shifts, species,
                                                 system_indices)


class PETZblScriptModule(torch.nn.Module):
    """:class:`PETScriptModule` with the ZBL per-atom energies as a second column: ``[N, 2]`` = (PET, ZBL), both from one
    graph build and one autograd node (its backward adds the ZBL ``dL/dR`` and ``dL/dcell``)."""

    def __init__(self, core, zbl):
        super().__init__()
        self.core = core
        self.zbl = zbl

    def forward(self, positions: torch.Tensor, cells: torch.Tensor, centers: torch.Tensor, neighbors: torch.Tensor,
                cell_shifts: torch.Tensor, species: torch.Tensor, system_indices: torch.Tensor) -> torch.Tensor:
        pet, rep = self.core.atomic_energies_zbl(positions, cells, centers, neighbors, cell_shifts, species,
                                                 system_indices, self.zbl)
        return torch.cat([pet, rep], dim=1)

    @torch.jit.export
    def energies_and_llf(self, positions: torch.Tensor, cells: torch.Tensor, centers: torch.Tensor,
                         neighbors: torch.Tensor, cell_shifts: torch.Tensor, species: torch.Tensor,
                         system_indices: torch.Tensor):
        pet, rep, llf = self.core.atomic_energies_and_llf_zbl(positions, cells, centers, neighbors, cell_shifts, species,
                                                              system_indices, self.zbl)
        return torch.cat([pet, rep], dim=1), llf


class EnergyAndForces(torch.nn.Module):
    """What an exported model does around the core: total energies per system and forces by autograd, all inside
    TorchScript."""

    def __init__(self, core, n_systems_hint: int = 1):
        super().__init__()
        self.pet = PETScriptModule(core)

    def forward(self, positions: torch.Tensor, cells: torch.Tensor, centers: torch.Tensor, neighbors: torch.Tensor,
                cell_shifts: torch.Tensor, species: torch.Tensor, system_indices: torch.Tensor):
        positions = positions.detach().requires_grad_(True)
        atomic = self.pet(positions, cells, centers, neighbors, cell_shifts, species, system_indices)
        energies = torch.zeros(cells.shape[0], dtype=atomic.dtype, device=atomic.device).index_add(
            0, system_indices.to(torch.long), atomic[:, 0])
        grads = torch.autograd.grad([energies.sum()], [positions])
        g = grads[0]
        assert g is not None
        return energies, -g


class ExportedEnergyModel(torch.nn.Module):
    """Tensor-level equivalent of what ``PET.forward`` does around the backbone at evaluation time
    (``pet/model.py:592-660``), scriptable end to end:

    * ``scale``: the scaler's per-target factor (``utils/scaler``: prediction * scale),
    * ``composition``: the additive composition model's per-species energies, indexed by atomic number
      (``utils/additive/composition.py``: + sum_i w[Z_i]); not differentiated (it does not depend on positions),
    * ``selected_atoms``: optional bool / index mask of the atoms that contribute to the per-system sums and that
      are returned per atom (metatomic's ``selected_atoms``); forces are still returned for every atom,
    * forces ``-dE/dR`` and, on request, the stress ``(1/V) dE/d(strain)`` assembled from ``dE/dR`` and
      ``dE/dcell`` of the HIP backward (``utils/evaluate_model.py`` strain trick, done analytically:
      ``dE/deps = R^T dE/dR + h^T dE/dh``).

    * ``zbl``: the ``ZblTable`` of a ``zbl: true`` model (:func:`make_zbl`, :func:`make_core_and_zbl`): per-atom
      and per-system energies are ``scale * PET + composition + ZBL`` -- the scaler does not touch additive terms
      (``pet/model.py:595-660``) --, forces and stress include the ZBL term, ``selected_atoms`` masks it like the rest.

    ``forward`` returns ``(energies [S], forces [N, 3], stress [S, 3, 3] or empty, per_atom [n_selected])``."""

    def __init__(self, core, scale: float = 1.0, composition: Optional[torch.Tensor] = None, zbl=None):
        super().__init__()
        self.pet = PETScriptModule(core) if zbl is None else PETZblScriptModule(core, zbl)
        self.scale = float(scale)
        self.register_buffer("composition", composition.detach().clone().to(torch.float32)
                             if composition is not None else torch.zeros(0, dtype=torch.float32))

    def forward(self, positions: torch.Tensor, cells: torch.Tensor, centers: torch.Tensor, neighbors: torch.Tensor,
                cell_shifts: torch.Tensor, species: torch.Tensor, system_indices: torch.Tensor,
                selected_atoms: Optional[torch.Tensor] = None, with_stress: bool = False):
        positions = positions.detach().requires_grad_(True)
        cells = cells.detach().requires_grad_(with_stress)
        out = self.pet(positions, cells, centers, neighbors, cell_shifts, species, system_indices)
        atomic = out[:, 0]
        atomic = atomic * self.scale
        if out.shape[1] > 1:  # the ZBL column of PETZblScriptModule: added after the scaler
            atomic = atomic + out[:, 1]
        keep = torch.ones(positions.shape[0], dtype=torch.bool, device=positions.device)
        if selected_atoms is not None:
            if selected_atoms.dtype == torch.bool:
                keep = selected_atoms.to(positions.device)
            else:
                keep = torch.zeros_like(keep).index_fill(0, selected_atoms.to(positions.device, torch.long), True)
        masked = torch.where(keep, atomic, torch.zeros_like(atomic))
        sysl = system_indices.to(torch.long)
        energies = torch.zeros(cells.shape[0], dtype=atomic.dtype, device=atomic.device).index_add(0, sysl, masked)
        wrt = [positions, cells] if with_stress else [positions]
        grads = torch.autograd.grad([energies.sum()], wrt)
        g_pos = grads[0]
        assert g_pos is not None
        stress = torch.zeros((0, 3, 3), dtype=atomic.dtype, device=atomic.device)
        if with_stress:
            g_cell = grads[1]
            assert g_cell is not None
            outer = positions.detach().unsqueeze(2) * g_pos.unsqueeze(1)  # [N, 3, 3]: R_a dE/dR_b per atom
            virial = torch.zeros((cells.shape[0], 3, 3), dtype=atomic.dtype, device=atomic.device).index_add(
                0, sysl, outer)
            virial = virial + torch.matmul(cells.detach().transpose(1, 2), g_cell)
            volume = torch.abs(torch.linalg.det(cells.detach()))
            stress = virial / volume.clamp_min(1e-30).reshape(-1, 1, 1)
        per_atom = atomic.detach()
        energies = energies.detach()
        if self.composition.numel() > 0:
            base = self.composition[species.to(torch.long)].to(atomic.dtype)
            per_atom = per_atom + base
            energies = energies + torch.zeros_like(energies).index_add(
                0, sysl, torch.where(keep, base, torch.zeros_like(base)))
        return energies, -g_pos, stress, per_atom[keep]


class ExportedLLPRModel(torch.nn.Module):
    """:class:`ExportedEnergyModel` plus the LLPR outputs of the energy (``llpr/model.py:362-670``), scriptable end to end:
    the per-atom energies and the last-layer features come from ONE backbone forward (``atomic_energies_and_llf``), the
    per-system rows, sigma and the ensemble from the HIP kernels behind ``pet_llpr_*``.

    ``llpr_state``: ``LLPRUncertainty.state_dict()`` of the same model (``covariance_energy_uncertainty``,
    ``cholesky_energy_uncertainty``, ``multiplier_energy_uncertainty`` and, for an ensemble,
    ``llpr_ensemble_layers.energy.weight``); pickled with the module as buffers (the dots of the last name replaced by
    underscores), with the fp32 inverse Cholesky factor the variance kernel reads.

    ``forward`` returns ``(energies [S], forces [N, 3], stress [S, 3, 3] or empty, per_atom [n_selected],
    energy_uncertainty [S], energy_uncertainty per selected atom [n_selected] or empty, energy_ensemble [S, K] or empty)``.
    Ensemble members carry no forces (one adjoint per member: not served). With ``zbl`` (as in
    :class:`ExportedEnergyModel`) the energies -- and so the mean the ensemble is centred on -- include the ZBL term;
    uncertainties and the spread of the ensemble do not change."""

    def __init__(self, core, llpr_state: Dict[str, torch.Tensor], scale: float = 1.0,
                 composition: Optional[torch.Tensor] = None, zbl=None):
        super().__init__()
        self.pet = PETScriptModule(core) if zbl is None else PETZblScriptModule(core, zbl)
        self.scale = float(scale)
        self.register_buffer("composition", composition.detach().clone().to(torch.float32)
                             if composition is not None else torch.zeros(0, dtype=torch.float32))
        chol = llpr_state["cholesky_energy_uncertainty"].detach().to(torch.float64).cpu()
        mult = llpr_state["multiplier_energy_uncertainty"].detach().to(torch.float64).cpu().reshape(-1)
        if mult.numel() != 1:
            raise PetHipError("the energy has one property: multiplier_energy_uncertainty must hold one number")
        if not bool(chol.diagonal().ne(0).all()):
            raise PetHipError("no Cholesky factor in the LLPR state (compute_cholesky_decomposition)")
        inv = torch.tril(torch.linalg.solve_triangular(chol, torch.eye(chol.shape[0], dtype=torch.float64), upper=False))
        self.register_buffer("covariance_energy_uncertainty",
                             llpr_state["covariance_energy_uncertainty"].detach().clone().to(torch.float64))
        self.register_buffer("cholesky_energy_uncertainty", chol.clone())
        self.register_buffer("multiplier_energy_uncertainty", mult.clone())
        self.register_buffer("inverse_cholesky", inv.to(torch.float32))
        w = llpr_state.get("llpr_ensemble_layers.energy.weight")
        self.register_buffer("llpr_ensemble_layers_energy_weight",
                             w.detach().clone().to(torch.float32) if w is not None else torch.zeros((0, chol.shape[0])))
        self.alpha = float(mult[0])
        self.num_ensemble_members = int(self.llpr_ensemble_layers_energy_weight.shape[0])

    def forward(self, positions: torch.Tensor, cells: torch.Tensor, centers: torch.Tensor, neighbors: torch.Tensor,
                cell_shifts: torch.Tensor, species: torch.Tensor, system_indices: torch.Tensor,
                selected_atoms: Optional[torch.Tensor] = None, with_stress: bool = False,
                per_atom_uncertainty: bool = False, with_ensemble: bool = True):
        # energies, forces, stress, per-atom energies: the operations of ExportedEnergyModel.forward, in the same order
        positions = positions.detach().requires_grad_(True)
        cells = cells.detach().requires_grad_(with_stress)
        atomic2, llf = self.pet.energies_and_llf(positions, cells, centers, neighbors, cell_shifts, species, system_indices)
        atomic = atomic2[:, 0]
        atomic = atomic * self.scale
        if atomic2.shape[1] > 1:  # the ZBL column: added after the scaler
            atomic = atomic + atomic2[:, 1]
        keep = torch.ones(positions.shape[0], dtype=torch.bool, device=positions.device)
        if selected_atoms is not None:
            if selected_atoms.dtype == torch.bool:
                keep = selected_atoms.to(positions.device)
            else:
                keep = torch.zeros_like(keep).index_fill(0, selected_atoms.to(positions.device, torch.long), True)
        masked = torch.where(keep, atomic, torch.zeros_like(atomic))
        sysl = system_indices.to(torch.long)
        energies = torch.zeros(cells.shape[0], dtype=atomic.dtype, device=atomic.device).index_add(0, sysl, masked)
        wrt = [positions, cells] if with_stress else [positions]
        grads = torch.autograd.grad([energies.sum()], wrt)
        g_pos = grads[0]
        assert g_pos is not None
        stress = torch.zeros((0, 3, 3), dtype=atomic.dtype, device=atomic.device)
        if with_stress:
            g_cell = grads[1]
            assert g_cell is not None
            outer = positions.detach().unsqueeze(2) * g_pos.unsqueeze(1)
            virial = torch.zeros((cells.shape[0], 3, 3), dtype=atomic.dtype, device=atomic.device).index_add(
                0, sysl, outer)
            virial = virial + torch.matmul(cells.detach().transpose(1, 2), g_cell)
            volume = torch.abs(torch.linalg.det(cells.detach()))
            stress = virial / volume.clamp_min(1e-30).reshape(-1, 1, 1)
        per_atom = atomic.detach()
        energies = energies.detach()
        if self.composition.numel() > 0:
            base = self.composition[species.to(torch.long)].to(atomic.dtype)
            per_atom = per_atom + base
            energies = energies + torch.zeros_like(energies).index_add(
                0, sysl, torch.where(keep, base, torch.zeros_like(base)))
        # LLPR: per-system rows of the selected atoms -> sigma and the ensemble re-centred on the energies
        mask = keep.to(torch.uint8) if selected_atoms is not None else torch.zeros(0, dtype=torch.uint8)
        # (the buffers follow the inputs' device: a no-op once the module was moved there)
        inv = self.inverse_cholesky.to(llf.device)
        rows = self.pet.core.llpr_rows(llf, system_indices.to(llf.device), cells.shape[0], mask.to(llf.device))
        sigma = self.pet.core.llpr_variance(rows, inv, self.alpha)
        sigma_atom = torch.zeros(0, dtype=sigma.dtype, device=sigma.device)
        if per_atom_uncertainty:
            sigma_atom = self.pet.core.llpr_variance(llf[keep], inv, self.alpha)
        ensemble = torch.zeros((0, 0), dtype=sigma.dtype, device=sigma.device)
        if with_ensemble and self.num_ensemble_members > 0:
            ensemble = self.pet.core.llpr_ensemble(rows, self.llpr_ensemble_layers_energy_weight.to(llf.device),
                                                   self.num_ensemble_members, energies.unsqueeze(1))
        return energies, -g_pos, stress, per_atom[keep], sigma, sigma_atom, ensemble
