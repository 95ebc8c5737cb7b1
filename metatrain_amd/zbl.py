"""ZBL short-range repulsion (``utils/additive/zbl.py``) on the HIP path: the additive model of ``zbl: true``.

The reference subtracts the ZBL energy and its gradients from the targets before training (``utils/additive/remove.py``),
trains the network on the remainder and adds the ZBL term back, after the scaler, at evaluation (``pet/model.py:616-660``).
:class:`ZBLHip` is that model: per-atom energies, ``dL/dR``, ``dL/dcell``, the strain gradient and Hessian-vector
products from the kernels of ``csrc/zbl.hip`` on a :class:`~metatrain_amd.runtime.HipGraph`,
:meth:`ZBLHip.remove_from_targets` for training and the reference's two checkpoint buffers. eV and Angstrom only, like the reference.
"""
import logging
from ctypes import byref, c_double, c_int32, c_void_p
from typing import Dict, List, Optional

import torch

from . import _lib
from . import runtime as rt
from ._lib import PetHipError, check

# Covalent radii in Angstrom for Z = 1 .. 36 (Cordero et al. 2008, the values ASE tabulates as ``ase.data.covalent_radii``).
# Written from memory, NOT verified against ASE: a checkpoint's own ``covalent_radii`` buffer always wins
# (:meth:`ZBLHip.from_state_dict`), and other values can be passed as ``covalent_radii={Z: radius}``.
DEFAULT_COVALENT_RADII: Dict[int, float] = {
    1: 0.31, 2: 0.28, 3: 1.28, 4: 0.96, 5: 0.84, 6: 0.76, 7: 0.71, 8: 0.66, 9: 0.57, 10: 0.58,
    11: 1.66, 12: 1.41, 13: 1.21, 14: 1.11, 15: 1.07, 16: 1.05, 17: 1.02, 18: 1.06,
    19: 2.03, 20: 1.76, 21: 1.70, 22: 1.60, 23: 1.53, 24: 1.39, 25: 1.39, 26: 1.32, 27: 1.26, 28: 1.24, 29: 1.32,
    30: 1.22, 31: 1.22, 32: 1.20, 33: 1.19, 34: 1.20, 35: 1.20, 36: 1.16,
}


def zbl_on_model_graph(zbl, wanted: bool, atomic_types: List[int], cutoff: float, adaptive: bool, what: str):
    """The :class:`ZBLHip` an entry point that evaluates on the model's own neighbour list adds, or None for a model
    without ZBL. ``zbl``: a ``ZBLHip`` (a checkpoint's radii), ``True`` (default radii), ``False`` (the network alone, on
    purpose) or None (``wanted``, the model's ``zbl`` hyper, decides). Raises when that list does not hold every ZBL pair:
    ``what`` names the entry point in the message."""
    if zbl is False or (zbl is None and not wanted):
        return None
    if zbl is None or zbl is True:
        zbl = ZBLHip(atomic_types)
    if list(zbl.atomic_types) != [int(z) for z in atomic_types]:
        raise PetHipError("the ZBL model and the model list different atomic types")
    if adaptive:
        raise PetHipError(f"zbl with num_neighbors_adaptive: the adaptive cutoff drops edges inside the ZBL range, and {what} "
                          "evaluates ZBL on the model's own neighbour list")
    if float(cutoff) + 1e-6 < zbl.cutoff:
        raise PetHipError(f"the model's cutoff {float(cutoff):.2f} A is below the ZBL cutoff {zbl.cutoff:.2f} A (twice the "
                          f"largest covalent radius): {what} evaluates ZBL on the model's own neighbour list and sizes its "
                          "halo by the model's cutoff")
    return zbl


class ZBLHip:
    """``ZBL`` of the reference for the model whose ``atomic_types`` (same list, same order: a graph's species indices
    index it) are given. ``covalent_radii``: ``{Z: radius in Angstrom}``, overriding :data:`DEFAULT_COVALENT_RADII` (an
    unverified table, see there); a type in neither is an error, a radius of 0.2 (ASE's "unknown") warns as the reference
    does."""

    def __init__(self, atomic_types: List[int], covalent_radii: Optional[Dict[int, float]] = None,
                 length_unit: str = "angstrom", energy_unit: str = "eV"):
        if str(length_unit).lower() not in ("angstrom", "a"):
            raise ValueError(f"ZBL only supports angstrom units, but a {length_unit} unit was provided.")
        if energy_unit != "eV":
            raise ValueError(f"ZBL only supports energies in eV, but a {energy_unit} unit was provided.")
        self.lib = _lib.load()
        self.atomic_types = [int(z) for z in atomic_types]
        table = dict(DEFAULT_COVALENT_RADII)
        table.update({int(z): float(r) for z, r in (covalent_radii or {}).items()})
        missing = [z for z in self.atomic_types if z not in table]
        if missing:
            raise ValueError(f"no covalent radius for atomic type(s) {missing}: pass covalent_radii={{Z: radius}}")
        self.covalent_radii = [table[z] for z in self.atomic_types]
        for z, r in zip(self.atomic_types, self.covalent_radii):
            if r == 0.2:
                logging.warning(f"Covalent radius for element {z} is not available in ASE. Using a default value of 0.2 Å.")
        n = len(self.atomic_types)
        self._handle = c_void_p()
        check(self.lib.pet_zbl_create((c_int32 * n)(*self.atomic_types), (c_double * n)(*self.covalent_radii), n,
                                      byref(self._handle)))
        self.cutoff = float(self.lib.pet_zbl_cutoff(self._handle))
        self._graph_model: Optional[rt.HipModel] = None

    def __del__(self):
        h = getattr(self, "_handle", None)
        try:
            if h is not None and h.value:
                self.lib.pet_zbl_destroy(h)
                self._handle = c_void_p()
        except Exception:
            pass

    @property
    def handle(self) -> c_void_p:
        return self._handle

    def pair_table(self) -> torch.Tensor:
        """``[n_types, n_types, 6]`` fp64 host table (rc, 1/a, K Zi Zj, A, B, C) the kernels read."""
        n = len(self.atomic_types)
        buf = (c_double * (n * n * 6))()
        check(self.lib.pet_zbl_pair_table(self._handle, buf))
        return torch.tensor(list(buf), dtype=torch.float64).reshape(n, n, 6)

    # ---- checkpoint buffers of the reference: additive_models.<k>.covalent_radii / .species_to_index ----------------
    def state_dict(self, prefix: str = "") -> Dict[str, torch.Tensor]:
        order = sorted(range(len(self.atomic_types)), key=lambda i: self.atomic_types[i])  # the reference sorts its types
        index = torch.full((max(self.atomic_types) + 1,), -1, dtype=torch.int32)
        for k, i in enumerate(order):
            index[self.atomic_types[i]] = k
        radii = torch.tensor([self.covalent_radii[i] for i in order], dtype=torch.float64)
        return {prefix + "covalent_radii": radii, prefix + "species_to_index": index}

    @classmethod
    def from_state_dict(cls, state: Dict[str, torch.Tensor], prefix: str = "",
                        atomic_types: Optional[List[int]] = None) -> "ZBLHip":
        """From a reference checkpoint's buffers (``prefix`` e.g. ``"additive_models.1."``): the radii come from the
        checkpoint, whatever the default table says. ``atomic_types``: the model's list when its order is not ascending."""
        try:
            radii = state[prefix + "covalent_radii"].detach().cpu().to(torch.float64)
            index = state[prefix + "species_to_index"].detach().cpu().to(torch.int64)
        except KeyError as e:
            raise PetHipError(f"no ZBL buffers under the prefix '{prefix}': missing {e}") from None
        by_z = {int(z): float(radii[int(index[z])]) for z in range(index.numel()) if int(index[z]) >= 0}
        types = sorted(by_z) if atomic_types is None else [int(z) for z in atomic_types]
        missing = [z for z in types if z not in by_z]
        if missing:
            raise ValueError(f"the checkpoint's ZBL model has no radius for atomic type(s) {missing}")
        return cls(types, covalent_radii={z: by_z[z] for z in types})

    # ---- graphs ---------------------------------------------------------------------------------------------------
    def serves(self, graph: rt.HipGraph) -> bool:
        """Whether ``graph`` holds every pair inside the ZBL range: built by a model with these atomic types at a fixed
        cutoff of at least :attr:`cutoff`."""
        m = graph.model
        return (list(m.atomic_types) == self.atomic_types and float(m.hypers["cutoff"]) + 1e-6 >= self.cutoff
                and not m.hypers.get("num_neighbors_adaptive") and getattr(graph, "_sys", None) is not None)

    def graph_for(self, graph_or_batch, pbcs=None) -> rt.HipGraph:
        """The graph ZBL runs on: the model's own ``HipGraph`` when it serves (:meth:`serves`), otherwise a second one at
        the ZBL cutoff (heavy elements, a short model cutoff, an adaptive cutoff) from a weight-less graph-only model and
        ``neighbor_list_batch``. ``graph_or_batch``: a ``HipGraph`` or ``{"positions", "cells", "species",
        "system_indices"}`` (and optionally ``"pbcs"``); ``pbcs`` ``[S][3]``: the periodic axes of every system, needed
        when a second graph is built and a cell is not zero -- a ``HipGraph`` does not record them, and a box is not
        evidence of periodicity. Systems with a zero cell are not periodic."""
        if isinstance(graph_or_batch, rt.HipGraph):
            g = graph_or_batch
            if self.serves(g):
                return g
            if getattr(g, "_sys", None) is None:
                raise PetHipError("ZBL needs positions: a graph made from batch_data has none")
            pos, cells, species, sysidx = g._pos, g._cells, g._species, g._sys
        else:
            b = graph_or_batch
            pos, cells, species, sysidx = b["positions"], b["cells"], b["species"], b["system_indices"]
            pbcs = b.get("pbcs") if pbcs is None else pbcs
        rt._require_cuda(pos, species, sysidx)
        cells = cells.to(pos.device)
        n_sys = int(cells.shape[0])
        counts = torch.bincount(sysidx.long(), minlength=n_sys).cpu().tolist()
        first = [0]
        for c in counts:
            first.append(first[-1] + int(c))
        host_cells = cells.detach().cpu().reshape(n_sys, 3, 3)
        if pbcs is None:
            if bool(host_cells.ne(0).any()):
                raise PetHipError("ZBL builds its own neighbour list here (the model's does not hold every ZBL pair) and a "
                                  "cell is not zero: pass pbcs=[[bool, bool, bool], ...], one entry per system")
            pbcs = [[False, False, False]] * n_sys
        if len(pbcs) != n_sys:
            raise PetHipError(f"pbcs has {len(pbcs)} entries for {n_sys} systems")
        pairs, _ = rt.neighbor_list_batch(pos, host_cells, pbcs, first, self.cutoff, want_vectors=False)
        if self._graph_model is None:
            from .pet.hypers import default_hypers

            gh = default_hypers()
            gh.update(cutoff=self.cutoff, cutoff_width=min(0.5, 0.5 * self.cutoff), cutoff_function="Cosine")
            self._graph_model = rt.HipModel(gh, self.atomic_types)
            self._graph_model.load_species_table()
        return rt.HipGraph(self._graph_model, pos, cells, pairs[:, 0], pairs[:, 1], pairs[:, 2:5], species, sysidx)

    # ---- the two launches -------------------------------------------------------------------------------------------
    def forward(self, graph: rt.HipGraph) -> torch.Tensor:
        """Per-atom ZBL energies ``[N]`` (``pet_zbl_forward``)."""
        dev = graph.workspace.device
        if dev.type != "cuda":
            raise PetHipError("metatrain_amd runs on MI355X only: there is no CPU path in this package.")
        atomic = torch.empty(graph.n_nodes, dtype=torch.float32, device=dev)
        check(self.lib.pet_zbl_forward(self._handle, graph.handle, rt._ptr(atomic), rt._stream()))
        return atomic

    def backward(self, graph: rt.HipGraph, grad_atomic: Optional[torch.Tensor] = None, want_cell_grad: bool = False,
                 want_strain: bool = False):
        """``dL/dR [N,3]`` for ``dL/d(atomic) = grad_atomic`` (None: ones, the plain energy), then on request ``dL/dcell``
        ``[S,3,3]`` and the direct strain gradient ``dE/d(eps) [S,3,3]`` (plain energy only), in that order
        (``pet_zbl_backward``; the pair terms are recomputed, no forward is needed)."""
        dev = graph.workspace.device
        ga = None
        if grad_atomic is not None:
            rt._require_cuda(grad_atomic)
            ga = grad_atomic.detach().to(torch.float32).reshape(-1).contiguous()
            if ga.numel() != graph.n_nodes:
                raise PetHipError(f"grad_atomic has {ga.numel()} entries for {graph.n_nodes} atoms")
        n, s = graph.n_nodes, graph.n_systems
        gpos = torch.empty((n, 3), dtype=torch.float32, device=dev)
        gcell = torch.empty((s, 3, 3), dtype=torch.float32, device=dev) if want_cell_grad else None
        gstrain = torch.empty((s, 3, 3), dtype=torch.float32, device=dev) if want_strain else None
        ws = None
        if want_cell_grad or want_strain:
            ws = torch.empty(int(self.lib.pet_zbl_workspace_bytes(n, s)), dtype=torch.uint8, device=dev)
        check(self.lib.pet_zbl_backward(self._handle, graph.handle, rt._ptr(ga), rt._ptr(gpos), rt._ptr(gcell),
                                        rt._ptr(gstrain), rt._ptr(ws), 0 if ws is None else ws.numel(), rt._stream()))
        out = [gpos] + ([gcell] if want_cell_grad else []) + ([gstrain] if want_strain else [])
        return out[0] if len(out) == 1 else tuple(out)

    def hessian_vector_product(self, graph: rt.HipGraph, u: torch.Tensor, u_cell: Optional[torch.Tensor] = None,
                               weights: Optional[torch.Tensor] = None, want_cells: bool = False, want_tangent: bool = False):
        """Hessian-vector product of the ZBL term (``pet_zbl_hessian_vector``), in the convention of
        :func:`metatrain_amd.runtime.hessian_vector_product`, to which it adds: with ``a'_i`` the derivative of the per-atom
        ZBL energies along ``(dR, dcell) = (u [N,3], u_cell [S,3,3])``, returns ``grad_R sum_i w_i a'_i`` ``[N,3]`` -- ``H u``
        of the ZBL energy for ``weights = None`` (ones) -- then, if asked for, ``grad_cell`` of the same ``[S,3,3]`` and the
        tangents ``a'_i [N]``. The pair terms are recomputed: no forward is needed."""
        rt._require_cuda(u)
        dev = u.device
        n, s = graph.n_nodes, graph.n_systems
        uu = u.detach().to(torch.float32).reshape(n, 3).contiguous()
        uc = None if u_cell is None else u_cell.detach().to(dev, torch.float32).reshape(s, 3, 3).contiguous()
        w = None if weights is None else weights.detach().to(dev, torch.float32).reshape(n).contiguous()
        hp = torch.empty((n, 3), dtype=torch.float32, device=dev)
        hc = torch.empty((s, 3, 3), dtype=torch.float32, device=dev) if want_cells else None
        tan = torch.empty(n, dtype=torch.float32, device=dev) if want_tangent else None
        ws = torch.empty(int(self.lib.pet_zbl_workspace_bytes(n, s)), dtype=torch.uint8, device=dev) if want_cells else None
        check(self.lib.pet_zbl_hessian_vector(self._handle, graph.handle, rt._ptr(w), rt._ptr(uu), rt._ptr(uc), rt._ptr(hp),
                                              rt._ptr(hc), rt._ptr(tan), rt._ptr(ws), 0 if ws is None else ws.numel(),
                                              rt._stream()))
        out = (hp,) + ((hc,) if want_cells else ()) + ((tan,) if want_tangent else ())
        return out[0] if len(out) == 1 else out

    def energies(self, graph: rt.HipGraph, atomic: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Per-structure ZBL energies ``[S]`` (fixed-order sums, ``pet_sum_over_atoms``)."""
        atomic = self.forward(graph) if atomic is None else atomic
        out = torch.zeros(graph.n_systems, dtype=torch.float32, device=atomic.device)
        check(self.lib.pet_sum_over_atoms(graph.handle, rt._ptr(atomic), rt._ptr(out), rt._stream()))
        return out

    def remove_from_targets(self, graph: rt.HipGraph, positions: torch.Tensor, cells: torch.Tensor,
                            energies: Optional[torch.Tensor] = None, gradients: Optional[torch.Tensor] = None,
                            strain_gradients: Optional[torch.Tensor] = None, pbcs=None):
        """The targets a ``zbl: true`` model trains on (``get_remove_additive_transform``, ``utils/additive/remove.py``):
        ``energies [S]``, ``gradients [N,3]`` (dE/dR = -forces) and ``strain_gradients [S,3,3]`` (dE/d strain) with the
        ZBL energy per structure, its ``dE/dR`` and its ``dE/d(eps)`` subtracted -- the tensors ``TrainStep.__call__`` /
        ``begin`` and ``SoapTrainStep.__call__`` take. ``graph``: the batch's graph (:meth:`graph_for` is applied to it, with ``pbcs``).
        Returns ``(energies, gradients, strain_gradients)`` with None where None was given."""
        rt._require_cuda(positions, *[t for t in (energies, gradients, strain_gradients) if t is not None])
        g = self.graph_for(graph, pbcs)
        if int(positions.shape[0]) != g.n_nodes or int(cells.shape[0]) != g.n_systems:
            raise PetHipError("positions / cells do not belong to this graph")
        out_e = out_g = out_s = None
        if energies is not None:
            out_e = energies - self.energies(g).to(energies.dtype).reshape(energies.shape)
        if gradients is not None or strain_gradients is not None:
            res = self.backward(g, want_strain=strain_gradients is not None)
            gpos, gstrain = res if strain_gradients is not None else (res, None)
            if gradients is not None:
                out_g = gradients - gpos.to(gradients.dtype).reshape(gradients.shape)
            if strain_gradients is not None:
                out_s = strain_gradients - gstrain.to(strain_gradients.dtype).reshape(strain_gradients.shape)
        return out_e, out_g, out_s
