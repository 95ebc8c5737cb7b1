"""Second derivatives of the PET energy w.r.t. the positions: Hessian-vector products and dense Hessian blocks.

The reference model is differentiable to second order through torch (``utils/testing/autograd.py:36-163`` runs
``gradgradcheck`` w.r.t. positions and cell), so a user gets ``H u`` from ``torch.autograd``. Here it is one call of the
C ABI, ``pet_hessian_vector`` (``csrc/gen_train.hip``: the dual forward of the size-generic training pass along ``u`` and
its joint reverse sweep carried down to the geometry), which is what phonons and vibrational modes, dimer / Lanczos
saddle searches and second-order relaxations need.

A ``zbl: true`` model has its short-range wall in the additive pair term alone, so its Hessian is the network's plus the
pair term's (``pet_zbl_hessian_vector``, ``csrc/zbl.hip``; :meth:`metatrain_amd.zbl.ZBLHip.hessian_vector_product`):
:func:`hessian` adds it when told where the term comes from (``zbl=``).

Out of scope: a Hessian-vector path on the tuned kernels (every size runs the size-generic pass), adaptive cutoffs, mixed
parameter / position derivatives beyond what training has, third order.
"""
from typing import Callable, List, Optional, Sequence

import torch

from .. import data
from .. import runtime as rt
from .._lib import PetHipError


def _zbl_term(model, zbl):
    """The :class:`~metatrain_amd.zbl.ZBLHip` whose products :func:`hessian` adds, or None. As for ``make_core``, the caller of
    a ``zbl: true`` model must say where the term goes: a ``ZBLHip`` (a checkpoint's radii), ``True`` (the default radii) or
    ``False`` (the bare network, on purpose)."""
    if zbl is None:
        if bool(getattr(model, "hypers", {}).get("zbl", False)):
            raise PetHipError("this model has a ZBL term and the network's Hessian alone is not the model's: pass zbl=<ZBLHip> "
                              "(e.g. ZBLHip.from_state_dict of the checkpoint) or zbl=True (default radii) to add the pair "
                              "term's Hessian, or zbl=False for the bare network")
        return None
    if zbl is False:
        return None
    if zbl is True:
        from ..zbl import ZBLHip

        zbl = ZBLHip(model.atomic_types)
    if list(zbl.atomic_types) != [int(z) for z in model.atomic_types]:
        raise PetHipError("the ZBL model and the model list different atomic types")
    return zbl


def replica_plan(n_atoms: int, atoms: Sequence[int], columns_per_launch: int) -> List[List[int]]:
    """The rows ``3 a + c`` of the block (``a`` in ``atoms``, ``c`` in x, y, z) split into launches of at most
    ``columns_per_launch`` rows: launch ``l`` computes ``plan[l][k]`` on replica ``k``."""
    if columns_per_launch < 1:
        raise ValueError("columns_per_launch must be at least 1")
    rows = []
    for a in atoms:
        if not 0 <= int(a) < n_atoms:
            raise ValueError(f"atom {int(a)} is not one of the system's {n_atoms}")
        rows.extend(3 * int(a) + c for c in range(3))
    return [rows[k: k + columns_per_launch] for k in range(0, len(rows), columns_per_launch)]


def hessian_from_hvp(hvp: Callable[[torch.Tensor], torch.Tensor], n_atoms: int, atoms: Sequence[int], columns_per_launch: int,
                     device=None) -> torch.Tensor:
    """The block ``[3 len(atoms), 3 n_atoms]`` of a symmetric Hessian from a batched Hessian-vector callable:
    ``hvp(U)`` takes the directions ``U [K, n_atoms, 3]`` of the ``K`` replicas of one launch and returns ``H U[k]`` for
    every replica, ``[K, n_atoms, 3]``. Row ``3 i + c`` of the result is ``H e_(atoms[i], c)``."""
    plan = replica_plan(n_atoms, atoms, columns_per_launch)
    out = []
    for rows in plan:
        u = torch.zeros((len(rows), 3 * n_atoms), dtype=torch.float32, device=device)
        u[torch.arange(len(rows), device=device), torch.tensor(rows, device=device)] = 1.0
        got = hvp(u.reshape(len(rows), n_atoms, 3))
        out.append(got.reshape(len(rows), 3 * n_atoms))
    if not out:
        return torch.zeros((0, 3 * n_atoms), dtype=torch.float32, device=device)
    return torch.cat(out)


def hessian(model: rt.HipModel, system: data.System, cutoff: Optional[float] = None, atoms: Optional[Sequence[int]] = None,
            columns_per_launch: int = 8, zbl=None) -> torch.Tensor:
    """Dense block ``[3 n, 3 N]`` of the Hessian ``d2E / dR dR`` of ONE system ``(positions, atomic numbers, cell, pbc)``:
    its rows are the ``n = len(atoms)`` atoms asked for (all ``N`` by default), x, y, z each.

    Columns are batched by REPLICATION: the system is collated ``K = columns_per_launch`` times into one graph
    (:func:`metatrain_amd.data.collate`), replica ``k`` carries the unit direction of one row, and one sweep of
    ``pet_hessian_vector`` yields ``K`` rows -- the replicas do not interact, so no kernel knows about it. The workspace
    grows with the replicas: ``pet_hvp_workspace_bytes_for`` of the replicated graph, about
    ``hvp_workspace_bytes(model, graph of one system)`` per replica (the dual activations of every layer: about 87 KB per
    token row, edges + atoms, for the default model, 43 KB for ``d_pet = 64`` -- 1.7 GB and 0.85 GB for a 1 000-atom box with
    18 762 edges, ``profiles/hvp_bench.json``), which is what bounds ``K``.

    ``zbl``: a :class:`~metatrain_amd.zbl.ZBLHip`, ``True`` (default radii) or ``False`` (the bare network). With a table,
    every launch adds the ZBL product on the same replicated graph, or on one at the ZBL cutoff (``ZBLHip.graph_for``) when
    the model's list does not hold every ZBL pair. A ``zbl: true`` model with ``zbl=None`` raises.
    """
    zbl = _zbl_term(model, zbl)
    pos, z, cell, pbc = system
    n_atoms = int(pos.shape[0])
    cutoff = float(model.hypers["cutoff"]) if cutoff is None else float(cutoff)
    atoms = list(range(n_atoms)) if atoms is None else [int(a) for a in atoms]
    graphs, zbl_graphs = {}, {}

    def hvp(u):
        k = int(u.shape[0])
        if k not in graphs:  # (the last launch may hold fewer replicas)
            batch = data.collate([(pos, z, cell, pbc)] * k, cutoff)
            graphs[k] = data.graph_of(model, batch)
            if zbl is not None:  # the model's graph when it holds every ZBL pair, else one at the ZBL cutoff
                listed = cutoff + 1e-6 >= zbl.cutoff  # (``cutoff`` may be shorter than the model's)
                zbl_graphs[k] = zbl.graph_for(graphs[k] if listed else batch, pbcs=[[bool(p) for p in pbc]] * k)
        out = rt.hessian_vector_product(model, graphs[k], u.reshape(k * n_atoms, 3))
        if zbl is not None:
            out = out + zbl.hessian_vector_product(zbl_graphs[k], u.reshape(k * n_atoms, 3))
        return out.reshape(k, n_atoms, 3)

    return hessian_from_hvp(hvp, n_atoms, atoms, columns_per_launch, device=pos.device)
