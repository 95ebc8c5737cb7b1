"""Second derivatives of the SOAP-BPNN energy w.r.t. the positions: dense Hessian blocks from
:meth:`SoapBpnnHip.hessian_vector_product` (``soap_hessian_vector``, ``csrc/soap_hvp.hip``).

The reference model is differentiable to second order through torch, so a user gets ``H u`` from ``torch.autograd``; here
it is one call of the C ABI, and the dense block is batched by replication exactly as for PET
(:mod:`metatrain_amd.pet.hessian`, whose ``replica_plan`` / ``hessian_from_hvp`` this module uses).

Out of scope: per-atom ``weights``, the slab partition, a product on the MFMA or packed kernels, third order.
"""
from typing import Optional, Sequence

import torch

from .. import data
from ..pet.hessian import _zbl_term, hessian_from_hvp, replica_plan  # noqa: F401  (replica_plan: re-exported)
from .model import SoapBpnnHip


def hessian(model: SoapBpnnHip, system: data.System, atoms: Optional[Sequence[int]] = None, columns_per_launch: int = 8,
            zbl=None) -> torch.Tensor:
    """Dense block ``[3 n, 3 N]`` of the Hessian ``d2E / dR dR`` of ONE system ``(positions, atomic numbers, cell, pbc)``:
    its rows are the ``n = len(atoms)`` atoms asked for (all ``N`` by default), x, y, z each.

    Columns are batched by REPLICATION: the system is collated ``K = columns_per_launch`` times into one graph at the
    model's cutoff, replica ``k`` carries the unit direction of one row, and one ``soap_hessian_vector`` sweep yields ``K``
    rows (the last launch may hold fewer). The forward of the replicated graph runs once per replica count.

    ``zbl``: a :class:`~metatrain_amd.zbl.ZBLHip`, ``True`` (default radii) or ``False`` (the bare network); with a table
    every launch adds the ZBL product on the same replicated graph, or on one at the ZBL cutoff when the model's list does
    not hold every ZBL pair. A ``zbl`` model (``hypers["zbl"]`` or a ``zbl=`` given at construction) with ``zbl=None``
    raises: the network's Hessian alone is not the model's.
    """
    if zbl is None and getattr(model, "zbl", None) is not None and not model.hypers.get("zbl", False):
        from .._lib import PetHipError

        raise PetHipError("this model has a ZBL term and the network's Hessian alone is not the model's: pass zbl=model.zbl "
                          "(or another ZBLHip), zbl=True (default radii) or zbl=False for the bare network")
    zbl = _zbl_term(model, zbl)
    pos, z, cell, pbc = system
    n_atoms = int(pos.shape[0])
    atoms = list(range(n_atoms)) if atoms is None else [int(a) for a in atoms]
    graphs, zbl_graphs = {}, {}

    def hvp(u):
        k = int(u.shape[0])
        if k not in graphs:
            batch = data.collate([(pos, z, cell, pbc)] * k, model.cutoff)
            graphs[k] = model.graph(batch["positions"], batch["cells"], batch["centers"], batch["neighbors"],
                                    batch["cell_shifts"], batch["species"], batch["system_indices"])
            if zbl is not None:
                listed = model.cutoff + 1e-6 >= zbl.cutoff
                zbl_graphs[k] = zbl.graph_for(graphs[k] if listed else batch, pbcs=[[bool(p) for p in pbc]] * k)
        out = model.hessian_vector_product(graphs[k], u.reshape(k * n_atoms, 3))
        if zbl is not None:
            out = out + zbl.hessian_vector_product(zbl_graphs[k], u.reshape(k * n_atoms, 3))
        return out.reshape(k, n_atoms, 3)

    return hessian_from_hvp(hvp, n_atoms, atoms, columns_per_launch, device=pos.device)
