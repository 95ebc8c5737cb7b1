"""fp64 torch restatement of the long-range operator's DEFINITION (``include/pet_hip.h``, block ``pet_ewald_*``; DESIGN.md
section 18), written independently of the product's k-set code, and the end-to-end long-range PET composed from it.
Everything is differentiable by autograd and runs in the dtype of its inputs (fp32 for the yardstick ``e32``).

    sigma = smearing, R = cutoff, lambda = kspace_resolution, Omega = |det cell|, a = sqrt(2) sigma, P = 1/2
    f(d) = (1 + cos(pi d / R)) / 2 for d < R, else 0;  G(k) = 4 pi exp(-sigma^2 k^2 / 2) / k^2
    periodic:  V_i = P [ (1/Omega) sum_{k != 0, |k| <= 2 pi / lambda} G(k) Re(e^{-i k.r_i} S(k)) - q_i sqrt(2/pi)/sigma
                         - (2 pi sigma^2 / Omega) sum_j q_j - sum_{edges (i -> j, S)} q_j erf(d/a)/d f(d) ]
    open:      V_i = P sum_{j != i} q_j (1 - f(d_ij)) / d_ij
"""
import itertools
import math
import os

import numpy as np
import torch

from oracle import nl as onl
from oracle import pet as opet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PREFACTOR = 0.5
TYPES = [1, 6, 7, 8]


def kvector_indices(cell: torch.Tensor, kspace_resolution: float) -> torch.Tensor:
    """Integer triples ``n [K, 3]`` with ``0 < |2 pi n cell^{-T}| <= 2 pi / lambda``, from a box of indices that surely
    contains the sphere (the bound |n_a| <= kmax |cell_a| / 2 pi, plus one)."""
    c = cell.detach().double()
    kmax = 2.0 * math.pi / kspace_resolution
    rec = 2.0 * math.pi * torch.linalg.inv(c).T
    bound = [int(math.ceil(kmax * float(torch.linalg.norm(c[a])) / (2.0 * math.pi))) + 1 for a in range(3)]
    n = torch.cartesian_prod(*[torch.arange(-b, b + 1) for b in bound]).double()
    k2 = ((n @ rec) ** 2).sum(1)
    return n[(k2 > 0) & (k2 <= kmax * kmax)]


def kvectors(cell: torch.Tensor, kspace_resolution: float) -> torch.Tensor:
    c = cell.double()
    return kvector_indices(c, kspace_resolution) @ (2.0 * math.pi * torch.linalg.inv(c).T)


def cutoff_f(d, R):
    return torch.where(d < R, 0.5 * (1.0 + torch.cos(math.pi * d / R)), torch.zeros_like(d))


def kspace_self_background(pos, cell, q, smearing, kspace_resolution, kmax=None):
    """The first three terms of the periodic definition, WITHOUT the prefactor."""
    dt = pos.dtype
    lam = kspace_resolution if kmax is None else 2.0 * math.pi / kmax
    n = kvector_indices(cell, lam).to(dt)
    k = n @ (2.0 * math.pi * torch.linalg.inv(cell).T)
    k2 = (k * k).sum(1)
    g = 4.0 * math.pi * torch.exp(-0.5 * smearing ** 2 * k2) / k2
    ph = k @ pos.T
    c, s = torch.cos(ph), torch.sin(ph)
    vol = torch.det(cell).abs()
    v = (c.T @ (g[:, None] * (c @ q)) + s.T @ (g[:, None] * (s @ q))) / vol
    return v - q * (math.sqrt(2.0 / math.pi) / smearing) - (2.0 * math.pi * smearing ** 2 / vol) * q.sum(0, keepdim=True)


def potential_periodic(pos, cell, q, edges, smearing, kspace_resolution, cutoff):
    """``edges = (i, j, S)`` of this system (local indices): the model's strict full neighbour list."""
    v = kspace_self_background(pos, cell, q, smearing, kspace_resolution)
    i, j, S = edges
    if len(i):
        D = pos[j] - pos[i] + S.to(pos.dtype) @ cell
        d = torch.linalg.norm(D, dim=1)
        w = torch.erf(d / (math.sqrt(2.0) * smearing)) / d * cutoff_f(d, cutoff)
        v = v - torch.zeros_like(q).index_add(0, i, w[:, None] * q[j])
    return PREFACTOR * v


def potential_open(pos, q, cutoff):
    n = pos.shape[0]
    D = pos[None, :, :] - pos[:, None, :]
    eye = torch.eye(n, dtype=torch.bool)
    d = torch.sqrt((D * D).sum(-1) + eye.to(pos.dtype))  # 1 on the diagonal, masked below
    kern = torch.where(eye, torch.zeros_like(d), (1.0 - cutoff_f(d, cutoff)) / d)
    return PREFACTOR * (kern @ q)


def potential_batch(pos, cells, pbcs, first_atom, q, centers, neighbors, shifts, smearing, kspace_resolution, cutoff):
    """The operator on a collated batch: global edge lists grouped by nothing in particular."""
    out = []
    for s in range(len(first_atom) - 1):
        a0, a1 = first_atom[s], first_atom[s + 1]
        if all(pbcs[s]):
            m = (centers >= a0) & (centers < a1)
            e = (centers[m] - a0, neighbors[m] - a0, shifts[m])
            out.append(potential_periodic(pos[a0:a1], cells[s], q[a0:a1], e, smearing, kspace_resolution, cutoff))
        else:
            assert not any(pbcs[s])
            out.append(potential_open(pos[a0:a1], q[a0:a1], cutoff))
    return torch.cat(out)


def madelung_nacl(smearing: float) -> float:
    """The NaCl Madelung constant (nearest distance 1) from the no-exclusion mode: k-space + self + background of the
    definition plus the real-space ``erfc`` sum over images."""
    pos, cell, q = nacl_system()
    v = kspace_self_background(pos, cell, q, smearing, None, kmax=9.0 / smearing)
    return float((v + real_space_erfc(pos, cell, q, smearing))[0, 0])


def nacl_system():
    """Rock salt with nearest distance 1: ``(positions [8, 3], cell [3, 3], charges [8, 1])``, fp64, the atom at the origin
    first and charged +1."""
    cell = torch.eye(3, dtype=torch.float64) * 2.0
    pos = torch.tensor(list(itertools.product(range(2), repeat=3)), dtype=torch.float64)
    q = torch.tensor([[(-1.0) ** int(p.sum())] for p in pos], dtype=torch.float64)
    return pos, cell, q


def real_space_erfc(pos, cell, q, smearing):
    """``sum over images j != i of q_j erfc(d / a) / d`` out to ``8 sigma``, without the prefactor (fp64)."""
    rc = 8.0 * smearing
    m = int(math.ceil(rc / float(cell.diagonal().min())))
    S = torch.cartesian_prod(*[torch.arange(-m, m + 1)] * 3).double()
    D = pos[None, :, None, :] - pos[:, None, None, :] + (S @ cell)[None, None]
    d = D.norm(dim=-1)
    i, j, s = torch.nonzero((d > 1e-9) & (d < rc), as_tuple=True)
    return torch.zeros_like(q).index_add(0, i, q[j] * (torch.erfc(d[i, j, s] / (math.sqrt(2.0) * smearing)) / d[i, j, s])[:, None])


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _nl(pos, cell, pbc, cutoff):
    i, j, s, _ = onl.neighbor_list(pos.numpy(), cell.numpy(), list(pbc), cutoff)
    return torch.tensor(i).long(), torch.tensor(j).long(), torch.tensor(s).long().reshape(-1, 3)


def collate(systems, cutoff):
    """``systems``: list of (positions [n,3] fp64, cell [3,3] fp64, pbc). Returns the batch dictionary."""
    pos, cells, pbcs, first, ctr, nbr, sh, sysidx = [], [], [], [0], [], [], [], []
    for s, (p, c, pbc) in enumerate(systems):
        i, j, S = _nl(p, c, pbc, cutoff)
        ctr.append(i + first[-1])
        nbr.append(j + first[-1])
        sh.append(S)
        pos.append(p)
        cells.append(c)
        pbcs.append([bool(x) for x in pbc])
        sysidx.append(torch.full((len(p),), s, dtype=torch.long))
        first.append(first[-1] + len(p))
    return {"positions": torch.cat(pos), "cells": torch.stack(cells), "pbcs": pbcs, "first_atom": first,
            "centers": torch.cat(ctr), "neighbors": torch.cat(nbr), "cell_shifts": torch.cat(sh),
            "system_indices": torch.cat(sysidx)}


def mixed_batch(cutoff=4.5):
    """A 1-atom periodic cell, a triclinic 43-atom cell (L ~ 9.5, off-diagonals ~ 0.3), a 130-atom cubic cell of L = 20
    (several thousand k-vectors) and a 17-atom open cluster: sizes that align with no tile of 32."""
    g = torch.Generator().manual_seed(5)
    tri = torch.eye(3, dtype=torch.float64) * 9.5 + 0.3 * torch.randn(3, 3, generator=g, dtype=torch.float64)
    cub = torch.eye(3, dtype=torch.float64) * 20.0
    one = torch.eye(3, dtype=torch.float64) * 6.0
    systems = [
        (torch.rand(1, 3, generator=g, dtype=torch.float64) @ one, one, [True] * 3),
        (torch.rand(43, 3, generator=g, dtype=torch.float64) @ tri, tri, [True] * 3),
        (torch.rand(130, 3, generator=g, dtype=torch.float64) @ cub, cub, [True] * 3),
        (torch.rand(17, 3, generator=g, dtype=torch.float64) * 7.0, torch.zeros(3, 3, dtype=torch.float64), [False] * 3),
    ]
    return systems


def small_cell():
    """3 atoms in a cubic cell of L = 4.0 < R = 4.5: every atom has edges to its own images."""
    g = torch.Generator().manual_seed(9)
    cell = torch.eye(3, dtype=torch.float64) * 4.0
    return [(torch.rand(3, 3, generator=g, dtype=torch.float64) @ cell, cell, [True] * 3)]


def operator_reference(batch, q, gv, smearing, kspace_resolution, cutoff, dtype):
    """(V, dL/dq, dL/dR, dL/dcell) for ``L = sum(gv * V)``, evaluated in ``dtype``, returned in fp64."""
    pos = batch["positions"].to(dtype).clone().requires_grad_(True)
    cells = batch["cells"].to(dtype).clone().requires_grad_(True)
    qq = q.to(dtype).clone().requires_grad_(True)
    v = potential_batch(pos, cells, batch["pbcs"], batch["first_atom"], qq, batch["centers"], batch["neighbors"],
                        batch["cell_shifts"], smearing, kspace_resolution, cutoff)
    gq, gp, gc = torch.autograd.grad((gv.to(dtype) * v).sum(), [qq, pos, cells], allow_unused=True)
    gc = torch.zeros_like(cells) if gc is None else gc
    return tuple(t.detach().double() for t in (v, gq, gp, gc))


# ---- the whole long-range model ---------------------------------------------------------------------------------------------
def featurizer_params(d: int, seed: int = 0):
    """Seeded featuriser weights under the reference's keys (``long_range_featurizer.*``), fp32."""
    g = torch.Generator().manual_seed(1000 + seed)
    out = {}
    for name in ("charges_map", "out_projection.0", "out_projection.2"):
        out[f"long_range_featurizer.{name}.weight"] = torch.randn(d, d, generator=g) / math.sqrt(d)
        out[f"long_range_featurizer.{name}.bias"] = 0.1 * torch.randn(d, generator=g)
    return out


def model_reference(params, lr_params, hypers, batch, dtype):
    """(per-atom energies, per-system energies, dE/dR, dE/dcell) of the long-range PET in ``dtype``, returned in fp64:
    ``oracle.pet.pet_atomic_energies(return_features="all")``, the Ewald oracle above, and the read-out lines of
    ``oracle/pet.py:412-418`` restated."""
    p = {k: (v if k == "species_to_species_index" else v.to(dtype)) for k, v in params.items()}
    lp = {k: v.to(dtype) for k, v in lr_params.items()}
    pos = batch["positions"].to(dtype).clone().requires_grad_(True)
    cells = batch["cells"].to(dtype).clone().requires_grad_(True)
    ctr_in, nbr_in, sh_in, sysidx = batch["centers"], batch["neighbors"], batch["cell_shifts"], batch["system_indices"]
    _, nfs, efs, graph = opet.pet_atomic_energies(p, hypers, pos, cells, ctr_in, nbr_in, sh_in, batch["species"], sysidx,
                                                  "energy", return_features="all")
    lr = hypers["long_range"]
    x = sum(nfs) / math.sqrt(len(nfs))
    lin = torch.nn.functional.linear
    pre = "long_range_featurizer."
    q = lin(x, lp[pre + "charges_map.weight"], lp[pre + "charges_map.bias"])
    v = potential_batch(pos, cells, batch["pbcs"], batch["first_atom"], q, ctr_in, nbr_in, sh_in, float(lr["smearing"]),
                        float(lr["kspace_resolution"]), float(hypers["cutoff"]))
    hid = torch.nn.functional.silu(lin(v, lp[pre + "out_projection.0.weight"], lp[pre + "out_projection.0.bias"]))
    feat = lin(hid, lp[pre + "out_projection.2.weight"], lp[pre + "out_projection.2.bias"])
    hs = [(h + feat) * math.sqrt(0.5) for h in nfs]
    # cutoff factors of the kept edges in the graph's order (strict list: every edge is kept)
    _, d_all = opet.edge_geometry(pos, cells, ctr_in, nbr_in, sh_in, sysidx)
    d0 = d_all[torch.as_tensor(graph.order)]
    cut = opet.cutoff_bump if hypers["cutoff_function"].lower() == "bump" else opet.cutoff_cosine
    fc = cut(d0, float(hypers["cutoff"]), float(hypers["cutoff_width"]))
    ctr = torch.as_tensor(graph.centers)
    silu = torch.nn.functional.silu
    atomic = None
    for l, (h, m) in enumerate(zip(hs, efs)):
        nl = silu(opet._linear(silu(opet._linear(h, p, f"node_heads.energy.{l}.0")), p, f"node_heads.energy.{l}.2"))
        el = silu(opet._linear(silu(opet._linear(m, p, f"edge_heads.energy.{l}.0")), p, f"edge_heads.energy.{l}.2"))
        node_pred = opet._linear(nl, p, f"node_last_layers.energy.{l}.energy")
        edge_pred = opet._linear(el, p, f"edge_last_layers.energy.{l}.energy") * fc[:, None]
        contrib = node_pred.index_add(0, ctr, edge_pred)
        atomic = contrib if atomic is None else atomic + contrib
    atomic = atomic[:, 0]
    energies = torch.zeros(cells.shape[0], dtype=dtype).index_add(0, sysidx, atomic)
    gp, gc = torch.autograd.grad(atomic.sum(), [pos, cells], allow_unused=True)
    gc = torch.zeros_like(cells) if gc is None else gc
    mags = (float(sum(nfs).detach().abs().max()), float(feat.detach().abs().max()))
    return tuple(t.detach().double() for t in (atomic, energies, gp, gc)) + (mags,)


def periodic_box_batch(n_atoms=64, seed=3, cutoff=4.5):
    pos, z, cell = opet.random_box(n_atoms, seed=seed, dtype=torch.float64)
    b = collate([(pos.double(), cell.double(), [True] * 3)], cutoff)
    b["species"] = z
    return b


def qm9_batch(n_frames=3, cutoff=4.5):
    g = dict(np.load(os.path.join(GOLDEN, "qm9_first5.npz")))
    systems = [(torch.tensor(g[f"pos{k}"]).double(), torch.zeros(3, 3, dtype=torch.float64), [False] * 3)
               for k in range(n_frames)]
    b = collate(systems, cutoff)
    b["species"] = torch.cat([torch.tensor(g[f"z{k}"]) for k in range(n_frames)])
    return b


def relmax(got, ref):
    got, ref = got.detach().cpu().double(), ref.double()
    return float((got - ref).abs().max() / ref.abs().max())
