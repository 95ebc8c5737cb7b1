"""Boxes that drive the per-layer exchange of ONE PET box over several ranks (``pet_graph_set_exchange``,
``metatrain_amd/pet/partition.py::energy_and_gradient_exchange``) to its slab, peer and stage-plan edges, shared by
``test_exchange_cases_cpu.py`` (the premises: each case is what it says) and ``test_gpu_exchange_edges.py`` (the device against
the fp64 oracle ``oracle/pet.py``). No GPU import at module level.

What runs around the host callback: ``exchange_forward`` / ``exchange_backward`` (pet_fwd.hip) with the staging kernels
``k_rows_gather`` and ``k_rows_scatter`` (copy, add, zero), between the edge transformer and the combination stage of every GNN
layer; a graph with an exchange never folds dXF into the combination adjoint (pet_plan.hip: ``dxf_fused`` carries ``!g.x_fn``).

Every case is fp32-rounded positions (the oracle is given those values), species drawn from ``TYPES``, the default hypers
(cutoff 4.5 A, two GNN layers) and ``synthetic_params(..., seed 0)``; every periodic extent is above two cutoffs.

  slab            198 atoms uniform in diag(36, 10, 11), periodic. World 2: both faces of a slab go to the ONE peer; 3, 4: two
                  peers; 8: slabs of exactly one cutoff; 12: 3 A slabs, every rank exchanges rows with ranks +-1 AND +-2
  triclinic       the same fractional coordinates in that cell sheared by [1,0] = 3, [2,0] = -2, [2,1] = 1.5
  surface         the slab box open along the slab axis: the end ranks have one peer. ``surface_zero_row``: the same with
                  metatomic's zero lattice row on the open axis
  cluster         60 atoms in a 16 x 8 x 8 A bounding box, no periodicity, zero cell
  clustered       40 atoms with x in [20, 25] of diag(60, 10, 10): of four ranks only rank 1 owns (or sees) anything
  gap             two groups of 30 atoms 24 A apart: both ranks work and have NOTHING to exchange (x_fn set, no rows)
  unwrapped       the slab box with every atom moved by a lattice vector of [-2, 2]^3: the plan is that of ``slab``
  dense           203 atoms in 20 x 9.2 x 9.2 A: the largest neighbour count lies in 33 .. 64 (64-slot attention tiles)
  isolated        ``cluster`` plus one atom 6 A beyond it along the slab axis: rank 2 owns an atom without a row
  isolated_alone  the same atom 9 A beyond: it is ALL rank 2 owns, whose sub-system has no edge

``REFUSALS``: boxes the exchange must refuse before anything is launched."""
import collections
import functools

import numpy as np
import torch

from _memo import memo_oracle
from oracle import nl as onl
from oracle import pet as opet

TYPES = [1, 6, 7, 8]
CUTOFF = float(opet.DEFAULT_HYPERS["cutoff"])
N_LAYERS = int(opet.DEFAULT_HYPERS["num_gnn_layers"])
SLAB_CELL = np.diag([36.0, 10.0, 11.0])
PERIODIC, OPEN = (True, True, True), (False, False, False)

Case = collections.namedtuple("Case", "name reason positions species cell pbc worlds")


def _f32(x):
    return torch.tensor(np.asarray(x, np.float64), dtype=torch.float32)


def _species(rng, n):
    return torch.tensor(np.array(TYPES)[rng.integers(0, 4, n)], dtype=torch.int32)


def _case(name, reason, pos, z, cell, pbc, worlds):
    return Case(name, reason, _f32(pos), z, _f32(cell), tuple(bool(p) for p in pbc), tuple(worlds))


def _build():
    rng = np.random.default_rng(7)
    n = 198
    frac, z = rng.uniform(0.0, 1.0, (n, 3)), _species(rng, n)
    tri = SLAB_CELL.copy()
    tri[1, 0], tri[2, 0], tri[2, 1] = 3.0, -2.0, 1.5
    zero_row = SLAB_CELL.copy()
    zero_row[0] = 0.0
    lattice = rng.integers(-2, 3, (n, 3)).astype(np.float64)
    cases = [
        _case("slab", "both faces to one peer (2), two peers (3, 4), one-cutoff slabs (8), peers two slabs away (12)",
              frac @ SLAB_CELL, z, SLAB_CELL, PERIODIC, (2, 3, 4, 8, 12)),
        _case("triclinic", "a sheared cell small enough for the oracle", frac @ tri, z, tri, PERIODIC, (3,)),
        _case("surface", "open along the slab axis: the end ranks have one peer", frac @ SLAB_CELL, z, SLAB_CELL,
              (False, True, True), (3,)),
        _case("surface_zero_row", "the same with a zero lattice row on the open axis", frac @ SLAB_CELL, z, zero_row,
              (False, True, True), (3,)),
        _case("unwrapped", "positions outside the cell: the plan of slab", (frac + lattice) @ SLAB_CELL, z, SLAB_CELL, PERIODIC,
              (3,)),
    ]
    rng = np.random.default_rng(11)
    cl = rng.uniform(0.0, 1.0, (60, 3)) * np.array([16.0, 8.0, 8.0])
    cl[0, 0], cl[1, 0] = 0.0, 16.0  # the bounding box is 16 A along the slab axis, whatever the draw
    zc = _species(rng, 60)
    z1 = _species(rng, 1)
    cases.append(_case("cluster", "an open system: slabs of the bounding box, zero cell", cl, zc, np.zeros((3, 3)), OPEN, (3,)))
    for name, reason, dx in (("isolated", "a rank owns an atom without a row", 6.0),
                             ("isolated_alone", "a rank owns only an atom without a row: no edge in its sub-system", 9.0)):
        far = np.array([[16.0 + dx, 4.0, 4.0]])
        cases.append(_case(name, reason, np.concatenate([cl, far]), torch.cat([zc, z1]), np.zeros((3, 3)), OPEN, (3,)))
    rng = np.random.default_rng(13)
    long_cell = np.diag([60.0, 10.0, 10.0])
    pos = rng.uniform(0.0, 1.0, (40, 3)) * np.array([5.0, 10.0, 10.0]) + np.array([20.0, 0.0, 0.0])
    cases.append(_case("clustered", "empty-slab ranks beside a working one", pos, _species(rng, 40), long_cell, PERIODIC, (4,)))
    rng = np.random.default_rng(17)
    pos = rng.uniform(0.0, 1.0, (60, 3)) * np.array([6.0, 10.0, 10.0])
    pos[:30, 0] += 5.0
    pos[30:, 0] += 35.0
    cases.append(_case("gap", "two working ranks with no row to exchange", pos, _species(rng, 60), long_cell, PERIODIC, (2,)))
    rng = np.random.default_rng(DENSE_SEED)
    dense_cell = np.diag([20.0, 9.2, 9.2])
    nd = int(round(0.12 * 20.0 * 9.2 * 9.2))
    cases.append(_case("dense", "33 .. 64 neighbours: 64-slot attention tiles under the exchange",
                       rng.uniform(0.0, 1.0, (nd, 3)) @ dense_cell, _species(rng, nd), dense_cell, PERIODIC, (2,)))
    return collections.OrderedDict((c.name, c) for c in cases)


DENSE_SEED = 19
CASES = _build()
CASE_WORLDS = [(c.name, w) for c in CASES.values() for w in c.worlds]
PER_RANK = [("slab", 3), ("surface", 3)]       # rank r's own gradient against d(sum of its owned energies)/dR
STAGE_FORM_CASES = [("slab", 3), ("dense", 2)]
STAGE_FORMS = ["default", "trr=0", "attn_fused=0", "emlp_s=2,attn_fused=7", "node_planes=0", "trr_compress=0", "center_fused=0"]
FORCED = "emlp_s=2,attn_fused=7"
HALO = [("slab", 2), ("slab", 3), ("surface", 3), ("cluster", 3), ("clustered", 4)]


def _refusals():
    rng = np.random.default_rng(23)
    thin = np.diag([36.0, 8.5, 11.0])  # 8.5 A < two cutoffs: some pair is connected by two images
    n = 198
    two = _case("two_images", "a periodic extent of 8.5 A", rng.uniform(0.0, 1.0, (n, 3)) @ thin, _species(rng, n), thin,
                PERIODIC, (2,))
    cell = np.diag([18.0, 9.2, 9.2])
    n = int(round(0.4 * 18.0 * 9.2 * 9.2))
    crowd = _case("crowded", "more than 127 neighbours", rng.uniform(0.0, 1.0, (n, 3)) @ cell, _species(rng, n), cell,
                  PERIODIC, (2,))
    return {"two_images": two, "crowded": crowd}


REFUSALS = _refusals()


def hypers(**delta):
    return dict(opet.DEFAULT_HYPERS, **delta)


def params(**delta):
    return opet.synthetic_params(hypers(**delta), TYPES, {"energy": 1}, 0, torch.float32)


@functools.lru_cache(maxsize=None)
def neighbor_list(name):
    """``(i, j, S)`` of the whole box from the oracle's neighbour list, as int64 tensors"""
    c = CASES.get(name) or REFUSALS[name]
    i, j, s, _ = onl.neighbor_list(c.positions.double().numpy(), c.cell.double().numpy(), list(c.pbc), CUTOFF)
    return (torch.tensor(i.astype(np.int64)), torch.tensor(j.astype(np.int64)), torch.tensor(s.astype(np.int64)).reshape(-1, 3))


def neighbor_counts(name):
    c = CASES.get(name) or REFUSALS[name]
    return torch.bincount(neighbor_list(name)[0], minlength=len(c.species))


def owner(name, world):
    """the rank that owns every atom (the library's own host function: ``slab_owner``)"""
    from metatrain_amd.partition import slab_owner

    c = CASES[name]
    return slab_owner(c.positions, c.cell, list(c.pbc), world)


# ---- the oracle --------------------------------------------------------------------------------------------------------------
def _atomic(name, dtype, pos):
    c = CASES[name]
    i, j, s = neighbor_list(name)
    p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in params().items()}
    n = len(c.species)
    return opet.pet_atomic_energies(p, hypers(), pos, c.cell.to(dtype)[None], i, j, s, c.species.long(),
                                    torch.zeros(n, dtype=torch.long)).reshape(-1)


@memo_oracle
def _oracle(name, dtype):
    pos = CASES[name].positions.to(dtype).clone().requires_grad_(True)
    atomic = _atomic(name, dtype, pos)
    (grad,) = torch.autograd.grad(atomic.sum(), pos)
    return atomic.detach().double().numpy(), grad.double().numpy()


def oracle(name, dtype=torch.float64):
    """``(per-atom energies [N], dE/dR [N, 3])`` of the WHOLE box from the oracle in ``dtype``, as fp64 arrays"""
    return _oracle(name, dtype)


@memo_oracle
def owned_energy_gradients(name, world):
    """``[world, N, 3]``: d(sum of the energies rank r owns)/dR for every atom of the box, from one fp64 graph. This is what
    rank r of the HALO scheme returns (``partition.energy_and_gradient``: everything its energies read is computed locally)."""
    pos = CASES[name].positions.double().clone().requires_grad_(True)
    atomic = _atomic(name, torch.float64, pos)
    own = owner(name, world)
    out = np.zeros((world,) + tuple(pos.shape))
    for r in range(world):
        (g,) = torch.autograd.grad((atomic * (own == r).double()).sum(), pos, retain_graph=True)
        out[r] = g.numpy()
    return out


@memo_oracle
def rank_gradients(name, world):
    """``[world, N, 3]``: what rank r of the per-layer EXCHANGE returns, from one fp64 graph of the whole box. With the exchange
    a rank runs the edge transformers of the centres it owns for EVERYBODY: the adjoints its peers form on their ghost rows come
    home and flow on through its rows, and the adjoints on its own ghost rows leave. Its gradient is therefore not the gradient
    of its owned energies (that would need the peers' transformers) but the part of dE/dR -- E the energy of the whole box --
    that reaches the positions through the geometry (edge vector, distance, cutoff factor) of the rows whose centre it owns.
    The oracle is evaluated with one copy of the positions per rank, row ``i -> j`` reading both atoms from the copy of the
    owner of ``i``; the gradient with respect to copy r is rank r's result, halo atoms included, and the copies' gradients
    add up to dE/dR."""
    from unittest import mock

    c = CASES[name]
    own = owner(name, world)
    copies = c.positions.double()[None].repeat(world, 1, 1).requires_grad_(True)

    calls = []

    def geometry(positions, cells, centers, neighbors, cell_shifts, system_indices):  # oracle.pet.edge_geometry per copy
        calls.append(len(centers))
        r = own[centers]
        contrib = torch.einsum("ab,abc->ac", cell_shifts.to(copies.dtype), cells[system_indices[centers]])
        v = copies[r, neighbors] - copies[r, centers] + contrib
        return v, torch.linalg.norm(v, dim=-1) + 1e-15

    with mock.patch.object(opet, "edge_geometry", geometry):
        atomic = _atomic(name, torch.float64, c.positions.double())
    # the oracle took ALL its geometry from the copies, once: otherwise this would be the whole-box gradient in disguise
    # (the positions handed in carry no gradient: only the copies can have given ``atomic`` one)
    assert calls == [len(neighbor_list(name)[0])] and atomic.requires_grad, calls
    (grad,) = torch.autograd.grad(atomic.sum(), copies)
    return grad.numpy()


def relmax(got, ref):
    """max |got - ref| over max |ref| (0 where both vanish)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    diff = float(np.abs(got - ref).max()) if ref.size else 0.0
    return diff / scale if scale > 0 else diff


def ref32(name):
    """the fp32 oracle's own distance from the fp64 oracle: ``(relmax of the energies, of dE/dR)``"""
    a64, g64 = oracle(name)
    a32, g32 = oracle(name, torch.float32)
    return relmax(a32, a64), relmax(g32, g64)
