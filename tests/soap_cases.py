"""Inputs that drive the SOAP-BPNN pass (``metatrain_amd/csrc/soap.hip`` and its stage files ``soap_expand.hip``, ``soap_ps.hip``,
``soap_tail.hip``, ``soap_train.hip``; the plan is ``soap_plan.h``) into the kernels and branches its
host code selects by the model's dimensions and by the batch (DESIGN.md "SOAP-BPNN dispatch and its edge cases"), which the one
input shape of ``test_gpu_soap.py`` -- a cubic four-type box at 0.05 atoms / A^3 -- never reaches. Shared by
``test_soap_cases_cpu.py`` (the premises: each case is what it says) and ``test_gpu_soap_edges.py`` (the device against the fp64
oracle). No GPU import at module level.

A case is ``Case(name, reason, hypers, types, systems)`` with ``systems`` a list of ``(positions fp64 [n, 3], species [n],
cell fp64 [3, 3], pbc)``. All builders are seeded. Atoms sit on jittered lattice sites (a close pair would dominate the
max-normalised error of a case): every case keeps a minimum interatomic distance, images included, of ``MIN_DISTANCE``.
Positions and cells are fp32-representable, so the oracle and the device start from the same numbers."""
import collections
import functools
import itertools
import math

import numpy as np
import torch

from _memo import memo_oracle
from oracle import nl as onl
from oracle import soap as osoap

Case = collections.namedtuple("Case", "name reason hypers types systems")

CUTOFF = 5.0
MIN_DISTANCE = 0.8
N_PER_L = [8, 7, 7, 6, 6, 5, 5]
TYPES4 = [1, 6, 7, 8]
TYPES11 = [1, 6, 7, 8, 9, 14, 15, 16, 17, 35, 53]
PERIODIC, OPEN = (True, True, True), (False, False, False)
LEGACY = dict(osoap.DEFAULT_HYPERS, legacy=True)
ALCHEMICAL = dict(osoap.DEFAULT_HYPERS, legacy=False)


def _f32(t):
    return torch.as_tensor(t, dtype=torch.float64).float().double()


def _cubic(length):
    return _f32(torch.eye(3, dtype=torch.float64) * float(length))


NO_CELL = torch.zeros(3, 3, dtype=torch.float64)


# ---- builders --------------------------------------------------------------------------------------------------------------
def lattice_sites(n, cell, seed, jitter=0.15, grid=None):
    """``n`` of the ``m^3`` sites of a regular grid in ``cell`` (``m`` the smallest that holds them, or ``grid``), drawn under
    ``seed``, each moved by up to ``jitter`` grid spacings along every lattice direction."""
    m = grid or max(1, math.ceil(n ** (1.0 / 3.0) - 1e-9))
    g = torch.Generator().manual_seed(seed)
    sites = torch.tensor(list(itertools.product(range(m), repeat=3)), dtype=torch.float64)
    pick = torch.randperm(len(sites), generator=g)[:n].sort().values
    frac = (sites[pick] + 0.5 + jitter * (2.0 * torch.rand(n, 3, generator=g, dtype=torch.float64) - 1.0)) / m
    return _f32(frac @ cell)


def species_by_counts(counts, types, seed):
    """``counts[t]`` atoms of ``types[t]``, in a seeded order."""
    z = torch.cat([torch.full((c,), t, dtype=torch.long) for c, t in zip(counts, types)])
    return z[torch.randperm(len(z), generator=torch.Generator().manual_seed(seed))]


def species_all_present(n, types, seed):
    """Every type at least once, the rest uniform."""
    g = torch.Generator().manual_seed(seed)
    rest = torch.randint(0, len(types), (n - len(types),), generator=g)
    idx = torch.cat([torch.arange(len(types)), rest])[torch.randperm(n, generator=g)]
    return torch.tensor(types, dtype=torch.long)[idx]


def box(counts, types, rho, seed, jitter=0.15):
    """One cubic periodic box with ``counts[t]`` atoms of ``types[t]`` at density ``rho``."""
    n = int(sum(counts))
    cell = _cubic((n / rho) ** (1.0 / 3.0))
    return lattice_sites(n, cell, seed, jitter), species_by_counts(counts, types, seed + 1), cell, PERIODIC


def type_count_box(n_types, seed):
    types = TYPES11[:n_types]
    n = 40 + 3 * n_types
    cell = _cubic((n / 0.05) ** (1.0 / 3.0))
    return lattice_sites(n, cell, seed), species_all_present(n, types, seed + 1), cell, PERIODIC


def small_box(n, seed):
    """``n`` four-type atoms in a 6 A periodic cube (``n`` <= 8: a 2 x 2 x 2 grid, 3 A apart)."""
    cell = _cubic(6.0)
    z = torch.tensor(TYPES4, dtype=torch.long)[torch.arange(n) % 4]
    return lattice_sites(n, cell, seed, grid=2), z, cell, PERIODIC


def dense_lattice_system(seed=31):
    """4 x 4 x 4 sites 1.2 A apart in their own 4.8 A periodic cell: about 300 neighbours per centre, six self-images each."""
    cell = _cubic(4.8)
    z = species_all_present(64, TYPES4, seed + 1)
    return lattice_sites(64, cell, seed, jitter=0.15), z, cell, PERIODIC


CLUSTER_SIZES = (19, 22, 20, 21, 19, 20, 22, 21)
_CLUSTER_SITES = [s for s in itertools.product((-1.5, -0.5, 0.5, 1.5), repeat=3) if sum(c * c for c in s) < 3.0]  # 32 sites


def cluster(k, seed):
    """``k`` atoms on sites of a 1.3 A grid within 2.16 A of a point, jittered by up to 0.12 A per axis: every pair is closer
    than 4.8 A, so each atom has ``k - 1`` neighbours at the 5 A cutoff. Open, no cell."""
    g = torch.Generator().manual_seed(seed)
    sites = torch.tensor(_CLUSTER_SITES, dtype=torch.float64)
    pick = torch.randperm(len(sites), generator=g)[:k].sort().values
    pos = 1.3 * sites[pick] + 0.12 * (2.0 * torch.rand(k, 3, generator=g, dtype=torch.float64) - 1.0)
    z = species_all_present(k, TYPES4, seed + 1)
    return _f32(pos + 10.0), z, NO_CELL.clone(), OPEN


def clusters(holes=False):
    out = []
    for n, k in enumerate(CLUSTER_SIZES):
        out.append(cluster(k, 400 + 10 * n))
        if holes:  # one isolated atom (no pair) behind each cluster in atom order
            out.append((_f32([[1.0, 2.0, 3.0]]), torch.tensor([TYPES4[n % 4]]), NO_CELL.clone(), OPEN))
    return out


def empty_system():
    return torch.zeros(0, 3, dtype=torch.float64), torch.zeros(0, dtype=torch.long), _cubic(9.0), PERIODIC


def isolated_atom():
    return _f32([[0.5, 0.25, 0.75]]), torch.tensor([7]), NO_CELL.clone(), OPEN


def mixed():
    dilute = box((15, 15, 15, 15), TYPES4, 0.006, 51, jitter=0.3)
    return [dense_lattice_system(), empty_system(), dilute, isolated_atom()]


TRICLINIC = [[7.0, 0.0, 0.0], [2.5, 6.5, 0.0], [1.5, -2.0, 6.0]]
SHEARS = ([[8.0, 0.0, 0.0], [3.0, 7.5, 0.0], [0.0, 0.0, 9.0]],
          [[7.5, 0.0, 0.0], [0.0, 8.5, 0.0], [2.5, 3.0, 7.0]],
          [[9.0, 1.0, -1.5], [-2.0, 8.0, 0.5], [1.0, -3.0, 7.5]])


def triclinic_box(n, cell, seed):
    cell = _f32(cell)
    return lattice_sites(n, cell, seed), species_all_present(n, TYPES4, seed + 1), cell, PERIODIC


def lone_atom():
    return [(_f32([[0.7, 1.1, 1.9]]), torch.tensor([6]), _cubic(3.0), PERIODIC)]


def two_atoms_slab():
    """Two atoms in a triclinic cell periodic along its first two rows only."""
    cell = _f32([[3.5, 0.0, 0.0], [1.0, 3.0, 0.0], [0.5, 0.25, 8.0]])
    return [(_f32([[0.4, 0.3, 1.0], [2.1, 1.7, 2.6]]), torch.tensor([1, 8]), cell, (True, True, False))]


def left_handed():
    cell = _f32(TRICLINIC)[[1, 0, 2]].clone()
    return [triclinic_box(30, cell, 61)]


def sheared_batch():
    return [triclinic_box(n, cell, 70 + n) for n, cell in zip((21, 34, 27), SHEARS)]


CHUNK_COUNTS = (1, 343, 343, 343)


def _make(name, reason, systems, hypers=LEGACY, types=TYPES4):
    return Case(name, reason, hypers, list(types), systems)


TYPE_COUNTS_LEGACY = (1, 2, 3, 5, 8, 9, 10)
TYPE_COUNTS_ALCHEMICAL = (1, 9)
BUCKET_COUNTS = {"bucket_64_65_63_1": (64, 65, 63, 1), "bucket_70_0_1_0": (70, 0, 1, 0), "bucket_0_0_0_130": (0, 0, 0, 130),
                 "bucket_32_33_31_0": (32, 33, 31, 0), "bucket_1_1_1_0": (1, 1, 1, 0)}
SMALL_N = (1, 2, 3, 5, 6, 7)

_TYPE_REASON = {
    1: "C = 1: k_soap_expand / k_soap_expand_bwd, k_soap_ps_m<false> (nc 8), NT = 1 with half the stacked tile padding",
    2: "C = 2: k_soap_expand / k_soap_expand_bwd, k_soap_ps_m<false> (nc 16), NT = 1",
    3: "C = 3: k_soap_expand / k_soap_expand_bwd, k_soap_ps_m<false> (nc 24), NT = 2 with an odd network count",
    5: "C = 5: k_soap_expand / k_soap_expand_bwd, k_soap_ps_w (ncmax 40), NT = 3 with an odd network count",
    8: "C = 8: k_soap_ps_w (ncmax 64), (NCOEF + S) * 4 > 64 KB -> k_soap_ps_bwd, eight networks: the last sorted bucket",
    9: "C = 9: NT = 0 -> per-atom k_soap_tail (126 096 B of LDS) / k_soap_tail_bwd, nine networks in the training bucket table",
    10: "C = 10: NCOEF 2 800 of 3 072, k_soap_tail with 147 680 B of LDS, ten networks in the training bucket table",
}


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("legacy_types_"):
        c = int(name.rsplit("_", 1)[1])
        return _make(name, _TYPE_REASON[c], [type_count_box(c, 100 + c)], LEGACY, TYPES11[:c])
    if name.startswith("alchemical_types_"):
        c = int(name.rsplit("_", 1)[1])
        return _make(name, "legacy = False with %d species: C = 4 pair kernels, one network, species tables of %d rows" % (c, c),
                     [type_count_box(c, 200 + c)], ALCHEMICAL, TYPES11[:c])
    if name in BUCKET_COUNTS:
        counts = BUCKET_COUNTS[name]
        return _make(name, "k_sp_count / k_sp_scan / k_sp_fill, sp_tile, k_soap_tail_*_set and the weight-gradient kernels at "
                     "bucket sizes %s (64-atom tiles, WG_ATOMS = 32 batches, empty buckets)" % (counts,),
                     [box(counts, TYPES4, 0.05, 300 + sum(counts))])
    if name.startswith("small_"):
        n = int(name.rsplit("_", 1)[1])
        return _make(name, "cdiv(N, 4) wave-per-atom kernels at N %% 4 = %d" % (n % 4), [small_box(n, 500 + n)])
    return {
        "dense_lattice": lambda: _make("dense_lattice", "one centre's row crosses a 256-pair block of k_soap_expand_bwd_p and "
                                       "many 32-pair chunks of k_soap_expand_w; self-image pairs", [dense_lattice_system()]),
        "cluster_spans": lambda: _make("cluster_spans", "256-pair blocks that span 14 and 15 centres: the staged / unstaged edge "
                                       "of k_soap_expand_bwd_p at NCOEF = 1120", clusters()),
        "holes": lambda: _make("holes", "zero-length CSR rows inside a block's centre span", clusters(holes=True)),
        "mixed": lambda: _make("mixed", "staged and unstaged blocks in one launch; k_cell_grad over four systems, two without "
                               "pairs; an empty system", mixed()),
        "lone_atom": lambda: _make("lone_atom", "18 self-image pairs: dE/dR is zero, dE/dcell is not", lone_atom()),
        "two_atoms_slab": lambda: _make("two_atoms_slab", "triclinic, pbc (T, T, F)", two_atoms_slab()),
        "left_handed": lambda: _make("left_handed", "negative-determinant triclinic cell", left_handed()),
        "sheared_batch": lambda: _make("sheared_batch", "per-system dE/dcell of three differently sheared cells", sheared_batch()),
        "chunks": lambda: _make("chunks", "n_chunks = 2 in the training pass, one bucket smaller than the chunk count",
                                [box(CHUNK_COUNTS, TYPES4, 0.02, 900)]),
    }[name]()


TYPE_CASES = tuple("legacy_types_%d" % c for c in TYPE_COUNTS_LEGACY) + tuple("alchemical_types_%d" % c for c in TYPE_COUNTS_ALCHEMICAL)
BUCKET_CASES = tuple(BUCKET_COUNTS)
ROW_CASES = tuple("small_%d" % n for n in SMALL_N) + ("dense_lattice", "cluster_spans", "holes", "mixed")
CELL_CASES = ("lone_atom", "two_atoms_slab", "left_handed", "sheared_batch")
INFERENCE_CASES = TYPE_CASES + BUCKET_CASES + ROW_CASES + CELL_CASES
TRAINING_CASES = ("legacy_types_1", "legacy_types_5", "legacy_types_9", "legacy_types_10", "alchemical_types_9",
                  "bucket_32_33_31_0", "bucket_70_0_1_0", "bucket_0_0_0_130", "holes", "chunks")
ALL_CASES = INFERENCE_CASES + ("chunks",)


# ---- collation ---------------------------------------------------------------------------------------------------------------
def min_distance(pos, cell, pbc):
    """The smallest distance between two atoms of a system, images included (inf without a pair inside 2 A)."""
    if len(pos) == 0:
        return math.inf
    _, _, _, d = onl.neighbor_list(pos.numpy(), cell.numpy(), list(pbc), 2.0)
    return float(np.linalg.norm(d, axis=1).min()) if len(d) else math.inf


@functools.lru_cache(maxsize=None)
def batch(name):
    """The collated batch: the oracle's neighbour list of every system at the SOAP cutoff, centres offset per system.
    ``first_atom`` has one entry per system and the total: an empty system repeats an offset."""
    c = case(name)
    pos_l, z_l, cell_l, i_l, j_l, s_l, sys_l, first = [], [], [], [], [], [], [], [0]
    for k, (pos, z, cell, pbc) in enumerate(c.systems):
        off = first[-1]
        i, j, s, _ = onl.neighbor_list(pos.numpy(), cell.numpy(), list(pbc), CUTOFF)
        pos_l.append(pos); z_l.append(z.long()); cell_l.append(cell)
        i_l.append(torch.tensor(i, dtype=torch.long) + off); j_l.append(torch.tensor(j, dtype=torch.long) + off)
        s_l.append(torch.tensor(s, dtype=torch.long).reshape(-1, 3))
        sys_l.append(torch.full((len(pos),), k, dtype=torch.long))
        first.append(off + len(pos))
    return {"positions": torch.cat(pos_l), "species": torch.cat(z_l), "cells": torch.stack(cell_l), "centers": torch.cat(i_l),
            "neighbors": torch.cat(j_l), "cell_shifts": torch.cat(s_l), "system_indices": torch.cat(sys_l),
            "first_atom": first, "pbcs": [list(s[3]) for s in c.systems]}


def neighbour_counts(b):
    return torch.bincount(b["centers"], minlength=b["positions"].shape[0])


def self_image_pairs(b):
    return int((b["centers"] == b["neighbors"]).sum())


def type_counts(name):
    c, b = case(name), batch(name)
    return tuple(int((b["species"] == t).sum()) for t in c.types)


def centre_spans(b):
    """``ctr[min(p + 255, E - 1)] - ctr[p] + 1`` over the 256-pair blocks ``p = 0, 256, ...`` in centre-sorted order: the number
    of centres whose adjoint rows a workgroup of ``k_soap_expand_bwd_p`` would stage."""
    ctr = b["centers"]
    assert bool((ctr[1:] >= ctr[:-1]).all())
    e = len(ctr)
    return [int(ctr[min(p + 255, e - 1)] - ctr[p] + 1) for p in range(0, e, 256)]


def model_dims(n_types, legacy, n_per_l=N_PER_L, hidden=32):
    """The dimensions ``soap_model_create`` derives, and the byte counts its dispatch compares, from ``n_per_l`` alone."""
    c = n_types if legacy else 4
    ncoef = sum((2 * l + 1) * n * c for l, n in enumerate(n_per_l))
    s = sum((n * c) ** 2 for n in n_per_l)
    n_sets = n_types if legacy else 1
    return {"C": c, "ncmax": max(n_per_l) * c, "S": s, "NCOEF": ncoef, "n_sets": n_sets, "ps_bwd_bytes": (ncoef + s) * 4,
            "lds_tail": (s + 256 * (hidden + 1) + 8 + 2 * hidden) * 4, "NT": (n_sets + 1) // 2 if n_sets <= 8 else 0}


# ---- parameters and the oracle -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def params(name, seed=1):
    """``oracle.soap.synthetic_params`` in fp32 with the LayerNorm weights and biases perturbed (the folded weights of the
    stacked, sorted and packed tails must be exercised)."""
    c = case(name)
    p = osoap.synthetic_params(c.hypers, len(c.types), osoap.basis(c.hypers)[0], seed, torch.float32)
    g = torch.Generator().manual_seed(3)
    for k in p:
        if k.startswith("layernorm."):
            p[k] = p[k] + 0.3 * torch.randn(p[k].shape, generator=g)
    return p


@functools.lru_cache(maxsize=None)
def seed_weights(name):
    """The seed of the reverse pass: U(0.5, 1.5) per atom."""
    n = batch(name)["positions"].shape[0]
    return torch.rand(n, generator=torch.Generator().manual_seed(11), dtype=torch.float64) + 0.5


@memo_oracle
def _reference(p, hypers, types, b, w, dtype):
    p = {k: v.to(dtype) for k, v in p.items()}
    r = b["positions"].clone().to(dtype).requires_grad_(True)
    cells = b["cells"].clone().to(dtype).requires_grad_(True)
    a, f = osoap.soap_bpnn_atomic_energies(p, hypers, types, r, cells, b["centers"], b["neighbors"], b["cell_shifts"],
                                           b["species"], b["system_indices"], return_features=True)
    gr, gc = torch.zeros_like(r), torch.zeros_like(cells)
    if len(b["centers"]):
        gr, gc = torch.autograd.grad((a * w.to(dtype)).sum(), [r, cells])
    return {"atomic": a.detach().double(), "features": f.detach().double(), "grad_positions": gr.double(),
            "grad_cells": gc.double()}


def reference(name, dtype=torch.float64):
    """Per-atom energies, features, and ``dE/dR``, ``dE/dcell`` of ``sum_i w_i e_i`` (``w = seed_weights``) of the oracle
    evaluated in ``dtype`` on the fp32 parameters and inputs the device receives."""
    c = case(name)
    return _reference(params(name), c.hypers, c.types, batch(name), seed_weights(name), dtype)


@functools.lru_cache(maxsize=None)
def training_targets(name):
    """Seeded energy targets per system and gradient targets per atom."""
    b = batch(name)
    g = torch.Generator().manual_seed(5)
    te = torch.randn(b["cells"].shape[0], generator=g, dtype=torch.float64) * 3
    tg = torch.randn(b["positions"].shape[0], 3, generator=g, dtype=torch.float64) * 0.3
    return te, tg


@memo_oracle
def _training_reference(p, hypers, types, b, te, tg, with_forces):
    """The reference's step in torch autograd, fp64: E, dE/dR with create_graph, MSE(E/atom) + MSE(dE/dR), backward. A
    parameter the loss does not depend on (the network of an absent type) keeps ``None``."""
    p = {k: v.double().clone().requires_grad_(True) for k, v in p.items()}
    r = b["positions"].clone().requires_grad_(True)
    sysidx, n_sys = b["system_indices"], b["cells"].shape[0]
    atomic = osoap.soap_bpnn_atomic_energies(p, hypers, types, r, b["cells"], b["centers"], b["neighbors"], b["cell_shifts"],
                                             b["species"], sysidx)
    energies = torch.zeros(n_sys, dtype=torch.float64).index_add(0, sysidx, atomic)
    n_atoms = torch.bincount(sysidx, minlength=n_sys).double()
    loss = (((energies - te) / n_atoms) ** 2).mean()
    g = None
    if with_forces:
        (g,) = torch.autograd.grad(energies.sum(), r, create_graph=True)
        loss = loss + ((g - tg) ** 2).mean()
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in p.items()}, energies.detach(), None if g is None else g.detach()


def training_reference(name, with_forces=True):
    c = case(name)
    te, tg = training_targets(name)
    return _training_reference(params(name), c.hypers, c.types, batch(name), te, tg, with_forces)
