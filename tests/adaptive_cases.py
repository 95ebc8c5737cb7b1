"""Inputs that drive the adaptive cutoff (``num_neighbors_adaptive``, methods "solver" and "grid") to the rows, clamps, plateaus
and probe counts at which its kernels take another path, shared by ``test_adaptive_cases_cpu.py`` (the premises: each case is
what it says) and ``test_gpu_adaptive_edges.py`` (the device against the fp64 oracle ``oracle/pet.py``). No GPU import at module
level.

The kernels: ``k_adaptive_solve`` / ``k_adaptive_grid`` / ``k_adaptive_keep`` / ``k_reverse_all`` (graph.hip), the adjoints
``k_adapt_gr`` / ``k_adapt_dv`` / ``k_adapt_dv_grid`` / ``k_pos_grad_acc`` and the cell term (pet_bwd.hip), the tangents
``k_adapt_rdot`` / ``k_adapt_rdot_grid`` (so.hip). All of them walk an atom's row of the ALL-EDGE CSR (every input edge, kept
or not) with 16 lanes, and a launch covers 16 atoms per 256 threads: a row count of 0, 1, 15, 16, 17 ... and an atom count that
is no multiple of 16 are the structural edges; the clamp of the solver's cutoff to [rc / 16, rc] (which switches the
implicit-function gradient off), a root on a plateau of the neighbour count, a Newton step that leaves its bracket, rows of
self-images and the number of probe cutoffs of the grid method are the numerical ones.

Every geometric case is a FULL neighbour list (each edge has its partner) of fp32-rounded positions; the oracle is given those
values. A case carries its own target count and ``cutoff_width_adaptive``; the maximal cutoff is 4.5 A throughout.

  rows         open clusters in which every atom sees every other (``attn_token_cases.make_cluster``), sizes 1, 2, 3, 16, 17,
               18, 32, 33, 34, 49: all-edge rows of 0, 1, 2, 15, 16, 17, 31, 32, 33, 48 edges, 205 atoms (= 12 * 16 + 13: the
               last launch group runs the ``gid >= N`` fallback row). ``rows_small``: the first six clusters, 57 atoms.
  sparse       the target is above what is there: an isolated atom, a dimer at 4.4 A, a trimer and a dilute system periodic
               along x and y. Cutoffs in (rc - 0.6, rc]; the isolated atom's is rc.
  plateau      a 12-atom ball of diameter <= 0.9 A, target 12, width 1: at the root every bump is saturated (11 + 12 (r / rc)^3
               = 12), the root is rc 12^(-1/3) = 1.96556 A, only the cubic baseline has a slope (dn = 1.526) and d r / d d = 0.
  lower_clamp  a 61-atom ball of diameter <= 0.1 A, target 12, width 0.25: the root (about 0.2 A) lies below rc / 16 = 0.28125 A,
               every cutoff is clamped to exactly that and the cutoff gradient is switched off. The grid method has 64 probes
               here, the most that are served, and no probe at which the count crosses the target.
  shoulder     a centre with 4 close neighbours and 30 atoms on a shell of 3.5 A: the count is flat between the two, the first
               Newton step from rc / 2 leaves the bracket [rc / 2, rc] and the solver bisects (``solver_trace``).
  thin_cells   one batch of a 1-atom cubic cell of 3.0 A (18 edges, every one a self-image: dE/dR = 0, dE/dcell != 0 through
               the cutoffs), the 3-atom 4.0 A cell of ``_ewald_oracle.small_cell``, an empty system and a 17-atom open cluster.

``PROBE_COUNTS`` carries hypers, not geometry: the grid method's probe cutoffs are ``torch.arange(0.5, cutoff, width / 4)``,
whose length torch takes from Python doubles, while ``pet_hypers_t`` holds cutoff and width in float32.

Seeds: a case's seed is the first for which no input edge lies within ``MARGIN`` of its pair cutoff under either method
(``first_clear_seed``; the fp32 and fp64 oracles then keep the same edges, so kept-edge lists compare bit-exact)."""
import collections
import functools
import math

import numpy as np
import torch

import attn_token_cases as ac
from _memo import memo_oracle
from oracle import nl as onl
from oracle import pet as opet

TYPES = ac.TYPES
CUTOFF = 4.5
METHODS = ("solver", "grid")
MARGIN = 1e-4      # A: no input edge closer than this to its pair cutoff (fp64 oracle)
SEPARATION = 30.0  # A between the clusters of one open system

Spec = collections.namedtuple("Spec", "target width reason")
SPECS = {
    "rows": Spec(12.0, 1.0, "16-lane row loops at 0 .. 48 edges; 205 atoms: the fallback row of the last launch group"),
    "rows_small": Spec(12.0, 1.0, "the first six clusters of rows (57 atoms), for the second-order passes"),
    "sparse": Spec(12.0, 1.0, "the target is never reached: cutoffs just below rc, the isolated atom's exactly rc"),
    "plateau": Spec(12.0, 1.0, "root on a plateau of the count: only the cubic baseline has a slope, d r / d d = 0"),
    "lower_clamp": Spec(12.0, 0.25, "root below rc / 16: clamped, gradient switched off; 64 probes of the grid method. The "
                        "full PET oracle is well-behaved here (distances of 0.01 .. 0.1 A are ordinary numbers): all tests"),
    "shoulder": Spec(12.0, 1.0, "flat count between two shells: a Newton step leaves the bracket, the solver bisects"),
    "thin_cells": Spec(12.0, 1.0, "self-image rows, a cell thinner than the cutoff, an empty system, dE/dcell"),
}
GEOMETRIC = tuple(SPECS)
ROWS_CLUSTERS = (1, 2, 3, 16, 17, 18, 32, 33, 34, 49)
ROWS_SMALL_CLUSTERS = ROWS_CLUSTERS[:6]
# what each seeded construction is seeded with (first_clear_seed)
SEEDS = {"rows": {1: 0, 2: 0, 3: 0, 16: 0, 17: 1, 18: 0, 32: 0, 33: 15, 34: 0, 49: 1},
         "sparse": 0, "plateau": 0, "lower_clamp": 0, "shoulder": 0, "thin_cells": 0}

# (cutoff, cutoff_width_adaptive, probes of the reference or None where the device must refuse: 2 .. 64 are built)
PROBE_COUNTS = ((4.5, 0.64, 25), (4.5, 0.32, 50), (4.5, 0.25, 64), (4.5, 0.24, None), (0.7, 1.0, None))
GRID_MAX_PROBES = 64  # csrc/common.h (asserted by the premises test)

System = collections.namedtuple("System", "positions cells centers neighbors cell_shifts species system_indices group labels")


def hypers(case, method, **extra):
    s = SPECS[case]
    return dict(opet.DEFAULT_HYPERS, num_neighbors_adaptive=s.target, adaptive_cutoff_method=method,
                cutoff_width_adaptive=s.width, **extra)


# ---- probe counts ------------------------------------------------------------------------------------------------------------
def reference_probe_count(cutoff, width):
    """what the reference counts: the length of ``torch.arange(0.5, cutoff, width / 4)`` from Python doubles"""
    return len(torch.arange(0.5, cutoff, width / 4.0, dtype=torch.float64))


def float32_probe_count(cutoff, width):
    """``ceil((cutoff - 0.5) / (width / 4))`` on the float32-rounded hypers, as ``pet_hypers_t`` holds them"""
    c, w = float(np.float32(cutoff)), float(np.float32(width))
    return int(math.ceil((c - 0.5) / (w / 4.0)))


# ---- geometry ----------------------------------------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _species(rng, n):
    return np.array(TYPES)[rng.integers(0, 4, n)]


def _all_pairs(n):
    a, b = np.nonzero(~np.eye(n, dtype=bool))
    return a, b, np.zeros((len(a), 3), np.int64)


def _nl(pos, cell, pbc):
    i, j, s, _ = onl.neighbor_list(pos, cell, list(pbc), CUTOFF)
    return i.astype(np.int64), j.astype(np.int64), s.astype(np.int64).reshape(-1, 3)


def _collate(parts, n_systems=None):
    """parts: (positions [n, 3] fp32-representable, species, cell, (i, j, S), system, group); labels: one per group"""
    pos, z, ctr, nbr, sh, sysidx, group, off = [], [], [], [], [], [], [], 0
    n_sys = n_systems or max(p[4] for p in parts) + 1
    cells = np.zeros((n_sys, 3, 3))
    for p, zz, cell, (i, j, s), system, g in parts:
        assert np.array_equal(p, _f32(p)) and np.array_equal(cell, _f32(cell))
        pos.append(p)
        z.append(zz)
        ctr.append(i + off)
        nbr.append(j + off)
        sh.append(s)
        sysidx += [system] * len(p)
        group += [g] * len(p)
        cells[system] = cell
        off += len(p)
    return (torch.tensor(np.concatenate(pos), dtype=torch.float32), torch.tensor(cells, dtype=torch.float32),
            torch.tensor(np.concatenate(ctr)), torch.tensor(np.concatenate(nbr)), torch.tensor(np.concatenate(sh)),
            torch.tensor(np.concatenate(z)), torch.tensor(sysidx, dtype=torch.long), np.array(group))


OPEN_CELL = 1000.0 * np.eye(3)  # an open system: no edge carries a shift, the cell enters nothing


def cluster_part(m, seed, d_max, origin, system, group):
    c = ac.make_cluster(m, seed, d_max)
    return (_f32(c.positions + np.asarray(origin)), c.species, OPEN_CELL, _all_pairs(m), system, group)


def _rows_parts(sizes, seeds):
    return [cluster_part(m, seeds[m], ac.D_MAX, [SEPARATION * (k + 1), 0.0, 0.0], 0, k) for k, m in enumerate(sizes)]


def _sparse_parts(seed):
    rng = np.random.default_rng([seed, 101])
    parts = [(np.zeros((1, 3)), _species(rng, 1), np.zeros((3, 3)), _all_pairs(1), 0, 0),
             (_f32([[0.0, 0.0, 0.0], [0.0, 0.0, 4.4]]), _species(rng, 2), np.zeros((3, 3)), _all_pairs(2), 1, 1),
             (_f32([[0.0, 0.0, 0.0], [1.1, 0.0, 0.0], [0.3, 1.4, 0.2]] + rng.uniform(-0.1, 0.1, (3, 3))), _species(rng, 3),
              np.zeros((3, 3)), _all_pairs(3), 2, 2)]
    cell = _f32(np.diag([11.0, 12.0, 0.0]) + np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [0.0, 0.0, 0.0]]))
    pos = _f32(rng.uniform(0.0, 1.0, (14, 3)) * np.array([11.0, 12.0, 9.0]))
    parts.append((pos, _species(rng, 14), cell, _nl(pos, cell, (True, True, False)), 3, 3))
    return parts


def _shoulder_parts(seed):
    rng = np.random.default_rng([seed, 103])

    def sphere(n, radius, jitter):
        v = rng.normal(size=(n, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True) * (radius + rng.uniform(-jitter, jitter, (n, 1)))

    pos = _f32(np.concatenate([np.zeros((1, 3)), sphere(4, 1.2, 0.2), sphere(30, 3.5, 0.1)]))
    return [(pos, _species(rng, len(pos)), np.zeros((3, 3)), _nl(pos, np.zeros((3, 3)), (False,) * 3), 0, 0)]


def _thin_parts(seed):
    from _ewald_oracle import small_cell

    rng = np.random.default_rng([seed, 107])
    one = 3.0 * np.eye(3)
    p1 = _f32([[0.3, 0.7, 1.1]])
    (p3, c3, _), = small_cell()
    p3, c3 = _f32(p3.numpy()), c3.numpy()
    parts = [(p1, _species(rng, 1), one, _nl(p1, one, (True,) * 3), 0, 0),
             (p3, _species(rng, 3), c3, _nl(p3, c3, (True,) * 3), 1, 1),
             cluster_part(17, seed, ac.D_MAX, [0.0, 0.0, 0.0], 3, 2)]
    return parts  # system 2 has a cell and no atom


def _parts(case, seed):
    if case == "rows":
        return _rows_parts(ROWS_CLUSTERS, seed)
    if case == "rows_small":
        return _rows_parts(ROWS_SMALL_CLUSTERS, seed)
    if case == "sparse":
        return _sparse_parts(seed)
    if case == "plateau":
        return [cluster_part(12, seed, 0.9, [0.0, 0.0, 0.0], 0, 0)]
    if case == "lower_clamp":
        return [cluster_part(61, seed, 0.1, [0.0, 0.0, 0.0], 0, 0)]
    if case == "shoulder":
        return _shoulder_parts(seed)
    if case == "thin_cells":
        return _thin_parts(seed)
    raise KeyError(case)


LABELS = {"rows": ["m = %d" % m for m in ROWS_CLUSTERS], "rows_small": ["m = %d" % m for m in ROWS_SMALL_CLUSTERS],
          "sparse": ["isolated", "dimer", "trimer", "dilute xy"], "plateau": ["ball 12"], "lower_clamp": ["ball 61"],
          "shoulder": ["two shells"], "thin_cells": ["cell 3.0", "cell 4.0", "cluster 17"]}


def _build(case, seed):
    parts = _parts(case, seed)
    if case == "thin_cells":
        cell = 5.0 * np.eye(3)
        t = _collate(parts, 4)
        t[1][2] = torch.tensor(cell, dtype=torch.float32)
        return System(*t, LABELS[case])
    return System(*_collate(parts), LABELS[case])


@functools.lru_cache(maxsize=None)
def system(case):
    return _build(case, SEEDS["rows"] if case in ("rows", "rows_small") else SEEDS[case])


def inputs(case):
    """the case as the ``inp`` dictionary the oracle helpers of test_gpu_train.py take"""
    s = system(case)
    return {"positions": s.positions, "cells": s.cells, "centers": s.centers, "neighbors": s.neighbors,
            "cell_shifts": s.cell_shifts, "species": s.species, "system_indices": s.system_indices}


def all_edge_rows(s):
    return np.bincount(s.centers.numpy(), minlength=len(s.species))


# ---- the oracle on a case ----------------------------------------------------------------------------------------------------
def _cutoffs_of(s, target, width, method, dtype):
    _, d = opet.edge_geometry(s.positions.to(dtype), s.cells.to(dtype), s.centers, s.neighbors, s.cell_shifts, s.system_indices)
    solve = opet.adaptive_cutoffs_grid if method == "grid" else opet.adaptive_cutoffs_solver
    return solve(s.centers, d, target, len(s.species), CUTOFF, width), d


@memo_oracle
def _cutoffs(case, method, dtype):
    spec = SPECS[case]
    r, d = _cutoffs_of(system(case), spec.target, spec.width, method, dtype)
    return r.double().numpy(), d.double().numpy()


def cutoffs(case, method, dtype=torch.float64):
    """per-atom cutoffs of the oracle in ``dtype``, as an fp64 array"""
    return _cutoffs(case, method, dtype)[0]


def edge_margin(s, r, d):
    """smallest |d - pair cutoff| over the input edges (inf without edges)"""
    if not len(d):
        return np.inf
    i, j = s.centers.numpy(), s.neighbors.numpy()
    return float(np.abs(d - 0.5 * (r[i] + r[j])).min())


def margin(case, method):
    r, d = _cutoffs(case, method, torch.float64)
    return edge_margin(system(case), r, d)


def cutoff_gradient(case, method):
    """d(sum of the atomic cutoffs)/d(distance of every input edge) from autograd through the fp64 oracle"""
    s, spec = system(case), SPECS[case]
    _, d = opet.edge_geometry(s.positions.double(), s.cells.double(), s.centers, s.neighbors, s.cell_shifts, s.system_indices)
    d = d.clone().requires_grad_(True)
    solve = opet.adaptive_cutoffs_grid if method == "grid" else opet.adaptive_cutoffs_solver
    r = solve(s.centers, d, spec.target, len(s.species), CUTOFF, spec.width)
    (g,) = torch.autograd.grad(r.sum(), d, allow_unused=True)
    return np.zeros(len(d)) if g is None else g.numpy()


@memo_oracle
def _batch(case, method, dtype):
    s = system(case)
    p = opet.synthetic_params(hypers(case, method), TYPES, {"energy": 1}, 0, torch.float32)
    return opet.batch_tensors(hypers(case, method), p["species_to_species_index"], s.positions.to(dtype), s.cells.to(dtype),
                              s.centers, s.neighbors, s.cell_shifts, s.species, s.system_indices)


def batch(case, method, dtype=torch.float64):
    """the oracle's twelve ``batch_data`` tensors of the case"""
    return _batch(case, method, dtype)


def solver_trace(centers, d, target, n_nodes, max_cutoff, width):
    """An instrumented copy of the ten-step loop of ``oracle.pet.adaptive_cutoffs_solver``: (r after the loop, number of
    steps in which each atom's Newton step left the bracket and the bisection took over, the largest residual |n(r) - target|
    at that r)."""
    inv_rc = 1.0 / max_cutoff
    r_lo = torch.zeros(n_nodes, dtype=d.dtype)
    r_hi = torch.full((n_nodes,), max_cutoff, dtype=d.dtype)
    r = 0.5 * r_hi
    bisected = torch.zeros(n_nodes, dtype=torch.long)
    for _ in range(10):
        n, dn = opet._adaptive_n_and_dn(r, d, centers, n_nodes, width, inv_rc, target)
        f = n - target
        below = f <= 0
        r_lo = torch.where(below, r, r_lo)
        r_hi = torch.where(below, r_hi, r)
        r_newton = r - f / dn.clamp_min(1e-6)
        inside = (r_newton >= r_lo) & (r_newton <= r_hi)
        bisected += (~inside).long()
        r = torch.where(inside, r_newton, 0.5 * (r_lo + r_hi))
    n, _ = opet._adaptive_n_and_dn(r, d, centers, n_nodes, width, inv_rc, target)
    return r, bisected, (n - target).abs()


def trace(case):
    s, spec = system(case), SPECS[case]
    _, d = opet.edge_geometry(s.positions.double(), s.cells.double(), s.centers, s.neighbors, s.cell_shifts, s.system_indices)
    return solver_trace(s.centers, d, spec.target, len(s.species), CUTOFF, spec.width)


# ---- the seed search ---------------------------------------------------------------------------------------------------------
def _clear(s, spec):
    for method in METHODS:
        r, d = _cutoffs_of(s, spec.target, spec.width, method, torch.float64)
        if not edge_margin(s, r.numpy(), d.numpy()) >= MARGIN:
            return False
    return True


def first_clear_seed(case, m=None, start=0, limit=1000):
    """the first seed from ``start`` whose construction keeps every input edge ``MARGIN`` off its pair cutoff under both
    methods: of the case, or (``rows``: clusters are independent of each other) of its m-atom cluster"""
    spec = SPECS[case]
    for seed in range(start, limit):
        if m is None:
            s = _build(case, seed)
        else:
            s = System(*_collate([cluster_part(m, seed, ac.D_MAX, [SEPARATION, 0.0, 0.0], 0, 0)]), ["m"])
        if _clear(s, spec):
            return seed
    raise ValueError((case, m))


def rows_start_seed(m):
    """the seed the attention cases use for the cluster size, where they have one: the same cluster if it is clear"""
    return ac.CLUSTER_SEED.get(m, 0)


if __name__ == "__main__":  # the seed table
    print({"rows": {m: first_clear_seed("rows", m, rows_start_seed(m)) for m in ROWS_CLUSTERS},
           **{c: first_clear_seed(c) for c in GEOMETRIC if not c.startswith("rows")}})
