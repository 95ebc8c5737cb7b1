"""Inputs that drive the long-range (Ewald) operator (``metatrain_amd/csrc/ewald.hip``) into the tiles, channel widths, cells
and open-system paths that the handful of inputs of ``test_gpu_long_range.py`` never reaches, shared by
``test_ewald_cases_cpu.py`` (the premises: each case is what it says) and ``test_gpu_long_range_edges.py`` (the device against
the oracle). No GPU import at module level.

A case is ``Case(name, reason, systems, smearing, resolution, cutoff)`` with ``systems`` a list of ``(positions fp64 [n, 3],
cell fp64 [3, 3], pbc)`` that ``_ewald_oracle.collate`` takes. All builders are seeded; clusters and boxes are redrawn until no
two atoms (images included) are closer than ``MIN_DISTANCE``.

The second half holds what both GPU files share: the model's graph and the planned operator of a batch, one run of the
operator, and the per-system bar."""
import collections
import functools
import math
import os

import numpy as np
import torch

import _ewald_oracle as eo
from _memo import memo_oracle
from oracle import pet as opet

Case = collections.namedtuple("Case", "name reason systems smearing resolution cutoff")

SMEARING, RESOLUTION, CUTOFF = 1.4, 1.33, 4.5
MIN_DISTANCE = 0.5
PERIODIC, OPEN = [True] * 3, [False] * 3
NO_CELL = torch.zeros(3, 3, dtype=torch.float64)
QUANTITIES = ("potential", "grad_charges", "grad_positions", "grad_cells")
KINDS = ("atom", "atom", "atom", "system")
MADELUNG_NACL = -1.7475646
OPEN_TILE_SIZES = (32, 33, 64, 150, 1)


def _cubic(length):
    return torch.eye(3, dtype=torch.float64) * float(length)


def min_distance(pos, cell, pbc):
    """The smallest distance between two atoms of a system, images included for a periodic one (inf for fewer than two
    atoms without images inside 2 A)."""
    i, j, S = eo._nl(pos, cell, pbc, 2.0)
    if len(i) == 0:
        return math.inf
    return float(torch.linalg.norm(pos[j] - pos[i] + S.double() @ cell, dim=1).min())


def _spread(draw, cell, pbc, seed):
    """``draw(generator)`` under seed, seed + 1000, ... until the minimum distance is at least ``MIN_DISTANCE``."""
    for attempt in range(200):
        pos = draw(torch.Generator().manual_seed(seed + 1000 * attempt))
        if min_distance(pos, cell, pbc) >= MIN_DISTANCE:
            return pos
    raise AssertionError("no draw with min d >= %g" % MIN_DISTANCE)


def open_cluster(n, seed):
    """``n`` points uniform in a cube of edge 2.2 n^(1/3) A, no cell."""
    edge = 2.2 * n ** (1.0 / 3.0)
    pos = _spread(lambda g: torch.rand(n, 3, generator=g, dtype=torch.float64) * edge, NO_CELL, OPEN, seed)
    return pos, NO_CELL.clone(), OPEN


def periodic_box(n, cell, seed):
    pos = _spread(lambda g: torch.rand(n, 3, generator=g, dtype=torch.float64) @ cell, cell, PERIODIC, seed)
    return pos, cell, PERIODIC


def triclinic43():
    """The triclinic 43-atom system of ``_ewald_oracle.mixed_batch``."""
    return eo.mixed_batch(CUTOFF)[1]


SMALL_CELL = 3.0  # 28 walked k-vectors at lambda = 1.33: one partly filled k tile
ELONGATED = (84.5, 6.0, 6.5)
BEYOND_LIMIT = (85.5, 6.0, 6.5)
SHEARED = [[9.0, 0.0, 0.0], [7.5, 5.0, 0.0], [6.0, 4.0, 7.0]]


def open_tiles():
    return [open_cluster(n, 100 + n) for n in OPEN_TILE_SIZES]


def periodic_tiles():
    empty = (torch.zeros(0, 3, dtype=torch.float64), _cubic(9.0), PERIODIC)
    return [periodic_box(32, _cubic(9.0), 32), empty, periodic_box(33, _cubic(9.0), 33),
            periodic_box(2, _cubic(SMALL_CELL), 2)]


def elongated_limit():
    return [periodic_box(37, torch.diag(torch.tensor(ELONGATED, dtype=torch.float64)), 37)]


def sheared():
    return [periodic_box(33, torch.tensor(SHEARED, dtype=torch.float64), 34)]


def left_handed():
    pos, cell, pbc = triclinic43()
    return [(pos, cell[[1, 0, 2]].clone(), pbc)]


def unwrapped():
    pos, cell, pbc = triclinic43()
    g = torch.Generator().manual_seed(43)
    moves = torch.randint(-3, 4, (len(pos), 3), generator=g).double()
    return [(pos + moves @ cell, cell, pbc)]


def supercell():
    pos, cell, pbc = triclinic43()
    double = cell.clone()
    double[0] *= 2.0
    return [(pos, cell, pbc), (torch.cat([pos, pos + cell[0]]), double, pbc)]


def other_constants():
    return [triclinic43(), open_cluster(40, 140)]


def nacl():
    pos, cell, _ = eo.nacl_system()
    return [(pos, cell, PERIODIC)]


def _make(name, reason, systems, smearing=SMEARING, resolution=RESOLUTION, cutoff=CUTOFF):
    return Case(name, reason, systems, float(smearing), float(resolution), float(cutoff))


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "mixed":  # the batch of test_gpu_long_range.py, for the per-system bar
        return _make(name, "1-atom cell, triclinic 43, cubic 130, open 17", eo.mixed_batch(CUTOFF))
    return {
        "open_tiles": lambda: _make("open_tiles", "later chunks of k_ew_pairs, several row tiles, waves 1-3 and a second column "
                                    "round of k_ew_force<false>, self-exclusion at a0 > 0", open_tiles()),
        "periodic_tiles": lambda: _make("periodic_tiles", "exactly full and just-over tiles, a zero-atom system with k-vectors, "
                                        "fewer than 32 walked k-vectors, self-image edges", periodic_tiles()),
        "elongated_limit": lambda: _make("elongated_limit", "reciprocal index 63, the largest LDS table, strides 63 / 4 / 4",
                                         elongated_limit()),
        "sheared": lambda: _make("sheared", "box bound 6 / 6 / 7 around a 562-vector sphere, triclinic inverse in dL/dcell",
                                 sheared()),
        "left_handed": lambda: _make("left_handed", "det < 0: fabs(det) against the signed inverse", left_handed()),
        "unwrapped": lambda: _make("unwrapped", "wrapped phase tables against the unwrapped s_i of dL/dcell", unwrapped()),
        "supercell": lambda: _make("supercell", "k-set, weights and tiles as a function of size", supercell()),
        "other_constants": lambda: _make("other_constants", "the coefficients of k_ew_finish, inv_R in the open kernels and in "
                                         "ew_excl", other_constants(), 1.0, 1.0, 3.0),
        "nacl": lambda: _make("nacl", "Madelung constant", nacl(), 0.5, 2.0 * math.pi / 18.0, 1.5),
    }[name]()


OPERATOR_CASES = ("open_tiles", "periodic_tiles", "elongated_limit", "sheared", "left_handed", "unwrapped", "supercell",
                  "other_constants")
ALL_CASES = OPERATOR_CASES + ("nacl",)
# systems taken from ``mixed_batch`` as they are (the 43-atom cell: min d = 0.31 A), not drawn and redrawn here
GIVEN_SYSTEMS = {"left_handed": (0,), "unwrapped": (0,), "supercell": (0, 1), "other_constants": (0,)}


@functools.lru_cache(maxsize=None)
def batch(name):
    c = case(name)
    return eo.collate(c.systems, c.cutoff)


@functools.lru_cache(maxsize=None)
def charges(name, channels):
    """Seeded ``(charges, dL/dV)`` fp64 ``[N, C]``. ``supercell``: both halves of the 86-atom cell repeat the primitive cell's
    rows. ``nacl``: charges +-1."""
    n = batch(name)["positions"].shape[0]
    g = torch.Generator().manual_seed(17 + channels)
    if name == "supercell":
        n = n // 3
    q = torch.randn(n, channels, generator=g, dtype=torch.float64)
    gv = torch.randn(n, channels, generator=g, dtype=torch.float64)
    if name == "supercell":
        q, gv = torch.cat([q] * 3), torch.cat([gv] * 3)
    if name == "nacl":
        q = eo.nacl_system()[2].repeat(1, channels)
    return q, gv


@memo_oracle
def _reference(b, q, gv, smearing, resolution, cutoff, dtype):
    return eo.operator_reference(b, q, gv, smearing, resolution, cutoff, dtype)


def reference(name, channels, dtype):
    """(V, dL/dq, dL/dR, dL/dcell) of the oracle for ``charges(name, channels)``, evaluated in ``dtype``."""
    c = case(name)
    q, gv = charges(name, channels)
    return _reference(batch(name), q, gv, c.smearing, c.resolution, c.cutoff, dtype)


def max_reciprocal_index(cell, resolution):
    return int(eo.kvector_indices(cell, resolution).abs().max())


# ---- the Madelung composition ---------------------------------------------------------------------------------------------
def madelung_composition(potential, dtype=torch.float64):
    """From the operator's potential ``[8, 1]`` on ``nacl`` (k-space, self, background and exclusion, times P) to the
    full Coulomb potential at the atom at the origin: add back, in fp64, ``P sum_edges q_j erf(d/a) f(d) / d`` over the graph's
    edges and the real-space ``P sum_images q_j erfc(d/a) / d``. ``P * MADELUNG_NACL`` is the answer. ``potential=None``: the
    k-space part is ``_ewald_oracle.kspace_self_background`` evaluated in ``dtype`` (the yardstick e32)."""
    c, b = case("nacl"), batch("nacl")
    pos, cell, q = eo.nacl_system()
    i, j, S = b["centers"], b["neighbors"], b["cell_shifts"]
    d = torch.linalg.norm(pos[j] - pos[i] + S.double() @ cell, dim=1)
    w = torch.erf(d / (math.sqrt(2.0) * c.smearing)) / d * eo.cutoff_f(d, c.cutoff)
    excl = torch.zeros_like(q).index_add(0, i, w[:, None] * q[j])
    if potential is None:
        k = eo.kspace_self_background(pos.to(dtype), cell.to(dtype), q.to(dtype), c.smearing, c.resolution).double()
        potential = eo.PREFACTOR * (k - excl)
    v = potential.detach().cpu().double().reshape(8, 1)
    return float((v + eo.PREFACTOR * (excl + eo.real_space_erfc(pos, cell, q, c.smearing)))[0, 0])


# ---- the per-system bar ---------------------------------------------------------------------------------------------------
def system_rows(b, kind, s):
    """Rows of a quantity that belong to system ``s``: its atoms, or its one per-system entry."""
    return slice(b["first_atom"][s], b["first_atom"][s + 1]) if kind == "atom" else slice(s, s + 1)


def system_bar(ref, f32, rows):
    """``(bar, scale, e32, fell_back)`` of one quantity on one system: ``bar = max(1e-5 scale, 2 e32)`` with ``scale = max|ref|``
    and ``e32 = max|oracle_fp32 - ref|`` over the system's rows. Where the quantity vanishes by symmetry on that system
    (``scale < 1e-9`` of the batch-wide one) the batch-wide scale takes its place."""
    whole = float(ref.abs().max()) if ref.numel() else 0.0
    r, y = ref[rows], f32[rows]
    scale = float(r.abs().max()) if r.numel() else 0.0
    e32 = float((y - r).abs().max()) if r.numel() else 0.0
    fell_back = scale < 1e-9 * whole
    if fell_back:
        scale = whole
    return max(1e-5 * scale, 2.0 * e32), scale, e32, fell_back


def check_per_system(label, b, names, kinds, got, ref, f32):
    """Print ``(case, system, quantity, e32, relmax)`` for every system and quantity, then assert
    ``max|got - ref| <= max(1e-5 max|ref|, 2 max|oracle_fp32 - ref|)`` with every maximum over the system's rows."""
    bad = []
    for name, kind, g, r, y in zip(names, kinds, got, ref, f32):
        g = g.detach().cpu().double()
        assert g.shape == r.shape, (label, name, g.shape, r.shape)
        worst = (0.0, 0.0, -1)
        for s in range(len(b["first_atom"]) - 1):
            rows = system_rows(b, kind, s)
            if r[rows].numel() == 0:
                print(f"({label}, {s}, {name}: no rows)")
                continue
            bar, scale, e32, fell_back = system_bar(r, y, rows)
            err = float((g[rows] - r[rows]).abs().max())
            unit = scale if scale > 0.0 else 1.0
            note = " [zero by symmetry: batch-wide scale]" if fell_back else ""
            print(f"({label}, {s}, {name}, {e32 / unit:.2e}, {err / unit:.2e}){note}")
            if not fell_back and err / unit > worst[0]:
                worst = (err / unit, e32 / unit, s)
            if not err <= bar:
                bad.append((s, name, err / unit, e32 / unit))
        print(f"[worst] {label} | {name} | relmax {worst[0]:.1e} | e32 {worst[1]:.1e} | system {worst[2]}")
    assert not bad, (label, bad)


# ---- the device side ------------------------------------------------------------------------------------------------------
def lr_hypers(smearing=SMEARING, resolution=RESOLUTION, **extra):
    h = dict(opet.DEFAULT_HYPERS, **extra)
    h["long_range"] = {"enable": True, "use_ewald": True, "smearing": smearing, "kspace_resolution": resolution,
                       "interpolation_nodes": 5}
    return h


def graph(b, dev, hypers=None, species=None):
    """The model's strict graph of a batch (a weight-less model builds it: the operator reads rows and distances only)."""
    from metatrain_amd import runtime as rt

    model = rt.HipModel(hypers or lr_hypers(), eo.TYPES)
    model.load_species_table()
    n = b["positions"].shape[0]
    z = torch.full((n,), 6, dtype=torch.int32) if species is None else species
    g = rt.HipGraph(model, b["positions"].float().to(dev), b["cells"].float().to(dev), b["centers"].to(dev),
                    b["neighbors"].to(dev), b["cell_shifts"].to(dev), z.to(dev), b["system_indices"].int().to(dev))
    return model, g


def operator(b, dev, smearing=SMEARING, resolution=RESOLUTION, cutoff=CUTOFF):
    from metatrain_amd import long_range as lr

    hypers = None if cutoff == CUTOFF else lr_hypers(smearing, resolution, cutoff=cutoff)
    model, g = graph(b, dev, hypers)
    ew = lr.EwaldHip(smearing, resolution, cutoff).plan(b["cells"], b["pbcs"], b["first_atom"])
    return model, g, ew


def run(ew, g, b, q, gv, dev):
    pos = b["positions"].float().to(dev)
    qd, gd = q.float().to(dev), gv.float().to(dev)
    v = ew.potential(g, pos, qd)
    gq, gp, gc = ew.backward(g, pos, qd, gd, want_cell_grad=True)
    return v, gq, gp, gc


# ---- the whole model on a batch of open and periodic systems ---------------------------------------------------------------
FACE_ATOM, FACE_GAP, FACE_STEP = 5, 0.01, 0.03  # atom of the box, its distance from the face x = L, its step across it


@functools.lru_cache(maxsize=None)
def model_systems():
    """A 40-atom open cluster, the 64-atom periodic box of ``_ewald_oracle.periodic_box_batch`` with atom ``FACE_ATOM`` placed
    ``FACE_GAP`` A inside the face x = L, and the first QM9 frame; species alongside."""
    cluster = open_cluster(40, 240)
    pos, z, cell = opet.random_box(64, seed=3, dtype=torch.float64)
    pos = pos.clone()
    pos[FACE_ATOM, 0] = cell[0, 0] - FACE_GAP
    g = dict(np.load(os.path.join(eo.GOLDEN, "qm9_first5.npz")))
    qm9 = (torch.tensor(g["pos0"]).double(), NO_CELL.clone(), OPEN)
    zc = torch.tensor(eo.TYPES, dtype=torch.int32)[torch.randint(0, 4, (40,), generator=torch.Generator().manual_seed(41))]
    species = torch.cat([zc, z.to(torch.int32), torch.tensor(g["z0"]).to(torch.int32)])
    return [cluster, (pos, cell.double(), PERIODIC), qm9], species


@functools.lru_cache(maxsize=None)
def model_batch(moved=False):
    """``moved``: every atom displaced by a seeded step of up to 0.05 A per axis, ``FACE_ATOM`` of the box by ``FACE_STEP``
    along +x (across the face); same cells and layout."""
    systems, species = model_systems()
    if moved:
        g = torch.Generator().manual_seed(77)
        out = []
        for k, (p, c, pbc) in enumerate(systems):
            step = torch.randn(p.shape, generator=g, dtype=torch.float64)
            step = step / torch.linalg.norm(step, dim=1, keepdim=True) * (0.05 * torch.rand(len(p), 1, generator=g, dtype=torch.float64))
            if k == 1:
                step[FACE_ATOM] = torch.tensor([FACE_STEP, 0.0, 0.0], dtype=torch.float64)
            out.append((p + step, c, pbc))
        systems = out
    b = eo.collate(systems, CUTOFF)
    b["species"] = species
    return b
