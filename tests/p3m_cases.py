"""Inputs that drive the P3M operator (``metatrain_amd/csrc/p3m.hip``) into both node placements, folded stencils, floor
boundaries, anisotropic and left-handed meshes, long and empty bins, systems without a mesh and every channel path, shared by
``test_p3m_cpu.py`` (the premises: each case is what it says) and ``test_gpu_p3m.py`` (the device against the oracle
``_p3m_oracle``). No GPU import at module level.

A case is ``Case(name, reason, systems, nodes)``: ``systems`` as ``_ewald_oracle.collate`` takes them, ``nodes`` the
interpolation orders it runs at. Positions are rounded to fp32 once, here: the device reads fp32 positions, and the assignment
function of p <= 2 is not smooth where the stencil moves, so the oracle is given the very positions the device sees. Smearing,
mesh spacing and cutoff are the model defaults throughout."""
import collections
import functools

import torch

import _ewald_oracle as eo
import _p3m_oracle as po
import ewald_cases as ec
from _memo import memo_oracle

Case = collections.namedtuple("Case", "name reason systems nodes")

SMEARING, SPACING, CUTOFF = ec.SMEARING, ec.RESOLUTION, ec.CUTOFF
PERIODIC, OPEN = ec.PERIODIC, ec.OPEN
QUANTITIES, KINDS = ec.QUANTITIES, ec.KINDS
CHANNELS = (1, 3, 33, 256, 260)

TRICLINIC9 = [[9.0, 0.0, 0.0], [0.7, 8.8, 0.0], [-0.5, 0.6, 9.1]]
ANISOTROPIC = [[9.0, 0.0, 0.0], [3.0, 15.0, 0.0], [1.0, 1.0, 4.5]]  # mesh 8 x 16 x 4 at spacing 1.33, sheared
ON_NODES_CELL = 8.0  # cubic, mesh 8^3: mesh spacing exactly 1, every coordinate below exact in fp32
ON_NODES = [[1.0, 2.0, 3.0],    # on a mesh point (the floor boundary of even p)
            [2.5, 3.5, 4.5],    # half-way between mesh points (the floor boundary of odd p)
            [0.0, 4.0, 6.5],    # on the face x = 0
            [8.0, 1.0, 5.0],    # on the face x = L, unwrapped
            [5.0, 5.5, 0.0],
            [6.5, 7.0, 7.5]]
BINS_CELL = 12.0  # cubic, mesh 16^3, mesh spacing 0.75
BINS_NODE = (5, 9, 3)


def _f32(systems):
    return [(p.float().double(), c, pbc) for p, c, pbc in systems]


def _cubic(length):
    return torch.eye(3, dtype=torch.float64) * float(length)


def nodes20():
    return [ec.periodic_box(20, torch.tensor(TRICLINIC9, dtype=torch.float64), 20)]


def small_mesh():
    return [ec.periodic_box(2, _cubic(ec.SMALL_CELL), 2), eo.mixed_batch(CUTOFF)[0]]


def on_nodes():
    return [(torch.tensor(ON_NODES, dtype=torch.float64), _cubic(ON_NODES_CELL), PERIODIC)]


def anisotropic():
    cell = torch.tensor(ANISOTROPIC, dtype=torch.float64)
    pos, _, _ = ec.periodic_box(30, cell, 30)
    return [(pos, cell, PERIODIC), (pos, cell[[1, 0, 2]].clone(), PERIODIC)]


def bins():
    """33 atoms on a 4 x 4 x 3 lattice of pitch 0.15 mesh units (0.11 A) inside the lower half of one mesh cell (one stencil
    origin for p = 5 and for p = 4), the rest of the 12 A box empty."""
    h = BINS_CELL / 16.0
    offs = torch.tensor([0.02, 0.17, 0.32, 0.47], dtype=torch.float64)
    grid = torch.cartesian_prod(offs, offs, offs[:3])[:33]
    pos = (torch.tensor(BINS_NODE, dtype=torch.float64) + grid) * h
    return [(pos, _cubic(BINS_CELL), PERIODIC)]


def mixed():
    one, tri, _, cluster = eo.mixed_batch(CUTOFF)
    empty = (torch.zeros(0, 3, dtype=torch.float64), _cubic(9.0), PERIODIC)
    return [tri, empty, cluster, one]


@functools.lru_cache(maxsize=None)
def case(name):
    make = {
        "nodes": lambda: Case("nodes", "odd and even node placement, every order", nodes20(), (1, 2, 3, 4, 5)),
        "small_mesh": lambda: Case("small_mesh", "N = 4 < p = 5: nodes fold onto one mesh point; a 1-atom cell", small_mesh(), (5,)),
        "on_nodes": lambda: Case("on_nodes", "atoms on mesh points, half-way between them and on a cell face", on_nodes(), (5, 4)),
        "anisotropic": lambda: Case("anisotropic", "mesh 8 x 16 x 4, sheared, and its left-handed mirror", anisotropic(), (5,)),
        "unwrapped": lambda: Case("unwrapped", "wrapped weights against the unwrapped s_i of dL/dcell", ec.unwrapped(), (5,)),
        "bins": lambda: Case("bins", "a bin of 33 atoms next to empty bins", bins(), (5, 4)),
        "mixed": lambda: Case("mixed", "periodic 43, EMPTY periodic, open 17, periodic 1 in one batch", mixed(), (5,)),
        "channels": lambda: Case("channels", "scalar and 16-byte loads, more than one channel block", [ec.triclinic43()], (5,)),
        "supercell": lambda: Case("supercell", "a cell and its 2 x 1 x 1 supercell on commensurate meshes", ec.supercell(), (5,)),
    }[name]()
    return make._replace(systems=_f32(make.systems))


OPERATOR_CASES = ("nodes", "small_mesh", "on_nodes", "anisotropic", "unwrapped", "bins", "mixed", "supercell")
ALL_CASES = OPERATOR_CASES + ("channels",)
EXPECTED_MESHES = {
    "nodes": [[8, 8, 8]],
    "small_mesh": [[4, 4, 4], [8, 8, 8]],
    "on_nodes": [[8, 8, 8]],
    "anisotropic": [[8, 16, 4], [16, 8, 4]],
    "unwrapped": [[8, 8, 8]],
    "bins": [[16, 16, 16]],
    "mixed": [[8, 8, 8], [0, 0, 0], [0, 0, 0], [8, 8, 8]],
    "channels": [[8, 8, 8]],
    "supercell": [[8, 8, 8], [16, 8, 8]],
}


@functools.lru_cache(maxsize=None)
def batch(name):
    return eo.collate(case(name).systems, CUTOFF)


def meshes(name):
    """The mesh of every system of a case; zeros for an open or empty one."""
    out = []
    for pos, cell, pbc in case(name).systems:
        out.append(po.mesh_shape(cell, SPACING) if all(pbc) and len(pos) else [0, 0, 0])
    return out


@functools.lru_cache(maxsize=None)
def charges(name, channels):
    """Seeded ``(charges, dL/dV)`` fp64 ``[N, C]``; ``supercell``: both halves of the doubled cell repeat the primitive rows."""
    n = batch(name)["positions"].shape[0]
    g = torch.Generator().manual_seed(29 + channels)
    if name == "supercell":
        n = n // 3
    q = torch.randn(n, channels, generator=g, dtype=torch.float64)
    gv = torch.randn(n, channels, generator=g, dtype=torch.float64)
    if name == "supercell":
        q, gv = torch.cat([q] * 3), torch.cat([gv] * 3)
    return q, gv


@memo_oracle
def _reference(b, q, gv, nodes, dtype):
    return po.operator_reference(b, q, gv, SMEARING, SPACING, CUTOFF, nodes, dtype)


def reference(name, channels, nodes, dtype):
    q, gv = charges(name, channels)
    return _reference(batch(name), q, gv, nodes, dtype)


# ---- the device side ------------------------------------------------------------------------------------------------------
def lr_hypers(nodes=5, use_ewald=False, **extra):
    h = ec.lr_hypers(SMEARING, SPACING, **extra)
    h["long_range"].update(use_ewald=use_ewald, interpolation_nodes=nodes)
    return h


def operator(b, dev, nodes=5):
    from metatrain_amd import long_range as lr

    model, g = ec.graph(b, dev)
    op = lr.P3MHip(SMEARING, SPACING, CUTOFF, nodes).plan(b["cells"], b["pbcs"], b["first_atom"])
    return model, g, op
