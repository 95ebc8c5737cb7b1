"""The fp64 oracle of the MESH operator's second-order operation (``pet_p3m_second``; ``include/pet_hip.h``, DESIGN.md section
22): ``_ewald_second_oracle.second_reference`` -- torch's double backward -- with ``_p3m_oracle.potential_batch`` in place of
the Ewald definition, on the cases of ``tests/p3m_cases.py``. The B-spline weights of ``_p3m_oracle`` are differentiable
polynomials of the positions (the stencil's base is detached), so autograd differentiates them twice; ``M_p''`` jumps at a
stencil breakpoint for p <= 3, which the cases run there stay away from (``test_p3m_second_cpu.py``). No GPU import."""
import contextlib

import torch

import _ewald_oracle as eo
import _ewald_second_oracle as so
import _p3m_oracle as po
import p3m_cases as pc
from _memo import memo_oracle

NAMES, KINDS, PARAM_KEYS = so.NAMES, so.KINDS, so.PARAM_KEYS


@contextlib.contextmanager
def mesh_operator(nodes):
    """``_ewald_oracle.potential_batch`` is the P3M definition at ``nodes`` inside the block (the swap of
    ``_p3m_oracle.model_reference``)."""
    ewald = eo.potential_batch

    def p3m(pos, cells, pbcs, first_atom, q, centers, neighbors, shifts, smearing, spacing, cutoff):
        return po.potential_batch(pos, cells, pbcs, first_atom, q, centers, neighbors, shifts, smearing, spacing, cutoff, nodes)

    eo.potential_batch = p3m
    try:
        yield
    finally:
        eo.potential_batch = ewald


def cotangents(name, channels):
    """Seeded ``(u_q [N, C], u_r [N, 3])`` fp64 of a case of ``p3m_cases``; ``supercell``: the doubled cell's rows repeat the
    primitive ones, as its charges do.

    The seed base is chosen on the HOST, by the fp32 oracle's own error alone. On a one-atom cell ``(D_u A) g`` and ``H u``
    vanish for the Ewald sum; a mesh breaks translation invariance, so here they are a residue of 1e-5 .. 1e-4 of the batch's
    scale, which fp32 resolves to 1e-4 .. 1e-2 of ITSELF depending on the draw. Measured yardstick of the one-atom cells at
    C = 24 (``mixed`` / ``small_mesh``) for the bases 4100, 4200, ...: 1.7e-3 / 1.2e-4, 6.7e-3 / 6.8e-4, 9.9e-3 / 2.8e-4,
    3.9e-4 / 3.2e-4 (4400), 2.6e-3 / 1.1e-4, 3.3e-4 / 8.1e-4. 4400 is the first that keeps every GPU run under
    ``gen_shapes.Y_CAP`` (``test_p3m_second_cpu.py`` asserts it for every run)."""
    n = pc.batch(name)["positions"].shape[0]
    if name == "supercell":
        n = n // 3
    g = torch.Generator().manual_seed(4400 + channels)
    u_q, u_r = torch.randn(n, channels, generator=g, dtype=torch.float64), torch.randn(n, 3, generator=g, dtype=torch.float64)
    if name == "supercell":
        u_q, u_r = torch.cat([u_q] * 3), torch.cat([u_r] * 3)
    return u_q, u_r


def second_reference(batch, q, gv, u_q, u_r, nodes, dtype):
    with mesh_operator(nodes):
        return so.second_reference(batch, q, gv, u_q, u_r, pc.SMEARING, pc.SPACING, pc.CUTOFF, dtype)


_second_reference = memo_oracle(second_reference)


def reference(name, channels, nodes, dtype, halves=(True, True)):
    """The oracle on ``pc.charges(name, channels)`` and :func:`cotangents`; ``halves = (with u_q, with u_r)``."""
    q, gv = pc.charges(name, channels)
    u_q, u_r = cotangents(name, channels)
    return _second_reference(pc.batch(name), q, gv, u_q if halves[0] else None, u_r if halves[1] else None, nodes, dtype)


@memo_oracle
def featurizer_reference(batch, params, x, weights, target, nodes, dtype):
    """``_ewald_second_oracle.featurizer_reference`` (the force-matching loss through the featuriser) on the mesh operator."""
    with mesh_operator(nodes):
        return so.featurizer_reference.__wrapped__(batch, params, x, weights, target, pc.SMEARING, pc.SPACING, pc.CUTOFF, dtype)


def stencil_distance(name, nodes):
    """The smallest distance, in mesh units, of any atom's coordinate from a breakpoint of its order-``nodes`` stencil (an
    integer for even p, a half-integer for odd p), over the periodic systems of a case."""
    worst = float("inf")
    for pos, cell, pbc in pc.case(name).systems:
        if not all(pbc) or len(pos) == 0:
            continue
        shape = torch.tensor(po.mesh_shape(cell, pc.SPACING), dtype=torch.float64)
        s = pos @ torch.linalg.inv(cell)
        u = (s - torch.floor(s)) * shape
        x = u + 0.5 if nodes % 2 else u
        worst = min(worst, float((x - torch.round(x)).abs().min()))
    return worst
