"""The fp64 oracle of the CELL tangents of the long-range operator's second-order operation and of the long-range training
sweep (``pet_ewald_second_cell`` / ``pet_p3m_second_cell`` / ``pet_backward_train2_long_range_cell``).

Operator level: with ``V = potential_batch(pos, cells, q)`` and ``(gq, gpos, gcell) = d<gv, V>/d(q, pos, cells)`` under
``create_graph`` (``gcell`` at fixed Cartesian positions, the k-index set and the mesh shape fixed: both are integers of the
definition), the reference is the gradient of ``Psi = <u_q, gq> + <u_r, gpos> + <u_c, gcell>`` with respect to ``(q, gv)``, in the
device's order ``(out_charges, out_grad_potential)``. Under ``_p3m_second_oracle.mesh_operator(nodes)`` it is the mesh
operator's. Model level: ``J = <nu, e> + <u, dE/dR> + <u_cell, dE/dcell>``, its gradient per parameter tensor and the per-atom
tangents. Evaluated in fp64 for the reference and in fp32 for the yardstick. No GPU import."""
import functools
import math

import torch

import _ewald_oracle as eo
import _long_range_train_oracle as lo
import _p3m_second_oracle as so2
import ewald_cases as ec
import p3m_cases as pc
from _memo import memo_oracle

NAMES = ("out_charges", "out_grad_potential")
KINDS = ("atom", "atom")


def cell_direction(batch, seed):
    """``u_cell [S, 3, 3] = cell @ U`` with ``U = 0.1 randn`` from a seeded generator; zero rows for open systems."""
    cells = batch["cells"].double()
    g = torch.Generator().manual_seed(seed)
    U = 0.1 * torch.randn(cells.shape[0], 3, 3, generator=g, dtype=torch.float64)
    out = cells @ U
    for s, pbc in enumerate(batch["pbcs"]):
        if not all(pbc):
            out[s] = 0.0
    return out


def cotangents(batch, channels, base=4300):
    """Seeded ``(u_q [N, C], u_r [N, 3], u_c [S, 3, 3])`` fp64."""
    n = batch["positions"].shape[0]
    g = torch.Generator().manual_seed(base + channels)
    return (torch.randn(n, channels, generator=g, dtype=torch.float64), torch.randn(n, 3, generator=g, dtype=torch.float64),
            cell_direction(batch, base + 1000 + channels))


def second_cell_reference(batch, q, gv, u_q, u_r, u_c, smearing, resolution, cutoff, dtype):
    """``(dPsi/dq, dPsi/dg)`` evaluated in ``dtype``, returned in fp64; a ``None`` cotangent is a zero one."""
    pos = batch["positions"].to(dtype).clone().requires_grad_(True)
    cells = batch["cells"].to(dtype).clone().requires_grad_(True)
    qq = q.to(dtype).clone().requires_grad_(True)
    gg = gv.to(dtype).clone().requires_grad_(True)
    v = eo.potential_batch(pos, cells, batch["pbcs"], batch["first_atom"], qq, batch["centers"], batch["neighbors"],
                           batch["cell_shifts"], smearing, resolution, cutoff)
    gq, gpos, gcell = torch.autograd.grad((gg * v).sum(), [qq, pos, cells], create_graph=True, allow_unused=True)
    psi = 0.0
    if u_q is not None:
        psi = psi + (u_q.to(dtype) * gq).sum()
    if u_r is not None:
        psi = psi + (u_r.to(dtype) * gpos).sum()
    if u_c is not None and gcell is not None:
        psi = psi + (u_c.to(dtype) * gcell).sum()
    out = torch.autograd.grad(psi, [qq, gg], allow_unused=True)
    return tuple((torch.zeros_like(x) if o is None else o).detach().double() for o, x in zip(out, (qq, gg)))


_second_cell_reference = memo_oracle(second_cell_reference)


def _parts(cot, parts):
    return tuple(c if keep else None for c, keep in zip(cot, parts))


def reference(name, channels, dtype, parts=(True, True, True)):
    """The Ewald oracle on ``ec.charges(name, channels)`` and :func:`cotangents`; ``parts = (with u_q, with u_r, with u_c)``."""
    c, b = ec.case(name), ec.batch(name)
    q, gv = ec.charges(name, channels)
    return _second_cell_reference(b, q, gv, *_parts(cotangents(b, channels), parts), c.smearing, c.resolution, c.cutoff, dtype)


@memo_oracle
def _mesh_reference(batch, q, gv, u_q, u_r, u_c, nodes, dtype):
    with so2.mesh_operator(nodes):
        return second_cell_reference(batch, q, gv, u_q, u_r, u_c, pc.SMEARING, pc.SPACING, pc.CUTOFF, dtype)


def mesh_reference(name, channels, nodes, dtype, parts=(True, True, True)):
    """The same through the mesh operator, on the cases of ``p3m_cases``."""
    b = pc.batch(name)
    q, gv = pc.charges(name, channels)
    return _mesh_reference(b, q, gv, *_parts(cotangents(b, channels, 4400), parts), nodes, dtype)


# ---- the closed form of DESIGN.md section 23, for one periodic system ---------------------------------------------------------
def closed_form(pos, cell, x, edges, u, u_c, smearing, resolution, cutoff):
    """``(D A) X`` along ``(u, u_c)`` of ``_ewald_oracle.potential_periodic`` by the closed form: the position tangent at
    ``u' = u - r U`` of the k-space sum (k fixed), the weights' tangent, the background and the exclusion rows with
    ``dD = u_j - u_i + S u_c``."""
    inv = torch.linalg.inv(cell)
    U = inv @ u_c
    up = u - pos @ U
    n = eo.kvector_indices(cell, resolution).to(pos.dtype)
    k = n @ (2.0 * math.pi * inv.T)
    k2 = (k * k).sum(1)
    vol = torch.det(cell).abs()
    w = 4.0 * math.pi * torch.exp(-0.5 * smearing ** 2 * k2) / k2 / vol
    ph = k @ pos.T
    c, s = torch.cos(ph), torch.sin(ph)
    ku = k @ up.T                                   # [K, N]
    # d/dt of c_i (c.X) + s_i (s.X) with every phase moving by k.u'
    dc, ds = -s * ku, c * ku
    tangent = dc.T @ (w[:, None] * (c @ x)) + c.T @ (w[:, None] * (dc @ x)) + ds.T @ (w[:, None] * (s @ x)) + s.T @ (w[:, None] * (ds @ x))
    f = (smearing ** 2 + 2.0 / k2) * torch.einsum("ka,ab,kb->k", k, U, k) - torch.trace(U)
    weights = c.T @ ((w * f)[:, None] * (c @ x)) + s.T @ ((w * f)[:, None] * (s @ x))
    background = (2.0 * math.pi * smearing ** 2 / vol) * torch.trace(U) * x.sum(0, keepdim=True)
    i, j, S = edges
    D = pos[j] - pos[i] + S.to(pos.dtype) @ cell
    d = torch.linalg.norm(D, dim=1).clone().requires_grad_(True)
    wd = torch.erf(d / (math.sqrt(2.0) * smearing)) / d * eo.cutoff_f(d, cutoff)
    (dw,) = torch.autograd.grad(wd.sum(), d)
    dD = u[j] - u[i] + S.to(pos.dtype) @ u_c
    co = dw * ((D / d.detach()[:, None]) * dD).sum(1)
    exclusion = torch.zeros_like(x).index_add(0, i, co[:, None] * x[j])
    return eo.PREFACTOR * (tangent + weights + background - exclusion)


# ---- the model-level reference ------------------------------------------------------------------------------------------------
def two_cells():
    """Two different cells around an open system: the sheared cell of ``ewald_cases``, three open atoms without an edge and a
    32-atom cubic box; species from generator 4200. A per-system ``U`` indexed wrongly cannot pass it."""
    tri, _ = lo.three_atoms()
    systems = [ec.sheared()[0], tri, ec.periodic_box(32, ec._cubic(9.0), 32)]
    b = eo.collate(systems, lo.CUTOFF)
    n = b["positions"].shape[0]
    g = torch.Generator().manual_seed(4200)
    b["species"] = torch.tensor(eo.TYPES, dtype=torch.int32)[torch.randint(0, 4, (n,), generator=g)]
    return b


@functools.lru_cache(maxsize=None)
def batch_of(which):
    return two_cells() if which == "two_cells" else lo.batch_of(which)


@functools.lru_cache(maxsize=None)
def seeds(which):
    """``(nu, u, u_cell)``: ``nu`` uniform in [-0.5, 0.5], ``u`` random normal, ``u_cell = cell @ U``."""
    b = batch_of(which)
    n = b["positions"].shape[0]
    g = torch.Generator().manual_seed(4500)
    return (torch.rand(n, generator=g, dtype=torch.float64) - 0.5, torch.randn(n, 3, generator=g, dtype=torch.float64),
            cell_direction(b, 4501))


def evaluate_cell(params, hypers, batch, nu, u, u_cell, dtype):
    """One evaluation in ``dtype``, everything in fp64: ``atomic`` (e), ``grad`` (dE/dR), ``cell_grad`` (dE/dcell at fixed
    Cartesian positions), ``grads`` (dJ/dtheta per tensor, ``J = <nu, e> + <u, dE/dR> + <u_cell, dE/dcell>``; a ``None``
    direction is zero) and ``tangent`` (the per-atom tangents e' along ``(u, u_cell)``)."""
    p = lo.leaves_of(params, dtype)
    keys = [k for k in p if k != "species_to_species_index"]
    pos = batch["positions"].to(dtype).clone().requires_grad_(True)
    cells = batch["cells"].to(dtype).clone().requires_grad_(True)
    ones = torch.ones(pos.shape[0], dtype=dtype, requires_grad=True)
    e = lo.atomic_energies(p, hypers, batch, pos, cells)
    g, gc = torch.autograd.grad((ones * e).sum(), [pos, cells], create_graph=True)
    phi = 0.0
    if u is not None:
        phi = phi + (u.to(dtype) * g).sum()
    if u_cell is not None:
        phi = phi + (u_cell.to(dtype) * gc).sum()
    tangent = torch.zeros_like(ones)
    if u is not None or u_cell is not None:
        (tangent,) = torch.autograd.grad(phi, ones, retain_graph=True)
    J = (nu.to(dtype) * e).sum() + phi
    grads = torch.autograd.grad(J, [p[k] for k in keys], allow_unused=True)
    return {"atomic": e.detach().double(), "grad": g.detach().double(), "cell_grad": gc.detach().double(),
            "tangent": tangent.detach().double(),
            "grads": {k: (torch.zeros_like(p[k]) if gr is None else gr).detach().double() for k, gr in zip(keys, grads)}}


@functools.lru_cache(maxsize=None)
def reference_model(tag, which, nodes=0, with_u=True, with_cell=True):
    """(fp64 evaluation, fp32 evaluation) of a model case; ``nodes > 0``: through the mesh operator of that order."""
    hypers, params = lo.model_case(tag)
    nu, u, uc = seeds(which)
    b = batch_of(which)
    args = (params, hypers, b, nu, u if with_u else None, uc if with_cell else None)
    if nodes:
        with so2.mesh_operator(nodes):
            return evaluate_cell(*args, torch.float64), evaluate_cell(*args, torch.float32)
    return evaluate_cell(*args, torch.float64), evaluate_cell(*args, torch.float32)
