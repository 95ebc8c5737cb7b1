"""The fp64 oracle of the long-range operator's SECOND-order operation (``pet_ewald_second``; ``include/pet_hip.h``, DESIGN.md
section 20): torch's double backward through the restated definition of ``tests/_ewald_oracle.py``.

With ``V = potential_batch(pos, q)``, ``(gq, gpos) = d<gv, V>/d(q, pos)`` under ``create_graph`` and seeded cotangents ``u_q`` of
``gq`` and ``u_r`` of ``gpos``, the reference is the gradient of ``Psi = <u_q, gq> + <u_r, gpos>`` with respect to ``(q, gv, pos)``,
in the device's order ``(out_charges, out_grad_potential, out_positions)``. A ``None`` cotangent is a zero one. The featuriser
reference composes ``charges_map``, the operator, ``out_projection`` and the SiLU in torch for the force-matching loss of
``test_gpu_long_range_second.py``. No GPU import."""
import torch

import _ewald_oracle as eo
import ewald_cases as ec
from _memo import memo_oracle

NAMES = ("out_charges", "out_grad_potential", "out_positions")
KINDS = ("atom", "atom", "atom")
PARAM_KEYS = tuple("long_range_featurizer." + k for k in (
    "charges_map.weight", "charges_map.bias", "out_projection.0.weight", "out_projection.0.bias", "out_projection.2.weight",
    "out_projection.2.bias"))


def cotangents(name, channels):
    """Seeded ``(u_q [N, C], u_r [N, 3])`` fp64 of a case of ``ewald_cases``."""
    n = ec.batch(name)["positions"].shape[0]
    g = torch.Generator().manual_seed(4000 + channels)
    return torch.randn(n, channels, generator=g, dtype=torch.float64), torch.randn(n, 3, generator=g, dtype=torch.float64)


def second_reference(batch, q, gv, u_q, u_r, smearing, resolution, cutoff, dtype):
    """``(dPsi/dq, dPsi/dg, dPsi/dpos)`` evaluated in ``dtype``, returned in fp64; ``u_q`` / ``u_r`` ``None``: zero."""
    pos = batch["positions"].to(dtype).clone().requires_grad_(True)
    cells = batch["cells"].to(dtype)
    qq = q.to(dtype).clone().requires_grad_(True)
    gg = gv.to(dtype).clone().requires_grad_(True)
    if pos.shape[0] == 0:
        return tuple(torch.zeros_like(t).double() for t in (qq, gg, pos))
    v = eo.potential_batch(pos, cells, batch["pbcs"], batch["first_atom"], qq, batch["centers"], batch["neighbors"],
                           batch["cell_shifts"], smearing, resolution, cutoff)
    gq, gpos = torch.autograd.grad((gg * v).sum(), [qq, pos], create_graph=True)
    psi = 0.0
    if u_q is not None:
        psi = psi + (u_q.to(dtype) * gq).sum()
    if u_r is not None:
        psi = psi + (u_r.to(dtype) * gpos).sum()
    out = torch.autograd.grad(psi, [qq, gg, pos], allow_unused=True)
    return tuple((torch.zeros_like(x) if o is None else o).detach().double() for o, x in zip(out, (qq, gg, pos)))


_second_reference = memo_oracle(second_reference)


def reference(name, channels, dtype, halves=(True, True)):
    """The oracle on ``ec.charges(name, channels)`` and :func:`cotangents`; ``halves = (with u_q, with u_r)``."""
    c = ec.case(name)
    q, gv = ec.charges(name, channels)
    u_q, u_r = cotangents(name, channels)
    return _second_reference(ec.batch(name), q, gv, u_q if halves[0] else None, u_r if halves[1] else None, c.smearing,
                             c.resolution, c.cutoff, dtype)


# ---- the featuriser under a force-matching loss -----------------------------------------------------------------------------
def featurizer_inputs(batch, d):
    """Seeded ``(x [N, d], W [N, d], F* [N, 3])`` fp64: node features, the weights of the scalar whose position gradient is the
    'force', and the force target."""
    n = batch["positions"].shape[0]
    g = torch.Generator().manual_seed(6000 + d)
    return (torch.randn(n, d, generator=g, dtype=torch.float64), torch.randn(n, d, generator=g, dtype=torch.float64),
            torch.randn(n, 3, generator=g, dtype=torch.float64))


def featurizer_forward(x, pos, cells, batch, p, smearing, resolution, cutoff):
    lin = torch.nn.functional.linear
    pre = "long_range_featurizer."
    q = lin(x, p[pre + "charges_map.weight"], p[pre + "charges_map.bias"])
    v = eo.potential_batch(pos, cells, batch["pbcs"], batch["first_atom"], q, batch["centers"], batch["neighbors"],
                           batch["cell_shifts"], smearing, resolution, cutoff)
    hid = torch.nn.functional.silu(lin(v, p[pre + "out_projection.0.weight"], p[pre + "out_projection.0.bias"]))
    return lin(hid, p[pre + "out_projection.2.weight"], p[pre + "out_projection.2.bias"])


def force_loss(lr, pos, weights, target):
    """``((F - F*)^2).sum() + (lr^2).sum()`` with ``F = d (W . lr).sum() / d pos`` under ``create_graph``."""
    force, = torch.autograd.grad((weights * lr).sum(), pos, create_graph=True)
    return ((force - target) ** 2).sum() + (lr * lr).sum()


@memo_oracle
def featurizer_reference(batch, params, x, weights, target, smearing, resolution, cutoff, dtype):
    """Gradients of :func:`force_loss` with respect to ``x`` and the six featuriser tensors (``PARAM_KEYS`` order), evaluated in
    ``dtype``, returned in fp64."""
    p = {k: params[k].to(dtype).clone().requires_grad_(True) for k in PARAM_KEYS}
    xx = x.to(dtype).clone().requires_grad_(True)
    pos = batch["positions"].to(dtype).clone().requires_grad_(True)
    lr = featurizer_forward(xx, pos, batch["cells"].to(dtype), batch, p, smearing, resolution, cutoff)
    loss = force_loss(lr, pos, weights.to(dtype), target.to(dtype))
    grads = torch.autograd.grad(loss, [xx] + [p[k] for k in PARAM_KEYS])
    return tuple(g.detach().double() for g in grads)
