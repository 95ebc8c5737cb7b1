"""Second derivatives of the ZBL restatement ``tests/zbl_ref.py`` by torch's double backward, for the ZBL Hessian-vector
tests: with ``a_i`` the per-atom energies and ``E_lambda = sum_i lambda_i a_i``,

    g_R, g_cell = grad(E_lambda, [R, cell], create_graph=True)
    hvp_positions, hvp_cells, tangent_atomic = grad(<g_R, u> + <g_cell, u_cell>, [R, cell, lambda])

in fp64 (the reference the fixtures ``zbl_hvp_<case>.npz`` pin to 1e-11, ``golden/make_golden_zbl_hvp.py``) or with the
geometry in fp32 (the yardstick ``y`` of the fp32-floor bar ``max(1e-5, 2 y)``)."""
import functools
import os

import numpy as np
import torch

import zbl_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["box_a", "box_a_sheared", "box_b", "one_atom", "qm9_compressed"]


@functools.lru_cache(maxsize=None)
def fixture(name):
    """The inputs ``zbl_<name>.npz`` and the direction and results ``zbl_hvp_<name>.npz`` as one dict of fp64 / int64 tensors."""
    f = dict(np.load(os.path.join(GOLD, f"zbl_{name}.npz")))
    f.update(np.load(os.path.join(GOLD, f"zbl_hvp_{name}.npz")))
    return {k: torch.tensor(v) for k, v in f.items()}


def atomic_energies(pos, cells, sysidx, numbers, radii_of, pairs):
    """``zbl_ref.atomic_energies`` in the dtype of ``pos`` (``pair_energy`` promotes to fp64: its result is cast back)."""
    pairs = pairs.long()
    i, j, S = pairs[:, 0], pairs[:, 1], pairs[:, 2:5].to(pos.dtype)
    D = pos[j] - pos[i] + torch.einsum("ea,eab->eb", S, cells[sysidx[i]])
    r = torch.sqrt((D * D).sum(1))
    e = zbl_ref.pair_energy(numbers[i], numbers[j], radii_of[numbers[i]], radii_of[numbers[j]], r).to(pos.dtype)
    return torch.zeros(pos.shape[0], dtype=pos.dtype).index_add(0, i, e)


def gradient(pos, cells, sysidx, numbers, radii_of, pairs, lam):
    """(dE_lambda/dR, dE_lambda/dcell), fp64."""
    p, c = pos.double().clone().requires_grad_(True), cells.double().clone().requires_grad_(True)
    a = atomic_energies(p, c, sysidx, numbers, radii_of, pairs)
    gp, gc = torch.autograd.grad((lam.double() * a).sum(), [p, c], allow_unused=True)
    return gp, torch.zeros_like(c) if gc is None else gc


def double_backward(pos, cells, sysidx, numbers, radii_of, pairs, u, u_cell, lam, dtype=torch.float64):
    """(hvp_positions [N,3], hvp_cells [S,3,3], tangent_atomic [N]) as fp64 tensors, evaluated in ``dtype``."""
    p, c = pos.to(dtype).clone().requires_grad_(True), cells.to(dtype).clone().requires_grad_(True)
    w = lam.to(dtype).clone().requires_grad_(True)
    a = atomic_energies(p, c, sysidx, numbers, radii_of, pairs)
    gp, gc = torch.autograd.grad((w * a).sum(), [p, c], create_graph=True)
    hp, hc, tan = torch.autograd.grad((gp * u.to(dtype)).sum() + (gc * u_cell.to(dtype)).sum(), [p, c, w], allow_unused=True)
    hc = torch.zeros_like(c) if hc is None else hc
    return hp.double(), hc.double(), tan.double()


def of_fixture(name, u=None, u_cell=None, lam=None, dtype=torch.float64):
    """``double_backward`` on the inputs of a fixture, along its own direction and weights unless others are given."""
    f = fixture(name)
    return double_backward(f["positions"], f["cells"], f["system_indices"].long(), f["numbers"].long(), f["radii_table"],
                           f["pairs"], f["u"] if u is None else u, f["u_cell"] if u_cell is None else u_cell,
                           f["lambda"] if lam is None else lam, dtype)


def relmax(got, ref, what=""):
    """max|got - ref| / max|ref|; an all-zero reference must be met exactly (the absolute error is returned)."""
    got = torch.as_tensor(got).detach().cpu().double()
    ref = torch.as_tensor(ref).detach().cpu().double()
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    out = err / scale if scale > 0 else err
    if what:
        print(f"    relmax {what}: {out:.3e} (scale {scale:.4g})")
    return out


def bar(y):
    """The project's Hessian bar: the fp32 floor ``max(1e-5, 2 y)``; an input only pins something if ``y <= 1e-3``."""
    assert y <= 1e-3, f"fp32 yardstick {y:.2e}: this input pins nothing"
    return max(1e-5, 2.0 * y)
