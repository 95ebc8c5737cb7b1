"""Fixtures of the ZBL Hessian-vector tests -> ``zbl_hvp_<case>.npz``, from the reference's own ``ZBL.get_pairwise_zbl``
differentiated twice by torch in fp64, on the inputs of the five ``zbl_<case>.npz`` fixtures (``make_golden_zbl.py``, which
this script imports for the way it loads the reference and makes a ``ZBL`` object).

With ``a_i`` the per-atom energies, ``E_lambda = sum_i lambda_i a_i`` and a direction ``(u [N,3], u_cell [S,3,3])``:

    g_R, g_cell = grad(E_lambda, [R, cell], create_graph=True)
    hvp_positions, hvp_cells, tangent_atomic = grad(<g_R, u> + <g_cell, u_cell>, [R, cell, lambda])

Each file: u ~ N(0, 1), u_cell ~ 0.1 N(0, 1), lambda uniform in [0.5, 1.5] (one seeded generator per case) and the three
results. The restatement the tests use (``tests/zbl_ref.py``), differentiated the same way, must agree to 1e-11 relative.

    python tests/golden/make_golden_zbl_hvp.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_zbl as mg  # noqa: E402
import zbl_ref  # noqa: E402

CASES = ["box_a", "box_a_sheared", "box_b", "one_atom", "qm9_compressed"]
SEED = 3


def direction(n_atoms, n_systems, seed=SEED):
    """(u, u_cell, lambda) of a case, fp64."""
    gen = torch.Generator().manual_seed(seed)
    u = torch.randn(n_atoms, 3, generator=gen, dtype=torch.float64)
    u_cell = 0.1 * torch.randn(n_systems, 3, 3, generator=gen, dtype=torch.float64)
    lam = 0.5 + torch.rand(n_atoms, generator=gen, dtype=torch.float64)
    return u, u_cell, lam


def double_backward(pair_energy, positions, cells, system_indices, pairs, u, u_cell, lam):
    """(hvp_positions, hvp_cells, tangent_atomic) for ``pair_energy(i, j, r) -> e [E]``."""
    i, j, S = pairs[:, 0].long(), pairs[:, 1].long(), pairs[:, 2:5].to(positions.dtype)
    pos = positions.clone().requires_grad_(True)
    cel = cells.clone().requires_grad_(True)
    w = lam.clone().requires_grad_(True)
    D = pos[j] - pos[i] + torch.einsum("ea,eab->eb", S, cel[system_indices[i]])
    r = torch.sqrt((D * D).sum(1))
    atomic = torch.zeros(positions.shape[0], dtype=positions.dtype).index_add(0, i, pair_energy(i, j, r))
    g_pos, g_cell = torch.autograd.grad((w * atomic).sum(), [pos, cel], create_graph=True)
    hp, hc, tan = torch.autograd.grad((g_pos * u).sum() + (g_cell * u_cell).sum(), [pos, cel, w], allow_unused=True)
    return hp, torch.zeros_like(cells) if hc is None else hc, tan


def main():
    torch.set_default_dtype(torch.float64)
    ZBL = mg.import_reference_zbl()
    radii = torch.tensor(mg.RADII)
    for name in CASES:
        f = dict(np.load(os.path.join(HERE, f"zbl_{name}.npz")))
        pos, cells = torch.tensor(f["positions"]), torch.tensor(f["cells"])
        numbers, sysidx = torch.tensor(f["numbers"]).long(), torch.tensor(f["system_indices"]).long()
        pairs = torch.tensor(f["pairs"])
        model = mg.reference_model(ZBL, [int(t) for t in f["atomic_types"]])
        u, u_cell, lam = direction(pos.shape[0], cells.shape[0])
        ref = double_backward(lambda i, j, r: model.get_pairwise_zbl(numbers[i], numbers[j], r), pos, cells, sysidx, pairs,
                              u, u_cell, lam)
        mine = double_backward(lambda i, j, r: zbl_ref.pair_energy(numbers[i], numbers[j], radii[numbers[i]],
                                                                   radii[numbers[j]], r), pos, cells, sysidx, pairs,
                               u, u_cell, lam)
        for what, a, b in zip(("hvp_positions", "hvp_cells", "tangent_atomic"), mine, ref):
            scale = float(b.abs().max())  # (an all-zero result must be met exactly)
            assert float((a - b).abs().max()) <= 1e-11 * scale, (name, what, float((a - b).abs().max()), scale)
        print(f"{name}: max|H u| {float(ref[0].abs().max()):.6g}, max|(H u)_cell| {float(ref[1].abs().max()):.6g}, "
              f"max|tangent| {float(ref[2].abs().max()):.6g}")
        np.savez_compressed(os.path.join(HERE, f"zbl_hvp_{name}.npz"), **{
            "u": u.numpy(), "u_cell": u_cell.numpy(), "lambda": lam.numpy(), "hvp_positions": ref[0].numpy(),
            "hvp_cells": ref[1].numpy(), "tangent_atomic": ref[2].numpy()})


if __name__ == "__main__":
    main()
