"""CPU tests around the Hessian-vector product (``pet_hessian_vector``, ``metatrain_amd/pet/hessian.py``): the replica
bookkeeping of ``hessian()`` against a fake batched HVP built from a known dense matrix, the self-consistency of the fp64
oracle that the GPU tests use as their yardstick (its HVP against central differences of its own gradient, and its
symmetry, for both cutoff functions), and the two new C-ABI symbols. No GPU call anywhere."""
import os

import numpy as np
import pytest
import torch

from metatrain_amd import _lib
from metatrain_amd.pet import hessian as H
from oracle import nl as onl
from oracle import pet as opet

TYPES = [1, 6, 7, 8]


def _fake_hvp(dense, calls):
    def hvp(u):  # u [K, n, 3] -> H u per replica
        calls.append(int(u.shape[0]))
        k = u.shape[0]
        return (u.reshape(k, -1).double() @ dense.T).float().reshape(u.shape)

    return hvp


@pytest.mark.parametrize("n_atoms,atoms,k", [(5, None, 4), (5, None, 1), (5, [3, 0], 4), (4, None, 12), (4, None, 5), (3, [], 2)])
def test_replica_bookkeeping_reproduces_a_known_matrix(n_atoms, atoms, k):
    """Every row of the block is asked for exactly once, on the replica and in the launch ``replica_plan`` says, whatever
    the launch width: wider than the block, not a divisor of its row count, one column at a time, a subset of atoms in
    the caller's order, no atom at all."""
    a = torch.randn(3 * n_atoms, 3 * n_atoms, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    dense = a + a.T
    atoms_l = list(range(n_atoms)) if atoms is None else atoms
    calls = []
    got = H.hessian_from_hvp(_fake_hvp(dense, calls), n_atoms, atoms_l, k)
    rows = [3 * i + c for i in atoms_l for c in range(3)]
    assert got.shape == (len(rows), 3 * n_atoms)
    assert torch.equal(got, dense[rows].float())
    plan = H.replica_plan(n_atoms, atoms_l, k)
    assert [r for launch in plan for r in launch] == rows
    assert calls == [len(launch) for launch in plan] and all(1 <= c <= k for c in calls)
    assert len(calls) == -(-len(rows) // k)


def test_replica_plan_rejects_bad_arguments():
    with pytest.raises(ValueError):
        H.replica_plan(4, [0, 4], 2)
    with pytest.raises(ValueError):
        H.replica_plan(4, [0], 0)


def test_a_model_with_a_zbl_term_is_refused():
    class M:
        hypers = {"zbl": True}

    with pytest.raises(_lib.PetHipError, match="ZBL"):
        H.hessian(M(), (torch.zeros(2, 3), torch.tensor([1, 1]), torch.zeros(3, 3), [False] * 3))


def _oracle_grad_fn(hypers, inp, params):
    p64 = {k: (v if k == "species_to_species_index" else v.double()) for k, v in params.items()}

    def energy(pos, cells):
        return opet.pet_atomic_energies(p64, hypers, pos, cells, inp["centers"], inp["neighbors"], inp["cell_shifts"],
                                        inp["species"], inp["system_indices"].long(), "energy")[:, 0].sum()

    return energy


@pytest.mark.parametrize("cutoff_function", ["Bump", "Cosine"])
def test_oracle_hvp_is_symmetric_and_matches_central_differences(golden_dir, cutoff_function):
    """The yardstick of the GPU tests: ``grad(E, R, create_graph=True)`` then ``grad(<g, u>, [R, cells])`` of the fp64
    oracle. ``w^T H u = u^T H w`` to rounding (1e-12 relative), and ``H u`` equals the central difference of the oracle's
    own gradient at ``h = 1e-5`` to 1e-6 of ``max|H u|`` (truncation ``h^2 |d3 g| / 6`` ~ 1e-10 relative, rounding
    ``eps |g| / h`` ~ 1e-11 absolute: both far inside). A small model on the first QM9 molecule keeps it to a second."""
    g = dict(np.load(os.path.join(golden_dir, "qm9_first5.npz")))
    pos, z = torch.tensor(g["pos0"]), torch.tensor(g["z0"])
    n = len(z)
    cell = np.zeros((3, 3))
    i, j, s, _ = onl.neighbor_list(pos.numpy(), cell, [False] * 3, opet.DEFAULT_HYPERS["cutoff"])
    inp = {"positions": pos, "cells": torch.zeros(1, 3, 3, dtype=torch.float64), "centers": torch.tensor(i).long(),
           "neighbors": torch.tensor(j).long(), "cell_shifts": torch.tensor(s).long(), "species": z,
           "system_indices": torch.zeros(n, dtype=torch.long)}
    assert len(i) == n * (n - 1)
    hypers = dict(opet.DEFAULT_HYPERS, d_pet=32, d_node=32, d_feedforward=48, d_head=24, num_heads=2,
                  cutoff_function=cutoff_function)
    params = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    energy = _oracle_grad_fn(hypers, inp, params)
    gen = torch.Generator().manual_seed(1)
    u = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    w = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    cells = inp["cells"]

    def grad(pos):
        pos = pos.clone().requires_grad_(True)
        (gr,) = torch.autograd.grad(energy(pos, cells), pos)
        return gr

    def hvp(vec):
        pos = inp["positions"].clone().requires_grad_(True)
        (gr,) = torch.autograd.grad(energy(pos, cells), pos, create_graph=True)
        (hv,) = torch.autograd.grad((gr * vec).sum(), pos)
        return hv

    hu, hw = hvp(u), hvp(w)
    assert float(hu.abs().max()) > 0
    lhs, rhs = float((w * hu).sum()), float((u * hw).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    h = 1e-5
    fd = (grad(inp["positions"] + h * u) - grad(inp["positions"] - h * u)) / (2 * h)
    assert float((fd - hu).abs().max() / hu.abs().max()) < 1e-6


def test_the_two_symbols_are_declared_and_bound():
    """(``tests/test_abi_cpu.py`` checks that the header's declarations, ``_lib.SYMBOLS`` and the library's exports are one
    set; this pins the two names and their prototypes.)"""
    assert {"pet_hvp_workspace_bytes_for", "pet_hessian_vector"} <= set(_lib.SYMBOLS)
    lib = _lib.load()
    assert lib.pet_hvp_workspace_bytes_for.restype is _lib.c_int64
    assert len(lib.pet_hessian_vector.argtypes) == 11
    assert lib.pet_hvp_workspace_bytes_for(None, None) == -1
    assert lib.pet_hessian_vector(None, None, None, 0, None, None, None, None, None, None, None) == _lib.PET_ERR_ARGUMENT
