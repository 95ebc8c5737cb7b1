"""Premises of the second-order long-range tests that need no GPU: the oracle of ``tests/_ewald_second_oracle.py`` is what it
says (finite differences, symmetry of the Hessian), the two ``pet_ewald_second*`` symbols exist and refuse on the host what
they document, and the Python entry points refuse P3M and CPU tensors before any device call."""
import ctypes
import os
import re

import pytest
import torch

import _ewald_oracle as eo
import _ewald_second_oracle as so
import ewald_cases as ec
from metatrain_amd import _lib
from metatrain_amd import long_range as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_STEP = 1e-4
FD_BOUND = 1.2e-7


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from metatrain_amd import build

        build.build(verbose=False)
    return _lib.load()


def _psi(b, c, q, gv, u_q, u_r):
    _, gq, gpos, _ = eo.operator_reference(b, q, gv, c.smearing, c.resolution, c.cutoff, torch.float64)
    return float((u_q * gq).sum() + (u_r * gpos).sum())


def test_oracle_agrees_with_finite_differences_of_the_adjoint():
    """``sheared`` at C = 3, fp64: central differences of ``operator_reference``'s ``(gq, gpos)`` along one seeded direction each
    of ``q``, ``g`` and ``pos``, contracted with ``(u_q, u_r)`` as in Psi, against ``<out, direction>`` of ``second_reference``.
    Step 1e-4 (A for positions; Psi is linear in q and in g, where the step does not matter). Measured relative
    disagreement: 1.0e-11 (q), 1.9e-13 (g: both the cancellation of the difference quotient), 1.2e-8 (pos: the O(h^2) term
    of the central difference); asserted: 1.2e-7, a decade above the largest."""
    name, channels = "sheared", 3
    c, b = ec.case(name), ec.batch(name)
    q, gv = ec.charges(name, channels)
    u_q, u_r = so.cotangents(name, channels)
    out = so.reference(name, channels, torch.float64)
    g = torch.Generator().manual_seed(99)
    for k, (label, base) in enumerate((("q", q), ("g", gv), ("pos", b["positions"]))):
        step = torch.randn(base.shape, generator=g, dtype=torch.float64)
        sides = []
        for sign in (1.0, -1.0):
            moved = base + sign * FD_STEP * step
            bb = dict(b, positions=moved) if label == "pos" else b
            sides.append(_psi(bb, c, moved if label == "q" else q, moved if label == "g" else gv, u_q, u_r))
        fd = (sides[0] - sides[1]) / (2.0 * FD_STEP)
        want = float((out[k] * step).sum())
        rel = abs(fd - want) / abs(want)
        print(f"(fd along {label}: {fd:.12e} against {want:.12e}, relative {rel:.1e})")
        assert rel <= FD_BOUND, (label, rel)


def test_position_hessian_of_the_oracle_is_symmetric():
    """``<u2, H u1> = <u1, H u2>`` with ``H u = out_positions`` at ``u_q = None``, on ``sheared`` at C = 3 in fp64."""
    name, channels = "sheared", 3
    c, b = ec.case(name), ec.batch(name)
    q, gv = ec.charges(name, channels)
    g = torch.Generator().manual_seed(7)
    u1, u2 = (torch.randn(b["positions"].shape, generator=g, dtype=torch.float64) for _ in range(2))
    h1 = so.second_reference(b, q, gv, None, u1, c.smearing, c.resolution, c.cutoff, torch.float64)[2]
    h2 = so.second_reference(b, q, gv, None, u2, c.smearing, c.resolution, c.cutoff, torch.float64)[2]
    a, d = float((u2 * h1).sum()), float((u1 * h2).sum())
    print(f"(<u2, H u1> {a:.12e}, <u1, H u2> {d:.12e})")
    assert abs(a - d) <= 1e-11 * max(abs(a), abs(d))


def test_oracle_vanishes_on_a_one_atom_cell():
    """A single atom in a periodic cell: nothing depends on its position, so only ``out_grad_potential = A u_q`` survives."""
    one = [eo.mixed_batch(ec.CUTOFF)[0]]
    b = eo.collate(one, ec.CUTOFF)
    g = torch.Generator().manual_seed(3)
    q, gv, u_q = (torch.randn(1, 3, generator=g, dtype=torch.float64) for _ in range(3))
    u_r = torch.randn(1, 3, generator=g, dtype=torch.float64)
    out = so.second_reference(b, q, gv, u_q, u_r, ec.SMEARING, ec.RESOLUTION, ec.CUTOFF, torch.float64)
    tiny = 1e-15 * float(out[1].abs().max())  # (rounding residue of the k-space sines: 5e-18 measured)
    assert float(out[0].abs().max()) <= tiny and float(out[2].abs().max()) <= tiny
    v = eo.operator_reference(b, u_q, gv, ec.SMEARING, ec.RESOLUTION, ec.CUTOFF, torch.float64)[0]
    assert torch.allclose(out[1], v, rtol=1e-13, atol=0.0)


def test_second_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "pet_hip.h")).read()
    for name in ("pet_ewald_second_workspace_bytes", "pet_ewald_second"):
        assert re.search(r"\b" + name + r"\s*\(const pet_ewald_t\* e", header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_second_workspace_bytes_refuses_on_the_host(lib):
    """-1 for a handle without a plan, for one in P3M mode (``pet_ewald_set_p3m``) and for ``n_channels < 1``; none of these
    touches a device."""
    plain, mesh = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.pet_ewald_create(1.4, 1.33, 4.5, ctypes.byref(plain)))
    _lib.check(lib.pet_ewald_create(1.4, 1.33, 4.5, ctypes.byref(mesh)))
    _lib.check(lib.pet_ewald_set_p3m(mesh, 5))
    try:
        assert lib.pet_ewald_second_workspace_bytes(plain, 8) == -1
        assert lib.pet_ewald_second_workspace_bytes(mesh, 8) == -1
        assert lib.pet_ewald_second_workspace_bytes(plain, 0) == -1
        assert lib.pet_ewald_second_workspace_bytes(None, 8) == -1
    finally:
        lib.pet_ewald_destroy(plain)
        lib.pet_ewald_destroy(mesh)


def test_p3m_second_is_refused_before_any_device_call():
    op = lr.P3MHip(1.4, 1.33, 4.5, 5)
    x = torch.zeros(2, 3)
    with pytest.raises(_lib.PetHipError, match="second derivatives through P3M are not built.*trains.*Ewald"):
        op.second(None, x, x, x, u_positions=x)


def test_second_rejects_cpu_tensors_and_two_missing_cotangents():
    op = lr.EwaldHip(1.4, 1.33, 4.5)
    x = torch.zeros(2, 3)
    with pytest.raises(_lib.PetHipError, match="no CPU path"):
        op.second(None, x, x, x, u_charges=x)
    with pytest.raises(_lib.PetHipError, match="both None"):
        op.second(None, x, x, x)
