"""CPU tests around the ZBL Hessian-vector product (``pet_zbl_hessian_vector``, ``ZBLHip.hessian_vector_product``, the
``zbl=`` argument of ``pet/hessian.py::hessian``): the C-ABI symbol, the refusal of a ``zbl: true`` model whose caller does
not say where the term goes, and the self-consistency in fp64 of the yardstick the GPU tests use (``tests/zbl_hvp_ref.py``
on the committed fixtures ``zbl_hvp_<case>.npz``). No GPU call anywhere."""
import os
import re

import pytest
import torch

import zbl_hvp_ref as R
import zbl_ref
from metatrain_amd import _lib
from metatrain_amd.pet import hessian as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "pet_hip.h")).read()
    assert re.search(r"\bint pet_zbl_hessian_vector\(const pet_zbl_t\* z, const pet_graph_t\* g,", header)
    assert "pet_zbl_hessian_vector" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "pet_zbl_hessian_vector")  # exported by the library
    assert len(lib.pet_zbl_hessian_vector.argtypes) == 11
    assert lib.pet_zbl_hessian_vector(None, None, None, None, None, None, None, None, None, 0, None) == _lib.PET_ERR_ARGUMENT


def test_a_zbl_model_is_refused_until_the_caller_says_where_the_term_goes():
    class M:
        hypers = {"zbl": True}
        atomic_types = [1]

    system = (torch.zeros(2, 3), torch.tensor([1, 1]), torch.zeros(3, 3), [False] * 3)
    with pytest.raises(_lib.PetHipError, match="ZBL") as err:
        H.hessian(M(), system)
    assert "zbl=" in str(err.value) and "zbl=False" in str(err.value)


@pytest.mark.parametrize("name", R.CASES)
def test_the_fixture_is_the_fp64_double_backward_of_the_restatement(name):
    """What ``make_golden_zbl_hvp.py`` asserted against the reference when it wrote the file: 1e-11 relative."""
    f = R.fixture(name)
    for what, got in zip(("hvp_positions", "hvp_cells", "tangent_atomic"), R.of_fixture(name)):
        scale = float(f[what].abs().max())
        assert float((got - f[what]).abs().max()) <= 1e-11 * scale, (name, what)
    if name == "one_atom":  # six self-image edges depend on no position
        assert float(f["hvp_positions"].abs().max()) == 0.0 and float(f["hvp_cells"].abs().max()) > 0.1
    if name == "qm9_compressed":
        assert float(f["hvp_cells"].abs().max()) == 0.0


@pytest.mark.parametrize("name", R.CASES)
def test_yardstick_is_symmetric_and_matches_central_differences(name):
    """``w^T H u = u^T H w`` over (positions, cells) to rounding (1e-12 relative), and ``H u`` equals the central difference
    of the yardstick's own gradient at ``h = 1e-5`` to 1e-6 of ``max|H u|`` over both blocks -- the bars of
    ``test_hvp_cpu.py``, by the same reasoning: truncation ``h^2 |d3 g| / 6`` and rounding ``eps |g| / h`` are orders of
    magnitude inside it. The third derivative of ``e`` jumps at ``rc``, where the second is zero: a pair that crosses ``rc``
    inside ``+-h`` adds a term of order ``h`` times that jump, as far inside."""
    f = R.fixture(name)
    n, s = f["positions"].shape[0], f["cells"].shape[0]
    gen = torch.Generator().manual_seed(7)
    w = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    w_cell = 0.1 * torch.randn(s, 3, 3, generator=gen, dtype=torch.float64)
    hu, hw = R.of_fixture(name), R.of_fixture(name, w, w_cell)
    lhs = float((w * hu[0]).sum() + (w_cell * hu[1]).sum())
    rhs = float((f["u"] * hw[0]).sum() + (f["u_cell"] * hw[1]).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    h = 1e-5
    args = (f["system_indices"].long(), f["numbers"].long(), f["radii_table"], f["pairs"], f["lambda"])
    plus = R.gradient(f["positions"] + h * f["u"], f["cells"] + h * f["u_cell"], *args)
    minus = R.gradient(f["positions"] - h * f["u"], f["cells"] - h * f["u_cell"], *args)
    scale = max(float(hu[0].abs().max()), float(hu[1].abs().max()))
    for k in range(2):
        assert float(((plus[k] - minus[k]) / (2 * h) - hu[k]).abs().max()) < 1e-6 * scale, (name, k)
    # the tangent is the contracted gradient differentiated w.r.t. the weights: sum_i lambda_i e'_i = <u, g_R> + <u_cell, g_cell>
    g = R.gradient(f["positions"], f["cells"], *args)
    contracted = float((f["u"] * g[0]).sum() + (f["u_cell"] * g[1]).sum())
    assert abs(float((f["lambda"] * hu[2]).sum()) - contracted) <= 1e-12 * max(abs(contracted), float(hu[2].abs().max()))


@pytest.mark.parametrize("name", R.CASES)
def test_second_derivative_of_the_pair_term_is_continuous_through_rc(name):
    """``e''`` just inside and just outside ``rc`` (``rc (1 -+ 1e-9)``) is at most 1e-6 of the largest ``|e''|`` over the
    fixture's pairs: ``A``, ``B``, ``C`` make ``e``, ``e'`` and ``e''`` vanish there, so the product has no jump to resolve."""
    f = R.fixture(name)
    pairs, numbers, radii = f["pairs"].long(), f["numbers"].long(), f["radii_table"]
    zi, zj = numbers[pairs[:, 0]], numbers[pairs[:, 1]]
    pos, cells = f["positions"], f["cells"]
    D = pos[pairs[:, 1]] - pos[pairs[:, 0]] + torch.einsum("ea,eab->eb", pairs[:, 2:5].double(),
                                                          cells[f["system_indices"].long()[pairs[:, 0]]])
    rc = radii[zi] + radii[zj]

    def second(r):
        r = r.clone().requires_grad_(True)
        e = zbl_ref.pair_energy(zi, zj, radii[zi], radii[zj], r)
        (de,) = torch.autograd.grad(e.sum(), r, create_graph=True)
        (d2e,) = torch.autograd.grad(de.sum(), r)
        return d2e

    largest = float(second(torch.sqrt((D * D).sum(1))).abs().max())
    assert largest > 0
    for side in (1 - 1e-9, 1 + 1e-9):
        assert float(second(rc * side).abs().max()) <= 1e-6 * largest, (name, side)
