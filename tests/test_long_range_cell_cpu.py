"""CPU tests of the cell-tangent oracle (``tests/_long_range_cell_oracle.py``), of the closed form the
kernels evaluate, of the seeds a stress loss feeds to the sweep, and of what the new entry points refuse without a GPU."""
import ctypes
import types

import pytest
import torch

import _ewald_oracle as eo
import _long_range_cell_oracle as co
import _long_range_train_oracle as lo
import ewald_cases as ec
from oracle import pet as opet


def _energies(tag, which, h):
    hypers, params = lo.model_case(tag)
    b = co.batch_of(which)
    _, u, uc = co.seeds(which)
    p = {k: (v if k == "species_to_species_index" else v.double()) for k, v in params.items()}
    with torch.no_grad():
        return lo.atomic_energies(p, hypers, b, b["positions"].double() + h * u, b["cells"].double() + h * uc)


@pytest.mark.parametrize("tag,which", [("residual", "box"), ("odd33", "model_batch")])
def test_tangents_are_the_directional_derivative_of_the_energies(tag, which):
    """``e'_i`` along ``(u, u_cell)`` at fixed Cartesian positions against ``(e(R + h u, cell + h u_cell) - e(R - h u, cell -
    h u_cell)) / 2h`` at h = 1e-5, to 1e-6 of the largest tangent (measured 3.1e-8 and 4.2e-8: O(h^2)); their sum is
    ``<u, dE/dR> + <u_cell, dE/dcell>``."""
    ref, _ = co.reference_model(tag, which)
    _, u, uc = co.seeds(which)
    h = 1e-5
    fd = (_energies(tag, which, h) - _energies(tag, which, -h)) / (2.0 * h)
    scale = float(ref["tangent"].abs().max())
    err = float((fd - ref["tangent"]).abs().max())
    print(f"({tag} {which}, central difference against the tangents, {err / scale:.2e})")
    assert scale > 1e-4 and err <= 1e-6 * scale
    want = float((u * ref["grad"]).sum() + (uc * ref["cell_grad"]).sum())
    assert abs(float(ref["tangent"].sum()) - want) <= 1e-12 * scale * len(fd)
    assert float((uc * ref["cell_grad"]).sum()) != 0.0


def test_closed_form_against_autograd_on_the_sheared_cell():
    """The four terms of section 23 against ``torch.autograd.functional.jvp`` of ``_ewald_oracle.potential_periodic`` along
    ``(u, u_c)`` on the sheared cell with its partly unwrapped atoms, to 1e-12 absolute."""
    c, b = ec.case("sheared"), ec.batch("sheared")
    pos, cell = b["positions"].double()[: b["first_atom"][1]], b["cells"][0].double()
    n = pos.shape[0]
    m = b["centers"] < n
    edges = (b["centers"][m], b["neighbors"][m], b["cell_shifts"][m])
    g = torch.Generator().manual_seed(23)
    x = torch.randn(n, 3, generator=g, dtype=torch.float64)
    u = torch.randn(n, 3, generator=g, dtype=torch.float64)
    u_c = cell @ (0.1 * torch.randn(3, 3, generator=g, dtype=torch.float64))
    _, want = torch.autograd.functional.jvp(
        lambda p, h: eo.potential_periodic(p, h, x, edges, c.smearing, c.resolution, c.cutoff), (pos, cell), (u, u_c))
    got = co.closed_form(pos, cell, x, edges, u, u_c, c.smearing, c.resolution, c.cutoff)
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print(f"(sheared, {n} atoms, {len(eo.kvector_indices(cell, c.resolution))} k-vectors, {int(m.sum())} edges, closed form against "
          f"autograd {err:.1e} at a scale of {scale:.2f})")
    assert scale > 0.1 and err <= 1e-12


def test_operator_oracle_is_the_derivative_of_the_first_order_cell_gradient():
    """``out_grad_potential`` with ``u_c`` alone is ``d<u_c, dL/dcell>/dg``: against a central difference of the first-order
    oracle's dL/dcell along a direction of ``g``."""
    name, channels = "sheared", 3
    c, b = ec.case(name), ec.batch(name)
    q, gv = ec.charges(name, channels)
    _, _, u_c = co.cotangents(b, channels)
    out_q, out_g = co.reference(name, channels, torch.float64, (False, False, True))
    dg = torch.randn(gv.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    h = 1e-4
    plus = eo.operator_reference(b, q, gv + h * dg, c.smearing, c.resolution, c.cutoff, torch.float64)[3]
    minus = eo.operator_reference(b, q, gv - h * dg, c.smearing, c.resolution, c.cutoff, torch.float64)[3]
    fd = float((u_c * (plus - minus)).sum() / (2.0 * h))
    got = float((out_g * dg).sum())
    print(f"(sheared, <out_grad_potential, dg> {got:.10e}, central difference {fd:.10e})")
    assert abs(got - fd) <= 1e-8 * abs(fd)


def test_strain_seeds_reproduce_the_gradient_of_a_stress_loss():
    """``strain_loss_and_seeds`` on the oracle's dE/dR and dE/dcell, its seeds fed to ``evaluate_cell``: dL/dtheta of an MSE on
    dE/d(strain) formed the reference's way (``positions @ strain``, ``cell @ strain``), to 1e-10 relative."""
    from metatrain_amd.pet.trainer import strain_loss_and_seeds

    tag, which = "odd33", "two_cells"
    hypers, params = lo.model_case(tag)
    b = co.batch_of(which)
    n_sys = len(b["first_atom"]) - 1
    sysidx = b["system_indices"].long()
    target = torch.randn(n_sys, 3, 3, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    p = lo.leaves_of(params, torch.float64)
    keys = [k for k in p if k != "species_to_species_index"]
    strain = torch.eye(3, dtype=torch.float64).repeat(n_sys, 1, 1).requires_grad_(True)
    pos0, cells0 = b["positions"].double(), b["cells"].double()
    pos = torch.einsum("na,nab->nb", pos0, strain[sysidx])
    cells = cells0 @ strain
    e = lo.atomic_energies(p, hypers, b, pos, cells)
    (virial,) = torch.autograd.grad(e.sum(), strain, create_graph=True)
    loss = ((virial - target) ** 2).mean()
    want = torch.autograd.grad(loss, [p[k] for k in keys], allow_unused=True)
    first = co.evaluate_cell(params, hypers, b, torch.zeros(len(pos0), dtype=torch.float64), None, None, torch.float64)
    loss_s, u, u_cell = strain_loss_and_seeds(pos0, cells0, sysidx, first["grad"], first["cell_grad"], target, 1.0)
    assert abs(float(loss_s) - float(loss)) <= 1e-12 * abs(float(loss))
    got = co.evaluate_cell(params, hypers, b, torch.zeros(len(pos0), dtype=torch.float64), u, u_cell, torch.float64)["grads"]
    worst = 0.0
    for k, w in zip(keys, want):
        w = torch.zeros_like(p[k]) if w is None else w
        scale = float(w.abs().max())
        if scale == 0.0:
            assert float(got[k].abs().max()) == 0.0, k
            continue
        worst = max(worst, float((got[k] - w).abs().max()) / scale)
    print(f"(two_cells, stress-loss gradient through the seeds, worst tensor {worst:.1e})")
    assert worst <= 1e-10


def test_two_cells_is_the_batch_the_issue_names():
    b = co.batch_of("two_cells")
    assert b["positions"].shape[0] == 68 and list(b["first_atom"]) == [0, 33, 36, 68]
    assert [all(p) for p in b["pbcs"]] == [True, False, True]
    assert not torch.equal(b["cells"][0], b["cells"][2])
    print(f"(two_cells, {len(b['centers'])} edges)")
    uc = co.seeds("two_cells")[2]
    assert float(uc[1].abs().max()) == 0.0 and float(uc[0].abs().max()) > 0.0 and float(uc[2].abs().max()) > 0.0


# ---- the library without a GPU ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from metatrain_amd import _lib

    return _lib.load()


NEW_SYMBOLS = ("pet_ewald_second_cell_workspace_bytes", "pet_ewald_second_cell", "pet_p3m_second_cell_workspace_bytes",
               "pet_p3m_second_cell", "pet_train2_long_range_cell_workspace_bytes", "pet_backward_train2_long_range_cell")


def test_new_symbols_exist(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


def test_workspace_functions_refuse_on_the_host(lib):
    """-1 without a plan, on the other mode's handle, for C < 1 and for a null handle."""
    plain, mesh = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.pet_ewald_create(1.4, 1.33, 4.5, ctypes.byref(plain)) == 0
    assert lib.pet_ewald_create(1.4, 1.33, 4.5, ctypes.byref(mesh)) == 0
    assert lib.pet_ewald_set_p3m(mesh, 5) == 0
    try:
        for fn in (lib.pet_ewald_second_cell_workspace_bytes, lib.pet_p3m_second_cell_workspace_bytes):
            for handle, c in ((plain, 8), (mesh, 8), (plain, 0), (mesh, 0), (None, 8)):
                assert fn(handle, c) == -1
        assert lib.pet_train2_long_range_cell_workspace_bytes(None, None, None) == -1
        for fn in (lib.pet_ewald_second_cell, lib.pet_p3m_second_cell):
            assert fn(None, None, None, None, None, None, None, None, 8, None, None, None, 0, None) != 0
        assert lib.pet_backward_train2_long_range_cell(None, None, None, None, None, 0, None, None, None, None, None, None) != 0
    finally:
        lib.pet_ewald_destroy(plain)
        lib.pet_ewald_destroy(mesh)


def _lr_hypers(**extra):
    h = dict(opet.DEFAULT_HYPERS, **extra)
    h["long_range"] = {"enable": True, "use_ewald": True, "smearing": 1.4, "kspace_resolution": 1.33, "interpolation_nodes": 5}
    return h


def test_refusals_are_unchanged_without_the_opt_in():
    from metatrain_amd import long_range as lr

    h = _lr_hypers()
    feat = lr.LongRangeFeaturizerHip(h)
    assert feat.cell_tangents is False
    fw = lr.LongRangeForward(types.SimpleNamespace(hypers=h, lib=None), feat, None, None)
    with pytest.raises(lr.PetHipError, match="u_cell .a cell tangent: the stress / strain-gradient loss. of a long-range model is not built"):
        fw.backward_train2(None, None, None, u_cell=torch.zeros(1, 3, 3))
    with pytest.raises(lr.PetHipError, match="target_strain_gradients .the stress loss. of a long-range model are not built"):
        lr.LongRangeTrainStep._refuse(fw, torch.zeros(1, 3, 3), None)
    # with the opt-in the same calls pass the gate (and what stays refused still is)
    on = lr.LongRangeFeaturizerHip(h, cell_tangents=True)
    assert on.cell_tangents is True
    fw_on = lr.LongRangeForward(types.SimpleNamespace(hypers=h, lib=None), on, None, None)
    lr.LongRangeTrainStep._refuse(fw_on, torch.zeros(1, 3, 3), None)
    with pytest.raises(lr.PetHipError, match="extra_targets"):
        lr.LongRangeTrainStep._refuse(fw_on, torch.zeros(1, 3, 3), {"non_conservative_forces": {}})
    with pytest.raises(lr.PetHipError, match="seed_features"):
        fw_on.backward_train2(None, None, None, u_cell=torch.zeros(1, 3, 3), seed_features=(None, None))


def test_p3m_cell_tangents_need_second_order_by_name():
    from metatrain_amd import long_range as lr

    h = _lr_hypers()
    with pytest.raises(lr.PetHipError, match="cell_tangents=True with method='p3m' needs second_order=True"):
        lr.LongRangeFeaturizerHip(h, method="p3m", cell_tangents=True)
    with pytest.raises(lr.PetHipError, match="cell_tangents=True with method='p3m' needs second_order=True"):
        lr.LongRangeFeaturizerHip.from_state_dict(h, eo.featurizer_params(h["d_node"]), method="p3m", cell_tangents=True)
    feat = lr.LongRangeFeaturizerHip(h, method="p3m", second_order=True, cell_tangents=True)
    assert feat.cell_tangents and feat.ewald.second_order
    with pytest.raises(lr.PetHipError, match="cell tangents through P3M are not built on this operator"):
        lr.P3MHip(1.4, 1.33, 4.5, 5).second_cell(None, None, None, None, u_cells=torch.zeros(1, 3, 3))
