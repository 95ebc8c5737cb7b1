"""Premises of the mesh operator's second-order tests that need no GPU: the oracle of ``tests/_p3m_second_oracle.py`` is what
it says (central differences, symmetry of the Hessian), every case the GPU tests run keeps its fp32 yardstick under the
project's cap and (for p <= 3) its atoms away from the stencil's breakpoints, the three new symbols exist and refuse on the
host what they document, the ``second_order`` switch is an opt-in, and the transform hook's host side does what
``P3MHip._mesh_potential`` does."""
import ctypes
import os
import re

import pytest
import torch

import _p3m_second_oracle as so2
import ewald_cases as ec
import gen_shapes
import p3m_cases as pc
from metatrain_amd import _lib
from metatrain_amd import long_range as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Seven digits, the bound of test_ewald_second_cpu.py. The O(h^2) term of the central difference along positions is 2e-8 .. 3e-7
# at h = 1e-4 on these cases (it scales with the fourth derivative of a spline of order p); at h = 2.5e-5 it is 16 times
# smaller, and the rounding of the difference quotient (1e-16 / h) is still five decades below the bound.
FD_STEP = 2.5e-5
FD_BOUND = 1.2e-7

# every (case, nodes, channels) the GPU tests run against the oracle (test_gpu_p3m_second.py imports this list)
GPU_RUNS = ([("nodes", p, 24) for p in (1, 2, 3, 4, 5)] + [("small_mesh", 5, 24), ("on_nodes", 5, 24), ("on_nodes", 4, 24),
            ("anisotropic", 5, 24), ("unwrapped", 5, 24), ("bins", 5, 24), ("bins", 4, 24), ("mixed", 5, 24), ("supercell", 5, 24)]
            + [("channels", 5, c) for c in pc.CHANNELS])
# the run that is repeated with one cotangent alone. Not ``mixed``: with u_q alone the one-atom cell's out_positions is the mesh's
# residue of a first-order force (2e-6 of the batch's scale), and the fp32 oracle resolves it to 1.3e-3 of itself, above the cap.
HALF_RUN = ("anisotropic", 5, 24)
HALVES = {"both": (True, True), "u_positions=None": (True, False), "u_charges=None": (False, True)}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from metatrain_amd import build

        build.build(verbose=False)
    return _lib.load()


def _psi(b, q, gv, u_q, u_r, nodes):
    import _p3m_oracle as po

    _, gq, gpos, _ = po.operator_reference(b, q, gv, pc.SMEARING, pc.SPACING, pc.CUTOFF, nodes, torch.float64)
    return float((u_q * gq).sum() + (u_r * gpos).sum())


@pytest.mark.parametrize("name, nodes", [("nodes", 5), ("nodes", 3), ("mixed", 5)])
def test_oracle_agrees_with_central_differences(name, nodes):
    """C = 3, fp64: central differences of the first-order oracle's ``(gq, gpos)`` along one seeded direction each of ``q``,
    ``g`` and ``pos``, contracted with ``(u_q, u_r)``, against ``<out, direction>`` of the second-order oracle."""
    channels = 3
    b = pc.batch(name)
    q, gv = pc.charges(name, channels)
    u_q, u_r = so2.cotangents(name, channels)
    out = so2.reference(name, channels, nodes, torch.float64)
    g = torch.Generator().manual_seed(99)
    for k, (label, base) in enumerate((("q", q), ("g", gv), ("pos", b["positions"]))):
        step = torch.randn(base.shape, generator=g, dtype=torch.float64)
        sides = []
        for sign in (1.0, -1.0):
            moved = base + sign * FD_STEP * step
            bb = dict(b, positions=moved) if label == "pos" else b
            sides.append(_psi(bb, moved if label == "q" else q, moved if label == "g" else gv, u_q, u_r, nodes))
        fd = (sides[0] - sides[1]) / (2.0 * FD_STEP)
        want = float((out[k] * step).sum())
        rel = abs(fd - want) / abs(want)
        print(f"(fd {name} p={nodes} along {label}: {fd:.12e} against {want:.12e}, relative {rel:.1e})")
        assert rel <= FD_BOUND, (label, rel)


def test_position_hessian_of_the_oracle_is_symmetric():
    """``<v, H u> = <u, H v>`` with ``H u = out_positions`` at ``u_q = None``, on ``nodes`` at p = 5 and C = 3 in fp64."""
    b = pc.batch("nodes")
    q, gv = pc.charges("nodes", 3)
    g = torch.Generator().manual_seed(7)
    u, v = (torch.randn(b["positions"].shape, generator=g, dtype=torch.float64) for _ in range(2))
    hu = so2.second_reference(b, q, gv, None, u, 5, torch.float64)[2]
    hv = so2.second_reference(b, q, gv, None, v, 5, torch.float64)[2]
    a, d = float((v * hu).sum()), float((u * hv).sum())
    print(f"(<v, H u> {a:.12e}, <u, H v> {d:.12e})")
    assert abs(a - d) <= 1e-11 * max(abs(a), abs(d))


CAP_RUNS = [r + ("both",) for r in GPU_RUNS if r[2] <= 33] + [HALF_RUN + (h,) for h in HALVES if h != "both"]


@pytest.mark.parametrize("name, nodes, channels, halves", CAP_RUNS, ids=lambda v: str(v))
def test_yardstick_of_every_gpu_run_stays_under_the_cap(name, nodes, channels, halves):
    """``y = max|oracle_fp32 - oracle_fp64| / max|oracle_fp64|`` per system and result stays under ``gen_shapes.Y_CAP``: the
    bar ``gen_shapes.bar(y)`` of the GPU tests pins something. (The C = 256 and 260 runs of ``channels`` share their system
    with C = 33 and are measured on the GPU side, where the oracle is computed anyway.)"""
    b = pc.batch(name)
    ref = so2.reference(name, channels, nodes, torch.float64, HALVES[halves])
    f32 = so2.reference(name, channels, nodes, torch.float32, HALVES[halves])
    worst = 0.0
    for r, y in zip(ref, f32):
        for s in range(len(b["first_atom"]) - 1):
            rows = ec.system_rows(b, "atom", s)
            if r[rows].numel() == 0:
                continue
            _, scale, e32, fell_back = ec.system_bar(r, y, rows)
            if scale > 0.0:
                worst = max(worst, e32 / scale)
    print(f"(yardstick {name} p={nodes} C={channels} {halves}: {worst:.2e})")
    assert worst <= gen_shapes.Y_CAP


@pytest.mark.parametrize("name, nodes", sorted({(n, p) for n, p, _ in GPU_RUNS if p <= 3}))
def test_low_orders_stay_off_the_stencil_breakpoints(name, nodes):
    """``M_3''`` (and ``M_2'``, ``M_1``) jump where the stencil moves: no atom of a case run at p <= 3 lies within 1e-4 mesh
    units of such a point, so the oracle's derivative and the device's agree on which side they are."""
    d = so2.stencil_distance(name, nodes)
    print(f"(breakpoint distance {name} p={nodes}: {d:.3e} mesh units)")
    assert d >= 1e-4


def test_new_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "pet_hip.h")).read()
    for name in ("pet_p3m_set_transform", "pet_p3m_second_workspace_bytes", "pet_p3m_second"):
        assert re.search(r"\b" + name + r"\s*\((const )?pet_ewald_t\* e", header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_workspace_bytes_and_hook_refuse_on_the_host(lib):
    """``pet_p3m_second_workspace_bytes`` is -1 without a plan, on an Ewald-mode handle, for C < 1 and for a null handle;
    ``pet_p3m_set_transform`` refuses an Ewald-mode handle and takes and removes a hook on a P3M-mode one. No device call."""
    plain, mesh = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.pet_ewald_create(1.4, 1.33, 4.5, ctypes.byref(plain)))
    _lib.check(lib.pet_ewald_create(1.4, 1.33, 4.5, ctypes.byref(mesh)))
    _lib.check(lib.pet_ewald_set_p3m(mesh, 5))
    hook = _lib.P3M_TRANSFORM_FN(lambda *a: 0)
    try:
        for handle, c in ((mesh, 8), (plain, 8), (mesh, 0), (None, 8)):
            assert lib.pet_p3m_second_workspace_bytes(handle, c) == -1
        assert lib.pet_p3m_set_transform(plain, hook, None) == _lib.PET_ERR_ARGUMENT
        assert lib.pet_p3m_set_transform(mesh, hook, None) == 0
        assert lib.pet_p3m_set_transform(mesh, _lib.P3M_TRANSFORM_FN(), None) == 0
        # the second-order entry refuses a handle without a plan before it looks at anything else
        rc = lib.pet_p3m_second(mesh, None, None, None, None, None, None, 8, None, None, None, None, 0, None)
        assert rc == _lib.PET_ERR_ARGUMENT
    finally:
        lib.pet_ewald_destroy(plain)
        lib.pet_ewald_destroy(mesh)


def test_second_order_is_an_opt_in():
    op = lr.P3MHip(1.4, 1.33, 4.5, 5, second_order=True)
    assert op.second_order and op._hook is not None
    assert not lr.P3MHip(1.4, 1.33, 4.5, 5).second_order
    x = torch.zeros(2, 3)
    with pytest.raises(_lib.PetHipError, match="no CPU path"):
        op.second(None, x, x, x, u_charges=x)
    with pytest.raises(_lib.PetHipError, match="both None"):
        op.second(None, x, x, x)
    with pytest.raises(_lib.PetHipError, match="at least one set"):
        op.second(None, x, x, x, u_charges=x, results=(False, False, False))
    with pytest.raises(_lib.PetHipError, match="second derivatives through P3M are not built.*second_order=True"):
        lr.P3MHip(1.4, 1.33, 4.5, 5).second(None, x, x, x, u_positions=x)
    h = pc.lr_hypers(5)
    assert lr.LongRangeFeaturizerHip(h, method="p3m", second_order=True).ewald.second_order
    assert not lr.LongRangeFeaturizerHip(h, method="p3m").ewald.second_order
    state = lr.LongRangeFeaturizerHip(h, method="p3m").state_dict()
    assert lr.LongRangeFeaturizerHip.from_state_dict(h, state, method="p3m", second_order=True).ewald.second_order
    for method in ("ewald", None):
        with pytest.raises(_lib.PetHipError, match="second_order=True is the switch of the P3M operator"):
            lr.LongRangeFeaturizerHip(pc.lr_hypers(5, use_ewald=True), method=method, second_order=True)


def test_hook_transforms_the_packed_meshes_in_place_and_keeps_an_exception():
    """The hook's host side on a CPU workspace: two meshes (8 x 4 x 2 and 4 x 4 x 4) packed at C = 3 behind 256 bytes of
    something else; forward into the half spectrum, inverse back: ``irfftn(rfftn(x), norm="forward") = M x`` per mesh, and
    the bytes around the two buffers untouched. An exception inside the hook comes back from ``_with_hook``; without a
    workspace the hook itself raises by name."""
    op = lr.P3MHip(1.4, 1.33, 4.5, 5, second_order=True)
    C = 3
    op._meshes = [((8, 4, 2), 0, 0), ((4, 4, 4), 64, 64)]
    m_pts, s_pts = 64 + 64, 64 + 48
    mesh_off, spec_off = 256, 256 + 4 * m_pts * C + 256
    total = spec_off + 8 * s_pts * C + 256
    ws = torch.full((total,), 0x5A, dtype=torch.uint8)
    x = torch.randn(m_pts * C, generator=torch.Generator().manual_seed(1))
    ws[mesh_off:mesh_off + 4 * m_pts * C].view(torch.float32).copy_(x)
    calls = []
    op._with_hook(ws, lambda: calls.append(op._hook(None, 0, mesh_off, spec_off, C)) or 0)
    spec = ws[spec_off:spec_off + 8 * s_pts * C].view(torch.complex64)
    want0 = torch.fft.rfftn(x[:64 * C].view(C, 8, 4, 2), dim=(1, 2, 3)).reshape(-1)
    want1 = torch.fft.rfftn(x[64 * C:].view(C, 4, 4, 4), dim=(1, 2, 3)).reshape(-1)
    assert torch.allclose(spec, torch.cat([want0, want1]), rtol=1e-5, atol=1e-5)
    op._with_hook(ws, lambda: calls.append(op._hook(None, 1, mesh_off, spec_off, C)) or 0)
    back = ws[mesh_off:mesh_off + 4 * m_pts * C].view(torch.float32)
    assert torch.allclose(back, 64.0 * x, rtol=1e-5, atol=1e-4)
    assert calls == [0, 0] and op.transform_calls == 2
    for lo, hi in ((0, mesh_off), (mesh_off + 4 * m_pts * C, spec_off), (spec_off + 8 * s_pts * C, total)):
        assert bool((ws[lo:hi] == 0x5A).all())

    def broken(*a):
        raise ZeroDivisionError("inside the hook")

    op._transform = broken
    with pytest.raises(ZeroDivisionError, match="inside the hook"):
        op._with_hook(ws, lambda: op._hook(None, 0, mesh_off, spec_off, C))
    del op._transform
    assert op._hook(None, 0, mesh_off, spec_off, C) == 1 and isinstance(op._hook_error, _lib.PetHipError)
