"""GPU tests of the P3M operator (``csrc/p3m.hip``, ``metatrain_amd.long_range.P3MHip``) and of the whole long-range PET under
``method="p3m"`` against the fp64 oracle of the definition (``tests/_p3m_oracle.py``), on the cases of ``tests/p3m_cases.py``.

Bar, per quantity and PER SYSTEM (``ewald_cases.check_per_system``):
``max|got - ref| <= max(1e-5 max|ref|, 2 max|oracle_fp32 - ref|)`` over one system's rows, ``ref`` the oracle in fp64 and
``oracle_fp32`` the same oracle in fp32 on the host; the batch-wide scale only where a quantity vanishes by symmetry on a system
(below 1e-9 of the batch-wide one). dL/dcell of an open system is exactly 0. Every test prints
``(case, system, quantity, e32, relmax)`` before it asserts; the measured table is in DESIGN.md section 19."""
import functools

import pytest
import torch

import _ewald_oracle as eo
import _p3m_oracle as po
import ewald_cases as ec
import p3m_cases as pc
from _memo import memo_oracle
from oracle import pet as opet

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _run_case(name, nodes, channels=24, label=None):
    dev = torch.device(DEV)
    b = pc.batch(name)
    q, gv = pc.charges(name, channels)
    _, graph, op = pc.operator(b, dev, nodes)
    assert [op.mesh_shape(s) for s in range(len(b["first_atom"]) - 1)] == pc.EXPECTED_MESHES[name]
    got = ec.run(op, graph, b, q, gv, dev)
    ref, f32 = pc.reference(name, channels, nodes, torch.float64), pc.reference(name, channels, nodes, torch.float32)
    ec.check_per_system(label or f"{name} p={nodes} C={channels}", b, pc.QUANTITIES, pc.KINDS, got, ref, f32)
    for s, pbc in enumerate(b["pbcs"]):
        if not any(pbc):
            assert float(got[3][s].abs().max()) == 0.0, (name, s)
    return got


CASE_RUNS = [(name, p) for name in pc.OPERATOR_CASES for p in pc.case(name).nodes]


@pytest.mark.parametrize("name, nodes", CASE_RUNS, ids=[f"{n}-p{p}" for n, p in CASE_RUNS])
def test_operator_case(name, nodes):
    """Potential, dL/dq, dL/dR and dL/dcell of every case of p3m_cases at C = 24, per system."""
    got = _run_case(name, nodes)
    if name == "supercell":
        # the primitive cell against the first copy inside its 2 x 1 x 1 supercell: the same mesh spacing, so the same operator
        b = pc.batch(name)
        ref, f32 = pc.reference(name, 24, nodes, torch.float64), pc.reference(name, 24, nodes, torch.float32)
        n = b["first_atom"][1]
        for k, quantity in enumerate(pc.QUANTITIES[:3]):
            bar = ec.system_bar(ref[k], f32[k], slice(0, n))[0] + ec.system_bar(ref[k], f32[k], slice(n, 2 * n))[0]
            err = float((got[k][:n] - got[k][n:2 * n]).abs().max())
            print(f"(supercell, primitive against supercell, {quantity}, {err:.2e}, bar {bar:.2e})")
            assert err <= bar, quantity


@pytest.mark.parametrize("channels", pc.CHANNELS)
def test_operator_channel_widths(channels):
    """C = 1, 3 (scalar loads), 33 (a partly filled chunk of 8 and of 64), 256 and 260 (16-byte loads, a fifth block of 64; 260
    is no multiple of 8): the 43-atom triclinic system."""
    _run_case("channels", 5, channels)


def test_operator_from_misaligned_views_and_a_larger_workspace():
    """Charges and dL/dV that start 4 bytes into their allocations give the bits of aligned ones (C = 256: the 16-byte loads
    are off), and C = 3 on the workspace that C = 260 left behind gives the bits of C = 3 on a fresh operator."""
    dev = torch.device(DEV)
    b = pc.batch("channels")
    _, graph, op = pc.operator(b, dev, 5)
    q, gv = pc.charges("channels", 256)
    aligned = ec.run(op, graph, b, q, gv, dev)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
        view = buf[1:].view(t.shape)
        view.copy_(t.float())
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view

    pos = b["positions"].float().to(dev)
    qs, gs = shifted(q), shifted(gv)
    v = op.potential(graph, pos, qs)
    gq, gp, gc = op.backward(graph, pos, qs, gs, want_cell_grad=True)
    for name, x, y in zip(pc.QUANTITIES, aligned, (v, gq, gp, gc)):
        assert torch.equal(x, y), name
    q260, g260 = pc.charges("channels", 260)
    ec.run(op, graph, b, q260, g260, dev)
    big = op._workspace.numel()
    q3, g3 = pc.charges("channels", 3)
    on_big = ec.run(op, graph, b, q3, g3, dev)
    assert op._workspace.numel() == big
    _, graph1, fresh = pc.operator(b, dev, 5)
    alone = ec.run(fresh, graph1, b, q3, g3, dev)
    assert fresh._workspace.numel() < big
    for name, x, y in zip(pc.QUANTITIES, on_big, alone):
        assert torch.equal(x, y), name


def test_operator_is_deterministic_and_its_mesh_is_batch_independent():
    """The whole operator twice: the same bits. The spread mesh of the 43-atom system alone and inside the mixed batch: the
    same bits. The whole operator alone against inside the batch: within the bar (the transforms of a batch of one and of
    several meshes are torch's)."""
    from metatrain_amd import runtime as rt
    from metatrain_amd._lib import check

    dev = torch.device(DEV)
    b = pc.batch("mixed")
    q, gv = pc.charges("mixed", 24)
    _, graph, op = pc.operator(b, dev, 5)
    a = ec.run(op, graph, b, q, gv, dev)
    again = ec.run(op, graph, b, q, gv, dev)
    assert all(torch.equal(x, y) for x, y in zip(a, again))
    n = b["first_atom"][1]
    alone = eo.collate(pc.case("mixed").systems[:1], pc.CUTOFF)
    assert torch.equal(alone["positions"], b["positions"][:n])
    _, graph1, op1 = pc.operator(alone, dev, 5)

    def spread(o, g, bb, x):
        pos, xx = bb["positions"].float().to(dev), x.float().to(dev).contiguous()
        ws = o._ws(24, dev)
        mesh = torch.full((o._mesh_points * 24,), float("nan"), dtype=torch.float32, device=dev)
        check(o.lib.pet_p3m_spread(o.handle, g.handle, rt._ptr(pos), rt._ptr(xx), 24, rt._ptr(mesh), rt._ptr(ws), ws.numel(),
                                      rt._stream()))
        return mesh

    inside, single = spread(op, graph, b, q), spread(op1, graph1, alone, q[:n])
    assert single.numel() == 24 * 512 and not bool(torch.isnan(inside).any())
    assert torch.equal(inside[:single.numel()], single)
    c = ec.run(op1, graph1, alone, q[:n], gv[:n], dev)
    ref, f32 = pc.reference("mixed", 24, 5, torch.float64), pc.reference("mixed", 24, 5, torch.float32)
    for k, (name, kind) in enumerate(zip(pc.QUANTITIES, pc.KINDS)):
        rows = ec.system_rows(b, kind, 0)
        bar = ec.system_bar(ref[k], f32[k], rows)[0]
        err = float((a[k][rows] - c[k]).abs().max())
        print(f"(mixed, alone against inside the batch, {name}, {err:.2e}, bar {bar:.2e})")
        assert err <= bar, name


def test_operator_refuses_before_any_launch():
    """A mesh axis above 512, a missing workspace and the Ewald entry points on a P3M-mode handle, each by name."""
    from metatrain_amd import long_range as lr
    from metatrain_amd import runtime as rt
    from metatrain_amd._lib import check

    dev = torch.device(DEV)
    with pytest.raises(lr.PetHipError, match="at most 512 per mesh axis"):
        lr.P3MHip(pc.SMEARING, pc.SPACING, pc.CUTOFF).plan(torch.diag(torch.tensor([700.0, 9.0, 9.0]))[None], [[True] * 3], [0, 4])
    b = pc.batch("channels")
    _, graph, op = pc.operator(b, dev, 5)
    pos = b["positions"].float().to(dev)
    q = pc.charges("channels", 3)[0].float().to(dev)
    mesh = torch.zeros(3 * 512, dtype=torch.float32, device=dev)
    rc = op.lib.pet_p3m_spread(op.handle, graph.handle, rt._ptr(pos), rt._ptr(q), 3, rt._ptr(mesh), None, 0, rt._stream())
    with pytest.raises(lr.PetHipError, match="P3M workspace missing or too small"):
        check(rc)
    with pytest.raises(lr.PetHipError, match="P3M-mode handle"):
        lr.EwaldHip.potential(op, graph, pos, q)


# ---- the whole model --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_case():
    hypers = pc.lr_hypers(5)  # the reference's defaults: use_ewald false, interpolation_nodes 5
    params = opet.synthetic_params(hypers, eo.TYPES, {"energy": 1}, 0, torch.float32)
    return hypers, params, eo.featurizer_params(hypers["d_node"], 0)


@memo_oracle
def _model_reference(params, lr_params, hypers, batch, dtype):
    return po.model_reference(params, lr_params, hypers, batch, dtype)


def _model_on(b, dev):
    from metatrain_amd import long_range as lr
    from metatrain_amd import runtime as rt

    hypers, params, lr_params = _model_case()
    model = rt.HipModel(hypers, eo.TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    graph = rt.HipGraph(model, b["positions"].float().to(dev), b["cells"].float().to(dev), b["centers"].to(dev),
                        b["neighbors"].to(dev), b["cell_shifts"].to(dev), b["species"].to(dev), b["system_indices"].int().to(dev))
    feat = lr.LongRangeFeaturizerHip.from_state_dict(hypers, lr_params, device=dev, method="p3m")
    return model, graph, feat


def test_long_range_model_under_p3m():
    """Default hypers (``use_ewald: false``) under ``method="p3m"`` on a batch of a 40-atom open cluster, the 64-atom periodic
    box and a QM9 frame: per-atom and per-system energies, dE/dR and dE/dcell per system; then an MD step with
    ``replan=False`` against ``replan=True``: the same bits."""
    from metatrain_amd import long_range as lr

    dev = torch.device(DEV)
    hypers, params, lr_params = _model_case()
    b = ec.model_batch(False)
    model, graph, feat = _model_on(b, dev)
    assert isinstance(feat.ewald, lr.P3MHip)
    got = lr.energy_and_gradient(model, feat, graph, b["pbcs"], want_cell_grad=True)
    ref = _model_reference(params, lr_params, hypers, b, torch.float64)
    f32 = _model_reference(params, lr_params, hypers, b, torch.float32)
    names, kinds = ("atomic", "energies", "grad", "cell_grad"), ("atom", "system", "atom", "system")
    ec.check_per_system("model p3m", b, names, kinds, got, ref[:4], f32[:4])
    for s, pbc in enumerate(b["pbcs"]):
        if not any(pbc):
            assert float(got[3][s].abs().max()) == 0.0
    moved = ec.model_batch(True)
    _, graph2, _ = _model_on(moved, dev)
    kept = lr.energy_and_gradient(model, feat, graph2, moved["pbcs"], want_cell_grad=True, replan=False)
    _, graph3, fresh = _model_on(moved, dev)
    replanned = lr.energy_and_gradient(model, fresh, graph3, moved["pbcs"], want_cell_grad=True, replan=True)
    assert all(torch.equal(x, y) for x, y in zip(kept, replanned))
    assert not torch.equal(kept[0], got[0])
