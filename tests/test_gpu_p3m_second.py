"""GPU tests of the mesh operator's second-order operation (``pet_p3m_second``, ``P3MHip.second`` under
``second_order=True``, double backward through a P3M ``LongRangeFeaturizerHip``) against the fp64
oracle's double backward (``tests/_p3m_second_oracle.py``), on the cases of ``tests/p3m_cases.py``.

Bar, per SYSTEM and result (``ewald_cases.check_per_system``): ``max|got - ref| <= max(1e-5 max|ref|, 2 max|oracle_fp32 - ref|)``
over the system's rows -- ``gen_shapes.bar(y)`` in absolute form; ``test_p3m_second_cpu.py`` holds every run's ``y`` under
``gen_shapes.Y_CAP``. All three results are per-atom. A result whose reference is identically zero comes back identically
zero. Every test prints ``(case, system, quantity, e32, relmax)`` and a ``[worst]`` line per result before it asserts; the
measured table is in DESIGN.md section 22."""
import functools

import pytest
import torch

import _ewald_oracle as eo
import _ewald_second_oracle as so
import _p3m_second_oracle as so2
import ewald_cases as ec
import gen_shapes
import p3m_cases as pc
from test_p3m_second_cpu import GPU_RUNS, HALF_RUN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOTH, ONLY_CHARGES, ONLY_POSITIONS = (True, True), (True, False), (False, True)
ALL = (True, True, True)


def _operator(b, nodes=5):
    from metatrain_amd import long_range as lr

    _, graph = ec.graph(b, torch.device(DEV))
    op = lr.P3MHip(pc.SMEARING, pc.SPACING, pc.CUTOFF, nodes, second_order=True).plan(b["cells"], b["pbcs"], b["first_atom"])
    return op, graph


@functools.lru_cache(maxsize=None)
def _shared(name, nodes):
    """One graph and one planned operator per (case, order), for the tests that do not look at the handle's state."""
    return _operator(pc.batch(name), nodes)


def _inputs(name, channels, rows=slice(None)):
    dev = torch.device(DEV)
    q, gv = pc.charges(name, channels)
    u_q, u_r = so2.cotangents(name, channels)
    pos = pc.batch(name)["positions"]
    return tuple(t[rows].float().to(dev) for t in (pos, q, gv, u_q, u_r))


def _second(op, graph, inputs, halves=BOTH, results=ALL):
    pos, q, gv, u_q, u_r = inputs
    return op.second(graph, pos, q, gv, u_q if halves[0] else None, u_r if halves[1] else None, results=results)


def _check(name, nodes, channels, got, halves=BOTH, label=None):
    ref = so2.reference(name, channels, nodes, torch.float64, halves)
    f32 = so2.reference(name, channels, nodes, torch.float32, halves)
    ec.check_per_system(label or f"p3m second {name} p={nodes} C={channels}", pc.batch(name), so2.NAMES, so2.KINDS, got, ref, f32)
    for k, r in enumerate(ref):
        if float(r.abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, (name, so2.NAMES[k])
    return ref, f32


@functools.lru_cache(maxsize=None)
def _device(name, nodes, channels):
    op, graph = _shared(name, nodes)
    return _second(op, graph, _inputs(name, channels))


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name, nodes, channels", GPU_RUNS, ids=[f"{n}-p{p}-C{c}" for n, p, c in GPU_RUNS])
def test_second_against_the_oracle(name, nodes, channels):
    """All three results. ``nodes``: every order (p = 1: the tangent weight vanishes, so only ``A u_q`` and the exclusion rows
    survive; p = 2: the Hessian weight vanishes). ``small_mesh``: N = 4 < p and a one-atom cell. ``on_nodes``: atoms on the
    floor boundaries of both parities. ``anisotropic``: du through a sheared, left-handed cell on an 8 x 16 x 4 mesh.
    ``unwrapped``: wrapped weights. ``bins``: 33 atoms in one bin. ``mixed``: an empty periodic system, an open cluster, a
    one-atom cell. ``channels``: C = 1, 3 (scalar), 33 (a partly filled chunk of 8 and of 64), 256, 260 (a fifth block of 64).
    ``supercell``: the doubled cell's rows repeat the primitive ones within the sum of their bars."""
    assert name in pc.ALL_CASES and nodes in pc.case(name).nodes
    op, _ = _shared(name, nodes)
    assert [op.mesh_shape(s) for s in range(op.n_systems)] == pc.EXPECTED_MESHES[name]
    got = _device(name, nodes, channels)
    ref, f32 = _check(name, nodes, channels, got)
    if channels > 33:  # (the cap of the wide runs, which the CPU suite leaves to this side)
        for r, y in zip(ref, f32):
            assert gen_shapes.bar(float((y - r).abs().max()) / float(r.abs().max())) > 0.0
    if name == "supercell":
        n = pc.batch(name)["first_atom"][1]
        for k, quantity in enumerate(so2.NAMES):
            bar = ec.system_bar(ref[k], f32[k], slice(0, n))[0] + ec.system_bar(ref[k], f32[k], slice(n, 2 * n))[0]
            err = float((got[k][:n] - got[k][n:2 * n]).abs().max())
            print(f"(supercell, primitive against supercell, {quantity}, {err:.2e}, bar {bar:.2e})")
            assert err <= bar, quantity


@pytest.mark.parametrize("halves", [ONLY_CHARGES, ONLY_POSITIONS], ids=["u_positions=None", "u_charges=None"])
def test_one_cotangent_alone(halves):
    """``anisotropic`` at C = 24 with one cotangent ``None``, against the oracle with that half zero (u_q alone: one
    transform pair for ``A u_q``, a second for the first-order force; u_r alone: ``phi_a`` is ``K (D_u W) q`` alone)."""
    name, nodes, channels = HALF_RUN
    op, graph = _shared(name, nodes)
    got = _second(op, graph, _inputs(name, channels), halves)
    _check(name, nodes, channels, got, halves, label=f"p3m second {name} C={channels} halves={halves}")
    if halves == ONLY_CHARGES:
        assert float(got[0].abs().max()) == 0.0  # (D_u A) g without a direction


RESULT_SETS = [(True, False, False), (False, True, False), (False, False, True), (True, False, True)]


@pytest.mark.parametrize("results", RESULT_SETS, ids=["charges", "grad_potential", "positions", "charges+positions"])
def test_a_selection_has_the_bits_of_the_full_call(results):
    """``mixed`` at C = 24: the results asked for alone (the dual pass asks for the second alone in its forward sweep, the
    first alone or the first and third in its reverse) against the full call; the others come back ``None``. The hook is
    called twice per transform pair: 2 pairs for either row result alone, 4 with the positions."""
    op, graph = _shared("mixed", 5)
    full = _device("mixed", 5, 24)
    before = op.transform_calls
    got = _second(op, graph, _inputs("mixed", 24), results=results)
    assert op.transform_calls - before == (8 if results[2] else 4)
    for k, want in enumerate(results):
        assert (got[k] is not None) == want
        if want:
            assert torch.equal(got[k], full[k]), so2.NAMES[k]


def test_a_second_call_gives_the_same_bits():
    op, graph = _shared("channels", 5)
    again = _second(op, graph, _inputs("channels", 260))
    assert _equal(again, _device("channels", 5, 260))


def test_a_system_alone_gives_the_bits_of_its_rows_in_the_batch():
    """The 43-atom system of ``mixed`` planned and run alone at C = 24: one mesh in place of two, no open system beside it."""
    b = pc.batch("mixed")
    n = b["first_atom"][1]
    assert n == 43
    alone = eo.collate(pc.case("mixed").systems[:1], pc.CUTOFF)
    assert torch.equal(alone["positions"], b["positions"][:n])
    op, graph = _operator(alone)
    got = _second(op, graph, _inputs("mixed", 24, slice(0, n)))
    assert _equal(got, tuple(t[:n] for t in _device("mixed", 5, 24)))


def test_first_order_adjoint_is_untouched_by_a_second_call():
    """``backward`` before and after ``second`` on one handle: identical bits."""
    op, graph = _operator(pc.batch("mixed"))
    pos, q, gv, u_q, u_r = _inputs("mixed", 24)
    before = op.backward(graph, pos, q, gv, want_cell_grad=True)
    op.second(graph, pos, q, gv, u_q, u_r)
    after = op.backward(graph, pos, q, gv, want_cell_grad=True)
    assert _equal(before, after)


def test_open_systems_alone_never_call_the_hook():
    """Two open clusters on a P3M handle: no mesh, no transform, and the results of the Ewald-mode handle's open path."""
    cluster = pc.case("mixed").systems[2]
    b = eo.collate([cluster, cluster], pc.CUTOFF)
    op, graph = _operator(b)
    assert [op.mesh_shape(s) for s in range(2)] == [[0, 0, 0], [0, 0, 0]]
    dev = torch.device(DEV)
    n = b["positions"].shape[0]
    g = torch.Generator().manual_seed(11)
    q, gv, u_q = (torch.randn(n, 24, generator=g, dtype=torch.float64) for _ in range(3))
    u_r = torch.randn(n, 3, generator=g, dtype=torch.float64)
    got = op.second(graph, *(t.float().to(dev) for t in (b["positions"], q, gv, u_q, u_r)))
    assert op.transform_calls == 0
    ref = so2.second_reference(b, q, gv, u_q, u_r, 5, torch.float64)
    f32 = so2.second_reference(b, q, gv, u_q, u_r, 5, torch.float32)
    ec.check_per_system("p3m second open only C=24", b, so2.NAMES, so2.KINDS, got, ref, f32)


def test_an_exception_inside_the_hook_surfaces_as_itself():
    """A hook that raises: the call returns (no hang), raises THAT exception (not a silent zero, not the C side's message),
    and the operator works again afterwards."""
    op, graph = _operator(pc.batch("nodes"))
    inputs = _inputs("nodes", 24)

    class Boom(RuntimeError):
        pass

    def broken(*a):
        raise Boom("the transform failed")

    good = op._transform
    op._transform = broken
    with pytest.raises(Boom, match="the transform failed"):
        _second(op, graph, inputs)
    op._transform = good
    torch.cuda.synchronize()
    assert _equal(_second(op, graph, inputs), _device("nodes", 5, 24))


def test_refusals_by_name():
    """No hook: ``PET_ERR_ARGUMENT`` naming ``pet_p3m_set_transform``. An Ewald-mode handle on the P3M entry and a P3M-mode
    handle on the Ewald entry: refused as before."""
    from metatrain_amd import long_range as lr
    from metatrain_amd import runtime as rt
    from metatrain_amd._lib import PET_ERR_ARGUMENT, check

    b = pc.batch("nodes")
    dev = torch.device(DEV)
    _, graph = ec.graph(b, dev)
    plain = lr.P3MHip(pc.SMEARING, pc.SPACING, pc.CUTOFF, 5).plan(b["cells"], b["pbcs"], b["first_atom"])
    pos, q, gv, u_q, u_r = _inputs("nodes", 3)
    outs = torch.empty_like(q), torch.empty_like(q), torch.empty_like(pos)
    nbytes = int(plain.lib.pet_p3m_second_workspace_bytes(plain.handle, 3))
    assert nbytes > int(plain.lib.pet_p3m_workspace_bytes(plain.handle, 3))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call(entry, handle):
        return entry(handle, graph.handle, rt._ptr(pos), rt._ptr(q), rt._ptr(gv), rt._ptr(u_q), rt._ptr(u_r), 3, rt._ptr(outs[0]),
                     rt._ptr(outs[1]), rt._ptr(outs[2]), rt._ptr(ws), ws.numel(), rt._stream())

    assert call(plain.lib.pet_p3m_second, plain.handle) == PET_ERR_ARGUMENT
    with pytest.raises(lr.PetHipError, match="pet_p3m_set_transform"):
        check(call(plain.lib.pet_p3m_second, plain.handle))
    with pytest.raises(lr.PetHipError, match="P3M-mode handle"):
        check(call(plain.lib.pet_ewald_second, plain.handle))
    assert int(plain.lib.pet_ewald_second_workspace_bytes(plain.handle, 3)) == -1
    ewald = lr.EwaldHip(pc.SMEARING, pc.SPACING, pc.CUTOFF).plan(b["cells"], b["pbcs"], b["first_atom"])
    assert call(ewald.lib.pet_p3m_second, ewald.handle) == PET_ERR_ARGUMENT
    with pytest.raises(lr.PetHipError, match="Ewald-mode handle"):
        check(call(ewald.lib.pet_p3m_second, ewald.handle))
    assert int(ewald.lib.pet_p3m_second_workspace_bytes(ewald.handle, 3)) == -1


# ---- torch double backward through the featuriser ----------------------------------------------------------------------------
D_NODE = 24


def _featurizer(second_order):
    from metatrain_amd import long_range as lr

    b = pc.batch("mixed")
    feat = lr.LongRangeFeaturizerHip.from_state_dict(pc.lr_hypers(5, d_node=D_NODE), eo.featurizer_params(D_NODE),
                                                     device=torch.device(DEV), method="p3m", second_order=second_order)
    return feat.plan(b["cells"], b["pbcs"], b["first_atom"])


def _device_loss(feat, cells_require_grad=False):
    dev = torch.device(DEV)
    b = pc.batch("mixed")
    _, graph = ec.graph(b, dev)
    x, weights, target = (t.float().to(dev) for t in so.featurizer_inputs(b, D_NODE))
    x.requires_grad_(True)
    pos = b["positions"].float().to(dev).requires_grad_(True)
    cells = b["cells"].float().to(dev).requires_grad_(cells_require_grad)
    for k in feat.params:
        feat.params[k].requires_grad_(True)
    loss = so.force_loss(feat(x, pos, cells, graph), pos, weights, target)
    leaves = [x] + [feat.params[k[len("long_range_featurizer."):]] for k in so.PARAM_KEYS]
    return torch.autograd.grad(loss, leaves)


def test_force_loss_gradients_through_the_featurizer():
    """The force-loss double backward of ``test_gpu_long_range_second.py`` with ``method="p3m", second_order=True`` on the
    ``mixed`` batch of ``p3m_cases`` at d_node = C = 24, against the same loss on the P3M oracle. Bar per tensor:
    ``max(1e-5 max|ref|, 2 max|ref_fp32 - ref|)``."""
    b = pc.batch("mixed")
    got = _device_loss(_featurizer(True))
    args = (b, eo.featurizer_params(D_NODE)) + so.featurizer_inputs(b, D_NODE) + (5,)
    ref, f32 = so2.featurizer_reference(*args, torch.float64), so2.featurizer_reference(*args, torch.float32)
    bad = []
    for name, g, r, y in zip(("x",) + so.PARAM_KEYS, got, ref, f32):
        g = g.detach().cpu().double()
        assert g.shape == r.shape, (name, g.shape, r.shape)
        scale, e32, err = float(r.abs().max()), float((y - r).abs().max()), float((g - r).abs().max())
        print(f"(p3m force loss mixed, {name}, {e32 / scale:.2e}, {err / scale:.2e})")
        assert e32 / scale <= gen_shapes.Y_CAP
        if not err <= max(1e-5 * scale, 2.0 * e32):
            bad.append((name, err / scale, e32 / scale))
    assert not bad, bad


def test_double_backward_refusals_that_remain():
    from metatrain_amd._lib import PetHipError

    with pytest.raises(PetHipError, match="mixed position / cell second derivatives"):
        _device_loss(_featurizer(True), cells_require_grad=True)
    with pytest.raises(PetHipError, match="second derivatives through P3M are not built"):
        _device_loss(_featurizer(False))
