"""GPU tests of the cell tangents of the long-range operator's second-order operation (``pet_ewald_second_cell`` /
``pet_p3m_second_cell``, ``EwaldHip.second_cell`` / ``P3MHip.second_cell``) against the fp64 oracle
``tests/_long_range_cell_oracle.py`` (autograd of ``Psi = <u_q, A g> + <u_r, grad_r Phi> + <u_c, grad_cell Phi>``).

Bar, per SYSTEM and result (``ewald_cases.check_per_system``): ``max|got - ref| <= max(1e-5 max|ref|, 2 max|oracle_fp32 - ref|)``
over the system's rows. Both results are per-atom. Every test prints ``(case, system, quantity, e32, relmax)`` and a ``[worst]``
line per result before it asserts. Without the feature ``second_cell`` does not exist: every test here fails."""
import functools

import pytest
import torch

import _ewald_oracle as eo
import _long_range_cell_oracle as co
import ewald_cases as ec
import p3m_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL = (True, True, True)
PARTS = {"u_charges alone": (True, False, False), "u_positions alone": (False, True, False), "u_cells alone": (False, False, True)}


def _ewald(name, systems=None):
    c = ec.case(name)
    b = ec.batch(name) if systems is None else eo.collate(systems, c.cutoff)
    _, graph, ew = ec.operator(b, torch.device(DEV), c.smearing, c.resolution, c.cutoff)
    return ew, graph


def _mesh(name, nodes, systems=None):
    from metatrain_amd import long_range as lr

    b = pc.batch(name) if systems is None else eo.collate(systems, pc.CUTOFF)
    _, graph = ec.graph(b, torch.device(DEV))
    op = lr.P3MHip(pc.SMEARING, pc.SPACING, pc.CUTOFF, nodes, second_order=True).plan(b["cells"], b["pbcs"], b["first_atom"])
    return op, graph


@functools.lru_cache(maxsize=None)
def _shared(name, nodes=0):
    """One graph and one planned operator per (case, order); ``nodes = 0``: the Ewald operator on ``ewald_cases``."""
    return _mesh(name, nodes) if nodes else _ewald(name)


def _inputs(name, channels, nodes=0, rows=slice(None), systems=slice(None)):
    dev = torch.device(DEV)
    cases = pc if nodes else ec
    b = cases.batch(name)
    q, gv = cases.charges(name, channels)
    u_q, u_r, u_c = co.cotangents(b, channels, 4400 if nodes else 4300)
    return tuple(t.float().to(dev) for t in (b["positions"][rows], q[rows], gv[rows], u_q[rows], u_r[rows], u_c[systems]))


def _run(op, graph, inputs, parts=ALL, results=(True, True)):
    pos, q, gv, u_q, u_r, u_c = inputs
    return op.second_cell(graph, pos, q, gv, u_q if parts[0] else None, u_r if parts[1] else None, u_c if parts[2] else None,
                          results=results)


@functools.lru_cache(maxsize=None)
def _device(name, channels, nodes=0):
    op, graph = _shared(name, nodes)
    return _run(op, graph, _inputs(name, channels, nodes))


def _check(name, channels, nodes, got, parts=ALL, label=None):
    if nodes:
        ref, f32 = (co.mesh_reference(name, channels, nodes, dt, parts) for dt in (torch.float64, torch.float32))
        b = pc.batch(name)
    else:
        ref, f32 = (co.reference(name, channels, dt, parts) for dt in (torch.float64, torch.float32))
        b = ec.batch(name)
    ec.check_per_system(label or f"second_cell {name} p={nodes} C={channels}", b, co.NAMES, co.KINDS, got, ref, f32)


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


EWALD_CASES = [("periodic_tiles", 3), ("periodic_tiles", 260), ("sheared", 3), ("left_handed", 3), ("unwrapped", 3), ("mixed", 24)]


@pytest.mark.parametrize("name,channels", EWALD_CASES)
def test_ewald_against_the_oracle(name, channels):
    """``periodic_tiles``: 32 and 33 atoms around an empty system and the 2-atom cell whose edges are mostly self-images (their
    edge vectors move with the cell alone); C = 260 a second column block. ``sheared`` / ``left_handed``: U through a cell
    inverse that is not diagonal and a negative determinant. ``unwrapped``: r U of atoms outside the cell. ``mixed``: an open
    system (its row of ``u_cells`` is ignored) beside three different cells."""
    _check(name, channels, 0, _device(name, channels))


MESH_CASES = [(n, p, c) for n in ("anisotropic", "small_mesh", "unwrapped", "mixed") for p in (2, 5) for c in (3, 33)]


@pytest.mark.parametrize("name,nodes,channels", MESH_CASES, ids=[f"{n}-p{p}-C{c}" for n, p, c in MESH_CASES])
def test_p3m_against_the_oracle(name, nodes, channels):
    """The filter's tangent on an 8 x 16 x 4 mesh of a sheared left-handed cell, on N = 4 < p, with wrapped weights, and beside
    an open and an empty system; both parities of the stencil; C = 33: a partly filled chunk of 8."""
    _check(name, channels, nodes, _device(name, channels, nodes))


@pytest.mark.parametrize("nodes", [0, 5], ids=["ewald", "p3m"])
@pytest.mark.parametrize("parts", list(PARTS.values()), ids=list(PARTS))
def test_each_cotangent_alone(parts, nodes):
    name = "mixed"
    op, graph = _shared(name, nodes)
    got = _run(op, graph, _inputs(name, 24, nodes), parts)
    _check(name, 24, nodes, got, parts, label=f"second_cell {name} p={nodes} C=24 parts={parts}")
    if parts == PARTS["u_charges alone"]:
        assert float(got[0].abs().max()) == 0.0  # (D A) g without a direction


def test_all_cotangents_missing_and_no_result_are_refused():
    from metatrain_amd._lib import PetHipError

    op, graph = _shared("mixed")
    pos, q, gv, u_q, u_r, u_c = _inputs("mixed", 24)
    with pytest.raises(PetHipError, match="all None"):
        op.second_cell(graph, pos, q, gv)
    with pytest.raises(PetHipError, match="at least one"):
        op.second_cell(graph, pos, q, gv, u_q, u_r, u_c, results=(False, False))


@pytest.mark.parametrize("nodes", [0, 5], ids=["ewald", "p3m"])
def test_a_selection_has_the_bits_of_the_full_call(nodes):
    op, graph = _shared("mixed", nodes)
    full = _device("mixed", 24, nodes)
    for k, results in enumerate([(True, False), (False, True)]):
        got = _run(op, graph, _inputs("mixed", 24, nodes), results=results)
        assert got[1 - k] is None and torch.equal(got[k], full[k]), results


@pytest.mark.parametrize("nodes", [0, 5], ids=["ewald", "p3m"])
def test_zero_cell_direction_and_open_systems_give_the_bits_of_second(nodes):
    """``u_cells`` of zeros: ``second``'s two results, bit for bit (u' = u exactly, the weights' and the filter's tangent add
    zeros). ``open_tiles`` (no periodic system) with any ``u_cells``: the same."""
    op, graph = _shared("mixed", nodes)
    pos, q, gv, u_q, u_r, u_c = _inputs("mixed", 24, nodes)
    got = op.second_cell(graph, pos, q, gv, u_q, u_r, torch.zeros_like(u_c))
    want = op.second(graph, pos, q, gv, u_q, u_r)
    assert _equal(got, want[:2])
    b = ec.batch("open_tiles")
    op, graph = _mesh(None, nodes, ec.case("open_tiles").systems) if nodes else _shared("open_tiles")
    dev = torch.device(DEV)
    q, gv = ec.charges("open_tiles", 3)
    u_q, u_r, _ = co.cotangents(b, 3)
    any_cells = torch.randn(len(b["pbcs"]), 3, 3, generator=torch.Generator().manual_seed(5))
    args = tuple(t.float().to(dev) for t in (b["positions"], q, gv, u_q, u_r))
    got = op.second_cell(graph, *args, any_cells.to(dev))
    assert _equal(got, op.second(graph, *args)[:2])


@pytest.mark.parametrize("nodes", [0, 5], ids=["ewald", "p3m"])
def test_a_second_call_gives_the_same_bits(nodes):
    op, graph = _shared("mixed", nodes)
    assert _equal(_run(op, graph, _inputs("mixed", 24, nodes)), _device("mixed", 24, nodes))


def test_a_system_alone_gives_the_bits_of_its_rows_in_the_batch():
    """The 33-atom system of ``periodic_tiles`` (Ewald, C = 260) and the triclinic 43-atom cell of the mesh ``mixed`` (p = 5,
    C = 24), each planned and run alone with its own row of ``u_cells``."""
    b = ec.batch("periodic_tiles")
    rows = slice(b["first_atom"][2], b["first_atom"][3])
    assert rows.stop - rows.start == 33
    ew, graph = _ewald("periodic_tiles", [ec.case("periodic_tiles").systems[2]])
    alone = _run(ew, graph, _inputs("periodic_tiles", 260, 0, rows, slice(2, 3)))
    assert _equal(alone, tuple(t[rows] for t in _device("periodic_tiles", 260)))
    b = pc.batch("mixed")
    rows = slice(b["first_atom"][0], b["first_atom"][1])
    assert rows.stop - rows.start == 43
    op, graph = _mesh("mixed", 5, [pc.case("mixed").systems[0]])
    alone = _run(op, graph, _inputs("mixed", 24, 5, rows, slice(0, 1)))
    assert _equal(alone, tuple(t[rows] for t in _device("mixed", 24, 5)))


@pytest.mark.parametrize("nodes", [0, 5], ids=["ewald", "p3m"])
def test_backward_and_second_are_untouched_by_a_cell_call(nodes):
    """``backward`` and ``second`` before and after ``second_cell`` on one handle: identical bits."""
    name = "mixed"
    op, graph = _mesh(name, nodes) if nodes else _ewald(name)
    inputs = _inputs(name, 24, nodes)
    pos, q, gv, u_q, u_r, u_c = inputs
    before = op.backward(graph, pos, q, gv, want_cell_grad=True) + tuple(op.second(graph, pos, q, gv, u_q, u_r))
    _run(op, graph, inputs)
    after = op.backward(graph, pos, q, gv, want_cell_grad=True) + tuple(op.second(graph, pos, q, gv, u_q, u_r))
    assert _equal(before, after)


def test_hook_calls_are_those_the_header_states():
    """``include/pet_hip.h``: with ``d_u_cells``, 4 hook calls per result formed (two transform pairs), 8 for both, whichever of
    ``u_q`` / ``u_r`` are given; the filter's tangent adds none."""
    op, graph = _mesh("mixed", 5)
    inputs = _inputs("mixed", 24, 5)
    for parts in (ALL, PARTS["u_positions alone"], PARTS["u_cells alone"]):
        for results, want in (((True, True), 8), ((True, False), 4), ((False, True), 4)):
            before = op.transform_calls
            _run(op, graph, inputs, parts, results)
            print(f"(hook calls, parts {parts}, results {results}, {op.transform_calls - before})")
            assert op.transform_calls - before == want, (parts, results)
