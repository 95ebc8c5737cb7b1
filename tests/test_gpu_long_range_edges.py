"""GPU tests of the long-range (Ewald) operator (``csrc/ewald.hip``) at its tile, channel, cell and open-system edges: the
cases of ``tests/ewald_cases.py`` against the fp64 oracle of the definition (``tests/_ewald_oracle.py``), two identities on
device results alone (supercell, Madelung) and the whole model on a batch of open and periodic systems, moved as MD moves it.

Bar, per SYSTEM and quantity: with ``err``, ``e32`` and ``scale`` the maxima of ``|got - oracle|``, ``|oracle_fp32 - oracle|`` and
``|oracle|`` over the rows of one system (its atoms; for dL/dcell its 3 x 3 block), ``err <= max(1e-5 scale, 2 e32)``: the bar
of ``test_gpu_long_range.py`` with every maximum taken per system, so that an error confined to a small system is not
measured against a large one's magnitudes. Where a quantity vanishes by symmetry on a system (``scale`` below 1e-9 of the
batch-wide one) the batch-wide scale takes its place, and the printed line says so. Every test prints
``(case, system, quantity, e32, relmax)`` before it asserts; the measured table is in DESIGN.md section 18."""
import pytest
import torch

import _ewald_oracle as eo
import ewald_cases as ec
import test_gpu_long_range as base

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _device_run(name, channels, ew_and_graph=None):
    dev = torch.device(DEV)
    c, b = ec.case(name), ec.batch(name)
    q, gv = ec.charges(name, channels)
    if ew_and_graph is None:
        _, graph, ew = ec.operator(b, dev, c.smearing, c.resolution, c.cutoff)
    else:
        ew, graph = ew_and_graph
    return ew, graph, ec.run(ew, graph, b, q, gv, dev)


def _check_case(name, channels, got, label=None):
    b = ec.batch(name)
    ec.check_per_system(label or f"{name} C={channels}", b, ec.QUANTITIES, ec.KINDS, got,
                        ec.reference(name, channels, torch.float64), ec.reference(name, channels, torch.float32))
    for s, pbc in enumerate(b["pbcs"]):
        if not any(pbc):
            assert float(got[3][s].abs().max()) == 0.0, (name, s, "dL/dcell of an open system")


def test_mixed_batch_per_system():
    """The batch of ``test_operator_on_a_mixed_batch`` at C = 24 under the per-system bar: the 1-atom cell and the 17-atom
    cluster measured against their own magnitudes, not the 130-atom cell's."""
    _, _, got = _device_run("mixed", 24)
    _check_case("mixed", 24, got)


@pytest.mark.parametrize("name", ec.OPERATOR_CASES)
def test_operator_case(name):
    """Every case of ``ewald_cases`` at C = 24: potential and the three adjoints, per system."""
    ew, _, got = _device_run(name, 24)
    if name == "elongated_limit":
        assert ew.num_kvectors(0) == 5914
    if name == "periodic_tiles":
        assert ew.num_kvectors(3) == 56 and ew.num_kvectors(1) == ew.num_kvectors(0) > 1000
    if name == "open_tiles":
        assert all(ew.num_kvectors(s) == 0 for s in range(5))
    _check_case(name, 24, got)


@pytest.mark.parametrize("channels", [3, 33, 100, 260, 388])
@pytest.mark.parametrize("name", ["open_tiles", "periodic_tiles"])
def test_channel_widths(name, channels):
    """C = 3: scalar loads whose [g | q] boundary falls inside a group of four; 33: one column in the second half-wave; 100: a
    partly active second wave; 260: a second grid row with four channels; 388: a second grid row that reaches past channel
    384 (at 260 a row stride of 128 in place of 256 still writes every channel, twice: the second row then covers 128..383)."""
    _, _, got = _device_run(name, channels)
    _check_case(name, channels, got)


def test_inputs_that_start_four_bytes_into_an_allocation():
    """C = 24 (C % 4 == 0) with charges and dL/dV contiguous views one float into a larger allocation: ``k_ew_force`` must take
    its scalar loads. Same bar; whether the bits equal the aligned run is printed, not asserted."""
    dev = torch.device(DEV)
    name, channels = "periodic_tiles", 24
    b = ec.batch(name)
    ew, graph, aligned = _device_run(name, channels)
    pos = b["positions"].float().to(dev)
    views = []
    for t in ec.charges(name, channels):
        store = torch.zeros(t.numel() + 8, dtype=torch.float32, device=dev)
        view = store[1:1 + t.numel()].view(t.shape)
        view.copy_(t.float())
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        views.append(view)
    v = ew.potential(graph, pos, views[0])
    got = (v,) + tuple(ew.backward(graph, pos, views[0], views[1], want_cell_grad=True))
    print("bit for bit equal to the aligned run:", {n: torch.equal(x, y) for n, x, y in zip(ec.QUANTITIES, got, aligned)})
    _check_case(name, channels, got, label=f"{name} C={channels} misaligned")


def test_a_workspace_larger_than_needed_is_reused():
    """One ``EwaldHip``: C = 260 first, then C = 3 on the same plan and workspace."""
    ew, graph, wide = _device_run("periodic_tiles", 260)
    nbytes = ew._workspace.numel()
    _, _, narrow = _device_run("periodic_tiles", 3, (ew, graph))
    assert ew._workspace.numel() == nbytes > int(ew.lib.pet_ewald_workspace_bytes(ew.handle, 3))
    _check_case("periodic_tiles", 260, wide)
    _check_case("periodic_tiles", 3, narrow, label="periodic_tiles C=3 after C=260")


def test_supercell_halves_equal_the_primitive_cell_on_the_device():
    """Potential, dL/dq and dL/dR of each half of the 2 x 1 x 1 supercell against the primitive cell's DEVICE result: another
    k-set, other weights and other tiles must give the same numbers. Each side is within one per-system bar of the truth, so
    the two are within the sum of their bars. (Not dL/dcell: at fixed Cartesian positions the replicas do not move with the
    cell.)"""
    _, _, got = _device_run("supercell", 24)
    b = ec.batch("supercell")
    ref, f32 = ec.reference("supercell", 24, torch.float64), ec.reference("supercell", 24, torch.float32)
    bad = []
    for name, g, r, y in zip(ec.QUANTITIES[:3], got, ref, f32):
        g = g.cpu().double()
        bar0, scale, e0, _ = ec.system_bar(r, y, ec.system_rows(b, "atom", 0))
        bar1, _, e1, _ = ec.system_bar(r, y, ec.system_rows(b, "atom", 1))
        for half, rows in enumerate((slice(43, 86), slice(86, 129))):
            err = float((g[rows] - g[:43]).abs().max())
            print(f"(supercell half {half} against primitive, 1, {name}, {(e0 + e1) / scale:.2e}, {err / scale:.2e})")
            if not err <= bar0 + bar1:
                bad.append((name, half, err / scale))
    assert not bad, bad


def test_madelung_constant_from_the_device_potential():
    """NaCl, nearest distance 1, charges +-1, sigma = 0.5, |k| <= 9 / sigma, R = 1.5: the device potential at C = 1 plus, on the
    host in fp64, the exclusion term over the graph's own edges and the real-space erfc sum is P (-1.7475646) at the origin.
    Independent of the oracle's k-space code."""
    _, _, got = _device_run("nacl", 1)
    want = eo.PREFACTOR * ec.MADELUNG_NACL
    value = ec.madelung_composition(got[0])
    e32 = abs(ec.madelung_composition(None, torch.float32) - want) / abs(want)
    err = abs(value - want) / abs(want)
    print(f"(nacl, 0, madelung {value / eo.PREFACTOR:.8f}, {e32:.2e}, {err:.2e})")
    assert err <= max(1e-5, 2.0 * e32)


# ---- the whole model ---------------------------------------------------------------------------------------------------------
MODEL_NAMES = ("atomic", "energies", "grad", "cell_grad")
MODEL_KINDS = ("atom", "system", "atom", "system")


def _model_graph(model, b, dev):
    from metatrain_amd import runtime as rt

    return rt.HipGraph(model, b["positions"].float().to(dev), b["cells"].float().to(dev), b["centers"].to(dev),
                       b["neighbors"].to(dev), b["cell_shifts"].to(dev), b["species"].to(dev),
                       b["system_indices"].int().to(dev))


def _check_model(label, b, got, hypers, params, lr_params):
    ref = base._model_reference(params, lr_params, hypers, b, torch.float64)
    f32 = base._model_reference(params, lr_params, hypers, b, torch.float32)
    ec.check_per_system(label, b, MODEL_NAMES, MODEL_KINDS, got, ref[:4], f32[:4])
    for s in (0, 2):
        assert float(got[3][s].abs().max()) == 0.0, (label, s, "dE/dcell of an open system")


def test_model_on_open_and_periodic_systems_and_after_an_md_step():
    """Default hypers (tuned path) on one batch of a 40-atom open cluster, a 64-atom periodic box and a QM9 frame; then the
    MD pattern: every atom moved by up to 0.05 A, one atom of the box across a cell face, a new graph with the same cells and
    layout, and ``replan=False`` equal to ``replan=True`` bit for bit."""
    from metatrain_amd import long_range as lr
    from metatrain_amd import runtime as rt

    dev = torch.device(DEV)
    hypers, params, lr_params = base._model_case("default")
    b, moved = ec.model_batch(False), ec.model_batch(True)
    assert b["pbcs"] == [[False] * 3, [True] * 3, [False] * 3] and b["first_atom"][:3] == [0, 40, 104]
    assert b["first_atom"] == moved["first_atom"] and torch.equal(b["cells"], moved["cells"])
    assert float((moved["positions"] - b["positions"]).norm(dim=1).max()) <= 0.05 + 1e-12
    a, length = 40 + ec.FACE_ATOM, float(b["cells"][1, 0, 0])
    assert length - 0.02 < float(b["positions"][a, 0]) < length < float(moved["positions"][a, 0])  # it crossed the face
    model = rt.HipModel(hypers, eo.TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    feat = lr.LongRangeFeaturizerHip.from_state_dict(hypers, lr_params, device=dev)
    got = lr.energy_and_gradient(model, feat, _model_graph(model, b, dev), b["pbcs"], want_cell_grad=True)
    _check_model("model open+periodic", b, got, hypers, params, lr_params)
    graph = _model_graph(model, moved, dev)
    kept = lr.energy_and_gradient(model, feat, graph, moved["pbcs"], want_cell_grad=True, replan=False)
    fresh = lr.energy_and_gradient(model, feat, graph, moved["pbcs"], want_cell_grad=True, replan=True)
    assert all(torch.equal(x, y) for x, y in zip(kept, fresh))
    assert not torch.equal(kept[0], got[0])
    _check_model("model after an MD step", moved, kept, hypers, params, lr_params)
