"""GPU tests of the long-range operator's second-order operation (``pet_ewald_second``, ``EwaldHip.second``, double backward
through ``LongRangeFeaturizerHip``) against the fp64 oracle's double backward
(``tests/_ewald_second_oracle.py``), on the cases of ``tests/ewald_cases.py``.

Bar, per SYSTEM and output (``ewald_cases.check_per_system``): ``max|got - ref| <= max(1e-5 max|ref|, 2 max|oracle_fp32 - ref|)``
over the system's rows, the batch-wide scale where an output vanishes by symmetry on a system. All three outputs are per-atom.
Every test prints ``(case, system, quantity, e32, relmax)`` and a ``[worst]`` line per output before it asserts; the measured
table is in DESIGN.md section 20."""
import functools

import pytest
import torch

import _ewald_oracle as eo
import _ewald_second_oracle as so
import ewald_cases as ec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOTH, ONLY_CHARGES, ONLY_POSITIONS = (True, True), (True, False), (False, True)


def _operator(name, systems=None):
    c = ec.case(name)
    b = ec.batch(name) if systems is None else eo.collate(systems, c.cutoff)
    _, graph, ew = ec.operator(b, torch.device(DEV), c.smearing, c.resolution, c.cutoff)
    return ew, graph, b


@functools.lru_cache(maxsize=None)
def _shared(name):
    """One graph and one planned operator per case, for the tests that do not look at the handle's state."""
    return _operator(name)


def _inputs(name, channels, rows=slice(None)):
    dev = torch.device(DEV)
    q, gv = ec.charges(name, channels)
    u_q, u_r = so.cotangents(name, channels)
    pos = ec.batch(name)["positions"]
    return tuple(t[rows].float().to(dev) for t in (pos, q, gv, u_q, u_r))


def _second(ew, graph, inputs, halves=BOTH):
    pos, q, gv, u_q, u_r = inputs
    return ew.second(graph, pos, q, gv, u_q if halves[0] else None, u_r if halves[1] else None)


def _check(name, channels, got, halves=BOTH, label=None):
    ec.check_per_system(label or f"second {name} C={channels}", ec.batch(name), so.NAMES, so.KINDS, got,
                        so.reference(name, channels, torch.float64, halves), so.reference(name, channels, torch.float32, halves))


@functools.lru_cache(maxsize=None)
def _device(name, channels):
    ew, graph, _ = _shared(name)
    return _second(ew, graph, _inputs(name, channels))


CASES = ([("periodic_tiles", c) for c in (3, 33, 260)] + [("open_tiles", c) for c in (3, 260)] + [("mixed", 24)]
         + [(n, 3) for n in ("elongated_limit", "sheared", "left_handed", "unwrapped", "other_constants")])


@pytest.mark.parametrize("name,channels", CASES)
def test_second_against_the_oracle(name, channels):
    """``periodic_tiles``: 32 and 33 atoms around an empty system, the 2-atom cell with 28 walked k-vectors and self-image
    edges; C = 33 the loads that are not vectors, C = 260 a second column block. ``open_tiles``: later chunks, several row tiles,
    waves 1-3, a second column round, self-exclusion at a0 > 0. ``mixed``: the 1-atom cell, triclinic 43, cubic 130 with 14 242
    k-vectors beside an open system. ``elongated_limit``: nm = 64, the largest table in LDS beside the new staging.
    ``unwrapped``: k.u against the wrapped tables. ``other_constants``: inv_R, a and w'' at sigma = 1.0, R = 3.0."""
    if name == "elongated_limit":
        assert _shared(name)[0].num_kvectors(0) == 5914
    if name == "mixed":
        assert _shared(name)[0].num_kvectors(2) == 14242
    _check(name, channels, _device(name, channels))


@pytest.mark.parametrize("halves", [ONLY_CHARGES, ONLY_POSITIONS], ids=["u_positions=None", "u_charges=None"])
def test_one_cotangent_alone(halves):
    """``periodic_tiles`` at C = 3 with one cotangent ``None``, against the oracle with that half zero."""
    ew, graph, _ = _shared("periodic_tiles")
    got = _second(ew, graph, _inputs("periodic_tiles", 3), halves)
    _check("periodic_tiles", 3, got, halves, label=f"second periodic_tiles C=3 halves={halves}")
    if halves == ONLY_CHARGES:
        assert float(got[0].abs().max()) == 0.0  # (D_u A) g without a direction


def test_both_cotangents_missing_is_refused():
    from metatrain_amd._lib import PetHipError

    ew, graph, _ = _shared("periodic_tiles")
    pos, q, gv, _, _ = _inputs("periodic_tiles", 3)
    with pytest.raises(PetHipError, match="both None"):
        ew.second(graph, pos, q, gv)
    # (the C entry point says so itself)
    from metatrain_amd import runtime as rt

    out_q, out_g, out_r = torch.empty_like(q), torch.empty_like(q), torch.empty_like(pos)
    ws = torch.empty(int(ew.lib.pet_ewald_second_workspace_bytes(ew.handle, 3)), dtype=torch.uint8, device=q.device)
    rc = ew.lib.pet_ewald_second(ew.handle, graph.handle, rt._ptr(pos), rt._ptr(q), rt._ptr(gv), None, None, 3, rt._ptr(out_q),
                                 rt._ptr(out_g), rt._ptr(out_r), rt._ptr(ws), ws.numel(), rt._stream())
    assert rc != 0


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_second_call_gives_the_same_bits():
    ew, graph, _ = _shared("periodic_tiles")
    again = _second(ew, graph, _inputs("periodic_tiles", 260))
    assert _equal(again, _device("periodic_tiles", 260))


def test_inputs_four_bytes_into_an_allocation_give_the_aligned_bits():
    """C = 260 (C % 4 == 0): every input a contiguous view one float into a larger allocation, so the force-type kernels take
    their scalar loads; the bits are those of the aligned run."""
    dev = torch.device(DEV)
    ew, graph, _ = _shared("periodic_tiles")
    views = []
    for t in _inputs("periodic_tiles", 260):
        store = torch.zeros(t.numel() + 8, dtype=torch.float32, device=dev)
        view = store[1:1 + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        views.append(view)
    assert _equal(_second(ew, graph, tuple(views)), _device("periodic_tiles", 260))


def test_narrow_call_on_the_wide_workspace_gives_its_own_bits():
    """C = 3 on the workspace sized for C = 260 (the per-width cache pointed at it) against C = 3 on its own workspace."""
    ew, graph, _ = _operator("periodic_tiles")
    wide = _second(ew, graph, _inputs("periodic_tiles", 260))
    assert _equal(wide, _device("periodic_tiles", 260))
    own = _second(ew, graph, _inputs("periodic_tiles", 3))
    big = ew._second_workspaces[260]
    assert big.numel() > ew._second_workspaces[3].numel() == int(ew.lib.pet_ewald_second_workspace_bytes(ew.handle, 3))
    ew._second_workspaces[3] = big
    shared = _second(ew, graph, _inputs("periodic_tiles", 3))
    assert ew._second_workspaces[3] is big
    assert _equal(shared, own)
    _check("periodic_tiles", 3, shared, label="second periodic_tiles C=3 on the C=260 workspace")


def test_a_system_alone_gives_the_bits_of_its_rows_in_the_batch():
    """The 33-atom system of ``periodic_tiles`` planned and run alone at C = 260."""
    b = ec.batch("periodic_tiles")
    rows = slice(b["first_atom"][2], b["first_atom"][3])
    assert rows.stop - rows.start == 33
    ew, graph, _ = _operator("periodic_tiles", [ec.case("periodic_tiles").systems[2]])
    alone = _second(ew, graph, _inputs("periodic_tiles", 260, rows))
    assert _equal(alone, tuple(t[rows] for t in _device("periodic_tiles", 260)))


def test_first_order_adjoint_is_untouched_by_a_second_call():
    """``backward`` before and after ``second`` on one handle: identical bits."""
    ew, graph, _ = _operator("periodic_tiles")
    pos, q, gv, u_q, u_r = _inputs("periodic_tiles", 260)
    before = ew.backward(graph, pos, q, gv, want_cell_grad=True)
    ew.second(graph, pos, q, gv, u_q, u_r)
    after = ew.backward(graph, pos, q, gv, want_cell_grad=True)
    assert _equal(before, after)


# ---- torch double backward through the featuriser ----------------------------------------------------------------------------
D_NODE = 24


def _featurizer(method=None):
    from metatrain_amd import long_range as lr

    b = ec.batch("mixed")
    feat = lr.LongRangeFeaturizerHip.from_state_dict(ec.lr_hypers(d_node=D_NODE), eo.featurizer_params(D_NODE), device=torch.device(DEV),
                                                     method=method)
    return feat.plan(b["cells"], b["pbcs"], b["first_atom"])


def _device_loss(feat, cells_require_grad=False):
    dev = torch.device(DEV)
    b = ec.batch("mixed")
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
    """``mixed`` at d_node = C = 24: ``lr = featurizer(x, pos, cells, graph)``, ``F = d (W . lr).sum() / d pos`` under
    ``create_graph``, ``loss = ((F - F*)^2).sum() + (lr^2).sum()``; its gradients with respect to ``x`` and the six featuriser
    tensors against the fp64 featuriser reference. Bar per tensor: ``max(1e-5 max|ref|, 2 max|ref_fp32 - ref|)``."""
    b, c = ec.batch("mixed"), ec.case("mixed")
    got = _device_loss(_featurizer())
    args = (b, eo.featurizer_params(D_NODE)) + so.featurizer_inputs(b, D_NODE) + (c.smearing, c.resolution, c.cutoff)
    ref, f32 = so.featurizer_reference(*args, torch.float64), so.featurizer_reference(*args, torch.float32)
    bad = []
    for name, g, r, y in zip(("x",) + so.PARAM_KEYS, got, ref, f32):
        g = g.detach().cpu().double()
        assert g.shape == r.shape, (name, g.shape, r.shape)
        scale, e32, err = float(r.abs().max()), float((y - r).abs().max()), float((g - r).abs().max())
        print(f"(force loss mixed, {name}, {e32 / scale:.2e}, {err / scale:.2e})")
        if not err <= max(1e-5 * scale, 2.0 * e32):
            bad.append((name, err / scale, e32 / scale))
    assert not bad, bad


def test_cells_that_require_grad_are_refused_in_the_double_backward():
    from metatrain_amd._lib import PetHipError

    with pytest.raises(PetHipError, match="mixed position / cell second derivatives"):
        _device_loss(_featurizer(), cells_require_grad=True)


def test_a_p3m_featurizer_is_refused_in_the_double_backward():
    from metatrain_amd._lib import PetHipError

    with pytest.raises(PetHipError, match="second derivatives through P3M are not built"):
        _device_loss(_featurizer(method="p3m"))
