"""The adaptive cutoff (``num_neighbors_adaptive``, methods "solver" and "grid") at its row, clamp, plateau and probe-count edges:
the cases of ``adaptive_cases.py`` (premises: ``test_adaptive_cases_cpu.py``) on the device against the fp64 oracle
``oracle/pet.py``.

  1. graph        ``export_batch()`` against ``batch_tensors``: integer keys bit-exact, the atomic cutoffs, cutoff factors, edge
                  vectors and distances; ``plateau`` against its closed form, ``lower_clamp`` exactly rc / 16;
  2. first order  per-atom energies, dE/dR and dE/dcell against fp64 autograd: the tuned pass under the default policy and with
                  ``trr = 0``, one size-generic model (the ``s64_adaptive`` sizes) on ``rows`` and ``thin_cells``;
  3. second order ``backward_train2``: the force-loss parameter gradients and the tangent identity on ``rows_small`` and
                  ``thin_cells``;
  4. probe counts the grid method at the widths where float32 hypers count one probe too many, and the refusals;
  5. repeatability a second build and pass give the same bits; a system alone gives the bits of its rows in the batch.

Bars. Every bar is ``max(floor, 3 y)`` with y the same error figure of the oracle evaluated by torch in fp32 on the same inputs
(never the device's own output): floor 3e-6 for the atomic cutoffs (relative, per atom), 1e-5 for energies, dE/dR, dE/dcell
(per cluster or system: ``cluster_errors`` of ``test_gpu_attn_token_edges.py``) and for the parameter gradients (per key,
``max |got - ref| / max |ref|``). Cutoff factors, vectors and distances: the tolerances of
``test_adaptive_cutoff_matches_reference``. Every ``(case, quantity, y, device error)`` is printed before it is asserted; the
figures of one run are in DESIGN.md.

The switches a test needs are set here and restored in ``try / finally``."""
import functools

import numpy as np
import pytest
import torch

import adaptive_cases as A
from _memo import memo_oracle
from oracle import pet as opet
from test_gpu_attn_token_edges import cluster_errors

pytestmark = pytest.mark.gpu
TOL = 1e-5
TOL_CUTOFF = 3e-6
TYPES = A.TYPES
INT_KEYS = ["element_indices_nodes", "element_indices_neighbors", "padding_mask", "reverse_neighbor_index",
            "centers", "neighbors", "nef_to_edges_neighbor", "cell_shifts"]
S64 = dict(d_pet=64, d_node=128, d_feedforward=128, d_head=64, num_heads=4)  # test_gpu_gen_train.py "s64_adaptive"
SIZES = {"default": {}, "s64": S64}
FIRST_ORDER = [c for c in A.GEOMETRIC if c != "rows_small"]  # (rows holds the same clusters)
SECOND_ORDER = ["rows_small", "thin_cells"]
CASE_METHOD = pytest.mark.parametrize("case,method", [(c, m) for c in A.GEOMETRIC for m in A.METHODS])


def _hypers(case, method, size="default"):
    return A.hypers(case, method, **SIZES[size])


def _params(case, method, size="default"):
    return opet.synthetic_params(_hypers(case, method, size), TYPES, {"energy": 1}, 0, torch.float32)


def _seed_vector(n):
    return torch.rand(n, generator=torch.Generator().manual_seed(7)) + 0.5


def _dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _model_for(target, width, method, size):
    """one device model per distinct hypers (the cases share target 12 / width 1 but for ``lower_clamp``)"""
    from metatrain_amd import runtime as rt

    hypers = dict(opet.DEFAULT_HYPERS, num_neighbors_adaptive=target, adaptive_cutoff_method=method,
                  cutoff_width_adaptive=width, **SIZES[size])
    model = rt.HipModel(hypers, TYPES)
    params = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    model.load({k: v.to(_dev()) for k, v in params.items()}, "energy")
    return model


def _model(case, method, size="default"):
    spec = A.SPECS[case]
    return _model_for(spec.target, spec.width, method, size)


def _graph_of(model, s):
    from metatrain_amd import runtime as rt

    dev = _dev()
    return rt.HipGraph(model, s.positions.to(dev), s.cells.to(dev), s.centers.to(dev), s.neighbors.to(dev),
                       s.cell_shifts.to(dev), s.species.to(dev), s.system_indices.int().to(dev))


def _graph(case, method, size="default"):
    return _graph_of(_model(case, method, size), A.system(case))


def _bar(floor, y):
    return max(floor, 3.0 * y)


def _relative(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


# ---- 1. the graph ------------------------------------------------------------------------------------------------------------
def _cutoff_errors(case, method, got):
    """(y, device error): largest per-atom relative error of the fp32 oracle's and of the device's cutoffs"""
    r64 = A.cutoffs(case, method)
    y = float((np.abs(A.cutoffs(case, method, torch.float32) - r64) / r64).max())
    e = float((np.abs(np.asarray(got, np.float64) - r64) / r64).max())
    return y, e


@CASE_METHOD
def test_graph_against_the_oracle(case, method):
    b = A.batch(case, method)
    out = {k: v.cpu().numpy() for k, v in _graph(case, method).export_batch().items()}
    y, e = _cutoff_errors(case, method, out["atomic_cutoffs_stats"])
    print(f"adaptive-edges: {case} {method}  cutoffs  fp32 oracle {y:.2e}  device {e:.2e}  "
          f"kept {len(b['centers'])} of {len(A.system(case).centers)} edges")
    for k in INT_KEYS:
        assert out[k].dtype == b[k].dtype and out[k].shape == b[k].shape, k
        assert np.array_equal(out[k], b[k]), f"{k} is not bit-exact"
    assert e <= _bar(TOL_CUTOFF, y), (e, y)
    np.testing.assert_allclose(out["cutoff_factors"], b["cutoff_factors"], rtol=2e-4, atol=3e-6)
    for k in ("edge_vectors", "edge_distances"):
        np.testing.assert_allclose(out[k], b[k], rtol=2e-6, atol=2e-6, err_msg=k)
    if method == "solver" and case == "plateau":
        root = A.CUTOFF * 12.0 ** (-1.0 / 3.0)
        closed = float(np.abs(out["atomic_cutoffs_stats"].astype(np.float64) - root).max() / root)
        print(f"adaptive-edges: plateau solver  cutoffs against rc 12^(-1/3) = {root:.5f} A: {closed:.2e}")
        assert closed <= _bar(TOL_CUTOFF, y)
    if method == "solver" and case == "lower_clamp":
        assert (out["atomic_cutoffs_stats"] == np.float32(A.CUTOFF / 16.0)).all()
    if method == "solver":  # an atom without any input edge: the root is rc itself
        alone = A.all_edge_rows(A.system(case)) == 0
        assert (A.cutoffs(case, "solver")[alone] == A.CUTOFF).all()


# ---- 2. first order ----------------------------------------------------------------------------------------------------------
@memo_oracle
def _oracle_first_order(case, method, size, dtype):
    """(per-atom energies, d(sum_i w_i e_i)/dR, .../dcell) of the oracle in ``dtype``, as fp64 arrays"""
    s = A.system(case)
    p = {k: (v if k == "species_to_species_index" else v.to(dtype)) for k, v in _params(case, method, size).items()}
    pos = s.positions.to(dtype).clone().requires_grad_(True)
    cells = s.cells.to(dtype).clone().requires_grad_(True)
    a = opet.pet_atomic_energies(p, _hypers(case, method, size), pos, cells, s.centers, s.neighbors, s.cell_shifts, s.species,
                                 s.system_indices, "energy")[:, 0]
    g, gc = torch.autograd.grad((a * _seed_vector(len(a)).to(dtype)).sum(), [pos, cells], allow_unused=True)
    gc = torch.zeros_like(cells) if gc is None else gc
    return a.detach().double().numpy(), g.double().numpy(), gc.double().numpy().reshape(-1, 9)


def _run(model, s, w=None):
    """a fresh graph, forward, dE/dR and dE/dcell of sum_i w_i e_i: (cutoffs, energies, dE/dR, dE/dcell) as numpy arrays"""
    from metatrain_amd import runtime as rt

    graph = _graph_of(model, s)
    fw = rt.HipForward(model, graph)
    atomic = fw.forward().clone()
    w = _seed_vector(len(s.species)) if w is None else w
    grad, gcell = fw.backward(w.to(_dev()), want_cell_grad=True)
    torch.cuda.synchronize()
    stats = graph.export_batch()["atomic_cutoffs_stats"]
    return (stats.cpu().numpy(), atomic.cpu().numpy().reshape(-1), grad.cpu().numpy(), gcell.cpu().numpy().reshape(-1, 9))


@functools.lru_cache(maxsize=None)
def _device(case, method, size, policy):
    """Two builds and passes of the case under the switches ``policy`` (a tuple of items): the first one's arrays and whether
    the second gave the same bits. Cached: the tests below look at the same run from several sides."""
    from metatrain_amd import runtime as rt

    model = _model(case, method, size)
    try:
        for k, v in policy:
            rt.config_set(k, v)
        first, second = _run(model, A.system(case)), _run(model, A.system(case))
    finally:
        for k, _ in policy:
            rt.config_set(k, {"trr": 1}[k])
    return first, all(np.array_equal(a, b) for a, b in zip(first, second))


def _check_first_order(case, method, size, tag, got):
    """Print every (case, group, quantity, fp32-oracle error, device error), then assert the bars."""
    s = A.system(case)
    ref, f32 = _oracle_first_order(case, method, size, torch.float64), _oracle_first_order(case, method, size, torch.float32)
    _, atomic, grad, gcell = got
    assert np.isfinite(atomic).all() and np.isfinite(grad).all() and np.isfinite(gcell).all()
    systems = np.arange(len(s.cells))
    rows, bad = [], []
    for what, dev, r, f, groups, names in (("energy", atomic, ref[0], f32[0], s.group, s.labels),
                                           ("dE/dR", grad, ref[1], f32[1], s.group, s.labels),
                                           ("dE/dcell", gcell, ref[2], f32[2], systems, ["system %d" % k for k in systems])):
        if not r.any():  # (an open system's cell enters nothing)
            assert not dev.any(), f"{what} of {case} is exactly zero in the oracle"
            continue
        y, e = cluster_errors(f, r, groups), cluster_errors(dev, r, groups)
        for k, name in enumerate(names):
            rows.append((f"{case} {method}{tag}", name, what, y[k], e[k]))
            if not e[k] <= _bar(TOL, y[k]):
                bad.append(rows[-1])
    for r in rows:
        print("adaptive-edges: %s  %-10s  %-8s  fp32 oracle %.2e  device %.2e" % r)
    assert not bad, f"beyond max(1e-5, 3 x fp32 oracle): {bad}"
    if case == "thin_cells":  # every edge of the one-atom cell is a self-image: no position enters its energy
        assert not ref[1][0].any() and not grad[0].any(), grad[0]
        assert np.abs(ref[2][0]).max() > 1e-3  # ... while its cell does, through the vectors AND the cutoff
    alone = A.all_edge_rows(s) == 0
    assert not grad[alone].any()


@pytest.mark.parametrize("policy", [(), (("trr", 0),)], ids=["default", "trr=0"])
@pytest.mark.parametrize("case,method", [(c, m) for c in FIRST_ORDER for m in A.METHODS])
def test_first_order_on_the_tuned_pass(case, method, policy):
    got, same = _device(case, method, "default", policy)
    _check_first_order(case, method, "default", " trr=0" if policy else "", got)
    assert same, "a second build and pass differ"


@pytest.mark.parametrize("case", ["rows", "thin_cells"])
def test_first_order_on_the_size_generic_pass(case):
    got, same = _device(case, "solver", "s64", ())
    _check_first_order(case, "solver", "s64", " s64", got)
    assert same, "a second build and pass differ"


# ---- 3. second order ---------------------------------------------------------------------------------------------------------
def _direction(n):
    return torch.randn(n, 3, generator=torch.Generator().manual_seed(2))


@memo_oracle
def _oracle_second_order(case, method, dtype):
    """d<u, dE/dR>/dtheta per parameter key and dE/dR of the oracle in ``dtype`` (fp64 tensors)"""
    s = A.system(case)
    p = {k: (v if k == "species_to_species_index" else v.to(dtype).clone().requires_grad_(True))
         for k, v in _params(case, method).items()}
    pos = s.positions.to(dtype).clone().requires_grad_(True)
    a = opet.pet_atomic_energies(p, _hypers(case, method), pos, s.cells.to(dtype), s.centers, s.neighbors, s.cell_shifts,
                                 s.species, s.system_indices, "energy")[:, 0]
    (g,) = torch.autograd.grad(a.sum(), pos, create_graph=True)
    keys = [k for k in p if k != "species_to_species_index"]
    grads = torch.autograd.grad((_direction(len(a)).to(dtype) * g).sum(), [p[k] for k in keys], allow_unused=True)
    return {k: gr.double() for k, gr in zip(keys, grads) if gr is not None}, g.detach().double()


def _worst_key(got, ref):
    worst = ("", 0.0)
    for k, r in ref.items():
        scale = float(r.abs().max())
        if scale > 1e-12:
            e = float((got[k].double() - r).abs().max()) / scale
            worst = max(worst, (k, e), key=lambda t: t[1])
    return worst


@pytest.mark.parametrize("method", A.METHODS)
@pytest.mark.parametrize("case", SECOND_ORDER)
def test_second_order_parameter_gradients_and_tangent(case, method):
    """As ``test_adaptive_cutoff_cell_gradient_and_second_order``: the tangents of the cutoffs (so.hip k_adapt_rdot /
    k_adapt_rdot_grid) carry d<u, dE/dR>/dtheta; the tangent energies sum to <u, dE/dR>."""
    from metatrain_amd import runtime as rt

    dev = _dev()
    s = A.system(case)
    n = len(s.species)
    model = _model(case, method)
    fw = rt.HipForward(model, _graph(case, method), train=True)
    fw.forward()
    ones = torch.ones(n, device=dev)
    grad = fw.backward(ones)
    u = _direction(n)
    model.zero_grad()
    tan = fw.backward_train2(ones, None, u.to(dev), want_tangent=True)
    got = {k: v.cpu() for k, v in model.grads().items()}
    ref, g64 = _oracle_second_order(case, method, torch.float64)
    f32, g32 = _oracle_second_order(case, method, torch.float32)
    y_g, e_g = _relative(g32.numpy(), g64.numpy()), _relative(grad.cpu().numpy(), g64.numpy())
    (ky, y), (ke, e) = _worst_key(f32, ref), _worst_key(got, ref)
    lhs, rhs = float(tan.double().sum()), float((u.to(dev).double() * grad.double()).sum())
    print(f"adaptive-edges: {case} {method}  dE/dR  fp32 oracle {y_g:.2e}  device {e_g:.2e}")
    print(f"adaptive-edges: {case} {method}  force-loss parameter gradients  fp32 oracle {y:.2e} ({ky})  device {e:.2e} ({ke})")
    print(f"adaptive-edges: {case} {method}  sum of tangent energies {lhs:.6e}  <u, dE/dR> {rhs:.6e}")
    assert e_g <= _bar(TOL, y_g)
    assert abs(lhs - rhs) < 1e-4 * max(1.0, abs(rhs))
    assert e <= _bar(TOL, y), (ke, e, y)


# ---- 4. probe counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff,width,probes", [p for p in A.PROBE_COUNTS if p[2] is not None])
def test_grid_probe_counts_follow_the_reference(cutoff, width, probes):
    """The probe grid is ``torch.arange(0.5, cutoff, width / 4)``, counted from Python doubles: 25 probes at width 0.64 and 50 at
    0.32, where the same formula on float32 hypers counts 26 and 51 (one probe more moves these cutoffs by up to 0.1 A)."""
    from metatrain_amd import runtime as rt

    s = A.system("rows_small")
    hypers = dict(opet.DEFAULT_HYPERS, cutoff=cutoff, num_neighbors_adaptive=12.0, adaptive_cutoff_method="grid",
                  cutoff_width_adaptive=width)
    assert A.reference_probe_count(cutoff, width) == probes
    model = rt.HipModel(hypers, TYPES)
    model.load_species_table()
    got = _graph_of(model, s).export_batch()["atomic_cutoffs_stats"].cpu().numpy().astype(np.float64)
    r = {}
    for dtype in (torch.float64, torch.float32):
        _, d = opet.edge_geometry(s.positions.to(dtype), s.cells.to(dtype), s.centers, s.neighbors, s.cell_shifts,
                                  s.system_indices)
        r[dtype] = opet.adaptive_cutoffs_grid(s.centers, d, 12.0, len(s.species), cutoff, width).double().numpy()
    y = float((np.abs(r[torch.float32] - r[torch.float64]) / r[torch.float64]).max())
    e = float((np.abs(got - r[torch.float64]) / r[torch.float64]).max())
    print(f"adaptive-edges: probes ({cutoff}, {width}) = {probes}  cutoffs  fp32 oracle {y:.2e}  device {e:.2e}")
    assert e <= _bar(TOL_CUTOFF, y), (e, y)


@pytest.mark.parametrize("cutoff,width", [p[:2] for p in A.PROBE_COUNTS if p[2] is None])
def test_unserved_probe_counts_are_refused_by_name(cutoff, width):
    """67 probes (more than the 64 that are built) and 1 probe: ``PET_ERR_UNSUPPORTED`` from ``pet_model_create``, a host call
    without a stream -- before any graph is built or any kernel launched."""
    from metatrain_amd import _lib
    from metatrain_amd import runtime as rt

    hypers = dict(opet.DEFAULT_HYPERS, cutoff=cutoff, num_neighbors_adaptive=12.0, adaptive_cutoff_method="grid",
                  cutoff_width_adaptive=width)
    assert not 2 <= A.reference_probe_count(cutoff, width) <= A.GRID_MAX_PROBES
    with pytest.raises(_lib.PetHipError, match=f"error {_lib.PET_ERR_UNSUPPORTED}: .*probe cutoffs"):
        rt.HipModel(hypers, TYPES)
    rt.HipModel(dict(hypers, adaptive_cutoff_method="solver"), TYPES)  # the solver has no probes


# ---- 5. repeatability --------------------------------------------------------------------------------------------------------
def _alone(s, k):
    """system ``k`` of the batch as a batch of its own"""
    atoms = np.nonzero(s.system_indices.numpy() == k)[0]
    first = int(atoms[0])
    e = np.nonzero(s.system_indices.numpy()[s.centers.numpy()] == k)[0]
    return A.System(s.positions[atoms], s.cells[k:k + 1], s.centers[e] - first, s.neighbors[e] - first, s.cell_shifts[e],
                    s.species[atoms], torch.zeros(len(atoms), dtype=torch.long), s.group[atoms], s.labels), atoms


@pytest.mark.parametrize("method", A.METHODS)
def test_a_system_alone_gives_the_bits_of_its_rows_in_the_batch(method):
    s = A.system("thin_cells")
    (stats, atomic, grad, _), same = _device("thin_cells", method, "default", ())
    assert same
    w = _seed_vector(len(s.species))
    for k in sorted(set(s.system_indices.tolist())):
        sub, atoms = _alone(s, k)
        stats_k, atomic_k, grad_k, _ = _run(_model("thin_cells", method), sub, w[atoms])  # the batch's seeds of these atoms
        for what, a, b in (("cutoffs", stats_k, stats[atoms]), ("energies", atomic_k, atomic[atoms]),
                           ("dE/dR", grad_k, grad[atoms])):
            assert np.array_equal(a, b), f"system {k} alone: {what} differ from its rows in the batch"
