"""The premises of ``adaptive_cases.py`` (no GPU): every case is what it says. For every geometric case and both methods

  * the list is a full neighbour list of fp32-representable positions, every input edge inside the 4.5 A maximal cutoff;
  * no input edge lies within 1e-4 A of its pair cutoff in the fp64 oracle, the fp32 torch oracle's cutoffs lie within 1e-5 A of
    the fp64 ones (measured: at most 7.2e-7 A) and it keeps the same edges: kept-edge lists may be demanded bit-exact;
  * the solver has converged: ``|n(r) - target| < 1e-9`` at the cutoff it returns -- or, where the clamp to rc / 16 has moved
    the cutoff (``lower_clamp``), at the root before the clamp. (The ten-step loop alone does NOT converge for an atom whose
    root is rc, the isolated atom: f <= 0 at every step, every Newton step overshoots rc, ten bisections end at rc (1 - 2^-11)
    with a residual of 1.8e-2; the implicit-function step behind the loop is one more Newton step, which lands 1.1e-6 A above rc
    and is clamped to exactly rc, where the residual is 0. That is the reference's algorithm, and the device follows it.)

and per case what its name says. The seed table is what the search gives."""
import os
import re

import numpy as np
import pytest
import torch

import adaptive_cases as A
from oracle import pet as opet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metatrain_amd", "csrc")
CASE_METHOD = [(c, m) for c in A.GEOMETRIC for m in A.METHODS]


def test_the_cases_use_the_default_cutoff_and_the_kernels_constants():
    h = opet.DEFAULT_HYPERS
    assert (h["cutoff"], h["cutoff_width"], h["cutoff_function"], h["cutoff_width_adaptive"]) == (A.CUTOFF, 0.5, "Bump", 1.0)
    common = open(os.path.join(CSRC, "common.h")).read()
    assert int(re.search(r"constexpr int GRID_MAX_PROBES = (\d+);", common).group(1)) == A.GRID_MAX_PROBES
    graph = open(os.path.join(CSRC, "graph.hip")).read()
    # the launch shapes the row cases are built for: 16 lanes per atom, 16 atoms per 256-thread workgroup
    assert re.search(r"k_adaptive_solve<<<cdiv\(n_nodes, 16\), 256, 0, st>>>", graph)
    assert re.search(r"k_adaptive_grid<<<cdiv\(n_nodes, 16\), 256, 0, st>>>", graph)
    assert "const float lo = rc * (1.0f / 16.0f);" in graph


@pytest.mark.parametrize("case", A.GEOMETRIC)
def test_every_case_is_a_full_list_of_fp32_positions(case):
    s = A.system(case)
    n = len(s.species)
    assert s.positions.dtype == torch.float32 and s.cells.dtype == torch.float32 and s.positions.shape == (n, 3)
    assert len(s.group) == n == len(s.system_indices) and set(s.group) == set(range(len(s.labels)))
    assert (np.diff(s.system_indices.numpy()) >= 0).all() and int(s.system_indices.max()) < len(s.cells)
    i, j, sh = s.centers.numpy(), s.neighbors.numpy(), s.cell_shifts.numpy()
    assert np.array_equal(s.system_indices.numpy()[i], s.system_indices.numpy()[j])
    key = lambda a, b, c: sorted(zip(a.tolist(), b.tolist(), map(tuple, c.tolist())))  # noqa: E731
    fwd = key(i, j, sh)
    assert len(set(fwd)) == len(fwd) and fwd == key(j, i, -sh), "an edge without its partner, or twice"
    assert not ((i == j) & ~sh.any(axis=1)).any()
    _, d = A._cutoffs(case, "solver", torch.float64)
    assert d.max() < A.CUTOFF and d.min() > 1e-3


@pytest.mark.parametrize("case,method", CASE_METHOD)
def test_no_edge_near_its_pair_cutoff_and_the_fp32_oracle_agrees(case, method):
    s = A.system(case)
    r64, d = A._cutoffs(case, method, torch.float64)
    r32 = A.cutoffs(case, method, torch.float32)
    assert np.isfinite(r64).all() and np.isfinite(r32).all()
    m = A.edge_margin(s, r64, d)
    gap = np.abs(r32 - r64).max()
    print(f"adaptive-cases: {case} {method}  margin {m:.2e} A  |fp32 - fp64| cutoffs {gap:.2e} A")
    assert m >= A.MARGIN
    assert gap <= 1e-5
    b64, b32 = A.batch(case, method), A.batch(case, method, torch.float32)
    for k in ("centers", "neighbors", "cell_shifts", "padding_mask", "reverse_neighbor_index", "nef_to_edges_neighbor",
              "element_indices_neighbors"):
        assert np.array_equal(b64[k], b32[k]), k


@pytest.mark.parametrize("case", A.GEOMETRIC)
def test_the_solver_has_converged(case):
    s, spec = A.system(case), A.SPECS[case]
    r, d = A._cutoffs(case, "solver", torch.float64)
    n, _ = opet._adaptive_n_and_dn(torch.tensor(r), torch.tensor(d), s.centers, len(r), spec.width, 1.0 / A.CUTOFF, spec.target)
    at_returned = (n - spec.target).abs().numpy()
    _, _, at_root = A.trace(case)
    low = r == A.CUTOFF / 16.0
    residual = np.where(low, at_root.numpy(), at_returned)
    print(f"adaptive-cases: {case}  solver residual {residual.max():.2e}  ({int(low.sum())} atoms at the lower clamp)")
    assert residual.max() < 1e-9
    assert low.all() if case == "lower_clamp" else not low.any()


def test_the_seed_table_is_what_the_search_gives():
    got = {"rows": {m: A.first_clear_seed("rows", m, A.rows_start_seed(m)) for m in A.ROWS_CLUSTERS}}
    got.update({c: A.first_clear_seed(c) for c in A.GEOMETRIC if not c.startswith("rows")})
    assert got == A.SEEDS


# ---- per case ----------------------------------------------------------------------------------------------------------------
def test_rows_has_the_stated_rows_and_a_fallback_group():
    s = A.system("rows")
    rows = A.all_edge_rows(s)
    assert len(rows) == 205 and 205 % 16 == 13
    assert np.array_equal(rows, np.repeat(np.array(A.ROWS_CLUSTERS) - 1, A.ROWS_CLUSTERS))
    assert sorted(set(rows)) == [0, 1, 2, 15, 16, 17, 31, 32, 33, 48]
    small = A.system("rows_small")
    assert len(small.species) == 57 and sorted(set(A.all_edge_rows(small))) == [0, 1, 2, 15, 16, 17]
    assert np.array_equal(small.positions.numpy(), s.positions.numpy()[:57])  # the same clusters
    assert np.array_equal(A.cutoffs("rows_small", "solver"), A.cutoffs("rows", "solver")[:57])
    for method in A.METHODS:  # the cutoffs do cut: kept rows differ from the all-edge rows, and among the atoms
        kept = np.bincount(A.batch("rows", method)["centers"], minlength=205)
        assert (kept < rows).any() and (kept == rows).any() and len(set(kept)) > 10
    d = A._cutoffs("rows", "solver", torch.float64)[1]
    assert d.max() < 4.4 and d.min() > 0.5


def test_sparse_stays_below_the_target():
    s = A.system("sparse")
    rows = A.all_edge_rows(s)
    assert rows[0] == 0 and list(rows[1:6]) == [1, 1, 2, 2, 2] and rows.max() <= 5 < A.SPECS["sparse"].target
    d = A._cutoffs("sparse", "solver", torch.float64)[1]
    dimer = (s.group[s.centers.numpy()] == 1)
    assert np.allclose(d[dimer], 4.4, atol=1e-6)
    r = A.cutoffs("sparse", "solver")
    assert (r > A.CUTOFF - 0.6).all() and (r <= A.CUTOFF).all()
    assert r[0] == A.CUTOFF
    assert (s.cell_shifts.numpy()[s.group[s.centers.numpy()] == 3] != 0).any()  # the dilute system crosses its cell
    assert not s.cell_shifts.numpy()[:, 2].any()


def test_plateau_root_is_the_closed_form():
    s = A.system("plateau")
    assert len(s.species) == 12 and (A.all_edge_rows(s) == 11).all()
    r, d = A._cutoffs("plateau", "solver", torch.float64)
    assert d.max() <= 0.9 + 1e-6
    root = A.CUTOFF * 12.0 ** (-1.0 / 3.0)
    assert abs(root - 1.96556) < 1e-5 and root - 1.0 > d.max()  # every bump is saturated at the root
    assert np.abs(r - root).max() < 1e-12
    assert not A.cutoff_gradient("plateau", "solver").any()
    _, dn = opet._adaptive_n_and_dn(torch.tensor(r), torch.tensor(d), s.centers, 12, 1.0, 1.0 / A.CUTOFF, 12.0)
    assert np.allclose(dn.numpy(), 36.0 * 12.0 ** (-2.0 / 3.0) / A.CUTOFF, rtol=1e-12)  # 1.526: the cubic baseline alone


def test_lower_clamp_is_clamped_and_has_no_gradient():
    s = A.system("lower_clamp")
    assert len(s.species) == 61 and (A.all_edge_rows(s) == 60).all() and A.SPECS["lower_clamp"].width == 0.25
    r, d = A._cutoffs("lower_clamp", "solver", torch.float64)
    assert d.max() <= 0.1 + 1e-7
    assert (r == A.CUTOFF / 16.0).all() and A.CUTOFF / 16.0 == 0.28125
    assert not A.cutoff_gradient("lower_clamp", "solver").any()
    root, _, _ = A.trace("lower_clamp")
    assert 0.0 < root.min() and root.max() < 0.28125  # the unclamped root lies below the clamp
    assert A.reference_probe_count(A.CUTOFF, 0.25) == A.GRID_MAX_PROBES
    assert (A.cutoffs("lower_clamp", "grid") == 0.5 + 63 * 0.0625).all()  # every count is above the target: the last probe
    # the full PET oracle is finite here, in both precisions
    for dtype in (torch.float64, torch.float32):
        assert all(np.isfinite(v).all() for v in A.batch("lower_clamp", "solver", dtype).values())


def test_shoulder_takes_the_bisection_fallback():
    _, bisected, _ = A.trace("shoulder")
    assert int(bisected[0]) >= 1  # the centre: 4 close neighbours, a flat count up to the shell at 3.5 A
    assert int((bisected > 0).sum()) >= 1
    s = A.system("shoulder")
    d = A._cutoffs("shoulder", "solver", torch.float64)[1]
    row0 = np.sort(d[s.centers.numpy() == 0])
    assert len(row0) == 34 and row0[3] < 1.45 and row0[4] > 3.35
    # the other cases take it too where a root is rc (ten bisections) -- the plateau never
    assert int(A.trace("plateau")[1].max()) == 0 and int(A.trace("rows")[1].max()) == 10


def test_thin_cells_holds_self_images_an_empty_system_and_a_cluster():
    s = A.system("thin_cells")
    i, j, sh = s.centers.numpy(), s.neighbors.numpy(), s.cell_shifts.numpy()
    sysidx = s.system_indices.numpy()
    assert list(np.bincount(sysidx, minlength=4)) == [1, 3, 0, 17] and s.cells.shape == (4, 3, 3)
    assert np.array_equal(s.cells[0].numpy(), 3.0 * np.eye(3)) and np.array_equal(s.cells[1].numpy(), 4.0 * np.eye(3))
    row0 = i == 0
    assert row0.sum() == 18 and (j[row0] == 0).all() and sh[row0].any(axis=1).all()  # 6 at 3.0 A, 12 at 4.243 A
    assert ((i == j) & (sysidx[i] == 1)).any()  # the 4.0 A cell has self-images too
    assert not sh[sysidx[i] == 3].any() and (A.all_edge_rows(s)[sysidx == 3] == 16).all()
    for method in A.METHODS:  # the one-atom cell keeps its 6 nearest images only: its cutoff cuts between the two shells
        r = A.cutoffs("thin_cells", method)
        assert 3.0 < r[0] < 3.0 * 2 ** 0.5


# ---- probe counts ------------------------------------------------------------------------------------------------------------
def test_probe_counts_where_float32_hypers_miscount():
    """Over a scan of widths at the cutoffs 4.5, 5.0 and 6.0: where ``ceil((cutoff - 0.5) / (width / 4))`` on the float32-rounded
    hypers differs from the length of ``torch.arange(0.5, cutoff, width / 4)``. (4.5, 0.64) and (4.5, 0.32) are among the
    disagreements, (4.5, 0.25) is not; the Python layer's count (``runtime.grid_probe_count``) is the reference's everywhere."""
    from metatrain_amd import runtime as rt

    widths = [0.05, 0.08, 0.1, 0.16, 0.2, 0.24, 0.25, 0.32, 0.4, 0.5, 0.64, 0.8, 1.0, 1.28, 1.6]
    differ = set()
    for cutoff in (4.5, 5.0, 6.0):
        for w in widths:
            ref = A.reference_probe_count(cutoff, w)
            assert rt.grid_probe_count(cutoff, w) == ref, (cutoff, w)
            if A.float32_probe_count(cutoff, w) != ref:
                differ.add((cutoff, w, ref, A.float32_probe_count(cutoff, w)))
    print("adaptive-cases: float32 probe counts that differ from torch.arange's:", sorted(differ))
    assert {(4.5, 0.64, 25, 26), (4.5, 0.32, 50, 51)} <= differ
    assert not any((c, w) == (4.5, 0.25) for c, w, _, _ in differ)
    for cutoff, w, stated in A.PROBE_COUNTS:
        ref = A.reference_probe_count(cutoff, w)
        assert (ref == stated) if stated is not None else not (2 <= ref <= A.GRID_MAX_PROBES), (cutoff, w, ref)
    assert A.reference_probe_count(4.5, 0.24) == 67 and A.reference_probe_count(0.7, 1.0) == 1


def test_the_hypers_struct_carries_the_reference_probe_count():
    from metatrain_amd import runtime as rt

    for cutoff, w, _ in A.PROBE_COUNTS:
        hy = dict(opet.DEFAULT_HYPERS, cutoff=cutoff, cutoff_width_adaptive=w, num_neighbors_adaptive=12.0,
                  adaptive_cutoff_method="grid")
        assert rt.hypers_struct(hy, [1, 6]).adaptive_grid_probes == A.reference_probe_count(cutoff, w)
    # nothing to count without the grid method
    assert rt.hypers_struct(dict(opet.DEFAULT_HYPERS, num_neighbors_adaptive=12.0), [1, 6]).adaptive_grid_probes == 0
    assert rt.hypers_struct(dict(opet.DEFAULT_HYPERS, adaptive_cutoff_method="grid"), [1, 6]).adaptive_grid_probes == 0
