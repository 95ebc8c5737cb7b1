"""The long-range operator's second-order surface computes, to the bit, what it computed before its two modes went behind one
internal interface (``LrCall``, ``csrc/long_range.h``) and every launch list was stated once:
``tests/golden/long_range_second_parent_digests.json`` holds the SHA-256 of every fp32 result, the workspace sizes and the
transform hook's call counts, recorded by ``tests/golden/make_long_range_second_digests.py`` on a build of the commit named
in the file (twice; the two records were equal in every entry, so no quantity is left out). The sums are atomics-free and
the kernels launched in a fixed order, so equality is the assertion. ``test_gpu_long_range_digests.py`` is the first-order
counterpart.

  ewald        ``EwaldHip.second`` on ``test_gpu_long_range_second.CASES``, both cotangents; ``periodic_tiles`` at C = 33 with
               each cotangent alone
  p3m          ``P3MHip.second`` on ``test_p3m_second_cpu.GPU_RUNS``; ``HALF_RUN`` under the three ``HALVES``, under each single
               ``results`` flag and under ``(True, False, True)``
  second_cell  both modes on the cases of ``test_gpu_long_range_cell_second.py``; on ``mixed``: ``u_cells`` alone, ``u_cells=None``
               (the bits of ``second``'s first two results) and each single ``results`` flag
  model        both methods on ``("odd33", "model_batch")``, ``("residual", "box")`` and ``("odd33", "two_cells")``: ``flat_grad()``
               and the tangent after ``backward_train`` and after ``backward_train2`` with ``u``, with ``u`` and ``u_cell`` and with
               ``u_cell`` alone; ``hessian_vector_product`` with and without ``lambda_atomic``
  double       a double backward through ``LongRangeFeaturizerHip.__call__``: the gradients of ``<u, dE/dR>`` with respect to
               the features, the positions and the six tensors
  empty        a plan without atoms through the four second-order entry points and the three sweeps: ``PET_OK``, no hook call"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_long_range_second_digests",
                                               os.path.join(GOLDEN, "make_long_range_second_digests.py"))
digests = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(digests)

WANT = json.load(open(os.path.join(GOLDEN, "long_range_second_parent_digests.json")))


def _same(got, want, what):
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for key in sorted(set(want) - {"digests"}):
        assert got[key] == want[key], f"{what}: {key} {got[key]} != {want[key]}"
    if "digests" in want:
        assert set(got["digests"]) == set(want["digests"]), (what, set(got["digests"]) ^ set(want["digests"]))
        differ = sorted(k for k in want["digests"] if got["digests"][k] != want["digests"][k])
        assert not differ, f"{what}: differs from the build of {WANT['commit'][:7]}: {differ}"


def test_record_covers_every_case():
    import test_gpu_long_range_cell_second as cell
    import test_gpu_long_range_second as second
    import test_p3m_second_cpu as mesh

    for group, runs, key, _ in digests.GROUPS:
        assert set(WANT[group]) == {key(*run) for run in runs}, group
    assert [(n, c) for n, c, h in digests.EWALD_RUNS if h == "both"] == second.CASES
    assert [r[:3] for r in digests.P3M_RUNS[:len(mesh.GPU_RUNS)]] == mesh.GPU_RUNS
    assert {(h, r) for *run, h, r in digests.P3M_RUNS if tuple(run) == mesh.HALF_RUN} >= (
        {(h, digests.ALL3) for h in mesh.HALVES} | {("both", r) for r in digests.SINGLE3 + [(True, False, True)]})
    full = [r[:3] for r in digests.CELL_RUNS if r[3] == "all" and r[4] == (True, True)]
    assert full == [(n, 0, c) for n, c in cell.EWALD_CASES] + cell.MESH_CASES
    for case in digests.CELL_VARIANTS:
        assert {r[3:] for r in digests.CELL_RUNS if r[:3] == case} == {
            ("all", (True, True)), ("u_cells", (True, True)), ("no_cell", (True, True)), ("all", (True, False)), ("all", (False, True))}
    for group in ("ewald", "p3m", "second_cell"):
        for key, rec in WANT[group].items():
            assert set(digests.SECOND_QUERIES) <= set(rec), key
    for key, rec in list(WANT["model"].items()) + list(WANT["empty"].items()):
        assert set(digests.SWEEP_QUERIES) <= set(rec), key
    for rec in WANT["empty"].values():
        assert set(rec["rc"].values()) == {0} and rec.get("transform_calls", 0) == 0


def _ids(runs, key):
    return [key(*run) for run in runs]


@pytest.mark.parametrize("run", digests.EWALD_RUNS, ids=_ids(digests.EWALD_RUNS, digests.ewald_key))
def test_ewald_second(run):
    key = digests.ewald_key(*run)
    _same(digests.ewald_record(*run), WANT["ewald"][key], f"ewald {key}")


@pytest.mark.parametrize("run", digests.P3M_RUNS, ids=_ids(digests.P3M_RUNS, digests.p3m_key))
def test_p3m_second(run):
    key = digests.p3m_key(*run)
    _same(digests.p3m_record(*run), WANT["p3m"][key], f"p3m {key}")


@pytest.mark.parametrize("run", digests.CELL_RUNS, ids=_ids(digests.CELL_RUNS, digests.cell_key))
def test_second_cell(run):
    key = digests.cell_key(*run)
    got = digests.cell_record(*run)
    if run[3] == "no_cell":
        assert got["equals_second"]
    _same(got, WANT["second_cell"][key], f"second_cell {key}")


@pytest.mark.parametrize("run", digests.MODEL_RUNS, ids=_ids(digests.MODEL_RUNS, digests.model_key))
def test_whole_model(run):
    key = digests.model_key(*run)
    _same(digests.model_record(*run), WANT["model"][key], f"model {key}")


@pytest.mark.parametrize("method", digests.METHODS)
def test_double_backward_through_the_featurizer(method):
    _same(digests.double_record(method), WANT["double"][method], f"double {method}")


@pytest.mark.parametrize("method", digests.METHODS)
def test_plan_without_atoms(method):
    got = digests.empty_record(method)
    assert set(got["rc"].values()) == {0} and got.get("transform_calls", 0) == 0
    _same(got, WANT["empty"][method], f"empty {method}")
