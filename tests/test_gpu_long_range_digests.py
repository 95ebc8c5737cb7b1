"""The long-range operator computes, to the bit, what it computed before the part that its two evaluations share moved
into one header (``csrc/long_range.h``, included by ``ewald.hip`` and ``p3m.hip``) and its local terms into two host
functions: ``tests/golden/long_range_parent_digests.json`` holds the SHA-256 of fp32 V, dL/dq, dL/dR and dL/dcell, the
workspace sizes (P3M: with the mesh and half-spectrum element counts) and the k-vector counts or mesh shapes, recorded by
``tests/golden/make_long_range_digests.py`` on a build of the commit named in the file. The sums are atomics-free and the
kernels launched in a fixed order (``w.F`` is accumulated across launches), so equality is the assertion: a moved rounding
or a reordered launch shows here.

  ewald   every case of ``ewald_cases.OPERATOR_CASES`` and ``mixed`` at C = 24; ``open_tiles`` and ``periodic_tiles`` at
          C = 3 (scalar loads) and C = 260 (a second grid row)
  p3m     every ``(name, nodes)`` of ``test_gpu_p3m.CASE_RUNS`` at C = 24; ``channels`` at every width of ``p3m_cases.CHANNELS``
  model   ``energy_and_gradient(..., want_cell_grad=True)`` on ``ewald_cases.model_batch()`` under both methods
  empty   a plan without atoms, both modes: dL/dcell is zeros"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_long_range_digests", os.path.join(GOLDEN, "make_long_range_digests.py"))
digests = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(digests)

WANT = json.load(open(os.path.join(GOLDEN, "long_range_parent_digests.json")))


def _same(got, want, what):
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for key in sorted(set(want) - {"digests"}):
        assert got[key] == want[key], f"{what}: {key} {got[key]} != {want[key]}"
    assert set(got["digests"]) == set(want["digests"]), (what, set(got["digests"]) ^ set(want["digests"]))
    differ = sorted(k for k in want["digests"] if got["digests"][k] != want["digests"][k])
    assert not differ, f"{what}: differs from the build of {WANT['commit'][:7]}: {differ}"


def test_record_covers_every_case():
    import test_gpu_p3m

    assert set(WANT["ewald"]) == {digests.ewald_key(*run) for run in digests.EWALD_RUNS}
    assert set(WANT["p3m"]) == {digests.p3m_key(*run) for run in digests.P3M_RUNS}
    assert [(name, p) for name, p, channels in digests.P3M_RUNS if name != "channels"] == test_gpu_p3m.CASE_RUNS
    assert set(WANT["model"]) == set(WANT["empty"]) == set(digests.METHODS)
    for group in ("ewald", "p3m"):
        for key, rec in WANT[group].items():
            assert set(rec["digests"]) == set(digests.ec.QUANTITIES), key


@pytest.mark.parametrize("name, channels", digests.EWALD_RUNS, ids=[digests.ewald_key(*run) for run in digests.EWALD_RUNS])
def test_ewald_case(name, channels):
    key = digests.ewald_key(name, channels)
    _same(digests.ewald_record(name, channels), WANT["ewald"][key], f"ewald {key}")


@pytest.mark.parametrize("name, nodes, channels", digests.P3M_RUNS, ids=[digests.p3m_key(*run) for run in digests.P3M_RUNS])
def test_p3m_case(name, nodes, channels):
    key = digests.p3m_key(name, nodes, channels)
    _same(digests.p3m_record(name, nodes, channels), WANT["p3m"][key], f"p3m {key}")


@pytest.mark.parametrize("method", digests.METHODS)
def test_whole_model(method):
    _same(digests.model_record(method), WANT["model"][method], f"model {method}")


@pytest.mark.parametrize("method", digests.METHODS)
def test_plan_without_atoms(method):
    got = digests.empty_record(method)
    assert got["grad_cells_max"] == 0.0
    _same(got, WANT["empty"][method], f"empty {method}")
