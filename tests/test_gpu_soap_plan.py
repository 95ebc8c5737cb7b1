"""The SOAP-BPNN pass computes, to the bit, what it computed before the choice of every stage's kernel moved into one plan
(``csrc/soap_plan.h``) and ``soap.hip`` was split by stage: ``tests/golden/soap_plan_parent_digests.json`` holds the SHA-256
of per-atom energies, dE/dR, dE/dcell (the features where the forward hands them out; every parameter gradient and the
tangent energies of the training pass), the workspace sizes and the profiled stage names, recorded by
``tests/golden/make_soap_digests.py`` on a build of the commit named in the file, twice in two processes with equal results.
The kernels are atomics-free and launched in a fixed order, so equality is the assertion. The cases reach every value of the
plan:

  box/default              wave expansion ``k_soap_expand_w<6>`` / ``k_soap_expand_bwd_p<6>`` with staged rows, packed power
                           spectrum ``k_soap_ps_m<true>`` / ``k_soap_ps_bwd_m<true>``, bucketing and the sorted tail on the
                           packed weights
  box/soap_packed=0        ``k_soap_ps_m<false>`` / ``k_soap_ps_bwd_m<false>``, sorted tail on the full layout
  box/soap_ps_mfma=0       ``k_soap_ps_w`` / ``k_soap_ps_bwd_s``
  box/soap_pair=0          first generation: ``k_soap_expand`` / ``k_soap_expand_bwd``, ``k_soap_ps`` / ``k_soap_ps_bwd``
  box/soap_sorted=0        stacked tail ``k_soap_tail_fwd_mfma<2>`` / ``k_soap_tail_bwd_mfma<2>``, no bucketing
  box/soap_mfma=0          per-atom tail ``k_soap_tail`` / ``k_soap_tail_bwd``
  box/features             a forward that hands out its features keeps the full layout under the default switches
  catalogue/legacy_types_3     C = 3: first-generation expansion, an odd network count on the sorted tail, full layout
  catalogue/legacy_types_5     ncmax 40: ``k_soap_ps_w``
  catalogue/legacy_types_8     the dF row no longer fits 64 KB: ``k_soap_ps_bwd``; the eighth bucket
  catalogue/legacy_types_9     NT = 0: per-atom tail with more than 64 KB of LDS
  catalogue/alchemical_types_9 centre encoding: never packed, one network
  catalogue/bucket_*, small_*, holes, mixed, lone_atom   bucket edges and empty buckets, N % 4, zero-length rows inside a
                           staged block, systems without pairs, self-image pairs only
  models/max_angular_8     ``wide_l``: the ``MAXL`` instantiation of the wave expansion and of its adjoint
  models/hidden_layers_3   the continuation kernels ``k_soap_tail_extra_fwd`` / ``_bwd``
  train/*                  the training pass behind a default (packed) forward: the rebuild of the full layout through
                           ``soap_ps_full``, the 8-network bucket table and (``legacy_types_9``) the 16-network one, the
                           front-of-the-tail pass (``alchemical_types_9``), an empty bucket, with and without a tangent; no
                           batch above 1 024 atoms (``make_soap_digests.py`` says why)

and one refusal: a species-sorted tail adjoint behind a forward that did not bucket the atoms says so."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_soap_digests", os.path.join(GOLDEN, "make_soap_digests.py"))
digests = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(digests)

WANT = json.load(open(os.path.join(GOLDEN, "soap_plan_parent_digests.json")))


def _same(got, want, what):
    for key in ("workspace_bytes", "train_workspace_bytes", "stages"):
        assert got.get(key) == want.get(key), f"{what}: {key} {got.get(key)} != {want.get(key)}"
    assert set(got["digests"]) == set(want["digests"]), (what, set(got["digests"]) ^ set(want["digests"]))
    differ = sorted(k for k in want["digests"] if got["digests"][k] != want["digests"][k])
    assert not differ, f"{what}: differs from the build of {WANT['commit'][:7]}: {differ}"


def test_record_covers_every_case():
    for group, cases, _ in digests.GROUPS:
        assert set(WANT[group]) == set(cases), group
    atomic = [WANT["box"][c]["digests"]["atomic"] for c in digests.DISTINCT]
    assert len(set(atomic)) == len(atomic), "two routes of the box give the same bits: a wrong route would pass"


@pytest.mark.parametrize("case", digests.BOX)
def test_box_keeps_its_bits(case):
    _same(digests.box_record(case), WANT["box"][case], f"box/{case}")


@pytest.mark.parametrize("name", digests.CATALOGUE)
def test_catalogue_case_keeps_its_bits(name):
    _same(digests.catalogue_record(name), WANT["catalogue"][name], f"catalogue/{name}")


@pytest.mark.parametrize("variant", list(digests.MODELS))
def test_model_variant_keeps_its_bits(variant):
    _same(digests.model_record(variant), WANT["models"][variant], f"models/{variant}")


@pytest.mark.parametrize("case", digests.TRAIN)
def test_training_pass_keeps_its_bits(case):
    _same(digests.train_record(case), WANT["train"][case], f"train/{case}")


def test_sorted_adjoint_refuses_a_forward_that_did_not_bucket():
    """A forward with ``soap_sorted = 0`` runs the stacked tail and fills neither ``perm`` nor ``info``. With the switch back
    on before ``soap_backward`` the species-sorted adjoint would read them: the plan refuses (a host-side error in front of
    every launch, nothing faults). A fresh forward and adjoint with the switch on then give the bits of the default record."""
    from metatrain_amd import runtime as rt

    m, b = digests.box_model(), digests.box_inputs()
    g = digests._graph(m, b)
    seed = digests._seed(g.n_nodes)
    try:
        rt.config_set("soap_sorted", 0)
        m.forward(g)
        rt.config_set("soap_sorted", 1)
        with pytest.raises(rt.PetHipError, match="soap_sorted"):
            m.backward(g, seed)
    finally:
        rt.config_set("soap_sorted", 1)
    atomic = m.forward(g)
    grad, cell_grad = m.backward(g, seed, want_cell_grad=True)
    torch.cuda.synchronize()
    want = WANT["box"]["default"]["digests"]
    assert digests.sha(atomic) == want["atomic"]
    assert digests.sha(grad) == want["grad"] and digests.sha(cell_grad) == want["cell_grad"]
