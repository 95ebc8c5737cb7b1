"""The tuned first-order PET pass computes, to the bit, what it computed before the choice of every stage's kernel moved
into one plan (``csrc/pet_plan.h``): ``tests/golden/stage_plan_parent_digests.json`` holds the SHA-256 of per-atom
energies, dE/dR, dE/dcell (and the flat parameter gradient of the training pass) and the workspace sizes, recorded by
``tests/golden/make_stage_digests.py`` on a build of the commit named in the file. The kernels are atomics-free and
launched in a fixed order, so equality is the assertion. The cases reach every form of every stage:

  small/default            pipelined edge kernels (compress, edge MLP with [v; g] saved, combination with dXF folded in, edge
                           head), three-kernel attention, ``k_node2<1, true>`` split with the next centre tokens written by
                           the node kernel, ``k_center`` for the first layer, ``k_center_bwd<true>``
  small/trr=0              LDS-tile kernels of every stage, ``k_dxf``
  small/attn_fused=0       as default (a small graph is not fused by default): the switch alone
  small/side_stream=0      one stream
  small/trr_compress=0     LDS-tile compress, edge head and their adjoints beside the pipelined layers
  small/node_planes=0      ``k_node`` / ``k_swiglu_bwd<256>`` + ``k_expand_bwd``, ``k_center`` in every layer
  small/node_planes=2      the 32-row node kernels forced (as default at this size)
  small/center_fused=0     ``k_center`` by its own launch in every layer
  small/dxf_fused=0        ``k_dxf`` behind the pipelined combination adjoint
  small/node_split=0       ``k_node2<1>`` / ``k_node_bwd2<1>`` unsplit
  small/emlp_s=0           the ring kernels off (as default at this size)
  small/emlp_s=2,attn_fused=7   ring kernels in every edge stage, the edge MLP's adjoint recomputing [v; g], the ring node chain
                           and its adjoint, ``k_rowlin_s`` for the centre contraction, its adjoint and the expansion adjoint,
                           the fused attention block and its adjoint (32-slot tiles, ``k_dfc_attn`` over head sums)
  small/save=0             forward alone, nothing stored (the fused block needs no adjoint to follow)
  dense/*                  the 64-slot tiles of the fused block and its adjoint; the three-kernel form at four tiles
  variants/*               LayerNorm on the pipelined kernels; PostLN on the LDS-tile layers between pipelined compress and
                           head, one stream; the residual featuriser with ``k_resmix``, no centre tokens written into a
                           residual layer, one stream in the adjoint; no centre tokens written behind the conditioning add;
                           each again with ``trr = 0``
  train/*                  the training forward (three-kernel attention, everything saved; ``emlp_s = 2``: ring edge kernels
                           storing [v; g], ring node chain) and ``pet_backward_train`` with the TRAIN instantiations of the
                           pipelined and LDS-tile adjoints, one stream
  edgeless/*               no edge rows at all; atoms without neighbours among others
  boxes/below_1000         default policy below every threshold
  boxes/edge_rows          ring kernels in every edge stage from 28 672 edge rows, the recomputing adjoint
  boxes/tiles              the fused attention block from 3 840 32-slot tiles; more than 128 node tiles: unsplit
  boxes/split_off          more than 128 node tiles below the tile threshold: ``k_node2<1>`` unsplit, ``k_center_bwd<false>``
  boxes/atoms_16384        ``k_rowlin_s`` for the first centre contraction and every contraction adjoint, still 32-row node
                           kernels (which write the other centre tokens and the expansion adjoint)
  boxes/atoms_16385        the 64-row node kernels ``k_node2w`` / ``k_node_bwd2<2>``, ``k_rowlin_s`` in all three places
  boxes/atoms_28672        the ring node chain of ``pet_node_s.hip`` and its adjoint on the second stream

and two refusals: an adjoint whose switches no longer allow what its forward left unsaved says so."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_stage_digests", os.path.join(GOLDEN, "make_stage_digests.py"))
digests = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(digests)

WANT = json.load(open(os.path.join(GOLDEN, "stage_plan_parent_digests.json")))
FORCED = "emlp_s=2,attn_fused=7"


def _same(got, want, what):
    for key in ("workspace_bytes", "stages"):
        assert got.get(key) == want.get(key), f"{what}: {key} {got.get(key)} != {want.get(key)}"
    assert set(got["digests"]) == set(want["digests"]), (what, set(got["digests"]) ^ set(want["digests"]))
    differ = sorted(k for k in want["digests"] if got["digests"][k] != want["digests"][k])
    assert not differ, f"{what}: differs from the build of {WANT['commit'][:7]}: {differ}"


def test_record_covers_every_case():
    for group, cases in (("small", digests.SMALL), ("dense", digests.DENSE), ("variants", digests.VARIANT_CASES),
                         ("train", digests.TRAIN), ("edgeless", digests.EDGELESS), ("boxes", digests.BOXES)):
        assert set(WANT[group]) == set(cases), group


@pytest.mark.parametrize("case", digests.SMALL)
def test_small_graph_keeps_its_bits(case):
    _same(digests.small_record(case), WANT["small"][case], f"small/{case}")


@pytest.mark.parametrize("case", digests.DENSE)
def test_dense_box_keeps_its_bits(case):
    _same(digests.dense_record(case), WANT["dense"][case], f"dense/{case}")


@pytest.mark.parametrize("case", digests.VARIANT_CASES)
def test_variant_keeps_its_bits(case):
    _same(digests.variant_record(case), WANT["variants"][case], f"variants/{case}")


@pytest.mark.parametrize("case", digests.TRAIN)
def test_training_pass_keeps_its_bits(case):
    _same(digests.train_record(case), WANT["train"][case], f"train/{case}")


@pytest.mark.parametrize("case", digests.EDGELESS)
def test_edgeless_batch_keeps_its_bits(case):
    _same(digests.edgeless_record(case), WANT["edgeless"][case], f"edgeless/{case}")


@pytest.mark.parametrize("name", digests.BOXES)
def test_threshold_box_keeps_its_bits(name):
    want = WANT["boxes"][name]
    got = digests.box_record(want["n_atoms"])
    n, e = got["n_atoms"], got["n_edges"]
    assert e == want["n_edges"] and got["max_neighbors"] == want["max_neighbors"] <= 63
    fused = "attn_blk" in got["stages"]
    # the counts against the thresholds of the policy, not against an estimate of the box that crosses them
    if name == "below_1000":
        assert e < digests.MIN_ROWS and n <= 32 * digests.SPLIT_TILES and not fused
    elif name == "edge_rows":
        assert e >= digests.MIN_ROWS and n < digests.MIN_TILES and not fused
    elif name == "tiles":
        assert fused and digests.MIN_TILES <= n <= digests.NODE_ROWS_ATOMS
    elif name == "split_off":
        assert 4096 < n < digests.NODE_ROWS_ATOMS and -(-n // 32) > digests.SPLIT_TILES
    elif name == "atoms_16384":
        assert n == digests.NODE_ROWS_ATOMS
    elif name == "atoms_16385":
        assert n == digests.NODE_ROWS_ATOMS + 1
    else:
        assert digests.NODE_ROWS_ATOMS < n and n >= digests.MIN_ROWS
    _same(got, want, f"boxes/{name}")


@pytest.mark.parametrize("flip,message", [("emlp_s", "did not save the edge MLP's pre-activations"),
                                          ("attn_fused", "ran the fused attention block")])
def test_adjoint_refuses_what_its_forward_left_unsaved(flip, message):
    """A forward under the forced policy leaves Q, K, V and [v; g] unwritten. With the switch of either kernel family off
    before ``pet_backward`` the adjoint refuses (a host-side error, nothing faults); with the switch back, the adjoint of
    the same workspace gives the bits of an uninterrupted run."""
    from metatrain_amd import runtime as rt

    model = digests.default_model()
    with digests.switches(FORCED):
        graph = digests.refusal_graph()
        fw = rt.HipForward(model, graph)
        atomic = fw.forward()
        ones = torch.ones_like(atomic)
        rt.config_set(flip, 0)
        try:
            with pytest.raises(rt.PetHipError, match=message):
                fw.backward(ones)
        finally:
            rt.config_set(flip, {"emlp_s": 2, "attn_fused": 7}[flip])
        grad, cell_grad = fw.backward(ones, want_cell_grad=True)
        torch.cuda.synchronize()
    want = WANT["small"][FORCED]["digests"]
    assert digests.sha(atomic) == want["atomic"]
    assert digests.sha(grad) == want["grad"] and digests.sha(cell_grad) == want["cell_grad"]
