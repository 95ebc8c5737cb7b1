"""The row kernels on the shared weight ring compute, to the bit, what they computed before the ring's protocol -- constants,
wave frame, stage sync, stage body, slot addresses, row-tile DMA, launch -- moved into one header (``csrc/rows_s.h``):
``tests/golden/ring_rows_parent_digests.json`` holds the SHA-256 of the outputs, recorded by
``tests/golden/make_ring_rows_digests.py`` on a build of the commit named in the file (two recordings of that build agreed on
every quantity). The kernels are atomics-free and launched in a fixed order, so equality is the assertion.
``tests/test_gpu_stage_plan.py`` pins the ring kernels of the default model's inference pass; the cases here reach the other
instantiations, all under the forced policy ``emlp_s=2`` (``attn_fused=7`` for inference):

  layernorm      ``k_emlp_s<true>``, ``k_emlp_bwd_s<true, *>``, ``k_rowgemm_s_k2<2>``, the LayerNorm form of ``k_rowgemm_s_n2<1>``
  partial_tile   E mod 128 in 1 .. 31: the last workgroup has a partial tile and three dead waves
  dead_waves     E mod 128 == 32: a full last tile and three dead waves
  second_order   the force-loss step: generic ``k_rowgemm_s`` with and without the addend, nk > 1, nn > 1
  layers=1, 2    ``k_compress_bwd_s<true | false>``, ``k_comb_s<true | false>``, ``k_comb_bwd_s<*>``, inference and training"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_ring_rows_digests", os.path.join(GOLDEN, "make_ring_rows_digests.py"))
digests = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(digests)

WANT = json.load(open(os.path.join(GOLDEN, "ring_rows_parent_digests.json")))
RING_STAGES = {"emlp", "emlp_bwd", "comb", "comb_bwd", "compress_bwd", "head_edge", "head_edge_bwd", "center", "center_bwd"}


def test_record_covers_every_case():
    assert set(WANT["cases"]) == set(digests.CASES)
    for name in digests.BOXES:
        assert WANT["cases"][name]["n_atoms"] == digests.BOXES[name][0]


def test_box_residues():
    """The edge counts of the two boxes leave the last workgroup what the cases are about (128 rows per workgroup, 32 per wave)."""
    partial, dead = WANT["cases"]["partial_tile"]["n_edges"], WANT["cases"]["dead_waves"]["n_edges"]
    assert 1 <= partial % 128 <= 31
    assert dead % 32 == 0 and dead % 128 == 32


@pytest.mark.parametrize("case", digests.CASES)
def test_ring_rows_keep_their_bits(case):
    got, want = digests.record(case), WANT["cases"][case]
    assert set(got) == set(want), (case, set(got) ^ set(want))
    for key in sorted(set(want) - {"digests"}):
        assert got[key] == want[key], f"{case}: {key} {got[key]} != {want[key]}"
    if "stages" in want:  # the forced policy did send every ring stage to its ring kernel's launch
        assert RING_STAGES <= set(want["stages"]), RING_STAGES - set(want["stages"])
    assert set(got["digests"]) == set(want["digests"]), (case, set(got["digests"]) ^ set(want["digests"]))
    differ = sorted(k for k in want["digests"] if got["digests"][k] != want["digests"][k])
    assert not differ, f"{case}: differs from the build of {WANT['commit'][:7]}: {differ}"
