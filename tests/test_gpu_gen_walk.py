"""The size-generic PET pass computes, to the bit, what it computed before its four hand-written walks over the
architecture became the two of ``csrc/gen_walk.h``: ``tests/golden/gen_walk_parent_digests.json`` holds the SHA-256 of every
output of the path (inference fused and staged, both training passes, the Hessian-vector product, two multi-target steps)
and its four workspace sizes, recorded by ``tests/golden/make_gen_digests.py`` on a build of the commit named in the file.
The kernels are atomics-free and launched in a fixed order, so equality is the assertion; a digest that differs names the
quantity whose launches or buffers changed. No oracle evaluation."""
import importlib.util
import json
import os

import pytest

import gen_shapes as gs

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_gen_digests", os.path.join(gs.GOLDEN, "make_gen_digests.py"))
digests = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(digests)

WANT = json.load(open(os.path.join(gs.GOLDEN, "gen_walk_parent_digests.json")))


def _same(got, want, what):
    assert set(got) == set(want), (what, set(got) ^ set(want))
    differ = sorted(k for k in want if got[k] != want[k])
    assert not differ, f"{what}: differs from the build of {WANT['commit'][:7]}: {differ}"


def test_record_covers_every_pair():
    assert set(WANT["pairs"]) == {f"{tag}-{which}" for tag, which in gs.PAIRS}
    assert set(WANT["steps"]) == set(digests.STEPS)


@pytest.mark.parametrize("tag,which", gs.PAIRS)
def test_pair_keeps_its_bits(tag, which):
    got, want = digests.pair_record(tag, which), WANT["pairs"][f"{tag}-{which}"]
    _same(got["workspace_bytes"], want["workspace_bytes"], f"{tag}-{which} workspace sizes")
    _same(got["digests"], want["digests"], f"{tag}-{which}")


@pytest.mark.parametrize("which", digests.STEPS)
def test_multitarget_step_keeps_its_bits(which):
    _same(digests.step_record(which)["digests"], WANT["steps"][which]["digests"], f"flat32 step {which}")
