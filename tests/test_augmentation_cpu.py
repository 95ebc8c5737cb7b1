"""Host side of the device augmenter (``metatrain_amd/augmentation.py``, ``pet_o3_draw`` / ``pet_o3_apply``): what is
refused and how, what passes through, the state round trip and the C entry points' argument checks. No GPU call is made:
every check below fires on the host before a launch."""
import ctypes
import os
import re

import pytest
import torch

from metatrain_amd import _lib
from metatrain_amd import runtime as rt
from metatrain_amd.augmentation import O3Augmenter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from metatrain_amd import build

        build.build(verbose=False)
    return _lib.load()


def _batch(n_per_system=(2, 3)):
    """A collated batch's shape on the CPU (the pair list is never looked at by the augmenter)."""
    n, s = sum(n_per_system), len(n_per_system)
    g = torch.Generator().manual_seed(0)
    return {
        "positions": torch.rand((n, 3), generator=g),
        "cells": torch.eye(3).repeat(s, 1, 1) * 5,
        "centers": torch.zeros(4, dtype=torch.int32),
        "neighbors": torch.ones(4, dtype=torch.int32),
        "cell_shifts": torch.zeros((4, 3), dtype=torch.int32),
        "species": torch.ones(n, dtype=torch.int32),
        "system_indices": torch.cat([torch.full((k,), i, dtype=torch.int32) for i, k in enumerate(n_per_system)]),
        "energy": torch.rand((s, 1), generator=g),
        "forces": torch.rand((n, 3), generator=g),
    }


KINDS = {"energy": "scalar", "forces": "vector"}


def test_header_declares_both_entry_points_and_the_library_exports_them(lib):
    header = open(os.path.join(ROOT, "include", "pet_hip.h")).read()
    declared = set(re.findall(r"\b(pet_[a-z0-9_]+)\s*\(", header))
    for name in ("pet_o3_draw", "pet_o3_apply"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert declared == set(_lib.SYMBOLS)
    # the ctypes mirror has the header's layout: two pointers, a count, a pointer, two int32
    assert ctypes.sizeof(_lib.O3Array) == 40
    for macro, value in (("PET_O3_GROUP_O3", _lib.PET_O3_GROUPS["O3"]), ("PET_O3_GROUP_INVERSIONS", _lib.PET_O3_GROUPS["inversions"]),
                         ("PET_O3_VECTOR", _lib.PET_O3_KINDS["vector"]), ("PET_O3_TENSOR2", _lib.PET_O3_KINDS["tensor2"]),
                         ("PET_O3_MAX_ARRAYS", _lib.PET_O3_MAX_ARRAYS)):
        assert re.search(rf"^#define {macro} {value}$", header, re.M), macro


def test_cpu_tensors_raise_no_cpu_path():
    aug = O3Augmenter(KINDS)
    with pytest.raises(_lib.PetHipError, match="no CPU path"):
        aug.apply_random_augmentations(_batch())
    assert aug.counter == 0  # nothing was drawn
    with pytest.raises(_lib.PetHipError, match="no CPU path"):
        aug.apply_augmentations(_batch(), torch.eye(3).repeat(2, 1, 1))
    with pytest.raises(_lib.PetHipError, match="no CPU path"):
        rt.o3_draw(4, 0, 0, "O3", "cpu")
    with pytest.raises(_lib.PetHipError, match="no CPU path"):
        rt.o3_apply(torch.eye(3).repeat(2, 1, 1), [(torch.zeros(2, 3), "vector", None)])


def test_unknown_kinds_groups_and_spherical_targets_are_refused():
    with pytest.raises(ValueError, match="unknown kind 'pseudovector'"):
        O3Augmenter({"forces": "pseudovector"})
    with pytest.raises(ValueError, match="unknown transformation group"):
        O3Augmenter(KINDS, group="SO3")
    for lam in (1, 2):
        with pytest.raises(ValueError, match="Wigner-D"):
            O3Augmenter({"multipole": {"kind": "spherical", "lambda": lam}})
    with pytest.raises(ValueError, match="Wigner-D"):  # a pseudoscalar changes sign under an improper rotation
        O3Augmenter({"chirality": {"kind": "spherical", "lambda": 0, "sigma": -1}})
    O3Augmenter({"energy": {"kind": "spherical", "lambda": 0}})  # an invariant: a scalar
    with pytest.raises(ValueError, match="part of the batch itself"):
        O3Augmenter({"positions": "vector"})
    with pytest.raises(ValueError, match=r"seed must be in \[0, 2\^32\)"):
        O3Augmenter(KINDS, seed=2**32)
    with pytest.raises(ValueError, match="unknown kind 'axial'"):
        O3Augmenter({"a": {"kind": "axial", "per_atom": True}})
    with pytest.raises(ValueError, match="unknown entries"):
        O3Augmenter({"a": {"kind": "vector", "per_system": True}})


def test_a_tensor_the_augmenter_was_not_told_about_is_refused():
    b = _batch()
    b["dipole"] = torch.zeros(2, 3)
    with pytest.raises(ValueError, match="'dipole'"):
        O3Augmenter(KINDS).apply_random_augmentations(b)


@pytest.mark.parametrize("kind,shape", [("vector", (5, 4)), ("vector", (5,)), ("vector", (5, 2, 2)),
                                        ("tensor2", (2, 3)), ("tensor2", (2, 3, 4)), ("tensor2", (5, 12))])
def test_wrong_trailing_shapes_are_refused(kind, shape):
    b = _batch()
    b["t"] = torch.zeros(shape)
    aug = O3Augmenter(dict(KINDS, t=kind))
    with pytest.raises(ValueError, match=f"a {kind} needs"):
        aug.apply_random_augmentations(b)
    with pytest.raises(ValueError, match=f"a {kind} needs"):
        aug.apply_augmentations(b, torch.eye(3).repeat(2, 1, 1))


def test_row_counts_and_dtypes_are_checked():
    b = _batch()
    b["t"] = torch.zeros(4, 3)  # neither 5 atoms nor 2 systems
    with pytest.raises(ValueError, match="neither the batch's 5 atoms nor its 2 systems"):
        O3Augmenter(dict(KINDS, t="vector")).apply_random_augmentations(b)
    b["t"] = torch.zeros(2, 3)
    with pytest.raises(ValueError, match="2 rows for 5 atoms"):
        O3Augmenter(dict(KINDS, t={"kind": "vector", "per_atom": True})).apply_random_augmentations(b)
    b["t"] = torch.zeros(5, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="float32"):
        O3Augmenter(dict(KINDS, t="vector")).apply_random_augmentations(b)


def test_non_orthogonal_matrices_are_refused():
    aug = O3Augmenter(KINDS)
    good = torch.eye(3, dtype=torch.float64).repeat(2, 1, 1)
    for bad in (good * 1.001, good + torch.tensor([[0.0, 3e-4, 0], [0, 0, 0], [0, 0, 0]]), good * float("nan")):
        with pytest.raises(ValueError, match="not orthogonal"):
            aug.apply_augmentations(_batch(), bad)
    with pytest.raises(ValueError, match=r"\[2,3,3\]"):
        aug.apply_augmentations(_batch(), good[:1])
    # an orthogonal one (to 1e-4) gets as far as the device check
    with pytest.raises(_lib.PetHipError, match="no CPU path"):
        aug.apply_augmentations(_batch(), good * (1 + 2e-5))


def test_masks_scalars_and_non_tensors_need_no_kind_and_are_not_planned():
    """``*_mask`` entries (augmentation.py:118-120), scalars and non-tensor entries are not among the arrays the kernels
    get: the plan (host only) lists positions, cells and the Cartesian targets, nothing else."""
    b = _batch()
    b["forces_mask"] = torch.ones(5, 3, dtype=torch.bool)
    b["pbcs"] = [[True] * 3] * 2
    b["stress"] = torch.zeros(2, 3, 3)
    aug = O3Augmenter(dict(KINDS, stress="tensor2"))
    plan, n, s, tensors = aug._plan(b)
    assert (n, s) == (5, 2)
    assert plan == [("positions", "vector", True), ("cells", "vector", "cells"), ("forces", "vector", True),
                    ("stress", "tensor2", False)]
    assert not any(t is b["forces_mask"] for t in tensors)


def test_state_dict_round_trip():
    aug = O3Augmenter(KINDS, group="inversions", seed=7, stream=3)
    aug.counter = 41
    state = aug.state_dict()
    assert state == {"seed": 7, "stream": 3, "counter": 41, "group": "inversions"}
    other = O3Augmenter(KINDS)
    other.load_state_dict(state)
    assert other.state_dict() == state and other.key == aug.key == (3 << 32) | 7
    # the stream is in the key, not in the counter: two ranks never share a (key, counter) pair
    assert O3Augmenter(KINDS, seed=7, stream=0).key != O3Augmenter(KINDS, seed=7, stream=1).key
    with pytest.raises(ValueError, match="unknown transformation group"):
        other.load_state_dict(dict(state, group="SO3"))
    with pytest.raises(ValueError, match="out of range"):
        other.load_state_dict(dict(state, counter=-1))


def test_c_entry_points_check_their_arguments(lib):
    """PET_ERR_ARGUMENT (-3) before any launch: an unknown group or kind, more than eight arrays, negative counts, an
    in-place request. Pointers are never followed on the host, so made-up ones serve."""
    fake = ctypes.c_void_p(0x1000)
    assert lib.pet_o3_draw(0, 0, 2, 4, fake, None) == _lib.PET_ERR_ARGUMENT
    assert b"group" in lib.pet_last_error()
    assert lib.pet_o3_draw(0, 0, 0, -1, fake, None) == _lib.PET_ERR_ARGUMENT
    assert lib.pet_o3_draw(0, 0, 0, 0, None, None) == 0  # nothing to draw

    def apply(descs, n_systems=2, n=None):
        arr = (_lib.O3Array * max(1, len(descs)))(*descs)
        return lib.pet_o3_apply(fake, n_systems, len(descs) if n is None else n, arr, None)

    ok = _lib.O3Array(0x2000, 0x3000, 2, None, 1, 0)
    assert apply([ok] * 9) == _lib.PET_ERR_ARGUMENT and b"n_arrays" in lib.pet_last_error()
    assert apply([ok], n=-1) == _lib.PET_ERR_ARGUMENT
    assert apply([]) == 0
    assert apply([_lib.O3Array(0x2000, 0x3000, 2, None, 1, 2)]) == _lib.PET_ERR_ARGUMENT and b"kind" in lib.pet_last_error()
    assert apply([_lib.O3Array(0x2000, 0x3000, -2, None, 1, 0)]) == _lib.PET_ERR_ARGUMENT
    assert apply([_lib.O3Array(0x2000, 0x3000, 2, None, -1, 1)]) == _lib.PET_ERR_ARGUMENT
    assert apply([_lib.O3Array(0x2000, 0x2000, 2, None, 1, 0)]) == _lib.PET_ERR_ARGUMENT and b"out of place" in lib.pet_last_error()
    assert apply([_lib.O3Array(0x2000, 0x3000, 3, None, 1, 0)]) == _lib.PET_ERR_ARGUMENT  # 3 rows, 2 systems, no map
    assert apply([ok], n_systems=-1) == _lib.PET_ERR_ARGUMENT
    assert apply([_lib.O3Array(0x2000, 0x3000, 0, None, 4, 1)]) == 0  # an empty array launches nothing
