"""Host side of the spherical-target path of the device augmenter (``pet_o3_wigner`` / ``pet_o3_apply_spherical``): what the
augmenter accepts and refuses, the C entry points' argument checks, the identities of the numpy oracle the GPU tests lean on
(``tests/_wigner_oracle.py``), and the recursion of ``csrc/wigner.h`` itself, compiled by the host compiler into a stand-alone
program (``tests/wigner_host_main.cpp``) and compared with that oracle. No GPU call is made."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _wigner_oracle as wo
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
    }


def _rotation(seed: int, proper: bool = True) -> np.ndarray:
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if (np.linalg.det(q) > 0) == proper else -q


# ---- the augmenter's host side ------------------------------------------------------------------------------------------------
def test_the_reference_spelling_is_accepted_and_checked():
    for lam in range(9):
        for sigma in (1, -1):
            aug = O3Augmenter({"t": {"kind": "spherical", "o3_lambda": lam, "o3_sigma": sigma, "per_atom": True}})
            if (lam, sigma) == (0, 1):  # an invariant: a scalar, no table
                assert aug.kinds["t"]["kind"] == "scalar" and aug.l_max is None
            else:
                assert aug.kinds["t"] == {"kind": "spherical", "per_atom": True, "o3_lambda": lam, "o3_sigma": sigma}
                assert aug.l_max == lam
    aug = O3Augmenter({"a": {"kind": "spherical", "o3_lambda": 3}, "b": {"kind": "spherical", "o3_lambda": 1, "o3_sigma": -1},
                       "forces": "vector"})
    assert aug.l_max == 3 and aug.kinds["a"]["o3_sigma"] == 1
    assert O3Augmenter({"energy": "scalar", "forces": "vector"}).l_max is None
    with pytest.raises(ValueError, match=r"o3_lambda must be an integer in \[0, 8\], got 9"):
        O3Augmenter({"t": {"kind": "spherical", "o3_lambda": 9}})
    with pytest.raises(ValueError, match="o3_lambda must be an integer"):
        O3Augmenter({"t": {"kind": "spherical", "o3_lambda": -1}})
    with pytest.raises(ValueError, match=r"o3_sigma must be \+1 or -1, got 0"):
        O3Augmenter({"t": {"kind": "spherical", "o3_lambda": 2, "o3_sigma": 0}})
    for kind in ("vector", "tensor2", "scalar"):
        with pytest.raises(ValueError, match="'o3_lambda' / 'o3_sigma' belong to the kind 'spherical'"):
            O3Augmenter({"t": {"kind": kind, "o3_lambda": 1}})
    with pytest.raises(ValueError, match="not both"):
        O3Augmenter({"t": {"kind": "spherical", "o3_lambda": 1, "sigma": 1}})
    for name in ("o3_wigner", "o3_parity"):
        with pytest.raises(ValueError, match="part of the batch itself"):
            O3Augmenter({name: "vector"})
    with pytest.raises(ValueError, match="Wigner-D"):  # the short spelling keeps its refusal
        O3Augmenter({"t": {"kind": "spherical", "lambda": 1}})


@pytest.mark.parametrize("lam,shape", [(2, (5, 4)), (2, (5,)), (2, (5, 3, 2)), (1, (2, 4)), (8, (5, 16))])
def test_wrong_trailing_shapes_of_a_spherical_block_are_refused(lam, shape):
    b = _batch()
    b["t"] = torch.zeros(shape)
    aug = O3Augmenter({"t": {"kind": "spherical", "o3_lambda": lam}})
    message = rf"a spherical block of o3_lambda = {lam} needs \(2l\+1\) x P = {2 * lam + 1} x P values per row"
    with pytest.raises(ValueError, match=message):
        aug.apply_random_augmentations(b)
    with pytest.raises(ValueError, match=message):
        aug.apply_augmentations(b, torch.eye(3).repeat(2, 1, 1))


def test_spherical_blocks_are_planned_and_the_added_keys_are_not():
    b = _batch()
    b["q"] = torch.zeros(5, 5, 2)  # per atom, l = 2, P = 2
    b["mu"] = torch.zeros(2, 3)  # per system, l = 1
    b["e"] = torch.zeros(2, 1)
    b["o3_wigner"], b["o3_parity"] = torch.zeros(2, 10), torch.zeros(2)  # an augmented batch handed in again
    aug = O3Augmenter({"q": {"kind": "spherical", "o3_lambda": 2}, "mu": {"kind": "spherical", "o3_lambda": 1, "o3_sigma": -1},
                       "e": {"kind": "spherical", "o3_lambda": 0, "o3_sigma": 1}})
    plan, n, s, tensors = aug._plan(b)
    assert plan == [("positions", "vector", True), ("cells", "vector", "cells"), ("q", "spherical", True), ("mu", "spherical", False)]
    assert not any(t is b["o3_wigner"] or t is b["o3_parity"] or t is b["e"] for t in tensors)
    b["mu"] = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="neither the batch's 5 atoms nor its 2 systems"):
        aug._plan(b)
    b["mu"] = torch.zeros(2, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="float32"):
        aug._plan(b)


def test_cpu_tensors_raise_no_cpu_path():
    b = _batch()
    b["mu"] = torch.zeros(2, 3)
    aug = O3Augmenter({"mu": {"kind": "spherical", "o3_lambda": 1}})
    with pytest.raises(_lib.PetHipError, match="no CPU path"):
        aug.apply_random_augmentations(b)
    assert aug.counter == 0
    with pytest.raises(_lib.PetHipError, match="no CPU path"):
        rt.o3_wigner(torch.eye(3).repeat(2, 1, 1), 2)
    with pytest.raises(_lib.PetHipError, match="no CPU path"):
        rt.o3_apply_spherical(torch.zeros(2, 10), torch.ones(2), 1, [(torch.zeros(2, 3), 1, 1, None)])
    table = torch.arange(2 * 35, dtype=torch.float32).reshape(2, 35)  # the view needs no device
    block = rt.o3_wigner_block(table, 2)
    assert block.shape == (2, 5, 5) and block.data_ptr() == table[:, 10:].data_ptr() and float(block[1, 4, 4]) == 69.0
    with pytest.raises(ValueError, match="holds no block of l = 4"):
        rt.o3_wigner_block(table, 4)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_symbols_and_struct_agree(lib):
    header = open(os.path.join(ROOT, "include", "pet_hip.h")).read()
    declared = set(re.findall(r"\b(pet_[a-z0-9_]+)\s*\(", header))
    for name in ("pet_o3_wigner", "pet_o3_apply_spherical"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert declared == set(_lib.SYMBOLS)
    # two pointers, a count, a pointer, three int32, padded to the pointers' alignment; pet_o3_array_t is untouched
    assert ctypes.sizeof(_lib.O3SphericalArray) == 48 and ctypes.sizeof(_lib.O3Array) == 40
    assert [f[0] for f in _lib.O3SphericalArray._fields_] == ["src", "dst", "rows", "system_of_row", "n_properties", "o3_lambda",
                                                              "o3_sigma"]
    struct = re.search(r"typedef struct pet_o3_spherical_array \{(.*?)\} pet_o3_spherical_array_t;", header, re.S).group(1)
    assert re.findall(r"(\w+);", struct) == [f[0] for f in _lib.O3SphericalArray._fields_]
    assert re.search(rf"^#define PET_O3_MAX_L {_lib.PET_O3_MAX_L}$", header, re.M) and _lib.PET_O3_MAX_L == wo.L_MAX == 8
    assert [wo.offset(l) for l in range(4)] == [0, 1, 10, 35] and wo.width(8) == 969


def test_c_entry_points_check_their_arguments(lib):
    """PET_ERR_ARGUMENT (-3) before any launch. Pointers are never followed on the host, so made-up ones serve."""
    fake, fake2, fake3 = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x5000), ctypes.c_void_p(0x9000)
    bad = _lib.PET_ERR_ARGUMENT
    assert lib.pet_o3_wigner(fake, 4, -1, fake2, fake3, None) == bad and b"l_max" in lib.pet_last_error()
    assert lib.pet_o3_wigner(fake, 4, 9, fake2, fake3, None) == bad
    assert lib.pet_o3_wigner(fake, -1, 2, fake2, fake3, None) == bad
    assert lib.pet_o3_wigner(fake, 4, 2, None, fake3, None) == bad
    assert lib.pet_o3_wigner(fake, 4, 2, fake, fake3, None) == bad  # the table over the matrices
    assert lib.pet_o3_wigner(None, 0, 2, None, None, None) == 0  # nothing to build

    def apply(descs, n_systems=2, n=None, l_max=8):
        arr = (_lib.O3SphericalArray * max(1, len(descs)))(*descs)
        return lib.pet_o3_apply_spherical(fake, fake2, l_max, n_systems, len(descs) if n is None else n, arr, None)

    def desc(src=0x2000, dst=0x3000, rows=2, sor=None, p=1, lam=1, sigma=1):
        return _lib.O3SphericalArray(src, dst, rows, sor, p, lam, sigma)

    assert apply([desc()] * 9) == bad and b"n_arrays" in lib.pet_last_error()
    assert apply([desc()], n=-1) == bad
    assert apply([]) == 0
    assert apply([desc()], l_max=9) == bad and b"l_max" in lib.pet_last_error()
    assert apply([desc()], l_max=-1) == bad
    assert apply([desc(lam=9)]) == bad and b"o3_lambda" in lib.pet_last_error()
    assert apply([desc(lam=-1)]) == bad
    assert apply([desc(lam=3)], l_max=2) == bad and b"above the table's l_max" in lib.pet_last_error()
    for sigma in (0, 2, -2):
        assert apply([desc(sigma=sigma)]) == bad and b"o3_sigma" in lib.pet_last_error()
    assert apply([desc(rows=-2)]) == bad
    assert apply([desc(p=-1)]) == bad
    assert apply([desc(dst=0x2000)]) == bad and b"out of place" in lib.pet_last_error()
    assert apply([desc(rows=3)]) == bad  # 3 rows, 2 systems, no map
    assert apply([desc()], n_systems=-1) == bad
    assert apply([desc(rows=0, p=4)]) == 0 and apply([desc(p=0)]) == 0  # an empty array launches nothing
    # the Cartesian entry point is as it was: it knows no third kind
    assert lib.pet_o3_apply(fake, 2, 1, (_lib.O3Array * 1)(_lib.O3Array(0x2000, 0x3000, 2, None, 1, 2)), None) == bad


# ---- the oracle's own identities ------------------------------------------------------------------------------------------------
def test_oracle_harmonics_are_the_stated_ones_and_orthonormal():
    u = wo.SAMPLES[:50]
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    pi = math.pi
    assert np.abs(wo.real_harmonics(0, u)[:, 0] - math.sqrt(1 / (4 * pi))).max() < 1e-15
    assert np.abs(wo.real_harmonics(1, u) - math.sqrt(3 / (4 * pi)) * np.stack([y, z, x], 1)).max() < 1e-15
    y2 = np.stack([math.sqrt(15 / (4 * pi)) * x * y, math.sqrt(15 / (4 * pi)) * y * z, math.sqrt(5 / (16 * pi)) * (3 * z * z - 1),
                   math.sqrt(15 / (4 * pi)) * x * z, math.sqrt(15 / (16 * pi)) * (x * x - y * y)], 1)
    assert np.abs(wo.real_harmonics(2, u) - y2).max() < 1e-15
    # orthonormal on the sphere: a Gauss-Legendre x uniform-azimuth rule that is exact for polynomials of degree 2 * 8
    nodes, weights = np.polynomial.legendre.leggauss(12)
    phi = 2 * pi * np.arange(20) / 20
    zz, pp = np.meshgrid(nodes, phi, indexing="ij")
    st = np.sqrt(1 - zz ** 2)
    grid = np.stack([st * np.cos(pp), st * np.sin(pp), zz], -1).reshape(-1, 3)
    wts = np.repeat(weights, 20) * (2 * pi / 20)
    for l in range(9):
        yl = wo.real_harmonics(l, grid)
        assert np.abs((yl * wts[:, None]).T @ yl - np.eye(2 * l + 1)).max() < 1e-13, l


def test_oracle_identities():
    q1, q2 = _rotation(1), _rotation(2)
    for l in range(9):
        assert wo.condition_number(l) <= 1.5, l
        d1, d2, d12 = wo.wigner_d(l, q1), wo.wigner_d(l, q2), wo.wigner_d(l, q1 @ q2)
        assert np.abs(d1 @ d1.T - np.eye(2 * l + 1)).max() < 4e-15, l
        assert np.abs(d1 @ d2 - d12).max() < 3e-15, l
        # the defining property on vectors that are not among the fitted samples
        u = np.random.default_rng(5).standard_normal((20, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        assert np.abs(wo.real_harmonics(l, u @ q1.T) - wo.real_harmonics(l, u) @ d1.T).max() < 5e-15, l
    assert np.abs(wo.wigner_d(1, q1) - wo.P_YZX @ q1 @ wo.P_YZX.T).max() < 8e-16
    t = np.random.default_rng(3).standard_normal((3, 3))
    t = t + t.T
    t -= np.eye(3) * np.trace(t) / 3
    got = wo.wigner_d(2, q1) @ wo.symmetric_traceless_to_l2(t)
    assert np.abs(got - wo.symmetric_traceless_to_l2(q1 @ t @ q1.T)).max() < 7e-16 * max(1.0, np.abs(t).max())
    tab, det = wo.table(-q2, 3)
    assert det == -1.0 and tab.shape == (84,) and np.abs(tab[10:35].reshape(5, 5) - wo.wigner_d(2, q2)).max() < 1e-15


# ---- the recursion, on the host ---------------------------------------------------------------------------------------------------
HOST_MATRICES = [_rotation(21), _rotation(22), _rotation(23), _rotation(24, False), _rotation(25, False), np.eye(3)]


@pytest.fixture(scope="module")
def host_tables(tmp_path_factory):
    """``csrc/wigner.h`` through the host compiler: the tables (fp64, before the device's one rounding) of six matrices."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ to build the host program with")
    exe = str(tmp_path_factory.mktemp("wigner") / "wigner_host")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "metatrain_amd", "csrc"),
                    os.path.join(ROOT, "tests", "wigner_host_main.cpp"), "-o", exe], check=True)

    def run(matrices, l_max=8):
        text = f"{l_max}\n" + "\n".join(" ".join(repr(float(v)) for v in np.asarray(m).reshape(-1)) for m in matrices)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
        rows = np.array([[float(v) for v in line.split()] for line in out.strip().split("\n")])
        return rows[:, 0], rows[:, 1:]

    return run


def test_the_recursion_on_the_host_matches_the_oracle(host_tables):
    parity, tables = host_tables(HOST_MATRICES)
    assert tables.shape == (6, 969)
    assert parity.tolist() == [1.0, 1.0, 1.0, -1.0, -1.0, 1.0]
    for i, m in enumerate(HOST_MATRICES):
        want, det = wo.table(m, 8)
        assert det == parity[i]
        for l in range(9):
            got = tables[i, wo.offset(l):wo.offset(l + 1)]
            err = np.abs(got - want[wo.offset(l):wo.offset(l + 1)]).max()
            assert err <= 1e-13, (i, l, err)
            if i == 5:
                assert np.array_equal(got.reshape(2 * l + 1, 2 * l + 1), np.eye(2 * l + 1)), l  # exactly, not to rounding


def test_the_recursion_on_the_host_handles_inversion_nan_and_short_tables(host_tables):
    nan = np.eye(3)
    nan[1, 2] = float("nan")
    parity, tables = host_tables([-np.eye(3), nan, HOST_MATRICES[0] * (1 + 1e-5)])
    assert parity[0] == -1.0 and np.array_equal(tables[0], wo.table(np.eye(3), 8)[0].round())  # -I: identity blocks, exactly
    assert math.isnan(parity[1]) and np.isnan(tables[1]).all()  # the l = 0 entry included
    # a matrix 1e-5 away from orthogonal gives a table about l x 1e-5 away, not garbage (entries are degree-l polynomials)
    want = wo.table(HOST_MATRICES[0], 8)[0]
    for l in range(9):
        sl = slice(wo.offset(l), wo.offset(l + 1))
        assert np.abs(tables[2][sl] - (1 + 1e-5) ** l * want[sl]).max() <= 1e-13, l
    _, short = host_tables(HOST_MATRICES[:2], l_max=3)
    _, full = host_tables(HOST_MATRICES[:2])
    assert short.shape == (2, 84) and np.array_equal(short, full[:, :84])
