"""Composition baselines and target scales, host side: ``fit`` of ``CompositionHip`` / ``ScalerHip`` from hand-made accumulators
against the fp64 restatement of the reference (``tests/_baseline_oracle.py``), the state round trip, a 2-rank gloo all-reduce
of host accumulators, the refusals, and the translation unit's register report. No GPU."""
import os
import re
import shutil
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _baseline_oracle as oracle
from metatrain_amd import _lib, baseline as bl, build as mbuild
from metatrain_amd._lib import PetHipError

TYPES = [1, 6, 7, 8]
ENERGY = {"energy": {"per_atom": False, "shape": [1]}}


def _structures(rng, n_sys, n_types, absent=None, lo=1, hi=12):
    """Random per-structure type counts [S, T] with the column ``absent`` zero."""
    c = rng.integers(lo, hi, size=(n_sys, n_types))
    c[rng.random((n_sys, n_types)) < 0.3] = 0
    c[:, 0] += 1  # no empty system
    if absent is not None:
        c[:, absent] = 0
    return c.astype(np.int64)


def _set(comp, name, xtx, xty, block=None):
    block = name if block is None else block
    comp.XTX[name][block] = torch.tensor(np.asarray(xtx), dtype=torch.int64)
    comp.XTY[name][block] = torch.tensor(np.asarray(xty), dtype=torch.float64)


def test_fit_ordinary_four_types_matches_the_oracle_solve():
    rng = np.random.default_rng(0)
    X = _structures(rng, 40, 4)
    w_true = np.array([[-13.6], [-1030.0], [-1480.0], [-2040.0]])
    Y = X @ w_true + rng.normal(size=(40, 1))
    xtx, xty = oracle.composition_accumulate(False, X, Y)
    comp = bl.CompositionHip(TYPES, ENERGY)
    _set(comp, "energy", xtx, xty)
    comp.fit()
    want = oracle.composition_fit(TYPES, False, xtx, xty)
    got = comp.weights("energy").numpy()
    assert got.shape == (4, 1) and got.dtype == np.float64
    cond = np.linalg.cond(xtx.astype(np.float64))
    assert np.abs(got - want).max() <= 10 * cond * 2.0 ** -53 * np.abs(want).max()
    assert np.abs(got - w_true).max() < 1.0  # and it is a fit of the data
    table = comp.table("energy")
    assert table.dtype == torch.float32 and tuple(table.shape) == (9,)
    assert torch.equal(table[torch.tensor(TYPES)], torch.tensor(got[:, 0]).float())
    assert float(table[torch.tensor([0, 2, 3, 4, 5])].abs().max()) == 0.0


def test_fit_type_never_seen_gets_exactly_zero():
    rng = np.random.default_rng(1)
    X = _structures(rng, 30, 4, absent=2)
    Y = X @ np.array([[-1.0], [-2.0], [5.0], [-3.0]]) + 0.01 * rng.normal(size=(30, 1))
    xtx, xty = oracle.composition_accumulate(False, X, Y)
    comp = bl.CompositionHip(TYPES, ENERGY)
    _set(comp, "energy", xtx, xty)
    comp.fit()
    got = comp.weights("energy").numpy()
    assert got[2, 0] == 0.0  # a zero row and column with the regulariser on the diagonal: 0 / reg
    want = oracle.composition_fit(TYPES, False, xtx, xty)
    assert want[2, 0] == 0.0
    seen = [0, 1, 3]
    cond = np.linalg.cond(xtx[np.ix_(seen, seen)].astype(np.float64))
    assert np.abs(got - want).max() <= 10 * cond * 2.0 ** -53 * np.abs(want).max()


def test_fit_all_zero_xtx_gives_zeros():
    comp = bl.CompositionHip(TYPES, {"e": {"per_atom": False, "shape": [3, 2]}})
    comp.XTY["e"]["e"] += 7.0  # whatever XTY holds
    comp.fit()
    assert torch.equal(comp.weights("e"), torch.zeros((4, 6), dtype=torch.float64))
    assert np.array_equal(oracle.composition_fit(TYPES, False, np.zeros((4, 4)), np.full((4, 6), 7.0)), np.zeros((4, 6)))


def test_fixed_weights_float_dict_and_missing_type():
    comp = bl.CompositionHip(TYPES, {"energy": {"per_atom": False, "shape": [1]}, "other": {"per_atom": False, "shape": [2]}})
    rng = np.random.default_rng(2)
    X = _structures(rng, 20, 4)
    xtx, xty = oracle.composition_accumulate(False, X, rng.normal(size=(20, 2)))
    _set(comp, "other", xtx, xty)
    comp.fit(fixed_weights={"energy": 2.5, "unknown": 1.0})
    assert np.array_equal(comp.weights("energy").numpy(), oracle.composition_fit(TYPES, False, xtx, np.zeros((4, 1)), fixed=2.5))
    assert np.abs(comp.weights("other").numpy() - oracle.composition_fit(TYPES, False, xtx, xty)).max() < 1e-12  # still fitted
    d = {1: -0.5, 6: -37.0, 7: -54.0, 8: -75.0}
    comp.fit(fixed_weights={"other": d})
    assert np.array_equal(comp.weights("other").numpy(), oracle.composition_fit(TYPES, False, xtx, xty, fixed=d))
    assert np.array_equal(comp.weights("other").numpy()[:, 1], [-0.5, -37.0, -54.0, -75.0])
    with pytest.raises(ValueError, match="missing the following atomic types"):
        comp.fit(fixed_weights={"other": {1: 0.0, 6: 0.0, 8: 0.0}})
    with pytest.raises(ValueError, match="missing the following atomic types"):
        oracle.composition_fit(TYPES, False, xtx, xty, fixed={1: 0.0, 6: 0.0, 8: 0.0})


def test_per_atom_fit_with_a_zero_count_type():
    rng = np.random.default_rng(3)
    species = rng.choice([1, 6, 8], size=50)  # no nitrogen
    Y = rng.normal(size=(50, 3))
    X = oracle.one_hot(TYPES, species)
    xtx, xty = oracle.composition_accumulate(True, X, Y)
    comp = bl.CompositionHip(TYPES, {"q": {"per_atom": True, "shape": [3]}})
    _set(comp, "q", xtx, xty)
    comp.fit()
    got = comp.weights("q").numpy()
    assert np.array_equal(got, oracle.composition_fit(TYPES, True, xtx, xty))  # one division per entry: the same bits
    assert np.array_equal(got[2], np.zeros(3))
    for k, z in enumerate(TYPES):
        if z != 7:
            assert np.allclose(got[k], Y[species == z].mean(axis=0), rtol=1e-13, atol=1e-15)


def test_not_finite_weights_raise():
    comp = bl.CompositionHip(TYPES, {"q": {"per_atom": True, "shape": [1]}})
    _set(comp, "q", np.diag([3, 2, 0, 1]), [[1.0], [float("nan")], [0.0], [2.0]])
    with pytest.raises(PetHipError, match="not finite"):
        comp.fit()


def test_scaler_fit_and_no_samples_gives_one():
    sc = bl.ScalerHip(TYPES, {"energy": {"per_atom": False, "shape": [1]}, "q": {"per_atom": True, "shape": [1]}})
    sc.N["energy"][:] = 0
    sc.N["q"] = torch.tensor([10, 0, 4, 1])
    sc.Y2["q"] = torch.tensor([2.5, 0.0, 16.0, 9.0], dtype=torch.float64)
    sc.fit()
    assert sc.scale("energy") == 1.0  # 0 / 0 -> NaN -> 1.0
    want = oracle.scaler_fit([10, 0, 4, 1], [2.5, 0.0, 16.0, 9.0])
    assert np.array_equal(sc.scale("q").numpy(), want) and want[1] == 1.0 and want[2] == 2.0
    sc.fit(fixed_weights={"energy": 3.0, "q": {1: 1.0, 6: 2.0, 7: 3.0, 8: 4.0}})
    assert sc.scale("energy") == 3.0 and sc.scale("q").tolist() == [1.0, 2.0, 3.0, 4.0]
    with pytest.raises(ValueError, match="Atomic type 7 is missing"):
        sc.fit(fixed_weights={"q": {1: 1.0, 6: 2.0, 8: 4.0}})
    with pytest.raises(ValueError, match="not supported for per-structure"):
        sc.fit(fixed_weights={"energy": {1: 1.0, 6: 2.0, 7: 3.0, 8: 4.0}})


def test_per_property_scales_multiply_per_target_ones():
    sc = bl.ScalerHip(TYPES, {"nc": {"per_atom": False, "shape": {"a": [3, 2], "b": [4]}}})
    assert sc.multi_property == ["nc"]
    sc.N["nc"][:] = 50
    sc.Y2["nc"][:] = 200.0
    sc.fit()
    assert sc.scale("nc") == 2.0
    sc.per_property_N["nc"]["a"] = torch.tensor([[30, 0]])
    sc.per_property_Y2["nc"]["a"] = torch.tensor([[270.0, 0.0]], dtype=torch.float64)
    sc.per_property_N["nc"]["b"] = torch.tensor([[5, 5, 5, 5]])
    sc.per_property_Y2["nc"]["b"] = torch.tensor([[5.0, 20.0, 45.0, 1.25]], dtype=torch.float64)
    sc.fit_per_property()
    pp = sc.property_scales("nc")
    assert pp["a"].tolist() == [3.0, 1.0] and pp["b"].tolist() == [1.0, 2.0, 3.0, 0.5]
    full = sc.full_scales("nc")
    for b, n, y2 in (("a", [30, 0], [270.0, 0.0]), ("b", [5] * 4, [5.0, 20.0, 45.0, 1.25])):
        with np.errstate(invalid="ignore"):
            raw = np.sqrt(np.array(y2) / np.array(n))
        assert np.array_equal(full[b].numpy(), oracle.full_scales(2.0, raw))  # _base_scaler.py:599-607
    assert full["a"].tolist() == [6.0, 1.0]


def test_refusals_name_what_is_not_served():
    with pytest.raises(ValueError, match="per-property scales.*per atomic type"):
        bl.ScalerHip(TYPES, {"q": {"per_atom": True, "shape": [3]}})
    with pytest.raises(ValueError, match="atomic-basis"):
        bl.CompositionHip(TYPES, {"rho": {"per_atom": True, "shape": [1], "atom_type": True}})
    with pytest.raises(ValueError, match="atom-pair"):
        bl.ScalerHip(TYPES, {"h": {"sample_kind": "atom_pair", "shape": [1]}})
    with pytest.raises(ValueError, match="o3_lambda_1"):
        bl.CompositionHip(TYPES, {"t": {"per_atom": False, "shape": [3, 3, 1], "o3_lambda_1": True}})
    with pytest.raises(PetHipError, match="TensorMap checkpoint buffers"):
        bl.CompositionHip(TYPES, ENERGY).load_state_dict({"energy_composition_buffer": b"..."})
    with pytest.raises(PetHipError, match="call fit"):
        bl.CompositionHip(TYPES, ENERGY).weights("energy")
    cpu_batch = {"species": torch.tensor([1, 6], dtype=torch.int32), "system_indices": torch.zeros(2, dtype=torch.int32),
                 "cells": torch.zeros(1, 3, 3), "energy": torch.zeros(1, dtype=torch.float64)}
    with pytest.raises(PetHipError, match="MI355X only"):
        bl.CompositionHip(TYPES, ENERGY).accumulate(cpu_batch)
    with pytest.raises(PetHipError, match="MI355X only"):
        bl.ScalerHip(TYPES, ENERGY).accumulate(cpu_batch)


def test_state_dict_round_trip():
    rng = np.random.default_rng(4)
    X = _structures(rng, 25, 4)
    xtx, xty = oracle.composition_accumulate(False, X, rng.normal(size=(25, 1)))
    comp = bl.CompositionHip(TYPES, ENERGY)
    _set(comp, "energy", xtx, xty)
    comp.fit()
    state = comp.state_dict()
    assert all(torch.is_tensor(v) for v in state.values())
    other = bl.CompositionHip(TYPES, ENERGY)
    other.load_state_dict(state)
    assert torch.equal(other.weights("energy"), comp.weights("energy"))
    assert torch.equal(other.XTX["energy"]["energy"], comp.XTX["energy"]["energy"])  # accumulators included: a resumed fit goes on
    other.fit()
    assert torch.equal(other.weights("energy"), comp.weights("energy"))
    with pytest.raises(ValueError, match="atomic types"):
        bl.CompositionHip([1, 6], ENERGY).load_state_dict(state)

    sc = bl.ScalerHip(TYPES, {"energy": {"per_atom": False, "shape": [1]}, "nc": {"per_atom": False, "shape": [3, 2]}})
    sc.N["energy"][:] = 7
    sc.Y2["energy"][:] = 28.0
    sc.per_property_N["nc"]["nc"][:] = 3
    sc.per_property_Y2["nc"]["nc"] = torch.tensor([[3.0, 12.0]], dtype=torch.float64)
    sc._declare_zbl(True)
    sc.fit()
    sc.fit_per_property()
    s2 = bl.ScalerHip(TYPES, {"energy": {"per_atom": False, "shape": [1]}, "nc": {"per_atom": False, "shape": [3, 2]}})
    s2.load_state_dict(sc.state_dict())
    assert s2.scale("energy") == 2.0 and s2.zbl_removed is True
    assert s2.property_scales("nc")["nc"].tolist() == [1.0, 2.0]
    assert torch.equal(s2.N["energy"], sc.N["energy"]) and torch.equal(s2.per_property_Y2["nc"]["nc"], sc.per_property_Y2["nc"]["nc"])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_data(rank):
    rng = np.random.default_rng(100 + rank)
    X = _structures(rng, 16, 4)
    Y = X @ np.array([[-1.0], [-2.0], [-3.0], [-4.0]]) + rng.normal(size=(16, 1))
    return X, Y


def _reduce_worker(rank, world, port, out):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    X, Y = _rank_data(rank)
    xtx, xty = oracle.composition_accumulate(False, X, Y)
    comp = bl.CompositionHip(TYPES, ENERGY)
    _set(comp, "energy", xtx, xty)
    comp.all_reduce()
    comp.fit()
    w = comp.weights("energy")
    r = oracle.residual(False, Y, w.numpy(), X, X.sum(axis=1))
    n, y2 = oracle.n_and_y2(False, r, False)
    sc = bl.ScalerHip(TYPES, ENERGY)
    sc.N["energy"] += torch.tensor(n.reshape(-1))
    sc.Y2["energy"] += torch.tensor(y2.reshape(-1))
    sc.all_reduce()
    sc.fit()
    out.put((rank, w.numpy(), comp.XTX["energy"]["energy"].numpy(), sc.scale("energy"), int(sc.N["energy"][0])))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_rank_gloo_all_reduce_gives_the_single_process_fit():
    world = 2
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((out.get(timeout=120) for _ in range(world)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (X0, Y0), (X1, Y1) = _rank_data(0), _rank_data(1)
    X, Y = np.concatenate([X0, X1]), np.concatenate([Y0, Y1])
    single = bl.CompositionHip(TYPES, ENERGY)
    a0, b0 = oracle.composition_accumulate(False, X0, Y0)
    a1, b1 = oracle.composition_accumulate(False, X1, Y1)
    _set(single, "energy", a0 + a1, b0 + b1)  # a two-term sum is the same in either order
    single.fit()
    w = single.weights("energy").numpy()
    n, y2 = oracle.n_and_y2(False, oracle.residual(False, Y, w, X, X.sum(axis=1)), False)
    for rank, w_r, xtx_r, scale_r, n_r in res:
        assert np.array_equal(xtx_r, X.T @ X)
        assert np.array_equal(w_r, w)  # both ranks: the bits of the single-process fit
        assert n_r == 32
        assert abs(scale_r - float(oracle.scaler_fit(n, y2)[0, 0])) <= 1e-14 * scale_r
    assert res[0][3] == res[1][3]
    with pytest.raises(PetHipError, match="process group"):
        single.all_reduce()


def test_header_symbols_are_listed_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(bl.__file__))), "include", "pet_hip.h")).read()
    names = ["pet_baseline_workspace_bytes", "pet_species_counts", "pet_composition_accumulate", "pet_target_moments",
             "pet_targets_remove"]
    lib = _lib.load()
    for n in names:
        assert re.search(rf"\b{n}\(", header) and n in _lib.SYMBOLS and hasattr(lib, n)
    assert lib.pet_baseline_workspace_bytes(257, 4, 3) >= 8 * 2 * 4 * (4 + 3)
    assert lib.pet_baseline_workspace_bytes(-1, 4, 3) < 0


def test_translation_unit_cross_compiles_without_scratch(tmp_path):
    """``baseline.hip`` with the build's own flags for gfx950: part of SOURCES and NO_RDC (its report is per file), every
    kernel at ScratchSize 0."""
    assert "baseline.hip" in mbuild.SOURCES and "baseline.hip" in mbuild.NO_RDC
    assert shutil.which("hipcc") is not None, "the build needs hipcc"
    cmd = ["hipcc", *mbuild.FLAGS, "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(mbuild.CSRC, "baseline.hip"), "-o", str(tmp_path / "baseline.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(kernels) >= 7 and len(scratch) == len(kernels)
    assert scratch == [0] * len(scratch), dict(zip(kernels, scratch))
