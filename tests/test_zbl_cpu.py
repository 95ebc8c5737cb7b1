"""ZBL additive model, host side: the pair table of ``pet_zbl_create`` against constants recomputed in torch fp64, the test
helper (``tests/zbl_ref.py``) against the reference's per-pair energies recorded in ``tests/golden/zbl_*.npz``
(``make_golden_zbl.py``), the cutoff, the checkpoint buffers, and the refusals. No GPU."""
import logging
import os

import numpy as np
import pytest
import torch

import zbl_ref
from metatrain_amd import zbl as mzbl
from metatrain_amd._lib import PetHipError

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["box_a", "box_a_sheared", "box_b", "one_atom", "qm9_compressed"]


def load(name):
    return dict(np.load(os.path.join(GOLD, f"zbl_{name}.npz")))


@pytest.mark.parametrize("name", CASES)
def test_pair_table_matches_recomputed_constants(name):
    f = load(name)
    types = [int(z) for z in f["atomic_types"]]
    z = mzbl.ZBLHip(types, covalent_radii=dict(zip(types, f["radii"].tolist())))
    table = z.pair_table()
    zz = torch.tensor(types)
    rad = torch.tensor(f["radii"])
    want = zbl_ref.pair_constants(zz[:, None].expand(-1, len(types)), zz[None, :].expand(len(types), -1),
                                  rad[:, None].expand(-1, len(types)), rad[None, :].expand(len(types), -1))
    rel = ((table - want).abs() / want.abs().clamp_min(1e-300)).max()
    assert float(rel) < 1e-12, float(rel)
    assert z.cutoff == pytest.approx(2.0 * float(rad.max()), abs=1e-15)


@pytest.mark.parametrize("name", CASES)
def test_helper_reproduces_reference_pair_energies(name):
    f = load(name)
    pos, cells = torch.tensor(f["positions"]), torch.tensor(f["cells"])
    numbers, sysidx = torch.tensor(f["numbers"]).long(), torch.tensor(f["system_indices"]).long()
    pairs = torch.tensor(f["pairs"]).long()
    radii_of = torch.tensor(f["radii_table"])
    i, j, S = pairs[:, 0], pairs[:, 1], pairs[:, 2:5].double()
    D = pos[j] - pos[i] + torch.einsum("ea,eab->eb", S, cells[sysidx[i]])
    r = torch.sqrt((D * D).sum(1))
    e = zbl_ref.pair_energy(numbers[i], numbers[j], radii_of[numbers[i]], radii_of[numbers[j]], r)
    ref = torch.tensor(f["pair_energy"])
    assert float((e - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    atomic = zbl_ref.atomic_energies(pos, cells, sysidx, numbers, radii_of, pairs)
    assert float((atomic - torch.tensor(f["atomic"])).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    assert int((ref != 0).sum()) >= 6  # the fixture is not all zeros


def test_helper_gradients_match_reference_autograd():
    f = load("box_a_sheared")
    pos = torch.tensor(f["positions"], requires_grad=True)
    cells = torch.tensor(f["cells"], requires_grad=True)
    numbers, sysidx = torch.tensor(f["numbers"]).long(), torch.tensor(f["system_indices"]).long()
    a = zbl_ref.atomic_energies(pos, cells, sysidx, numbers, torch.tensor(f["radii_table"]), torch.tensor(f["pairs"]))
    gp, gc = torch.autograd.grad(a.sum(), [pos, cells])
    scale = float(np.abs(f["grad_positions"]).max())
    assert float((gp - torch.tensor(f["grad_positions"])).abs().max()) < 1e-11 * scale
    assert float((gc - torch.tensor(f["grad_cells"])).abs().max()) < 1e-11 * float(np.abs(f["grad_cells"]).max())
    # dE/d(eps) = R^T dE/dR + h^T dE/dh
    virial = pos.detach().T @ gp + cells.detach()[0].T @ gc[0]
    assert float((virial - torch.tensor(f["grad_strain"][0])).abs().max()) < 1e-10 * float(np.abs(f["grad_strain"]).max())


def test_default_radii_equal_the_fixture_table():
    table = load("box_a")["radii_table"]
    assert sorted(mzbl.DEFAULT_COVALENT_RADII) == list(range(1, 37))
    for z, r in mzbl.DEFAULT_COVALENT_RADII.items():
        assert r == table[z], (z, r, table[z])


def test_state_dict_round_trip_uses_the_reference_keys():
    z = mzbl.ZBLHip([1, 6, 8, 29])
    sd = z.state_dict("additive_models.1.")
    assert set(sd) == {"additive_models.1.covalent_radii", "additive_models.1.species_to_index"}
    assert sd["additive_models.1.covalent_radii"].dtype == torch.float64
    assert sd["additive_models.1.covalent_radii"].tolist() == [0.31, 0.76, 0.66, 1.32]
    idx = sd["additive_models.1.species_to_index"]
    assert idx.dtype == torch.int32 and idx.shape == (30,) and [int(idx[k]) for k in (1, 6, 8, 29)] == [0, 1, 2, 3]
    assert int((idx >= 0).sum()) == 4
    # the checkpoint's radii win over the default table
    sd["additive_models.1.covalent_radii"] = torch.tensor([0.35, 0.70, 0.60, 1.40], dtype=torch.float64)
    back = mzbl.ZBLHip.from_state_dict(sd, "additive_models.1.")
    assert back.atomic_types == [1, 6, 8, 29] and back.covalent_radii == [0.35, 0.70, 0.60, 1.40]
    assert back.cutoff == pytest.approx(2.8)
    again = back.state_dict("additive_models.1.")
    assert all(torch.equal(again[k], sd[k]) for k in sd)
    # a model whose types are not in ascending order keeps its own order
    perm = mzbl.ZBLHip.from_state_dict(sd, "additive_models.1.", atomic_types=[8, 1])
    assert perm.covalent_radii == [0.60, 0.35]
    with pytest.raises(PetHipError, match="no ZBL buffers"):
        mzbl.ZBLHip.from_state_dict(sd, "additive_models.0.")


def test_refusals(caplog):
    with pytest.raises(ValueError, match="no covalent radius"):
        mzbl.ZBLHip([1, 92])
    assert mzbl.ZBLHip([1, 92], covalent_radii={92: 1.96}).cutoff == pytest.approx(3.92)
    with pytest.raises(ValueError, match="no radius"):
        mzbl.ZBLHip.from_state_dict(mzbl.ZBLHip([1, 6]).state_dict(), atomic_types=[1, 7])
    with pytest.raises(ValueError, match="only supports angstrom"):
        mzbl.ZBLHip([1], length_unit="bohr")
    with pytest.raises(ValueError, match="eV"):
        mzbl.ZBLHip([1], energy_unit="kcal/mol")
    with caplog.at_level(logging.WARNING):
        mzbl.ZBLHip([1, 6], covalent_radii={6: 0.2})
    assert "Covalent radius for element 6 is not available" in caplog.text
    z = mzbl.ZBLHip([1, 6])
    cpu = torch.zeros((2, 3))
    with pytest.raises(PetHipError, match="no CPU path"):
        z.remove_from_targets(None, cpu, torch.zeros((1, 3, 3)), energies=torch.zeros(1))
    with pytest.raises(PetHipError, match="no CPU path"):
        z.graph_for({"positions": cpu, "cells": torch.zeros((1, 3, 3)), "species": torch.tensor([1, 6]),
                     "system_indices": torch.tensor([0, 0])})


def test_hypers_zbl_is_honoured_or_refused():
    from metatrain_amd.pet import script
    from metatrain_amd.pet.hypers import default_hypers

    hy = default_hypers()
    assert script.make_zbl(hy, [1, 6, 8]) is None
    hy["zbl"] = True
    with pytest.raises(PetHipError, match="neighbour list of 4.06"):  # K: 2 x 2.03 A
        script.make_zbl(dict(hy, cutoff=3.0), [1, 19])
    with pytest.raises(PetHipError, match="adaptive"):
        script.make_zbl(dict(hy, num_neighbors_adaptive=16.0), [1, 6])
    table = script.make_zbl(hy, [1, 6, 8, 29])
    assert table.cutoff() == pytest.approx(2.64)
    # make_core returns the network alone, always: for a `zbl: true` model the caller has to say where the term goes
    with pytest.raises(PetHipError, match="make_core_and_zbl"):
        script.make_core(hy, [1, 6, 8, 29], {}, "energy")


def test_exported_models_with_zbl_script_and_pickle():
    import io

    from metatrain_amd import build
    from metatrain_amd.pet import script
    from metatrain_amd.pet.hypers import default_hypers
    from metatrain_amd.synthetic import synthetic_params

    if not os.path.exists(build.TORCH_LIB):
        build.build(verbose=False)
        build.build_torch_ops(verbose=False)
    types = [1, 6, 8, 29]
    hypers = dict(default_hypers(), zbl=True)
    params = synthetic_params(hypers, types, {"energy": 1}, 0, torch.float32)
    parts = script.make_core_and_zbl(hypers, types, params, "energy")
    assert parts.zbl.cutoff() == pytest.approx(2.64)
    off = script.make_core_and_zbl(dict(hypers, zbl=False), types, params, "energy")
    assert off.zbl is None and type(off.core) is type(parts.core)  # one return type, with ZBL or without
    assert type(script.make_core(hypers, types, params, "energy", zbl=False)) is type(parts.core)
    mod = torch.jit.script(script.ExportedEnergyModel(parts.core, 2.0, zbl=parts.zbl))
    buf = io.BytesIO()
    torch.jit.save(mod, buf)
    buf.seek(0)
    back = torch.jit.load(buf)
    assert back.pet.zbl.cutoff() == pytest.approx(2.64)  # the table is rebuilt from the pickled types and radii
    assert "atomic_energies_zbl" in str(back.pet.graph)
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU path"):
        back(z(2, 3), z(1, 3, 3), z(0, dtype=torch.int32), z(0, dtype=torch.int32), z(0, 3, dtype=torch.int32),
             torch.tensor([1, 6]), z(2, dtype=torch.int32))
    # a table for other types than the model's is refused before anything runs
    other = script.make_zbl(hypers, [1, 6], True)
    with pytest.raises(RuntimeError, match="different atomic types"):
        script.ExportedEnergyModel(parts.core, zbl=other)(
            z(2, 3), z(1, 3, 3), z(0, dtype=torch.int32), z(0, dtype=torch.int32), z(0, 3, dtype=torch.int32),
            torch.tensor([1, 6]), z(2, dtype=torch.int32))


def test_eager_llpr_wrapper_refuses_a_zbl_model():
    """``LLPRUncertainty.forward`` evaluates the network alone: for a ``zbl: true`` model it raises before anything runs."""
    import types

    from metatrain_amd.pet.llpr import LLPRUncertainty

    fake = types.SimpleNamespace(model=types.SimpleNamespace(hypers={"zbl": True}))
    with pytest.raises(PetHipError, match="ExportedLLPRModel"):
        LLPRUncertainty.forward(fake, None, {"energy": "system"})


def test_partitioned_boxes_refuse_a_zbl_model_they_cannot_serve():
    """The multi-GPU entry points add the ZBL term on the sub-system's own graph; where that graph does not hold every ZBL
    pair (a model cutoff below the ZBL cutoff, an adaptive cutoff) they raise before anything runs."""
    import types

    from metatrain_amd.pet import partition as pet_partition
    from metatrain_amd.soap_bpnn import partition as soap_partition

    pos, z, cell = torch.zeros((2, 3)), torch.tensor([1, 29]), torch.eye(3) * 20
    short = types.SimpleNamespace(hypers={"zbl": True, "cutoff": 2.0, "num_gnn_layers": 2}, atomic_types=[1, 29])
    adaptive = types.SimpleNamespace(hypers={"zbl": True, "cutoff": 4.5, "num_gnn_layers": 2, "num_neighbors_adaptive": 16.0},
                                     atomic_types=[1, 29])
    for fn, extra in ((pet_partition.energy_and_gradient, ()), (pet_partition.energy_and_gradient_exchange, (None,))):
        with pytest.raises(PetHipError, match="below the ZBL cutoff"):
            fn(short, pos, z, cell, (True, True, True), 2, 0, *extra)
        with pytest.raises(PetHipError, match="adaptive"):
            fn(adaptive, pos, z, cell, (True, True, True), 2, 0, *extra)
    soap = types.SimpleNamespace(cutoff=2.0, zbl=mzbl.ZBLHip([1, 29]), atomic_types=[1, 29])
    with pytest.raises(PetHipError, match="below the ZBL cutoff"):
        soap_partition.energy_and_gradient(soap, pos, z, cell, (True, True, True), 2, 0)
