"""Long-range (Ewald) features, the parts that need no GPU: the fp64 oracle of the definition (``tests/_ewald_oracle.py``)
against two facts about Ewald sums, the product's host k-set against the oracle's, every refusal with its message, the
reference's state-dict keys and the hypers defaults."""
import math
import types

import pytest
import torch

import _ewald_oracle as eo
from oracle import pet as opet


def _lr_hypers(**extra):
    h = dict(opet.DEFAULT_HYPERS)
    h["long_range"] = dict({"enable": True, "use_ewald": True}, **extra)
    return h


@pytest.mark.parametrize("smearing", [0.3, 0.5])
def test_oracle_gives_the_nacl_madelung_constant(smearing):
    """No-exclusion mode (real-space erfc term + k-space + self): -1.7475646, independent of the smearing."""
    assert abs(eo.madelung_nacl(smearing) - (-1.7475646)) < 1e-6


def test_oracle_converges_in_the_kset():
    """43-atom triclinic box, sigma = 1.4, against |k| <= 8: the truncation at kspace_resolution 1.33 / 2.0 / 2.66 leaves
    5e-11 / 1.2e-5 / 1.4e-3 of the largest value (the factor exp(-(sigma 2 pi / lambda)^2 / 2) = 3e-10 / 6e-5 / 4e-3)."""
    torch.manual_seed(0)
    cell = torch.eye(3, dtype=torch.float64) * 9.5 + 0.3 * torch.randn(3, 3, dtype=torch.float64)
    pos = torch.rand(43, 3, dtype=torch.float64) @ cell
    q = torch.randn(43, 5, dtype=torch.float64)
    ref = eo.kspace_self_background(pos, cell, q, 1.4, None, kmax=8.0)
    rel = {}
    for lam in (1.33, 2.0, 2.66):
        v = eo.kspace_self_background(pos, cell, q, 1.4, lam)
        rel[lam] = float((v - ref).abs().max() / ref.abs().max())
    print(rel)
    assert rel[1.33] < 1e-9 and 1e-7 < rel[2.0] < 1e-4 and 1e-5 < rel[2.66] < 1e-2, rel


@pytest.mark.parametrize("kind", ["cubic", "triclinic"])
def test_product_kvectors_equal_the_oracle_set(kind):
    from metatrain_amd import long_range as lr

    g = torch.Generator().manual_seed(2)
    cell = torch.eye(3, dtype=torch.float64) * 9.5
    if kind == "triclinic":
        cell = cell + 0.3 * torch.randn(3, 3, generator=g, dtype=torch.float64)
    got = lr.kvectors(cell, 1.33)
    ref = eo.kvectors(cell, 1.33)
    assert got.shape == ref.shape and got.shape[0] > 500 and got.shape[0] % 2 == 0

    def canon(k):  # rows sorted by their integer indices
        n = torch.round(k @ cell.T / (2.0 * math.pi)).long()
        order = sorted(range(len(n)), key=lambda r: tuple(n[r].tolist()))
        return k[order], n[order]

    (gk, gn), (rk, rn) = canon(got), canon(ref)
    assert torch.equal(gn, rn)
    assert float((gk - rk).abs().max()) < 1e-12


def test_hypers_defaults():
    from metatrain_amd.pet import hypers as H

    assert H.DEFAULT_LONG_RANGE_HYPERS == {"enable": False, "use_ewald": False, "smearing": 1.4, "kspace_resolution": 1.33,
                                           "interpolation_nodes": 5}
    # a dictionary with only `enable` keeps working and is completed with the reference's defaults
    full = H.long_range_hypers({"long_range": {"enable": True}})
    assert full == dict(H.DEFAULT_LONG_RANGE_HYPERS, enable=True)
    assert H.default_hypers()["long_range"]["enable"] is False


def test_state_dict_keys_and_shapes():
    from metatrain_amd import long_range as lr

    h = _lr_hypers()
    f = lr.LongRangeFeaturizerHip(h)
    sd = f.state_dict()
    assert tuple(sd) == lr.REFERENCE_KEYS
    d = h["d_node"]
    for k, v in sd.items():
        assert tuple(v.shape) == ((d, d) if k.endswith("weight") else (d,)) and v.dtype == torch.float32
    ref = eo.featurizer_params(d, 0)
    assert set(ref) == set(sd)
    g = lr.LongRangeFeaturizerHip.from_state_dict(h, ref)
    assert all(torch.equal(g.state_dict()[k], ref[k]) for k in ref)
    bad = dict(ref)
    del bad["long_range_featurizer.out_projection.2.bias"]
    with pytest.raises(lr.PetHipError, match="out_projection.2.bias"):
        lr.LongRangeFeaturizerHip.from_state_dict(h, bad)


def test_refusals_name_what_they_refuse():
    from metatrain_amd import long_range as lr
    from metatrain_amd import runtime as rt
    from metatrain_amd.pet import backend, llpr, partition, script, trainer

    h = _lr_hypers()
    model = types.SimpleNamespace(hypers=h)
    with pytest.raises(lr.PetHipError, match=r"training \(TrainStep\) of a long-range model"):
        trainer.TrainStep(model)
    with pytest.raises(lr.PetHipError, match="Hessian-vector product of a long-range model"):
        rt.hessian_vector_product(model, None, torch.zeros(1, 3))
    with pytest.raises(lr.PetHipError, match="LLPR of a long-range model"):
        llpr.LLPRUncertainty(model, {}, {})
    with pytest.raises(lr.PetHipError, match="box partition of a long-range model"):
        partition.energy_and_gradient(model, None, None, None, [True] * 3, 1, 0)
    with pytest.raises(lr.PetHipError, match="per-layer exchange of a long-range model"):
        partition.energy_and_gradient_exchange(model, None, None, None, [True] * 3, 1, 0, None)
    with pytest.raises(lr.PetHipError, match="scripted model .ExportedEnergyModel"):
        script.make_core(h, eo.TYPES, {}, "energy")
    with pytest.raises(lr.PetHipError, match="three-node PETBackend mirror"):
        backend.PETBackend(h, eo.TYPES)
    with pytest.raises(lr.PetHipError, match="auxiliary outputs .*feature"):
        lr.energy_and_gradient(model, None, None, None, outputs=("feature",))
    with pytest.raises(lr.PetHipError, match="mixed pbc"):
        lr.EwaldHip().plan(torch.eye(3)[None] * 10.0, [[True, True, False]], [0, 4])
    with pytest.raises(lr.PetHipError, match="num_neighbors_adaptive"):
        lr.LongRangeFeaturizerHip(dict(h, num_neighbors_adaptive=16.0))
    p3m = _lr_hypers(use_ewald=False)
    with pytest.raises(lr.PetHipError, match="p3m_as_ewald=True"):
        lr.LongRangeFeaturizerHip(p3m)
    lr.LongRangeFeaturizerHip(p3m, p3m_as_ewald=True)  # the explicit opt-in loads
    with pytest.raises(lr.PetHipError, match="long_range.enable is false"):
        lr.LongRangeFeaturizerHip(dict(opet.DEFAULT_HYPERS))
    # models without long_range.enable are untouched by all of this
    rt.refuse_long_range(dict(opet.DEFAULT_HYPERS), "anything")
    # CPU tensors raise like the rest of the product
    with pytest.raises(lr.PetHipError, match="no CPU path"):
        lr.EwaldHip().potential(None, torch.zeros(2, 3), torch.zeros(2, 4))


def test_unconverged_kset_warns_once(caplog):
    from metatrain_amd import long_range as lr

    lr._warned_kset = False
    with caplog.at_level("WARNING"):
        lr.EwaldHip(1.4, 1.33)
        assert not caplog.records  # 3e-10: converged
        lr.EwaldHip(1.4, 2.66)
        lr.EwaldHip(1.4, 2.66)
    assert len([r for r in caplog.records if "shape of the k-set" in r.getMessage().lower()]) == 1


def test_a_mesh_operator_does_not_warn_about_the_kset(caplog):
    """``P3MHip`` is built through ``EwaldHip.__init__`` and walks no k-set: it neither warns nor uses up the one warning."""
    from metatrain_amd import long_range as lr

    lr._warned_kset = False
    with caplog.at_level("WARNING"):
        op = lr.P3MHip(1.4, 2.66, 4.5, 3)
    assert not caplog.records and lr._warned_kset is False
    assert (op.smearing, op.kspace_resolution, op.cutoff, op.interpolation_nodes, op.n_systems) == (1.4, 2.66, 4.5, 3, -1)
