"""CPU tests of the long-range training oracle (``tests/_long_range_train_oracle.py``) and of the refusals of the long-range
training step that need no GPU. The oracle's premises are checked in fp64 on the first three QM9 frames: the tangents against a
central difference of the energies, the symmetry of the Hessian and its translation invariance per system."""
import types

import pytest
import torch

import _ewald_oracle as eo
import _long_range_train_oracle as lo
from oracle import pet as opet


def _energies(tag, which, shift):
    hypers, params = lo.model_case(tag)
    b = lo.batch_of(which)
    p = {k: (v if k == "species_to_species_index" else v.double()) for k, v in params.items()}
    with torch.no_grad():
        return lo.atomic_energies(p, hypers, b, b["positions"].double() + shift, b["cells"].double())


@pytest.mark.parametrize("tag", ["odd33", "residual"])
def test_tangents_are_the_directional_derivative_of_the_energies(tag):
    """``e'_i`` (and so ``sum e' = <u, dE/dR>``) against ``(e(R + h u) - e(R - h u)) / 2h``: O(h^2) apart."""
    ref, _ = lo.reference(tag, "qm9")
    _, u, _ = lo.seeds("qm9")
    h = 1e-4
    fd = (_energies(tag, "qm9", h * u) - _energies(tag, "qm9", -h * u)) / (2.0 * h)
    scale = float(ref["tangent"].abs().max())
    assert scale > 1e-4
    assert float((fd - ref["tangent"]).abs().max()) <= 1e-5 * scale   # third derivatives times h^2 / 6 = 2e-9
    assert abs(float(fd.sum()) - float((u * ref["grad"]).sum())) <= 1e-5 * scale * len(fd)
    assert abs(float(ref["tangent"].sum()) - float((u * ref["grad"]).sum())) <= 1e-12 * scale * len(fd)


@pytest.mark.parametrize("tag", ["odd33", "residual"])
def test_hessian_is_symmetric_and_translation_invariant(tag):
    """``<v, H u> = <u, H v>`` and ``sum_i (H u)_i = 0`` per system, in fp64."""
    ru, _ = lo.reference(tag, "qm9")
    rv, _ = lo.reference(tag, "qm9", direction="v")
    _, u, v = lo.seeds("qm9")
    a, b = float((v * ru["hvp"]).sum()), float((u * rv["hvp"]).sum())
    assert abs(a - b) <= 1e-10 * max(abs(a), abs(b))
    batch = lo.batch_of("qm9")
    scale = float(ru["hvp"].abs().max())
    for s in range(len(batch["first_atom"]) - 1):
        rows = slice(batch["first_atom"][s], batch["first_atom"][s + 1])
        assert float(ru["hvp"][rows].sum(0).abs().max()) <= 1e-12 * scale * (rows.stop - rows.start)


def test_three_atoms_without_an_edge_still_interact():
    """Three open atoms about 6 A apart: no edge, and forces, a Hessian and featuriser gradients from K(d) = (1 - f) / d."""
    b = lo.batch_of("three")
    assert len(b["centers"]) == 0
    ref, f32 = lo.reference("odd33", "three")
    assert float(ref["grad"].abs().max()) > 1e-4 and float(ref["hvp"].abs().max()) > 1e-4
    assert all(float(ref["grads"][lo.PRE + k].abs().max()) > 0.0 for k in ("charges_map.weight", "out_projection.0.weight"))


def _lr_hypers(**extra):
    h = dict(opet.DEFAULT_HYPERS, **extra)
    h["long_range"] = {"enable": True, "use_ewald": True, "smearing": 1.4, "kspace_resolution": 1.33, "interpolation_nodes": 5}
    return h


def test_new_refusals_name_what_they_refuse():
    from metatrain_amd import long_range as lr

    h = _lr_hypers()
    model = types.SimpleNamespace(hypers=h, _ckeys={})
    feat = lr.LongRangeFeaturizerHip(h)
    with pytest.raises(lr.PetHipError, match="P3M featuriser"):
        lr.LongRangeTrainStep(model, lr.LongRangeFeaturizerHip(h, method="p3m"))
    with pytest.raises(lr.PetHipError, match="P3M featuriser"):
        lr.hessian_vector_product(model, lr.LongRangeFeaturizerHip(h, method="p3m"), None, None, torch.zeros(1, 3))
    with pytest.raises(lr.PetHipError, match="num_neighbors_adaptive"):
        lr.LongRangeTrainStep(types.SimpleNamespace(hypers=dict(h, num_neighbors_adaptive=8.0)), feat)
    with pytest.raises(lr.PetHipError, match="no long_range.enable"):
        lr.LongRangeTrainStep(types.SimpleNamespace(hypers=dict(opet.DEFAULT_HYPERS)), feat)
    # a model loaded without the six tensors: by key
    with pytest.raises(lr.PetHipError, match="long_range_featurizer.charges_map.weight"):
        lr.LongRangeTrainStep(model, feat)
    with pytest.raises(lr.PetHipError, match="long_range_featurizer.out_projection.2.bias"):
        feat.bind(types.SimpleNamespace(_ckeys={k: None for k in lr.REFERENCE_KEYS[:-1]}))
    # what the long-range forward refuses of a training step's calls
    fw = lr.LongRangeForward(types.SimpleNamespace(hypers=h, lib=None), feat, None, None)
    with pytest.raises(lr.PetHipError, match="u_cell"):
        fw.backward_train2(None, None, None, u_cell=torch.zeros(1, 3, 3))
    with pytest.raises(lr.PetHipError, match="seed_features"):
        fw.backward_train2(None, None, None, seed_features=(None, None))
    with pytest.raises(lr.PetHipError, match="seed_features"):
        fw.backward_train(None, seed_features=(None, None))
    with pytest.raises(lr.PetHipError, match="target_strain_gradients"):
        lr.LongRangeTrainStep._refuse(fw, torch.zeros(1, 3, 3), None)
    with pytest.raises(lr.PetHipError, match="extra_targets"):
        lr.LongRangeTrainStep._refuse(fw, None, {"non_conservative_forces": {}})
    with pytest.raises(lr.PetHipError, match="needs a LongRangeForward"):
        lr.LongRangeTrainStep._refuse(object(), None, None)
    # a CPU direction raises like the rest of the product
    with pytest.raises(lr.PetHipError, match="no CPU path"):
        lr.hessian_vector_product(model, feat, None, None, torch.zeros(1, 3))


def test_old_refusals_still_raise():
    from metatrain_amd import long_range as lr
    from metatrain_amd import runtime as rt
    from metatrain_amd.pet import trainer

    model = types.SimpleNamespace(hypers=_lr_hypers())
    with pytest.raises(lr.PetHipError, match=r"training \(TrainStep\) of a long-range model"):
        trainer.TrainStep(model)
    with pytest.raises(lr.PetHipError, match="Hessian-vector product of a long-range model"):
        rt.hessian_vector_product(model, None, torch.zeros(1, 3))
    assert eo.TYPES == [1, 6, 7, 8]
