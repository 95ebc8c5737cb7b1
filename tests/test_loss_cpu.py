"""CPU tests of the loss path: the shorthand rules of the ``loss`` hyper (``utils/omegaconf.py:432-724``) against
hand-written expected dicts, every refusal by its message, and the host-side argument checks of ``pet_loss_count`` /
``pet_loss_pointwise`` (every call is refused before a launch: no GPU call is made)."""
import ctypes
import os

import pytest
import torch

import _loss_oracle as O
from metatrain_amd import _lib
from metatrain_amd import loss as L
from metatrain_amd import runtime as rt
from oracle import pet as opet

MSE = {"type": "mse", "weight": 1.0, "reduction": "mean"}
TARGETS = {"energy": {"is_energy": True, "gradients": ["positions", "strain"]}, "mtt::dos": {}}


def test_global_type_sets_every_target_and_gradient():
    """Form 1, ``loss: <type>``."""
    mae = dict(MSE, type="mae")
    assert L.expand_loss_hypers("mae", TARGETS) == {
        "energy": dict(mae, gradients={"positions": dict(mae), "strain": dict(mae)}),
        "mtt::dos": dict(mae, gradients={}),
    }
    huber = dict(MSE, type="huber", delta=1.0)  # the default delta of a Huber loss
    assert L.expand_loss_hypers("huber", {"energy": {"gradients": ["positions"]}}) == {
        "energy": dict(huber, gradients={"positions": dict(huber)})}


def test_per_target_types_leave_gradients_at_their_defaults():
    """Form 2, ``loss: {target: type}``; a target that is not named keeps every default; None is all defaults."""
    assert L.expand_loss_hypers({"energy": "mae"}, TARGETS) == {
        "energy": dict(MSE, type="mae", gradients={"positions": dict(MSE), "strain": dict(MSE)}),
        "mtt::dos": dict(MSE, gradients={}),
    }
    assert L.expand_loss_hypers(None, ["energy"]) == {"energy": dict(MSE, gradients={})}


def test_energy_shorthands_expand_to_gradients():
    """Form 3: ``forces`` -> ``gradients.positions``, ``stress`` / ``virial`` -> ``gradients.strain``, a type or a dict."""
    got = L.expand_loss_hypers({"energy": {"type": "huber", "delta": 0.5, "forces": "mae",
                                           "stress": {"type": "huber", "weight": 0.1, "reduction": "sum"}}}, TARGETS)
    assert got["energy"] == {
        "type": "huber", "delta": 0.5, "weight": 1.0, "reduction": "mean",
        "gradients": {"positions": dict(MSE, type="mae"),
                      "strain": {"type": "huber", "weight": 0.1, "reduction": "sum", "delta": 1.0}}}
    got = L.expand_loss_hypers({"energy": {"virial": "mae"}}, TARGETS)
    assert got["energy"] == dict(MSE, gradients={"positions": dict(MSE), "strain": dict(MSE, type="mae")})


def test_explicit_gradients_and_idempotence():
    """Form 4, ``gradients: {positions: type or dict}``; the expanded dict expands to itself (a checkpoint's round trip)."""
    loss = {"energy": {"type": "mse", "weight": 2.0, "gradients": {"positions": {"type": "masked_huber", "delta": 0.25, "weight": 0.7},
                                                                    "strain": "mae"}},
            "mtt::dos": {"type": "masked_mae", "reduction": "sum"}}
    got = L.expand_loss_hypers(loss, TARGETS)
    assert got == {
        "energy": {"type": "mse", "weight": 2.0, "reduction": "mean",
                   "gradients": {"positions": {"type": "masked_huber", "delta": 0.25, "weight": 0.7, "reduction": "mean"},
                                 "strain": dict(MSE, type="mae")}},
        "mtt::dos": {"type": "masked_mae", "weight": 1.0, "reduction": "sum", "gradients": {}},
    }
    assert L.expand_loss_hypers(got, TARGETS) == got


def test_refusals_name_what_they_refuse():
    with pytest.raises(ValueError, match=r"Invalid top-level loss entry 'forces'\. Allowed keys are: \['energy', 'mtt::dos'\] or a "
                                         "single string"):
        L.expand_loss_hypers({"forces": "mae"}, TARGETS)
    with pytest.raises(ValueError, match=r"Unknown loss 'rmse'\. Valid types: mse, mae, huber, masked_mse, masked_mae, masked_huber, "
                                         "pointwise, masked_pointwise, shift_agnostic_mse"):
        L.expand_loss_hypers("rmse", TARGETS)
    with pytest.raises(ValueError, match="Unknown loss 'l2'"):
        L.expand_loss_hypers({"energy": {"forces": "l2"}}, TARGETS)
    for kind in ("shift_agnostic_mse", "gaussian_nll_ensemble", "gaussian_crps_ensemble", "empirical_crps_ensemble", "pointwise",
                 "masked_pointwise"):
        with pytest.raises(NotImplementedError, match=f"'{kind}' is not served"):
            L.expand_loss_hypers({"mtt::dos": kind}, TARGETS)
    with pytest.raises(NotImplementedError, match="'reduction: none' is not served"):
        L.expand_loss_hypers({"energy": {"reduction": "none"}}, TARGETS)
    with pytest.raises(ValueError, match="unknown reduction 'median'"):
        L.expand_loss_hypers({"energy": {"forces": {"reduction": "median"}}}, TARGETS)
    with pytest.raises(ValueError, match="only allowed for energy-like targets, but target 'mtt::dos' is not energy-like"):
        L.expand_loss_hypers({"mtt::dos": {"forces": "mae"}}, TARGETS)
    with pytest.raises(ValueError, match="Both 'stress' and 'virial' provided for target 'energy'"):
        L.expand_loss_hypers({"energy": {"stress": "mae", "virial": "mae"}}, TARGETS)
    for delta in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="Huber delta must be positive"):
            L.expand_loss_hypers({"energy": {"type": "huber", "delta": delta}}, TARGETS)


def test_loss_beside_loss_weights_is_refused_and_cpu_tensors_raise():
    from metatrain_amd.pet.trainer import TrainStep

    model = rt.HipModel(dict(opet.DEFAULT_HYPERS), [1, 6, 7, 8])
    with pytest.raises(ValueError, match="both `loss` and `loss_weights`"):
        TrainStep(model, {"loss": "huber", "loss_weights": {"energy": 1.0, "forces": 10.0}})
    with pytest.raises(ValueError, match="load the model"):  # the targets of a `loss` hyper are the model's
        TrainStep(model, {"loss": "huber"})
    assert TrainStep(model, {"loss_weights": {"energy": 1.0, "forces": 10.0}}).loss_spec is None  # the step as it was
    term = L.PointwiseLoss()
    with pytest.raises(_lib.PetHipError, match="no CPU path"):
        term.count(torch.zeros(3, 2), torch.zeros(3, 2))
    with pytest.raises(_lib.PetHipError, match="no CPU path"):
        term(torch.zeros(3, 2), torch.zeros(3, 2), kind="mse")
    with pytest.raises(_lib.PetHipError, match="no CPU path"):
        L.LossMetrics().update({"energy": torch.zeros(4, dtype=torch.float64)})


def test_oracle_follows_the_table_at_the_kinks():
    """Host only: at d = 0 (MAE) and d = +-delta (Huber) torch gives what the header's table states."""
    d = torch.tensor([0.0, 0.25, -0.25, 1.0, -1.0, 2.0, -0.125])
    z = torch.zeros_like(d)
    assert O.term(d, z, "mae", "sum")["seed"].tolist() == [0.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0]
    assert O.term(d, z, "huber", "sum", delta=0.25)["seed"].tolist() == [0.0, 0.25, -0.25, 0.25, -0.25, 0.25, -0.125]
    assert O.term(d, z, "huber", "sum", delta=1.0)["seed"].tolist() == [0.0, 0.25, -0.25, 1.0, -1.0, 1.0, -0.125]
    assert float(O.term(d, z, "huber", "sum", delta=1.0)["loss"]) == 0.5 * (2 * 0.0625 + 2 * 1.0 + 0.015625) + (2.0 - 0.5)
    assert float(O.term(d, torch.full_like(d, float("nan")), "mse")["loss"]) == 0.0


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from metatrain_amd import build

        build.build(verbose=False)
    return _lib.load()


def test_c_entry_points_check_their_arguments(lib):
    """Every call below has one defect and is refused with PET_ERR_ARGUMENT on the host, before any launch; the non-null
    pointers are never followed."""
    buf = (ctypes.c_double * 8)()
    a = ctypes.c_void_p(ctypes.addressof(buf))
    b = ctypes.c_void_p(ctypes.addressof(buf) + 32)
    null = ctypes.c_void_p(0)
    E = _lib.PET_ERR_ARGUMENT
    assert lib.pet_loss_workspace_bytes(-1, 1) == -1 and lib.pet_loss_workspace_bytes(4, 0) == -1
    assert lib.pet_loss_workspace_bytes(0, 3) == 8
    assert lib.pet_loss_workspace_bytes(256, 3) == 8 * 4 + 8 and lib.pet_loss_workspace_bytes(257, 9) == 8 * 4 * 2 + 8
    assert lib.pet_loss_count(a, null, 4, 3, null, null) == E       # no count
    assert lib.pet_loss_count(null, null, 4, 3, a, null) == E       # no target
    assert lib.pet_loss_count(a, null, -1, 3, b, null) == E         # negative rows
    assert lib.pet_loss_count(a, null, 4, 0, b, null) == E          # no values per row
    assert b"null" in lib.pet_last_error() or b"row" in lib.pet_last_error()

    def pointwise(pred=a, target=a, cs=null, n_cs=0, rows=4, width=3, kind=0, delta=1.0, weight=1.0, reduction=0, count=a,
                  seed=b, ws=a, ws_bytes=1 << 20):
        return lib.pet_loss_pointwise(pred, target, null, null, cs, n_cs, rows, width, kind, delta, weight, reduction, count, seed,
                                      null, null, ws, ws_bytes, null)

    assert pointwise(pred=null) == E and pointwise(target=null) == E
    assert pointwise(rows=-1) == E and pointwise(width=0) == E
    assert pointwise(kind=3) == E and pointwise(kind=-1) == E
    assert b"unknown loss kind" in lib.pet_last_error()
    assert pointwise(reduction=2) == E
    assert b"unknown reduction" in lib.pet_last_error()
    assert pointwise(kind=2, delta=0.0) == E and pointwise(kind=2, delta=-0.5) == E and pointwise(kind=2, delta=float("nan")) == E
    assert pointwise(count=null) == E                               # a mean without its denominator
    assert pointwise(seed=a) == E                                   # seed aliases pred
    assert b"seed == pred" in lib.pet_last_error()
    assert pointwise(cs=a, n_cs=2) == E and pointwise(cs=a, n_cs=0) == E and pointwise(cs=null, n_cs=3) == E
    assert pointwise(ws=null) == E and pointwise(ws_bytes=8 * 4) == E and pointwise(rows=257, ws_bytes=8 * 4 + 8) == E
    assert b"workspace too small" in lib.pet_last_error()
    # an empty term is served (nothing to launch): the accumulators stay as they are
    assert pointwise(rows=0, pred=null, target=null, seed=null) == 0
    assert lib.pet_loss_count(null, null, 0, 3, a, null) == 0
