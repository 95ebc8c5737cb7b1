"""Host side of training further targets (``TrainStep(extra_targets=...)``): the loss terms and their seeds against a
torch restatement of the reference's semantics -- per-atom averaging of per-structure targets unless the name is in
``per_structure_targets`` (``utils/per_atom.py``), ``process_non_conservative_stress`` (``backend.py``), one MSE over all
blocks of a target with NaN targets dropped (``utils/loss.py``), and the micro-batch shares."""
import torch

from metatrain_amd.pet.trainer import extra_target_count, extra_target_loss, process_non_conservative_stress


def _reference_stress(p, cells, sys):  # backend.py process_non_conservative_stress
    t = p.reshape(-1, 3, 3, p.shape[1] // 9)
    vol = torch.abs(torch.det(cells))
    vol[vol == 0.0] = torch.inf
    t = t / vol[sys].unsqueeze(1).unsqueeze(2).unsqueeze(3)
    return ((t + t.transpose(1, 2)) / 2.0).reshape(p.shape[0], -1)


def _batch():
    g = torch.Generator().manual_seed(5)
    sys = torch.tensor([0] * 5 + [1] * 3 + [2] * 4)
    cells = torch.rand((3, 3, 3), generator=g, dtype=torch.float64) + 3.0 * torch.eye(3, dtype=torch.float64)
    cells[2] = 0.0  # a non-periodic cluster: zero cell, infinite volume
    return g, sys, cells, torch.bincount(sys).double()


def test_non_conservative_stress_processing_matches_reference():
    g, sys, cells, _ = _batch()
    p = torch.randn((12, 18), generator=g, dtype=torch.float64)
    torch.testing.assert_close(process_non_conservative_stress(p, cells, sys), _reference_stress(p, cells, sys))
    assert torch.all(process_non_conservative_stress(p, cells, sys)[sys == 2] == 0)


def test_per_structure_target_averaging_and_nan_mask():
    g, sys, cells, n_atoms = _batch()
    pred = torch.randn((12, 2), generator=g, dtype=torch.float64, requires_grad=True)
    target = torch.randn((3, 2), generator=g, dtype=torch.float64)
    target[1, 0] = float("nan")
    spec = {"values": target, "per_atom": False}
    for name, per_structure in (("dipole", ()), ("dipole", ("dipole",))):
        loss = extra_target_loss(name, spec, {name: pred}, sys, n_atoms, cells, 0.5, per_structure)
        s = torch.zeros((3, 2), dtype=torch.float64).index_add(0, sys, pred)
        t = target
        if not per_structure:  # average_by_num_atoms: predictions AND targets (pet/trainer.py:431-435)
            s, t = s / n_atoms[:, None], t / n_atoms[:, None]
        m = ~torch.isnan(t)
        ref = 0.5 * ((s[m] - t[m]) ** 2).mean()
        torch.testing.assert_close(loss, ref)
        (ga,) = torch.autograd.grad(loss, pred)
        (gr,) = torch.autograd.grad(ref, pred)
        torch.testing.assert_close(ga, gr)


def test_stress_target_is_not_averaged_when_per_structure():
    g, sys, cells, n_atoms = _batch()
    pred = torch.randn((12, 9), generator=g, dtype=torch.float64)
    target = torch.randn((3, 3, 3, 1), generator=g, dtype=torch.float64)
    target[2] = float("nan")  # the cluster has no stress
    loss = extra_target_loss("non_conservative_stress", {"values": target, "per_atom": False}, {"non_conservative_stress": pred},
                             sys, n_atoms, cells, 2.0, ("non_conservative_stress",))
    s = torch.zeros((3, 9), dtype=torch.float64).index_add(0, sys, _reference_stress(pred, cells, sys)).reshape(-1)
    t = target.reshape(-1)
    m = ~torch.isnan(t)
    torch.testing.assert_close(loss, 2.0 * ((s[m] - t[m]) ** 2).mean())


def test_blocks_share_one_mean_and_micro_batch_shares_add_up():
    g, sys, cells, n_atoms = _batch()
    pa = torch.randn((12, 3), generator=g, dtype=torch.float64)
    pb = torch.randn((12, 6), generator=g, dtype=torch.float64)
    ta = torch.randn((12, 3), generator=g, dtype=torch.float64)
    tb = torch.randn((12, 3, 2), generator=g, dtype=torch.float64)
    tb[0, 1, 1] = float("nan")
    spec = {"values": {"a": ta, "b": tb}}
    loss = extra_target_loss("multi", spec, {"a": pa, "b": pb}, sys, n_atoms, cells, 1.0)
    d = torch.cat([(pa - ta).reshape(-1), (pb - tb.reshape(12, 6)).reshape(-1)])
    d = d[~torch.isnan(d)]
    torch.testing.assert_close(loss, (d * d).mean())
    assert extra_target_count("multi", spec) == 12 * 9 - 1
    # two micro-batches (atoms 0-7 and 8-11) with the whole step's denominator add up to the one-batch loss
    total = extra_target_count("multi", spec)
    parts = []
    for rows in (slice(0, 8), slice(8, 12)):
        sub = {"values": {"a": ta[rows], "b": tb[rows]}}
        s_sys = sys[rows] - sys[rows].min()
        parts.append(extra_target_loss("multi", sub, {"a": pa[rows], "b": pb[rows]}, s_sys, torch.bincount(s_sys).double(),
                                       None, 1.0, count=total))
    torch.testing.assert_close(parts[0] + parts[1], loss)


def test_per_property_scales_apply_to_predictions_only():
    g, sys, cells, n_atoms = _batch()
    pb = torch.randn((12, 6), generator=g, dtype=torch.float64)
    tb = torch.randn((12, 3, 2), generator=g, dtype=torch.float64)
    sc = torch.tensor([2.0, 0.5], dtype=torch.float64)
    loss = extra_target_loss("multi", {"values": {"b": tb}, "scales": {"b": sc}}, {"b": pb}, sys, n_atoms, cells, 1.0)
    ref = ((pb.reshape(12, 3, 2) * sc - tb) ** 2).mean()  # scaler.apply_scales(use_per_property_scales=True)
    torch.testing.assert_close(loss, ref)
