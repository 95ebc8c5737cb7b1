"""GPU tests of the ``loss`` hyper through the native ``TrainStep`` (default model unless said otherwise): MAE, Huber and
masked losses whose values and seeds come from ``csrc/loss.hip``, against torch's (double) backward through the fp64 CPU
oracle of the SAME loss built with torch's loss modules (``_loss_oracle.py``).

Bar: every parameter's gradient within 1e-5 relative (max|d| / max|ref| per tensor) of the oracle's, the bar and comparison
of ``test_gpu_train.py::test_force_loss_parameter_gradients_match_oracle_double_backward``.

Targets are the oracle's own fp64 predictions plus offsets of magnitude in [0.05, 3] that stay 0.05 away from the Huber
delta of 0.5, so every residual is at least 1e-3 (asserted on the oracle's residuals) from a kink of its loss: the fp32 pass's
predictions differ from the oracle's by at most 1e-5 and cannot move an entry across one.

On the parent commit ``TrainStep`` ignored the ``loss`` key and trained with MSE:
``test_huber_and_mae_parameter_gradients_match_oracle`` fails there."""
import os

import numpy as np
import pytest
import torch

import _loss_oracle as O
from oracle import pet as opet

from _memo import memo_oracle

pytestmark = pytest.mark.gpu

TOL = 1e-5
TYPES = [1, 6, 7, 8]
DELTA = 0.5
MARGIN = 1e-3
S64 = dict(d_pet=64, d_node=128, d_feedforward=128, d_head=64, num_heads=4)  # the size-generic pass (test_gpu_gen_train.py)
NCF = "non_conservative_forces"
# The further target's Huber delta and residuals (magnitudes in [0.5, 1.9] or [2.1, 6]) are of the size of its predictions
# (|p| up to 4, fp32 forward error about 1e-6 |p|): a head's bias gradient is the SIGNED sum of the seeds, which on the
# quadratic branch are the residuals themselves, so residuals far below |p| would put the prediction's fp32 rounding, not
# the loss, above the 1e-5 bar (with delta 0.5 and residuals from 0.05 the head gradients sit at 1.3e-5 .. 3.6e-5).
NCF_DELTA = 2.0
# oracle-side terms: (kind, delta, weight); product-side `loss` hypers saying the same
TERMS_A = {"energy": ("huber", DELTA, 1.0), "forces": ("mae", 1.0, 0.7)}
LOSS_A = {"energy": {"type": "huber", "delta": DELTA, "weight": 1.0, "gradients": {"positions": {"type": "mae", "weight": 0.7}}}}
TERMS_B = {"energy": ("mae", 1.0, 1.0), "forces": ("huber", DELTA, 0.7)}
LOSS_B = {"energy": {"type": "mae", "weight": 1.0, "gradients": {"positions": {"type": "huber", "delta": DELTA, "weight": 0.7}}}}


def _inputs(golden_dir, name):
    g = dict(np.load(os.path.join(golden_dir, name)))
    return {k[3:]: torch.tensor(v) for k, v in g.items() if k.startswith("in_")}


def _n_atoms(inp):
    s = inp["system_indices"].long()
    return torch.bincount(s, minlength=int(s.max()) + 1).double()


def _p64(params, grad):
    return {k: (v if k == "species_to_species_index" else v.double().clone().requires_grad_(grad)) for k, v in params.items()}


def _forward64(p64, hypers, inp, pos, with_ncf):
    s = inp["system_indices"].long()

    def run(target):
        return opet.pet_atomic_energies(p64, hypers, pos, inp["cells"].double(), inp["centers"], inp["neighbors"],
                                        inp["cell_shifts"], inp["species"], s, target)

    e = torch.zeros(int(s.max()) + 1, dtype=torch.float64).index_add(0, s, run("energy")[:, 0])
    return e, (run(NCF) if with_ncf else None)


@memo_oracle
def _oracle_predictions(params, hypers, inp, with_ncf):
    """The oracle's energies [S], dE/dR [N,3] and (optionally) non-conservative forces [N,3], fp64."""
    pos = inp["positions"].double().clone().requires_grad_(True)
    e, ncf = _forward64(_p64(params, False), hypers, inp, pos, with_ncf)
    (g,) = torch.autograd.grad(e.sum(), pos)
    return e.detach(), g, None if ncf is None else ncf.detach()


def _offsets(shape, seed, delta=DELTA, lo=0.05, hi=3.0, gap=0.05):
    """Signed offsets with magnitudes in [lo, delta - gap] or [delta + gap, hi] (by default [0.05, 0.45] or [0.55, 3]): both
    Huber branches, no kink within ``gap``."""
    gen = torch.Generator().manual_seed(seed)
    r = torch.rand(shape, generator=gen, dtype=torch.float64)
    small = torch.rand(shape, generator=gen) < 0.5
    mag = torch.where(small, lo + (delta - gap - lo) * r, delta + gap + (hi - delta - gap) * r)
    return mag * (torch.randint(2, shape, generator=gen) * 2.0 - 1.0)


def _targets(params, hypers, inp, with_ncf=False):
    e, g, ncf = _oracle_predictions(params, hypers, inp, with_ncf)
    n = _n_atoms(inp)
    off_e = _offsets(e.shape, 21)
    if e.numel() >= 2:
        off_e[0], off_e[1] = 0.3, -1.7   # one structure on each Huber branch
    t = {"energy": e - off_e * n, "forces": g - _offsets(g.shape, 22)}  # the energy residual is taken per atom
    if with_ncf:
        t["ncf"] = ncf - _offsets(ncf.shape, 23, NCF_DELTA, 0.5, 6.0, 0.1)
    return t


@memo_oracle
def _oracle(params, hypers, inp, terms, t_e, t_f, t_ncf=None, ncf_mask=None):
    """The loss of ``terms`` built with torch's loss modules in fp64, its parameter gradients (double backward when the
    forces are in it) and every term's residuals."""
    p64 = _p64(params, True)
    pos = inp["positions"].double().clone().requires_grad_(True)
    n = _n_atoms(inp)
    e, ncf = _forward64(p64, hypers, inp, pos, "ncf" in terms)
    kind, delta, weight = terms["energy"]
    pe, te = O.scaled(e, t_e.double(), 1.0 / n)
    loss = weight * O.compute_flattened([pe], [te], None, kind, "mean", delta)
    res = {"energy": (pe - te).detach()}
    if "forces" in terms:
        kind, delta, weight = terms["forces"]
        (g,) = torch.autograd.grad(e.sum(), pos, create_graph=True)
        loss = loss + weight * O.compute_flattened([g], [t_f.double()], None, kind, "mean", delta)
        res["energy_positions_gradients"] = (g - t_f.double()).detach()
    if "ncf" in terms:
        kind, delta, weight = terms["ncf"]
        loss = loss + weight * O.compute_flattened([ncf], [t_ncf.double()], None if ncf_mask is None else [ncf_mask], kind,
                                                   "mean", delta)
        r = (ncf - t_ncf.double()).detach()
        res[NCF] = torch.where(ncf_mask, r, torch.full_like(r, float("nan"))) if ncf_mask is not None else r
    keys = [k for k in p64 if k != "species_to_species_index"]
    grads = torch.autograd.grad(loss, [p64[k] for k in keys], allow_unused=True)
    return float(loss.detach()), {k: (torch.zeros_like(p64[k]) if g is None else g) for k, g in zip(keys, grads)}, res


def _assert_margins(res, terms):
    """No valid residual within MARGIN of a kink; a Huber term of more than one entry has both branches."""
    for key, name in (("energy", "energy"), ("forces", "energy_positions_gradients"), ("ncf", NCF)):
        if key not in terms:
            continue
        kind, delta, _ = terms[key]
        d = res[name].reshape(-1)
        d = d[~torch.isnan(d)].abs()
        if kind == "mae":
            assert float(d.min()) >= MARGIN, (key, float(d.min()))
        if kind == "huber":
            assert float((d - delta).abs().min()) >= MARGIN, (key, float((d - delta).abs().min()))
            if d.numel() > 1:
                assert bool((d < delta).any()) and bool((d > delta).any()), key


def _setup(golden_dir, case, hypers_extra=None, targets=None):
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    hypers = dict(opet.DEFAULT_HYPERS, **(hypers_extra or {}))
    params = opet.synthetic_params(hypers, TYPES, targets or {"energy": 1}, 0, torch.float32)
    inp = _inputs(golden_dir, case)
    model = rt.HipModel(hypers, TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    graph = rt.HipGraph(model, inp["positions"].float().to(dev), inp["cells"].float().to(dev), inp["centers"].to(dev),
                        inp["neighbors"].to(dev), inp["cell_shifts"].to(dev), inp["species"].to(dev),
                        inp["system_indices"].int().to(dev))
    return dev, hypers, params, inp, model, graph, rt.HipForward(model, graph, train=True)


def _train_step(model, loss=None, **hypers):
    from metatrain_amd.pet.trainer import TrainStep

    h = dict({"grad_clip_norm": 0.0, "learning_rate": 0.0}, **hypers)  # the parameters stay, the gradients can be read
    if loss is not None:
        h["loss"] = loss
    return TrainStep(model, h)


def _compare(got, ref, what, tol=TOL):
    assert set(got) == set(ref), set(got) ^ set(ref)
    worst = {}
    for k, r in ref.items():
        r = r.numpy()
        g = got[k].cpu().numpy().astype(np.float64)
        assert g.shape == r.shape, k
        scale = np.abs(r).max()
        err = np.abs(g - r).max()
        worst[k] = err / scale if scale > 1e-12 else err
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print(what, [(f"{v:.2e}", k) for k, v in top])
    bad = {k: v for k, v in worst.items() if not v < tol}
    assert not bad, f"{what}: parameter gradients off: {bad}"


def _args(inp, dev, graph, fw, t):
    return dict(graph=graph, fw=fw, n_atoms=_n_atoms(inp).float().to(dev), target_energies=t["energy"].float().to(dev),
                target_gradients=t["forces"].float().to(dev))


@pytest.mark.parametrize("swap", [False, True], ids=["huber_energy_mae_forces", "mae_energy_huber_forces"])
@pytest.mark.parametrize("case", ["batch_two_systems.npz", "pet_default_box64.npz"])
def test_huber_and_mae_parameter_gradients_match_oracle(golden_dir, case, swap):
    """Measured worst per-tensor error on the MI355X: 3.2e-6 / 3.7e-6 (two systems), 1.7e-6 / 1.8e-6 (64-atom box)."""
    dev, hypers, params, inp, model, graph, fw = _setup(golden_dir, case)
    terms, loss = (TERMS_B, LOSS_B) if swap else (TERMS_A, LOSS_A)
    t = _targets(params, hypers, inp)
    ref_loss, ref, res = _oracle(params, hypers, inp, terms, t["energy"], t["forces"])
    _assert_margins(res, terms)
    out = _train_step(model, loss)(**_args(inp, dev, graph, fw, t))
    print("loss", float(out["loss"]), ref_loss)
    assert abs(float(out["loss"]) - ref_loss) <= TOL * abs(ref_loss)
    _compare(model.grads(), ref, f"{case} swap={swap}")


@pytest.mark.parametrize("what", ["energy_forces_strain", "further_targets"])
def test_mse_on_the_new_path_equals_the_legacy_step(golden_dir, what):
    """``loss: "mse"`` runs every term through the kernel; the torch functions of the step without a ``loss`` key compute
    the same loss on the same batch: energy + forces + strain gradients (the virial's fixed-order per-structure sum against
    ``index_add_``), and energy + non-conservative forces (per atom) + non-conservative stress (per structure: its
    post-processing and sum stay in torch's autograd, the residual is averaged by the atom count)."""
    NCS = "non_conservative_stress"
    extras = what == "further_targets"
    dev, hypers, params, inp, model, graph, fw = _setup(golden_dir, "batch_two_systems.npz",
                                                        targets={"energy": 1, NCF: 3, NCS: 9} if extras else None)
    t = _targets(params, hypers, inp)
    args = _args(inp, dev, graph, fw, t)
    gen = torch.Generator().manual_seed(17)
    n, n_sys = inp["positions"].shape[0], int(inp["system_indices"].max()) + 1
    if extras:
        del args["target_gradients"]
        ncs = torch.randn((n_sys, 3, 3, 1), generator=gen) * 1e-3
        ncs[-1, 0, 1, 0] = float("nan")
        args.update(cells=inp["cells"].float().to(dev),
                    extra_targets={NCF: {"values": (torch.randn((n, 3), generator=gen) * 0.1).to(dev)},
                                   NCS: {"values": ncs.to(dev), "per_atom": False}})
        keys = {"energy", NCF, NCS}
    else:
        args.update(target_strain_gradients=torch.randn((n_sys, 3, 3), generator=gen).to(dev),
                    positions=inp["positions"].float().to(dev), cells=inp["cells"].float().to(dev))
        keys = {"energy", "energy_positions_gradients", "energy_strain_gradients"}
    legacy = _train_step(model)(**args)
    assert "terms" not in legacy
    g_legacy = {k: v.clone() for k, v in model.grads().items()}
    new = _train_step(model, "mse")(**args)
    assert set(new["terms"]) == keys
    print("loss", float(new["loss"]), float(legacy["loss"]))
    assert abs(float(new["loss"]) - float(legacy["loss"])) <= 1e-6 * abs(float(legacy["loss"]))
    assert torch.equal(new["energies"], legacy["energies"])
    _compare(model.grads(), {k: v.cpu().double() for k, v in g_legacy.items()}, f"mse, {what}: new path against legacy")


def test_nan_labels_are_dropped(golden_dir):
    """Five force components and one energy without a label: the gradients are the oracle's with those entries dropped
    (``utils/loss.py:203-207``)."""
    dev, hypers, params, inp, model, graph, fw = _setup(golden_dir, "batch_two_systems.npz")
    t = {k: v.clone() for k, v in _targets(params, hypers, inp).items()}
    t["energy"][1] = float("nan")
    for i, c in ((0, 0), (3, 2), (7, 1), (8, 1), (t["forces"].shape[0] - 1, 2)):
        t["forces"][i, c] = float("nan")
    ref_loss, ref, res = _oracle(params, hypers, inp, TERMS_A, t["energy"], t["forces"])
    _assert_margins(res, TERMS_A)
    out = _train_step(model, LOSS_A)(**_args(inp, dev, graph, fw, t))
    assert abs(float(out["loss"]) - ref_loss) <= TOL * abs(ref_loss)
    _compare(model.grads(), ref, "NaN labels")
    from metatrain_amd.loss import read_stats

    assert read_stats(out["terms"]["energy"])["count"] == 1
    assert read_stats(out["terms"]["energy_positions_gradients"])["count"] == t["forces"].numel() - 5


class _ReadBacks:
    """Counts the host read-backs of device tensors inside a ``with`` block."""

    NAMES = ("item", "__int__", "__float__", "__bool__", "__index__", "cpu", "tolist", "numpy")

    def __enter__(self):
        self.count, self._saved = 0, {}
        for name in self.NAMES:
            orig = getattr(torch.Tensor, name)
            self._saved[name] = torch.Tensor.__dict__.get(name)  # None: inherited, the patch is deleted again

            def wrapped(t, *a, _orig=orig, **kw):
                if t.device.type == "cuda":
                    self.count += 1
                return _orig(t, *a, **kw)

            setattr(torch.Tensor, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, orig in self._saved.items():
            if orig is None:
                delattr(torch.Tensor, name)
            else:
                setattr(torch.Tensor, name, orig)


def test_masked_huber_on_a_further_target_and_no_read_back(golden_dir):
    """Energy (MSE) + non-conservative forces (``masked_huber`` with a mask and NaN labels) against the oracle (measured
    worst 8.7e-6, on the further target's last layer); no host read-back in the step; the mask is required."""
    dev, hypers, params, inp, model, graph, fw = _setup(golden_dir, "batch_two_systems.npz", targets={"energy": 1, NCF: 3})
    t = {k: v.clone() for k, v in _targets(params, hypers, inp, with_ncf=True).items()}
    gen = torch.Generator().manual_seed(5)
    mask = torch.rand(t["ncf"].shape, generator=gen) < 0.7
    t["ncf"][2, 1] = float("nan")
    t["ncf"][5] = float("nan")
    terms = {"energy": ("mse", 1.0, 1.0), "ncf": ("huber", NCF_DELTA, 0.6)}
    loss = {"energy": "mse", NCF: {"type": "masked_huber", "delta": NCF_DELTA, "weight": 0.6}}
    ref_loss, ref, res = _oracle(params, hypers, inp, terms, t["energy"], None, t["ncf"], mask)
    _assert_margins(res, terms)
    args = dict(graph=graph, fw=fw, n_atoms=_n_atoms(inp).float().to(dev), target_energies=t["energy"].float().to(dev),
                extra_targets={NCF: {"values": t["ncf"].float().to(dev), "mask": mask.to(dev)}})
    step = _train_step(model, loss)
    step(**args)  # (first use: the terms' workspaces are allocated)
    with _ReadBacks() as rb:
        out = step(**args)
    assert rb.count == 0, f"{rb.count} host read-backs in a step on the `loss` path"
    assert abs(float(out["loss"]) - ref_loss) <= TOL * abs(ref_loss)
    _compare(model.grads(), ref, "masked_huber NC forces")
    # a masked type without its mask is refused with the reference's message
    with pytest.raises(ValueError, match=f"Expected extra_data to contain TensorMap under '{NCF}_mask'"):
        step(**dict(args, extra_targets={NCF: {"values": args["extra_targets"][NCF]["values"]}}))


def _single_system_batches(rt, model, inp, args, dev):
    """The batch as one micro-batch per structure (the construction of test_gpu_multitarget_train.py)."""
    sys = inp["system_indices"].long()
    assert bool((sys[1:] >= sys[:-1]).all())
    batches = []
    for si in range(int(sys.max()) + 1):
        atoms = torch.nonzero(sys == si).squeeze(1)
        a0 = int(atoms[0])
        keep = sys[inp["centers"].long()] == si
        g_s = rt.HipGraph(model, inp["positions"][atoms].float().to(dev), inp["cells"][si:si + 1].float().to(dev),
                          (inp["centers"][keep] - a0).to(dev), (inp["neighbors"][keep] - a0).to(dev),
                          inp["cell_shifts"][keep].to(dev), inp["species"][atoms].to(dev),
                          torch.zeros(len(atoms), dtype=torch.int32, device=dev))
        batches.append(dict(graph=g_s, fw=rt.HipForward(model, g_s, train=True), n_atoms=args["n_atoms"][si:si + 1],
                            target_energies=args["target_energies"][si:si + 1],
                            target_gradients=args["target_gradients"][atoms.to(dev)]))
    return batches


def test_microbatched_begin_end_terms_and_bitwise_repeat(golden_dir):
    from metatrain_amd import runtime as rt
    from metatrain_amd.loss import LossMetrics

    dev, hypers, params, inp, model, graph, fw = _setup(golden_dir, "batch_two_systems.npz")
    t = _targets(params, hypers, inp)
    args = _args(inp, dev, graph, fw, t)
    step = _train_step(model, LOSS_A)
    out = step(**args)
    one = {k: v.clone() for k, v in model.grads().items()}
    # two identical steps from the same state (learning rate 0) are bitwise equal: gradients, loss and statistics
    again = step(**args)
    for k, v in model.grads().items():
        assert torch.equal(v, one[k]), k
    assert torch.equal(again["loss"].view(torch.int64), out["loss"].view(torch.int64))
    for k in out["terms"]:
        assert torch.equal(again["terms"][k].view(torch.int64), out["terms"][k].view(torch.int64)), k
    # begin / end is __call__
    step.begin(**args)
    split = step.end()
    assert set(split) == set(out) and torch.equal(split["loss"], out["loss"])
    for k, v in model.grads().items():
        assert torch.equal(v, one[k]), k
    # "terms" -> LossMetrics: the RMSE / MAE of the oracle's residuals
    _, _, res = _oracle(params, hypers, inp, TERMS_A, t["energy"], t["forces"])
    metrics = LossMetrics()
    metrics.update(out["terms"])
    metrics.update(split["terms"])   # a second batch with the same residuals: the means stay
    got = metrics.finalize()
    assert set(got) == {f"{k} {m}" for k in res for m in ("RMSE", "MAE")}
    for k, d in res.items():
        print(k, got[f"{k} RMSE"], float((d * d).mean().sqrt()), got[f"{k} MAE"], float(d.abs().mean()))
        assert got[f"{k} RMSE"] == pytest.approx(float((d * d).mean().sqrt()), rel=1e-6)
        assert got[f"{k} MAE"] == pytest.approx(float(d.abs().mean()), rel=1e-6)
    assert set(LossMetrics().finalize()) == set()
    per_atom = metrics.finalize(not_per_atom=["positions_gradients"])
    assert set(per_atom) == {"energy RMSE (per atom)", "energy MAE (per atom)", "energy_positions_gradients RMSE",
                             "energy_positions_gradients MAE"}
    # two micro-batches of one structure each: counted first, then the passes; the means are the whole step's
    micro = step.microbatched(_single_system_batches(rt, model, inp, args, dev))
    assert abs(float(micro["loss"]) - float(out["loss"])) <= 1e-5 * abs(float(out["loss"]))
    assert torch.allclose(micro["energies"], out["energies"], rtol=1e-6, atol=1e-6)
    for k, v in model.grads().items():
        ref = one[k].cpu().numpy()
        np.testing.assert_allclose(v.cpu().numpy(), ref, rtol=0, atol=1e-5 * max(float(np.abs(ref).max()), 1e-12), err_msg=k)
    # the expanded spec round-trips through state_dict
    state = step.state_dict()
    other = _train_step(model)
    assert other.loss_spec is None
    other.load_state_dict(state)
    assert other.loss_spec == step.loss_spec and other.loss_spec["energy"]["gradients"]["positions"] == {
        "type": "mae", "weight": 0.7, "reduction": "mean"}


def test_size_generic_pass_huber_energy_mae_forces(golden_dir):
    """The ``d_pet = 64`` model of ``test_gpu_gen_train.py`` (``s64``) at that file's bar; measured worst 9.5e-6."""
    dev, hypers, params, inp, model, graph, fw = _setup(golden_dir, "batch_two_systems.npz", hypers_extra=S64)
    t = _targets(params, hypers, inp)
    ref_loss, ref, res = _oracle(params, hypers, inp, TERMS_A, t["energy"], t["forces"])
    _assert_margins(res, TERMS_A)
    out = _train_step(model, LOSS_A)(**_args(inp, dev, graph, fw, t))
    assert abs(float(out["loss"]) - ref_loss) <= TOL * abs(ref_loss)
    _compare(model.grads(), ref, "s64 huber energy + mae forces")
