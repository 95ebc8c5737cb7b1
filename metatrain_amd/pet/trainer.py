"""Host side of the PET training step, mirroring the reference's loop body
``pet/trainer.py:417-472``:

    optimizer.zero_grad() -> evaluate_model(is_training=True) -> average_by_num_atoms -> loss
    -> loss.backward() -> clip_grad_norm_ -> optimizer.step() -> lr_scheduler.step()

Everything that touches activations or weights runs in libpet_hip (forward, reverse pass, weight
gradients, clip + Adam, re-pack); torch only does the per-structure loss arithmetic on ``[S]`` /
``[N,3]`` tensors and the RCCL all-reduce of the flat gradient bucket. With a ``loss`` hyper (MAE, Huber, masked losses,
sum reduction: ``metatrain_amd/loss.py``) the loss terms and their seeds come from ``csrc/loss.hip`` instead.
"""
import math
from typing import Dict, Optional

import torch

from .. import distributed as D
from ..loss import STATE_WORDS, PointwiseLoss, expand_loss_hypers
from ..runtime import HipForward, HipGraph, HipModel, refuse_long_range

DEFAULT_TRAINER_HYPERS = {  # pet/documentation.py TrainerHypers defaults that the step depends on
    "learning_rate": 1e-4,
    "weight_decay": None,
    "grad_clip_norm": 1.0,
    "num_epochs": 1000,
    "warmup_fraction": 0.01,
    "loss_weights": {"energy": 1.0, "forces": 1.0},
}


def lr_lambda(step: int, total_steps: int, warmup_fraction: float, min_lr_ratio: float = 0.0) -> float:
    """Linear warm-up then cosine decay (``pet/trainer.py:56-86``, ``get_scheduler``)."""
    warmup_steps = int(warmup_fraction * total_steps)
    if step < warmup_steps:
        return float(step) / float(max(1, warmup_steps))
    progress = (step - warmup_steps) / float(max(1, total_steps - warmup_steps))
    return min_lr_ratio + (1.0 - min_lr_ratio) * 0.5 * (1.0 + math.cos(math.pi * progress))


def energy_loss_and_seeds(energies: torch.Tensor, targets: torch.Tensor, n_atoms: torch.Tensor,
                          system_of_atom: torch.Tensor, weight: float = 1.0):
    """MSE (mean over structures) of per-atom-averaged energies (``utils/per_atom.py``,
    ``utils/loss.py`` "mse"/"mean") and dL/dE_i for every atom i (the seed of the reverse pass)."""
    diff = (energies - targets) / n_atoms
    loss = weight * (diff * diff).mean()
    d_energy = weight * 2.0 * diff / (n_atoms * energies.numel())  # dL/dE_s
    return loss, d_energy[system_of_atom]


def force_loss_and_seeds(grad_positions: torch.Tensor, target_gradients: torch.Tensor, weight: float = 1.0):
    """MSE (mean over the N*3 components) on the position gradient dE/dR = -forces, which the per-atom
    averaging leaves untouched (``utils/per_atom.py``: samples carry "atom"), and u = dL/d(dE/dR)."""
    diff = grad_positions - target_gradients
    loss = weight * (diff * diff).mean()
    return loss, weight * 2.0 * diff / diff.numel()


def strain_loss_and_seeds(positions: torch.Tensor, cells: torch.Tensor, system_of_atom: torch.Tensor,
                          grad_positions: torch.Tensor, grad_cells: torch.Tensor, target_strain_gradients: torch.Tensor,
                          weight: float = 1.0):
    """The strain derivative of ``utils/evaluate_model.py:305-321`` (``positions @ strain``, ``cell @ strain``, gradient at
    strain = 1) from dE/dR and dE/dcell: ``dE/deps[s] = R_s^T dE/dR_s + cell_s^T dE/dcell_s`` ``[S,3,3]``; MSE (mean over
    the 9 S components) against the targets and the seeds ``u = dL/d(dE/dR)`` ``[N,3]``, ``u_cell = dL/d(dE/dcell)``
    ``[S,3,3]`` of the second-order pass. ``[S]``-sized torch arithmetic."""
    n_sys = cells.shape[0]
    virial = torch.zeros((n_sys, 3, 3), dtype=grad_positions.dtype, device=grad_positions.device)
    virial.index_add_(0, system_of_atom, positions[:, :, None] * grad_positions[:, None, :])
    virial = virial + cells.transpose(1, 2) @ grad_cells
    diff = virial - target_strain_gradients
    loss = weight * (diff * diff).mean()
    g = weight * 2.0 * diff / diff.numel()                       # dL/d(dE/deps)
    u = (positions[:, None, :] @ g[system_of_atom]).squeeze(1)    # d(dE/deps_ab)/d(gR_ib) = R_ia
    return loss, u, cells @ g


def process_non_conservative_stress(pred: torch.Tensor, cells: torch.Tensor, system_of_atom: torch.Tensor) -> torch.Tensor:
    """``backend.py`` ``process_non_conservative_stress`` on per-atom predictions ``[N, 9 P]``: divided by the volume of
    the atom's cell (a zero volume -- a non-periodic system -- counts as infinite) and symmetrised."""
    n, p = pred.shape[0], pred.shape[1] // 9
    t = pred.reshape(n, 3, 3, p)
    c = cells.to(pred.dtype)
    vol = torch.abs((c[:, 0] * torch.linalg.cross(c[:, 1], c[:, 2])).sum(-1))  # |det|, elementwise (fixed order)
    vol = torch.where(vol == 0.0, torch.full_like(vol, float("inf")), vol)
    t = t / vol[system_of_atom][:, None, None, None]
    return ((t + t.transpose(1, 2)) / 2.0).reshape(n, 9 * p)


def _extra_blocks(name: str, spec: dict) -> Dict[str, torch.Tensor]:
    values = spec["values"]
    return values if isinstance(values, dict) else {name: values}


def extra_target_count(name: str, spec: dict) -> int:
    """The number of non-NaN target entries of one extra target (the denominator of its MSE)."""
    return int(sum(int((~torch.isnan(t)).sum()) for t in _extra_blocks(name, spec).values()))


class _SumOverAtoms(torch.autograd.Function):
    """Per-structure sums of per-atom columns in a fixed order (``pet_sum_over_atoms``; index_add's float atomics make
    the step's seeds vary run to run)."""

    @staticmethod
    def forward(ctx, p, fw, system_of_atom):
        ctx.save_for_backward(system_of_atom)
        return torch.stack([fw.sum_over_atoms(p[:, j].contiguous()) for j in range(p.shape[1])], dim=1)

    @staticmethod
    def backward(ctx, g):
        (s,) = ctx.saved_tensors
        return g[s], None, None


def extra_target_loss(name: str, spec: dict, preds: Dict[str, torch.Tensor], system_of_atom: torch.Tensor,
                      n_atoms: torch.Tensor, cells: Optional[torch.Tensor], weight: float, per_structure_targets=(),
                      count: Optional[int] = None, structure_sum=None) -> torch.Tensor:
    """The reference's loss term of one further target (``pet/trainer.py:430-451``, ``utils/loss.py:144-217``, "mse" /
    "mean"): every block's per-atom predictions ``preds[block]`` ``[N, P]`` -> (``non_conservative_stress``:
    :func:`process_non_conservative_stress`) -> per-structure targets (``spec["per_atom"] = False``): summed over the atoms
    -> ``average_by_num_atoms`` (``utils/per_atom.py``): per-structure predictions AND targets divided by n_atoms unless
    the name is in ``per_structure_targets`` -> per-property scales (``spec["scales"] = {block: [n_properties]}``,
    ``scaler.apply_scales(use_per_property_scales=True)``: predictions only) -> one MSE over the concatenation of all
    blocks' flattened values, NaN targets dropped. ``count``: the denominator (the whole step's non-NaN entries when
    micro-batched); ``structure_sum(p)``: the per-structure sum ``[S, P]`` (default: index_add)."""
    per_atom = spec.get("per_atom", True)
    scales = spec.get("scales") or {}
    diffs = []
    for b, target in _extra_blocks(name, spec).items():
        p = preds[b]
        if name == "non_conservative_stress":
            if cells is None:
                raise ValueError("a non_conservative_stress target needs `cells`")
            p = process_non_conservative_stress(p, cells, system_of_atom)
        t = target.to(device=p.device, dtype=p.dtype)
        if not per_atom:
            if structure_sum is not None:
                p = structure_sum(p)
            else:
                p = torch.zeros((n_atoms.numel(), p.shape[1]), dtype=p.dtype, device=p.device).index_add(0, system_of_atom, p)
            t = t.reshape(p.shape)
            if name not in per_structure_targets:
                n = n_atoms.to(device=p.device, dtype=p.dtype)[:, None]
                p, t = p / n, t / n
        t = t.reshape(p.shape)
        if b in scales:  # the innermost axis of a block's values is its properties
            sc = torch.as_tensor(scales[b]).to(device=p.device, dtype=p.dtype).reshape(-1)
            p = (p.reshape(p.shape[0], -1, sc.numel()) * sc).reshape(p.shape)
        valid = ~torch.isnan(t)
        diffs.append((p - torch.nan_to_num(t))[valid])
    d = torch.cat(diffs)
    n = d.numel() if count is None else count
    return weight * (d * d).sum() / max(n, 1)


class TrainStep:
    """One optimizer step on one batch (a ``HipGraph`` of several structures).

    A ``zbl: true`` model is trained on ``ZBLHip.remove_from_targets(...)`` of its energy, gradient and strain-gradient
    targets (``metatrain_amd/zbl.py``), as the reference's ``get_remove_additive_transform`` does: the ZBL term has no
    parameters, is not part of the loss graph and is added back at evaluation (``ExportedEnergyModel(..., zbl=...)``)."""

    _serves_long_range = False  # a subclass that evaluates the long-range featuriser (long_range.LongRangeTrainStep) sets it

    def __init__(self, model: HipModel, hypers: Optional[dict] = None, steps_per_epoch: int = 1):
        if not self._serves_long_range:
            refuse_long_range(getattr(model, "hypers", None) or {}, "training (TrainStep)")
        self.model = model
        self.hypers = dict(DEFAULT_TRAINER_HYPERS)
        self.hypers.update(hypers or {})
        self._terms: Dict[str, PointwiseLoss] = {}
        self._set_loss_spec()
        self.total_steps = int(self.hypers["num_epochs"]) * int(steps_per_epoch)
        self.step_index = 0  # optimizer steps taken so far (LambdaLR's last_epoch)
        self.comm_events: Optional[list] = None  # a list here collects (start, end) events around every gradient all-reduce

    def _set_loss_spec(self) -> None:
        """The ``loss`` hyper (``pet/documentation.py:368``), expanded and validated; None without one: the MSE / mean
        functions of this module with ``loss_weights``. The targets are the model's: the fused target may carry position
        and strain gradients, every further target with an uploaded head is a plain one."""
        self.loss_spec = None
        if self.hypers.get("loss") is None:
            return
        if self.hypers["loss_weights"] != DEFAULT_TRAINER_HYPERS["loss_weights"]:
            raise ValueError("both `loss` and `loss_weights` were given: with a `loss` hyper the weights are its `weight` entries")
        targets = {}
        if self.model.target is not None:
            targets[self.model.target] = {"is_energy": True, "gradients": ["positions", "strain"]}
        for t, _ in (self.model.head_keys() if hasattr(self.model, "_ckeys") else {}).values():  # (nothing before load())
            targets.setdefault(t, {"is_energy": False})
        if not targets:
            raise ValueError("a `loss` hyper names the model's targets: load the model before building its TrainStep")
        self.loss_spec = expand_loss_hypers(self.hypers["loss"], targets)
        self.hypers["loss"] = self.loss_spec  # (expanding an expanded spec changes nothing: state_dict round-trips it)

    def state_dict(self) -> Dict[str, object]:
        """What the reference's trainer checkpoint keeps of the optimizer and scheduler (``pet/trainer.py:697-717``:
        ``optimizer_state_dict``, ``scheduler_state_dict``, epoch): Adam's moments, the step counter that drives both
        the bias correction and the LambdaLR schedule, and the hypers the schedule was built from."""
        return {"step_index": self.step_index, "total_steps": self.total_steps, "hypers": dict(self.hypers),
                "optimizer": {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in self.model.optimizer_state().items()}}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        self.step_index = int(state["step_index"])
        self.total_steps = int(state["total_steps"])
        self.hypers.update(state["hypers"])
        self._set_loss_spec()
        self.model.load_optimizer_state(state["optimizer"])

    def current_lr(self) -> float:
        h = self.hypers
        return h["learning_rate"] * lr_lambda(self.step_index, self.total_steps, h["warmup_fraction"])

    def __call__(self, graph: HipGraph, fw: HipForward, target_energies: Optional[torch.Tensor],
                 n_atoms: torch.Tensor, target_gradients: Optional[torch.Tensor] = None,
                 target_strain_gradients: Optional[torch.Tensor] = None, positions: Optional[torch.Tensor] = None,
                 cells: Optional[torch.Tensor] = None, extra_targets: Optional[Dict[str, dict]] = None
                 ) -> Dict[str, torch.Tensor]:
        """``target_gradients`` [N,3] = dE/dR targets (-forces); None trains on energies only.
        ``target_strain_gradients`` [S,3,3] = dE/dstrain targets (stress x volume; needs ``positions`` and ``cells``,
        weight ``loss_weights["strain"]``, default 1).
        ``extra_targets``: further targets whose heads were uploaded under their own names (non-conservative forces and
        stress, several blocks or properties), ``{name: {"values": [N|S, ...] or {block: [N|S, ...]}, "per_atom": bool
        (default True), "weight": float (default loss_weights[name]), "scales": optional {block: per-property scales}}}``; NaN target entries are dropped, a
        ``non_conservative_stress`` target needs ``cells``. ``target_energies`` may then be None (a model loaded with
        ``target=None``). One forward and one backbone reverse sweep serve all targets.

        With a ``loss`` entry in the hypers (the reference's ``loss`` hyper, :func:`metatrain_amd.loss.expand_loss_hypers`)
        every term is formed on the device by ``csrc/loss.hip``: MSE, MAE or Huber, mean or sum, NaN targets dropped in
        every term, weights from the ``loss`` entry (``loss_weights`` and a spec's ``"weight"`` are refused beside it), a
        ``masked_*`` type with ``spec["mask"]`` (the values' shape, or ``{block: ...}``; non-zero = counted). The result
        then also holds ``"terms"``: per term a statistics block for :class:`metatrain_amd.loss.LossMetrics`. Without a
        ``loss`` entry the step is the MSE / mean step it always was."""
        self.model.zero_grad()
        if self.loss_spec is not None:
            out = self._native([dict(graph=graph, fw=fw, target_energies=target_energies, n_atoms=n_atoms,
                                     target_gradients=target_gradients, target_strain_gradients=target_strain_gradients,
                                     positions=positions, cells=cells, extra_targets=extra_targets)])
            out["grad_norm"] = self._finish(self._trained(target_energies is not None, [extra_targets]))
            return out
        loss, energies = self._accumulate(graph, fw, target_energies, n_atoms, target_gradients, target_strain_gradients,
                                          positions, cells, 1.0, 1.0, 1.0, extra_targets)
        norm = self._finish(self._trained(target_energies is not None, [extra_targets]))
        return {"loss": loss, "grad_norm": norm, "energies": energies}

    def microbatched(self, batches) -> Dict[str, torch.Tensor]:
        """ONE optimizer step over several micro-batches (gradient accumulation): the training workspace holds every
        tangent of a batch (100 KB per edge), so a rank's share of a large batch -- BASELINE
        ``configs[3]``: 64 x 10 000-atom boxes per GPU -- is walked a few boxes at a time. Each element of ``batches`` is a
        dict with the arguments of :meth:`__call__` (``graph, fw, target_energies, n_atoms`` and optionally
        ``target_gradients, target_strain_gradients, positions, cells``); the losses are the full batch's means
        (``utils/loss.py`` "mean" reduction over ALL structures / components), so the result equals the one-batch step up
        to fp32 summation order."""
        batches = list(batches)
        if self.loss_spec is not None:  # every micro-batch is counted on the device first: the means are the whole step's
            self.model.zero_grad()
            out = self._native(batches)
            out["grad_norm"] = self._finish(self._trained(any(b.get("target_energies") is not None for b in batches),
                                                          [b.get("extra_targets") for b in batches]))
            return out
        s_tot = float(sum(int(b["n_atoms"].numel()) for b in batches))
        n_tot = float(sum(int(b["graph"].n_nodes) for b in batches))
        counts = {}  # extra targets: the whole step's non-NaN entries (their MSE's denominator)
        for b in batches:
            for name, spec in (b.get("extra_targets") or {}).items():
                counts[name] = counts.get(name, 0) + extra_target_count(name, spec)
        self.model.zero_grad()
        loss, energies = None, []
        for b in batches:
            s_b, n_b = float(b["n_atoms"].numel()), float(b["graph"].n_nodes)
            l_b, e_b = self._accumulate(b["graph"], b["fw"], b.get("target_energies"), b["n_atoms"],
                                        b.get("target_gradients"), b.get("target_strain_gradients"), b.get("positions"),
                                        b.get("cells"), s_b / s_tot, n_b / n_tot, s_b / s_tot, b.get("extra_targets"), counts)
            loss = l_b if loss is None else loss + l_b
            energies.append(e_b)
        norm = self._finish(self._trained(any(b.get("target_energies") is not None for b in batches),
                                          [b.get("extra_targets") for b in batches]))
        return {"loss": loss, "grad_norm": norm, "energies": None if energies[0] is None else torch.cat(energies)}

    def begin(self, graph: HipGraph, fw: HipForward, target_energies: Optional[torch.Tensor], n_atoms: torch.Tensor,
              target_gradients: Optional[torch.Tensor] = None, target_strain_gradients: Optional[torch.Tensor] = None,
              positions: Optional[torch.Tensor] = None, cells: Optional[torch.Tensor] = None,
              extra_targets: Optional[Dict[str, dict]] = None) -> None:
        """First half of :meth:`__call__`: the three sweeps of the batch, then the gradient all-reduce is STARTED
        (``distributed.all_reduce_gradients_async``: RCCL runs it on its own stream). Whatever the caller launches before
        :meth:`end` -- the next batch's neighbour lists and graph build, as the reference's DataLoader workers do beside
        ``loss.backward()`` (``pet/trainer.py:417-472``) -- overlaps the collective."""
        self.model.zero_grad()
        if self.loss_spec is not None:
            self._pending = self._native([dict(graph=graph, fw=fw, target_energies=target_energies, n_atoms=n_atoms,
                                               target_gradients=target_gradients,
                                               target_strain_gradients=target_strain_gradients, positions=positions,
                                               cells=cells, extra_targets=extra_targets)])
        else:
            self._pending = self._accumulate(graph, fw, target_energies, n_atoms, target_gradients, target_strain_gradients,
                                             positions, cells, 1.0, 1.0, 1.0, extra_targets)
        self._pending_trained = self._trained(target_energies is not None, [extra_targets])
        self._reduce = D.all_reduce_gradients_async(self.model, self.comm_events)

    def end(self) -> Dict[str, torch.Tensor]:
        """Second half: wait for the reduced gradients (a stream dependency under RCCL), clip + AdamW + schedule."""
        pending, self._pending = self._pending, None
        norm = self._finish(self._pending_trained)
        if isinstance(pending, dict):  # the `loss` path
            return dict(pending, grad_norm=norm)
        loss, energies = pending
        return {"loss": loss, "grad_norm": norm, "energies": energies}

    def _trained(self, with_energy: bool, extra_list) -> Dict[str, Optional[set]]:
        """target -> the blocks this step's loss reads (None: every block)."""
        out: Dict[str, Optional[set]] = {}
        if with_energy and self.model.target is not None:
            out[self.model.target] = None
        for extra in extra_list:
            for name, spec in (extra or {}).items():
                out.setdefault(name, set()).update(_extra_blocks(name, spec))
        return out

    def _finish(self, trained: Optional[Dict[str, Optional[set]]] = None) -> torch.Tensor:
        m = self.model
        reduce = getattr(self, "_reduce", None) or D.all_reduce_gradients_async(m, self.comm_events)
        self._reduce = None
        reduce.wait()
        # heads and last layers of targets (blocks) absent from this step's loss have no .grad in the reference's loop,
        # so torch's optimizer leaves them and their moments alone (weight decay included)
        idle = []
        if trained is not None:
            for key, (t, b) in m.head_keys().items():
                if t not in trained or (b is not None and trained[t] is not None and b not in trained[t]):
                    idle.append(key)
        with m.frozen_for_step(idle):
            norm = m.adam_step(self.current_lr(), self.step_index + 1, weight_decay=self.hypers["weight_decay"],
                               max_grad_norm=self.hypers["grad_clip_norm"] or 0.0)
        self.step_index += 1
        return norm

    def _extra(self, graph, fw, n_atoms, cells, extra_targets, extra_counts):
        """Predictions of the further targets from the training forward's features, their loss terms, and the summed
        adjoints of the heads' inputs (``train_predict_backward``, which also adds the heads' parameter gradients).

        With several readout layers (the residual featuriser) a block's prediction is the sum over the layers of that
        layer's head output (``backend.py:468-481``); post-processing and the loss act on the sum, so one
        dL/d(prediction) seeds every layer, and the seeds come back as ``(node list, edge list)``, one pair per layer."""
        w = self.hypers["loss_weights"]
        sys = graph.system_of_atom().long()
        n_layers = self.model.num_readout_layers()
        loss, seed_features = None, None
        for name, spec in extra_targets.items():
            preds = {}
            for b in _extra_blocks(name, spec):
                p = fw.train_predict(name, b)
                for layer in range(1, n_layers):  # fixed order
                    p = p + fw.train_predict(name, b, readout_layer=layer)
                preds[b] = p.requires_grad_(True)
            weight = float(spec.get("weight", w.get(name, 1.0)))
            count = None if extra_counts is None else extra_counts[name]
            loss_t = extra_target_loss(name, spec, preds, sys, n_atoms, cells, weight,
                                       self.hypers.get("per_structure_targets", ()), count,
                                       lambda p: _SumOverAtoms.apply(p, fw, sys))
            grads = torch.autograd.grad(loss_t, list(preds.values()))
            for layer in range(n_layers):
                seed_features = fw.train_predict_backward(name, dict(zip(preds, grads)), readout_layer=layer,
                                                          seed_features=seed_features)
            loss = loss_t.detach() if loss is None else loss + loss_t.detach()
        return loss, seed_features

    def _accumulate(self, graph, fw, target_energies, n_atoms, target_gradients, target_strain_gradients, positions, cells,
                    share_e: float, share_f: float, share_s: float, extra_targets=None, extra_counts=None):
        """Forward + reverse passes of one (micro-)batch, parameter gradients ADDED to the model's slots; ``share_*`` =
        this batch's fraction of the structures / force components / strain components of the whole step.
        ``extra_targets``: further targets (see :meth:`__call__`), served by the same forward and the same one backbone
        reverse sweep."""
        w = self.hypers["loss_weights"]
        if fw.graph is not graph:  # micro-batches may share one workspace allocation
            fw.rebind(graph)
        if target_energies is None:
            if target_gradients is not None or target_strain_gradients is not None:
                raise ValueError("force / strain-gradient targets need the energy target")
            if not extra_targets:
                raise ValueError("no target to train")
            fw.forward(want_atomic=False)
            loss, seeds, energies = None, None, None
        else:
            atomic = fw.forward()
            energies = fw.sum_over_atoms(atomic)
            loss, seeds = energy_loss_and_seeds(energies, target_energies, n_atoms, graph.system_of_atom(),
                                                w["energy"] * share_e)
        seed_features = None
        if extra_targets:
            loss_x, seed_features = self._extra(graph, fw, n_atoms, cells, extra_targets, extra_counts)
            loss = loss_x if loss is None else loss + loss_x
        if target_gradients is None and target_strain_gradients is None:
            fw.backward_train(seeds, seed_features=seed_features)
        else:
            ones = torch.ones_like(atomic)
            # evaluate_model: autograd.grad(E.sum(), [R, strain], create_graph=True)
            grad_positions, grad_cells = fw.backward(ones, want_cell_grad=True)
            u = torch.zeros_like(grad_positions)
            u_cell = None
            if target_gradients is not None:
                loss_f, u = force_loss_and_seeds(grad_positions, target_gradients, w["forces"] * share_f)
                loss = loss + loss_f
            if target_strain_gradients is not None:
                if positions is None or cells is None:
                    raise ValueError("a strain-gradient (stress) target needs `positions` and `cells`")
                loss_s, u_s, u_cell = strain_loss_and_seeds(
                    positions.to(torch.float32), cells.to(torch.float32), graph.system_of_atom().long(), grad_positions,
                    grad_cells, target_strain_gradients, w.get("strain", 1.0) * share_s)
                loss = loss + loss_s
                u = u + u_s
            fw.backward_train2(ones, seeds, u, u_cell=u_cell, seed_features=seed_features)
        return loss, energies

    # ---- the `loss` hyper: every term on csrc/loss.hip (metatrain_amd/loss.py) ---------------------------------------------

    def _term_arrays(self, b):
        """(term key, loss node, target, mask) of every target array of one (micro-)batch, in the order the step runs
        them; the keys are the reference's metric keys (``utils/metrics.py:149-156``)."""
        spec, name = self.loss_spec, self.model.target
        if b.get("target_energies") is not None:
            yield name, spec[name], b["target_energies"], None
            if b.get("target_gradients") is not None:
                yield f"{name}_positions_gradients", spec[name]["gradients"]["positions"], b["target_gradients"], None
            if b.get("target_strain_gradients") is not None:
                yield f"{name}_strain_gradients", spec[name]["gradients"]["strain"], b["target_strain_gradients"], None
        for x, xs in (b.get("extra_targets") or {}).items():
            if x not in spec:
                raise ValueError(f"no loss for the target '{x}': the model has no head of that name (loss entries: {sorted(spec)})")
            if "weight" in xs:
                raise ValueError(f"target '{x}': with a `loss` hyper the weight is the `weight` entry of its loss")
            masks = xs.get("mask")
            if spec[x]["type"].startswith("masked_"):
                if masks is None:
                    raise ValueError(f"Expected extra_data to contain TensorMap under '{x}_mask'")  # utils/loss.py:272-275
                masks = masks if isinstance(masks, dict) else {x: masks}
            else:
                masks = {}  # (an unmasked type does not look at a mask, as in the reference)
            for blk, t in _extra_blocks(x, xs).items():
                yield x, spec[x], t, masks.get(blk)

    def _run_term(self, key, node, pred, target, total, **kw):
        kind = node["type"][len("masked_"):] if node["type"].startswith("masked_") else node["type"]
        return self._terms[key](pred, target, kind=kind, delta=node.get("delta", 1.0), weight=node["weight"],
                                reduction=node["reduction"], loss_out=total, **kw)[1]

    def _native(self, batches) -> Dict[str, object]:
        """The sweeps of one optimizer step over ``batches`` (dicts of :meth:`__call__`'s arguments) with every loss term
        formed by :class:`metatrain_amd.loss.PointwiseLoss`: the valid entries of every term are counted over ALL batches
        first, on the device, so a mean is over the step's valid entries (``utils/loss.py:203-217``) without a read-back.
        Returns ``loss``, ``energies`` and ``terms = {key: statistics block}`` (fp64 ``[4]`` device tensors, zeroed per
        step: what ``LossMetrics.update`` takes)."""
        dev = batches[0]["n_atoms"].device
        arrays = [list(self._term_arrays(b)) for b in batches]
        keys = list(dict.fromkeys(k for a in arrays for k, _, _, _ in a))
        state = torch.zeros((len(keys), STATE_WORDS), dtype=torch.int64, device=dev)
        for i, k in enumerate(keys):
            self._terms.setdefault(k, PointwiseLoss()).bind(state[i])
        for a in arrays:
            for k, _, t, m in a:
                self._terms[k].count(t, t, m)
        total = torch.zeros((), dtype=torch.float64, device=dev)
        energies = [self._accumulate_native(total=total, **b) for b in batches]
        return {"loss": total, "energies": None if energies[0] is None else (energies[0] if len(energies) == 1 else torch.cat(energies)),
                "terms": {k: self._terms[k].stats() for k in keys}}

    def _extra_native(self, graph, fw, inv_n, cells, extra_targets, total):
        """:meth:`_extra` with the seeds from the kernel: dL/d(prediction) goes straight to ``train_predict_backward``;
        torch's autograd is used only for what stands between a head's output and the loss's prediction (the
        non-conservative stress's post-processing, the per-structure sum)."""
        sys = graph.system_of_atom().long()
        n_layers = self.model.num_readout_layers()
        seed_features = None
        for name, xs in extra_targets.items():
            node = self.loss_spec[name]
            per_atom = xs.get("per_atom", True)
            scales = xs.get("scales") or {}
            masks = xs.get("mask") if node["type"].startswith("masked_") else None
            masks = masks if isinstance(masks, dict) else {name: masks}
            grads = {}
            for b, target in _extra_blocks(name, xs).items():
                p = fw.train_predict(name, b)
                for layer in range(1, n_layers):  # fixed order
                    p = p + fw.train_predict(name, b, readout_layer=layer)
                q = p
                if name == "non_conservative_stress" or not per_atom:
                    p.requires_grad_(True)
                    if name == "non_conservative_stress":
                        if cells is None:
                            raise ValueError("a non_conservative_stress target needs `cells`")
                        q = process_non_conservative_stress(p, cells, sys)
                    if not per_atom:
                        q = _SumOverAtoms.apply(q, fw, sys)
                rs = inv_n if not per_atom and name not in self.hypers.get("per_structure_targets", ()) else None
                seed = self._run_term(name, node, q.detach(), target, total, row_scale=rs, col_scale=scales.get(b),
                                      mask=masks.get(b))
                grads[b] = seed if q is p else torch.autograd.grad(q, p, seed)[0]
            for layer in range(n_layers):
                seed_features = fw.train_predict_backward(name, grads, readout_layer=layer, seed_features=seed_features)
        return seed_features

    def _accumulate_native(self, graph, fw, n_atoms, total, target_energies=None, target_gradients=None,
                           target_strain_gradients=None, positions=None, cells=None, extra_targets=None):
        """:meth:`_accumulate` on the `loss` path: the loss is added to ``total`` on the device; returns the energies."""
        if fw.graph is not graph:  # micro-batches may share one workspace allocation
            fw.rebind(graph)
        name = self.model.target
        inv_n = n_atoms.to(torch.float64).reciprocal()
        if target_energies is None:
            if target_gradients is not None or target_strain_gradients is not None:
                raise ValueError("force / strain-gradient targets need the energy target")
            if not extra_targets:
                raise ValueError("no target to train")
            fw.forward(want_atomic=False)
            seeds, energies = None, None
        else:
            node = self.loss_spec[name]
            atomic = fw.forward()
            energies = fw.sum_over_atoms(atomic)
            d_energy = self._run_term(name, node, energies, target_energies, total, row_scale=inv_n)  # dL/dE_s
            seeds = d_energy[graph.system_of_atom().long()]
        seed_features = None
        if extra_targets:
            seed_features = self._extra_native(graph, fw, inv_n, cells, extra_targets, total)
        if target_gradients is None and target_strain_gradients is None:
            fw.backward_train(seeds, seed_features=seed_features)
            return energies
        ones = torch.ones_like(atomic)
        grad_positions, grad_cells = fw.backward(ones, want_cell_grad=True)
        u, u_cell = None, None
        if target_gradients is not None:
            u = self._run_term(f"{name}_positions_gradients", node["gradients"]["positions"], grad_positions, target_gradients,
                               total)
        if target_strain_gradients is not None:
            if positions is None or cells is None:
                raise ValueError("a strain-gradient (stress) target needs `positions` and `cells`")
            pos, cell, sys = positions.to(torch.float32), cells.to(torch.float32), graph.system_of_atom().long()
            outer = (pos[:, :, None] * grad_positions[:, None, :]).reshape(-1, 9)
            # the per-structure sum in a fixed order (index_add's float atomics would make the seeds vary run to run)
            virial = torch.stack([fw.sum_over_atoms(outer[:, j].contiguous()) for j in range(9)], dim=1).reshape(-1, 3, 3)
            virial = virial + cell.transpose(1, 2) @ grad_cells
            g = self._run_term(f"{name}_strain_gradients", node["gradients"]["strain"], virial, target_strain_gradients,
                               total)                              # dL/d(dE/deps)
            u_s = (pos[:, None, :] @ g[sys]).squeeze(1)             # d(dE/deps_ab)/d(gR_ib) = R_ia
            u = u_s if u is None else u + u_s
            u_cell = cell @ g
        fw.backward_train2(ones, seeds, u, u_cell=u_cell, seed_features=seed_features)
        return energies
