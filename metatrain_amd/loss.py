"""Training losses formed on the device (``utils/loss.py``, ``utils/omegaconf.py:432-724``, ``utils/metrics.py``): the
reference trainer's ``loss`` hyper -- per target and per gradient ``type: mse | mae | huber | masked_mse | masked_mae |
masked_huber``, ``weight``, ``reduction: mean | sum`` and, for Huber, ``delta`` -- restated for plain tensors. Model-agnostic:
nothing here knows PET.

:func:`expand_loss_hypers` turns the shorthand forms into the fully explicit dict and refuses what is not served.
:class:`PointwiseLoss` is one loss TERM (one prediction array against one target array) on ``csrc/loss.hip``: the number of
valid entries is counted on the device (:meth:`PointwiseLoss.count`), and the loss, its seeds dL/d(prediction) and the sums of
the reference's RMSE / MAE accumulators come out of one call that reads that count from device memory -- fp64 arithmetic,
fixed summation order, bitwise reproducible, no read-back. :class:`LossMetrics` adds the terms' statistics up over the batches
of an epoch and reads them back once.

    spec = expand_loss_hypers({"energy": {"type": "huber", "delta": 0.1, "forces": "mae"}},
                              {"energy": {"is_energy": True, "gradients": ["positions"]}})
    term = PointwiseLoss()
    term.count(pred, target)
    loss, seed = term(pred, target, kind="huber", delta=0.1, weight=1.0, reduction="mean", row_scale=1.0 / n_atoms)

Not served, each refused by name: ``reduction: none``, ``shift_agnostic_mse``, the ``*_ensemble`` losses, the ``pointwise`` /
``masked_pointwise`` base classes (they take a torch module, not a type).
"""
from typing import Dict, Iterable, Optional, Tuple

import torch

from . import _lib
from . import runtime as rt
from ._lib import check

SERVED_TYPES = ("mse", "mae", "huber", "masked_mse", "masked_mae", "masked_huber")
# utils/loss.py:1186-1205 LossType, in its order
REFERENCE_TYPES = SERVED_TYPES + ("pointwise", "masked_pointwise", "shift_agnostic_mse", "gaussian_nll_ensemble",
                                  "gaussian_crps_ensemble", "empirical_crps_ensemble")
DEFAULT_HUBER_DELTA = 1.0
GRADIENT_SHORTHANDS = {"forces": "positions", "stress": "strain", "virial": "strain"}
STATE_WORDS = 5  # the device state of a term, 8 bytes each: the valid count of the step (int64), then pet_loss_stats_t


def _check_node(node: dict, where: str) -> dict:
    """Defaults (``_add_defaults_in_place``, ``utils/omegaconf.py:523-539``) and the refusals of one {type, weight, ...}."""
    node = dict(node)
    node.setdefault("type", "mse")
    node.setdefault("weight", 1.0)
    node.setdefault("reduction", "mean")
    kind = node["type"]
    if kind not in REFERENCE_TYPES:
        raise ValueError(f"Unknown loss '{kind}'. Valid types: {', '.join(REFERENCE_TYPES)}")  # utils/loss.py:1233-1234
    if kind not in SERVED_TYPES:
        raise NotImplementedError(f"{where}: the loss type '{kind}' is not served (served: {', '.join(SERVED_TYPES)})")
    if node["reduction"] == "none":
        raise NotImplementedError(f"{where}: 'reduction: none' is not served (a training loss is a scalar: mean or sum)")
    if node["reduction"] not in ("mean", "sum"):
        raise ValueError(f"{where}: unknown reduction '{node['reduction']}'. Valid reductions: mean, sum")
    node["weight"] = float(node["weight"])
    if kind.endswith("huber"):
        node["delta"] = float(node.get("delta", DEFAULT_HUBER_DELTA))
        if not node["delta"] > 0.0:
            raise ValueError(f"{where}: the Huber delta must be positive, got {node['delta']}")
    return node


def expand_loss_hypers(loss, targets) -> Dict[str, dict]:
    """``expand_loss_config`` (``utils/omegaconf.py:432-724``) without the dataset section. ``loss``: None (all defaults), one
    type for every target and gradient, ``{target: type}``, or ``{target: {type, weight, reduction, delta, forces | stress |
    virial | gradients: {positions | strain: type or dict}}}``. ``targets``: the targets that exist, ``{name: {"is_energy":
    bool, "gradients": ["positions", "strain"]}}`` (``is_energy`` defaults to ``name == "energy"``; a list of names: no
    gradients). Returns ``{target: {"type", "weight", "reduction", ["delta"], "gradients": {name: {...}}}}`` for every
    target, each gradient a target carries included."""
    if not isinstance(targets, dict):
        targets = {str(n): {} for n in targets}
    flags = {}
    for name, info in targets.items():
        info = info or {}
        flags[name] = {"is_energy": bool(info.get("is_energy", name == "energy")), "gradients": list(info.get("gradients", ()))}
    if loss is not None and not isinstance(loss, (str, dict)):
        raise ValueError(f"the loss hyper is a type, or a dict of targets, got {type(loss).__name__}")
    if isinstance(loss, dict):
        for key in loss:
            if key not in flags:
                raise ValueError(f"Invalid top-level loss entry '{key}'. Allowed keys are: {sorted(flags)} or a single string.")
    out = {}
    for name, flag in flags.items():
        raw = loss.get(name) if isinstance(loss, dict) else None
        raw = {"type": raw} if isinstance(raw, str) else dict(raw or {})
        base = {k: v for k, v in raw.items() if k not in ("forces", "stress", "virial", "gradients")}
        gradients = {g: {} for g in flag["gradients"] if flag["is_energy"]}
        if isinstance(loss, str):
            base["type"] = loss
            for g in gradients.values():
                g["type"] = loss
        short = [k for k in GRADIENT_SHORTHANDS if k in raw]
        if short and not flag["is_energy"]:
            raise ValueError("'forces', 'stress', 'virial' loss entries are only allowed for energy-like targets, but target "
                             f"'{name}' is not energy-like.")
        if "stress" in raw and "virial" in raw:
            raise ValueError(f"Both 'stress' and 'virial' provided for target '{name}'. Use only one of them.")
        overrides = {}
        for k in short:
            overrides[GRADIENT_SHORTHANDS[k]] = {"type": raw[k]} if isinstance(raw[k], str) else dict(raw[k])
        for g, val in (raw.get("gradients") or {}).items():
            overrides.setdefault(g, {}).update({"type": val} if isinstance(val, str) else dict(val))
        for g, val in overrides.items():
            gradients.setdefault(g, {}).update(val)
        node = _check_node(base, f"loss of '{name}'")
        node["gradients"] = {g: _check_node(v, f"loss of the '{g}' gradient of '{name}'") for g, v in gradients.items()}
        out[name] = node
    return out


def _two_d(t: torch.Tensor) -> torch.Tensor:
    width = 1
    for d in t.shape[1:]:
        width *= int(d)
    return t.reshape(int(t.shape[0]) if t.dim() else 1, width)


class PointwiseLoss:
    """One loss term on the device. It owns its workspace and its device state: the step's valid count and the statistics
    block (``pet_loss_stats_t``), both ``+=`` across calls until :meth:`reset`.

    ``state``: an int64 ``[5]`` device tensor to keep them in (a caller with many terms zeroes one ``[terms, 5]`` tensor
    per step and hands out its rows); by default the term allocates its own on first use."""

    def __init__(self, state: Optional[torch.Tensor] = None):
        self._workspace: Optional[torch.Tensor] = None
        self._state: Optional[torch.Tensor] = None
        if state is not None:
            self.bind(state)

    def bind(self, state: torch.Tensor) -> "PointwiseLoss":
        rt._require_cuda(state)
        if state.dtype != torch.int64 or state.numel() != STATE_WORDS or not state.is_contiguous():
            raise ValueError(f"the state of a loss term is a contiguous int64 [{STATE_WORDS}] device tensor")
        self._state = state.reshape(STATE_WORDS)
        return self

    def reset(self) -> None:
        if self._state is not None:
            self._state.zero_()

    def _state_on(self, device) -> torch.Tensor:
        if self._state is None or self._state.device != device:
            self._state = torch.zeros(STATE_WORDS, dtype=torch.int64, device=device)
        return self._state

    def _prepare(self, like: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor]):
        rt._require_cuda(like, target, *([] if mask is None else [mask]))
        shape = _two_d(like).shape
        if target.numel() != like.numel():
            raise ValueError(f"target of {tuple(target.shape)} against a prediction of {tuple(like.shape)}")
        t = target.detach().to(torch.float32).reshape(shape).contiguous()
        m = None
        if mask is not None:
            if mask.numel() != like.numel():
                raise ValueError(f"mask of {tuple(mask.shape)} against a prediction of {tuple(like.shape)}")
            m = mask.detach().reshape(shape).contiguous()
            m = m.view(torch.uint8) if m.dtype == torch.bool else (m if m.dtype == torch.uint8 else (m != 0).view(torch.uint8))
        return int(shape[0]), int(shape[1]), t, m

    def count(self, pred_like: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None) -> None:
        """Add this array's valid entries (target not NaN, mask non-zero) to the term's device count: the denominator of
        ``reduction = "mean"``. ``pred_like`` gives the ``[rows, ...]`` shape; a prediction need not exist yet."""
        rows, width, t, m = self._prepare(pred_like, target, mask)
        state = self._state_on(t.device)
        with torch.cuda.device(t.device):
            check(_lib.load().pet_loss_count(rt._ptr(t), rt._ptr(m), rows, width, rt._ptr(state), rt._stream()))

    def __call__(self, pred: torch.Tensor, target: torch.Tensor, *, kind: str, delta: float = DEFAULT_HUBER_DELTA,
                 weight: float = 1.0, reduction: str = "mean", row_scale: Optional[torch.Tensor] = None,
                 col_scale: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, want_seed: bool = True,
                 loss_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """``(loss, seed)``: ``weight * sum l(d) / D`` as a 0-d fp64 device tensor (added to ``loss_out`` when one is
        given) and ``dL/d(pred)`` in ``pred``'s shape (None with ``want_seed = False``, the evaluation form), for
        ``d = pred * row_scale[row] * col_scale[property] - target * row_scale[row]``; ``D`` is what :meth:`count` has
        added up since the last :meth:`reset` (``mean``) or 1 (``sum``)."""
        if kind not in _lib.PET_LOSS_KINDS:
            raise ValueError(f"unknown loss kind '{kind}': one of {sorted(_lib.PET_LOSS_KINDS)} (a masked type is its kind plus a mask)")
        if reduction not in _lib.PET_LOSS_REDUCTIONS:
            raise ValueError(f"unknown reduction '{reduction}': mean or sum")
        if pred.dtype != torch.float32:
            raise ValueError(f"float32 predictions, got {pred.dtype}")
        rows, width, t, m = self._prepare(pred, target, mask)
        dev = t.device
        p = _two_d(pred.detach()).contiguous()
        rs = cs = None
        if row_scale is not None:
            rt._require_cuda(row_scale)
            rs = row_scale.detach().to(torch.float64).reshape(-1).contiguous()
            if rs.numel() != rows:
                raise ValueError(f"{rs.numel()} row scales for {rows} rows")
        if col_scale is not None:
            cs = torch.as_tensor(col_scale).detach().to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
            if cs.numel() < 1 or width % cs.numel():
                raise ValueError(f"{cs.numel()} column scales (properties) do not divide the {width} values of a row")
        state = self._state_on(dev)
        lib = _lib.load()
        need = int(lib.pet_loss_workspace_bytes(rows, width))
        if self._workspace is None or self._workspace.device != dev or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        if loss_out is None:
            loss_out = torch.zeros((), dtype=torch.float64, device=dev)
        elif loss_out.dtype != torch.float64 or loss_out.numel() != 1 or loss_out.device != dev:
            raise ValueError("loss_out is a float64 device scalar")
        seed = torch.empty(p.shape, dtype=torch.float32, device=dev) if want_seed else None
        with torch.cuda.device(dev):
            check(lib.pet_loss_pointwise(rt._ptr(p), rt._ptr(t), rt._ptr(m), rt._ptr(rs), rt._ptr(cs),
                                         0 if cs is None else int(cs.numel()), rows, width, _lib.PET_LOSS_KINDS[kind], float(delta),
                                         float(weight), _lib.PET_LOSS_REDUCTIONS[reduction], rt._ptr(state), rt._ptr(seed),
                                         rt._ptr(loss_out), rt._ptr(state[1:]), rt._ptr(self._workspace),
                                         self._workspace.numel(), rt._stream()))
        return loss_out, (None if seed is None else seed.reshape(pred.shape))

    def stats(self) -> torch.Tensor:
        """The statistics block as a float64 ``[4]`` device tensor (a view, no read-back): the loss, ``sum d^2``,
        ``sum |d|`` and, as the int64 behind the last entry, the valid count. :func:`read_stats` reads one back."""
        if self._state is None:
            raise _lib.PetHipError("the term has not been used yet")
        return self._state[1:].view(torch.float64)


def read_stats(block: torch.Tensor) -> Dict[str, float]:
    """A statistics block on the host (one read-back)."""
    b = block.detach().reshape(4).cpu()
    return {"loss": float(b[0]), "sum_sq": float(b[1]), "sum_abs": float(b[2]), "count": int(b.view(torch.int64)[3])}


class LossMetrics:
    """``RMSEAccumulator`` and ``MAEAccumulator`` of the reference (``utils/metrics.py``) over the statistics blocks of the
    training step (``TrainStep``'s ``"terms"``): SSE, SAE and counts are added up on the device, batch after batch, and read
    back once, in :meth:`finalize`."""

    def __init__(self):
        self._acc: Dict[str, torch.Tensor] = {}

    def update(self, terms: Dict[str, torch.Tensor]) -> None:
        for key, block in terms.items():
            rt._require_cuda(block)
            if block.dtype != torch.float64 or block.numel() != 4:
                raise ValueError(f"'{key}': a statistics block is a float64 [4] device tensor")
            block = block.detach().reshape(4)
            if key not in self._acc:
                self._acc[key] = block.clone()
            else:
                acc = self._acc[key]
                acc[:3] += block[:3]
                acc.view(torch.int64)[3:] += block.view(torch.int64)[3:]

    def finalize(self, is_distributed: bool = False, not_per_atom: Optional[Iterable[str]] = None) -> Dict[str, float]:
        """``{"<key> RMSE": sqrt(SSE / n), "<key> MAE": SAE / n}`` per term (``utils/metrics.py:195-242,384-431``), the keys
        as the reference writes them (``energy``, ``energy_positions_gradients``, ...). With ``not_per_atom`` (a list of
        strings) a key that contains none of them gets the reference's `` (per atom)`` suffix. ``is_distributed``: SSE, SAE
        and counts are summed over the ranks first, over the union of the ranks' keys."""
        keys = sorted(self._acc)
        if is_distributed:
            import torch.distributed as dist

            gathered = [None] * dist.get_world_size()
            dist.all_gather_object(gathered, keys)
            keys = sorted(set(k for ks in gathered for k in ks))
        if not keys:
            return {}
        device = next(iter(self._acc.values())).device if self._acc else torch.device("cuda", torch.cuda.current_device())
        zero = torch.zeros(4, dtype=torch.float64, device=device)
        blocks = torch.stack([self._acc.get(k, zero) for k in keys])
        sums, counts = blocks[:, 1:3].contiguous(), blocks.view(torch.int64)[:, 3].contiguous()
        if is_distributed:
            dist.all_reduce(sums)
            dist.all_reduce(counts)
        sums, counts = sums.cpu(), counts.cpu()
        out = {}
        for i, key in enumerate(keys):
            suffix = "" if not_per_atom is None or any(s in key for s in not_per_atom) else " (per atom)"
            n = float(counts[i])
            out[f"{key} RMSE{suffix}"] = (float(sums[i, 0]) / n) ** 0.5 if n else float("nan")
            out[f"{key} MAE{suffix}"] = float(sums[i, 1]) / n if n else float("nan")
        return out
