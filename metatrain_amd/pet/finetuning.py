"""Fine-tuning strategies of PET (``full``, ``lora``, ``heads``) for the native training step.

Behaviour follows the reference's ``pet/modules/finetuning.py``:

* ``LoRALinear`` wraps a ``torch.nn.Linear`` as ``linear`` and adds ``lora_A`` (``[rank, in]``) and ``lora_B``
  (``[out, rank]``), both bias-free; ``y = linear(x) + scaling * lora_B(lora_A(x))`` with ``scaling = alpha / rank``.
  The state-dict keys are ``<lin>.linear.weight``, ``<lin>.linear.bias``, ``<lin>.lora_A.weight``, ``<lin>.lora_B.weight``;
  the scaling is not in the state dict.
* ``lora`` freezes every parameter whose name does not contain ``lora_``; ``heads`` keeps trainable only the parameters
  whose names start with one of the head / last-layer prefixes and raises if none matches; ``full`` trains everything.

libpet_hip folds ``W + scaling B A`` into the kernels' weights (``pet_model_set_lora_scaling``) and skips the weight-gradient
work of frozen parameters (``pet_model_set_trainable``). Adapters are served on the Linears of the transformer layers
(``LORA_PLACES``), ranks 1 to 64.
"""
import re
from typing import Dict, Iterable, Optional

import torch

from .._lib import PetHipError
from ..runtime import HipModel

LORA_PLACES = ("attention.input_linear", "attention.output_linear", "mlp.w_in", "mlp.w_out", "center_mlp.w_in",
               "center_mlp.w_out", "center_contraction", "center_expansion")
DEFAULT_TARGET_MODULES = ("input_linear", "output_linear")
DEFAULT_HEADS_CONFIG = {
    "head_modules": ["node_heads", "edge_heads"],
    "last_layer_modules": ["node_last_layers", "edge_last_layers"],
}


_PLACE_RE = re.compile(r"gnn_layers\.\d+\.trans\.layers\.\d+\.(" + "|".join(re.escape(p) for p in LORA_PLACES) + r")")


def _served(lin: str) -> bool:
    return _PLACE_RE.fullmatch(lin) is not None


class LoRALinear(torch.nn.Module):
    """A Linear with a low-rank adapter: ``linear(x) + scaling * lora_B(lora_A(x))``."""

    def __init__(self, linear_layer: torch.nn.Linear, rank: int = 4, alpha: float = 1.0):
        super().__init__()
        self.linear = linear_layer
        p = linear_layer.weight
        self.lora_A = torch.nn.Linear(linear_layer.in_features, rank, bias=False, device=p.device, dtype=p.dtype)
        self.lora_B = torch.nn.Linear(rank, linear_layer.out_features, bias=False, device=p.device, dtype=p.dtype)
        self.scaling: float = float(alpha) / float(rank)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.linear(x) + self.scaling * self.lora_B(self.lora_A(x))


def inject_lora(backend: torch.nn.Module, target_modules: Iterable[str] = DEFAULT_TARGET_MODULES, rank: int = 4,
                alpha: float = 8.0) -> torch.nn.Module:
    """Replace every ``torch.nn.Linear`` attribute named in ``target_modules`` by a :class:`LoRALinear` (in place, like
    the reference's ``inject_lora_layers``). Returns ``backend``."""
    targets = tuple(target_modules)
    found = [(name, module, attr) for name, module in backend.named_modules() for attr in targets
             if isinstance(getattr(module, attr, None), torch.nn.Linear)]
    sync = getattr(backend, "_sync_core", None)
    if callable(sync):  # the mirror: refuse a placement the kernels do not serve before anything is changed
        bad = [f"{name}.{attr}" for name, _, attr in found if not _served(f"{name}.{attr}")]
        if bad:
            raise PetHipError(f"LoRA adapter on '{bad[0]}' is not served: adapters go on "
                              f"gnn_layers.<g>.trans.layers.<a>.{{{', '.join(LORA_PLACES)}}}")
    for _, module, attr in found:
        setattr(module, attr, LoRALinear(getattr(module, attr), rank=rank, alpha=alpha))
    if callable(sync):
        sync()  # the mirror (pet/backend.py) rebuilds its kernel front end for the new parameter list
    return backend


def lora_scalings(backend: torch.nn.Module) -> Dict[str, float]:
    """``{"<lin>": scaling}`` of every adapted Linear (what ``HipModel.load(..., lora_scaling=...)`` takes). Works with
    this module's :class:`LoRALinear` and the reference's (anything with ``linear``, ``lora_A``, ``lora_B``, ``scaling``)."""
    out: Dict[str, float] = {}
    for name, module in backend.named_modules():
        if all(hasattr(module, a) for a in ("linear", "lora_A", "lora_B", "scaling")):
            out[name] = float(module.scaling)
    return out


def apply_finetuning(backend: torch.nn.Module, strategy: dict, model: Optional[HipModel] = None) -> torch.nn.Module:
    """Apply a fine-tuning strategy (``{"method": "full" | "lora" | "heads", "config": {...}}``) to ``backend``: inject
    adapters (``lora``, unless already injected) and set ``requires_grad`` by the reference's rules. With ``model`` (a
    :class:`HipModel` loaded from ``backend``'s state dict), the same trainable set goes to the library, so that the native
    step (``TrainStep``) trains exactly those parameters. Returns ``backend``."""
    for p in backend.parameters():
        p.requires_grad_(True)
    method = strategy["method"]
    if method == "full":
        pass
    elif method == "lora":
        cfg = strategy.get("config", {})
        targets = tuple(cfg.get("target_modules", DEFAULT_TARGET_MODULES))
        if not lora_scalings(backend):
            inject_lora(backend, targets, rank=cfg.get("rank", 4), alpha=cfg.get("alpha", 8))
            if not lora_scalings(backend):
                raise ValueError("No LoRA layers were injected: no modules matching 'target_modules' "
                                 f"{list(targets)} were found in the model. Please check that these module names are "
                                 "correct.")
        for name, p in backend.named_parameters():
            if "lora_" not in name:
                p.requires_grad_(False)
    elif method == "heads":
        cfg = strategy.get("config", DEFAULT_HEADS_CONFIG)
        keywords = list(cfg.get("head_modules", [])) + list(cfg.get("last_layer_modules", []))
        matched = False
        for name, p in backend.named_parameters():
            on = any(name.startswith(kw) for kw in keywords)
            p.requires_grad_(on)
            matched = matched or on
        if not matched:
            raise ValueError(f"No parameters were found matching the specified 'head_modules' "
                             f"({cfg.get('head_modules', [])}) or 'last_layer_modules' ({cfg.get('last_layer_modules', [])}). "
                             "Please check that these module name prefixes are correct.")
    else:
        raise ValueError(f"Unknown finetuning strategy: {method}. Available methods are: 'full', 'lora', 'heads'.")
    if model is not None:
        set_trainable_from(backend, model)
    return backend


def set_trainable_from(backend: torch.nn.Module, model: HipModel) -> None:
    """Give ``model`` the ``requires_grad`` flags of ``backend``'s parameters (same state-dict keys)."""
    flags = {k: p.requires_grad for k, p in backend.named_parameters() if k in model._ckeys}
    model.set_trainable(flags)
