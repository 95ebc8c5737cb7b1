"""Default PET hyper-parameters (mirror of ``ModelHypers``,
src/metatrain/pet/documentation.py:159-259) -- constants only."""

DEFAULT_MODEL_HYPERS = {
    "cutoff": 4.5,
    "num_neighbors_adaptive": None,
    "adaptive_cutoff_method": "solver",
    "cutoff_function": "Bump",
    "cutoff_width": 0.5,
    "cutoff_width_adaptive": 1.0,
    "d_pet": 128,
    "d_head": 128,
    "d_node": 256,
    "d_feedforward": 256,
    "num_heads": 8,
    "num_attention_layers": 2,
    "num_gnn_layers": 2,
    "normalization": "RMSNorm",
    "activation": "SwiGLU",
    "attention_temperature": 1.0,
    "transformer_type": "PreLN",
    "featurizer_type": "feedforward",
    "zbl": False,
    "long_range": {"enable": False},  # completed from DEFAULT_LONG_RANGE_HYPERS where the other keys are read
    "system_conditioning": False,
    "max_charge": 10,
    "max_spin_multiplicity": 10,
}

# ``LongRangeHypers`` (src/metatrain/utils/long_range.py:11-26). A model dictionary may carry only ``enable``: the other four
# keys are filled in from here (``long_range_hypers``).
DEFAULT_LONG_RANGE_HYPERS = {
    "enable": False,
    "use_ewald": False,
    "smearing": 1.4,
    "kspace_resolution": 1.33,
    "interpolation_nodes": 5,
}


def long_range_hypers(hypers: dict) -> dict:
    """The ``long_range`` block of ``hypers`` with the reference's defaults for the keys it leaves out."""
    out = dict(DEFAULT_LONG_RANGE_HYPERS)
    out.update(hypers.get("long_range") or {})
    return out


def default_hypers() -> dict:
    out = dict(DEFAULT_MODEL_HYPERS)
    out["long_range"] = dict(DEFAULT_MODEL_HYPERS["long_range"])
    return out
