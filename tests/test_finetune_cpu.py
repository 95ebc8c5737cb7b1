"""Fine-tuning strategies on the host (no GPU): LoRA injection and its state-dict schema, the reference's freeze rules."""
import os

import numpy as np
import pytest
import torch

from metatrain_amd.pet.finetuning import LoRALinear, apply_finetuning, inject_lora, lora_scalings
from oracle import pet as opet


class _Attention(torch.nn.Module):
    def __init__(self, d):
        super().__init__()
        self.input_linear = torch.nn.Linear(d, 3 * d)
        self.output_linear = torch.nn.Linear(d, d)


class _Layer(torch.nn.Module):
    def __init__(self, d):
        super().__init__()
        self.attention = _Attention(d)
        self.norm_attention = torch.nn.LayerNorm(d)


class _Trans(torch.nn.Module):
    def __init__(self, d, n):
        super().__init__()
        self.layers = torch.nn.ModuleList([_Layer(d) for _ in range(n)])


class _Gnn(torch.nn.Module):
    def __init__(self, d, n):
        super().__init__()
        self.trans = _Trans(d, n)


class _Backend(torch.nn.Module):
    """The reference's module names around the adapted Linears, heads and last layers (a few of them)."""

    def __init__(self, d=8, n_gnn=2, n_attn=2):
        super().__init__()
        self.gnn_layers = torch.nn.ModuleList([_Gnn(d, n_attn) for _ in range(n_gnn)])
        self.combination_mlps = torch.nn.ModuleList([torch.nn.Sequential(torch.nn.Linear(2 * d, d))])
        self.node_heads = torch.nn.ModuleDict({"energy": torch.nn.Sequential(torch.nn.Linear(d, d))})
        self.edge_heads = torch.nn.ModuleDict({"energy": torch.nn.Sequential(torch.nn.Linear(d, d))})
        self.node_last_layers = torch.nn.ModuleDict({"energy": torch.nn.Linear(d, 1)})
        self.edge_last_layers = torch.nn.ModuleDict({"energy": torch.nn.Linear(d, 1)})


def test_lora_linear_schema_and_forward():
    lin = torch.nn.Linear(6, 5)
    m = LoRALinear(lin, rank=3, alpha=6.0)
    assert list(m.state_dict()) == ["linear.weight", "linear.bias", "lora_A.weight", "lora_B.weight"]
    assert m.lora_A.weight.shape == (3, 6) and m.lora_B.weight.shape == (5, 3) and m.scaling == 2.0
    x = torch.randn(4, 6)
    w_eff = lin.weight + m.scaling * m.lora_B.weight @ m.lora_A.weight
    assert torch.allclose(m(x), x @ w_eff.T + lin.bias, atol=1e-6)
    torch.jit.script(m)  # TorchScript compiles with LoRALinear in place of nn.Linear


def test_injected_keys_match_the_reference_fixture(golden_dir):
    h = opet.DEFAULT_HYPERS
    be = inject_lora(_Backend(n_gnn=h["num_gnn_layers"], n_attn=h["num_attention_layers"]), rank=4, alpha=8)
    keys = [k for k in be.state_dict() if ".lora_" in k]
    g = np.load(os.path.join(golden_dir, "pet_lora_box64.npz"))
    assert keys == [str(k) for k in g["lora_keys"]]
    scal = lora_scalings(be)
    assert set(scal.values()) == {float(g["scaling"])} and len(scal) == len(keys) // 2
    names = [n for n, _ in be.named_parameters()]
    assert len(names) == len(set(names)) == len(list(be.parameters()))


def _flags(be):
    return {n: p.requires_grad for n, p in be.named_parameters()}


def test_apply_finetuning_follows_the_reference_rules():
    be = apply_finetuning(_Backend(), {"method": "full"})
    assert all(_flags(be).values())
    be = apply_finetuning(_Backend(), {"method": "lora", "config": {"rank": 2, "alpha": 4}})
    f = _flags(be)
    assert any(".lora_" in n for n in f)
    assert all(on == ("lora_" in n) for n, on in f.items())
    assert set(lora_scalings(be).values()) == {2.0}
    be = apply_finetuning(_Backend(), {"method": "heads"})
    heads = ("node_heads", "edge_heads", "node_last_layers", "edge_last_layers")
    assert all(on == n.startswith(heads) for n, on in _flags(be).items())
    be = apply_finetuning(_Backend(), {"method": "heads", "config": {"head_modules": ["node_heads"],
                                                                      "last_layer_modules": []}})
    assert all(on == n.startswith("node_heads") for n, on in _flags(be).items())
    with pytest.raises(ValueError, match="No parameters were found"):
        apply_finetuning(_Backend(), {"method": "heads", "config": {"head_modules": ["nope"], "last_layer_modules": []}})
    with pytest.raises(ValueError, match="No LoRA layers were injected"):
        apply_finetuning(_Backend(), {"method": "lora", "config": {"target_modules": ["nope"]}})
    with pytest.raises(ValueError, match="Unknown finetuning strategy"):
        apply_finetuning(_Backend(), {"method": "dora"})


def test_new_exports_are_declared():
    from metatrain_amd import _lib

    assert "pet_model_set_lora_scaling" in _lib.SYMBOLS and "pet_model_set_trainable" in _lib.SYMBOLS


# ---- the mirror (metatrain_amd.pet.PETBackend) ------------------------------------------------------------------
def _mirror():
    from metatrain_amd.pet import PETBackend, default_hypers

    be = PETBackend(default_hypers(), [1, 6, 7, 8])
    be.add_output("energy", {"energy": [1]})
    return be


def test_injected_mirror_lists_every_parameter_once_and_scripts(golden_dir):
    be = inject_lora(_mirror(), rank=4, alpha=8)
    named = dict(be.named_parameters())
    listed = be._params()
    assert len(listed) == len(named) == len({id(p) for p in listed})
    assert {id(p) for p in listed} == {id(p) for p in named.values()}
    g = np.load(os.path.join(golden_dir, "pet_lora_box64.npz"))
    assert [k for k in be.state_dict() if ".lora_" in k] == [str(k) for k in g["lora_keys"]]
    assert set(be._lora_scaling.values()) == {2.0} and len(be._lora_scaling) == 8
    torch.jit.script(be)  # compiles with LoRALinear in place of nn.Linear


def test_mirror_follows_an_injection_it_was_not_told_about():
    """The reference's inject_lora_layers swaps attributes without telling the mirror: the next call (or
    torch.jit.script) rebuilds the kernel front end."""
    be = _mirror()
    layer = be.gnn_layers[0].trans.layers[1]
    layer.mlp.w_out = LoRALinear(layer.mlp.w_out, rank=2, alpha=3.0)
    be._sync_core()
    assert be._lora_scaling == {"gnn_layers.0.trans.layers.1.mlp.w_out": 1.5}
    assert len(be._params()) == len(list(be.parameters()))
    torch.jit.script(be)


def test_unserved_mirror_placement_is_refused_before_any_change():
    from metatrain_amd._lib import PetHipError

    be = _mirror()
    before = list(be.state_dict())
    with pytest.raises(PetHipError, match=r"LoRA adapter on '\S+\.0' is not served"):
        inject_lora(be, ("input_linear", "0"), rank=2, alpha=2)
    assert list(be.state_dict()) == before
