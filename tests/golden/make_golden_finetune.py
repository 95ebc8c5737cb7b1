"""Generate ``pet_lora_box64.npz``: a LoRA-injected PET evaluated by the reference itself.

The reference ``PETBackend`` (default hypers, ``oracle.pet.synthetic_params`` seed 0, the inputs of
``pet_default_box64.npz``) gets the reference's own ``inject_lora_layers(("input_linear", "output_linear"), rank=4,
alpha=8)`` (pet/modules/finetuning.py); every ``lora_A`` / ``lora_B`` is then filled from a seeded generator, rounded to
fp32 so that the fp32 library sees the same values. Stored (fp64 unless noted):

    lora_keys            the adapter keys, as the reference's state dict spells them (str)
    lora::<key>          the adapter tensors (fp32 values)
    scaling              alpha / rank
    energies, atomic, grad        E, per-atom E, dE/dR
    seed_w [N], seed_u [N,3]      the loss L = sum_i w_i E_i + sum u . dE/dR
    dL::<key>            dL/d(adapter) by autograd (create_graph) through the reference
    in_*                 the inputs of pet_default_box64.npz

Run from the repository root with the reference checkout available (not needed by any test).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

RANK, ALPHA = 4, 8.0


def import_reference_finetuning():
    class TargetInfo:  # annotation-only name
        pass

    for pkg in ("metatrain.utils", "metatrain.utils.data"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    m = types.ModuleType("metatrain.utils.data.target_info")
    m.TargetInfo = TargetInfo
    sys.modules[m.__name__] = m
    name = "metatrain.pet.modules.finetuning"
    spec = importlib.util.spec_from_file_location(name, f"{make_golden.REF}/pet/modules/finetuning.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    from oracle import pet as opet

    PETBackend = make_golden.import_reference_backend()
    ft = import_reference_finetuning()
    torch.set_num_threads(8)
    hyp = dict(opet.DEFAULT_HYPERS)
    be, _ = make_golden._reference_backend(PETBackend, hyp, torch.float64)
    be = ft.inject_lora_layers(be, target_modules=("input_linear", "output_linear"), rank=RANK, alpha=ALPHA,
                               dtype=torch.float64)
    sd = be.state_dict()
    lora_keys = [k for k in sd if ".lora_" in k]
    gen = torch.Generator().manual_seed(2024)
    with torch.no_grad():
        for k in lora_keys:
            p = dict(be.named_parameters())[k]
            p.copy_((0.05 * torch.randn(p.shape, generator=gen, dtype=torch.float64)).float().double())
    scalings = {m.scaling for m in be.modules() if isinstance(m, ft.LoRALinear)}
    assert scalings == {ALPHA / RANK}, scalings

    g = dict(np.load(os.path.join(HERE, "pet_default_box64.npz")))
    inp = {k: torch.tensor(v) for k, v in g.items() if k.startswith("in_")}
    pos = inp["in_positions"].double().clone().requires_grad_(True)
    cells = inp["in_cells"].double()
    sysidx = inp["in_system_indices"].long()
    batch = be.preprocess(pos, inp["in_centers"].long(), inp["in_neighbors"].long(), inp["in_species"].long(), cells,
                          inp["in_cell_shifts"].long(), sysidx, 1.0)
    nf, ef = be.calculate_features(batch)
    pred, _, _ = be.predict(nf, ef, batch, cells, sysidx, ["energy"])
    atomic = pred["energy"][0][:, 0]
    (grad,) = torch.autograd.grad(atomic.sum(), pos, create_graph=True)
    n = atomic.shape[0]
    sg = torch.Generator().manual_seed(11)
    w = (torch.rand(n, generator=sg, dtype=torch.float64) - 0.5).float().double()
    u = torch.randn(n, 3, generator=sg, dtype=torch.float64).float().double()
    loss = (w * atomic).sum() + (u * grad).sum()
    named = dict(be.named_parameters())
    dl = torch.autograd.grad(loss, [named[k] for k in lora_keys])

    store = {k: v for k, v in g.items() if k.startswith("in_")}
    store["lora_keys"] = np.array(lora_keys)
    store["scaling"] = np.array(ALPHA / RANK)
    for k in lora_keys:
        store["lora::" + k] = named[k].detach().float().numpy()
    for k, d in zip(lora_keys, dl):
        store["dL::" + k] = d.numpy()
    store["energies"] = atomic.detach().sum().reshape(1, 1).numpy()
    store["atomic"] = atomic.detach()[:, None].numpy()
    store["grad"] = grad.detach().numpy()
    store["seed_w"] = w.numpy()
    store["seed_u"] = u.numpy()
    out = os.path.join(HERE, "pet_lora_box64.npz")
    np.savez_compressed(out, **store)
    print("pet_lora_box64: E =", float(store["energies"][0, 0]), "|grad|max =", float(np.abs(store["grad"]).max()),
          len(lora_keys), "adapter tensors,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
