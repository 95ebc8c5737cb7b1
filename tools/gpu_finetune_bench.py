"""Native training step (energy + force loss, Adam) under the three fine-tuning strategies, on the bench_train.py
workload: ``full`` (every parameter), ``lora`` (rank-4 adapters on attention.input_linear / output_linear, everything
else frozen) and ``heads`` (heads and last layers only). The three models are stepped in turn, one step each per round,
in one process, so that slow drifts of the box hit all three alike. Prints one JSON line with ms/step per strategy.

  python tools/gpu_finetune_bench.py --boxes 16 --atoms 1000 --rounds 10 --warmup 2
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=16)
    ap.add_argument("--atoms", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    from metatrain_amd import runtime as rt
    from metatrain_amd.pet import default_hypers
    from metatrain_amd.pet.finetuning import apply_finetuning, inject_lora, lora_scalings
    from metatrain_amd.pet.trainer import TrainStep
    from metatrain_amd.synthetic import random_box, synthetic_params

    dev = torch.device("cuda:0")
    types = [1, 6, 7, 8]
    hypers = dict(default_hypers())
    base = synthetic_params(hypers, types, {"energy": 1}, 0, torch.float32)

    class _Holder(torch.nn.Module):
        """The state dict as a module tree (Linears where a weight / bias pair is), so that the strategies can name and
        adapt its parameters."""

        def __init__(self, params):
            super().__init__()
            for k, v in params.items():
                if k == "species_to_species_index":
                    continue
                path, leaf = k.rsplit(".", 1)
                w = params.get(path + ".weight")
                is_lin = w is not None and w.dim() == 2 and path + ".bias" in params
                mod = self
                parts = path.split(".")
                for i, p in enumerate(parts):
                    if not hasattr(mod, p):
                        last = i == len(parts) - 1
                        mod.add_module(p, torch.nn.Linear(w.shape[1], w.shape[0]) if last and is_lin else torch.nn.Module())
                    mod = getattr(mod, p)
                with torch.no_grad():
                    if is_lin:
                        getattr(mod, leaf).copy_(v)
                    else:
                        mod.register_parameter(leaf, torch.nn.Parameter(v.clone()))

    gen = torch.Generator().manual_seed(1234)
    pos_l, z_l, cell_l, pair_l, sys_l = [], [], [], [], []
    models, steps, fws = {}, {}, {}
    for mode in ("full", "lora", "heads"):
        holder = _Holder(base)
        if mode == "lora":
            inject_lora(holder, ("input_linear", "output_linear"), rank=4, alpha=8)
            for n, p in holder.named_parameters():
                if "lora_" in n:
                    torch.nn.init.normal_(p, std=0.05, generator=gen)
        apply_finetuning(holder, {"method": mode, "config": {"rank": 4, "alpha": 8}} if mode == "lora" else {"method": mode})
        params = {"species_to_species_index": base["species_to_species_index"], **holder.state_dict()}
        model = rt.HipModel(hypers, types)
        model.load({k: v.detach().to(dev) for k, v in params.items()}, "energy", lora_scaling=lora_scalings(holder) or None)
        if mode != "full":
            model.set_trainable({k: p.requires_grad for k, p in holder.named_parameters()})
        models[mode] = model
        steps[mode] = TrainStep(model, {"warmup_fraction": 0.0, "num_epochs": 10**6})

    for b in range(args.boxes):
        pos, z, cell = random_box(args.atoms, seed=b)
        posd = pos.to(dev)
        pairs, _ = rt.neighbor_list(posd, cell, [True] * 3, hypers["cutoff"])
        pairs = pairs.clone()
        pairs[:, 0:2] += b * args.atoms
        pos_l.append(posd); z_l.append(z.to(dev)); cell_l.append(cell.to(dev)); pair_l.append(pairs)
        sys_l.append(torch.full((args.atoms,), b, dtype=torch.int32, device=dev))
    pairs = torch.cat(pair_l)
    per_box = torch.full((args.boxes,), float(args.atoms), device=dev)
    target_e = (torch.randn(args.boxes, generator=gen) * 0.1).to(dev) * per_box
    target_g = (torch.randn(args.boxes * args.atoms, 3, generator=gen) * 0.1).to(dev)
    graphs = {}
    for mode, model in models.items():
        graphs[mode] = rt.HipGraph(model, torch.cat(pos_l), torch.stack(cell_l), pairs[:, 0].contiguous(),
                                   pairs[:, 1].contiguous(), pairs[:, 2:5].contiguous(), torch.cat(z_l), torch.cat(sys_l))
        fws[mode] = rt.HipForward(model, graphs[mode], train=True)

    def one(mode):
        return steps[mode](graphs[mode], fws[mode], target_e, per_box, target_g)

    for _ in range(args.warmup):
        for mode in models:
            one(mode)
    torch.cuda.synchronize()
    times = {mode: [] for mode in models}
    for _ in range(args.rounds):
        for mode in models:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one(mode)
            torch.cuda.synchronize()
            times[mode].append((time.perf_counter() - t0) * 1e3)
    med = {mode: sorted(t)[len(t) // 2] for mode, t in times.items()}
    print(json.dumps({"workload": f"{args.boxes} x {args.atoms} atoms, energy + force loss, Adam",
                      "ms_per_step_median": med, "ms_per_step_all": times}))


if __name__ == "__main__":
    main()
