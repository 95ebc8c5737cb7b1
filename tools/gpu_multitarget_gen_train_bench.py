"""Native training step with further targets on the SIZE-GENERIC pass: a d_pet = 64 model (``s64`` of
``tests/test_gpu_gen_train.py``) on 8 x 1 000-atom boxes, the whole batch at once. ``ef`` = energy + force loss, ``ef_x3`` =
the same plus non-conservative forces, non-conservative stress and a two-block per-atom target. One model holds every head
and the two configurations are timed in turn, in one process, with bench_train.py's loop (a host clock around ``--steps``
steps that end in a device synchronise); in ``ef`` the idle heads are left out of Adam, as torch's optimizer leaves a
parameter without .grad. Prints one JSON line per configuration.

  python tools/gpu_multitarget_gen_train_bench.py --boxes 8 --atoms 1000 --steps 5 --rounds 5 --warmup 2
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S64 = dict(d_pet=64, d_node=128, d_feedforward=128, d_head=64, num_heads=4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=8)
    ap.add_argument("--atoms", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    from metatrain_amd import runtime as rt
    from metatrain_amd.pet import default_hypers
    from metatrain_amd.pet.trainer import TrainStep
    from metatrain_amd.synthetic import random_box, synthetic_params

    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    dev = torch.device("cuda:0")
    types = [1, 6, 7, 8]
    hypers = dict(default_hypers(), **S64)
    targets = {"energy": 1, "non_conservative_forces": 3, "non_conservative_stress": 9, "multi": {"a": 3, "b": 6}}
    params = synthetic_params(hypers, types, targets, 0, torch.float32)
    model = rt.HipModel(hypers, types)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")

    gen = torch.Generator().manual_seed(1234)
    pos_l, z_l, cell_l, pair_l, sys_l = [], [], [], [], []
    for b in range(args.boxes):
        pos, z, cell = random_box(args.atoms, seed=b)
        posd = pos.to(dev)
        pairs, _ = rt.neighbor_list(posd, cell, [True] * 3, hypers["cutoff"])
        pairs = pairs.clone()
        pairs[:, 0:2] += b * args.atoms
        pos_l.append(posd); z_l.append(z.to(dev)); cell_l.append(cell.to(dev)); pair_l.append(pairs)
        sys_l.append(torch.full((args.atoms,), b, dtype=torch.int32, device=dev))
    pairs = torch.cat(pair_l)
    cells = torch.stack(cell_l)
    graph = rt.HipGraph(model, torch.cat(pos_l), cells, pairs[:, 0].contiguous(), pairs[:, 1].contiguous(),
                        pairs[:, 2:5].contiguous(), torch.cat(z_l), torch.cat(sys_l))
    fw = rt.HipForward(model, graph, train=True)
    n = args.boxes * args.atoms
    per_box = torch.full((args.boxes,), float(args.atoms), device=dev)
    target_e = (torch.randn(args.boxes, generator=gen) * 0.1).to(dev) * per_box
    target_g = (torch.randn(n, 3, generator=gen) * 0.1).to(dev)
    extras = {
        "non_conservative_forces": {"values": (torch.randn(n, 3, generator=gen) * 0.1).to(dev)},
        "non_conservative_stress": {"values": (torch.randn(args.boxes, 3, 3, 1, generator=gen) * 1e-3).to(dev), "per_atom": False},
        "multi": {"values": {"a": torch.randn(n, 3, generator=gen).to(dev), "b": torch.randn(n, 3, 2, generator=gen).to(dev)}},
    }
    configs = {"ef": None, "ef_x3": extras}
    hyp = {"warmup_fraction": 0.0, "num_epochs": 10**6, "per_structure_targets": ["non_conservative_stress"],
           "loss_weights": {"energy": 1.0, "forces": 1.0, "non_conservative_forces": 1.0, "non_conservative_stress": 1.0, "multi": 1.0}}
    steps = {c: TrainStep(model, hyp) for c in configs}

    def one(c):
        return steps[c](graph, fw, target_e, per_box, target_g, cells=cells, extra_targets=configs[c])

    for _ in range(args.warmup):
        for c in configs:
            one(c)
    torch.cuda.synchronize()
    times = {c: [] for c in configs}
    loss = {}
    for _ in range(args.rounds):
        for c in configs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss[c] = one(c)["loss"]
            torch.cuda.synchronize()
            times[c].append((time.perf_counter() - t0) / args.steps * 1e3)
    med = {c: sorted(t)[len(t) // 2] for c, t in times.items()}
    for c in configs:
        assert float(loss[c]) == float(loss[c]), "training diverged to NaN"
        print(json.dumps({
            "config": c, "workload": f"{args.boxes} x {args.atoms} atoms ({graph.n_edges} edges), d_pet = 64 model on the size-generic "
                                     "training pass, energy + force loss" + (" + NC forces + NC stress + two-block target" if configs[c] else "")
                                     + ", Adam",
            "ms_per_step": med[c], "atom_steps_per_s": n / med[c] * 1e3, "ratio_to_ef": med[c] / med["ef"],
            "steps_per_round": args.steps, "ms_per_step_rounds": times[c]}), flush=True)


if __name__ == "__main__":
    main()
