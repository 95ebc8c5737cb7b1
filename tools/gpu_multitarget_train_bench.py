"""Native training step with further targets on the bench_train.py workload (64 x 1 000-atom boxes, default model, the
whole batch at once): ``ef`` (energy + force loss), ``ef_ncf`` (+ non-conservative forces) and ``ef_ncf_ncs``
(+ non-conservative stress). One model holds the three targets' heads and the three configurations are stepped in turn,
one step each per round, in one process, so that slow drifts of the box hit all three alike (in ``ef`` the two idle
heads are left out of Adam, as torch's optimizer leaves a parameter without .grad). Prints one JSON line with ms/step
per configuration.

  python tools/gpu_multitarget_train_bench.py --boxes 64 --atoms 1000 --rounds 10 --warmup 2
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
    ap.add_argument("--boxes", type=int, default=64)
    ap.add_argument("--atoms", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    from metatrain_amd import runtime as rt
    from metatrain_amd.pet import default_hypers
    from metatrain_amd.pet.trainer import TrainStep
    from metatrain_amd.synthetic import random_box, synthetic_params

    dev = torch.device("cuda:0")
    types = [1, 6, 7, 8]
    hypers = dict(default_hypers())
    params = synthetic_params(hypers, types, {"energy": 1, "non_conservative_forces": 3, "non_conservative_stress": 9},
                              0, torch.float32)
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
    ncf = {"values": (torch.randn(n, 3, generator=gen) * 0.1).to(dev)}
    ncs = {"values": (torch.randn(args.boxes, 3, 3, 1, generator=gen) * 1e-3).to(dev), "per_atom": False}
    configs = {"ef": {}, "ef_ncf": {"non_conservative_forces": ncf},
               "ef_ncf_ncs": {"non_conservative_forces": ncf, "non_conservative_stress": ncs}}
    hyp = {"warmup_fraction": 0.0, "num_epochs": 10**6, "per_structure_targets": ["non_conservative_stress"],
           "loss_weights": {"energy": 1.0, "forces": 1.0, "non_conservative_forces": 1.0, "non_conservative_stress": 1.0}}
    steps = {c: TrainStep(model, hyp) for c in configs}

    def one(c):
        return steps[c](graph, fw, target_e, per_box, target_g, cells=cells, extra_targets=configs[c] or None)

    for _ in range(args.warmup):
        for c in configs:
            one(c)
    torch.cuda.synchronize()
    times = {c: [] for c in configs}
    for _ in range(args.rounds):
        for c in configs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one(c)
            torch.cuda.synchronize()
            times[c].append((time.perf_counter() - t0) * 1e3)
    med = {c: sorted(t)[len(t) // 2] for c, t in times.items()}
    over = {c: med[c] / med["ef"] - 1.0 for c in configs if c != "ef"}
    print(json.dumps({"workload": f"{args.boxes} x {args.atoms} atoms, default model, energy + force loss (+ NC targets), Adam",
                      "ms_per_step_median": med, "overhead_vs_ef": over, "ms_per_step_all": times}))


if __name__ == "__main__":
    main()
