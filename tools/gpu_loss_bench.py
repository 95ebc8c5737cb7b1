"""Step time of the `loss` path (every loss term formed by csrc/loss.hip) against the legacy torch MSE functions, on the
bench_train.py workload (64 x 1 000-atom boxes, default model, the whole batch at once): ``ef_legacy`` / ``ef_loss``
(energy + force loss; `loss: "mse"` on the new path) and ``ncf_legacy`` / ``ncf_loss`` (+ non-conservative forces: the
legacy step reads the NaN count of a further target back in every step, the new one counts on the device). The four
configurations are stepped in turn, one step each per round, in one process, so that slow drifts of the box hit all alike.
Prints one JSON line with ms/step per configuration and the two ratios new / legacy; ``--out`` also writes it to a file.

  python tools/gpu_loss_bench.py --boxes 64 --atoms 1000 --rounds 10 --warmup 2 --out profiles/loss_bench.json
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from metatrain_amd import runtime as rt
    from metatrain_amd.pet import default_hypers
    from metatrain_amd.pet.trainer import TrainStep
    from metatrain_amd.synthetic import random_box, synthetic_params

    dev = torch.device("cuda:0")
    types = [1, 6, 7, 8]
    hypers = dict(default_hypers())
    params = synthetic_params(hypers, types, {"energy": 1, "non_conservative_forces": 3}, 0, torch.float32)
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
    configs = {"ef_legacy": (None, {}), "ef_loss": ("mse", {}), "ncf_legacy": (None, {"non_conservative_forces": ncf}),
               "ncf_loss": ("mse", {"non_conservative_forces": ncf})}
    hyp = {"warmup_fraction": 0.0, "num_epochs": 10**6}
    steps = {c: TrainStep(model, dict(hyp, **({} if loss is None else {"loss": loss}))) for c, (loss, _) in configs.items()}

    def one(c):
        return steps[c](graph, fw, target_e, per_box, target_g, cells=cells, extra_targets=configs[c][1] or None)

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
    ratio = {"ef": med["ef_loss"] / med["ef_legacy"], "ncf": med["ncf_loss"] / med["ncf_legacy"]}
    out = json.dumps({"workload": f"{args.boxes} x {args.atoms} atoms, default model, MSE energy + force loss (+ NC forces), Adam; "
                                  "legacy = torch loss functions, loss = csrc/loss.hip (`loss: mse`)",
                      "ms_per_step_median": med, "ratio_loss_over_legacy": ratio, "rounds": args.rounds, "warmup": args.warmup,
                      "ms_per_step_all": times})
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
