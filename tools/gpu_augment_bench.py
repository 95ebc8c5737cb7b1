"""Rotational augmentation on the device data path, measured on the two training workloads (64 x 1 000 and 8 x 10 000 atoms,
default PET, energy + force loss, Adam):

  (a) the augmenter call alone (``O3Augmenter.apply_random_augmentations``: positions, cells and a force target), and its
      two launches alone (``runtime.o3_draw``, ``runtime.o3_apply``); ``enqueue`` is the host time of a call before any
      synchronisation, i.e. what the launches and the Python around them cost;
  (b) ``data.collate`` alone (the neighbour search and the concatenation);
  (c) one optimizer step with the batch collated ONCE and augmented every step, against a step that collates again every
      step (what a loop has to do when it rotates before the neighbour search, as the reference does). Both build the
      graph from their pair list every step; the two arms alternate in one process.

A step walks its boxes in ``--micro`` micro-batches (gradient accumulation, ``TrainStep.microbatched``; default: two), each
with its own cached batch, because the training workspace of all 64 000 / 80 000 atoms at once takes most of the device.
Times are host clocks around work that ends in a device synchronisation, medians over ``--steps`` samples after
``--warmup``. Prints one JSON line.

  python tools/gpu_augment_bench.py --steps 5 --warmup 2
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def _timed(fn, warmup, steps, inner=1):
    """ms per call of ``fn``: ``inner`` calls between two synchronisations per sample. Returns (median, all, median host
    time per call before the synchronisation)."""
    for _ in range(warmup):
        fn()
    total, enqueue = [], []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        total.append((time.perf_counter() - t0) * 1e3 / inner)
        enqueue.append((t1 - t0) * 1e3 / inner)
    return _median(total), total, _median(enqueue)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--micro", type=int, default=2, help="micro-batches per optimizer step")
    ap.add_argument("--inner", type=int, default=20, help="augmenter calls per timed sample of (a)")
    ap.add_argument("--sizes", default="64x1000,8x10000", help="boxes x atoms, comma separated")
    args = ap.parse_args()

    from metatrain_amd import data
    from metatrain_amd import runtime as rt
    from metatrain_amd._lib import PetHipError
    from metatrain_amd.augmentation import O3Augmenter
    from metatrain_amd.pet import default_hypers
    from metatrain_amd.pet.trainer import TrainStep
    from metatrain_amd.synthetic import random_box, synthetic_params

    dev = torch.device("cuda:0")
    types = [1, 6, 7, 8]
    hypers = dict(default_hypers())
    cutoff = float(hypers["cutoff"])
    params = synthetic_params(hypers, types, {"energy": 1}, 0, torch.float32)
    model = rt.HipModel(hypers, types)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    train = TrainStep(model, {"warmup_fraction": 0.0, "num_epochs": 10**6})
    gen = torch.Generator().manual_seed(1234)
    result = {"workload": "default PET, training step (energy + force loss, Adam); the batch collated once and augmented every "
                          "step against collating every step, arms alternating in one process (ms, host clock)",
              "steps": args.steps, "warmup": args.warmup, "micro_batches_per_step": args.micro}

    for size in args.sizes.split(","):
        boxes, atoms = (int(x) for x in size.split("x"))
        per = (boxes + args.micro - 1) // args.micro
        micro_systems, micro_targets = [], []
        for m0 in range(0, boxes, per):
            systems, energies, forces = [], [], []
            for seed in range(m0, min(boxes, m0 + per)):
                pos, z, cell = random_box(atoms, seed=seed)
                systems.append((pos.to(dev), z.to(dev), cell, [True] * 3))
                energies.append((torch.randn(1, generator=gen) * 0.1 * atoms).to(dev))
                forces.append((torch.randn(atoms, 3, generator=gen) * 0.1).to(dev))
            micro_systems.append(systems)
            micro_targets.append({"energy": energies, "forces": forces})

        def collate(k):
            return data.collate(micro_systems[k], cutoff, micro_targets[k])

        cached = [collate(k) for k in range(len(micro_systems))]
        aug = O3Augmenter({"energy": "scalar", "forces": "vector"}, seed=1)
        n_atoms = [torch.full((len(s),), float(atoms), device=dev) for s in micro_systems]
        state = {"fw": rt.HipForward(model, data.graph_of(model, max(cached, key=lambda b: b["centers"].numel())), train=True)}

        def step(batches):
            """One optimizer step over the micro-batches, graphs built from the batches' pair lists."""
            args_l = []
            for k, b in enumerate(batches):
                graph = data.graph_of(model, b)
                try:
                    state["fw"].rebind(graph)
                except PetHipError:  # a pair at the cutoff kept after the rotation: a few more edges than the workspace was sized for
                    state["fw"] = rt.HipForward(model, graph, train=True)
                args_l.append(dict(graph=graph, fw=state["fw"], target_energies=b["energy"], n_atoms=n_atoms[k],
                                   target_gradients=-b["forces"]))
            return train.microbatched(args_l) if len(args_l) > 1 else train(
                args_l[0]["graph"], args_l[0]["fw"], args_l[0]["target_energies"], args_l[0]["n_atoms"], args_l[0]["target_gradients"])

        def step_cached():
            return step([aug.apply_random_augmentations(b) for b in cached])

        def step_recollate():
            return step([collate(k) for k in range(len(micro_systems))])

        # (a) and (b): per optimizer step, i.e. over all micro-batches
        mats = [rt.o3_draw(len(s), aug.key, 0, "O3", dev) for s in micro_systems]
        cell_rows = [torch.arange(3 * len(s), dtype=torch.int32, device=dev) // 3 for s in micro_systems]

        def apply_only():
            for k, b in enumerate(cached):
                rt.o3_apply(mats[k], [(b["positions"], "vector", b["system_indices"]),
                                      (b["cells"].reshape(-1, 3), "vector", cell_rows[k]),
                                      (b["forces"], "vector", b["system_indices"])])

        a_ms, a_all, a_enq = _timed(lambda: [aug.apply_random_augmentations(b) for b in cached], args.warmup, args.steps, args.inner)
        d_ms, _, d_enq = _timed(lambda: [rt.o3_draw(len(s), aug.key, 0, "O3", dev) for s in micro_systems], args.warmup, args.steps,
                                args.inner)
        p_ms, _, p_enq = _timed(apply_only, args.warmup, args.steps, args.inner)
        c_ms, c_all, _ = _timed(lambda: [collate(k) for k in range(len(micro_systems))], args.warmup, args.steps)

        # (c): the arms alternate
        for _ in range(args.warmup):
            step_cached()
            step_recollate()
        times = {"cached_augmented": [], "recollated": []}
        losses = []
        for _ in range(args.steps):
            for name, fn in (("cached_augmented", step_cached), ("recollated", step_recollate)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
                losses.append(float(out["loss"]))
        assert all(x == x for x in losses), "training diverged to NaN"
        med = {k: _median(v) for k, v in times.items()}
        result[f"batch_{boxes}x{atoms}"] = {
            "boxes": boxes, "atoms_per_box": atoms, "pairs": int(sum(b["centers"].numel() for b in cached)),
            "augment_ms_per_step": {"call": a_ms, "draw_alone": d_ms, "apply_alone": p_ms,
                                    "enqueue": {"call": a_enq, "draw_alone": d_enq, "apply_alone": p_enq},
                                    "launches": 2 * len(cached), "calls_per_sample": args.inner, "all": a_all},
            "collate_ms_per_step": {"median": c_ms, "all": c_all},
            "train_step_ms": {"median": med, "all": times},
            "recollated_over_cached_augmented": med["recollated"] / med["cached_augmented"],
            "augment_share_of_step": a_ms / med["cached_augmented"],
        }
        del cached, state, micro_systems, micro_targets, mats
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
