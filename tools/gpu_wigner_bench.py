"""Rotational augmentation of spherical targets, measured on the 64 x 1 000 atom training workload (default PET, energy +
force loss, Adam). The cached batch carries, next to energy and forces, one per-atom target of 16 properties with the blocks
``o3_lambda = 0, 1, 2, 3`` and one per-system ``o3_lambda = 8`` block:

  (a) the two launches a spherical kind adds, alone: ``runtime.o3_wigner`` (tables up to ``l = 8``) and
      ``runtime.o3_apply_spherical`` (the four arrays that are not invariants), next to the Cartesian ``runtime.o3_apply`` of
      positions, cells and forces on the same batch; device times from the library's event brackets
      (``runtime.profile``), host-clock medians beside them;
  (b) one optimizer step with the batch augmented EVERY step (spherical targets included) against the same step on a batch
      transformed once; the two arms alternate in one process. ``TrainStep`` trains energy and forces; the spherical targets
      ride along, which is what the augmentation costs a loop whatever head consumes them.

A step walks its boxes in ``--micro`` micro-batches, as ``tools/gpu_augment_bench.py``. Medians over ``--steps`` samples
after ``--warmup``. Prints one JSON line.

  python tools/gpu_wigner_bench.py --steps 7 --warmup 3
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROPERTIES = 16


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def _timed(fn, warmup, steps, inner=1):
    for _ in range(warmup):
        fn()
    total = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        total.append((time.perf_counter() - t0) * 1e3 / inner)
    return _median(total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--micro", type=int, default=2, help="micro-batches per optimizer step")
    ap.add_argument("--inner", type=int, default=20, help="calls per timed sample of (a)")
    ap.add_argument("--boxes", type=int, default=64)
    ap.add_argument("--atoms", type=int, default=1000)
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
    boxes, atoms = args.boxes, args.atoms
    kinds = {"energy": "scalar", "forces": "vector", "big": {"kind": "spherical", "o3_lambda": 8, "o3_sigma": 1}}
    kinds.update({f"atomic_l{l}": {"kind": "spherical", "o3_lambda": l, "o3_sigma": 1} for l in range(4)})

    per = (boxes + args.micro - 1) // args.micro
    cached, n_atoms = [], []
    for m0 in range(0, boxes, per):
        systems, targets = [], {name: [] for name in kinds}
        for seed in range(m0, min(boxes, m0 + per)):
            pos, z, cell = random_box(atoms, seed=seed)
            systems.append((pos.to(dev), z.to(dev), cell, [True] * 3))
            targets["energy"].append((torch.randn(1, generator=gen) * 0.1 * atoms).to(dev))
            targets["forces"].append((torch.randn(atoms, 3, generator=gen) * 0.1).to(dev))
            targets["big"].append(torch.randn(1, 17, 1, generator=gen).to(dev))
            for l in range(4):
                targets[f"atomic_l{l}"].append(torch.randn(atoms, 2 * l + 1, PROPERTIES, generator=gen).to(dev))
        cached.append(data.collate(systems, cutoff, targets))
        n_atoms.append(torch.full((len(systems),), float(atoms), device=dev))
    aug = O3Augmenter(kinds, seed=1)
    state = {"fw": rt.HipForward(model, data.graph_of(model, max(cached, key=lambda b: b["centers"].numel())), train=True)}

    def step(batches):
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

    once = [aug.apply_random_augmentations(b) for b in cached]

    # (a) the launches alone, per optimizer step (all micro-batches)
    mats = [b["o3_matrices"] for b in once]
    tables = [rt.o3_wigner(m, 8) for m in mats]
    cell_rows = [torch.arange(3 * m.shape[0], dtype=torch.int32, device=dev) // 3 for m in mats]

    def wigner_only():
        for m in mats:
            rt.o3_wigner(m, 8)

    def spherical_only():
        for b, (t, p) in zip(cached, tables):
            rt.o3_apply_spherical(t, p, 8, [(b[f"atomic_l{l}"], l, 1, b["system_indices"]) for l in (1, 2, 3)] + [(b["big"], 8, 1, None)])

    def cartesian_only():
        for k, b in enumerate(cached):
            rt.o3_apply(mats[k], [(b["positions"], "vector", b["system_indices"]), (b["cells"].reshape(-1, 3), "vector", cell_rows[k]),
                                  (b["forces"], "vector", b["system_indices"])])

    def call():
        for b in cached:
            aug.apply_random_augmentations(b)

    host = {name: _timed(fn, args.warmup, args.steps, args.inner)
            for name, fn in (("wigner", wigner_only), ("apply_spherical", spherical_only), ("apply_cartesian", cartesian_only), ("call", call))}
    rt.profile(True)
    for _ in range(args.inner):
        call()
    torch.cuda.synchronize()
    device = {r["name"]: {"ms_per_step": r["total_ms"] / args.inner, "launches_per_step": r["calls"] / args.inner,
                          "GB_per_s": r["bytes"] / max(r["total_ms"], 1e-9) * 1e-6} for r in rt.profile_report()}
    rt.profile(False)

    # (b) the arms alternate
    def step_every():
        return step([aug.apply_random_augmentations(b) for b in cached])

    def step_once():
        return step(once)

    for _ in range(args.warmup):
        step_every()
        step_once()
    times = {"augmented_every_step": [], "transformed_once": []}
    losses = []
    for _ in range(args.steps):
        for name, fn in (("augmented_every_step", step_every), ("transformed_once", step_once)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            losses.append(float(out["loss"]))
    assert all(x == x for x in losses), "training diverged to NaN"
    med = {k: _median(v) for k, v in times.items()}
    print(json.dumps({
        "workload": f"default PET, training step (energy + force loss, Adam), {boxes} x {atoms} atoms in {len(cached)} micro-batches; "
                    f"per-atom spherical target l = 0..3 x {PROPERTIES} properties, per-system l = 8 block",
        "steps": args.steps, "warmup": args.warmup, "calls_per_sample": args.inner,
        "launches_device_ms": device, "host_ms_per_step": host,
        "train_step_ms": {"median": med, "all": times},
        "augmented_every_step_over_transformed_once": med["augmented_every_step"] / med["transformed_once"],
    }))


if __name__ == "__main__":
    main()
