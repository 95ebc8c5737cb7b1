"""Composition baseline and target scale on the device, measured on the training workload of ``bench_train.py``'s default
configuration (64 boxes of 1 000 atoms, default PET, energy + force loss, Adam; raw fp64 energies near -1e6 eV per box and
fp64 dE/dR targets in the cached batches):

  (a) fitting: ``CompositionHip.accumulate`` over the training set and ``fit``, then ``ScalerHip.accumulate`` (the residual
      formed on the fly from the fitted weights) and ``fit`` -- what runs once before the first optimizer step;
  (b) one optimizer step that applies ``TargetTransform`` to its cached batches every step (composition and scale removed
      from the energies, the scale from the gradients, one read-back of the error flag per batch) against a step on targets
      transformed once beforehand. The two arms alternate in one process, as for every A/B number of this repository.

A step walks its boxes in ``--micro`` micro-batches (``TrainStep.microbatched``; default: two). Times are host clocks around
work that ends in a device synchronisation, medians over ``--steps`` samples after ``--warmup``. Writes one JSON object to
``--out`` (default ``profiles/baseline_bench.json``) and prints it.

  python tools/gpu_baseline_bench.py --steps 7 --warmup 2
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def _timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return _median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--micro", type=int, default=2, help="micro-batches per optimizer step")
    ap.add_argument("--boxes", type=int, default=64)
    ap.add_argument("--atoms", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "baseline_bench.json"))
    args = ap.parse_args()

    from metatrain_amd import data
    from metatrain_amd import runtime as rt
    from metatrain_amd.baseline import CompositionHip, ScalerHip, TargetTransform
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
    per_species = {1: -13.6, 6: -1029.5, 7: -1485.3, 8: -2042.6}  # eV per atom, the size of raw DFT energies

    boxes, atoms = args.boxes, args.atoms
    per = (boxes + args.micro - 1) // args.micro
    cached = []
    for m0 in range(0, boxes, per):
        systems, energies, gradients = [], [], []
        for seed in range(m0, min(boxes, m0 + per)):
            pos, z, cell = random_box(atoms, seed=seed)
            systems.append((pos.to(dev), z.to(dev), cell, [True] * 3))
            base = sum(per_species[int(v)] for v in z.tolist())
            energies.append((torch.tensor([base], dtype=torch.float64) + torch.randn(1, generator=gen).double() * 0.05 * atoms).to(dev))
            gradients.append((torch.randn(atoms, 3, generator=gen).double() * 0.5).to(dev))
        cached.append(data.collate(systems, cutoff, {"energy": energies, "dE_dR": gradients}))
        del systems

    spec = {"energy": {"per_atom": False, "shape": [1]}}
    fitted = {}

    def fit_composition():
        comp = CompositionHip(types, spec)
        for b in cached:
            comp.accumulate(b)
        comp.fit()
        fitted["comp"] = comp

    def fit_scaler():
        sc = ScalerHip(types, spec)
        for b in cached:
            sc.accumulate(b, composition=fitted["comp"])
        sc.fit()
        fitted["sc"] = sc

    fc_ms, fc_all = _timed(fit_composition, args.warmup, args.steps)
    fs_ms, fs_all = _timed(fit_scaler, args.warmup, args.steps)
    comp, sc = fitted["comp"], fitted["sc"]
    transform = TargetTransform(comp, sc)
    names = {"energies": "energy", "gradients": "dE_dR"}
    t_ms, t_all = _timed(lambda: [transform(b, names) for b in cached], args.warmup, args.steps)

    graphs = [data.graph_of(model, b) for b in cached]
    fw = rt.HipForward(model, max(graphs, key=lambda g: g.n_edges), train=True)
    once = [transform(b, names) for b in cached]

    def step(targets):
        args_l = [dict(graph=g, fw=fw, target_energies=t["target_energies"], n_atoms=t["n_atoms"],
                       target_gradients=t["target_gradients"]) for g, t in zip(graphs, targets)]
        if len(args_l) > 1:
            return train.microbatched(args_l)
        a = args_l[0]
        return train(a["graph"], a["fw"], a["target_energies"], a["n_atoms"], a["target_gradients"])

    arms = (("transform_every_step", lambda: step([transform(b, names) for b in cached])), ("transformed_once", lambda: step(once)))
    for _ in range(args.warmup):
        for _, fn in arms:
            fn()
    times = {name: [] for name, _ in arms}
    losses = []
    for _ in range(args.steps):
        for name, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            losses.append(float(out["loss"]))
    assert all(x == x for x in losses), "training diverged to NaN"
    med = {k: _median(v) for k, v in times.items()}
    result = {
        "workload": f"default PET, {boxes} boxes x {atoms} atoms in {len(cached)} micro-batches, raw fp64 energies and dE/dR; "
                    "fit of the composition baseline and the target scale, and a training step (energy + force loss, Adam) "
                    "with TargetTransform applied every step against targets transformed once, arms alternating (ms, host clock)",
        "steps": args.steps, "warmup": args.warmup, "boxes": boxes, "atoms_per_box": atoms, "micro_batches_per_step": len(cached),
        "fit_ms": {"composition_accumulate_and_fit": fc_ms, "scaler_accumulate_and_fit": fs_ms, "total": fc_ms + fs_ms,
                   "all": {"composition": fc_all, "scaler": fs_all}},
        "fitted": {"weights_eV": comp.weights("energy")[:, 0].tolist(), "scale": sc.scale("energy")},
        "transform_ms_per_step": {"median": t_ms, "all": t_all},
        "train_step_ms": {"median": med, "all": times},
        "transform_every_step_over_transformed_once": med["transform_every_step"] / med["transformed_once"],
    }
    text = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
