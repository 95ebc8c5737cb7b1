"""Cost of the LLPR outputs on the inference step, on the bench batch (8 boxes of 10 000 atoms, default model): the plain
fused step (``HipForward`` forward + backward, what bench.py times), energy + forces through ``LLPRUncertainty.forward``
(no LLF pass), the same with ``energy_uncertainty``, and the same with a 128-member ``energy_ensemble``, the four steps taken
in turn, one each per round. The LLPR share is then broken down by timing its pieces alone on the same batch: the backbone
forward with feature copies, ``pet_llpr_features`` (heads recomputed, LLF packed), the per-system rows, sigma, the ensemble.
Also the covariance kernel alone on the per-atom rows of one 10 000-atom box (LPR rows, R = 10 000, F = 256: 2 R F^2 algorithmic FLOPs counted in full, though only the upper triangle of tiles is computed) against
the 155 TFLOP/s fp32 matrix peak. Prints one JSON line.

  python tools/gpu_llpr_bench.py --boxes 8 --atoms 10000 --rounds 10 --warmup 2 --out profiles/llpr_bench.json
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
    ap.add_argument("--boxes", type=int, default=8)
    ap.add_argument("--atoms", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--members", type=int, default=128)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    from metatrain_amd import runtime as rt
    from metatrain_amd.pet import default_hypers
    from metatrain_amd.pet.llpr import LLPRUncertainty
    from metatrain_amd.synthetic import random_box, synthetic_params

    dev = torch.device("cuda:0")
    types = [1, 6, 7, 8]
    hypers = dict(default_hypers())
    params = {k: v.to(dev) for k, v in synthetic_params(hypers, types, {"energy": 1}, 0, torch.float32).items()}
    model = rt.HipModel(hypers, types)
    model.load(params, "energy")
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
    graph = rt.HipGraph(model, torch.cat(pos_l), torch.stack(cell_l), pairs[:, 0].contiguous(), pairs[:, 1].contiguous(),
                        pairs[:, 2:5].contiguous(), torch.cat(z_l), torch.cat(sys_l))

    u = LLPRUncertainty(model, params, {"energy": "system"}, num_ensemble_members={"energy": args.members})
    u.compute_covariance([graph])
    u.compute_cholesky_decomposition()
    u.generate_ensemble(torch.Generator().manual_seed(0))
    grads = {"energy": ["positions"]}
    cases = {
        "energy_forces_llpr_wrapper": {"energy": "system"},
        "with_uncertainty": {"energy": "system", "energy_uncertainty": "system"},
        "with_ensemble": {"energy": "system", "energy_uncertainty": "system", "energy_ensemble": "system"},
    }
    fw0 = rt.HipForward(model, graph)
    ones = torch.ones(graph.n_nodes, device=dev)

    def one(case):
        if case == "plain_fused":
            fw0.forward()
            return fw0.backward(ones)
        return u.forward(graph, cases[case], explicit_gradients=grads)

    names = ["plain_fused", *cases]
    for _ in range(args.warmup):
        for c in names:
            one(c)
    torch.cuda.synchronize()

    def timed(fn, reps):
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    times = {c: [] for c in names}
    for _ in range(args.rounds):
        for c in names:
            times[c] += timed(lambda: one(c), 1)
    med = {c: sorted(t)[len(t) // 2] for c, t in times.items()}

    # the pieces alone (medians of `rounds` repetitions each)
    fw1 = rt.HipForward(model, graph)
    _, nf, ef = fw1.forward(want_features=True)
    _, llf_all = u.features(graph, fw1, ["energy"], feats=([nf], [ef]))["energy"]
    rows = u.rows(graph, llf_all, mean=False)
    inv = u._inverse_cholesky("energy")
    W = u.buffers["llpr_ensemble_layers.energy.weight"]
    pred = torch.zeros(graph.n_systems, 1, device=dev)
    pieces = {
        "forward_plain": lambda: fw1.forward(),
        "forward_with_feature_copies": lambda: fw1.forward(want_features=True),
        "llpr_features": lambda: u.features(graph, fw1, ["energy"], feats=([nf], [ef])),
        "rows": lambda: u.rows(graph, llf_all, mean=False),
        "variance": lambda: u.sigma(rows, inv),
        "ensemble": lambda: u.ensemble(rows, W, args.members, pred),
    }
    piece_ms = {}
    for k, fn in pieces.items():
        timed(fn, 2)
        t = timed(fn, args.rounds)
        piece_ms[k] = sorted(t)[len(t) // 2]

    # covariance kernel alone: per-atom rows of one box
    fw = rt.HipForward(model, graph)
    _, llf = u.features(graph, fw, ["energy"])["energy"]
    x = llf[: args.atoms].contiguous()
    C = torch.zeros((u.F, u.F), dtype=torch.float64, device=dev)
    for _ in range(3):
        u.accumulate(x, C)
    torch.cuda.synchronize()
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        u.accumulate(x, C)
    torch.cuda.synchronize()
    cov_ms = (time.perf_counter() - t0) * 1e3 / reps
    tflops = 2.0 * x.shape[0] * u.F * u.F / (cov_ms * 1e-3) / 1e12
    base = med["plain_fused"]
    line = json.dumps({
        "workload": f"{args.boxes} x {args.atoms} atoms, default PET, inference step (energy + forces)",
        "ms_per_step_median": med,
        "overhead_pct_vs_plain_fused": {c: 100.0 * (med[c] / base - 1.0) for c in names if c != "plain_fused"},
        "pieces_ms_median": piece_ms,
        "covariance_per_atom_rows": {"R": int(x.shape[0]), "F": u.F, "ms": cov_ms, "tflops": tflops,
                                     "fraction_of_155tf_peak": tflops / 155.0},
        "ms_per_step_all": times,
    })
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
