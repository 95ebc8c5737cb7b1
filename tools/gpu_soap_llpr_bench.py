"""Cost of the SOAP-BPNN LLPR outputs on the 100 000-atom box of ``bench_soap.py`` (default legacy model, four types, F = 128):
``SoapBpnnHip.evaluate`` alone (forward + dE/dR, the baseline on the same commit), then ``evaluate`` plus a per-system
``energy_uncertainty``, plus a per-atom ``energy_uncertainty``, plus a K = 128 per-system ``energy_ensemble`` -- the four taken in
turn, one each per round, each timed by a host clock between device synchronisations. The graph is built once outside the timed
steps. Then the pieces alone: ``soap_llpr_features`` against a device copy of as many bytes as it moves in the same run (its
distance from the memory roof), the per-system rows, sigma, the ensemble, and covariance accumulation over 64 batches of 1 000
atoms (``compute_covariance``). Prints one JSON line.

  python tools/gpu_soap_llpr_bench.py --atoms 100000 --rounds 10 --warmup 2 --out profiles/soap_llpr_bench.json
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench_params(model, hypers, alchemical=False):
    """The random weights of bench_soap.py."""
    S, H = model.feature_size, hypers["bpnn"]["num_neurons_per_layer"]
    gen = torch.Generator().manual_seed(0)
    params = {}
    if alchemical:
        params["species_embedding.weight"] = torch.randn(4, 4, generator=gen)
        params["center_encoding.weight"] = torch.randn(4, S, generator=gen)
    for s in range(1 if alchemical else 4):
        params[f"layernorm.{s}.weight"] = 1 + 0.1 * torch.randn(S, generator=gen)
        params[f"layernorm.{s}.bias"] = 0.1 * torch.randn(S, generator=gen)
        params[f"bpnn.{s}.0.weight"] = torch.randn(H, S, generator=gen) / S**0.5
        params[f"bpnn.{s}.2.weight"] = torch.randn(H, H, generator=gen) / H**0.5
        params[f"last_layers.energy.{s}.weight"] = torch.randn(1, H, generator=gen) / H**0.5
    return params


def box_graph(model, rt, n, seed, dev):
    from metatrain_amd.synthetic import random_box

    pos, z, cell = random_box(n, seed=seed)
    posd = pos.to(dev)
    pairs, _ = rt.neighbor_list(posd, cell, [True] * 3, model.cutoff)
    return model.graph(posd, cell[None].to(dev), pairs[:, 0].contiguous(), pairs[:, 1].contiguous(),
                       pairs[:, 2:5].contiguous(), z.to(dev), torch.zeros(n, dtype=torch.int32, device=dev))


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def median(t):
    return sorted(t)[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--members", type=int, default=128)
    ap.add_argument("--cov-batches", type=int, default=64)
    ap.add_argument("--cov-atoms", type=int, default=1000)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_soap_llpr_bench.py needs an MI355X"

    from metatrain_amd import runtime as rt
    from metatrain_amd._lib import check
    from metatrain_amd.soap_bpnn import SoapBpnnHip, SoapLLPRUncertainty, default_hypers

    dev = torch.device("cuda:0")
    hypers = default_hypers()
    hypers["legacy"] = True
    model = SoapBpnnHip(hypers, [1, 6, 7, 8])
    params = {k: v.to(dev) for k, v in bench_params(model, hypers).items()}
    model.load(params)
    g = box_graph(model, rt, args.atoms, 0, dev)
    train = [box_graph(model, rt, args.cov_atoms, 100 + b, dev) for b in range(args.cov_batches)]

    u = SoapLLPRUncertainty(model, params, sample_kind="system", num_ensemble_members=args.members)
    u.compute_covariance(train)
    u.compute_cholesky_decomposition()
    u.generate_ensemble(torch.Generator().manual_seed(0))
    grads = {"energy": ["positions"]}
    cases = {
        "with_system_uncertainty": {"energy": "system", "energy_uncertainty": "system"},
        "with_atom_uncertainty": {"energy": "atom", "energy_uncertainty": "atom"},
        "with_ensemble": {"energy": "system", "energy_ensemble": "system"},
    }
    names = ["evaluate", *cases]

    def one(case):
        if case == "evaluate":
            return model.evaluate(g)
        return u.forward(g, cases[case], explicit_gradients=grads)

    for _ in range(args.warmup):
        for c in names:
            one(c)
    times = {c: [] for c in names}
    for _ in range(args.rounds):
        for c in names:
            times[c] += timed(lambda: one(c), 1)
    med = {c: median(t) for c, t in times.items()}

    # the pieces alone
    model.forward(g)
    llf = model.last_layer_features(g)
    ws, N, F, H = model._workspace(g), g.n_nodes, u.F, hypers["bpnn"]["num_neurons_per_layer"]
    rows = u.rows(g, llf, mean=False)
    inv = u._inverse_cholesky()
    W = u.buffers["llpr_ensemble_layers.energy.weight"]
    pred = torch.zeros(g.n_systems, 1, device=dev)
    moved = N * (H + F) * 4 + N * 4  # the activations read, the array written, the species index
    src, dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)

    def features_kernel():
        check(model.lib.soap_llpr_features(model._handle, g.handle, rt._ptr(ws), ws.numel(), 0, rt._ptr(llf), rt._stream()))

    reps = 50

    def many(fn):
        def run():
            for _ in range(reps):
                fn()
        return run

    pieces = {
        f"soap_llpr_features_x{reps}": many(features_kernel),
        f"device_copy_same_bytes_x{reps}": many(lambda: dst.copy_(src)),
        "rows_system": lambda: u.rows(g, llf, mean=False),
        "sigma_system": lambda: u.sigma(rows, inv),
        "sigma_atom": lambda: u.sigma(llf, inv),
        "ensemble_system": lambda: u.ensemble(rows, W, args.members, pred),
        "compute_covariance": lambda: u.compute_covariance(train),
    }
    piece_ms = {}
    for k, fn in pieces.items():
        timed(fn, 2)
        piece_ms[k] = median(timed(fn, args.rounds))
    feat_ms = piece_ms[f"soap_llpr_features_x{reps}"] / reps
    copy_ms = piece_ms[f"device_copy_same_bytes_x{reps}"] / reps
    base = med["evaluate"]
    line = json.dumps({
        "workload": f"SOAP-BPNN legacy default, one {args.atoms}-atom box ({int(g.n_edges)} pairs), F = {F}; graph built "
                    "outside the timed steps",
        "ms_per_step_median": med,
        "ratio_to_evaluate": {c: med[c] / base for c in names if c != "evaluate"},
        "pieces_ms_median": piece_ms,
        "soap_llpr_features": {"bytes_moved": moved, "ms": feat_ms, "gb_per_s": moved / (feat_ms * 1e-3) / 1e9,
                               "device_copy_ms": copy_ms, "device_copy_gb_per_s": moved / (copy_ms * 1e-3) / 1e9,
                               "fraction_of_copy_bandwidth": copy_ms / feat_ms,
                               "note": f"{reps} back-to-back launches per timed window; the copy reads and writes "
                                       "bytes_moved / 2 each"},
        "compute_covariance": {"batches": args.cov_batches, "atoms_per_batch": args.cov_atoms,
                               "ms": piece_ms["compute_covariance"],
                               "includes": "forward, last-layer features, per-system rows and accumulation per batch"},
        "ms_per_step_all": times,
    })
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
