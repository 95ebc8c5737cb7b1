"""Cost of the SOAP-BPNN Hessian-vector product (``soap_hessian_vector``) and of the stress term of its training step, on one
periodic box of 1 000 and of 10 000 atoms (default hypers, four atomic types):

* ``hvp``: one product behind a forward that has already run (what a Lanczos or dimer iteration pays per direction);
* ``fwd_bwd``: ``forward + backward`` of the same graph, one energy + forces evaluation -- a central difference of the forces
  along ``u`` costs two of these;
* ``train_gradients``: the training pass's second-order sweep ``soap_train_gradients`` with force seeds, which computes the
  same tangent sweep and tail plus every parameter gradient, but not the last stage to the pair vectors;
* ``step`` / ``step_strain``: one ``SoapTrainStep`` on energies and forces, without and with a strain target.

Within one process the arms alternate after the warm-up, each timed by a host clock between two device synchronisations;
each figure is the median of ``--rounds`` (20) after ``--warmup`` (5). Nothing is asserted: the pass is per-atom workgroups,
correctness first, and the numbers are recorded. ``--accuracy-log`` takes the output of
``pytest -s tests/test_gpu_soap_hvp.py`` and records its ``(case, y, relmax)`` lines.

The driver itself does not touch the GPU: every box is a child process under its own time limit, and the first failure ends
the run.

  python tools/gpu_soap_hvp_bench.py --out profiles/soap_hvp_bench.json [--accuracy-log FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(args):
    import torch

    from metatrain_amd import runtime as rt
    from metatrain_amd.soap_bpnn import SoapBpnnHip, SoapTrainStep, default_hypers
    from metatrain_amd.synthetic import random_box
    from oracle import soap as osoap

    dev = torch.device("cuda:0")
    types = [1, 6, 7, 8]
    hypers = default_hypers()
    model = SoapBpnnHip(hypers, types)
    n_per_l = osoap.basis(hypers)[0]
    model.load({k: v.to(dev) for k, v in osoap.synthetic_params(hypers, len(types), n_per_l, 1, torch.float32).items()})
    pos, z, cell = random_box(args.atoms, seed=0)
    posd, cells = pos.to(dev), cell[None].to(dev)
    pairs, _ = rt.neighbor_list(posd, cell, [True] * 3, model.cutoff)
    graph = model.graph(posd, cells, pairs[:, 0].contiguous(), pairs[:, 1].contiguous(), pairs[:, 2:5].contiguous(), z.to(dev),
                        torch.zeros(args.atoms, dtype=torch.int32, device=dev))
    n = graph.n_nodes
    gen = torch.Generator().manual_seed(1)
    u = torch.randn(n, 3, generator=gen).to(dev)
    seeds = (torch.randn(n, generator=gen) * 0.01).to(dev)
    te, tg, ts = torch.zeros(1, device=dev), (torch.randn(n, 3, generator=gen) * 0.3).to(dev), torch.randn(1, 3, 3, generator=gen).to(dev)
    n_atoms = torch.full((1,), float(n), device=dev)
    step = SoapTrainStep(model, {"learning_rate": 0.0})  # the timing must not walk the parameters away
    model.zero_grad()
    ones = torch.ones(n, device=dev)

    def hvp():
        model.hessian_vector_product(graph, u)

    def fwd_bwd():
        model.backward(graph, torch.ones_like(model.forward(graph)))

    def train_gradients():
        model.train_gradients(graph, seeds, u)

    def step_plain():
        step(graph, te, n_atoms, tg)

    def step_strain():
        step(graph, te, n_atoms, tg, target_strain_gradients=ts, positions=posd, cells=cells)

    def prepared(fn):  # hvp and train_gradients read the forward of this graph: restore it outside the clock
        def run():
            model.forward(graph)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        return run

    def plain(fn):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        return run

    arms = {"hvp": prepared(hvp), "fwd_bwd": plain(fwd_bwd), "train_gradients": prepared(train_gradients),
            "step": plain(step_plain), "step_strain": plain(step_strain)}
    for _ in range(args.warmup):
        for fn in arms.values():
            fn()
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            times[k].append(fn())
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(json.dumps({"atoms": n, "graph_edges": graph.n_edges,
                      "hvp_workspace_bytes": int(model.lib.soap_hvp_workspace_bytes(model._handle, n, graph.n_edges)),
                      "ms_median": med, "hvp_over_fwd_bwd": med["hvp"] / med["fwd_bwd"],
                      "hvp_over_train_gradients": med["hvp"] / med["train_gradients"],
                      "step_strain_over_step": med["step_strain"] / med["step"], "ms_all": times}))


def run(cmd, limit):
    cmd = ["timeout", "-k", "10", str(limit)] + cmd
    print("+", " ".join(cmd), flush=True)
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"step failed with exit status {p.returncode}: nothing more is started")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def accuracy(path):
    with open(path) as fh:
        return [ln.strip().lstrip(".") for ln in fh if ln.lstrip(".").startswith(("soap hvp ", "soap dense Hessian", "soap stress "))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soap_hvp_bench.json"))
    ap.add_argument("--accuracy-log")
    ap.add_argument("--atoms", type=int, default=0)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    out = {"what": "SOAP-BPNN Hessian-vector product and stress term; ms, median of %d after %d warm-up; host clock between two "
                   "device synchronisations, arms alternating in one process" % (args.rounds, args.warmup), "boxes": {}}
    for atoms in args.sizes:
        out["boxes"][str(atoms)] = run([sys.executable, os.path.abspath(__file__), "--worker", "--atoms", str(atoms), "--rounds",
                                        str(args.rounds), "--warmup", str(args.warmup)], args.limit)
    if args.accuracy_log:
        out["accuracy"] = accuracy(args.accuracy_log)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: {a: b for a, b in v.items() if a != "ms_all"} for k, v in out["boxes"].items()}))


if __name__ == "__main__":
    main()
