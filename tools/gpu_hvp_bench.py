"""Cost of one Hessian-vector product (``pet_hessian_vector``) on one 1 000-atom box, for the default PET model and for
``d_pet = 64``, against its two alternatives on the same model and graph:

* ``fd``: two energy + forces evaluations (``HipForward`` forward + backward twice), what a central difference of the
  forces along ``u`` costs -- the default size runs its tuned inference kernels there, the Hessian-vector product the
  size-generic dual pass;
* ``train2``: this build's second-order training sweep ``pet_backward_train2`` alone (after one training forward and
  ``pet_backward``), which computes the same dual forward and reverse sweep plus every parameter gradient -- for the default
  size on the tuned second-order kernels.

Within one process the arms alternate after a warm-up, each timed by a host clock between two device synchronisations;
what counts is the ratio of the medians in the same run. There is no speed bar: the size-generic pass is correctness-first.
``--accuracy-log`` takes the output of ``pytest -s tests/test_gpu_hvp.py`` and records its ``(case, y, relmax)`` lines.

``--zbl`` measures the ZBL arm instead (``profiles/zbl_hvp_bench.json``): on the same box, default model, ``pet_hessian_vector``
alone against ``pet_hessian_vector`` + ``pet_zbl_hessian_vector`` on the same graph, what ``hessian(..., zbl=table)`` and the
exported op of a ``zbl: true`` model run per product; ``--accuracy-log`` then takes ``pytest -s tests/test_gpu_zbl_hvp.py``, and
``--bench-log`` a file of ``bench.py`` result lines, each prefixed ``parent `` or ``this `` (the inference step of the two
commits, alternating), whose medians are recorded beside it.

The driver itself does not touch the GPU: every model is a child process under its own time limit, and the first failure
ends the run.

  python tools/gpu_hvp_bench.py --out profiles/hvp_bench.json [--accuracy-log FILE]
  python tools/gpu_hvp_bench.py --zbl [--accuracy-log FILE] [--bench-log FILE]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODELS = {"default": {}, "d_pet_64": dict(d_pet=64, d_node=128, d_feedforward=128, d_head=64, num_heads=4)}


def worker(args):
    import torch

    from metatrain_amd import runtime as rt
    from metatrain_amd.pet import default_hypers
    from metatrain_amd.synthetic import random_box, synthetic_params

    dev = torch.device("cuda:0")
    types = [1, 6, 7, 8]
    hypers = dict(default_hypers(), **MODELS[args.worker])
    model = rt.HipModel(hypers, types)
    model.load({k: v.to(dev) for k, v in synthetic_params(hypers, types, {"energy": 1}, 0, torch.float32).items()}, "energy")
    pos, z, cell = random_box(args.atoms, seed=0)
    posd = pos.to(dev)
    pairs, _ = rt.neighbor_list(posd, cell, [True] * 3, hypers["cutoff"])
    graph = rt.HipGraph(model, posd, cell[None].to(dev), pairs[:, 0].contiguous(), pairs[:, 1].contiguous(),
                        pairs[:, 2:5].contiguous(), z.to(dev), torch.zeros(args.atoms, dtype=torch.int32, device=dev))
    n = graph.n_nodes
    u = torch.randn(n, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    ones = torch.ones(n, device=dev)
    ws = torch.empty(rt.hvp_workspace_bytes(model, graph), dtype=torch.uint8, device=dev)
    inf = rt.HipForward(model, graph)
    tr = rt.HipForward(model, graph, train=True)
    model.zero_grad()
    tr.forward()
    tr.backward(ones)

    def hvp():
        rt.hessian_vector_product(model, graph, u, workspace=ws)

    def fd():
        for _ in range(2):
            inf.forward()
            inf.backward(ones)

    def train2():
        tr.backward_train2(ones, None, u)

    arms = {"hvp": hvp, "fd": fd, "train2": train2}
    if args.zbl:
        from metatrain_amd.zbl import ZBLHip

        table = ZBLHip(types)
        touched = int((table.forward(graph) != 0).sum())

        def hvp_zbl():
            rt.hessian_vector_product(model, graph, u, workspace=ws) + table.hessian_vector_product(graph, u)

        arms = {"hvp": hvp, "hvp_zbl": hvp_zbl}
    for _ in range(args.warmup):
        for fn in arms.values():
            fn()
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    if args.zbl:
        print(json.dumps({"atoms": n, "graph_edges": graph.n_edges, "atoms_with_a_zbl_energy": touched, "ms_median": med,
                          "hvp_zbl_over_hvp": med["hvp_zbl"] / med["hvp"], "ms_all": times}))
        return
    print(json.dumps({"atoms": n, "graph_edges": graph.n_edges, "hvp_workspace_bytes": int(ws.numel()),
                      "ms_median": med, "hvp_over_fd": med["hvp"] / med["fd"], "hvp_over_train2": med["hvp"] / med["train2"],
                      "ms_all": times}))


def run(cmd, limit):
    cmd = ["timeout", "-k", "10", str(limit)] + cmd
    print("+", " ".join(cmd), flush=True)
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"step failed with exit status {p.returncode}: nothing more is started")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def accuracy(path):
    """``hvp <case>: (y, relmax) positions (a, b) cells (c, d) tangent (e, f)`` lines of the GPU tests' output."""
    out = []
    pair = r"\(([-+.e\d]+|nan), ([-+.e\d]+|nan)\)"
    for ln in open(path):
        m = re.search(r"hvp ([\w ]+): \(y, relmax\) (.*)", ln)
        if not m:
            continue
        row = {"case": m.group(1)}
        for what, y, e in re.findall(r"(\w+) " + pair, m.group(2)):
            row[what] = {"y": float(y), "relmax": float(e)}
        out.append(row)
    return out


def bench_medians(path):
    """Medians of the ``parent <json>`` / ``this <json>`` lines of alternating ``bench.py`` runs."""
    runs = {"parent": [], "this": []}
    for ln in open(path):
        who, _, rest = ln.partition(" ")
        if who in runs and rest.startswith("{"):
            runs[who].append(json.loads(rest))
    out = {}
    for who, rows in runs.items():
        keys = [k for k, v in rows[0].items() if isinstance(v, (int, float)) and not isinstance(v, bool)] if rows else []
        out[who] = {"runs": len(rows), "median": {k: sorted(r[k] for r in rows)[len(rows) // 2] for k in keys},
                    "all": rows}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=list(MODELS), default=None)
    ap.add_argument("--atoms", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--accuracy-log", default=None)
    ap.add_argument("--zbl", action="store_true", help="the ZBL arm: pet_hessian_vector with and without the pair term's")
    ap.add_argument("--bench-log", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed to each GPU step")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "zbl_hvp_bench.json" if args.zbl else "hvp_bench.json")
    me = [sys.executable, os.path.abspath(__file__)]
    common = ["--atoms", str(args.atoms), "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
    result = {"workload": "one Hessian-vector product on one periodic box, arms alternating in one process (ms, host clock); "
                          "train2 is THIS build's pet_backward_train2 (its gradient has the bits of the build before the "
                          "Hessian-vector mode: tests/golden/gen_train_parent_digest.json)"}
    if args.zbl:
        result = {"workload": "one Hessian-vector product on one periodic box, default model, without and with the ZBL pair "
                              "term's product on the same graph, arms alternating in one process (ms, host clock)",
                  "default": run(me + ["--worker", "default", "--zbl"] + common, args.limit)}
        if args.bench_log:
            result["bench_py_gpus1_steps20_warmup5"] = bench_medians(args.bench_log)
    else:
        for name in MODELS:
            result[name] = run(me + ["--worker", name] + common, args.limit)
    if args.accuracy_log:
        result["accuracy_vs_fp64_oracle"] = accuracy(args.accuracy_log)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
