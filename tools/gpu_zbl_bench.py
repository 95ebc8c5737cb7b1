"""Cost of the ZBL additive model on the inference step (energy + forces), default PET model on the bench's synthetic boxes:
8 x 10 000 atoms and one 1 000-atom box. Within one process the two arms -- the plain step (``HipForward`` forward +
backward) and the step with ``ZBLHip`` forward + backward on the same graph -- alternate after a warm-up, each timed by a
host clock between two device synchronisations; what counts is the ratio of their medians in the same run. The ZBL
kernels' own time comes from a separate ``rocprofv3 --kernel-trace --stats`` run of the ZBL calls alone, and is set
against the bytes the kernels must read (24 B per graph edge -- geometry 16, centre 4, neighbour species 4 -- plus 8 B per
atom, in each of the two kernels) for the achieved bytes/s.

The driver itself does not touch the GPU: every step is a child process under its own time limit, and the first failure
ends the run.

  python tools/gpu_zbl_bench.py --out profiles/zbl_bench.json
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12  # B/s, MI355X


def _batch(boxes, atoms):
    import torch

    from metatrain_amd import runtime as rt
    from metatrain_amd.pet import default_hypers
    from metatrain_amd.synthetic import random_box, synthetic_params
    from metatrain_amd.zbl import ZBLHip

    dev = torch.device("cuda:0")
    types = [1, 6, 7, 8]
    hypers = default_hypers()
    model = rt.HipModel(hypers, types)
    model.load({k: v.to(dev) for k, v in synthetic_params(hypers, types, {"energy": 1}, 0, torch.float32).items()}, "energy")
    pos_l, z_l, cell_l, pair_l, sys_l = [], [], [], [], []
    for b in range(boxes):
        pos, z, cell = random_box(atoms, seed=b)
        posd = pos.to(dev)
        pairs, _ = rt.neighbor_list(posd, cell, [True] * 3, hypers["cutoff"])
        pairs = pairs.clone()
        pairs[:, 0:2] += b * atoms
        pos_l.append(posd); z_l.append(z.to(dev)); cell_l.append(cell.to(dev)); pair_l.append(pairs)
        sys_l.append(torch.full((atoms,), b, dtype=torch.int32, device=dev))
    pairs = torch.cat(pair_l)
    graph = rt.HipGraph(model, torch.cat(pos_l), torch.stack(cell_l), pairs[:, 0].contiguous(), pairs[:, 1].contiguous(),
                        pairs[:, 2:5].contiguous(), torch.cat(z_l), torch.cat(sys_l))
    return rt, model, graph, ZBLHip(types)


def worker_time(args):
    import torch

    rt, model, graph, zbl = _batch(args.boxes, args.atoms)
    fw = rt.HipForward(model, graph)
    ones = torch.ones(graph.n_nodes, device="cuda:0")

    def step(with_zbl):
        atomic = fw.forward()
        grad = fw.backward(ones)
        if with_zbl:
            atomic = atomic + zbl.forward(graph)
            grad = grad + zbl.backward(graph)
        return atomic, grad

    for _ in range(args.warmup):
        step(False), step(True)
    times = {"off": [], "on": []}
    for _ in range(args.rounds):
        for arm, flag in (("off", False), ("on", True)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(flag)
            torch.cuda.synchronize()
            times[arm].append((time.perf_counter() - t0) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    inside = int((zbl.forward(graph) != 0).sum())
    print(json.dumps({"boxes": args.boxes, "atoms_per_box": args.atoms, "graph_edges": graph.n_edges,
                      "atoms_with_zbl_energy": inside, "ms_per_step_median": med, "ratio_on_over_off": med["on"] / med["off"],
                      "ms_per_step_all": times}))


def worker_kernels(args):
    import torch

    rt, model, graph, zbl = _batch(args.boxes, args.atoms)
    for _ in range(args.warmup + args.rounds):
        zbl.forward(graph)
        zbl.backward(graph)
    torch.cuda.synchronize()
    print(json.dumps({"graph_edges": graph.n_edges, "atoms": graph.n_nodes, "calls": args.warmup + args.rounds}))


def run(cmd, limit):
    cmd = ["timeout", "-k", "10", str(limit)] + cmd
    print("+", " ".join(cmd), flush=True)
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"step failed with exit status {p.returncode}: nothing more is started")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["time", "kernels"], default=None)
    ap.add_argument("--boxes", type=int, default=8)
    ap.add_argument("--atoms", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zbl_bench.json"))
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed to each GPU step")
    args = ap.parse_args()
    if args.worker == "time":
        return worker_time(args)
    if args.worker == "kernels":
        return worker_kernels(args)

    me = [sys.executable, os.path.abspath(__file__)]
    common = ["--rounds", str(args.rounds), "--warmup", str(args.warmup)]
    result = {"workload": "default PET, inference step (energy + forces), ZBL off / on alternating in one process"}
    result["batch_8x10000"] = run(me + ["--worker", "time", "--boxes", str(args.boxes), "--atoms", str(args.atoms)] + common,
                                  args.limit)
    result["box_1000"] = run(me + ["--worker", "time", "--boxes", "1", "--atoms", "1000"] + common, args.limit)
    with tempfile.TemporaryDirectory() as tmp:
        info = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "zbl", "--"] + me +
                   ["--worker", "kernels", "--boxes", str(args.boxes), "--atoms", str(args.atoms)] + common, args.limit)
        kernels = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                if "k_zbl" not in r["Kernel_Name"]:
                    continue
                name = "k_zbl_rows<bwd>" if "ILb1E" in r["Kernel_Name"] or "<true>" in r["Kernel_Name"] else \
                    "k_zbl_rows<fwd>" if "k_zbl_rows" in r["Kernel_Name"] else "k_zbl_sys"
                kernels.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    if not kernels:
        raise SystemExit("the kernel trace holds no ZBL kernel")
    need = info["graph_edges"] * 24.0 + info["atoms"] * 8.0
    result["zbl_kernels"] = {"graph_edges": info["graph_edges"], "atoms": info["atoms"], "bytes_needed_per_launch": need}
    for name, us in kernels.items():
        med = sorted(us)[len(us) // 2]
        result["zbl_kernels"][name] = {"calls": len(us), "median_us": med, "achieved_bytes_per_s": need / (med * 1e-6),
                                       "fraction_of_hbm_peak": need / (med * 1e-6) / HBM_PEAK}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
