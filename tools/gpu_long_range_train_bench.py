"""Cost of the long-range PET's force-loss training sweep on the 1 000-atom synthetic box of ``profiles/long_range_bench.json``
at the default size, next to the same model without long range. A record, not a gate: writes
``profiles/long_range_train_bench.json``.

    python tools/gpu_long_range_train_bench.py [--atoms 1000] [--repeats 10] [--calls 20]

Legs, alternating in one process (host clock around ``--calls`` calls and a synchronise, median of ``--repeats`` samples, spread
reported): the second-order call and the whole optimizer step, each with long range (``LongRangeForward`` /
``LongRangeTrainStep``) and without (``HipForward(train=True)`` / ``TrainStep``: the tuned pass serves the default size there);
the operator's full second-order call (``EwaldHip.second``: all three results, what the parent commit had) next to the sweep's
own operator calls, which are read from the library's event profiler in a pass of their own (``ewald_second_g``: the dual
forward's tangent alone; ``ewald_second_q``: the training reverse's ``(D_u A) lambda_V`` alone; ``ewald_fwd``: ``A x``).
Kernel shares: ``rocprofv3 --kernel-trace --stats -- python tools/gpu_long_range_train_bench.py --profile-sweeps 5``, a run
of its own.

    python tools/gpu_long_range_train_bench.py --p3m [--atoms 1000 10000]

The same sweep and step THROUGH THE MESH OPERATOR (``method="p3m", second_order=True``), per box, next to
the Ewald legs above alternated in the same run where the Ewald plan serves the box (it refuses cells beyond 63 reciprocal
indices per axis: the 10 000-atom box has no Ewald legs). Legs: the sweep, the whole step, ``P3MHip.second`` with all three
results and with each result alone, energies and forces; the sweep's own operator stages (``p3m_*`` / ``ewald_*``) from the
event profiler. Calls per sample scale down with the box (``--calls`` at 1 000 atoms). Writes
``profiles/long_range_p3m_train_bench.json``.

    python tools/gpu_long_range_train_bench.py --stress [--atoms 1000]

The cost of the CELL tangent (``cell_tangents=True``), by Ewald summation and through P3M on one box: the
sweep with ``(u, u_cell)`` against the same sweep with ``u`` alone on the same build, the whole step with and without the strain
term, and ``second_cell`` against ``second`` without its position result; all legs alternating. The sweeps' operator stages from
the event profiler in a pass of their own. ``--profile-sweeps K --stress [--p3m]`` runs K sweeps with ``(u, u_cell)`` alone, for a
kernel trace. Writes ``profiles/long_range_stress_train_bench.json``."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from metatrain_amd import long_range as lr  # noqa: E402
from metatrain_amd import runtime as rt  # noqa: E402
from metatrain_amd import synthetic  # noqa: E402
from metatrain_amd.pet.hypers import default_hypers  # noqa: E402
from metatrain_amd.pet.trainer import TrainStep  # noqa: E402

TYPES = [1, 6, 7, 8]
LR = {"enable": True, "use_ewald": True, "smearing": 1.4, "kspace_resolution": 1.33, "interpolation_nodes": 5}


def build(enable, pos, z, cell, dev, method=None, cell_tangents=False):
    hypers = default_hypers()
    if enable:
        hypers["long_range"] = dict(LR)
    params = dict(synthetic.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32))
    feat = None
    if enable:
        torch.manual_seed(0)  # (the featuriser draws its six tensors: the same ones for either operator)
        feat = lr.LongRangeFeaturizerHip(hypers, device=dev, method=method, second_order=method == "p3m",
                                         cell_tangents=cell_tangents)
        params.update({k: v.cpu() for k, v in feat.state_dict().items()})
    model = rt.HipModel(hypers, TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    n = pos.shape[0]
    pairs, _ = rt.neighbor_list(pos.to(dev), cell, [True] * 3, hypers["cutoff"])
    graph = rt.HipGraph(model, pos.to(dev), cell[None].to(dev), pairs[:, 0], pairs[:, 1], pairs[:, 2:5], z.to(dev),
                        torch.zeros(n, dtype=torch.int32, device=dev))
    return hypers, model, graph, feat


def p3m_box(n, args, dev):
    """The legs of one box through the mesh operator, and through the Ewald sum where its plan serves the box."""
    pos, z, cell = synthetic.random_box(n, seed=11)
    pbcs = [[True] * 3]
    gen = torch.Generator(device=dev).manual_seed(0)
    nu = torch.rand(n, device=dev, generator=gen) - 0.5
    u = torch.randn(n, 3, device=dev, generator=gen)
    ones = torch.ones(n, device=dev)
    te, tg, n_atoms = torch.zeros(1, device=dev), torch.zeros(n, 3, device=dev), torch.full((1,), float(n), device=dev)
    train = {"learning_rate": 1e-6, "warmup_fraction": 0.0, "num_epochs": 10**9}
    calls = max(2, args.calls * 1000 // n)
    p32 = pos.to(dev)
    legs, ops, sweeps, refused = {}, {}, {}, None
    for tag, method in (("p3m", "p3m"), ("ewald", None)):
        hyp, model, graph, feat = build(True, pos, z, cell, dev, method)
        fw = lr.LongRangeForward(model, feat, graph, pbcs)
        step = lr.LongRangeTrainStep(model, feat, train)
        c = hyp["d_node"]
        q, g, uq = (torch.randn(n, c, device=dev, generator=gen) for _ in range(3))

        def sweep(model=model, fw=fw):
            model.zero_grad()
            fw.backward_train2(ones, nu, u)

        try:
            sweep()
        except lr.PetHipError as exc:  # (the Ewald plan of a box it does not serve)
            if tag == "p3m":
                raise
            refused = str(exc)
            continue
        op = ops[tag] = feat.ewald
        sweeps[tag] = sweep
        legs[f"second_order_{tag}"] = sweep
        legs[f"step_{tag}"] = lambda step=step, graph=graph, fw=fw: step(graph, fw, te, n_atoms, tg)
        legs[f"energy_and_forces_{tag}"] = lambda model=model, feat=feat, graph=graph: lr.energy_and_gradient(
            model, feat, graph, pbcs, replan=False)
        legs[f"operator_second_all_results_{tag}"] = lambda op=op, graph=graph, q=q, g=g, uq=uq: op.second(graph, p32, q, g, uq, u)
        if tag == "p3m":
            for k, name in enumerate(("out_charges", "out_grad_potential", "out_positions")):
                sel = tuple(j == k for j in range(3))
                legs[f"operator_second_{name}_alone_p3m"] = lambda op=op, graph=graph, q=q, g=g, uq=uq, sel=sel: op.second(
                    graph, p32, q, g, uq, u, results=sel)
        edges, mesh = graph.n_edges, (op.mesh_shape(0) if tag == "p3m" else None)
        if tag == "p3m":
            p3m_edges, p3m_mesh = edges, mesh
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in legs}
    for _ in range(args.repeats):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            samples[name].append(1e3 * (time.perf_counter() - t0) / calls)
    med = {k: statistics.median(v) for k, v in samples.items()}
    stages, operator_ms = {}, {}
    for tag, sweep in sweeps.items():
        rt.profile(True)
        for _ in range(calls):
            sweep()
        torch.cuda.synchronize()
        stages[tag] = {r["name"]: {"ms_per_call": r["total_ms"] / max(r["calls"], 1), "calls_per_sweep": r["calls"] / calls}
                       for r in rt.profile_report() if r["name"].startswith(("ewald", "p3m"))}
        rt.profile(False)
        operator_ms[tag] = sum(s["ms_per_call"] * s["calls_per_sweep"] for s in stages[tag].values())
    return {"atoms": n, "channels": c, "graph_edges": p3m_edges, "mesh": p3m_mesh, "calls_per_sample": calls,
            "kvectors": ops["ewald"].num_kvectors(0) if "ewald" in ops else None, "ewald_refused": refused, "ms": samples,
            "ms_median": med, "ms_min": {k: min(v) for k, v in samples.items()}, "ms_max": {k: max(v) for k, v in samples.items()},
            "sweep_operator_stages": stages, "sweep_operator_ms_device_events": operator_ms,
            "transform_hook_calls_per_sweep": None if "p3m" not in ops else _hook_calls(ops["p3m"], sweeps["p3m"])}


def stress_main(args):
    dev = torch.device("cuda:0")
    n = (args.atoms or [1000])[0]
    pos, z, cell = synthetic.random_box(n, seed=11)
    pbcs = [[True] * 3]
    gen = torch.Generator(device=dev).manual_seed(0)
    nu = torch.rand(n, device=dev, generator=gen) - 0.5
    u = torch.randn(n, 3, device=dev, generator=gen)
    u_cell = cell.to(dev)[None] @ (0.1 * torch.randn(1, 3, 3, device=dev, generator=gen))
    ones = torch.ones(n, device=dev)
    te, tg, n_atoms = torch.zeros(1, device=dev), torch.zeros(n, 3, device=dev), torch.full((1,), float(n), device=dev)
    ts = torch.zeros(1, 3, 3, device=dev)
    train = {"learning_rate": 1e-6, "warmup_fraction": 0.0, "num_epochs": 10**9}
    p32, c32 = pos.to(dev), cell[None].to(dev)
    legs, sweeps, info = {}, {}, {}
    for tag, method in (("ewald", None), ("p3m", "p3m")):
        if args.profile_sweeps and (tag == "p3m") != args.p3m:
            continue
        hyp, model, graph, feat = build(True, pos, z, cell, dev, method, cell_tangents=True)
        fw = lr.LongRangeForward(model, feat, graph, pbcs)
        step = lr.LongRangeTrainStep(model, feat, train)
        c = hyp["d_node"]
        q, g, uq = (torch.randn(n, c, device=dev, generator=gen) for _ in range(3))
        op = feat.ewald

        def sweep(model=model, fw=fw, uc=None):
            model.zero_grad()
            fw.backward_train2(ones, nu, u, u_cell=uc)

        sweeps[tag] = (sweep, lambda sweep=sweep: sweep(uc=u_cell))
        legs[f"sweep_u_{tag}"] = sweeps[tag][0]
        legs[f"sweep_u_and_u_cell_{tag}"] = sweeps[tag][1]
        legs[f"step_energy_forces_{tag}"] = lambda step=step, graph=graph, fw=fw: step(graph, fw, te, n_atoms, tg)
        legs[f"step_energy_forces_strain_{tag}"] = lambda step=step, graph=graph, fw=fw: step(
            graph, fw, te, n_atoms, tg, target_strain_gradients=ts, positions=p32, cells=c32)
        if tag == "p3m":
            legs["operator_second_two_results_p3m"] = lambda op=op, graph=graph, q=q, g=g, uq=uq: op.second(
                graph, p32, q, g, uq, u, results=(True, True, False))
        legs[f"operator_second_cell_{tag}"] = lambda op=op, graph=graph, q=q, g=g, uq=uq: op.second_cell(graph, p32, q, g, uq, u, u_cell)
        info[tag] = {"graph_edges": graph.n_edges, "channels": c, "op": op}
    if args.profile_sweeps:
        for fn in sweeps.values():
            for _ in range(args.profile_sweeps + 1):
                fn[1]()
        torch.cuda.synchronize()
        return
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    for tag, v in info.items():   # (the plan exists after the first sweep)
        op = v.pop("op")
        v.update(kvectors=op.num_kvectors(0) if tag == "ewald" else None, mesh=op.mesh_shape(0) if tag == "p3m" else None)
    samples = {k: [] for k in legs}
    for _ in range(args.repeats):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            samples[name].append(1e3 * (time.perf_counter() - t0) / args.calls)
    med = {k: statistics.median(v) for k, v in samples.items()}
    stages = {}
    for tag, pair in sweeps.items():
        for which, fn in zip(("u", "u_and_u_cell"), pair):
            rt.profile(True)
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            stages[f"{which}_{tag}"] = {r["name"]: {"ms_per_call": r["total_ms"] / max(r["calls"], 1),
                                                   "calls_per_sweep": r["calls"] / args.calls}
                                        for r in rt.profile_report() if r["name"].startswith(("ewald", "p3m"))}
            rt.profile(False)
    result = {"workload": f"{n}-atom synthetic periodic box, default PET, long-range featuriser with cell_tangents=True by Ewald "
                          "summation and through P3M (interpolation_nodes 5, mesh spacing 1.33); ms per call on the host clock "
                          f"around {args.calls} calls and a synchronise, median of {args.repeats} samples, all legs alternating, "
                          "after one warm-up call each; operator stages from device events in passes of their own",
              "atoms": n, "info": info, "ms": samples, "ms_median": med, "ms_min": {k: min(v) for k, v in samples.items()},
              "ms_max": {k: max(v) for k, v in samples.items()},
              "cell_tangent_ms": {t: med[f"sweep_u_and_u_cell_{t}"] - med[f"sweep_u_{t}"] for t in sweeps},
              "strain_term_ms": {t: med[f"step_energy_forces_strain_{t}"] - med[f"step_energy_forces_{t}"] for t in sweeps},
              "sweep_operator_stages": stages}
    out = args.out or os.path.join(ROOT, "profiles", "long_range_stress_train_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh)
    print(json.dumps({k: v for k, v in result.items() if k != "ms"}))


def _hook_calls(op, sweep):
    before = op.transform_calls
    sweep()
    torch.cuda.synchronize()
    return op.transform_calls - before


def p3m_main(args):
    dev = torch.device("cuda:0")
    boxes = [p3m_box(n, args, dev) for n in args.atoms]
    result = {"workload": "synthetic periodic boxes, default PET, long-range featuriser through P3M (interpolation_nodes 5, mesh "
                          "spacing 1.33) and, where its plan serves the box, through the Ewald sum; ms per call on the host clock "
                          "around calls_per_sample calls and a synchronise, median of "
                          f"{args.repeats} samples, all legs of a box alternating, after one warm-up call each; operator stages "
                          "from device events in a pass of their own", "boxes": boxes}
    out = args.out or os.path.join(ROOT, "profiles", "long_range_p3m_train_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh)
    for b in boxes:
        print(json.dumps({k: v for k, v in b.items() if k != "ms"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p3m", action="store_true", help="the legs through the mesh operator (profiles/long_range_p3m_train_bench.json)")
    ap.add_argument("--atoms", type=int, nargs="+", default=None, help="1000; with --p3m one or more boxes, default 1000 10000")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-sweeps", type=int, default=0,
                    help="run only this many long-range second-order sweeps after one warm-up and exit: the command to put "
                         "under rocprofv3 --kernel-trace --stats (profiles/long_range_train_kernel_stats.csv)")
    ap.add_argument("--stress", action="store_true",
                    help="the cost of the cell tangent and of the strain term (profiles/long_range_stress_train_bench.json)")
    args = ap.parse_args()
    if args.stress:
        return stress_main(args)
    if args.p3m:
        args.atoms = args.atoms or [1000, 10000]
        return p3m_main(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "long_range_train_bench.json")
    dev = torch.device("cuda:0")
    n = (args.atoms or [1000])[0]
    pos, z, cell = synthetic.random_box(n, seed=11)
    pbcs = [[True] * 3]
    gen = torch.Generator(device=dev).manual_seed(0)
    nu = torch.rand(n, device=dev, generator=gen) - 0.5
    u = torch.randn(n, 3, device=dev, generator=gen)
    ones = torch.ones(n, device=dev)
    te = torch.zeros(1, device=dev)
    tg = torch.zeros(n, 3, device=dev)
    n_atoms = torch.full((1,), float(n), device=dev)
    hyp_l, model_l, graph_l, feat = build(True, pos, z, cell, dev)
    hyp_s, model_s, graph_s, _ = build(False, pos, z, cell, dev)
    fw_l = lr.LongRangeForward(model_l, feat, graph_l, pbcs)
    fw_s = rt.HipForward(model_s, graph_s, train=True)
    train = {"learning_rate": 1e-6, "warmup_fraction": 0.0, "num_epochs": 10**9}
    step_l = lr.LongRangeTrainStep(model_l, feat, train)
    step_s = TrainStep(model_s, train)
    ew = feat.ewald
    c = hyp_l["d_node"]
    q, g, uq = (torch.randn(n, c, device=dev, generator=gen) for _ in range(3))
    p32 = pos.to(dev)

    def sweep_l():
        model_l.zero_grad()
        fw_l.backward_train2(ones, nu, u)

    def sweep_s():
        model_s.zero_grad()
        fw_s.forward()
        fw_s.backward_train2(ones, nu, u)

    if args.profile_sweeps:
        for _ in range(args.profile_sweeps + 1):
            sweep_l()
        torch.cuda.synchronize()
        return
    legs = {"second_order_long_range": sweep_l, "forward_and_second_order_short_range": sweep_s,
            "step_long_range": lambda: step_l(graph_l, fw_l, te, n_atoms, tg),
            "step_short_range": lambda: step_s(graph_s, fw_s, te, n_atoms, tg),
            "operator_second_all_results": lambda: ew.second(graph_l, p32, q, g, uq, u),
            "energy_and_forces_long_range": lambda: lr.energy_and_gradient(model_l, feat, graph_l, pbcs, replan=False)}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in legs}
    for _ in range(args.repeats):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            samples[name].append(1e3 * (time.perf_counter() - t0) / args.calls)
    med = {k: statistics.median(v) for k, v in samples.items()}
    # the sweep's own operator calls, from the event profiler (a pass of its own: the events serialise nothing on one stream,
    # but they are not part of the timed legs)
    rt.profile(True)
    for _ in range(args.calls):
        sweep_l()
    torch.cuda.synchronize()
    stages = {r["name"]: {"ms_per_call": r["total_ms"] / max(r["calls"], 1), "calls_per_sweep": r["calls"] / args.calls}
              for r in rt.profile_report() if r["name"].startswith("ewald")}
    rt.profile(False)
    ewald_ms = sum(s["ms_per_call"] * s["calls_per_sweep"] for s in stages.values())
    result = {"workload": f"{n}-atom synthetic periodic box, default PET (d_node = {c}), {ew.num_kvectors(0)} k-vectors, "
                          f"{graph_l.n_edges} edges; ms per call on the host clock around {args.calls} calls and a synchronise, "
                          f"median of {args.repeats} samples, the legs alternating, after one warm-up call each",
              "atoms": n, "channels": c, "kvectors": ew.num_kvectors(0), "graph_edges": graph_l.n_edges, "ms": samples,
              "ms_median": med, "ms_min": {k: min(v) for k, v in samples.items()}, "ms_max": {k: max(v) for k, v in samples.items()},
              "sweep_operator_stages": stages, "sweep_operator_ms": ewald_ms,
              "sweep_operator_share": ewald_ms / med["second_order_long_range"]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh)
    print(json.dumps({k: v for k, v in result.items() if k != "ms"}))


if __name__ == "__main__":
    main()
