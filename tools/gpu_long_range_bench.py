"""Times of the long-range (Ewald) operator and of the whole long-range PET on the 1 000-atom synthetic box at C = d_node =
256, next to the same box without long range. A record, not a gate: writes ``profiles/long_range_bench.json``.

    python tools/gpu_long_range_bench.py [--atoms 1000] [--repeats 10] [--out profiles/long_range_bench.json]

``--leg second`` times the operator's second-order call (``EwaldHip.second``) next to its first-order adjoint (``backward``
without cell gradients) on the same box in one process, alternating the two, and writes ``profiles/long_range_second_bench.json``.
"""
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

TYPES = [1, 6, 7, 8]


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def second_leg(args):
    """``second`` (both cotangents) against ``backward`` on the box at C = d_node: samples of ``--calls`` calls each, the two
    alternating, after a warm-up of both."""
    dev = torch.device("cuda:0")
    hypers = default_hypers()
    hypers["long_range"] = {"enable": True, "use_ewald": True, "smearing": 1.4, "kspace_resolution": 1.33, "interpolation_nodes": 5}
    pos, z, cell = synthetic.random_box(args.atoms, seed=11)
    n, c = args.atoms, hypers["d_node"]
    model = rt.HipModel(hypers, TYPES)
    model.load_species_table()
    pairs, _ = rt.neighbor_list(pos.to(dev), cell, [True] * 3, hypers["cutoff"])
    graph = rt.HipGraph(model, pos.to(dev), cell[None].to(dev), pairs[:, 0], pairs[:, 1], pairs[:, 2:5], z.to(dev),
                        torch.zeros(n, dtype=torch.int32, device=dev))
    ew = lr.EwaldHip(1.4, 1.33, hypers["cutoff"]).plan(cell[None], [[True] * 3], [0, n])
    gen = torch.Generator(device=dev).manual_seed(0)
    q, g, uq = (torch.randn(n, c, device=dev, generator=gen) for _ in range(3))
    ur = torch.randn(n, 3, device=dev, generator=gen)
    p32 = pos.to(dev)
    legs = {"backward": lambda: ew.backward(graph, p32, q, g), "second": lambda: ew.second(graph, p32, q, g, uq, ur),
            "second_u_positions_only": lambda: ew.second(graph, p32, q, g, None, ur),
            "second_u_charges_only": lambda: ew.second(graph, p32, q, g, uq, None)}
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
    result = {"workload": f"{n}-atom synthetic periodic box, C = {c}, {ew.num_kvectors(0)} k-vectors, {graph.n_edges} edges; ms per "
                          f"call on the host clock around {args.calls} calls and a synchronise, median of {args.repeats} samples, "
                          "the legs alternating, after one warm-up call each",
              "atoms": n, "channels": c, "kvectors": ew.num_kvectors(0), "graph_edges": graph.n_edges, "ms": samples,
              "ms_median": med, "ms_min": {k: min(v) for k, v in samples.items()}, "ms_max": {k: max(v) for k, v in samples.items()},
              "second_over_backward": med["second"] / med["backward"],
              "gemm_count": {"second": {"structure_factors": 5, "gathers": 3, "force_type_products": 3},
                             "backward": {"structure_factors": 2, "gathers": 1, "force_type_products": 1}}}
    os.makedirs(os.path.dirname(args.second_out), exist_ok=True)
    with open(args.second_out, "w") as fh:
        json.dump(result, fh)
    print(json.dumps({k: v for k, v in result.items() if k != "ms"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_range_bench.json"))
    ap.add_argument("--leg", choices=("model", "second"), default="model")
    ap.add_argument("--calls", type=int, default=20, help="calls per timed sample of --leg second")
    ap.add_argument("--second-out", default=os.path.join(ROOT, "profiles", "long_range_second_bench.json"))
    args = ap.parse_args()
    if args.leg == "second":
        return second_leg(args)
    dev = torch.device("cuda:0")
    pos, z, cell = synthetic.random_box(args.atoms, seed=11)
    n = args.atoms
    sysidx = torch.zeros(n, dtype=torch.int32, device=dev)
    result = {"workload": f"{n}-atom synthetic periodic box, default PET (d_node = 256), ms on the host clock, median of "
                          f"{args.repeats} after one warm-up", "atoms": n}
    arms = {}
    for name, enable in (("long_range", True), ("short_range", False)):
        hypers = default_hypers()
        if enable:
            hypers["long_range"] = {"enable": True, "use_ewald": True, "smearing": 1.4, "kspace_resolution": 1.33,
                                    "interpolation_nodes": 5}
        params = synthetic.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
        model = rt.HipModel(hypers, TYPES)
        model.load({k: v.to(dev) for k, v in params.items()}, "energy")
        pairs, _ = rt.neighbor_list(pos.to(dev), cell, [True] * 3, hypers["cutoff"])
        graph = rt.HipGraph(model, pos.to(dev), cell[None].to(dev), pairs[:, 0], pairs[:, 1], pairs[:, 2:5], z.to(dev), sysidx)
        arm = {"graph_edges": graph.n_edges}
        if enable:
            feat = lr.LongRangeFeaturizerHip(hypers, device=dev)
            feat.plan(cell[None], [[True] * 3], [0, n])
            ew = feat.ewald
            c = hypers["d_node"]
            k = ew.num_kvectors(0)
            arm.update(kvectors=k, channels=c,
                       gflop_per_application=2.0 * 2.0 * n * (k // 2) * c * 2.0 / 1e9)  # structure factor + gather, re and im
            q = torch.randn(n, c, device=dev)
            g = torch.randn(n, c, device=dev)
            p32 = pos.to(dev)
            arm["ms_potential"] = timed(lambda: ew.potential(graph, p32, q), args.repeats)
            arm["ms_backward"] = timed(lambda: ew.backward(graph, p32, q, g, want_cell_grad=True), args.repeats)
            t0 = time.perf_counter()
            feat.plan(cell[None], [[True] * 3], [0, n])
            arm["ms_plan"] = 1e3 * (time.perf_counter() - t0)
            arm["ms_energy_forces"] = timed(
                lambda: lr.energy_and_gradient(model, feat, graph, [[True] * 3], replan=False), args.repeats)
        else:
            fw = rt.HipForward(model, graph)

            def step():
                atomic = fw.forward()
                fw.backward(torch.ones_like(atomic))

            arm["ms_energy_forces"] = timed(step, args.repeats)
        arm["ms_median"] = {k[3:]: statistics.median(v) for k, v in arm.items() if k.startswith("ms_") and isinstance(v, list)}
        arms[name] = arm
    result.update(arms)
    result["long_over_short_energy_forces"] = (arms["long_range"]["ms_median"]["energy_forces"]
                                               / arms["short_range"]["ms_median"]["energy_forces"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh)
    print(json.dumps({k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if not isinstance(b, list)})
                      for k, v in result.items()}))


if __name__ == "__main__":
    main()
