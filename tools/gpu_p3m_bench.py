"""Times of the long-range operator under both methods (Ewald, P3M) and of the whole long-range PET on the 1 000-atom synthetic
box of ``profiles/long_range_bench.json`` at C = d_node = 256, in one process, and of a 10 000-atom box under P3M. A record, not
a gate: writes ``profiles/p3m_bench.json``. Host clock around work that ends in a device synchronise, every shape warmed up
first, median of ``--repeats`` windows of ``--inner`` calls each; the P3M stages are timed one by one as well, so the record
says where an application spends its time.

    python tools/gpu_p3m_bench.py [--atoms 1000] [--large 10000] [--repeats 10] [--inner 5] [--out profiles/p3m_bench.json]
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
from metatrain_amd._lib import check  # noqa: E402
from metatrain_amd.pet.hypers import default_hypers  # noqa: E402

TYPES = [1, 6, 7, 8]


def timed(fn, repeats, inner):
    fn()
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / inner)
    return out


def p3m_stages(op, graph, pos, q, repeats, inner):
    """ms of the five stages of one application, each from the inputs the stage before left behind."""
    c = int(q.shape[1])
    ws = op._ws(c, q.device)
    mesh = torch.empty(max(op._mesh_points * c, 1), dtype=torch.float32, device=q.device)
    spec = torch.empty(max(op._spec_points * c, 1), dtype=torch.complex64, device=q.device)
    out = torch.empty_like(q)
    views = []
    for n, moff, soff in op._meshes:
        m, mh = n[0] * n[1] * n[2], n[0] * n[1] * (n[2] // 2 + 1)
        views.append((n, mesh[moff * c:(moff + m) * c].view(c, *n), spec[soff * c:(soff + mh) * c].view(c, n[0], n[1], n[2] // 2 + 1)))

    def spread():
        check(op.lib.pet_p3m_spread(op.handle, graph.handle, rt._ptr(pos), rt._ptr(q), c, rt._ptr(mesh), rt._ptr(ws), ws.numel(),
                                    rt._stream()))

    def forward_fft():
        for n, real, half in views:
            torch.fft.rfftn(real, dim=(1, 2, 3), out=half)

    def filt():
        check(op.lib.pet_p3m_filter(op.handle, c, rt._ptr(spec), rt._stream()))

    def backward_fft():
        for n, real, half in views:
            torch.fft.irfftn(half, s=n, dim=(1, 2, 3), norm="forward", out=real)

    def finish():
        check(op.lib.pet_p3m_finish(op.handle, graph.handle, rt._ptr(pos), rt._ptr(q), c, rt._ptr(mesh), rt._ptr(out), rt._ptr(ws),
                                    ws.numel(), rt._stream()))

    stages = {}
    for name, fn in (("spread", spread), ("rfftn", forward_fft), ("filter", filt), ("irfftn", backward_fft), ("finish", finish)):
        stages[name] = statistics.median(timed(fn, repeats, inner))
    return stages


def box(n_atoms, methods, dev, repeats, inner, model_too=True):
    pos, z, cell = synthetic.random_box(n_atoms, seed=11)
    sysidx = torch.zeros(n_atoms, dtype=torch.int32, device=dev)
    hypers = default_hypers()
    hypers["long_range"] = {"enable": True, "use_ewald": True, "smearing": 1.4, "kspace_resolution": 1.33, "interpolation_nodes": 5}
    params = synthetic.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    model = rt.HipModel(hypers, TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    pairs, _ = rt.neighbor_list(pos.to(dev), cell, [True] * 3, hypers["cutoff"])
    graph = rt.HipGraph(model, pos.to(dev), cell[None].to(dev), pairs[:, 0], pairs[:, 1], pairs[:, 2:5], z.to(dev), sysidx)
    c = hypers["d_node"]
    gen = torch.Generator(device=dev).manual_seed(5)
    q = torch.randn(n_atoms, c, device=dev, generator=gen)
    g = torch.randn(n_atoms, c, device=dev, generator=gen)
    p32 = pos.to(dev)
    result = {"atoms": n_atoms, "graph_edges": graph.n_edges, "channels": c, "cell": [float(x) for x in cell.diagonal()]}
    for method in methods:
        feat = lr.LongRangeFeaturizerHip(hypers, device=dev, method=method)
        t0 = time.perf_counter()
        feat.plan(cell[None], [[True] * 3], [0, n_atoms])
        torch.cuda.synchronize()
        arm = {"ms_plan": 1e3 * (time.perf_counter() - t0)}
        op = feat.ewald
        if method == "p3m":
            arm["mesh"] = op.mesh_shape(0)
        else:
            arm["kvectors"] = op.num_kvectors(0)
        arm["ms_potential"] = timed(lambda: op.potential(graph, p32, q), repeats, inner)
        arm["ms_backward"] = timed(lambda: op.backward(graph, p32, q, g, want_cell_grad=True), repeats, inner)
        if model_too:
            arm["ms_energy_forces"] = timed(lambda: lr.energy_and_gradient(model, feat, graph, [[True] * 3], replan=False), repeats,
                                            inner)
        if method == "p3m":
            arm["ms_stage_median"] = p3m_stages(op, graph, p32, q, repeats, inner)
        arm["ms_median"] = {k[3:]: statistics.median(v) for k, v in arm.items() if k.startswith("ms_") and isinstance(v, list)}
        result[method] = arm
    if "p3m" in result and "ewald" in result:
        a, b = result["p3m"]["ms_median"], result["ewald"]["ms_median"]
        result["p3m_over_ewald"] = {k: a[k] / b[k] for k in a if k in b}
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=1000)
    ap.add_argument("--large", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p3m_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_p3m_bench.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    result = {"workload": "synthetic periodic boxes, default PET (d_node = 256), smearing 1.4, spacing 1.33, p = 5; ms per call on "
                          f"the host clock, median of {args.repeats} windows of {args.inner} calls after two warm-up calls"}
    result["box"] = box(args.atoms, ("ewald", "p3m"), dev, args.repeats, args.inner)
    if args.large > 0:
        result["large_box"] = box(args.large, ("p3m",), dev, args.repeats, args.inner)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh)

    def brief(v):
        return {a: brief(b) for a, b in v.items() if not isinstance(b, list) or a in ("mesh", "cell")} if isinstance(v, dict) else v

    print(json.dumps(brief(result)))


if __name__ == "__main__":
    main()
