"""SHA-256 digests of what the long-range operator computes in both of its modes (``csrc/ewald.hip``, ``csrc/p3m.hip`` and
the part they share, ``csrc/long_range.h``), for ``tests/test_gpu_long_range_digests.py``. The kernels are atomics-free in
every sum and launched in a fixed order, so every output has fixed bits: a change that is meant to move code between the
files and leave kernels, grids and launch order alone is checked to the bit, not to a tolerance.

Per case: fp32 V, dL/dq, dL/dR and dL/dcell, the workspace size (P3M: with the mesh and half-spectrum element counts) and
the k-vector count or the mesh shape of every system. The cases are those of ``tests/ewald_cases.py`` and
``tests/p3m_cases.py`` as the GPU tests run them, the whole model of ``ewald_cases.model_batch()`` under both methods, and a
plan without atoms. Only ``metatrain_amd`` calls; the case modules supply inputs, no oracle is evaluated.

  python tests/golden/make_long_range_digests.py COMMIT OUT.json

writes the record of the build in the tree, labelled with the commit it was built from. ``long_range_parent_digests.json``
is the record of the commit before ``csrc/long_range.h``; it is never regenerated from a later build."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(GOLDEN)
for _p in (os.path.dirname(TESTS), TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _ewald_oracle as eo  # noqa: E402  (collate, TYPES and the seeded featuriser weights: inputs only)
import ewald_cases as ec  # noqa: E402
import p3m_cases as pc  # noqa: E402

EWALD_RUNS = [(name, 24) for name in ec.OPERATOR_CASES + ("mixed",)]
EWALD_RUNS += [(name, channels) for name in ("open_tiles", "periodic_tiles") for channels in (3, 260)]
# (name, nodes) as test_gpu_p3m.CASE_RUNS at C = 24, then every channel width of the 43-atom system
P3M_RUNS = [(name, p, 24) for name in pc.OPERATOR_CASES for p in pc.case(name).nodes]
P3M_RUNS += [("channels", 5, channels) for channels in pc.CHANNELS]
METHODS = ("ewald", "p3m")
MODEL_NAMES = ("atomic", "energies", "grad", "cell_grad")


def sha(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
    return hashlib.sha256(a.tobytes()).hexdigest()


def ewald_key(name, channels):
    return f"{name}/C={channels}"


def p3m_key(name, nodes, channels):
    return f"{name}/p={nodes}/C={channels}"


def _plan_facts(op, n_systems, channels):
    from metatrain_amd import long_range as lr

    if isinstance(op, lr.P3MHip):
        return {"workspace_bytes": int(op.lib.pet_p3m_workspace_bytes(op.handle, channels)),
                "mesh_elements": int(op.lib.pet_p3m_mesh_elements(op.handle, channels)),
                "spectrum_elements": int(op.lib.pet_p3m_spectrum_elements(op.handle, channels)),
                "mesh_shapes": [op.mesh_shape(s) for s in range(n_systems)]}
    return {"workspace_bytes": int(op.lib.pet_ewald_workspace_bytes(op.handle, channels)),
            "num_kvectors": [op.num_kvectors(s) for s in range(n_systems)]}


def _operator_record(op, graph, b, q, gv, dev):
    got = ec.run(op, graph, b, q, gv, dev)
    rec = {"digests": {name: sha(t) for name, t in zip(ec.QUANTITIES, got)}}
    rec.update(_plan_facts(op, len(b["first_atom"]) - 1, int(q.shape[1])))
    return rec


def ewald_record(name, channels):
    dev = torch.device("cuda:0")
    c, b = ec.case(name), ec.batch(name)
    q, gv = ec.charges(name, channels)
    _, graph, op = ec.operator(b, dev, c.smearing, c.resolution, c.cutoff)
    return _operator_record(op, graph, b, q, gv, dev)


def p3m_record(name, nodes, channels):
    dev = torch.device("cuda:0")
    b = pc.batch(name)
    q, gv = pc.charges(name, channels)
    _, graph, op = pc.operator(b, dev, nodes)
    return _operator_record(op, graph, b, q, gv, dev)


def model_record(method):
    """``energy_and_gradient`` on ``ec.model_batch()`` as test_model_on_open_and_periodic_systems_and_after_an_md_step
    (Ewald) and test_long_range_model_under_p3m build it: seeded weights, the graph from the collated batch."""
    from metatrain_amd import long_range as lr
    from metatrain_amd import runtime as rt
    from oracle.pet import synthetic_params  # (seeded weights, as the tests draw them: nothing of the oracle is evaluated)

    dev = torch.device("cuda:0")
    hypers = pc.lr_hypers(5) if method == "p3m" else ec.lr_hypers(ec.SMEARING, ec.RESOLUTION)
    params = synthetic_params(hypers, eo.TYPES, {"energy": 1}, 0, torch.float32)
    b = ec.model_batch(False)
    model = rt.HipModel(hypers, eo.TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    graph = rt.HipGraph(model, b["positions"].float().to(dev), b["cells"].float().to(dev), b["centers"].to(dev),
                        b["neighbors"].to(dev), b["cell_shifts"].to(dev), b["species"].to(dev), b["system_indices"].int().to(dev))
    feat = lr.LongRangeFeaturizerHip.from_state_dict(hypers, eo.featurizer_params(hypers["d_node"], 0), device=dev, method=method)
    got = lr.energy_and_gradient(model, feat, graph, b["pbcs"], want_cell_grad=True)
    return {"digests": {name: sha(t) for name, t in zip(MODEL_NAMES, got)}}


def empty_record(method):
    """A plan without atoms (one periodic and one open system, both empty) through the adjoint's entry point itself (the
    Python wrappers cannot shape ``[0, C]`` rows): nothing is launched, and dL/dcell, given as NaN, comes back as zeros."""
    from metatrain_amd import runtime as rt
    from metatrain_amd._lib import check

    dev = torch.device("cuda:0")
    none = torch.zeros(0, 3, dtype=torch.float64)
    b = eo.collate([(none, torch.eye(3, dtype=torch.float64) * 9.0, ec.PERIODIC), (none, ec.NO_CELL.clone(), ec.OPEN)], ec.CUTOFF)
    _, graph, op = pc.operator(b, dev, 5) if method == "p3m" else ec.operator(b, dev)
    gcell = torch.full((2, 3, 3), float("nan"), dtype=torch.float32, device=dev)
    ws = op._ws(24, dev)
    tail = (rt._ptr(gcell), rt._ptr(ws), ws.numel(), rt._stream())
    if method == "p3m":
        check(op.lib.pet_p3m_backward(op.handle, graph.handle, None, None, None, 24, None, None, None, None, None, *tail))
    else:
        check(op.lib.pet_ewald_backward(op.handle, graph.handle, None, None, None, 24, None, None, *tail))
    rec = {"digests": {"grad_cells": sha(gcell)}, "grad_cells_max": float(gcell.abs().max())}
    rec.update(_plan_facts(op, 2, 24))
    return rec


def main():
    commit, path = sys.argv[1], sys.argv[2]
    record = {"commit": commit, "ewald": {}, "p3m": {}, "model": {}, "empty": {}}
    for method in METHODS:
        record["empty"][method] = empty_record(method)
        print("empty", method, "done", flush=True)
    for name, channels in EWALD_RUNS:
        record["ewald"][ewald_key(name, channels)] = ewald_record(name, channels)
        print("ewald", name, channels, "done", flush=True)
    for name, nodes, channels in P3M_RUNS:
        record["p3m"][p3m_key(name, nodes, channels)] = p3m_record(name, nodes, channels)
        print("p3m", name, nodes, channels, "done", flush=True)
    for method in METHODS:
        record["model"][method] = model_record(method)
        print("model", method, "done", flush=True)
    with open(path, "w") as fh:
        json.dump(record, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
