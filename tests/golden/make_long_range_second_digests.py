"""SHA-256 digests of the long-range operator's SECOND-ORDER surface in both of its modes, for
``tests/test_gpu_long_range_second_digests.py``: the counterpart of ``make_long_range_digests.py`` (first order). The kernels
are atomics-free and launched in a fixed order, so a change that is meant to move host code and leave kernels, grids and launch
order alone is checked to the bit, not to a tolerance.

  second       ``EwaldHip.second`` / ``P3MHip.second``: the three fp32 results, by cotangent halves and ``results`` selection
  second_cell  ``second_cell`` of both modes: the two results, by cotangent parts and ``results`` selection
  model        ``LongRangeForward.backward_train`` / ``backward_train2`` (``u``, ``u`` and ``u_cell``, ``u_cell`` alone):
               ``model.flat_grad()`` and the tangent; ``hessian_vector_product`` with and without ``lambda_atomic``
  double       a double backward through ``LongRangeFeaturizerHip.__call__``: the gradients of ``<u, dE/dR>``
  empty        a plan without atoms through the four second-order entry points and the three sweeps: ``PET_OK``

Beside the digests every record holds integers: the ``*_workspace_bytes`` values that bear on it and, for P3M, the transform
hook's call count of every call (a structural invariant of the launch lists). Only ``metatrain_amd`` calls; the case modules
supply inputs, no oracle is evaluated.

  python tests/golden/make_long_range_second_digests.py COMMIT OUT.json

writes the record of the build in the tree, labelled with the commit it was built from. ``long_range_second_parent_digests.json``
is the record of the commit before the operator's one internal interface (``LrCall``, ``csrc/long_range.h``); it is never
regenerated from a later build."""
import functools
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
import _ewald_second_oracle as so  # noqa: E402  (seeded cotangents and featuriser inputs)
import _long_range_cell_oracle as co  # noqa: E402
import _long_range_train_oracle as lo  # noqa: E402
import _p3m_second_oracle as so2  # noqa: E402
import ewald_cases as ec  # noqa: E402
import p3m_cases as pc  # noqa: E402
from test_gpu_long_range_cell_second import EWALD_CASES as CELL_EWALD_CASES, MESH_CASES as CELL_MESH_CASES  # noqa: E402
from test_gpu_long_range_second import CASES as EWALD_CASES  # noqa: E402
from test_p3m_second_cpu import GPU_RUNS, HALF_RUN, HALVES  # noqa: E402

ALONE = [h for h in HALVES if h != "both"]
SINGLE3 = [(True, False, False), (False, True, False), (False, False, True)]
ALL3 = (True, True, True)
# (name, channels, halves)
EWALD_RUNS = [(n, c, "both") for n, c in EWALD_CASES] + [("periodic_tiles", 33, h) for h in ALONE]
# (name, nodes, channels, halves, results)
P3M_RUNS = [r + ("both", ALL3) for r in GPU_RUNS] + [HALF_RUN + (h, ALL3) for h in ALONE]
P3M_RUNS += [HALF_RUN + ("both", r) for r in SINGLE3 + [(True, False, True)]]
# (name, nodes, channels, parts, results); nodes = 0: the Ewald operator on ``ewald_cases``
PARTS = {"all": (True, True, True), "u_cells": (False, False, True), "no_cell": (True, True, False)}
CELL_VARIANTS = [("mixed", 0, 24), ("mixed", 5, 33)]  # one case per mode that takes the variants below
CELL_RUNS = [(n, 0, c, "all", (True, True)) for n, c in CELL_EWALD_CASES] + [(n, p, c, "all", (True, True)) for n, p, c in CELL_MESH_CASES]
for _n, _p, _c in CELL_VARIANTS:
    CELL_RUNS += [(_n, _p, _c, "u_cells", (True, True)), (_n, _p, _c, "no_cell", (True, True))]
    CELL_RUNS += [(_n, _p, _c, "all", (True, False)), (_n, _p, _c, "all", (False, True))]
METHODS = ("ewald", "p3m")
MODEL_CASES = [("odd33", "model_batch"), ("residual", "box"), ("odd33", "two_cells")]
MODEL_RUNS = [(m, tag, which) for m in METHODS for tag, which in MODEL_CASES]
SECOND_QUERIES = ("pet_ewald_second_workspace_bytes", "pet_ewald_second_cell_workspace_bytes", "pet_p3m_second_workspace_bytes",
                  "pet_p3m_second_cell_workspace_bytes")
SWEEP_QUERIES = ("pet_train2_long_range_workspace_bytes", "pet_train2_long_range_cell_workspace_bytes",
                 "pet_hvp_long_range_workspace_bytes")
D_NODE = 24


def sha(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
    return hashlib.sha256(a.tobytes()).hexdigest()


def _flags(f):
    return "".join("1" if x else "0" for x in f)


def ewald_key(name, channels, halves):
    return f"{name}/C={channels}/{halves}"


def p3m_key(name, nodes, channels, halves, results):
    return f"{name}/p={nodes}/C={channels}/{halves}/results={_flags(results)}"


def cell_key(name, nodes, channels, parts, results):
    return f"{name}/p={nodes}/C={channels}/{parts}/results={_flags(results)}"


def model_key(method, tag, which):
    return f"{method}/{tag}/{which}"


def _dev():
    return torch.device("cuda:0")


def _second_queries(op, channels):
    """The four second-order size queries on this handle (-1: the other mode's)."""
    return {q: int(getattr(op.lib, q)(op.handle, channels)) for q in SECOND_QUERIES}


@functools.lru_cache(maxsize=None)
def _operator(name, nodes):
    """One graph and one planned operator per (case, order); ``nodes = 0``: the Ewald operator on ``ewald_cases``."""
    from metatrain_amd import long_range as lr

    if nodes == 0:
        c, b = ec.case(name), ec.batch(name)
        _, graph, op = ec.operator(b, _dev(), c.smearing, c.resolution, c.cutoff)
        return op, graph, b
    b = pc.batch(name)
    _, graph = ec.graph(b, _dev())
    op = lr.P3MHip(pc.SMEARING, pc.SPACING, pc.CUTOFF, nodes, second_order=True).plan(b["cells"], b["pbcs"], b["first_atom"])
    return op, graph, b


def _record(op, channels, names, outs, calls_before):
    rec = {"digests": {n: sha(t) for n, t in zip(names, outs) if t is not None}, "formed": [t is not None for t in outs]}
    rec.update(_second_queries(op, channels))
    if hasattr(op, "transform_calls"):
        rec["transform_calls"] = op.transform_calls - calls_before
    return rec


def _second(name, nodes, channels, halves, results=None):
    op, graph, b = _operator(name, nodes)
    cases, oracle = (pc, so2) if nodes else (ec, so)
    q, gv = cases.charges(name, channels)
    u_q, u_r = oracle.cotangents(name, channels)
    pos, q, gv, u_q, u_r = (t.float().to(_dev()) for t in (b["positions"], q, gv, u_q, u_r))
    with_q, with_r = HALVES[halves]
    before = getattr(op, "transform_calls", 0)
    kw = {} if results is None else {"results": results}
    outs = op.second(graph, pos, q, gv, u_q if with_q else None, u_r if with_r else None, **kw)
    return _record(op, channels, so.NAMES, outs, before)


def ewald_record(name, channels, halves):
    return _second(name, 0, channels, halves)


def p3m_record(name, nodes, channels, halves, results):
    return _second(name, nodes, channels, halves, results)


def cell_record(name, nodes, channels, parts, results):
    """``second_cell``; ``no_cell`` (``u_cells=None``) also runs ``second`` and records whether its first two results have
    the same bits."""
    op, graph, b = _operator(name, nodes)
    cases = pc if nodes else ec
    q, gv = cases.charges(name, channels)
    u_q, u_r, u_c = co.cotangents(b, channels, 4400 if nodes else 4300)
    pos, q, gv, u_q, u_r, u_c = (t.float().to(_dev()) for t in (b["positions"], q, gv, u_q, u_r, u_c))
    p = PARTS[parts]
    before = getattr(op, "transform_calls", 0)
    outs = op.second_cell(graph, pos, q, gv, u_q if p[0] else None, u_r if p[1] else None, u_c if p[2] else None, results=results)
    rec = _record(op, channels, co.NAMES, outs, before)
    if parts == "no_cell":
        want = op.second(graph, pos, q, gv, u_q, u_r)
        rec["equals_second"] = all(torch.equal(a, b_) for a, b_ in zip(outs, want[:2]))
    return rec


def model_record(method, tag, which):
    """The sweeps of a whole model (``cell_tangents=True``; ``p3m``: with ``second_order=True``): ``flat_grad()`` and the
    tangent of every form, ``H u`` and its tangent, the three sweep size queries, and for P3M the hook calls of every call."""
    from metatrain_amd import long_range as lr
    from metatrain_amd import runtime as rt

    dev = _dev()
    hypers, params = lo.model_case(tag)
    batch = co.batch_of(which)
    model = rt.HipModel(hypers, eo.TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    graph = rt.HipGraph(model, batch["positions"].float().to(dev), batch["cells"].float().to(dev), batch["centers"].to(dev),
                        batch["neighbors"].to(dev), batch["cell_shifts"].to(dev), batch["species"].to(dev),
                        batch["system_indices"].int().to(dev))
    kw = dict(method="p3m", second_order=True) if method == "p3m" else {}
    feat = lr.LongRangeFeaturizerHip.from_state_dict(hypers, params, device=dev, cell_tangents=True, **kw)
    nu, u, uc = (t.float().to(dev) for t in co.seeds(which))
    ones = torch.ones(len(nu), device=dev)
    fw = lr.LongRangeForward(model, feat, graph, batch["pbcs"])
    op = feat.ewald
    rec = {"digests": {}, "transform_calls": {}}

    def step(name, call, *more):
        before = getattr(op, "transform_calls", 0)
        model.zero_grad()
        out = call()
        outs = out if isinstance(out, tuple) else (out,)
        for label, t in zip(more, outs):
            if t is not None:
                rec["digests"][f"{name}/{label}"] = sha(t)
        if name != "hvp" and name != "hvp_lambda":
            rec["digests"][f"{name}/flat_grad"] = sha(model.flat_grad())
        rec["transform_calls"][name] = getattr(op, "transform_calls", 0) - before

    step("train", lambda: fw.backward_train(nu))
    step("train_tangent", lambda: fw._sweep(None, nu, None, True), "tangent")
    step("train2_u", lambda: fw.backward_train2(ones, nu, u, want_tangent=True), "tangent")
    step("train2_u_ucell", lambda: fw.backward_train2(ones, nu, u, want_tangent=True, u_cell=uc), "tangent")
    step("train2_ucell", lambda: fw.backward_train2(ones, nu, None, want_tangent=True, u_cell=uc), "tangent")
    step("hvp", lambda: lr.hessian_vector_product(model, feat, graph, batch["pbcs"], u, want_tangent=True, replan=False),
         "hvp", "tangent")
    step("hvp_lambda", lambda: lr.hessian_vector_product(model, feat, graph, batch["pbcs"], u, lambda_atomic=nu + 1.0,
                                                         want_tangent=True, replan=False), "hvp", "tangent")
    for q in SWEEP_QUERIES:
        rec[q] = int(getattr(model.lib, q)(model.handle, graph.handle, op.handle))
    if method == "ewald":
        del rec["transform_calls"]
    return rec


def double_record(method):
    """``mixed`` at d_node = C = 24 as the GPU tests' force loss builds it: ``lr = featurizer(x, pos, cells, graph)``,
    ``F = d (W . lr).sum() / d pos`` under ``create_graph``, ``J = <u, F>``; dJ/dx, dJ/dpos and dJ/d(the six tensors)."""
    from metatrain_amd import long_range as lr

    dev = _dev()
    cases, oracle = (pc, so2) if method == "p3m" else (ec, so)
    b = cases.batch("mixed")
    kw = dict(method="p3m", second_order=True) if method == "p3m" else {}
    hypers = pc.lr_hypers(5, d_node=D_NODE) if method == "p3m" else ec.lr_hypers(d_node=D_NODE)
    feat = lr.LongRangeFeaturizerHip.from_state_dict(hypers, eo.featurizer_params(D_NODE), device=dev, **kw)
    feat.plan(b["cells"], b["pbcs"], b["first_atom"])
    _, graph = ec.graph(b, dev)
    x, weights, _ = (t.float().to(dev) for t in so.featurizer_inputs(b, D_NODE))
    u = oracle.cotangents("mixed", D_NODE)[1].float().to(dev)
    x.requires_grad_(True)
    pos = b["positions"].float().to(dev).requires_grad_(True)
    cells = b["cells"].float().to(dev)
    for k in feat.params:
        feat.params[k].requires_grad_(True)
    before = getattr(feat.ewald, "transform_calls", 0)
    energy = (weights * feat(x, pos, cells, graph)).sum()
    force, = torch.autograd.grad(energy, pos, create_graph=True)
    keys = [k[len("long_range_featurizer."):] for k in so.PARAM_KEYS]
    # (the last bias shifts the energy by a constant: no force depends on it, and autograd returns None for it)
    grads = torch.autograd.grad((u * force).sum(), [x, pos] + [feat.params[k] for k in keys], allow_unused=True)
    names = ["x", "positions"] + keys
    rec = {"digests": {n: sha(t) for n, t in zip(names, grads) if t is not None},
           "unused": [n for n, t in zip(names, grads) if t is None]}
    if method == "p3m":
        rec["transform_calls"] = feat.ewald.transform_calls - before
    return rec


def empty_record(method):
    """A plan without atoms (one periodic and one open system, both empty) through the second-order entry points of the
    handle's mode and the three sweeps, every device pointer null: the return codes (``PET_OK`` = 0) and, for P3M, the hook's
    call count (0: nothing is launched)."""
    from metatrain_amd import long_range as lr
    from metatrain_amd import runtime as rt

    dev = _dev()
    none = torch.zeros(0, 3, dtype=torch.float64)
    b = eo.collate([(none, torch.eye(3, dtype=torch.float64) * 9.0, ec.PERIODIC), (none, ec.NO_CELL.clone(), ec.OPEN)], ec.CUTOFF)
    hypers, params = lo.model_case("odd33")
    C = int(hypers["d_node"])
    model = rt.HipModel(hypers, eo.TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    graph = rt.HipGraph(model, b["positions"].float().to(dev), b["cells"].float().to(dev), b["centers"].to(dev),
                        b["neighbors"].to(dev), b["cell_shifts"].to(dev), torch.zeros(0, dtype=torch.int32, device=dev),
                        b["system_indices"].int().to(dev))
    lrh = hypers["long_range"]
    op = (lr.P3MHip(lrh["smearing"], lrh["kspace_resolution"], hypers["cutoff"], 5, second_order=True) if method == "p3m"
          else lr.EwaldHip(lrh["smearing"], lrh["kspace_resolution"], hypers["cutoff"]))
    op.plan(b["cells"], b["pbcs"], b["first_atom"])
    u = torch.zeros(1, dtype=torch.float32, device=dev)  # (a cotangent that is not NULL; never read: there is no atom)
    pre = "pet_p3m" if method == "p3m" else "pet_ewald"
    st, lib, mh, gh, eh = rt._stream(), op.lib, model.handle, graph.handle, op.handle
    rec = {"rc": {}}
    rec["rc"]["second"] = int(getattr(lib, pre + "_second")(eh, gh, None, None, None, rt._ptr(u), None, C, None, None, None, None, 0, st))
    rec["rc"]["second_cell"] = int(getattr(lib, pre + "_second_cell")(eh, gh, None, None, None, rt._ptr(u), None, None, C, None, None,
                                                                      None, 0, st))
    rec["rc"]["train2"] = int(lib.pet_backward_train2_long_range(mh, gh, eh, None, None, 0, None, None, None, None, st))
    rec["rc"]["train2_cell"] = int(lib.pet_backward_train2_long_range_cell(mh, gh, eh, None, None, 0, None, None, None, None, None, st))
    rec["rc"]["hvp"] = int(lib.pet_hessian_vector_long_range(mh, gh, eh, None, None, 0, None, None, None, None, st))
    rec.update(_second_queries(op, C))
    for q in SWEEP_QUERIES:
        rec[q] = int(getattr(lib, q)(mh, gh, eh))
    if method == "p3m":
        rec["transform_calls"] = op.transform_calls
    return rec


GROUPS = (("ewald", EWALD_RUNS, ewald_key, ewald_record), ("p3m", P3M_RUNS, p3m_key, p3m_record),
          ("second_cell", CELL_RUNS, cell_key, cell_record), ("model", MODEL_RUNS, model_key, model_record),
          ("double", [(m,) for m in METHODS], str, double_record), ("empty", [(m,) for m in METHODS], str, empty_record))


def main():
    commit, path = sys.argv[1], sys.argv[2]
    record = {"commit": commit}
    for group, runs, key, make in GROUPS:
        record[group] = {}
        for run in runs:
            record[group][key(*run)] = make(*run)
            print(group, key(*run), "done", flush=True)
    with open(path, "w") as fh:
        json.dump(record, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
