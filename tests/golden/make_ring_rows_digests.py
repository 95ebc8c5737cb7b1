"""SHA-256 digests of what the row kernels on the shared weight ring compute (``csrc/rows_s.h`` and the seven files that
include it) at the instantiations that ``make_stage_digests.py`` does not reach, for ``tests/test_gpu_ring_rows_digests.py``.
The kernels are atomics-free and launched in a fixed order, so every output has fixed bits: a change that is meant to move
the ring's protocol between files and leave kernels, grids and launch order alone is checked to the bit.

Every case runs under the forced policy (``emlp_s=2,attn_fused=7``: the ring kernels serve graphs of any size):

  layernorm     ``pet_variant_layernorm_box64.npz`` through the layered calls and through pet_forward / pet_backward:
                ``k_emlp_s<true>``, ``k_emlp_bwd_s<true, *>``, ``k_rowgemm_s_k2<2>``, the LayerNorm form of ``k_rowgemm_s_n2<1>``
  partial_tile  a seeded box whose edge count leaves 1 .. 31 rows to the last workgroup: a partial tile and three dead waves
  dead_waves    a seeded box whose edge count leaves exactly 32 rows: a full last tile and three dead waves
  second_order  the force-loss step of test_gpu_train (forward, adjoint, ``backward_train2``) on ``pet_default_box64.npz``:
                the generic ``k_rowgemm_s`` with and without addend, nk > 1 and nn > 1
  layers=1|2    a model of one GNN layer and the default one of two, inference and the first-order training pass:
                ``k_compress_bwd_s`` / ``k_comb_s`` first-layer and later-layer forms, ``k_comb_bwd_s`` with and without the addend

  python tests/golden/make_ring_rows_digests.py COMMIT OUT.json

writes the record of the build in the tree, labelled with the commit it was built from. ``ring_rows_parent_digests.json`` is
the record of the commit before the ring's protocol moved into ``csrc/rows_s.h`` (two recordings of that build agreed on every
quantity in it); it is never regenerated from a later build."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_stage_digests", os.path.join(GOLDEN, "make_stage_digests.py"))
sd = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sd)  # (puts the repository root and tests/ on sys.path)

FORCED = "emlp_s=2,attn_fused=7"
# (atoms, seed) of metatrain_amd.synthetic.random_box at density 0.05: the smallest boxes with these residues of the edge
# count, found on the CPU with oracle/nl.py (2458 = 19 x 128 + 26 and 2592 = 20 x 128 + 32 edges)
BOXES = {"partial_tile": (130, 1), "dead_waves": (136, 1)}
LAYERS = (1, 2)
CASES = ["layernorm", *BOXES, "second_order", *(f"layers={n}" for n in LAYERS)]


def _layers_model(n):
    key = f"layers={n}"
    if key not in sd._MODELS:
        sd._MODELS[key] = sd.default_model() if n == 2 else sd._model(sd.hypers_of(num_gnn_layers=n))
    return sd._MODELS[key]


def layernorm_record():
    rec = sd.variant_record(f"layernorm/{FORCED}")
    model = sd._MODELS["layernorm"]
    with sd.switches(FORCED):
        fused = sd.fused_record(model, sd._golden_graph(model, "pet_variant_layernorm_box64.npz"))
    rec["digests"].update({f"fused_{k}": v for k, v in fused["digests"].items()})
    rec["stages"] = fused["stages"]
    return rec


def box_record(name):
    n, seed = BOXES[name]
    model = sd.default_model()
    with sd.switches(FORCED):
        graph = sd.box_graph(model, n, seed=seed)
        rec = sd.fused_record(model, graph)
    rec.update(n_atoms=n, n_edges=graph.n_edges)
    return rec


def second_order_record():
    """test_gpu_train.test_force_loss_parameter_gradients_match_oracle_double_backward with emlp_s = 2, device side only."""
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    model = sd.default_model()
    with sd.switches("emlp_s=2"):
        graph = sd._golden_graph(model, "pet_default_box64.npz")
        n = graph.n_nodes
        gen = torch.Generator().manual_seed(11)
        nu = torch.rand(n, generator=gen) - 0.5
        u = torch.randn(n, 3, generator=gen)
        fw = rt.HipForward(model, graph, train=True)
        model.zero_grad()
        atomic = fw.forward()
        ones = torch.ones(n, device=dev)
        gpos = fw.backward(ones)
        tan = fw.backward_train2(ones, nu.to(dev), u.to(dev), want_tangent=True)
        out = {"atomic": sd.sha(atomic), "forces": sd.sha(gpos), "tangent": sd.sha(tan), "flat_grad": sd.sha(model.flat_grad())}
        model.zero_grad()
    return {"digests": out}


def layers_record(n):
    from metatrain_amd import runtime as rt

    model = _layers_model(n)
    with sd.switches(FORCED):
        graph = sd._golden_graph(model, "pet_default_box64.npz")
        rec = sd.fused_record(model, graph)
        w = (torch.rand(graph.n_nodes, generator=torch.Generator().manual_seed(7)) + 0.5).to(torch.device("cuda:0"))
        fw = rt.HipForward(model, graph, train=True)
        model.zero_grad()
        atomic = fw.forward()
        gpos, gcell = fw.backward_train(w, want_position_grad=True, want_cell_grad=True)
        rec["digests"].update(train_atomic=sd.sha(atomic), train_grad=sd.sha(gpos), train_cell_grad=sd.sha(gcell),
                              train_flat_grad=sd.sha(model.flat_grad()))
        model.zero_grad()
    return rec


def record(case):
    if case == "layernorm":
        return layernorm_record()
    if case in BOXES:
        return box_record(case)
    if case == "second_order":
        return second_order_record()
    return layers_record(int(case.split("=")[1]))


def main():
    commit, path = sys.argv[1], sys.argv[2]
    out = {"commit": commit, "cases": {}}
    for case in CASES:
        out["cases"][case] = record(case)
        print(case, "done", flush=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
