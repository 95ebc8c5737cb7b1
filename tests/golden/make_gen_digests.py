"""SHA-256 digests of what the size-generic PET pass (``csrc/gen_common.h``, ``gen_walk.h``, ``gen.hip``,
``gen_train.hip``) computes, for ``tests/test_gpu_gen_walk.py``. The kernels of the path are atomics-free and their host
orchestration launches them in a fixed order, so every output has fixed bits: a change of the orchestration that is meant
to leave the launches alone is checked to the bit, not to a tolerance.

Per ``(case, input)`` pair of ``gen_shapes.PAIRS``: per-atom energies, dE/dR and (periodic input) dE/dcell through the
fused and through the staged calls; the flat parameter gradient of the energy-term pass and of the force-loss pass, with
the latter's tangent energies; the Hessian-vector product and its tangent; and the four workspace sizes. Beside the
pairs, two seeded steps of the multi-target trainer on ``flat32``: further targets beside the energy, and no fused
target at all. Only ``metatrain_amd.runtime`` calls and the models and inputs of the test modules; no oracle evaluation.

  python tests/golden/make_gen_digests.py COMMIT OUT.json

writes the record of the build in the tree, labelled with the commit it was built from. ``gen_walk_parent_digests.json``
is the record of the commit before ``gen_walk.h``; it is never regenerated from a later build."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.dirname(TESTS), TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gen_shapes as gs  # noqa: E402

WORKSPACES = ("pet_forward_workspace_bytes_for", "pet_train_workspace_bytes_for", "pet_train2_workspace_bytes_for",
              "pet_hvp_workspace_bytes_for")
STEPS = ("with_energy", "without_fused_target")


def sha(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
    return hashlib.sha256(a.tobytes()).hexdigest()


def _named(prefix, names, values):
    return {f"{prefix}_{n}": sha(v) for n, v in zip(names, values)}


def pair_record(tag, which):
    """{quantity: digest} and the workspace byte counts of one pair."""
    from metatrain_amd import runtime as rt
    from test_gpu_gen_shapes import _staged

    dev = torch.device("cuda:0")
    hypers, params, inp, nu, u, w = gs.case(tag, which)
    nu, u, w = nu.to(dev), u.to(dev), w.to(dev)
    model = rt.HipModel(hypers, gs.TYPES)
    model.load({k: v.to(dev) for k, v in params.items()}, "energy")
    graph = rt.HipGraph(model, inp["positions"].float().to(dev), inp["cells"].float().to(dev), inp["centers"].to(dev),
                        inp["neighbors"].to(dev), inp["cell_shifts"].to(dev), inp["species"].to(dev),
                        inp["system_indices"].int().to(dev))
    if "charge" in inp:
        graph.set_conditioning(inp["charge"].to(dev), inp["spin_multiplicity"].to(dev), inp["system_indices"].to(dev))
    cell = which == "a"
    names = ("atomic", "grad") + (("cell_grad",) if cell else ())
    ones = torch.ones(graph.n_nodes, device=dev)
    out = {}
    fw = rt.HipForward(model, graph)
    atomic = fw.forward()
    back = fw.backward(ones, want_cell_grad=cell)
    out.update(_named("fused", names, (atomic,) + (tuple(back) if cell else (back,))))
    out.update(_named("staged", names, _staged(rt, model, graph, cell)))
    fw = rt.HipForward(model, graph, train=True)
    model.zero_grad()
    fw.forward()
    fw.backward_train(w)
    out["energy_term_flat_grad"] = sha(model.flat_grad())
    model.zero_grad()
    fw.forward()
    fw.backward(ones)
    tangent = fw.backward_train2(ones, nu, u, want_tangent=True)
    out["force_loss_flat_grad"] = sha(model.flat_grad())
    out["force_loss_tangent"] = sha(tangent)
    hv = rt.hessian_vector_product(model, graph, u, want_cells=cell, want_tangent=True)
    out.update(_named("hvp", ("positions",) + (("cells",) if cell else ()) + ("tangent",), hv))
    torch.cuda.synchronize()
    sizes = {name: int(getattr(model.lib, name)(model.handle, graph.handle)) for name in WORKSPACES}
    return {"digests": out, "workspace_bytes": sizes}


def step_record(which):
    """One step of the multi-target trainer on ``flat32`` at learning rate 0: the flat gradient between the step's halves
    and the loss."""
    from test_gpu_multitarget_gen_train import _setup
    from test_gpu_multitarget_train import _inputs, _step

    with_energy = which == "with_energy"
    inp = _inputs(gs.GOLDEN)
    hypers, params, model, graph, fw = _setup("flat32", inp, "energy" if with_energy else None)
    step, args = _step(model, graph, fw, inp, with_energy=with_energy)
    step.begin(**args)
    flat = model.flat_grad().clone()
    out = step.end()
    return {"digests": {"flat_grad": sha(flat), "loss": sha(torch.as_tensor(out["loss"], dtype=torch.float32).reshape(1))}}


def main():
    commit, path = sys.argv[1], sys.argv[2]
    record = {"commit": commit, "pairs": {}, "steps": {}}
    for tag, which in gs.PAIRS:
        record["pairs"][f"{tag}-{which}"] = pair_record(tag, which)
        print(tag, which, "done", flush=True)
    for which in STEPS:
        record["steps"][which] = step_record(which)
        print(which, "done", flush=True)
    with open(path, "w") as fh:
        json.dump(record, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
