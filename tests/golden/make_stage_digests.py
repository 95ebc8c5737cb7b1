"""SHA-256 digests of what the tuned first-order PET pass (default model size: ``csrc/pet_fwd.hip``, ``pet_bwd.hip`` and
the kernel files they launch) computes, for ``tests/test_gpu_stage_plan.py``. The kernels of the pass are atomics-free and
launched in a fixed order, so every output has fixed bits: a change of how the pass chooses its kernels that is meant to
leave the launches alone is checked to the bit, not to a tolerance.

Per case: per-atom energies, dE/dR, dE/dcell where the input is periodic, and the forward workspace size; the training
cases add the flat parameter gradient. The cases walk every form of every stage: the default policy and each fallback
behind ``pet_config_set`` on a 64-atom box, the 64-slot attention tiles, the architecture variants, the first-order
training pass, batches without edges and with isolated atoms, and one seeded box just above each row, atom and tile
threshold of the default policy. Only ``metatrain_amd.runtime`` calls; no oracle evaluation.

  python tests/golden/make_stage_digests.py COMMIT OUT.json

writes the record of the build in the tree, labelled with the commit it was built from. ``stage_plan_parent_digests.json``
is the record of the commit before ``csrc/pet_plan.h``; it is never regenerated from a later build."""
import contextlib
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

from metatrain_amd.synthetic import random_box, synthetic_params  # noqa: E402

TYPES = [1, 6, 7, 8]
DEFAULTS = {"trr_compress": 3, "attn_fused": 3}  # every other switch of the cases below: 1
# the nine settings of test_gpu_parity.test_alternative_kernel_paths_agree, then the row kernels off and forced
SMALL = ["default", "trr=0", "attn_fused=0", "side_stream=0", "trr_compress=0", "node_planes=0", "node_planes=2",
         "center_fused=0", "dxf_fused=0", "node_split=0", "emlp_s=0", "emlp_s=2,attn_fused=7", "save=0"]
DENSE = ["attn_fused=7", "attn_fused=0"]
VARIANTS = {"layernorm": dict(normalization="LayerNorm"), "postln": dict(transformer_type="PostLN"),
            "residual": dict(featurizer_type="residual"), "conditioning": dict(system_conditioning=True)}
VARIANT_CASES = [f"{tag}/{sw}" for tag in VARIANTS for sw in ("default", "trr=0")]
TRAIN = ["default", "trr=0", "emlp_s=2"]
EDGELESS = ["no_edges", "isolated_atoms"]
# the thresholds of the default policy (csrc/pet_plan.h): edge rows and atoms against EMLP_S_MIN_ROWS, 32-slot attention
# tiles against ABLK_MIN_TILES, atoms against the 32-row limit of the node kernels and the limit of their split form
MIN_ROWS, MIN_TILES, NODE_ROWS_ATOMS, SPLIT_TILES = 28672, 3840, 16384, 128
BOXES = ["below_1000", "edge_rows", "tiles", "split_off", "atoms_16384", "atoms_16385", "atoms_28672"]
BOX_SEED = 5


def sha(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
    return hashlib.sha256(a.tobytes()).hexdigest()


def hypers_of(**delta):
    from oracle.pet import DEFAULT_HYPERS  # (a table of settings: nothing of the oracle is evaluated)

    return dict(DEFAULT_HYPERS, **delta)


@contextlib.contextmanager
def switches(spec):
    """``"key=value,key=value"`` through ``pet_config_set``; every key back at its default afterwards."""
    from metatrain_amd import runtime as rt

    pairs = [kv.split("=") for kv in spec.split(",") if "=" in kv and not kv.startswith("save")]
    try:
        for k, v in pairs:
            rt.config_set(k, int(v))
        yield
    finally:
        for k, _ in pairs:
            rt.config_set(k, DEFAULTS.get(k, 1))


def _model(hypers):
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    model = rt.HipModel(hypers, TYPES)
    model.load({k: v.to(dev) for k, v in synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32).items()}, "energy")
    return model


_MODELS = {}


def default_model():
    if "default" not in _MODELS:
        _MODELS["default"] = _model(hypers_of())
    return _MODELS["default"]


def _golden_graph(model, name):
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    g = dict(np.load(os.path.join(GOLDEN, name)))
    t = lambda k: torch.tensor(g[k]).to(dev)  # noqa: E731
    graph = rt.HipGraph(model, t("in_positions").float(), t("in_cells").float(), t("in_centers"), t("in_neighbors"),
                        t("in_cell_shifts"), t("in_species"), t("in_system_indices").int())
    if "in_charge" in g:
        graph.set_conditioning(t("in_charge"), t("in_spin_multiplicity"))
    return graph


def box_graph(model, n, seed=BOX_SEED, density=0.05):
    """A seeded random periodic box with the neighbour list built on the device."""
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    pos, z, cell = random_box(n, seed, density=density)
    pairs, _ = rt.neighbor_list(pos.to(dev), cell, [True] * 3, model.hypers["cutoff"])
    return rt.HipGraph(model, pos.to(dev), cell.to(dev)[None], pairs[:, 0].contiguous(), pairs[:, 1].contiguous(),
                       pairs[:, 2:5].contiguous(), z.to(dev), torch.zeros(n, dtype=torch.int32, device=dev))


def _workspace_bytes(model, graph):
    return int(model.lib.pet_forward_workspace_bytes_for(model.handle, graph.handle))


def fused_record(model, graph, cell=True):
    """pet_forward + pet_backward: digests, the workspace size and the profiled stage names of the two calls."""
    from metatrain_amd import runtime as rt

    fw = rt.HipForward(model, graph)
    rt.profile(True)
    try:
        atomic = fw.forward()
        back = fw.backward(torch.ones_like(atomic), want_cell_grad=cell)
        torch.cuda.synchronize()
        stages = sorted(r["name"] for r in rt.profile_report())
    finally:
        rt.profile(False)
    out = {"atomic": sha(atomic), "grad": sha(back[0] if cell else back)}
    if cell:
        out["cell_grad"] = sha(back[1])
    return {"digests": out, "workspace_bytes": _workspace_bytes(model, graph), "stages": stages}


def small_record(spec):
    """The 64-atom box of ``pet_default_box64.npz`` under one setting of the switches (set before the graph is built: a
    small graph plans its attention tiles only when the fused block is forced)."""
    from metatrain_amd import runtime as rt
    from metatrain_amd.runtime import _ptr, _stream, check

    model = default_model()
    with switches(spec):
        graph = _golden_graph(model, "pet_default_box64.npz")
        if spec != "save=0":
            return fused_record(model, graph)
        fw = rt.HipForward(model, graph)  # save_for_backward = 0: the forward alone, nothing kept
        atomic = torch.empty((graph.n_nodes,), dtype=torch.float32, device=torch.device("cuda:0"))
        check(fw.lib.pet_forward(model.handle, graph.handle, _ptr(fw.workspace), fw.nbytes, 0, _ptr(atomic), None, None,
                                 _stream()))
        return {"digests": {"atomic": sha(atomic)}, "workspace_bytes": _workspace_bytes(model, graph)}


def dense_record(spec):
    """The 400-atom box of 36 neighbours per atom of test_gpu_parity.test_fused_attention_block_on_a_dense_box."""
    model = default_model()
    with switches(spec):
        return fused_record(model, box_graph(model, 400, seed=5, density=0.095))


def variant_record(case):
    """Inference of an architecture variant through the layered calls (test_gpu_variants._energy_and_gradient)."""
    from metatrain_amd import runtime as rt
    from test_gpu_variants import _energy_and_gradient

    tag, spec = case.split("/")
    if tag not in _MODELS:
        _MODELS[tag] = _model(hypers_of(**VARIANTS[tag]))
    model = _MODELS[tag]
    name = "pet_conditioning_feedforward.npz" if tag == "conditioning" else f"pet_variant_{tag}_box64.npz"
    with switches(spec):
        graph = _golden_graph(model, name)
        atomic, grad, nfs, efs = _energy_and_gradient(rt, model, graph)
        out = {"atomic": sha(atomic), "grad": sha(grad)}
        for l, (nf, ef) in enumerate(zip(nfs, efs)):
            out[f"node_features_{l}"] = sha(nf)
            out[f"edge_features_{l}"] = sha(ef)
        return {"digests": out, "workspace_bytes": _workspace_bytes(model, graph)}


def train_record(spec):
    """pet_forward(save_for_backward = 2) + pet_backward_train on the small graph of test_gpu_train.py."""
    from metatrain_amd import runtime as rt

    model = default_model()
    with switches(spec):
        graph = _golden_graph(model, "pet_default_box64.npz")
        w = (torch.rand(graph.n_nodes, generator=torch.Generator().manual_seed(7)) + 0.5).to(torch.device("cuda:0"))
        fw = rt.HipForward(model, graph, train=True)
        model.zero_grad()
        atomic = fw.forward()
        gpos, gcell = fw.backward_train(w, want_position_grad=True, want_cell_grad=True)
        out = {"atomic": sha(atomic), "grad": sha(gpos), "cell_grad": sha(gcell), "flat_grad": sha(model.flat_grad())}
        model.zero_grad()
        return {"digests": out, "workspace_bytes": int(model.lib.pet_train_workspace_bytes_for(model.handle, graph.handle))}


def edgeless_record(which):
    from metatrain_amd import runtime as rt

    model = default_model()
    dev = torch.device("cuda:0")
    if which == "no_edges":  # two systems of atoms out of each other's reach, no periodicity
        pos = torch.tensor([[0.0, 0, 0], [30.0, 0, 0], [0, 30.0, 0], [0, 0, 30.0], [30.0, 30.0, 0]], device=dev)
        e0 = torch.zeros(0, dtype=torch.int32, device=dev)
        graph = rt.HipGraph(model, pos, torch.zeros(2, 3, 3, device=dev), e0, e0, torch.zeros((0, 3), dtype=torch.int32, device=dev),
                            torch.tensor([1, 6, 8, 7, 1], dtype=torch.int32, device=dev),
                            torch.tensor([0, 0, 0, 1, 1], dtype=torch.int32, device=dev))
        assert graph.n_edges == 0
        return fused_record(model, graph, cell=False)
    graph = box_graph(model, 60, seed=21, density=0.004)  # a dilute box: some atoms see nobody
    deg = torch.bincount(graph._ctr.long(), minlength=60)
    assert graph.n_edges > 0 and int(deg.min()) == 0, "the dilute box has lost its isolated atoms"
    return fused_record(model, graph)


def _smallest(lo, hi, step, crosses):
    """Smallest lo + k step in (lo, hi] for which ``crosses`` holds, by bisection (``crosses(hi)`` must hold)."""
    assert crosses(hi) and not crosses(lo)
    while hi - lo > step:
        mid = lo + (hi - lo) // (2 * step) * step
        lo, hi = (lo, mid) if crosses(mid) else (mid, hi)
    return hi


def box_atoms():
    """Atom count of every threshold box: the smallest seeded box that crosses the threshold, found on the device."""
    from metatrain_amd import runtime as rt

    model = default_model()

    def fused(n):
        fw = rt.HipForward(model, box_graph(model, n))
        rt.profile(True)
        try:
            fw.forward()
            torch.cuda.synchronize()
            return "attn_blk" in {r["name"] for r in rt.profile_report()}
        finally:
            rt.profile(False)

    return {"below_1000": 1000,
            "edge_rows": _smallest(1000, 2400, 1, lambda n: box_graph(model, n).n_edges >= MIN_ROWS),
            "tiles": _smallest(MIN_TILES - 16, 8192, 16, fused),
            "split_off": 32 * SPLIT_TILES + 1, "atoms_16384": NODE_ROWS_ATOMS, "atoms_16385": NODE_ROWS_ATOMS + 1,
            "atoms_28672": MIN_ROWS}


def box_record(n):
    """The default policy on the seeded box of ``n`` atoms; the counts the policy compares are part of the record."""
    model = default_model()
    graph = box_graph(model, n)
    rec = fused_record(model, graph)
    rec.update(n_atoms=n, n_edges=graph.n_edges, max_neighbors=graph.max_neighbors)
    return rec


def refusal_graph():
    """The small forced graph of the refusal tests (``attn_fused`` is read when the graph is built)."""
    return _golden_graph(default_model(), "pet_default_box64.npz")


def main():
    commit, path = sys.argv[1], sys.argv[2]
    record = {"commit": commit, "small": {}, "dense": {}, "variants": {}, "train": {}, "edgeless": {}, "boxes": {}}
    for group, cases, fn in (("small", SMALL, small_record), ("dense", DENSE, dense_record),
                             ("variants", VARIANT_CASES, variant_record), ("train", TRAIN, train_record),
                             ("edgeless", EDGELESS, edgeless_record)):
        for case in cases:
            record[group][case] = fn(case)
            print(group, case, "done", flush=True)
    for name, n in box_atoms().items():
        record["boxes"][name] = box_record(n)
        print("box", name, n, record["boxes"][name]["n_edges"], record["boxes"][name]["stages"], flush=True)
    with open(path, "w") as fh:
        json.dump(record, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
