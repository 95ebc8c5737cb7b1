"""SHA-256 digests of what the SOAP-BPNN pass (``csrc/soap.hip`` and the kernel files it launches) computes, for
``tests/test_gpu_soap_plan.py``. The kernels of the pass are atomics-free and launched in a fixed order, so every output has
fixed bits: a change of how the pass chooses its kernels that is meant to leave the launches alone is checked to the bit, not
to a tolerance.

Per case: per-atom energies, dE/dR, dE/dcell, the features where the forward hands them out, the workspace size and the
profiled stage names; the training cases add every parameter gradient, the tangent energies and the training workspace
size. The cases between them reach every value of the plan (``csrc/soap_plan.h``): every switch of the pass at 0 on the
64-atom four-type box of ``test_gpu_soap.py``, a forward that hands out its features, the type counts, buckets, rows and
cells of ``tests/soap_cases.py`` that change a kernel, the second instantiation of the expansion (``max_angular = 8``), a
third hidden layer, and the training pass behind a default (packed) forward. Only ``SoapBpnnHip`` calls; no oracle
evaluation (``oracle.soap`` gives the tables of settings and the seeded parameters).

A training batch above 1 024 atoms is no digest case: ``k_sp_fill`` orders the atoms of a bucket by workgroup arrival
there, so the summation order of the weight gradients is fixed only up to one workgroup (``chunks`` stays with its oracle
test).

  python tests/golden/make_soap_digests.py COMMIT OUT.json

writes the record of the build in the tree, labelled with the commit it was built from. ``soap_plan_parent_digests.json`` is
the record of the commit before ``csrc/soap_plan.h``; it is never regenerated from a later build."""
import contextlib
import functools
import hashlib
import itertools
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

TYPES = [1, 6, 7, 8]
SWITCHES = ("soap_packed", "soap_ps_mfma", "soap_pair", "soap_sorted", "soap_mfma")  # each 1 by default
BOX = ["default"] + [f"{k}=0" for k in SWITCHES] + ["features"]
# the routes whose energies must differ pairwise on the box, or a wrong route would pass unnoticed (asserted at record time)
DISTINCT = ["default", "soap_sorted=0", "soap_mfma=0", "soap_packed=0", "soap_pair=0"]
CATALOGUE = ["legacy_types_3", "legacy_types_5", "legacy_types_8", "legacy_types_9", "alchemical_types_9", "bucket_64_65_63_1",
             "bucket_0_0_0_130", "small_1", "small_5", "holes", "mixed", "lone_atom"]
MODELS = {"max_angular_8": dict(soap=dict(max_angular=8, max_radial=5)), "hidden_layers_3": dict(bpnn=dict(num_hidden_layers=3))}
TRAIN = ["legacy_types_1", "legacy_types_9", "alchemical_types_9", "bucket_70_0_1_0", "box/tangent", "box/energy_only"]
MAX_TRAIN_ATOMS = 1024  # one workgroup of k_sp_fill


def sha(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
    return hashlib.sha256(a.tobytes()).hexdigest()


@contextlib.contextmanager
def switches(spec):
    """``"key=value,key=value"`` through ``pet_config_set``; every key back at 1 afterwards."""
    from metatrain_amd import runtime as rt

    pairs = [kv.split("=") for kv in spec.split(",") if "=" in kv]
    try:
        for k, v in pairs:
            rt.config_set(k, int(v))
        yield
    finally:
        for k, _ in pairs:
            rt.config_set(k, 1)


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def box_inputs():
    """The 64-atom four-type periodic box of ``test_gpu_soap.py`` (seed 9) with the host neighbour list at 5 A."""
    from oracle import nl as onl
    from oracle import pet as opet

    pos, z, cell = opet.random_box(64, seed=9, dtype=torch.float64)
    i, j, s, _ = onl.neighbor_list(pos.numpy(), cell.numpy(), [True] * 3, 5.0)
    return {"positions": pos, "species": z, "cells": cell[None], "centers": torch.tensor(i), "neighbors": torch.tensor(j),
            "cell_shifts": torch.tensor(s).long(), "system_indices": torch.zeros(64, dtype=torch.long)}


def _graph(m, b):
    dev = _dev()
    return m.graph(b["positions"].float().to(dev), b["cells"].float().to(dev), b["centers"].to(dev), b["neighbors"].to(dev),
                   b["cell_shifts"].to(dev), b["species"].to(dev), b["system_indices"].int().to(dev))


@functools.lru_cache(maxsize=None)
def box_model(variant="default"):
    """The legacy four-type model on seeded parameters; ``variant``: a key of ``MODELS``."""
    from metatrain_amd.soap_bpnn import SoapBpnnHip
    from oracle import soap as osoap

    hypers = dict(osoap.DEFAULT_HYPERS, legacy=True)
    for key, delta in MODELS.get(variant, {}).items():
        hypers[key] = dict(hypers[key], **delta)
    params = osoap.synthetic_params(hypers, 4, osoap.basis(hypers)[0], 0, torch.float32)
    m = SoapBpnnHip(hypers, TYPES)
    m.load({k: v.to(_dev()) for k, v in params.items()})
    return m


def catalogue_model(name):
    import soap_cases as sc
    from metatrain_amd.soap_bpnn import SoapBpnnHip

    c = sc.case(name)
    m = SoapBpnnHip(c.hypers, c.types)
    m.load({k: v.to(_dev()) for k, v in sc.params(name).items()})
    return m


def _seed(n):
    """The seed of the reverse pass: U(0.5, 1.5) per atom."""
    return (torch.rand(n, generator=torch.Generator().manual_seed(11)) + 0.5).to(_dev())


def inference_record(m, b, features=False):
    """``soap_forward`` + ``soap_backward`` on one workspace: digests, workspace size, profiled stage names."""
    from metatrain_amd import runtime as rt

    g = _graph(m, b)
    rt.profile(True)
    try:
        out = m.forward(g, want_features=features)
        atomic, feats = out if features else (out, None)
        grad, gcell = m.backward(g, _seed(g.n_nodes), want_cell_grad=True)
        torch.cuda.synchronize()
        stages = sorted(r["name"] for r in rt.profile_report())
    finally:
        rt.profile(False)
    dig = {"atomic": sha(atomic), "grad": sha(grad), "cell_grad": sha(gcell)}
    if features:
        dig["features"] = sha(feats)
    return {"digests": dig, "workspace_bytes": int(m.lib.soap_workspace_bytes(m._handle, g.n_nodes, g.n_edges)),
            "stages": stages}


def box_record(case):
    with switches(case):
        return inference_record(box_model(), box_inputs(), features=case == "features")


def catalogue_record(name):
    import soap_cases as sc

    return inference_record(catalogue_model(name), sc.batch(name))


def model_record(variant):
    return inference_record(box_model(variant), box_inputs())


def train_record(case):
    """A default forward (packed where the model allows it), its adjoint, then ``soap_train_gradients`` with seeded per-atom
    seeds and, but for ``box/energy_only``, a seeded tangent direction."""
    if case.startswith("box/"):
        m, b = box_model(), box_inputs()
    else:
        import soap_cases as sc

        m, b = catalogue_model(case), sc.batch(case)
    n = b["positions"].shape[0]
    assert n <= MAX_TRAIN_ATOMS, (case, n)
    g = _graph(m, b)
    u = None
    if case != "box/energy_only":
        u = (0.1 * torch.randn(n, 3, generator=torch.Generator().manual_seed(13))).to(_dev())
    m.zero_grad()
    atomic = m.forward(g)
    grad, gcell = m.backward(g, torch.ones_like(atomic), want_cell_grad=True)
    tangent = m.train_gradients(g, _seed(n), u)
    torch.cuda.synchronize()
    dig = {"atomic": sha(atomic), "grad": sha(grad), "cell_grad": sha(gcell), "tangent_atomic": sha(tangent)}
    for key, t in m.grads().items():
        dig["grad/" + key] = sha(t)
    m.zero_grad()
    return {"digests": dig, "workspace_bytes": int(m.lib.soap_workspace_bytes(m._handle, g.n_nodes, g.n_edges)),
            "train_workspace_bytes": int(m.lib.soap_train_workspace_bytes(m._handle, g.n_nodes, g.n_edges))}


GROUPS = (("box", BOX, box_record), ("catalogue", CATALOGUE, catalogue_record), ("models", list(MODELS), model_record),
          ("train", TRAIN, train_record))


def main():
    commit, path = sys.argv[1], sys.argv[2]
    record = {"commit": commit}
    for group, cases, fn in GROUPS:
        record[group] = {}
        for case in cases:
            record[group][case] = fn(case)
            print(group, case, record[group][case].get("stages", ""), flush=True)
    with open(path, "w") as fh:
        json.dump(record, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for a, b in itertools.combinations(DISTINCT, 2):
        assert record["box"][a]["digests"]["atomic"] != record["box"][b]["digests"]["atomic"], \
            f"the energies of box/{a} and box/{b} have the same bits: a wrong route between them would pass"


if __name__ == "__main__":
    main()
