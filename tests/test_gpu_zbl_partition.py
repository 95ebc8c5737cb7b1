"""ONE box over several ranks with a ``zbl: true`` model (``pet/partition.py``, ``soap_bpnn/partition.py``): the ranks' partial
energies and gradients must add up to the same model's network-only result (``zbl=False`` / a model without ZBL) plus the
whole box's ZBL term from :class:`ZBLHip`, which ``tests/test_gpu_zbl.py`` pins to the reference. Bar: the project's
relmax < 1e-5 on the totals. The box is a jittered lattice (no pair below 1.1 A, so no single 1/r pair sets the scale) of
H, C, O and Cu, long enough along x for two slabs with (layers + 1)-cutoff halos that do not wrap onto themselves."""
import threading

import numpy as np
import pytest
import torch

from test_gpu_exchange import ThreadWorld

pytestmark = pytest.mark.gpu
TOL = 1e-5
TYPES = [1, 6, 8, 29]
WORLD = 2


def relmax(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.abs(a - b).max() / np.abs(b).max()
    print(f"    relmax {what}: {out:.3e} (scale {np.abs(b).max():.4g})")
    return out


@pytest.fixture(scope="module")
def box():
    """700 atoms on a 28 x 5 x 5 grid of spacing 2.15 A (0.10 atoms / A^3), each moved by up to 0.5 A per axis."""
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from metatrain_amd import runtime as rt
    from metatrain_amd.zbl import ZBLHip

    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(17)
    grid = torch.stack(torch.meshgrid(torch.arange(28), torch.arange(5), torch.arange(5), indexing="ij"), -1).reshape(-1, 3)
    pos = ((grid.float() + 0.5) * 2.15 + (torch.rand(grid.shape, generator=gen) - 0.5)).to(dev)
    cell = torch.diag(torch.tensor([28 * 2.15, 5 * 2.15, 5 * 2.15]))
    z = torch.tensor(TYPES)[torch.randint(0, 4, (pos.shape[0],), generator=gen)].int().to(dev)
    zbl = ZBLHip(TYPES)

    def whole_zbl(graph):
        atomic = zbl.forward(graph)
        assert int((atomic > 0).sum()) > 100 and float(atomic.sum()) > 10.0  # the term is there to be missed
        return float(atomic.double().sum()), zbl.backward(graph)

    return dict(dev=dev, rt=rt, pos=pos, cell=cell, z=z, whole_zbl=whole_zbl)


def _whole_graph(box, model, cutoff, soap=False):
    rt, dev = box["rt"], box["dev"]
    pairs, _ = rt.neighbor_list(box["pos"], box["cell"], [True] * 3, cutoff)
    args = (box["pos"], box["cell"][None].to(dev), pairs[:, 0].contiguous(), pairs[:, 1].contiguous(),
            pairs[:, 2:5].contiguous(), box["z"], torch.zeros(box["pos"].shape[0], dtype=torch.int32, device=dev))
    return model.graph(*args) if soap else rt.HipGraph(model, *args)


def _pet_model(box):
    from metatrain_amd.pet import default_hypers
    from metatrain_amd.synthetic import synthetic_params

    hypers = dict(default_hypers(), zbl=True)
    params = synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    model = box["rt"].HipModel(hypers, TYPES)
    model.load({k: v.to(box["dev"]) for k, v in params.items()}, "energy")
    return model


def _check(box, with_zbl, network, graph):
    e_zbl, g_zbl = box["whole_zbl"](graph)
    assert relmax([with_zbl[0]], [network[0] + e_zbl], "energy") < TOL
    assert relmax(with_zbl[1].cpu(), network[1].cpu().double() + g_zbl.cpu().double(), "dE/dR") < TOL


def test_pet_halo_partition_includes_zbl(box):
    from metatrain_amd.pet import partition

    model = _pet_model(box)

    def total(zbl):
        parts = [partition.energy_and_gradient(model, box["pos"], box["z"], box["cell"], [True] * 3, WORLD, r, zbl=zbl)
                 for r in range(WORLD)]
        assert sum(p[3] for p in parts) == box["pos"].shape[0]
        return sum(float(p[0]) for p in parts), sum(p[1] for p in parts)

    _check(box, total(None), total(False), _whole_graph(box, model, 4.5))  # None: hypers["zbl"] = True decides


def test_pet_per_layer_exchange_includes_zbl(box):
    from metatrain_amd.pet import partition

    rt, dev = box["rt"], box["dev"]
    model = _pet_model(box)
    rt.config_set("side_stream", 0)  # the rank threads share this process' streams
    try:
        def total(zbl):
            tw = ThreadWorld(WORLD)
            results, errors = [None] * WORLD, []

            def run(rank):
                try:
                    torch.cuda.set_device(dev)
                    results[rank] = partition.energy_and_gradient_exchange(
                        model, box["pos"], box["z"], box["cell"], [True] * 3, WORLD, rank, tw.all_to_all(rank), zbl=zbl)
                except BaseException as exc:  # noqa: BLE001
                    errors.append(exc)
                    tw.barrier.abort()

            threads = [threading.Thread(target=run, args=(r,)) for r in range(WORLD)]
            [t.start() for t in threads]
            [t.join() for t in threads]
            assert not errors, errors
            return sum(float(r[0]) for r in results), sum(r[1] for r in results)

        _check(box, total(None), total(False), _whole_graph(box, model, 4.5))
    finally:
        rt.config_set("side_stream", 1)


def test_soap_bpnn_partition_includes_zbl(box):
    from oracle import soap as osoap

    from metatrain_amd.soap_bpnn import SoapBpnnHip, partition

    hypers = dict(osoap.DEFAULT_HYPERS)
    params = {k: v.to(box["dev"]) for k, v in
              osoap.synthetic_params(hypers, len(TYPES), osoap.basis(hypers)[0], 0, torch.float32).items()}
    plain, with_zbl = SoapBpnnHip(hypers, TYPES), SoapBpnnHip(dict(hypers, zbl=True), TYPES)
    for m in (plain, with_zbl):
        m.load(params)

    def total(model):
        parts = [partition.energy_and_gradient(model, box["pos"], box["z"], box["cell"], [True] * 3, WORLD, r)
                 for r in range(WORLD)]
        return sum(float(p[0]) for p in parts), sum(p[1] for p in parts)

    _check(box, total(with_zbl), total(plain), _whole_graph(box, with_zbl, float(with_zbl.cutoff), soap=True))
