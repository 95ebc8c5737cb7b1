"""Bit identity of the ring kernels that read their weight fragments one stage ahead and their per-chunk biases through the
scalar cache (csrc/ablk.h ring_turn, ab_sload) against the schedule they replace. The change moves LDS reads, LDS-DMA
requests and bias loads in time; it keeps every product and the order of every sum, so per-atom energies and dE/dR must equal, to
the bit, what the library computed before the change.

The fixtures ``tests/golden/ring_parent_<case>_{atomic,grad}.npy`` were written by this file
(``python tests/test_gpu_ring_readahead.py tests/golden``) with the library of the commit before the read-ahead. The three
graphs are the smallest that reach every path of the kernels, which are forced onto them with the switches of
``tests/conftest.py``'s forced pass (``emlp_s = 2, attn_fused = 7``):
  box200      200 atoms, one box: one partial 128-row workgroup, a partial last tile, paired and single attention tiles
  box600      600 atoms: more than one workgroup per kernel
  batch2x300  two boxes of 300 atoms: the batch path
Synthetic weights (oracle.pet.synthetic_params, seed 0), random boxes (oracle.pet.random_box). Every graph runs twice and
the two runs must be equal too: a fragment read that races an LDS-DMA request shows as a run-to-run difference."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import nl as onl  # noqa: E402
from oracle import pet as opet  # noqa: E402

pytestmark = pytest.mark.gpu
TYPES = [1, 6, 7, 8]
CASES = {"box200": [(200, 11)], "box600": [(600, 12)], "batch2x300": [(300, 13), (300, 14)]}  # boxes of (atoms, seed)
FORCED = {"emlp_s": 2, "attn_fused": 7}
DEFAULT = {"emlp_s": 1, "attn_fused": 3}


def _inputs(case, hypers):
    pos_l, z_l, cell_l, i_l, j_l, s_l, sys_l, off = [], [], [], [], [], [], [], 0
    for k, (n, seed) in enumerate(CASES[case]):
        pos, z, cell = opet.random_box(n, seed=seed)
        i, j, s, _ = onl.neighbor_list(pos.numpy(), cell.numpy(), [True] * 3, hypers["cutoff"])
        pos_l.append(pos); z_l.append(z); cell_l.append(cell)
        i_l.append(torch.tensor(i) + off); j_l.append(torch.tensor(j) + off); s_l.append(torch.tensor(s).long())
        sys_l.append(torch.full((n,), k, dtype=torch.long))
        off += n
    return (torch.cat(pos_l), torch.stack(cell_l), torch.cat(i_l), torch.cat(j_l), torch.cat(s_l), torch.cat(z_l),
            torch.cat(sys_l))


def _run(case):
    """(atomic, grad) of two independent runs of the case under the forced policy, and the stages that ran"""
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    hypers = dict(opet.DEFAULT_HYPERS)
    model = rt.HipModel(hypers, TYPES)
    model.load({k: v.to(dev) for k, v in opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32).items()}, "energy")
    pos, cells, i, j, s, z, sysidx = _inputs(case, hypers)
    for k, v in FORCED.items():
        rt.config_set(k, v)
    try:
        graph = rt.HipGraph(model, pos.float().to(dev), cells.float().to(dev), i.int().to(dev), j.int().to(dev), s.int().to(dev),
                            z.to(dev), sysidx.int().to(dev))
        fw = rt.HipForward(model, graph)
        runs = []
        rt.profile(True)
        try:
            for _ in range(2):
                atomic = fw.forward().clone()
                grad = fw.backward(torch.ones_like(atomic)).clone()
                torch.cuda.synchronize()
                runs.append((atomic.cpu().numpy(), grad.cpu().numpy()))
            stages = {r["name"] for r in rt.profile_report()}
        finally:
            rt.profile(False)
    finally:
        for k, v in DEFAULT.items():
            rt.config_set(k, v)
    return runs, stages


@pytest.mark.parametrize("case", list(CASES))
def test_outputs_equal_the_previous_schedule_to_the_bit(case, golden_dir):
    assert torch.cuda.is_available(), "these tests need an MI355X"
    runs, stages = _run(case)
    assert {"emlp", "emlp_bwd"} <= stages  # the _s kernels served the small graph
    (a0, g0), (a1, g1) = runs
    assert np.isfinite(a0).all() and np.isfinite(g0).all()
    assert np.array_equal(a0, a1) and np.array_equal(g0, g1), "two runs of the same graph differ"
    atomic = np.load(os.path.join(golden_dir, f"ring_parent_{case}_atomic.npy"))
    grad = np.load(os.path.join(golden_dir, f"ring_parent_{case}_grad.npy"))
    assert a0.dtype == atomic.dtype and g0.dtype == grad.dtype
    assert np.array_equal(a0, atomic)
    assert np.array_equal(g0, grad)


if __name__ == "__main__":  # write the fixtures with the library that is built: python tests/test_gpu_ring_readahead.py DIR
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    for case in CASES:
        runs, stages = _run(case)
        assert {"emlp", "emlp_bwd"} <= stages, stages
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
        np.save(os.path.join(out, f"ring_parent_{case}_atomic.npy"), runs[0][0])
        np.save(os.path.join(out, f"ring_parent_{case}_grad.npy"), runs[0][1])
        print(case, runs[0][0].shape, runs[0][1].shape, sorted(stages), flush=True)
