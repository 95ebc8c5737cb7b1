"""The fused attention block's row accesses (csrc/ablk_rows.h: one branch-free slot -> row map used by every row request,
residual read, row store and key-bias access of k_ablk_fwd4 / k_ablk_fwd<2> / k_ablk_bwd<1> / k_ablk_bwd<2>) on tiles of every
shape the map distinguishes. The change forms addresses differently and touches no arithmetic, so per-atom energies and dE/dR
must equal, to the bit, what the library computed before it.

One open system of well-separated clusters in which every atom sees every other atom of its cluster: an atom of an m-atom
cluster has exactly m tokens (its centre token + m - 1 neighbours). The fused kernels are forced onto it with the switches of
``tests/conftest.py``'s forced pass (``emlp_s = 2, attn_fused = 7``).
  clusters   sizes 1, 2, 2, 15, 16, 17, 31, 32 (32-slot tiles; the planner of csrc/graph.hip, restated below, pairs them into
             1 + 31, 2 + 17, 15 + 17 (exactly 32 slots), 15 + 16, 16 + 16 (exactly 32) and leaves 31s and 32s alone: 89 tiles,
             not a multiple of the four waves of a workgroup, so the last workgroup has dead waves) and 33, 64 (the 64-slot
             kernels: a second half that holds one token, and a full one)
  tiny       sizes 3, 5: four paired tiles, one workgroup without a dead wave
Each case also runs with its neighbour list shuffled. The graph build sorts edges by centre only, so an atom's neighbours then
stand in other slots and the sums over keys run in another order: the library before the map gave dE/dR of the shuffled list
1.7e-7 (clusters) and 5.9e-7 (tiny) away from the ordered one, not equal. "The same arrays" for the shuffled list is therefore
what that library computed on the shuffled list, to the bit, and the oracle's values within the 1e-5 bar.
A third case is the 10 000-atom golden box on the device neighbour list, under the default policy: the size at which a missing
wait state behind the row stores showed (see the test).

The fixtures ``tests/golden/ablk_rows_parent.npz`` (data only: ``<case>[_shuffled]_{atomic,grad}``) and
``ablk_rows_parent_box10000.npz`` (``atomic``, ``grad``) were written by this file
(``python tests/test_gpu_ablk_rows.py tests/golden``) with the library of the commit before the map."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import pet as opet  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5
TYPES = [1, 6, 7, 8]
CASES = {"clusters": [1, 2, 2, 15, 16, 17, 31, 32, 33, 64], "tiny": [3, 5]}
FORCED = {"emlp_s": 2, "attn_fused": 7}
DEFAULT = {"emlp_s": 1, "attn_fused": 3}
GOLDEN_FILE = "ablk_rows_parent.npz"


def plan_tiles(sizes):
    """(32-slot tiles as (TA, TB), number of 64-slot tiles): plan_attention_tiles of csrc/graph.hip on this system's histogram"""
    rem = [0] * 33
    big = 0
    for m in sizes:
        if m <= 32:
            rem[m] += m
        else:
            big += m
    tiles = []
    for lo in range(1, 33):
        while rem[lo] > 0 and lo <= 16:
            h = 32 - lo
            while h >= lo and not (rem[h] > 0 and (h != lo or rem[lo] >= 2)):
                h -= 1
            if h < lo:
                break
            n = rem[lo] // 2 if h == lo else min(rem[lo], rem[h])
            tiles += [(lo, h)] * n
            rem[lo] -= n
            rem[h] -= n
        tiles += [(lo, 0)] * rem[lo]
        rem[lo] = 0
    return tiles, big


def _system(case, shuffled):
    """positions, species and the full neighbour list of the case: a jittered 4 x 4 x 4 grid at 0.6 A spacing (3.1 A across,
    inside the 4.5 A cutoff) gives a cluster its first m points; clusters stand 30 A apart"""
    rng = np.random.default_rng(7 + len(CASES[case]))
    grid = 0.6 * np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    pos, i_l, j_l, off = [], [], [], 0
    for k, m in enumerate(CASES[case]):
        p = grid[rng.permutation(64)[:m]] + rng.uniform(-0.1, 0.1, (m, 3)) + np.array([30.0 * (k + 1), 0.0, 0.0])
        pos.append(p)
        a, b = np.nonzero(~np.eye(m, dtype=bool))
        i_l.append(a + off)
        j_l.append(b + off)
        off += m
    pos = np.concatenate(pos)
    i, j = np.concatenate(i_l), np.concatenate(j_l)
    d = np.linalg.norm(pos[i] - pos[j], axis=1)
    assert d.min() > 0.3 and d.max() < 4.4  # every atom of a cluster inside every other's cutoff, nothing on top of another
    if shuffled:
        perm = np.random.default_rng(99).permutation(len(i))
        i, j = i[perm], j[perm]
    z = torch.tensor(TYPES)[torch.tensor(rng.integers(0, 4, off))].int()
    cell = torch.eye(3) * 1000.0  # an open system: no edge carries a shift, the cell enters nothing
    return (torch.tensor(pos, dtype=torch.float32), z, cell[None], torch.tensor(i), torch.tensor(j),
            torch.zeros(len(i), 3, dtype=torch.long), torch.zeros(off, dtype=torch.long))


def _run(case, shuffled):
    """(atomic, grad) of two independent runs under the forced policy, and the stages that ran"""
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    hypers = dict(opet.DEFAULT_HYPERS)
    model = rt.HipModel(hypers, TYPES)
    model.load({k: v.to(dev) for k, v in opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32).items()}, "energy")
    pos, z, cells, i, j, s, sysidx = _system(case, shuffled)
    for k, v in FORCED.items():
        rt.config_set(k, v)
    try:
        graph = rt.HipGraph(model, pos.to(dev), cells.to(dev), i.int().to(dev), j.int().to(dev), s.int().to(dev), z.to(dev),
                            sysidx.int().to(dev))
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


_ORACLE = {}


def _oracle(case):
    """fp64 CPU oracle of the case (computed once; the shuffled list describes the same system)"""
    if case not in _ORACLE:
        hypers = dict(opet.DEFAULT_HYPERS)
        params = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
        p64 = {k: (v.double() if v.is_floating_point() else v) for k, v in params.items()}
        pos, z, cells, i, j, s, sysidx = _system(case, False)
        p = pos.double().clone().requires_grad_(True)
        a = opet.pet_atomic_energies(p64, hypers, p, cells.double(), i, j, s, z, sysidx)[:, 0]
        (g,) = torch.autograd.grad(a.sum(), p)
        _ORACLE[case] = (a.detach().numpy(), g.numpy())
    return _ORACLE[case]


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / np.abs(b).max()


def test_the_cases_reach_every_tile_shape():
    tiles, big = plan_tiles(CASES["clusters"])
    assert len(tiles) % 4 != 0 and big == 33 + 64  # a workgroup with dead waves; both 64-slot shapes
    assert {(16, 16), (15, 17)} <= set(tiles)  # pairs that fill the 32 slots exactly
    assert any(0 < tb and ta + tb < 32 for ta, tb in tiles) and any(tb == 0 for ta, tb in tiles)
    assert {(1, 31), (31, 0), (32, 0)} <= set(tiles)  # a centre token alone in front of a partner; full single tiles
    tiles, big = plan_tiles(CASES["tiny"])
    assert len(tiles) == 4 and big == 0


@pytest.mark.parametrize("shuffled", [False, True], ids=["ordered", "shuffled"])
@pytest.mark.parametrize("case", list(CASES))
def test_rows_equal_the_previous_addressing_to_the_bit(case, shuffled, golden_dir):
    assert torch.cuda.is_available(), "these tests need an MI355X"
    runs, stages = _run(case, shuffled)
    assert {"attn_blk", "attn_blk_bwd"} <= stages and not stages & {"qkv", "attn_fwd", "oproj", "attn_bwd", "qkv_bwd"}, stages
    (a0, g0), (a1, g1) = runs
    assert np.isfinite(a0).all() and np.isfinite(g0).all()
    # (c) two runs
    assert np.array_equal(a0, a1) and np.array_equal(g0, g1), "two runs of the same graph differ"
    # (a) the parent's arrays, to the bit
    gold = np.load(os.path.join(golden_dir, GOLDEN_FILE))
    key = case + ("_shuffled" if shuffled else "")
    atomic, grad = gold[key + "_atomic"], gold[key + "_grad"]
    assert a0.dtype == atomic.dtype and g0.dtype == grad.dtype and a0.shape == atomic.shape and g0.shape == grad.shape
    print(f"{key}: differing entries vs parent: atomic {(a0 != atomic).sum()} / {a0.size}, grad {(g0 != grad).sum()} / {g0.size}")
    assert np.array_equal(a0, atomic)
    assert np.array_equal(g0, grad)
    # (b) the CPU oracle
    a_ref, g_ref = _oracle(case)
    ea, eg = relmax(a0.ravel(), a_ref), relmax(g0, g_ref)
    print(f"{key}: vs fp64 oracle: atomic {ea:.2e}, grad {eg:.2e}")
    assert ea < TOL and eg < TOL


def _run_box10000(reps):
    """per-atom energies and dE/dR of the 10 000-atom golden box (default policy: the fused kernels serve it unforced) on the
    device neighbour list, `reps` builds of the graph"""
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    hypers = dict(opet.DEFAULT_HYPERS)
    model = rt.HipModel(hypers, TYPES)
    model.load({k: v.to(dev) for k, v in opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32).items()}, "energy")
    g = np.load(os.path.join(ROOT, "tests", "golden", "pet_default_box10000.npz"))
    pos, z, cell = torch.tensor(g["in_positions"]), torch.tensor(g["in_species"]), torch.tensor(g["in_cell"])
    sysidx = torch.zeros(10000, dtype=torch.int32)
    pairs, _ = rt.neighbor_list(pos.to(dev), cell, [True] * 3, 4.5)
    runs = []
    for _ in range(reps):
        graph = rt.HipGraph(model, pos.to(dev), cell[None].to(dev), pairs[:, 0].contiguous(), pairs[:, 1].contiguous(),
                            pairs[:, 2:5].contiguous(), z.to(dev), sysidx.to(dev))
        fw = rt.HipForward(model, graph)
        atomic = fw.forward().clone()
        grad = fw.backward(torch.ones_like(atomic)).clone()
        torch.cuda.synchronize()
        runs.append((atomic.cpu().numpy(), grad.cpu().numpy()))
    return runs


def test_rows_at_size_equal_the_previous_addressing_to_the_bit(golden_dir):
    """The same on a graph that fills the GPU (2 500 workgroups per launch). The row stores are inline assembly, which the
    compiler's hazard recognizer does not see: without the wait states behind a 16-B store (csrc/ablk.h ab_store16_if) the
    small cases above passed and a few rows of this box came out wrong in two runs of three. Four builds of the graph, each
    against ``tests/golden/ablk_rows_parent_box10000.npz`` (the library before the map, same inputs)."""
    assert torch.cuda.is_available(), "these tests need an MI355X"
    gold = np.load(os.path.join(golden_dir, "ablk_rows_parent_box10000.npz"))
    for k, (a, g) in enumerate(_run_box10000(4)):
        print(f"box10000 run {k}: differing entries vs parent: atomic {(a != gold['atomic']).sum()}, grad {(g != gold['grad']).sum()}")
        assert np.array_equal(a, gold["atomic"]) and np.array_equal(g, gold["grad"])


if __name__ == "__main__":  # write the fixture with the library that is built: python tests/test_gpu_ablk_rows.py DIR
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    arrays = {}
    for case in CASES:
        for shuffled in (False, True):
            runs, stages = _run(case, shuffled)
            assert {"attn_blk", "attn_blk_bwd"} <= stages, stages
            assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
            key = case + ("_shuffled" if shuffled else "")
            arrays[key + "_atomic"], arrays[key + "_grad"] = runs[0]
            print(key, runs[0][0].shape, runs[0][1].shape, sorted(stages), flush=True)
        same = np.array_equal(arrays[case + "_atomic"], arrays[case + "_shuffled_atomic"]) and np.array_equal(
            arrays[case + "_grad"], arrays[case + "_shuffled_grad"])
        print(case, "shuffled list equal to the ordered one to the bit:", same,
              "relmax grad", relmax(arrays[case + "_shuffled_grad"], arrays[case + "_grad"]), flush=True)
        a_ref, g_ref = _oracle(case)
        print(case, "vs oracle", relmax(arrays[case + "_atomic"].ravel(), a_ref), relmax(arrays[case + "_grad"], g_ref), flush=True)
    np.savez(os.path.join(out, GOLDEN_FILE), **arrays)
    runs = _run_box10000(3)
    assert all(np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1]) for r in runs)
    np.savez(os.path.join(out, "ablk_rows_parent_box10000.npz"), atomic=runs[0][0], grad=runs[0][1])
