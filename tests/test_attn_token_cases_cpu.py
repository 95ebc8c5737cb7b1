"""The premises of ``attn_token_cases.py``, from the neighbour lists alone (no GPU): every atom has the stated token count, no
edge can cross the cutoff in fp32, every 16-key tile of every case holds keys with and without a cutoff bias for the ordered and
for the shuffled list, the tile counts and buckets are the stated ones, and ``so121`` is the first ``T_max`` whose second-order
reverse kernel needs the large-LDS opt-in as ``csrc/so.hip`` sizes it."""
import os
import re

import numpy as np
import pytest
import torch

import attn_token_cases as ac
from oracle import pet as opet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metatrain_amd", "csrc")
ORDERS = [False, True]


def _tokens(s):
    return np.bincount(s.centers.numpy(), minlength=len(s.sizes)) + 1


def test_the_cases_use_the_default_cutoff():
    h = opet.DEFAULT_HYPERS
    assert (h["cutoff"], h["cutoff_width"], h["cutoff_function"]) == (ac.CUTOFF, ac.CUTOFF_WIDTH, "Bump")
    d = np.array([0.5, 3.9, 4.0, 4.05, 4.2, 4.3, 4.4])
    assert np.array_equal(ac.bump(d), opet.cutoff_bump(torch.tensor(d), ac.CUTOFF, ac.CUTOFF_WIDTH).numpy())
    assert set(ac.CASES) == set(ac.STATED) == set(ac.FIRST_ORDER) | set(ac.SECOND_ORDER)


@pytest.mark.parametrize("shuffled", ORDERS, ids=["ordered", "shuffled"])
@pytest.mark.parametrize("case", list(ac.CASES))
def test_every_atom_has_the_stated_token_count(case, shuffled):
    s = ac.system(case, shuffled)
    assert len(s.sizes) == sum(ac.CASES[case]) == len(s.species) == len(s.positions)
    assert np.array_equal(_tokens(s), s.sizes)
    assert len(s.centers) == sum(m * (m - 1) for m in ac.CASES[case])
    # inside the cutoff by at least 0.1 A (fp32 cannot move an edge across it), nothing on top of another atom
    d = ac.distances(s)
    assert d.min() > 0.5 and d.max() < 4.4, (d.min(), d.max())
    # nothing between clusters; every edge has its reverse, once
    i, j = s.centers.numpy(), s.neighbors.numpy()
    assert np.array_equal(s.cluster[i], s.cluster[j]) and (i != j).all()
    n = len(s.sizes)
    fwd, rev = np.sort(i * n + j), np.sort(j * n + i)
    assert len(np.unique(fwd)) == len(fwd) and np.array_equal(fwd, rev)
    assert not s.cell_shifts.any()
    # the shuffled list is the same set of edges in another order, and not sorted by neighbour inside an atom
    o = ac.system(case, False)
    assert np.array_equal(np.sort(o.centers.numpy() * n + o.neighbors.numpy()), fwd)
    assert np.array_equal(o.positions.numpy(), s.positions.numpy())
    if shuffled:
        atom, token, _ = ac.key_slots(s)
        atom_o, token_o, _ = ac.key_slots(o)
        key = {(a, b): t for a, b, t in zip(i, j, token)}
        moved = sum(key[(a, b)] != t for a, b, t in zip(o.centers.numpy(), o.neighbors.numpy(), token_o))
        assert moved > 0.5 * len(i)  # the keys of an atom stand in other slots
        assert (np.diff(i) < 0).any() and (np.diff(s.cluster[i]) < 0).any()  # atoms and clusters interleaved


@pytest.mark.parametrize("shuffled", ORDERS, ids=["ordered", "shuffled"])
@pytest.mark.parametrize("case", list(ac.CASES))
def test_every_tile_holds_keys_with_and_without_a_cutoff_bias(case, shuffled):
    """For every tile index k below the largest tile count, over the atoms whose T reaches tile k: at least one has a key in
    tile k with fc < 0.99 (a bias below log 0.99, read from the wrong slot it changes the result) and at least one has a key
    there with fc = 1 (bias 0: a neighbour's bias read in its place changes the result too)."""
    s = ac.system(case, shuffled)
    atom, token, fc = ac.key_slots(s)
    assert token.min() == 1 and np.array_equal(np.bincount(atom, weights=token), s.sizes * (s.sizes - 1.0) / 2.0)
    nt = ac.STATED[case][1]
    assert token.max() // 16 == nt - 1
    for k in range(nt):
        in_tile = token // 16 == k
        low, one = np.unique(atom[in_tile & (fc < 0.99)]), np.unique(atom[in_tile & (fc == 1.0)])
        assert len(low) >= 1 and len(one) >= 1, (case, k, len(low), len(one))
    # the same inside every cluster of 16 atoms or more, for each of its own tiles: a one-token last tile (m = 1 mod 16) too
    for c, m in enumerate(ac.CASES[case]):
        for k in range(-(-m // 16) if m >= ac.COVERED_FROM else 0):
            in_tile = (s.cluster[atom] == c) & (token // 16 == k)
            low, one = np.unique(atom[in_tile & (fc < 0.99)]), np.unique(atom[in_tile & (fc == 1.0)])
            assert len(low) >= 1 and len(one) >= 1, (case, m, k, len(low), len(one))


def test_the_seed_table_is_what_the_search_gives():
    sizes = sorted({m for v in ac.CASES.values() for m in v if m >= ac.COVERED_FROM})
    assert sorted(ac.CLUSTER_SEED) == sizes
    assert {m: ac.first_covering_seed(m) for m in sizes} == ac.CLUSTER_SEED


@pytest.mark.parametrize("case", list(ac.CASES))
def test_tile_counts_and_buckets_are_the_stated_ones(case):
    s = ac.system(case)
    t = _tokens(s)
    t_max, nt = ac.STATED[case]
    assert t.max() == t_max == max(ac.CASES[case]) and -(-t_max // 16) == nt
    # csrc/graph.hip: bucket b = min(ceil((deg + 1) / 16), 5) - 1
    bucket = np.minimum(-(-t // 16), 5) - 1
    assert np.array_equal(bucket, np.minimum(-(-s.sizes // 16), 5) - 1)
    if case == "t64":  # both sides of every bucket edge, and the largest T of the preload kernels
        assert {m: int(np.minimum(-(-m // 16), 5) - 1) for m in ac.CASES[case]} == {
            1: 0, 2: 0, 16: 0, 17: 1, 32: 1, 33: 2, 48: 2, 49: 3, 64: 3}
    else:
        assert bucket.max() == 4
    # the dispatch regions (pet_fwd.hip forward_layers / pet_bwd.hip: nt <= 4 preload, 5 - 6 <6>, 7 - 8 <8>, > 8 size-generic)
    region = {"t64": nt <= 4, "t96": nt == 6, "t128": nt == 8, "t129": nt == 9, "so121": nt == 8, "so128": nt == 8}
    assert region[case]
    # a full last tile against a one-token last tile
    last = {m: (m - 1) % 16 + 1 for m in ac.CASES[case]}
    if case in ("t96", "t128"):
        assert sorted(v for m, v in last.items() if m > 64) == [1, 1, 16, 16]


def test_the_comparison_geometry_has_no_cutoff_bias():
    """``d_max = 3.9``: the same clusters, every key at fc = 1 -- what the scaled construction is compared with."""
    s = ac.system("t128", False, 3.9)
    d = ac.distances(s)
    assert d.min() > 0.5 and d.max() < 3.95 and (ac.bump(d) == 1.0).all()
    assert np.array_equal(_tokens(s), s.sizes)


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_so121_is_the_first_size_under_the_lds_opt_in():
    """``k_attn_rev`` takes ``T_max * (8 HD + 2 + 6)`` floats of dynamic LDS (so.hip backward_train2); ``allow_big_lds``
    (common.h) opts in above 64 KiB; the pass refuses ``T_max`` > 128. Read from the sources, so that a change of the formula
    that moves the first size under the opt-in away from 121 fails here."""
    model_h, so, common = _read("model.h"), _read("so.hip"), _read("common.h")
    d = int(re.search(r"constexpr int D = (\d+);", model_h).group(1))
    nhead = int(re.search(r"constexpr int NHEAD = (\d+);", model_h).group(1))
    assert re.search(r"constexpr int HD = D / NHEAD;", model_h)
    hd = d // nhead
    assert hd == 16
    m = re.search(r"const size_t lds_rev = \(size_t\)T_max \* \(([0-9HD+* ]+)\) \* sizeof\(float\);", so)
    assert m, "so.hip no longer sizes k_attn_rev's LDS as T_max * (...) * sizeof(float)"
    per_token = 4 * eval(m.group(1), {"__builtins__": {}}, {"HD": hd})
    assert per_token == 544
    assert re.search(r"allow_big_lds\(k_attn_rev, lds_rev\);", so)
    assert re.search(r"const int T_max = g\.max_nbr \+ 1;", so)
    limit = re.search(r"if \(bytes > (\d+) \* (\d+)\)", common)
    limit = int(limit.group(1)) * int(limit.group(2))
    assert limit == 65536
    assert per_token * 120 <= limit < per_token * 121
    assert re.search(r"PET_REQUIRE\(g\.max_nbr \+ 1 <= 128, PET_ERR_UNSUPPORTED", so)
    assert ac.STATED["so121"][0] == 121 and ac.STATED["so128"][0] == 128
    assert per_token * 128 <= 160 * 1024  # the largest served size fits a CU's LDS
