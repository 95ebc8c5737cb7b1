"""Graphs that put a given number of attention tokens on every atom, shared by ``test_attn_token_cases_cpu.py`` (the premises:
each case is what it says) and ``test_gpu_attn_token_edges.py`` (the device against the oracle ``oracle/pet.py``). No GPU import
at module level.

An atom's attention runs over T = neighbours + 1 tokens (token 0 is the centre token, token t >= 1 the atom's edge t - 1 in the
graph's order: edges stably sorted by centre), and T alone decides which kernel serves the atom -- see the dispatch table in
DESIGN.md. A case is one open system of well-separated clusters in which every atom of an m-atom cluster sees every other atom
of that cluster and nothing else: exactly m tokens.

A cluster is the first m points of a cubic grid ordered by distance from the origin, jittered, then
  * scaled so that its largest pair distance is ``D_MAX`` = 4.3 A (cutoff 4.5 A, width 0.5 A: pairs beyond 4.0 A carry
    fc < 1, i.e. a key bias log fc != 0), and
  * renumbered by a seeded permutation, which spreads those pairs over the 16-key tiles of an atom: without it they fall in the
    last two or three tiles only, and a bias read from the wrong slot of any other tile would change nothing.
Such a cluster is close to a ball, so only a few dozen of its pairs are that long, and whether one of them lands in a given tile
-- above all in a last tile of one token (m = 1 mod 16) -- depends on the seed. ``CLUSTER_SEED`` gives every cluster size the
smallest seed for which EVERY tile of the cluster holds a key with fc < 0.99 for some atom and a key with fc = 1 for some atom,
in the ordered and in the shuffled list (``first_covering_seed``; the premises test checks the coverage). A cluster's geometry,
species and shuffle depend on its size alone, so the 17- or 128-atom cluster is the same in every case that has one.

Clusters stand 30 A apart. Positions are rounded to fp32 once, here, and the oracle is given those values."""
import collections
import functools
import math

import numpy as np
import torch

TYPES = [1, 6, 7, 8]
CUTOFF, CUTOFF_WIDTH = 4.5, 0.5  # oracle.pet.DEFAULT_HYPERS (asserted by the premises test)
D_MAX = 4.3
SEPARATION = 30.0

# case -> cluster sizes
CASES = {
    "t64": [1, 2, 16, 17, 32, 33, 48, 49, 64],
    "t96": [1, 17, 65, 80, 81, 96],
    "t128": [1, 17, 97, 112, 113, 128],
    "t129": [33, 129],
    "so121": [3, 121],
    "so128": [3, 128],
}
FIRST_ORDER = ("t64", "t96", "t128", "t129")
SECOND_ORDER = ("so121", "so128")
# case -> (largest T, its 16-key tile count)
STATED = {"t64": (64, 4), "t96": (96, 6), "t128": (128, 8), "t129": (129, 9), "so121": (121, 8), "so128": (128, 8)}
# clusters below this size have no second key to compare a biased one with (1: no key; 2, 3: every pair is the longest or close)
COVERED_FROM = 16
# cluster size -> seed (first_covering_seed)
CLUSTER_SEED = {16: 0, 17: 1, 32: 0, 33: 15, 48: 0, 49: 1, 64: 0, 65: 3, 80: 0, 81: 11, 96: 0, 97: 38, 112: 0, 113: 8, 121: 1,
                128: 0, 129: 2}

System = collections.namedtuple("System", "positions species cells centers neighbors cell_shifts system_indices sizes cluster")
Cluster = collections.namedtuple("Cluster", "positions species order")


def bump(d):
    """fc of the default cutoff function (oracle.pet.cutoff_bump) in fp64"""
    x = np.clip((np.asarray(d, np.float64) - (CUTOFF - CUTOFF_WIDTH)) / CUTOFF_WIDTH, 1e-6, 1.0 - 1e-6)
    return 0.5 * (1.0 + np.tanh(1.0 / np.tan(math.pi * x)))


def make_cluster(m, seed, d_max=D_MAX):
    """[m, 3] float64 positions around the origin, species, and a sort key per directed pair (a, b), a != b, in row-major order,
    that puts the pairs in the shuffled list's order"""
    rng = np.random.default_rng([seed, m])
    k = np.arange(-4, 5)
    grid = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    by_distance = np.lexsort((grid[:, 2], grid[:, 1], grid[:, 0], (grid ** 2).sum(1)))
    p = grid[by_distance[:m]] + rng.uniform(-0.1, 0.1, (m, 3))  # at most 0.1 grid spacings per axis
    if m > 1:
        p = p * (d_max / np.linalg.norm(p[:, None] - p[None], axis=-1).max())
    p = p[rng.permutation(m)]
    return Cluster(p, np.array(TYPES)[rng.integers(0, 4, m)], rng.random(m * (m - 1)))


def cluster_pairs(m):
    a, b = np.nonzero(~np.eye(m, dtype=bool))
    return a, b


def tile_coverage(c, shuffled):
    """per 16-key tile of the cluster: (atoms with a key of fc < 0.99 in it, atoms with a key of fc = 1 in it). Token t >= 1 of an
    atom is its (t - 1)-th pair in list order."""
    m = len(c.positions)
    a, b = cluster_pairs(m)
    if shuffled:
        o = np.argsort(c.order, kind="stable")
        a, b = a[o], b[o]
    p = c.positions.astype(np.float32).astype(np.float64)
    fc = bump(np.linalg.norm(p[a] - p[b], axis=1))
    by_centre = np.argsort(a, kind="stable")
    token = np.empty(len(a), np.int64)
    token[by_centre] = np.arange(len(a)) % (m - 1) + 1
    return [(len(np.unique(a[(token // 16 == t) & (fc < 0.99)])), len(np.unique(a[(token // 16 == t) & (fc == 1.0)])))
            for t in range(-(-m // 16))]


def first_covering_seed(m, limit=100000):
    """the smallest seed whose m-atom cluster has both kinds of key in every tile, ordered and shuffled"""
    for seed in range(limit):
        c = make_cluster(m, seed)
        if all(lo > 0 and one > 0 for sh in (False, True) for lo, one in tile_coverage(c, sh)):
            return seed
    raise ValueError(m)


@functools.lru_cache(maxsize=None)
def system(case, shuffled=False, d_max=D_MAX):
    """The case as a ``System`` of torch tensors: fp32 positions, the full neighbour list (ordered by centre then neighbour, or
    in a seeded random order that interleaves the clusters), the stated token count of every atom and the index of its cluster.
    A ``d_max`` below 4.0 A gives every key fc = 1: the geometry the construction above is compared with."""
    pos, z, i_l, j_l, key, sizes, cluster, off = [], [], [], [], [], [], [], 0
    for k, m in enumerate(CASES[case]):
        c = make_cluster(m, CLUSTER_SEED.get(m, 0), d_max)
        pos.append(c.positions + np.array([SEPARATION * (k + 1), 0.0, 0.0]))
        z.append(c.species)
        a, b = cluster_pairs(m)
        i_l.append(a + off)
        j_l.append(b + off)
        key.append(c.order)
        sizes += [m] * m
        cluster += [k] * m
        off += m
    i, j = np.concatenate(i_l), np.concatenate(j_l)
    if shuffled:
        o = np.argsort(np.concatenate(key), kind="stable")
        i, j = i[o], j[o]
    cells = (torch.eye(3) * 1000.0)[None]  # an open system: no edge carries a shift, the cell enters nothing
    return System(torch.tensor(np.concatenate(pos), dtype=torch.float32), torch.tensor(np.concatenate(z)), cells,
                  torch.tensor(i), torch.tensor(j), torch.zeros(len(i), 3, dtype=torch.long), torch.zeros(off, dtype=torch.long),
                  np.array(sizes), np.array(cluster))


def inputs(case, shuffled=False, d_max=D_MAX):
    """the case as the ``inp`` dictionary the oracle helpers of test_gpu_train.py / test_gpu_hvp.py take"""
    s = system(case, shuffled, d_max)
    return {"positions": s.positions, "cells": s.cells, "centers": s.centers, "neighbors": s.neighbors,
            "cell_shifts": s.cell_shifts, "species": s.species, "system_indices": s.system_indices}


def distances(s):
    p = s.positions.double().numpy()
    return np.linalg.norm(p[s.centers.numpy()] - p[s.neighbors.numpy()], axis=1)


def key_slots(s):
    """(atom, token index of the key inside the atom's attention, fc) of every edge: the graph build sorts edges stably by centre
    and an atom's edge number e is its key e + 1"""
    i = s.centers.numpy()
    order = np.argsort(i, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=len(s.sizes)))])
    token = np.empty(len(i), np.int64)
    token[order] = np.arange(len(i)) - start[i[order]] + 1
    return i, token, bump(distances(s))


if __name__ == "__main__":  # the seed table
    print({m: first_covering_seed(m) for m in sorted({m for v in CASES.values() for m in v}) if m >= COVERED_FROM})
