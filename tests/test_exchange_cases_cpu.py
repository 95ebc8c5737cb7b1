"""The premises of ``exchange_cases.py``: each case is what it says. The host side of the per-layer exchange (``slab_partition``,
``slab_owner``, ``ExchangePlan``) over the oracle's neighbour list, the way ``test_pet_partition_cpu.py`` builds its
``_CsrGraph``; no GPU."""
import functools

import numpy as np
import pytest
import torch

import exchange_cases as X
from metatrain_amd.partition import slab_owner, slab_partition
from metatrain_amd.pet.partition import ExchangePlan
from oracle import nl as onl
from test_pet_partition_cpu import _CsrGraph


def _pairs(pos, cell, pbc):
    i, j, s, _ = onl.neighbor_list(pos.double().numpy(), cell.double().numpy(), list(pbc), X.CUTOFF)
    return torch.tensor(np.concatenate([i[:, None], j[:, None], s], axis=1), dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def _plans(name, world):
    """per rank what ``energy_and_gradient_exchange`` sets up: ``(index, owned, plan or None, global (i, j) of the own rows,
    of the export rows, of the ghost rows)``"""
    c = X.CASES.get(name) or X.REFUSALS[name]
    pbc = list(c.pbc)
    owner = slab_owner(c.positions, c.cell, pbc, world)
    out = []
    for rank in range(world):
        index, owned, _ = slab_partition(c.positions, c.cell, pbc, X.CUTOFF, world, rank)
        assert bool((owner[index][owned] == rank).all()) and int(owned.sum()) == int((owner == rank).sum())
        if not index.numel():
            out.append((index, owned, None, torch.zeros((0, 2), dtype=torch.long), None, None))
            continue
        pairs = _pairs(c.positions[index], c.cell, pbc)
        pairs = pairs[owned[pairs[:, 0].long()] | owned[pairs[:, 1].long()]]
        g = _CsrGraph(pairs)
        plan = ExchangePlan(g, index, owned, owner, world, 4)
        key = torch.stack([index[g.ctr.long()], index[g.nbr.long()]], 1)
        out.append((index, owned, plan, key[owned[g.ctr.long()]], key[plan.export_rows.long()], key[plan.ghost_rows.long()]))
    return owner, out


def _peers(plan, world):
    if plan is None:
        return set(), set()
    return ({q for q in range(world) if plan.send_splits[q]}, {q for q in range(world) if plan.recv_splits[q]})


@pytest.mark.parametrize("name,world", X.CASE_WORLDS)
def test_ownership_is_a_partition_and_every_edge_has_one_rank(name, world):
    c = X.CASES[name]
    n = len(c.species)
    owner, ranks = _plans(name, world)
    assert owner.shape == (n,) and int(owner.min()) >= 0 and int(owner.max()) < world
    seen = torch.zeros(n, dtype=torch.long)
    for index, owned, *_ in ranks:
        seen[index[owned]] += 1
    assert bool((seen == 1).all())
    i, j, _ = X.neighbor_list(name)
    whole = i * n + j
    assert whole.unique().numel() == whole.numel(), "a pair connected by two images"
    own = torch.cat([r[3][:, 0] * n + r[3][:, 1] for r in ranks])
    assert own.numel() == whole.numel() and torch.equal(own.sort().values, whole.sort().values)
    # what rank a exports to rank b is, row for row, what b holds as ghost rows from a
    for a, (_, _, pa, _, ea, _) in enumerate(ranks):
        for b, (_, _, pb, _, _, gb) in enumerate(ranks):
            cnt = 0 if pa is None else pa.send_splits[b]
            assert cnt == (0 if pb is None else pb.recv_splits[a])
            if cnt:
                sa, sb = sum(pa.send_splits[:b]), sum(pb.recv_splits[:a])
                assert torch.equal(ea[sa:sa + cnt], gb[sb:sb + cnt])


def test_sizes_and_extents():
    assert X.TYPES == [1, 6, 7, 8] and X.CUTOFF == 4.5 and X.N_LAYERS == 2
    sizes = {"slab": 198, "triclinic": 198, "surface": 198, "surface_zero_row": 198, "unwrapped": 198, "cluster": 60,
             "isolated": 61, "isolated_alone": 61, "clustered": 40, "gap": 60}
    for name, c in X.CASES.items():
        assert c.positions.dtype == torch.float32 and set(c.species.tolist()) <= set(X.TYPES)
        assert name == "dense" or len(c.species) == sizes[name]
        full = torch.where(torch.tensor(c.pbc)[:, None], c.cell, torch.eye(3) * 1e3).double()
        vol = abs(float(torch.det(full)))
        for a in range(3):
            if c.pbc[a]:  # every periodic extent (plane spacing) above two cutoffs
                area = float(torch.linalg.norm(torch.linalg.cross(full[(a + 1) % 3], full[(a + 2) % 3])))
                assert vol / area > 2 * X.CUTOFF, (name, a)
        if not any(c.pbc):
            assert float(c.cell.abs().max()) == 0.0
    assert float(X.CASES["surface_zero_row"].cell[0].abs().max()) == 0.0
    cl = X.CASES["cluster"].positions
    assert torch.allclose(cl.max(0).values - cl.min(0).values, torch.tensor([16.0, 8.0, 8.0]), atol=0.5)
    assert float(cl[:, 0].max() - cl[:, 0].min()) == 16.0
    e = X.neighbor_list("slab")[0].numel()
    assert 3000 < e < 4500 and int(X.neighbor_counts("slab").max()) <= 32
    print(f"slab: {e} edges, at most {int(X.neighbor_counts('slab').max())} neighbours")


@pytest.mark.parametrize("world", X.CASES["slab"].worlds)
def test_slab_peers(world):
    _, ranks = _plans("slab", world)
    reach = (1, 2) if world == 12 else (1,)
    for r, (index, owned, plan, *_) in enumerate(ranks):
        want = {(r + s * k) % world for k in reach for s in (1, -1)} - {r}
        assert _peers(plan, world) == (want, want), (world, r, _peers(plan, world), want)
    if world == 2:  # both faces of a slab go to the one peer
        c = X.CASES["slab"]
        _, _, plan, _, export, _ = ranks[0]
        x = c.positions[export[:, 1], 0]
        assert bool((x < 18.0 + X.CUTOFF).any()) and bool((x > 36.0 - X.CUTOFF).any())
    if world == 12:  # rows to the peers two slabs away
        far = [plan.send_splits[(r + 2) % world] for r, (_, _, plan, *_) in enumerate(ranks)]
        far += [plan.send_splits[(r - 2) % world] for r, (_, _, plan, *_) in enumerate(ranks)]
        print("slab, world 12: rows to the peers two slabs away:", far)
        assert min(far) >= 1
    rows = [int(p[3].shape[0] + p[5].shape[0]) for p in ranks]
    print(f"slab, world {world}: rows per rank {rows}")


@pytest.mark.parametrize("name", ["triclinic", "unwrapped"])
def test_periodic_world_3_peers_are_everybody_else(name):
    _, ranks = _plans(name, 3)
    for r, (_, _, plan, *_) in enumerate(ranks):
        assert _peers(plan, 3) == ({0, 1, 2} - {r},) * 2


@pytest.mark.parametrize("name", ["surface", "surface_zero_row", "cluster", "isolated"])
def test_open_slab_axis_end_ranks_have_one_peer(name):
    _, ranks = _plans(name, 3)
    for r, want in enumerate(({1}, {0, 2}, {1})):
        assert _peers(ranks[r][2], 3) == (want, want), (name, r)


def test_zero_row_surface_is_the_surface():
    a, b = _plans("surface", 3), _plans("surface_zero_row", 3)
    assert torch.equal(a[0], b[0])
    for ra, rb in zip(a[1], b[1]):
        assert torch.equal(ra[0], rb[0]) and torch.equal(ra[4], rb[4]) and torch.equal(ra[5], rb[5])


def test_unwrapped_gives_the_plan_of_slab():
    a, b = _plans("slab", 3), _plans("unwrapped", 3)
    moved = (X.CASES["unwrapped"].positions - X.CASES["slab"].positions).abs().max(1).values
    assert float(moved.min()) >= 0.0 and float(moved.max()) > 2 * 36.0 - 1.0 and int((moved > 5.0).sum()) > 150
    assert torch.equal(a[0], b[0])
    for ra, rb in zip(a[1], b[1]):
        assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])
        assert ra[2].send_splits == rb[2].send_splits and ra[2].recv_splits == rb[2].recv_splits
        assert torch.equal(ra[2].export_rows, rb[2].export_rows) and torch.equal(ra[2].ghost_rows, rb[2].ghost_rows)
        for k in (3, 4, 5):
            assert torch.equal(ra[k], rb[k])


def test_clustered_leaves_three_ranks_empty():
    owner, ranks = _plans("clustered", 4)
    assert bool((owner == 1).all())
    for r in (0, 2, 3):
        assert ranks[r][0].numel() == 0 and ranks[r][2] is None
    assert ranks[1][0].numel() == 40 and _peers(ranks[1][2], 4) == (set(), set())


def test_gap_ranks_work_and_exchange_nothing():
    owner, ranks = _plans("gap", 2)
    assert torch.bincount(owner, minlength=2).tolist() == [30, 30]
    for index, owned, plan, own_rows, _, _ in ranks:
        assert index.numel() == 30 and bool(owned.all()) and own_rows.shape[0] > 0
        assert plan.send_splits == [0, 0] and plan.recv_splits == [0, 0]
        assert plan.export_rows.numel() == 0 and plan.ghost_rows.numel() == 0


def test_dense_reaches_the_64_slot_tiles_and_stays_on_the_tuned_path():
    counts = X.neighbor_counts("dense")
    print(f"dense: {len(counts)} atoms, neighbours {int(counts.min())} .. {int(counts.max())}")
    assert 33 <= int(counts.max()) <= 64 and int(counts.max()) < 127
    _, ranks = _plans("dense", 2)
    for r, (index, owned, plan, *_) in enumerate(ranks):
        assert _peers(plan, 2) == ({1 - r}, {1 - r})
        # the sub-system's own counts (halo atoms keep only their edges towards owned atoms): the owned rows are complete
        pairs = _pairs(X.CASES["dense"].positions[index], X.CASES["dense"].cell, [True] * 3)
        pairs = pairs[owned[pairs[:, 0].long()] | owned[pairs[:, 1].long()]]
        sub = torch.bincount(pairs[:, 0].long(), minlength=index.numel())
        assert torch.equal(sub[owned], counts[index[owned]]) and 33 <= int(sub.max()) <= 64


def test_isolated_atom():
    for name, alone in (("isolated", False), ("isolated_alone", True)):
        counts = X.neighbor_counts(name)
        assert int(counts[60]) == 0 and int(counts[:60].min()) > 0
        owner, ranks = _plans(name, 3)
        index, owned, plan, own_rows, _, _ = ranks[2]
        assert int(owner[60]) == 2
        if alone:  # all the rank owns; its halo atoms keep no edge, so its sub-system has none
            assert index[owned].tolist() == [60] and index.numel() > 1
            assert own_rows.shape[0] == 0 and plan.export_rows.numel() == 0 and plan.ghost_rows.numel() == 0
            assert _peers(ranks[1][2], 3) == ({0}, {0}) and _peers(ranks[0][2], 3) == ({1}, {1})
        else:
            assert int(owned.sum()) > 1 and own_rows.shape[0] > 0


def test_refusal_boxes():
    n = len(X.REFUSALS["two_images"].species)
    i, j, _ = X.neighbor_list("two_images")
    key = i * n + j
    assert key.unique().numel() < key.numel()
    with pytest.raises(ValueError, match="wider than two cutoffs"):
        _plans("two_images", 2)
    assert int(X.neighbor_counts("crowded").max()) > 127
    assert float(X.REFUSALS["crowded"].cell.diagonal().min()) > 2 * X.CUTOFF


def test_oracle_per_rank_gradients_add_up():
    """the per-rank oracles of the GPU suite: each adds up to the oracle's dE/dR over the ranks, a halo atom's entry is not
    zero, and the two differ (a rank of the exchange does not return the gradient of its owned energies)"""
    atomic, grad = X.oracle("cluster")
    scale = np.abs(grad).max()
    own = X.owner("cluster", 3).numpy()
    exchange, halo = X.rank_gradients("cluster", 3), X.owned_energy_gradients("cluster", 3)
    for parts in (exchange, halo):
        assert atomic.shape == (60,) and parts.shape == (3, 60, 3)
        assert np.abs(parts.sum(0) - grad).max() < 1e-12 * scale
        assert np.abs(parts[0][own == 1]).max() > 1e-3 * scale
    assert np.abs(exchange[0][own == 2]).max() == 0.0  # no row of rank 0 touches an atom two slabs away ...
    assert np.abs(halo[0][own == 2]).max() > 1e-6 * scale  # ... while its energies read that far
    assert np.abs(exchange - halo).max() > 1e-3 * scale
    e32, g32 = X.ref32("cluster")
    print(f"cluster: fp32 oracle against fp64: energies {e32:.2e}  dE/dR {g32:.2e}")
    assert e32 < 1e-4 and g32 < 1e-3
