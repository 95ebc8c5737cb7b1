"""The premises of ``tests/soap_cases.py``, without a GPU: every case collates, evaluates in the fp64 oracle and keeps its
minimum distance, and reaches the counts it is named for -- computed from the collated batch and from ``n_per_l`` alone. A
broken case builder fails here and cannot pass as a kernel result in ``test_gpu_soap_edges.py``."""
import math

import pytest
import torch

import soap_cases as sc
from oracle import soap as osoap

KB = 1024


@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_case_collates_and_the_oracle_evaluates_it(name):
    c, b = sc.case(name), sc.batch(name)
    n, n_sys, e = b["positions"].shape[0], len(c.systems), len(b["centers"])
    assert b["first_atom"][-1] == n and len(b["first_atom"]) == n_sys + 1 and b["cells"].shape == (n_sys, 3, 3)
    assert b["species"].shape == (n,) and b["system_indices"].shape == (n,) and b["cell_shifts"].shape == (e, 3)
    assert set(b["species"].tolist()) <= set(c.types)
    assert torch.equal(b["positions"], b["positions"].float().double()) and torch.equal(b["cells"], b["cells"].float().double())
    for s in range(n_sys):  # pairs stay inside their system
        lo, hi = b["first_atom"][s], b["first_atom"][s + 1]
        mine = (b["centers"] >= lo) & (b["centers"] < hi)
        assert bool(((b["neighbors"][mine] >= lo) & (b["neighbors"][mine] < hi)).all())
    closest = min(sc.min_distance(p, cell, pbc) for p, _, cell, pbc in c.systems)
    assert closest >= sc.MIN_DISTANCE, (name, closest)
    if name == "chunks":  # (its fp64 evaluation is the training reference of the GPU file: shapes only here)
        print(name, "atoms", n, "pairs", e, "min d", closest)
        return
    ref = sc.reference(name)
    size = osoap.soap_size(osoap.basis(c.hypers)[0], len(c.types) if c.hypers["legacy"] else 4)
    shapes = {"atomic": (n,), "features": (n, size), "grad_positions": (n, 3), "grad_cells": (n_sys, 3, 3)}
    for key, shape in shapes.items():
        assert tuple(ref[key].shape) == shape and bool(torch.isfinite(ref[key]).all()), (name, key)
    counts = sc.neighbour_counts(b)
    print(name, "atoms", n, "pairs", e, "min d %.3f" % closest, "neighbours",
          (int(counts.min()), int(counts.max())) if n else None, "self-image pairs", sc.self_image_pairs(b))


def test_default_basis_is_the_one_the_dimensions_are_computed_from():
    assert osoap.basis(sc.LEGACY)[0] == sc.N_PER_L and sc.LEGACY["bpnn"] == {"num_hidden_layers": 2,
                                                                           "num_neurons_per_layer": 32, "layernorm": True}


@pytest.mark.parametrize("n_types", sc.TYPE_COUNTS_LEGACY)
def test_type_count_cases_hold_every_type_and_the_dimensions_they_rely_on(n_types):
    name = "legacy_types_%d" % n_types
    counts, n = sc.type_counts(name), sc.batch(name)["positions"].shape[0]
    assert len(counts) == n_types and min(counts) >= 1 and 40 <= n <= 70 and sc.batch(name)["pbcs"] == [[True] * 3]
    d = sc.model_dims(n_types, legacy=True)
    assert (d["C"], d["n_sets"], d["NCOEF"], d["S"], d["ncmax"]) == (n_types, n_types, 280 * n_types, 284 * n_types ** 2,
                                                                    8 * n_types)
    assert d["NCOEF"] <= 3072  # soap_model_create: NCOEF <= 256 * MAXK
    assert d["C"] != 4  # soap_pair_ok: the first-generation expansion kernels
    assert (d["ncmax"] <= 32) == (n_types <= 3) and d["ncmax"] < 128  # k_soap_ps_m<false> / k_soap_ps_w
    assert (d["ps_bwd_bytes"] <= 64 * KB) == (n_types <= 7)  # above: k_soap_ps_bwd
    assert d["NT"] == {1: 1, 2: 1, 3: 2, 5: 3, 8: 4, 9: 0, 10: 0}[n_types]
    assert d["lds_tail"] <= 160 * KB
    if n_types == 8:
        assert d["S"] == 18176 and d["ps_bwd_bytes"] == 81664
    if n_types >= 9:
        assert d["lds_tail"] == {9: 126096, 10: 147680}[n_types] and d["lds_tail"] > 64 * KB  # dynamic LDS above the default


def test_the_eleventh_legacy_type_is_beyond_the_compiled_limit():
    assert sc.model_dims(11, legacy=True)["NCOEF"] == 3080 > 3072


@pytest.mark.parametrize("n_types", sc.TYPE_COUNTS_ALCHEMICAL)
def test_alchemical_type_count_cases(n_types):
    name = "alchemical_types_%d" % n_types
    assert min(sc.type_counts(name)) >= 1 and len(sc.type_counts(name)) == n_types
    d = sc.model_dims(n_types, legacy=False)
    assert (d["C"], d["n_sets"], d["NCOEF"], d["S"], d["NT"]) == (4, 1, 1120, 4544, 1)


@pytest.mark.parametrize("name", sc.BUCKET_CASES)
def test_bucket_cases_have_their_counts(name):
    assert sc.type_counts(name) == sc.BUCKET_COUNTS[name]
    z = sc.batch(name)["species"]
    if len(set(z.tolist())) > 1 and len(z) > 3:  # the buckets are interleaved in atom order: perm is no identity
        assert not torch.equal(z, z.sort().values)


def test_small_boxes_cover_every_remainder_of_the_wave_per_atom_grids():
    sizes = [sc.batch("small_%d" % n)["positions"].shape[0] for n in sc.SMALL_N]
    assert sizes == list(sc.SMALL_N)
    assert {n % 4 for n in sizes} == {1, 2, 3} and {(n + 3) // 4 for n in sizes} == {1, 2}
    # N % 4 == 0 is what every other case of the path already runs (64, 96, 200 atoms); the edge-free N = 1 box has no pair
    assert len(sc.batch("small_1")["centers"]) == 0 and all(len(sc.batch("small_%d" % n)["centers"]) > 0 for n in sc.SMALL_N[1:])


def test_dense_lattice_rows_cross_a_block():
    b = sc.batch("dense_lattice")
    counts = sc.neighbour_counts(b)
    print("dense_lattice neighbours per centre", int(counts.min()), int(counts.max()))
    assert int(counts.min()) > 256 and int(counts.max()) < 320  # one row is longer than a 256-pair block
    assert sc.self_image_pairs(b) == 384
    assert max(sc.centre_spans(b)) == 2 and 1 in sc.centre_spans(b)  # a block lies inside one row, or across two


def test_cluster_spans_sit_on_the_staging_edge():
    b = sc.batch("cluster_spans")
    first = b["first_atom"]
    sizes = tuple(hi - lo for lo, hi in zip(first, first[1:]))
    assert sizes == sc.CLUSTER_SIZES and all(19 <= k <= 22 for k in sizes)
    counts = sc.neighbour_counts(b)
    assert torch.equal(counts, torch.cat([torch.full((k,), k - 1) for k in sizes]))  # every atom sees its whole cluster
    spans = set(sc.centre_spans(b))
    print("cluster_spans centre spans", sorted(spans))
    limit = 16384 // sc.model_dims(4, True)["NCOEF"]
    assert limit == 14 and {14, 15} <= spans


def test_holes_put_empty_rows_inside_a_blocks_span():
    b = sc.batch("holes")
    counts, ctr, e = sc.neighbour_counts(b), b["centers"], len(b["centers"])
    assert int((counts == 0).sum()) == len(sc.CLUSTER_SIZES)
    inside = 0
    for p in range(0, e, 256):
        lo, hi = int(ctr[p]), int(ctr[min(p + 255, e - 1)])
        inside += int((counts[lo:hi + 1] == 0).sum())
    assert inside >= 4


def test_mixed_batch_has_both_kinds_of_block_and_two_systems_without_pairs():
    b = sc.batch("mixed")
    first = b["first_atom"]
    assert first == [0, 64, 64, 124, 125] and b["pbcs"][3] == [False] * 3 and float(b["cells"][3].abs().max()) == 0.0
    spans = sc.centre_spans(b)
    print("mixed centre spans", sorted(set(spans)))
    assert max(spans) > 14 and min(spans) <= 14
    per_system = torch.bincount(b["system_indices"][b["centers"]], minlength=4).tolist()
    assert per_system[0] > 0 and per_system[2] > 0 and per_system[1] == 0 and per_system[3] == 0
    n, volume = 60, float(torch.det(b["cells"][2]))
    assert abs(n / volume - 0.006) < 1e-4


def test_cell_cases():
    b = sc.batch("lone_atom")
    assert b["positions"].shape[0] == 1 and sc.self_image_pairs(b) == 18 == len(b["centers"])
    ref = sc.reference("lone_atom")
    assert float(ref["grad_positions"].abs().max()) == 0.0 and float(ref["grad_cells"].abs().max()) > 1e-3
    b = sc.batch("two_atoms_slab")
    assert b["pbcs"] == [[True, True, False]] and bool((b["cell_shifts"][:, 2] == 0).all()) and len(b["centers"]) > 0
    assert bool((b["cell_shifts"][:, :2] != 0).any()) and float(b["cells"][0][1, 0]) != 0.0
    b = sc.batch("left_handed")
    assert float(torch.det(b["cells"][0])) < 0.0 and b["positions"].shape[0] == 30
    b = sc.batch("sheared_batch")
    assert b["cells"].shape[0] == 3 and all(float(torch.det(c)) > 0 for c in b["cells"])
    off_diagonal = [c - torch.diag(torch.diag(c)) for c in b["cells"]]
    assert all(float(o.abs().max()) > 1.0 for o in off_diagonal)
    gc = sc.reference("sheared_batch")["grad_cells"]
    assert all(float(gc[s].abs().max()) > 1e-3 for s in range(3))


def test_chunk_case_splits_into_two_chunks():
    b = sc.batch("chunks")
    n = b["positions"].shape[0]
    assert n == 1030 and math.ceil(n / 1024) == 2 and sc.type_counts("chunks") == (1, 343, 343, 343)
    assert min(sc.type_counts("chunks")) < math.ceil(n / 1024)  # a bucket smaller than the chunk count
    volume = float(torch.det(b["cells"][0]))
    assert abs(n / volume - 0.02) < 1e-4
    print("chunks pairs", len(b["centers"]))


def test_training_cases_are_catalogue_cases():
    assert set(sc.TRAINING_CASES) <= set(sc.ALL_CASES)
    # the types missing from a batch: torch leaves their networks' gradients None
    assert [t for t, c in zip(sc.TYPES4, sc.type_counts("bucket_70_0_1_0")) if c == 0] == [6, 8]
