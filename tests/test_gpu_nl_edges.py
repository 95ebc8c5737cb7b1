"""The device neighbour list (``pet_nl_build_batch``, csrc/nl.hip) at its structural edge cases (``-m gpu``): the inputs of
``nl_cases.py`` -- image-count and tile-overflow flushes, more than 64 centres in a bin, halved and capped bin counts, a
batch of open, periodic, thin and empty systems, pairs on the cutoff's last ulp, the host's refusals -- against the fp64
oracle ``oracle/nl.py``. ``test_nl_cases_cpu.py`` asserts that each case reaches the branch it is named for.

Pair sets are compared exactly. Vectors are compared bit for bit where the case is exact in fp32 (``nl_cases.DYADIC``) and
otherwise against the rounding of the expression the kernel evaluates, (r_j - r_i) + (Sa a + Sb b + Sc c): one subtraction,
three products, two sums and one add, each rounded once, so per component
|delta_k| <= 8 * 2^-24 * (|r_i,k| + |r_j,k| + sum_a |S_a c_a,k|), a factor 2 to spare."""
import functools

import numpy as np
import pytest
import torch

import nl_cases as nc
from oracle import nl as onl
from oracle import pet as opet

pytestmark = pytest.mark.gpu

TOL = 1e-5  # energies and dE/dR, the relmax convention of test_gpu_parity.py
SPECIES = [1, 6, 7, 8]


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from metatrain_amd import runtime

    return runtime


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(rt, dev):
    hypers = dict(opet.DEFAULT_HYPERS)
    params = opet.synthetic_params(hypers, SPECIES, {"energy": 1}, 0, torch.float32)
    m = rt.HipModel(hypers, SPECIES)
    m.load({k: v.to(dev) for k, v in params.items()}, "energy")
    return m


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / np.abs(b).max()


def _oracle_of(case, cutoff=None):
    i, j, s, d = onl.neighbor_list(case.positions.astype(np.float64), case.cell.astype(np.float64), case.pbc,
                                   case.cutoff if cutoff is None else cutoff)
    return np.column_stack([i, j, s]).astype(np.int64).reshape(-1, 5), d.reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """Rows ``(i, j, Sa, Sb, Sc)`` in lexicographic order and the fp64 vectors of a case, computed once and left unchanged."""
    rows, d = _oracle_of(nc.empty() if name == "empty" else nc.SINGLE[name])
    rows.setflags(write=False)
    d.setflags(write=False)
    return rows, d


def _device(rt, dev, case):
    pairs, vec = rt.neighbor_list(torch.from_numpy(case.positions).to(dev), torch.from_numpy(case.cell), list(case.pbc),
                                  case.cutoff)
    return pairs.cpu().numpy(), vec.cpu().numpy()


def _lexsort(rows):
    return np.lexsort((rows[:, 4], rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))


def _bits(x):
    return (np.ascontiguousarray(x, dtype=np.float32) + np.float32(0.0)).view(np.int32)  # -0.0 and +0.0 are one value


def _vector_bound(positions, cell, pbc, rows):
    c = np.where(np.asarray(pbc)[:, None], np.abs(cell.astype(np.float64)), 0.0)
    p = np.abs(positions.astype(np.float64))
    return 8.0 * 2.0 ** -24 * (p[rows[:, 0]] + p[rows[:, 1]] + np.abs(rows[:, 2:5]).astype(np.float64) @ c)


def _check_list(got, vec, positions, cell, pbc, ref_rows, ref_d, exact, label):
    """The properties every device list must have, against the oracle's rows and vectors (offsets already applied)."""
    got = got.astype(np.int64)
    assert got.shape == (len(ref_rows), 5) and vec.shape == (len(ref_rows), 3), f"{label}: {len(got)} pairs, oracle {len(ref_rows)}"
    assert np.all(np.diff(got[:, 0]) >= 0), f"{label}: rows are not grouped by centre in ascending order"
    order = _lexsort(got)
    srt = got[order]
    assert not np.any((srt[:, 0] == srt[:, 1]) & ~srt[:, 2:5].any(axis=1)), f"{label}: a row (i, i, 0)"
    assert not np.any(np.all(srt[1:] == srt[:-1], axis=1)), f"{label}: a duplicate row"
    assert np.array_equal(srt, ref_rows), f"{label}: the neighbour set differs from the oracle's"
    n = len(positions)
    assert np.array_equal(np.bincount(got[:, 0], minlength=n), np.bincount(ref_rows[:, 0], minlength=n))
    v = vec[order]
    if exact:
        assert np.array_equal(_bits(v), _bits(ref_d.astype(np.float32))), f"{label}: vectors are not bit-equal to fp32(oracle D)"
    else:
        excess = np.abs(v.astype(np.float64) - ref_d) - _vector_bound(positions, cell, pbc, ref_rows)
        assert excess.max(initial=-1.0) <= 0.0, f"{label}: a vector component misses its rounding bound by {excess.max():.3e}"
    _check_full_list(got, vec, label)


def _check_full_list(got, vec, label):
    """Every row (i, j, S) has its row (j, i, -S), and the two vectors are exact negatives."""
    mirror = np.column_stack([got[:, 1], got[:, 0], -got[:, 2:5]])
    a, b = _lexsort(got), _lexsort(mirror)
    assert np.array_equal(got[a], mirror[b]), f"{label}: not a full list"
    assert np.array_equal(_bits(vec[a]), _bits(-vec[b])), f"{label}: vectors of (i, j, S) and (j, i, -S) are not exact negatives"


@pytest.mark.parametrize("name", list(nc.SINGLE))
def test_edge_case_equals_oracle(rt, dev, name, monkeypatch):
    case = nc.SINGLE[name]
    calls = []
    if name == "lat125":  # 125 atoms not seen before: the first pair buffer holds 4 400 rows, the list has 11 500
        from metatrain_amd import _lib

        lib = _lib.load()
        build = lib.pet_nl_build_batch
        monkeypatch.setattr(lib, "pet_nl_build_batch", lambda *a: calls.append(int(a[9])) or build(*a))
        rt._nl_guess.pop(125, None)
    got, vec = _device(rt, dev, case)
    rows, d = _oracle(name)
    _check_list(got, vec, case.positions, case.cell, case.pbc, rows, d, name in nc.DYADIC, name)
    counts = np.bincount(got[:, 0], minlength=len(case.positions))
    if name in nc.PAIRS_TOTAL:
        assert len(got) == nc.PAIRS_TOTAL[name]
    if name in nc.PAIRS_PER_ATOM:
        assert (counts == nc.PAIRS_PER_ATOM[name]).all()
    if name.startswith("thin2"):
        assert counts.max() == 83
    if name == "sc1":
        assert not got[:, :2].any()
    if name == "lat125":  # the capacities of the two calls: the optimistic one, then what the first call counted
        assert calls == [4400, 11500] and rt._nl_guess[125] == 11500


def test_full_list_at_the_cutoff(rt, dev):
    """oncut: 3 750 of the 64 250 pairs within cutoff (1 + 1e-4) sit within 2e-5 cutoff of the cutoff, where fp32 rounding
    decides. Whatever it decides, it decides the same for (i, j, S) and (j, i, -S); everything outside that band is fixed."""
    case = nc.oncut()
    got, vec = _device(rt, dev, case)
    got = got.astype(np.int64)
    assert np.all(np.diff(got[:, 0]) >= 0)
    srt = got[_lexsort(got)]
    assert not np.any(np.all(srt[1:] == srt[:-1], axis=1)), "a duplicate row"
    assert not np.any((srt[:, 0] == srt[:, 1]) & ~srt[:, 2:5].any(axis=1)), "a row (i, i, 0)"
    _check_full_list(got, vec, "oncut")
    rows, d = _oracle_of(case, case.cutoff * (1 + 1e-4))
    dist = np.linalg.norm(d, axis=1)
    inside = {tuple(r) for r in rows[dist < case.cutoff * (1 - nc.BAND)].tolist()}
    allowed = {tuple(r) for r in rows[dist <= case.cutoff * (1 + nc.BAND)].tolist()}
    assert len(inside) == 60500 and len(allowed) - len(inside) == 3750
    device = {tuple(r) for r in got.tolist()}
    assert inside <= device, f"{len(inside - device)} pairs clearly inside the cutoff are missing"
    assert device <= allowed, f"{len(device - allowed)} pairs clearly outside the cutoff are listed"
    # the vectors of all rows, band included, against the oracle's
    index = {tuple(r): k for k, r in enumerate(rows.tolist())}
    ref = d[[index[tuple(r)] for r in got.tolist()]]
    excess = np.abs(vec.astype(np.float64) - ref) - _vector_bound(case.positions, case.cell, case.pbc, got)
    assert excess.max() <= 0.0


def _batch7_inputs(dev):
    systems = nc.batch7()
    first = np.concatenate([[0], np.cumsum([len(c.positions) for c in systems])]).tolist()
    pos = torch.from_numpy(np.concatenate([c.positions for c in systems])).to(dev)
    cells = torch.from_numpy(np.stack([c.cell for c in systems]))
    return systems, first, pos, cells, [list(c.pbc) for c in systems]


def test_batch_of_mixed_systems_is_the_concatenation_of_single_calls(rt, dev):
    """batch7: open, periodic, thin and empty systems in one call. Centres come out in atom order and an atom's neighbours in
    (bin, sorted-atom) order, neither depending on the system's bin base: rows and vectors equal those of the seven
    single-system calls one after the other, row for row and bit for bit."""
    systems, first, pos, cells, pbcs = _batch7_inputs(dev)
    pairs, vec = rt.neighbor_list_batch(pos, cells, pbcs, first, nc.CUTOFF)
    again, vagain = rt.neighbor_list_batch(pos, cells, pbcs, first, nc.CUTOFF)
    assert torch.equal(pairs, again) and torch.equal(vec.view(torch.int32), vagain.view(torch.int32))
    got, vec = pairs.cpu().numpy(), vec.cpu().numpy()
    single_rows, single_vec, ref_rows, ref_d = [], [], [], []
    for case, off in zip(systems, first):
        r, v = _device(rt, dev, case)
        assert r.shape == (len(_oracle(case.name)[0]), 5)
        shift = np.array([off, off, 0, 0, 0])
        single_rows.append(r + shift)
        single_vec.append(v)
        ref_rows.append(_oracle(case.name)[0] + shift)
        ref_d.append(_oracle(case.name)[1])
    ref_rows, ref_d = np.concatenate(ref_rows), np.concatenate(ref_d)
    assert len(got) == len(ref_rows)
    assert np.array_equal(got, np.concatenate(single_rows)), "the batched rows are not those of the single calls in order"
    assert np.array_equal(vec.view(np.int32), np.concatenate(single_vec).view(np.int32))
    # against the oracle: system by system (each system has its own cell for the vectors' bound)
    for k, case in enumerate(systems):
        lo, hi = np.searchsorted(got[:, 0], [first[k], first[k + 1]])
        rows, d = _oracle(case.name)
        sub = got[lo:hi] - np.array([first[k], first[k], 0, 0, 0])
        _check_list(sub, vec[lo:hi], case.positions, case.cell, case.pbc, rows, d, case.name in nc.DYADIC,
                    f"batch7[{k}] {case.name}")
    assert np.array_equal(got[_lexsort(got)], ref_rows)


def _species(n, k):
    return torch.tensor(SPECIES)[(torch.arange(n) * 5 + k) % 4].int()


@pytest.mark.parametrize("which", ["thin2", "batch7"])
def test_collate_graph_forward_backward_on_edge_cases(rt, model, dev, which):
    """The same lists through data.collate -> data.graph_of -> forward and backward: per-system energies and dE/dR against
    the fp64 oracle on the oracle's list. thin2 has up to 83 neighbours per atom and periodic self-images, whose reverse
    neighbour (i, i, S) <-> (i, i, -S) is the atom's own other entry; batch7 has an empty system between the others."""
    from metatrain_amd import data

    systems = [nc.thin2()] if which == "thin2" else nc.batch7()
    hypers = model.hypers
    assert float(hypers["cutoff"]) == nc.CUTOFF
    zs = [_species(len(c.positions), k) for k, c in enumerate(systems)]
    batch = data.collate([(torch.from_numpy(c.positions).to(dev), z.to(dev), torch.from_numpy(c.cell), list(c.pbc))
                          for c, z in zip(systems, zs)], nc.CUTOFF)
    graph = data.graph_of(model, batch)
    fw = rt.HipForward(model, graph)
    atomic = fw.forward()
    grad = fw.backward(torch.ones_like(atomic))
    energies = fw.sum_over_atoms(atomic).cpu().numpy()

    i_l, j_l, s_l, sys_l, off = [], [], [], [], 0
    for k, c in enumerate(systems):
        rows, _ = _oracle(c.name)
        i_l.append(torch.from_numpy(rows[:, 0] + off)); j_l.append(torch.from_numpy(rows[:, 1] + off))
        s_l.append(torch.from_numpy(rows[:, 2:5].copy()))
        sys_l.append(torch.full((len(c.positions),), k, dtype=torch.long))
        off += len(c.positions)
    i, j, s, sysidx = torch.cat(i_l), torch.cat(j_l), torch.cat(s_l), torch.cat(sys_l)
    assert graph.n_edges == len(i) and graph.max_neighbors == int(torch.bincount(i, minlength=off).max())
    params = opet.synthetic_params(hypers, SPECIES, {"energy": 1}, 0, torch.float64)
    p64 = torch.from_numpy(np.concatenate([c.positions for c in systems])).double().requires_grad_(True)
    c64 = torch.from_numpy(np.stack([c.cell for c in systems])).double()
    ref = opet.pet_atomic_energies(params, hypers, p64, c64, i, j, s, torch.cat(zs), sysidx)
    ref_e = torch.zeros(len(systems), dtype=torch.float64).index_add(0, sysidx, ref[:, 0])
    (gp,) = torch.autograd.grad(ref_e.sum(), p64)
    print(f"{which}: relmax E {relmax(energies, ref_e.detach().numpy()):.2e}, dE/dR {relmax(grad.cpu().numpy(), gp.numpy()):.2e}")
    assert relmax(energies, ref_e.detach().numpy()) < TOL
    assert relmax(atomic.cpu().numpy(), ref.detach().numpy().ravel()) < TOL
    assert relmax(grad.cpu().numpy(), gp.numpy()) < TOL
    if which == "batch7":
        assert energies[1] == 0.0


def test_host_refusals_leave_the_next_call_right(rt, dev):
    """What the host set-up refuses before any pair kernel is launched, each followed by an ordinary call."""
    case = nc.thin2()
    pos = torch.from_numpy(case.positions).to(dev)

    def ordinary():
        got, vec = _device(rt, dev, case)
        rows, d = _oracle(case.name)
        _check_list(got, vec, case.positions, case.cell, case.pbc, rows, d, False, "after a refusal")

    singular = torch.tensor([[5.0, 0, 0], [0, 0, 0], [0, 0, 5.0]])
    with pytest.raises(rt.PetHipError, match="singular cell"):
        rt.neighbor_list(pos, singular, [True] * 3, nc.CUTOFF)
    ordinary()
    with pytest.raises(rt.PetHipError, match="more than 100 times thinner"):
        rt.neighbor_list(pos, 0.04 * torch.eye(3), [True] * 3, nc.CUTOFF)
    ordinary()
    cells = torch.stack([torch.from_numpy(case.cell)] * 2)
    with pytest.raises(rt.PetHipError, match="first_atom must be non-decreasing"):
        rt.neighbor_list_batch(pos, cells, [[True] * 3] * 2, [0, 6, 4], nc.CUTOFF)
    ordinary()
