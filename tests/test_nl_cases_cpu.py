"""The neighbour-list edge cases of ``nl_cases.py`` on the CPU: each case still reaches the branch of ``nl.hip`` it is named
for (from the restated host set-up and the constants read out of the kernel source), the analytic pair counts hold, the two
oracles agree on the small cases, and the cases that the GPU test compares with ``==`` really are exact in fp32."""
import itertools

import numpy as np
import pytest

import nl_cases as nc
from oracle import nl as onl


def _oracle(case, cutoff=None):
    return onl.neighbor_list(case.positions.astype(np.float64), case.cell.astype(np.float64), case.pbc,
                             case.cutoff if cutoff is None else cutoff)


def test_image_count_flush_cases():
    """More occupied (bin, image) slots around one bin than ``NL_MAX_IMAGES``: reach >= 3 on some axis."""
    k = nc.kernel_constants()
    p = nc.plan(nc.sc1())
    assert p.nb == (1, 1, 1) and p.reach == (4, 4, 4) and p.max_slots == 729
    assert p.max_slots > 5 * k["NL_MAX_IMAGES"]  # several image-count flushes
    for case in (nc.thin2(), nc.thin2(unwrapped=True)):
        p = nc.plan(case)
        assert p.nb == (1, 1, 2) and p.reach == (4, 3, 1) and p.max_slots == 189
        assert p.max_slots > k["NL_MAX_IMAGES"] and max(p.reach) >= 3


def test_tile_overflow_and_many_centre_cases():
    k = nc.kernel_constants()
    for moved in (False, True):
        p = nc.plan(nc.lat216(moved))
        assert p.nb == (2, 2, 2) and p.reach == (1, 1, 1) and p.max_centres == 27 and p.max_slots == 27
        assert p.max_candidates == 729 > k["NL_TILE"] and p.max_slots <= k["NL_MAX_IMAGES"]  # overflow by candidates alone
        assert k["NL_TILE"] % 27 != 0  # the tile fills up part-way through the surrounding bins
    p = nc.plan(nc.lat125())
    assert p.nb == (1, 1, 1) and p.total_bins == 1 and p.max_centres == 125 > 64  # centres 64 + 61
    assert p.max_candidates == 3375 > 6 * k["NL_TILE"]  # `run` is carried over several flushes
    assert p.first_capacity == 4400 < nc.PAIRS_TOTAL["lat125"]  # the second, larger call of neighbor_list_batch
    # lat110: the overflow falls between the two loads (64 + 46) of one bin: 4 * 110 + 64 fits, the bin's remaining 46 do not
    p = nc.plan(nc.lat110())
    assert p.total_bins == 1 and p.max_centres == 110 and p.max_candidates == 27 * 110
    filled = 0
    while filled + 110 <= k["NL_TILE"]:
        filled += 110
    assert filled + 64 <= k["NL_TILE"] < filled + 110
    p = nc.plan(nc.open70())
    assert p.nb == (1, 1, 1) and p.max_centres == 70 > 64 and p.max_slots == 1
    p = nc.plan(nc.oncut())
    assert p.nb == (1, 1, 1) and p.reach == (1, 1, 1) and p.max_centres == 125 and p.max_candidates == 3375


def test_bin_halving_and_cap_cases():
    """``total_bins > n + 32``: the halving loop; 5000 A / 4.5 A = 1111 bins per axis are capped at 1024 first."""
    p = nc.plan(nc.sparse(200))
    assert p.uncapped_bins == 44 ** 3 > 5 + 32 and p.nb == (3, 3, 3) and p.total_bins <= 5 + 32
    p = nc.plan(nc.sparse(5000))
    assert p.uncapped_bins == 1111 ** 3 and 1111 > 1024 and p.nb == (2, 4, 4) and p.total_bins <= 5 + 32
    p = nc.plan(nc.sparse(200, periodic=False))
    assert p.uncapped_bins == 44 ** 3 and p.nb == (3, 3, 3) and p.reach == (1, 1, 1)
    # the pairs of sparse200: across a face, across a bin boundary, from an atom given outside the cell
    i, j, s, _ = _oracle(nc.sparse(200))
    rows = set(zip(i.tolist(), j.tolist(), map(tuple, s.tolist())))
    assert (0, 1, (-1, 0, 0)) in rows and (2, 3, (0, 0, 0)) in rows and (0, 4, (0, -1, -1)) in rows and len(rows) == 8
    c = nc.sparse(200)
    assert np.floor(c.positions[2] / (200.0 / 3)).tolist() != np.floor(c.positions[3] / (200.0 / 3)).tolist()


def test_batch7_mixes_the_upload_paths():
    systems = nc.batch7()
    assert [c.name for c in systems] == ["thin2", "empty", "open70", "slab60", "sc1", "sparse200", "wire40"]
    assert [len(c.positions) for c in systems] == [6, 0, 70, 60, 1, 5, 40]
    assert [c.pbc for c in systems] == [nc.PERIODIC, nc.PERIODIC, nc.OPEN, (True, True, False), nc.PERIODIC, nc.PERIODIC,
                                        (False, True, False)]
    frac = nc.slab60().positions.astype(np.float64) @ np.linalg.inv(np.asarray(nc.SLAB_CELL))
    assert frac.min() < -0.05 and frac.max() > 1.05  # atoms outside the cell on both sides


def test_analytic_pair_counts():
    # sc1: the integer vectors S with 0 < 1.5625 |S|^2 < 20.25, counted without the oracle
    expected = sorted(s for s in itertools.product(range(-4, 5), repeat=3) if 0 < 1.5625 * sum(x * x for x in s) < 20.25)
    assert len(expected) == 178 == nc.lattice_shell_count(1.25, 4.5)
    i, j, s, _ = _oracle(nc.sc1())
    assert not i.any() and not j.any() and sorted(map(tuple, s.tolist())) == expected
    # a = 1.5: |k|^2 <= 8, the shells (3,0,0) and (2,2,1) at exactly 4.5 A are excluded by the strict <
    assert nc.lattice_shell_count(1.5, 4.5) == 92
    assert sum(1 for k in itertools.product(range(-3, 4), repeat=3) if sum(x * x for x in k) == 9) == 30
    for name, total in nc.PAIRS_TOTAL.items():
        case = nc.SINGLE[name]
        i, j, s, _ = _oracle(case)
        assert len(i) == total, name
        counts = np.bincount(i, minlength=len(case.positions))
        if name in nc.PAIRS_PER_ATOM:
            assert (counts == nc.PAIRS_PER_ATOM[name]).all(), name
        if name.startswith("thin2"):
            assert counts.max() == 83 and (i == j).any()


def test_moved_atoms_change_the_shifts_only():
    a, b = nc.lat216(), nc.lat216(moved=True)
    wrap = np.rint((b.positions.astype(np.float64) - a.positions) / 9.0).astype(np.int64)
    assert np.array_equal(a.positions + (wrap * 9.0).astype(np.float32), b.positions)  # exact in fp32
    moved = np.abs(wrap).any(axis=1)
    assert moved.sum() == 72 and set(np.abs(wrap[moved]).ravel().tolist()) == {0, 1, 2}
    ia, ja, sa, da = _oracle(a)
    ib, jb, sb, db = _oracle(b)
    back = sb - (wrap[ib] - wrap[jb])  # r_b = r_a + wrap . cell, so S_b = S_a + wrap_i - wrap_j
    order = np.lexsort((back[:, 2], back[:, 1], back[:, 0], jb, ib))
    assert np.array_equal(ib[order], ia) and np.array_equal(jb[order], ja)
    assert np.array_equal(back[order], sa) and np.array_equal(db[order], da)
    assert not np.array_equal(sb[order], sa)


@pytest.mark.parametrize("name", [n for n, c in nc.SINGLE.items() if len(c.positions) <= 10])
def test_oracle_equals_bruteforce_on_small_cases(name):
    case = nc.SINGLE[name]
    fast = _oracle(case)
    slow = onl.neighbor_list_bruteforce(case.positions.astype(np.float64), case.cell.astype(np.float64), case.pbc, case.cutoff)
    assert len(fast[0]) > 0
    for x, y in zip(fast, slow):
        assert np.array_equal(x, y)


def test_oncut_band_is_small_and_unambiguous():
    case = nc.oncut()
    assert case.cell[0, 0] == np.float32(4.5) == np.float32(case.cutoff)  # fp32(0.9) * 5 rounds to the cutoff itself
    i, j, s, d = _oracle(case, case.cutoff * (1 + 1e-4))
    dist = np.linalg.norm(d, axis=1)
    band = np.abs(dist - case.cutoff) <= nc.BAND * case.cutoff
    inside = dist < case.cutoff * (1 - nc.BAND)
    assert len(i) == 64250 and band.sum() == 3750 and inside.sum() == 60500
    assert not (dist > case.cutoff * (1 + nc.BAND)).any()  # the next shell is 0.09 A away
    assert band.sum() / len(i) < 0.10  # 5.84 %: all that the GPU test may leave undecided
    # rounding decides the band pair by pair: in fp32 arithmetic some fall inside and some do not
    d2 = nc.fp32_d2(case, i[band], j[band], s[band])
    n_in = int((d2 < np.float32(case.cutoff) * np.float32(case.cutoff)).sum())
    assert n_in == 720 and 0 < n_in < band.sum()


@pytest.mark.parametrize("name", nc.DYADIC)
def test_dyadic_cases_are_exact_in_fp32(name):
    """Positions and cell taken as fp64 reproduce the fp32 d^2 bit for bit, no pair sits within the band around the cutoff
    except exactly on it, and no atom sits on a bin boundary."""
    case = nc.SINGLE[name]
    assert np.array_equal(case.positions * 4, np.rint(case.positions * 4)) and np.array_equal(case.cell * 4, np.rint(case.cell * 4))
    i, j, s, d = _oracle(case, case.cutoff * (1 + 1e-4))
    d2_64 = np.einsum("ij,ij->i", d, d)
    assert np.array_equal(nc.fp32_d2(case, i, j, s).astype(np.float64), d2_64)
    assert np.array_equal(d.astype(np.float32).astype(np.float64), d)
    near = np.abs(np.sqrt(d2_64) - case.cutoff) <= nc.BAND * case.cutoff
    assert (d2_64[near] == case.cutoff ** 2).all()
    p = nc.plan(case)
    c = nc.effective_cell(case.cell, case.pbc)
    frac = case.positions.astype(np.float64) @ np.linalg.inv(c)
    for a in range(3):
        if case.pbc[a]:
            x = (frac[:, a] - np.floor(frac[:, a])) * p.nb[a]
            # the device's fp32 fractional coordinate is off by a few 2^-24, times nb <= 4 bins: 1e-6 at the most
            assert np.abs(x - np.rint(x)).min() > 1e-5, "an atom on a bin boundary"


@pytest.mark.parametrize("name", [n for n in nc.SINGLE if n not in nc.DYADIC])
def test_other_cases_have_no_pair_that_rounding_decides(name):
    """Not exact in fp32, so set equality with the fp64 oracle needs every pair clear of the cutoff by more than the band.
    The periodic self-images (i, i, S) are exempt: their fp32 distance is |S . cell| of a dyadic cell, exact."""
    case = nc.SINGLE[name]
    i, j, s, d = _oracle(case, case.cutoff * (1 + 1e-4))
    dist = np.linalg.norm(d, axis=1)
    near = np.abs(dist - case.cutoff) <= nc.BAND * case.cutoff  # fp32 moves a distance of 4.5 A by about 1e-6 A
    assert (i[near] == j[near]).all()
    assert np.array_equal(case.cell * 4, np.rint(case.cell * 4)) or not near.any()
