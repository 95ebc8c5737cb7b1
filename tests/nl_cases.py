"""Inputs that drive the device neighbour list (``metatrain_amd/csrc/nl.hip``) into the branches of ``k_nlb_pairs`` and of the
host set-up that a random box at 0.05 atoms / A^3 never takes, shared by ``test_nl_cases_cpu.py`` and ``test_gpu_nl_edges.py``.
No GPU import here.

Every case is ``Case(name, positions fp32 [n,3], cell fp32 [3,3], pbc, cutoff)``. The lattice cases (``DYADIC``) use coordinates
that are multiples of 0.25 and lie off every bin boundary: positions, wrapped positions, image offsets and d^2 are exact in
fp32, so pair sets AND vectors compare with ``==``.

The second half restates, in plain fp64 numpy, what the host code of ``nl.hip`` derives from a system -- the completed lattice
and its heights (``lattice_params``, nl.hip:308-371), the bins and the search reach (``bin_params``, nl.hip:374-406), the bin of
an atom (``k_nlb_bin``, nl.hip:89-99) and the walk over the surrounding (bin, image) slots (``k_nlb_pairs``, nl.hip:201-243) --
so that the CPU test can assert that every case still reaches the branch it is named for. The two constants the branches
depend on are read from the source itself (``kernel_constants``): retuning ``NL_TILE`` or ``NL_MAX_IMAGES`` fails that
assertion instead of silently removing the coverage.
"""
import collections
import itertools
import math
import os
import re

import numpy as np

Case = collections.namedtuple("Case", "name positions cell pbc cutoff")

CUTOFF = 4.5
NL_SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metatrain_amd", "csrc", "nl.hip")

PERIODIC, OPEN = (True, True, True), (False, False, False)


def _case(name, positions, cell, pbc, cutoff=CUTOFF):
    return Case(name, np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3),
                np.ascontiguousarray(cell, dtype=np.float32).reshape(3, 3), tuple(bool(p) for p in pbc), float(cutoff))


def _grid(n):
    return np.array(list(itertools.product(range(n), repeat=3)), dtype=np.float64)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def sc1():
    """One atom in a 1.25 A cube: nb (1,1,1), reach (4,4,4), 729 occupied image slots -> several image-count flushes.
    178 pairs (0, 0, S) with 0 < 1.5625 |S|^2 < 20.25."""
    return _case("sc1", [[0.25, 0.5, 0.75]], 1.25 * np.eye(3), PERIODIC)


THIN2_CELL = [[1.5, 0.0, 0.0], [0.25, 1.75, 0.0], [0.5, -0.25, 12.0]]
THIN2_POS = [[0.1, 0.2, 0.3], [0.9, 1.0, 5.0], [0.3, 0.4, 7.1], [1.1, 0.2, 11.5], [0.6, 1.2, 2.2], [0.2, 0.9, 9.4]]


def thin2(unwrapped=False):
    """Six atoms in a triclinic cell thin along two axes: nb (1,1,2), reach (4,3,1), 189 slots; 424 pairs, at most 83 per
    atom, self-images included. ``unwrapped``: every position moved by -4.0 (outside the cell on all axes)."""
    pos = np.asarray(THIN2_POS, dtype=np.float32)
    if unwrapped:
        pos = pos - np.float32(4.0)
    return _case("thin2_unwrapped" if unwrapped else "thin2", pos, THIN2_CELL, PERIODIC)


def lat216(moved=False):
    """6 x 6 x 6 simple cubic, a = 1.5, cell 9.0: nb (2,2,2), 27 atoms per bin, 27 * 27 = 729 candidates per wave -> the tile
    overflows between the surrounding bins. 92 neighbours per atom (|k|^2 <= 8; the shells at exactly 4.5 A are outside the
    strict <). ``moved``: every third atom displaced by an integer combination (+-1, +-2) of cell rows, exact in fp32: only
    the expected shifts change."""
    pos = 0.25 + 1.5 * _grid(6)
    cell = 9.0 * np.eye(3)
    if moved:
        moves = np.array([[1, 0, -2], [-1, 2, 0], [0, -2, 1], [2, 1, -1], [-2, -1, 2]], dtype=np.float64)
        for k, a in enumerate(range(0, len(pos), 3)):
            pos[a] += moves[k % len(moves)] @ cell
    return _case("lat216_moved" if moved else "lat216", pos, cell, PERIODIC)


def lat125():
    """5 x 5 x 5 simple cubic, a = 1.5, cell 7.5: ONE bin with 125 centres (64 + 61) and 27 * 125 = 3375 candidates; 11 500
    pairs, 92 per atom. The first pair buffer of ``runtime.neighbor_list_batch`` holds 4 400 rows for 125 atoms: second call."""
    return _case("lat125", 0.25 + 1.5 * _grid(5), 7.5 * np.eye(3), PERIODIC)


def lat110():
    """lat125 without its last 15 atoms: a bin of 64 + 46 atoms, so the tile (4 * 110 + 64 = 504, + 46 > 512) overflows
    between the two 64-atom loads of ONE bin and the rest of that bin goes to the re-registered image slot 0."""
    return _case("lat110", (0.25 + 1.5 * _grid(5))[:110], 7.5 * np.eye(3), PERIODIC)


def open70():
    """70 random atoms in a 6 A cube, no periodicity, zero cell: one open bin with more than 64 centres."""
    rng = np.random.default_rng(70)
    return _case("open70", rng.random((70, 3)) * 6.0, np.zeros((3, 3)), OPEN)


def sparse(length, periodic=True):
    """Five atoms in a cube of 200 A or 5000 A: far more bins than atoms, so ``bin_params`` halves the bin counts (and caps
    them at 1024 first for 5000 A). Pairs across faces, across a bin boundary and from an atom given outside the cell."""
    big = float(length)
    pos = [[0.5, 0.5, 0.5], [big - 0.25, 0.5, 0.5], [66.5, 66.5, 66.5], [67.0, 66.5, 68.0],
           [-0.25, big - 0.5, big + 0.25]]
    name = "sparse%d" % int(length) + ("" if periodic else "_open")
    return _case(name, pos, big * np.eye(3) if periodic else np.zeros((3, 3)), PERIODIC if periodic else OPEN)


def oncut():
    """5 x 5 x 5 simple cubic with a = fp32(0.9), deliberately NOT dyadic; cell 5 a = 4.5 exactly in fp32 = the cutoff. The
    shells (5,0,0) a and (4,3,0) a -- 30 per atom, 3 750 pairs -- sit on the cutoff and fp32 rounding decides each one."""
    k = _grid(5).astype(np.float32)
    pos = np.float32(0.3) + np.float32(0.9) * k
    cell = (np.float32(0.9) * np.float32(5.0)) * np.eye(3, dtype=np.float32)
    return _case("oncut", pos, cell, PERIODIC)


SLAB_CELL = [[9.0, 1.0, -0.5], [0.75, 8.0, 0.5], [-0.5, 0.25, 10.0]]


def slab60():
    """60 atoms in a triclinic slab, periodic along a and b, fractional coordinates from -0.1 to 1.1."""
    rng = np.random.default_rng(60)
    return _case("slab60", (rng.random((60, 3)) * 1.2 - 0.1) @ np.asarray(SLAB_CELL), SLAB_CELL, (True, True, False))


def wire40():
    """40 atoms along a wire, periodic along b only, fractional coordinates from -0.1 to 1.1."""
    rng = np.random.default_rng(40)
    cell = np.asarray([[6.0, 0.5, 0.0], [0.5, 7.0, 0.25], [0.0, -0.5, 6.0]])
    return _case("wire40", (rng.random((40, 3)) * 1.2 - 0.1) @ cell, cell, (False, True, False))


def empty():
    return _case("empty", np.zeros((0, 3)), 5.0 * np.eye(3), PERIODIC)


def batch7():
    """The systems of one ``neighbor_list_batch`` call: periodic thin, empty, open, slab, single atom, sparse, wire."""
    return [thin2(), empty(), open70(), slab60(), sc1(), sparse(200), wire40()]


SINGLE = collections.OrderedDict((c.name, c) for c in (
    sc1(), thin2(), thin2(unwrapped=True), lat216(), lat216(moved=True), lat125(), lat110(), open70(), sparse(200),
    sparse(5000), sparse(200, periodic=False), slab60(), wire40()))
# exact in fp32: pair sets and vectors compare with ==
DYADIC = ("sc1", "lat216", "lat216_moved", "lat125", "lat110", "sparse200", "sparse5000", "sparse200_open")
# pairs per atom where the issue states them (every atom the same number), and the totals
PAIRS_PER_ATOM = {"sc1": 178, "lat216": 92, "lat216_moved": 92, "lat125": 92}
PAIRS_TOTAL = {"sc1": 178, "thin2": 424, "thin2_unwrapped": 424, "lat216": 19872, "lat216_moved": 19872, "lat125": 11500}

# oncut: the band around the cutoff inside which fp32 rounding may decide, as a fraction of the cutoff
BAND = 2e-5


def lattice_shell_count(spacing, cutoff):
    """Number of non-zero integer vectors k with |spacing k| < cutoff, counted one by one."""
    m = int(math.ceil(cutoff / spacing))
    return sum(1 for k in itertools.product(range(-m, m + 1), repeat=3)
               if 0 < spacing * spacing * (k[0] * k[0] + k[1] * k[1] + k[2] * k[2]) < cutoff * cutoff)


# ---- what nl.hip derives from a system, restated -------------------------------------------------------------------------------
def kernel_constants():
    """``NL_TILE`` and ``NL_MAX_IMAGES`` as the kernel source states them (nl.hip:71-72)."""
    with open(NL_SOURCE) as fh:
        text = fh.read()
    out = {}
    for name in ("NL_TILE", "NL_MAX_IMAGES"):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, "nl.hip no longer defines %s as a constexpr int" % name
        out[name] = int(m.group(1))
    return out


def effective_cell(cell, pbc):
    """lattice_params, nl.hip:309-346: periodic rows as given, the others completed with unit vectors orthogonal to the rest."""
    c = np.where(np.asarray(pbc)[:, None], np.asarray(cell, dtype=np.float64), 0.0)
    basis = []

    def residual(v):
        r = np.array(v, dtype=np.float64)
        for b in basis:
            r = r - (r @ b) * b
        return r

    def add(v):
        r = residual(v)
        if np.linalg.norm(r) > 1e-9:
            basis.append(r / np.linalg.norm(r))

    for a in range(3):
        if pbc[a]:
            add(c[a])
    for a in range(3):
        if pbc[a]:
            continue
        best, bestn = None, 0.0
        for e in np.eye(3):
            r = residual(e)
            if np.linalg.norm(r) > bestn + 1e-9:
                bestn, best = np.linalg.norm(r), r / np.linalg.norm(r)
        c[a] = best
        add(c[a])
    return c


def heights(c):
    """lattice_params, nl.hip:347-349 and 363-366: height along a = |det| / |c[a+1] x c[a+2]|, the determinant as the triple
    product (exact for the cubic cells here: a height equal to the cutoff must give reach 1, not 2)."""
    det = abs(float(c[0] @ np.cross(c[1], c[2])))
    return np.array([det / np.linalg.norm(np.cross(c[(a + 1) % 3], c[(a + 2) % 3])) for a in range(3)])


def bin_params(height, pbc, frac, cutoff, n_atoms):
    """bin_params, nl.hip:374-406: ``(nb, reach, origin, extent)``. ``frac``: the atoms' fractional coordinates (the bounding
    box of the open axes comes from them, nl.hip:380-384)."""
    nb, origin, extent = [0, 0, 0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    for a in range(3):
        span = height[a]
        if not pbc[a]:
            lo, hi = float(frac[:, a].min()), float(frac[:, a].max())
            extent[a] = max(hi - lo, 1e-3) * 1.0001 + 1e-4
            origin[a] = lo - 0.5e-4
            span = extent[a] * height[a]
        nb[a] = min(max(int(math.floor(span / cutoff)), 1), 1024)
    total = nb[0] * nb[1] * nb[2]
    while total > n_atoms + 32:
        a = max(range(3), key=lambda k: (nb[k], -k))  # the largest, the first of equals
        if nb[a] <= 1:
            break
        total //= nb[a]
        nb[a] = (nb[a] + 1) // 2
        total *= nb[a]
    reach = [0, 0, 0]
    for a in range(3):
        span = height[a] if pbc[a] else extent[a] * height[a]
        reach[a] = int(math.ceil(cutoff / (span / nb[a])))
        if not pbc[a] and reach[a] > nb[a]:
            reach[a] = nb[a]
    return nb, reach, origin, extent


Plan = collections.namedtuple("Plan", "nb reach uncapped_bins total_bins max_centres max_slots max_candidates first_capacity")


def plan(case):
    """What one wave of ``k_nlb_pairs`` meets at its worst in this case: the most centres in a bin, and around one bin the most
    occupied (bin, image) slots (nl.hip:216-218) and the most candidates staged (nl.hip:225-243)."""
    n = len(case.positions)
    pbc = case.pbc
    c = effective_cell(case.cell, pbc)
    h = heights(c)
    frac = case.positions.astype(np.float64) @ np.linalg.inv(c)
    nb, reach, origin, extent = bin_params(h, pbc, frac, case.cutoff, n)
    uncapped = 1
    for a in range(3):
        span = h[a] if pbc[a] else extent[a] * h[a]
        uncapped *= max(int(math.floor(span / case.cutoff)), 1)
    b = np.zeros((n, 3), dtype=np.int64)
    for a in range(3):  # k_nlb_bin, nl.hip:89-98
        if pbc[a]:
            f = frac[:, a] - np.floor(frac[:, a])
            b[:, a] = np.minimum((f * nb[a]).astype(np.int64), nb[a] - 1)
        else:
            b[:, a] = np.clip(((frac[:, a] - origin[a]) / extent[a] * nb[a]).astype(np.int64), 0, nb[a] - 1)
    occupancy = collections.Counter(map(tuple, b.tolist()))
    max_slots = max_candidates = 0
    for centre in occupancy:  # k_nlb_pairs, nl.hip:201-216
        slots = candidates = 0
        for d in itertools.product(*[range(-r, r + 1) for r in reach]):
            t = [centre[a] + d[a] for a in range(3)]
            if any(not pbc[a] and not 0 <= t[a] < nb[a] for a in range(3)):
                continue
            m = occupancy.get(tuple(t[a] % nb[a] for a in range(3)), 0)
            slots += m > 0
            candidates += m
        max_slots, max_candidates = max(max_slots, slots), max(max_candidates, candidates)
    # runtime.neighbor_list_batch: rows of the first, optimistic pair buffer for a batch of n atoms never seen before
    return Plan(tuple(nb), tuple(reach), uncapped, nb[0] * nb[1] * nb[2], max(occupancy.values()), max_slots, max_candidates,
                max(1024, int(1.1 * 32 * n)))


def fp32_d2(case, i, j, s):
    """d^2 of the pairs ``(i, j, S)`` in fp32 arithmetic, operation by operation as ``k_nlb_pairs`` evaluates it on unwrapped
    positions: (r_j - r_i) + (Sa c_a + Sb c_b + Sc c_c), then dx dx + dy dy + dz dz (nl.hip:173-175, 219-222)."""
    pos, cell = case.positions, case.cell
    sf = np.asarray(s).astype(np.float32)
    off = (sf[:, 0:1] * cell[0][None, :] + sf[:, 1:2] * cell[1][None, :]) + sf[:, 2:3] * cell[2][None, :]
    d = (pos[j] - pos[i]) + off
    assert d.dtype == np.float32
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
