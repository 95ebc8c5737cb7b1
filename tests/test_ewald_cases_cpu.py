"""The premises of ``tests/ewald_cases.py``, without a GPU: every case collates and evaluates in the oracle, reaches the count
it is named for, and the oracle itself satisfies the identities the cases were built around. A broken case builder fails here
and cannot pass as a kernel result in ``test_gpu_long_range_edges.py``."""
import math

import pytest
import torch

import _ewald_oracle as eo
import ewald_cases as ec


def _relmax(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("name", ec.ALL_CASES)
def test_case_collates_and_the_oracle_evaluates_it(name):
    c, b = ec.case(name), ec.batch(name)
    channels = 1 if name == "nacl" else 5
    n, n_sys = b["positions"].shape[0], len(c.systems)
    shapes = [(n, channels), (n, channels), (n, 3), (n_sys, 3, 3)]
    for dtype in (torch.float64, torch.float32):
        out = ec.reference(name, channels, dtype)
        for quantity, t, shape in zip(ec.QUANTITIES, out, shapes):
            assert tuple(t.shape) == shape and bool(torch.isfinite(t).all()), (name, quantity, dtype)
    closest = [ec.min_distance(p, cell, pbc) for p, cell, pbc in c.systems]
    print(name, "atoms", n, "edges", len(b["centers"]), "min d", closest)
    drawn = [d for s, d in enumerate(closest) if s not in ec.GIVEN_SYSTEMS.get(name, ())]
    assert all(d >= ec.MIN_DISTANCE for d in drawn)


def test_counts_the_cases_are_named_for():
    from metatrain_amd import long_range as lr

    cell = ec.case("elongated_limit").systems[0][1]
    assert ec.max_reciprocal_index(cell, ec.RESOLUTION) == 63
    assert eo.kvector_indices(cell, ec.RESOLUTION).abs().max(0).values.tolist() == [63, 4, 4]
    assert eo.kvector_indices(cell, ec.RESOLUTION).shape[0] == 5914
    assert ec.max_reciprocal_index(torch.diag(torch.tensor(ec.BEYOND_LIMIT, dtype=torch.float64)), ec.RESOLUTION) == 64
    small = ec.case("periodic_tiles").systems[3][1]
    assert float(small[0, 0]) == 3.0 and lr.kvectors(small, ec.RESOLUTION).shape[0] == 56
    first = ec.batch("periodic_tiles")["first_atom"]
    assert first == [0, 32, 32, 65, 67]  # a repeated entry: the empty system
    assert all(ec.batch("periodic_tiles")["pbcs"][s] == [True] * 3 for s in range(4))
    first = ec.batch("open_tiles")["first_atom"]
    assert tuple(b - a for a, b in zip(first, first[1:])) == (32, 33, 64, 150, 1)
    sheared = ec.case("sheared").systems[0][1]
    assert eo.kvector_indices(sheared, ec.RESOLUTION).shape[0] == 562
    assert [int(math.floor(float(torch.linalg.norm(sheared[a])) / ec.RESOLUTION)) for a in range(3)] == [6, 6, 7]
    assert float(torch.det(ec.case("left_handed").systems[0][1])) < 0.0 < float(torch.det(ec.triclinic43()[1]))
    pos, cell, _ = ec.case("unwrapped").systems[0]
    frac = pos @ torch.linalg.inv(cell)
    assert float(frac.min()) < -2.0 and float(frac.max()) > 3.0
    # atoms of a cell smaller than the cutoff see their own images
    b = ec.batch("periodic_tiles")
    assert int(((b["centers"] == b["neighbors"]) & (b["centers"] >= 65)).sum()) >= 12


def _wrapped_reference(channels=5):
    """The oracle on the 43-atom triclinic system alone with the charges of ``unwrapped`` / ``left_handed``."""
    b = eo.collate([ec.triclinic43()], ec.CUTOFF)
    q, gv = ec.charges("unwrapped", channels)
    return ec._reference(b, q, gv, ec.SMEARING, ec.RESOLUTION, ec.CUTOFF, torch.float64)


@pytest.mark.parametrize("name", ["unwrapped", "left_handed"])
def test_oracle_is_invariant_under_lattice_moves_and_handedness(name):
    """Potential, dL/dq and dL/dR do not see a move by a lattice vector nor a swap of two cell rows."""
    assert all(torch.equal(a, b) for a, b in zip(ec.charges(name, 5), ec.charges("unwrapped", 5)))
    ref, got = _wrapped_reference(), ec.reference(name, 5, torch.float64)
    for quantity, g, r in zip(ec.QUANTITIES[:3], got, ref):
        print(name, quantity, _relmax(g, r))
        assert _relmax(g, r) <= 1e-10, (name, quantity)


def test_unwrapped_cell_gradient_tells_the_two_fractional_coordinates_apart():
    """dL/dcell is at fixed Cartesian positions: an atom moved by a lattice vector does not move with the cell as its image
    does, so the case separates the wrapped s_i of the phase tables from the unwrapped s_i of dL/dcell."""
    ref, got = _wrapped_reference()[3], ec.reference("unwrapped", 5, torch.float64)[3]
    print("dL/dcell unwrapped against wrapped:", _relmax(got, ref))
    assert _relmax(got, ref) > 1.0


def test_supercell_halves_repeat_the_primitive_cell():
    v, gq, gp, _ = ec.reference("supercell", 5, torch.float64)
    for quantity, t in zip(ec.QUANTITIES[:3], (v, gq, gp)):
        for half in (slice(43, 86), slice(86, 129)):
            print(quantity, half, _relmax(t[half], t[:43]))
            assert _relmax(t[half], t[:43]) <= 1e-10, (quantity, half)


def _canon(k, cell):  # rows sorted by their integer indices
    n = torch.round(k @ cell.T / (2.0 * math.pi)).long()
    order = sorted(range(len(n)), key=lambda r: tuple(n[r].tolist()))
    return k[order], n[order]


@pytest.mark.parametrize("name, system", [("elongated_limit", 0), ("sheared", 0), ("left_handed", 0), ("periodic_tiles", 3)])
def test_product_kvectors_equal_the_oracle_set(name, system):
    from metatrain_amd import long_range as lr

    cell = ec.case(name).systems[system][1]
    got, ref = lr.kvectors(cell, ec.RESOLUTION), eo.kvectors(cell, ec.RESOLUTION)
    assert got.shape == ref.shape and got.shape[0] % 2 == 0
    (gk, gn), (rk, rn) = _canon(got, cell), _canon(ref, cell)
    assert torch.equal(gn, rn)
    assert float((gk - rk).abs().max()) < 1e-12


def test_plan_refuses_a_cell_beyond_the_served_index():
    """``pet_ewald_plan`` checks the index before its first device call: the refusal needs no GPU."""
    from metatrain_amd import long_range as lr

    cell = torch.diag(torch.tensor(ec.BEYOND_LIMIT, dtype=torch.float64))
    with pytest.raises(lr.PetHipError, match="reciprocal indices up to 64"):
        lr.EwaldHip(ec.SMEARING, ec.RESOLUTION, ec.CUTOFF).plan(cell[None], [[True] * 3], [0, 37])


def test_madelung_composition_with_the_oracle_as_the_device():
    c = ec.case("nacl")
    assert abs(2.0 * math.pi / c.resolution - 9.0 / c.smearing) < 1e-12
    q, _ = ec.charges("nacl", 1)
    b = ec.batch("nacl")
    v = eo.potential_batch(b["positions"], b["cells"], b["pbcs"], b["first_atom"], q, b["centers"], b["neighbors"],
                           b["cell_shifts"], c.smearing, c.resolution, c.cutoff)
    got = ec.madelung_composition(v)
    print("Madelung composition:", got / eo.PREFACTOR)
    assert abs(got - eo.PREFACTOR * ec.MADELUNG_NACL) < 1e-6
    assert abs(ec.madelung_composition(None, torch.float64) - got) < 1e-12
