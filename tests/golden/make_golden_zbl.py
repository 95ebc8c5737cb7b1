"""Fixtures of the ZBL tests -> ``zbl_*.npz``, from the reference's own ``ZBL.get_pairwise_zbl`` in fp64.

``utils/additive/zbl.py`` is loaded by path with stub modules for what it imports but ``get_pairwise_zbl`` never touches
(``metatensor.torch``, ``metatomic.torch``, the package-relative ``..data`` / ``..sum_over_atoms``) and an ``ase.data``
that carries the covalent radii below (Cordero 2008 as ASE tabulates them, Z = 1 .. 36; written from memory). A ``ZBL``
object is made without its ``__init__`` (which wants a DatasetInfo) and given the two buffers ``__init__`` registers.
torch's default dtype is float64 while it runs, so that ``zi ** 0.23`` of the integer atomic numbers is fp64 too.

Each file: positions, cells, numbers, system_indices, pbc, atomic_types, radii (per type), radii_table (index Z), pairs
``[E,5]`` (i, j, Sa, Sb, Sc; strict full list at 2 max(radius)), and from the reference function pair_energy ``[E]``, atomic
``[N]``, grad_positions ``[N,3]``, grad_cells ``[S,3,3]`` and grad_strain ``[S,3,3]`` by fp64 autograd.

    python tests/golden/make_golden_zbl.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import zbl_ref  # noqa: E402

REF = "/root/reference/src/metatrain"
RADII = [0.2, 0.31, 0.28, 1.28, 0.96, 0.84, 0.76, 0.71, 0.66, 0.57, 0.58, 1.66, 1.41, 1.21, 1.11, 1.07, 1.05, 1.02, 1.06,
         2.03, 1.76, 1.70, 1.60, 1.53, 1.39, 1.39, 1.32, 1.26, 1.24, 1.32, 1.22, 1.22, 1.20, 1.19, 1.20, 1.20, 1.16]


def import_reference_zbl():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    anything = type("Anything", (), {})
    stub("metatensor")
    stub("metatensor.torch", Labels=anything, TensorBlock=anything, TensorMap=anything)
    stub("metatomic")
    stub("metatomic.torch", ModelOutput=anything, NeighborListOptions=anything, System=anything)
    stub("ase")
    stub("ase.data", covalent_radii=np.array(RADII))
    pkg = stub("zbl_reference_pkg")
    pkg.__path__ = []
    stub("zbl_reference_pkg.data", DatasetInfo=anything, TargetInfo=anything)
    stub("zbl_reference_pkg.sum_over_atoms", sum_over_atoms=None)
    sub = stub("zbl_reference_pkg.additive")
    sub.__path__ = []
    spec = importlib.util.spec_from_file_location("zbl_reference_pkg.additive.zbl",
                                                  os.path.join(REF, "utils", "additive", "zbl.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.ZBL


def reference_model(ZBL, atomic_types):
    z = ZBL.__new__(ZBL)
    torch.nn.Module.__init__(z)
    index = torch.full((max(atomic_types) + 1,), -1, dtype=torch.int)
    for i, t in enumerate(atomic_types):
        index[t] = i
    z.register_buffer("species_to_index", index)
    z.register_buffer("covalent_radii", torch.tensor([RADII[t] for t in atomic_types], dtype=torch.float64))
    return z


def min_image_distance(p, others, cell):
    d = others - p
    if cell is not None:
        f = d @ torch.linalg.inv(cell)
        d = (f - torch.round(f)) @ cell
    return torch.linalg.norm(d, dim=1)


def random_box(rng, numbers, length, dmin, clustered=0.0):
    """Positions in a cube by rejection (minimum image distance >= dmin); with probability ``clustered`` a candidate is
    drawn 0.8 .. 1.5 Angstrom from an atom already placed (close pairs for the small-energy box)."""
    cell = torch.eye(3, dtype=torch.float64) * length
    pos = []
    while len(pos) < len(numbers):
        if pos and rng.random() < clustered:
            v = rng.normal(size=3)
            p = pos[rng.integers(len(pos))] + torch.tensor(v / np.linalg.norm(v) * rng.uniform(0.8, 1.5))
            p = p - torch.floor(p / length) * length
        else:
            p = torch.tensor(rng.uniform(0, length, size=3))
        if not pos or float(min_image_distance(p, torch.stack(pos), cell).min()) >= dmin:
            pos.append(p)
    return torch.stack(pos), cell


def make_case(ZBL, name, positions, cells, numbers, system_indices, periodic, min_inside, min_outside, dmin=0.7):
    atomic_types = sorted(set(int(z) for z in numbers))
    model = reference_model(ZBL, atomic_types)
    cutoff = 2.0 * float(model.covalent_radii.max())
    rows, first = [], 0
    for s in range(cells.shape[0]):
        sel = (system_indices == s).nonzero().reshape(-1)
        p = zbl_ref.brute_force_pairs(positions[sel], cells[s], cutoff, periodic=periodic[s])
        p[:, :2] += first
        rows.append(p)
        first += sel.numel()
    pairs = torch.cat(rows)
    i, j, S = pairs[:, 0], pairs[:, 1], pairs[:, 2:5].double()

    def energy(pos, cel, strain=None):
        if strain is not None:
            pos = torch.einsum("na,nab->nb", pos, strain[system_indices])
            cel = torch.matmul(cel, strain)
        D = pos[j] - pos[i] + torch.einsum("ea,eab->eb", S, cel[system_indices[i]])
        r = torch.sqrt((D * D).sum(1))
        e = model.get_pairwise_zbl(numbers[i], numbers[j], r)
        return e, r

    pos = positions.clone().requires_grad_(True)
    cel = cells.clone().requires_grad_(True)
    e, r = energy(pos, cel)
    g_pos, g_cell = torch.autograd.grad(e.sum(), [pos, cel])
    strain = torch.eye(3, dtype=torch.float64).repeat(cells.shape[0], 1, 1).requires_grad_(True)
    e2, _ = energy(positions, cells, strain)
    (g_strain,) = torch.autograd.grad(e2.sum(), [strain])
    atomic = torch.zeros(positions.shape[0], dtype=torch.float64).index_add(0, i, e.detach())
    rc = model.covalent_radii[model.species_to_index[numbers[i]]] + model.covalent_radii[model.species_to_index[numbers[j]]]
    inside = int((r <= rc).sum())
    outside = int((r > rc).sum())
    print(f"{name}: {positions.shape[0]} atoms, {pairs.shape[0]} listed pairs within {cutoff:.2f}, {inside} inside rc, "
          f"{outside} outside, {int((atomic != 0).sum())} atoms touched, max atomic {float(atomic.max()):.3f} eV, "
          f"max |dE/dR| {float(g_pos.abs().max()):.2f} eV/A, min r {float(r.min()):.3f}")
    assert inside >= min_inside, (name, inside)
    assert outside >= min_outside, (name, outside)
    assert float(r.min()) >= dmin, (name, float(r.min()))
    # the restatement the tests use agrees with the reference on every pair
    mine = zbl_ref.pair_energy(numbers[i], numbers[j], torch.tensor(RADII)[numbers[i]], torch.tensor(RADII)[numbers[j]], r.detach())
    assert float((mine - e.detach()).abs().max()) <= 1e-12 * max(1.0, float(e.abs().max())), name
    np.savez_compressed(
        os.path.join(HERE, f"zbl_{name}.npz"), positions=positions.numpy(), cells=cells.numpy(),
        numbers=numbers.numpy().astype(np.int32), system_indices=system_indices.numpy().astype(np.int32),
        pbc=np.array([[bool(p)] * 3 for p in periodic]), atomic_types=np.array(atomic_types, dtype=np.int32),
        radii=model.covalent_radii.numpy(), radii_table=np.array(RADII), pairs=pairs.numpy().astype(np.int32),
        pair_energy=e.detach().numpy(), atomic=atomic.numpy(), grad_positions=g_pos.numpy(), grad_cells=g_cell.numpy(),
        grad_strain=g_strain.numpy())


def main():
    torch.set_default_dtype(torch.float64)
    ZBL = import_reference_zbl()
    rng = np.random.default_rng(20240607)
    # Box A: 48 atoms of H / C / O / Cu at 0.10 per cubic Angstrom, and the same atoms in a sheared cell
    numbers = torch.tensor(rng.choice([1, 6, 8, 29], size=48))
    length = (48 / 0.10) ** (1 / 3)
    pos, cell = random_box(rng, numbers, length, 0.7)
    zeros = torch.zeros(48, dtype=torch.long)
    make_case(ZBL, "box_a", pos, cell[None], numbers, zeros, [True], 60, 30)
    sheared = cell.clone()
    sheared[1, 0], sheared[2, 1] = 1.3, -0.9
    frac = pos @ torch.linalg.inv(cell)
    make_case(ZBL, "box_a_sheared", frac @ sheared, sheared[None], numbers, zeros, [True], 60, 30)
    # Box B: 24 atoms of H / C / O at 0.08: energies of order 1 eV, where the cancellation at rc shows
    numbers = torch.tensor(rng.choice([1, 6, 8], size=24, p=[0.4, 0.4, 0.2]))
    pos, cell = random_box(rng, numbers, (24 / 0.08) ** (1 / 3), 0.8, clustered=0.8)
    make_case(ZBL, "box_b", pos, cell[None], numbers, torch.zeros(24, dtype=torch.long), [True], 10, 30, dmin=0.8)
    # one Cu atom in a 2.2 Angstrom cube: six self-image edges
    make_case(ZBL, "one_atom", torch.tensor([[0.3, 0.4, 0.5]]), 2.2 * torch.eye(3)[None], torch.tensor([29]),
              torch.zeros(1, dtype=torch.long), [True], 6, 0)
    # the five QM9 frames compressed to 0.8 of their size (unscaled, almost no pair is inside rc), one batch, no cells
    q = np.load(os.path.join(HERE, "qm9_first5.npz"))
    pos = torch.cat([torch.tensor(q[f"pos{k}"]) * 0.8 for k in range(5)])
    numbers = torch.cat([torch.tensor(q[f"z{k}"]).long() for k in range(5)])
    sysidx = torch.cat([torch.full((q[f"z{k}"].shape[0],), k) for k in range(5)])
    make_case(ZBL, "qm9_compressed", pos, torch.zeros((5, 3, 3)), numbers, sysidx, [False] * 5, 10, 0)


if __name__ == "__main__":
    main()
