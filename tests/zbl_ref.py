"""The ZBL pair model in torch fp64, written from its formulas (LAMMPS ``pair_style zbl`` with inner cutoff 0, cut at the
sum of the covalent radii): what the ZBL tests compare the library with, and -- through autograd -- its gradients.

    rc = rad(Zi) + rad(Zj),  a = 0.46850 / (Zi^0.23 + Zj^0.23),  phi(x) = sum_k c_k exp(-d_k x / a)
    E(x) = K Zi Zj / x phi(x),  e(r) = 1/2 [E(r) + A/3 r^3 + B/4 r^4 + C] for r <= rc, else 0
    A = (-3 E'(rc) + rc E''(rc)) / rc^2,  B = (2 E'(rc) - rc E''(rc)) / rc^3,  C = -E(rc) + rc E'(rc) / 2 - rc^2 E''(rc) / 12
"""
import torch

K = 14.399645478425668  # eV Angstrom
C = (0.02817, 0.28022, 0.50986, 0.18175)
D = (0.20162, 0.40290, 0.94229, 3.19980)


def _derivs(kzz, inva, r):
    c = torch.tensor(C, dtype=torch.float64)
    da = torch.tensor(D, dtype=torch.float64)[:, None] * inva[None]
    t = c[:, None] * torch.exp(-da * r[None])
    phi, dphi, d2phi = t.sum(0), (-da * t).sum(0), (da * da * t).sum(0)
    return kzz / r * phi, kzz / r * (dphi - phi / r), kzz / r * (d2phi - 2 * dphi / r + 2 * phi / r ** 2)


def pair_constants(zi, zj, rad_i, rad_j):
    """``[..., 6]`` = (rc, 1/a, K Zi Zj, A, B, C) for atomic numbers ``zi, zj`` and their radii (fp64 tensors)."""
    zi, zj = zi.double(), zj.double()
    rc = (rad_i + rad_j).double()
    inva = (zi ** 0.23 + zj ** 0.23) / 0.46850
    kzz = K * zi * zj
    E, dE, d2E = _derivs(kzz.reshape(-1), inva.reshape(-1), rc.reshape(-1))
    E, dE, d2E = E.reshape(rc.shape), dE.reshape(rc.shape), d2E.reshape(rc.shape)
    A = (-3 * dE + rc * d2E) / rc ** 2
    B = (2 * dE - rc * d2E) / rc ** 3
    Cc = -E + rc * dE / 2 - rc ** 2 * d2E / 12
    return torch.stack([rc, inva, kzz, A, B, Cc], dim=-1)


def pair_energy(zi, zj, rad_i, rad_j, r):
    """Per directed pair ``e(r)`` (half the pair energy; 0 beyond rc)."""
    rc, inva, kzz, A, B, Cc = pair_constants(zi, zj, rad_i, rad_j).unbind(-1)
    E = kzz / r * sum(c * torch.exp(-d * inva * r) for c, d in zip(C, D))
    e = 0.5 * (E + A / 3 * r ** 3 + B / 4 * r ** 4 + Cc)
    return torch.where(r > rc, torch.zeros_like(e), e)


def atomic_energies(positions, cells, system_indices, numbers, radii_of, pairs, strain=None):
    """Per-atom energies ``[N]`` fp64 of a batch: ``pairs [E,5]`` rows (i, j, Sa, Sb, Sc) with global atom indices,
    ``radii_of``: tensor indexed by atomic number. ``strain [S,3,3]``: positions and cells are multiplied by it
    (differentiate at the identity for dE/d(eps))."""
    pairs = pairs.long()
    i, j, S = pairs[:, 0], pairs[:, 1], pairs[:, 2:5].double()
    if strain is not None:
        positions = torch.einsum("na,nab->nb", positions, strain[system_indices])
        cells = torch.matmul(cells, strain)
    Dv = positions[j] - positions[i] + torch.einsum("ea,eab->eb", S, cells[system_indices[i]])
    r = torch.sqrt((Dv * Dv).sum(1))
    e = pair_energy(numbers[i], numbers[j], radii_of[numbers[i]], radii_of[numbers[j]], r)
    return torch.zeros(positions.shape[0], dtype=torch.float64).index_add(0, i, e)


def brute_force_pairs(positions, cell, cutoff, periodic=True):
    """All directed pairs (i, j, S) with |R_j - R_i + S cell| < cutoff of ONE system, grouped by i (fp64, O(N^2 images))."""
    n = positions.shape[0]
    shifts = [(0, 0, 0)]
    if periodic:
        inv = torch.linalg.inv(cell)
        heights = 1.0 / torch.linalg.norm(inv, dim=0)  # distances between lattice planes
        reach = [int(torch.ceil(cutoff / h)) for h in heights]
        shifts = [(a, b, c) for a in range(-reach[0], reach[0] + 1) for b in range(-reach[1], reach[1] + 1)
                  for c in range(-reach[2], reach[2] + 1)]
    rows = []
    for s in shifts:
        off = torch.tensor(s, dtype=torch.float64) @ cell
        d = torch.linalg.norm(positions[None, :, :] - positions[:, None, :] + off, dim=2)  # [i, j]
        ok = d < cutoff
        if s == (0, 0, 0):
            ok &= ~torch.eye(n, dtype=torch.bool)
        ij = ok.nonzero()
        rows.append(torch.cat([ij, torch.tensor(s).expand(ij.shape[0], 3)], dim=1))
    pairs = torch.cat(rows)
    return pairs[torch.argsort(pairs[:, 0], stable=True)]
