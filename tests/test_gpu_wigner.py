"""GPU tests of the spherical-target path of the device augmenter (``csrc/wigner.hip``: ``pet_o3_wigner``,
``pet_o3_apply_spherical``; ``metatrain_amd/augmentation.py``) against the fp64 numpy oracle ``_wigner_oracle.py``, which
shares no code or method with the kernels, and against the existing Cartesian kernels.

Bounds (``u = 2^-24``, the fp32 unit roundoff; ``d = max |O^T O - I|`` of an fp32 matrix, measured here in fp64):

* a table entry of block ``l`` against the oracle's ``D^l`` of the matrix's polar factor: ``e_l = u + 3 l d (1 + 3d)^(l-1)`` --
  one rounding of a number of size at most 1, plus the Lipschitz bound of a degree-``l`` polynomial representation between the
  matrix and its polar factor (about 3e-6 at ``l = 8``; a wrong convention or index is an error of order 1);
* an output of the apply kernel against fp64 with the device's own table: ``(2l+2) u sum_m' |D[m,m']| |x[m']|``, the standard
  forward bound of a length-``(2l+1)`` fp32 dot product;
* the Cartesian kernels: a three-term fp32 dot product ``3u sum |R| |x|``, two nested ones ``7u``; a matrix and its polar
  factor differ by at most ``2d`` per entry.

Cross-checks compare two device paths, each against the same exact fp64 image, and allow the sum of the two paths' bounds.
"""
import math

import numpy as np
import pytest
import torch

import _wigner_oracle as wo
from oracle import pet as opet

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = 2.0 ** -24
SIZES = (1, 2, 63, 65, 300)  # 431 atoms: system boundaries inside a wave, a one-atom system, more than one workgroup
N, S = sum(SIZES), len(SIZES)
SYSIDX = np.repeat(np.arange(S), SIZES)


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from metatrain_amd import runtime

    return runtime


def _orthogonal(seed: int, proper: bool) -> np.ndarray:
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if (np.linalg.det(q) > 0) == proper else -q


# eight fixed matrices, alternating proper and improper, rounded to fp32 (what the device sees), then I and -I
MATRICES32 = np.stack([_orthogonal(40 + i, i % 2 == 0) for i in range(8)] + [np.eye(3), -np.eye(3)]).astype(np.float32)
MATRICES = MATRICES32.astype(np.float64)
DEFECT = np.abs(np.einsum("sji,sjk->sik", MATRICES, MATRICES) - np.eye(3)).max(axis=(1, 2))  # d per matrix


def _table_bound(l: int, d: float) -> float:
    return U + 3 * l * d * (1 + 3 * d) ** (l - 1) if l else U


def _kernel_bound(d_exact: np.ndarray, x_exact: np.ndarray, l: int, e: float) -> np.ndarray:
    """``|kernel output - f D_exact x_exact|`` for an input that is ``x_exact`` rounded to fp32 and a table within ``e`` of
    ``D_exact [rows, 2l+1, 2l+1]``: the dot product's forward bound with the table's moduli, the table's error, the input's
    rounding."""
    a = np.abs(d_exact)
    return np.einsum("rmk,rkp->rmp", (a + e) * (2 * l + 2) * U + e + a * U, np.abs(x_exact) * (1 + U))


@pytest.fixture(scope="module")
def oracle_tables():
    """The oracle's tables (of the polar factors) and determinants of the ten matrices: computed once, never changed."""
    both = [wo.table(m, 8) for m in MATRICES]
    tables, dets = np.stack([t for t, _ in both]), np.array([d for _, d in both])
    tables.setflags(write=False)
    return tables, dets


@pytest.fixture(scope="module")
def device_tables(rt):
    table, parity = rt.o3_wigner(torch.from_numpy(MATRICES32).to(DEV), 8)
    return table, parity


def _blocks(table: torch.Tensor, l: int) -> np.ndarray:
    w = 2 * l + 1
    return table.double().cpu().numpy()[:, wo.offset(l):wo.offset(l + 1)].reshape(-1, w, w)


# ---- the table ------------------------------------------------------------------------------------------------------------------
def test_table_matches_the_oracle(rt, oracle_tables, device_tables):
    want, dets = oracle_tables
    table, parity = device_tables
    assert table.shape == (10, 969) and table.dtype == torch.float32 and parity.shape == (10,)
    assert np.array_equal(parity.cpu().numpy(), dets.astype(np.float32))
    assert dets.tolist() == [1.0, -1.0] * 4 + [1.0, -1.0]
    got = table.double().cpu().numpy()
    for l in range(9):
        sl = slice(wo.offset(l), wo.offset(l + 1))
        err = np.abs(got[:, sl] - want[:, sl]).max(axis=1)
        bound = np.array([_table_bound(l, d) for d in DEFECT])
        print(f"l = {l}: max |table - oracle| = {err.max():.3e}, smallest bound {bound.min():.3e}, largest {bound.max():.3e}")
        assert (err <= bound).all(), (l, err, bound)
        for s in (8, 9):  # I and -I: the identity, exactly
            assert np.array_equal(got[s, sl].reshape(2 * l + 1, 2 * l + 1), np.eye(2 * l + 1)), (l, s)
    for l_max in (0, 3):
        short, p = rt.o3_wigner(torch.from_numpy(MATRICES32).to(DEV), l_max)
        assert short.shape == (10, wo.width(l_max)) and torch.equal(short, table[:, :wo.width(l_max)]) and torch.equal(p, parity)
    view = rt.o3_wigner_block(table, 3)
    assert view.shape == (10, 7, 7) and view.data_ptr() == table[:, 35:].data_ptr()
    empty, p = rt.o3_wigner(torch.zeros((0, 3, 3), device=DEV), 2)
    assert empty.shape == (0, 35) and p.shape == (0,)


def test_a_nan_in_a_matrix_takes_that_systems_table_and_no_other(rt, device_tables):
    table, parity = device_tables
    for bad in (float("nan"), float("inf")):
        mats = torch.from_numpy(MATRICES32).to(DEV).clone()
        mats[3, 1, 2] = bad
        t, p = rt.o3_wigner(mats, 8)
        assert bool(torch.isnan(t[3]).all())  # the l = 0 entry, which depends on no entry, included
        keep = [i for i in range(10) if i != 3]
        assert torch.equal(t[keep], table[keep]) and torch.equal(p[keep], parity[keep])
    assert math.isnan(float(rt.o3_wigner(torch.full((1, 3, 3), float("nan"), device=DEV), 1)[1][0]))


# ---- the apply kernel against fp64 with the device's own table ---------------------------------------------------------------------
def _arrays():
    """Per-system arrays for every l, per-atom ones for l in (1, 2, 3, 8); P in (1, 5); both sigmas: 52 arrays."""
    g = torch.Generator().manual_seed(8)
    out = []
    for per_atom, ls in ((False, range(9)), (True, (1, 2, 3, 8))):
        for l in ls:
            for p in (1, 5):
                for sigma in (1, -1):
                    rows = N if per_atom else S
                    shape = (rows, (2 * l + 1) * p) if (l + p) % 2 else (rows, 2 * l + 1, p)  # flattened or not
                    out.append((torch.randn(shape, generator=g) * 3, l, sigma, per_atom))
    return out


def _reference(x, l, sigma, sys_of_row, blocks, dets):
    """fp64 ``f D x`` and the forward bound of the fp32 dot product, for ``x [rows, 2l+1, P]``."""
    x64 = x.double().cpu().numpy().reshape(x.shape[0], 2 * l + 1, -1)
    d = blocks[sys_of_row]
    f = np.where(dets[sys_of_row] < 0, sigma * (-1.0) ** l, 1.0)[:, None, None]
    ref = f * np.einsum("rmk,rkp->rmp", d, x64)
    bound = (2 * l + 2) * U * np.einsum("rmk,rkp->rmp", np.abs(d), np.abs(x64))
    return ref, bound


def test_apply_matches_fp64_with_the_devices_table(rt, device_tables):
    table, parity = device_tables
    table, parity, dets = table[:S].contiguous(), parity[:S].contiguous(), parity[:S].double().cpu().numpy()
    arrays = _arrays()
    assert len(arrays) == 52  # seven launches: the chunking at eight arrays is crossed several times
    sysidx = torch.from_numpy(SYSIDX.astype(np.int32)).to(DEV)
    dev = [(x.to(DEV), l, sigma, sysidx if per_atom else None) for x, l, sigma, per_atom in arrays]
    before = [a[0].clone() for a in dev]
    outs = rt.o3_apply_spherical(table, parity, 8, dev)
    worst = 0.0
    for (x, l, sigma, per_atom), out, src, keep in zip(arrays, outs, dev, before):
        assert out.shape == x.shape and out.data_ptr() != src[0].data_ptr() and torch.equal(src[0], keep)
        ref, bound = _reference(x, l, sigma, SYSIDX if per_atom else np.arange(S), _blocks(table, l), dets)
        err = np.abs(out.double().cpu().numpy().reshape(ref.shape) - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (l, sigma, per_atom, tuple(x.shape), float(err.max()))
    print(f"largest |out - f D x| / bound over 52 arrays: {worst:.3f}")
    # nine arrays in ONE call give what nine calls give
    nine = dev[36:45]
    together = rt.o3_apply_spherical(table, parity, 8, nine)
    for a, want in zip(nine, together):
        assert torch.equal(rt.o3_apply_spherical(table, parity, 8, [a])[0], want)
    # a table that reaches further than the arrays need serves them with the same bits; one that does not is refused
    l3 = [a for a in dev if a[1] <= 3]
    short = rt.o3_apply_spherical(table[:, :wo.width(3)].contiguous(), parity, 3, l3)
    for a, b in zip(short, [o for o, a in zip(outs, dev) if a[1] <= 3]):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="o3_lambda must be in"):
        rt.o3_apply_spherical(table[:, :wo.width(3)].contiguous(), parity, 3, [dev[-1]])


# ---- cross-checks through the Cartesian kernels -------------------------------------------------------------------------------------
def _polar(oracle_dets):
    return np.stack([d * wo.nearest_rotation(d * m) for m, d in zip(MATRICES[:S], oracle_dets[:S])])  # of O itself, det kept


def test_l1_is_the_vector_kernel_on_permuted_components(rt, oracle_tables, device_tables):
    """``l = 1, sigma = +1`` is a true vector in the order (y, z, x). Both paths read the SAME fp32 matrix entries (the l = 1
    block is the proper part's entries, exactly), so the exact image is ``O v`` and the tolerance the two dot-product bounds."""
    table, parity = device_tables
    g = torch.Generator().manual_seed(9)
    v = (torch.randn((N, 3, 5), generator=g) * 3).to(DEV)
    sysidx = torch.from_numpy(SYSIDX.astype(np.int32)).to(DEV)
    mats = torch.from_numpy(MATRICES32[:S]).to(DEV)
    perm = [1, 2, 0]
    (cart,) = rt.o3_apply(mats, [(v, "vector", sysidx)])
    (sph,) = rt.o3_apply_spherical(table[:S].contiguous(), parity[:S].contiguous(), 8, [(v[:, perm].contiguous(), 1, 1, sysidx)])
    scale = np.einsum("rab,rbp->rap", np.abs(MATRICES[SYSIDX]), np.abs(v.double().cpu().numpy()))
    err = np.abs(sph.double().cpu().numpy() - cart[:, perm].double().cpu().numpy())
    bound = (4 + 3) * U * scale[:, perm]
    print(f"l = 1 against VECTOR: largest error / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


def test_l2_is_the_traceless_symmetric_part_of_the_tensor_kernel(rt, oracle_tables, device_tables):
    want, dets = oracle_tables
    table, parity = device_tables
    rng = np.random.default_rng(10)
    t = rng.standard_normal((N, 3, 3, 2)) * 3
    t = t + t.transpose(0, 2, 1, 3)
    t -= np.eye(3)[None, :, :, None] * np.einsum("raap->rp", t)[:, None, None, :] / 3
    t32 = torch.from_numpy(t.astype(np.float32))  # symmetric exactly, traceless to rounding: the map ignores a trace
    t64 = t32.double().numpy()

    def to_l2(x):  # [rows, 3, 3, P] -> [rows, 5, P]
        s2, s6 = math.sqrt(2.0), math.sqrt(6.0)
        return np.stack([s2 * x[:, 0, 1], s2 * x[:, 1, 2], (2 * x[:, 2, 2] - x[:, 0, 0] - x[:, 1, 1]) / s6, s2 * x[:, 0, 2],
                         (x[:, 0, 0] - x[:, 1, 1]) / s2], 1)

    def abs_to_l2(x):  # the same map with the moduli of its coefficients: how an entrywise bound travels through it
        s2, s6 = math.sqrt(2.0), math.sqrt(6.0)
        return np.stack([s2 * x[:, 0, 1], s2 * x[:, 1, 2], (2 * x[:, 2, 2] + x[:, 0, 0] + x[:, 1, 1]) / s6, s2 * x[:, 0, 2],
                         (x[:, 0, 0] + x[:, 1, 1]) / s2], 1)

    x64 = to_l2(t64)
    x32 = torch.from_numpy(x64.astype(np.float32))  # the spherical path's input: rounded once more, |x32 - x64| <= u |x64|
    sysidx = torch.from_numpy(SYSIDX.astype(np.int32)).to(DEV)
    (cart,) = rt.o3_apply(torch.from_numpy(MATRICES32[:S]).to(DEV), [(t32.to(DEV), "tensor2", sysidx)])
    (sph,) = rt.o3_apply_spherical(table[:S].contiguous(), parity[:S].contiguous(), 8, [(x32.to(DEV), 2, 1, sysidx)])
    # the exact image both paths approximate: R0 T R0^T, R0 the polar factor (for an improper matrix the two signs cancel, and
    # f = sigma (-1)^2 = 1); D^2(R0) to_l2(T) = to_l2(R0 T R0^T) is the oracle identity test_wigner_cpu.py checks
    r0 = _polar(dets)[SYSIDX]
    exact = to_l2(np.einsum("rab,rbdp,rcd->racp", r0, t64, r0))
    d = DEFECT[:S][SYSIDX][:, None, None]
    d2 = np.abs(want[:S, wo.offset(2):wo.offset(3)].reshape(S, 5, 5))[SYSIDX]
    bound_sph = _kernel_bound(d2, x64, 2, _table_bound(2, DEFECT[:S].max()))
    a = np.abs(MATRICES[:S])[SYSIDX]
    bound_cart = abs_to_l2(7 * U * np.einsum("rab,rbdp,rcd->racp", a, np.abs(t64), a)
                           + 5 * d[..., None] * np.abs(t64).sum(axis=(1, 2))[:, None, None, :])
    err_sph = np.abs(sph.double().cpu().numpy() - exact)
    err_cart = np.abs(to_l2(cart.double().cpu().numpy()) - exact)
    err = np.abs(sph.double().cpu().numpy() - to_l2(cart.double().cpu().numpy()))
    print(f"l = 2 against TENSOR2: spherical / bound {(err_sph / bound_sph).max():.3f}, Cartesian / bound "
          f"{(err_cart / bound_cart).max():.3f}, difference / sum {(err / (bound_sph + bound_cart)).max():.3f}")
    assert (err <= bound_sph + bound_cart).all()


def test_l1_sigma_minus_is_the_cross_product_of_two_rotated_vectors(rt, oracle_tables, device_tables):
    want, dets = oracle_tables
    table, parity = device_tables
    g = torch.Generator().manual_seed(11)
    a32, b32 = torch.randn((N, 3, 2), generator=g) * 2, torch.randn((N, 3, 2), generator=g) * 2
    a64, b64 = a32.double().numpy(), b32.double().numpy()
    perm = [1, 2, 0]
    c64 = np.cross(a64, b64, axis=1)
    c32 = torch.from_numpy(c64.astype(np.float32))  # the pseudovector the spherical path gets: |c32 - c64| <= u |c64|
    sysidx = torch.from_numpy(SYSIDX.astype(np.int32)).to(DEV)
    ra, rb = rt.o3_apply(torch.from_numpy(MATRICES32[:S]).to(DEV), [(a32.to(DEV), "vector", sysidx), (b32.to(DEV), "vector", sysidx)])
    (sph,) = rt.o3_apply_spherical(table[:S].contiguous(), parity[:S].contiguous(), 8,
                                   [(c32[:, perm].contiguous().to(DEV), 1, -1, sysidx)])
    # exact image: (R0 a) x (R0 b) = det(R0) R0 (a x b), R0 the polar factor of O
    r0 = _polar(dets)[SYSIDX]
    ea, eb = np.einsum("rab,rbp->rap", r0, a64), np.einsum("rab,rbp->rap", r0, b64)
    exact = np.cross(ea, eb, axis=1)
    d = DEFECT[:S][SYSIDX][:, None, None]
    absm = np.abs(MATRICES[:S])[SYSIDX]
    da = 3 * U * np.einsum("rab,rbp->rap", absm, np.abs(a64)) + 2 * d * np.abs(a64).sum(axis=1, keepdims=True)
    db = 3 * U * np.einsum("rab,rbp->rap", absm, np.abs(b64)) + 2 * d * np.abs(b64).sum(axis=1, keepdims=True)

    def abs_cross(x, y):
        return np.stack([x[:, 1] * y[:, 2] + x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] + x[:, 0] * y[:, 2],
                         x[:, 0] * y[:, 1] + x[:, 1] * y[:, 0]], 1)

    bound_cart = abs_cross(da, np.abs(eb)) + abs_cross(np.abs(ea), db) + abs_cross(da, db)
    d1 = np.abs(want[:S, 1:10].reshape(S, 3, 3))[SYSIDX]
    bound_sph = _kernel_bound(d1, c64[:, perm], 1, _table_bound(1, DEFECT[:S].max()))
    got_cart = np.cross(ra.double().cpu().numpy(), rb.double().cpu().numpy(), axis=1)[:, perm]
    got_sph = sph.double().cpu().numpy()
    err = np.abs(got_sph - got_cart)
    total = bound_sph + bound_cart[:, perm]
    print(f"l = 1, sigma = -1 against the cross product: spherical / bound {(np.abs(got_sph - exact[:, perm]) / bound_sph).max():.3f}, "
          f"difference / sum {(err / total).max():.3f}")
    assert (err <= total).all()
    # improper systems did NOT flip the pseudovector, proper and improper ones both moved it
    assert float(np.abs(got_sph - c64[:, perm]).max()) > 0.1


# ---- NaN, zero rows, exactness, system index ---------------------------------------------------------------------------------------
def test_a_nan_takes_its_multiplet_and_nothing_else_and_zero_stays_zero(rt, device_tables):
    table, parity = device_tables
    table, parity = table[:S].contiguous(), parity[:S].contiguous()
    sysidx = torch.from_numpy(SYSIDX.astype(np.int32)).to(DEV)
    g = torch.Generator().manual_seed(12)
    x3, x8 = torch.randn((N, 7, 5), generator=g).to(DEV), torch.randn((S, 17, 5), generator=g).to(DEV)
    x3[200:210] = 0.0  # zero rows inside system 4
    x8[2, :, 1] = 0.0  # a zero multiplet
    clean3, clean8 = rt.o3_apply_spherical(table, parity, 8, [(x3, 3, -1, sysidx), (x8, 8, 1, None)])
    assert bool((clean3[200:210] == 0).all()) and bool((clean8[2, :, 1] == 0).all())
    assert bool((clean3[199] != 0).all()) and bool((clean8[2, :, 0] != 0).all())
    y3, y8 = x3.clone(), x8.clone()
    y3[100, 2, 3] = float("nan")  # row 100, m = -1, property 3
    y8[4, 16, 0] = float("nan")
    out3, out8 = rt.o3_apply_spherical(table, parity, 8, [(y3, 3, -1, sysidx), (y8, 8, 1, None)])
    assert bool(torch.isnan(out3[100, :, 3]).all()) and bool(torch.isnan(out8[4, :, 0]).all())
    out3[100, :, 3], out8[4, :, 0] = clean3[100, :, 3], clean8[4, :, 0]
    assert torch.equal(out3, clean3) and torch.equal(out8, clean8)  # every other multiplet, those of the same row included


def test_a_system_index_outside_the_batch_is_not_followed(rt, device_tables):
    table, parity = device_tables
    table, parity = table[:S].contiguous(), parity[:S].contiguous()
    g = torch.Generator().manual_seed(13)
    x = torch.randn((N, 5, 2), generator=g).to(DEV)
    good = torch.from_numpy(SYSIDX.astype(np.int32)).to(DEV)
    (clean,) = rt.o3_apply_spherical(table, parity, 8, [(x, 2, 1, good)])
    bad = good.clone()
    bad[0], bad[70], bad[300], bad[N - 1] = -1, S, -1, 2**31 - 1  # first lane of a wave, inside a wave, the last row
    (out,) = rt.o3_apply_spherical(table, parity, 8, [(x, 2, 1, bad)])
    rows = [0, 70, 300, N - 1]
    assert bool(torch.isnan(out[rows]).all())
    out[rows] = clean[rows]
    assert torch.equal(out, clean)


def _all_kinds():
    return {f"t{l}{'p' if sigma > 0 else 'm'}": {"kind": "spherical", "o3_lambda": l, "o3_sigma": sigma}
            for l in range(9) for sigma in (1, -1)}


def _apply_batch(extra):
    g = torch.Generator().manual_seed(3)
    batch = {
        "positions": torch.rand((N, 3), generator=g) * 20 - 4,
        "cells": torch.eye(3).repeat(S, 1, 1) * 11.0,
        "centers": torch.arange(10, dtype=torch.int32),
        "neighbors": torch.arange(10, dtype=torch.int32).flip(0).contiguous(),
        "cell_shifts": torch.zeros((10, 3), dtype=torch.int32),
        "species": torch.ones(N, dtype=torch.int32),
        "system_indices": torch.from_numpy(SYSIDX.astype(np.int32)),
    }
    batch.update(extra)
    return {k: v.to(DEV) for k, v in batch.items()}


def test_inversions_give_exactly_plus_or_minus_the_input(rt):
    from metatrain_amd.augmentation import O3Augmenter

    g = torch.Generator().manual_seed(14)
    kinds = _all_kinds()
    targets = {name: torch.randn((N if k["o3_lambda"] % 2 else S, (2 * k["o3_lambda"] + 1) * 2), generator=g)
               for name, k in kinds.items()}
    batch = _apply_batch(targets)
    aug = O3Augmenter(kinds, group="inversions", seed=4)
    out = aug.apply_random_augmentations(batch)
    parity = out["o3_parity"].cpu()
    assert set(parity.tolist()) == {1.0, -1.0}  # both signs among the five systems (seed 4), or the test shows nothing
    assert torch.equal(out["o3_matrices"].cpu(), parity[:, None, None] * torch.eye(3))
    assert aug.l_max == 8 and out["o3_wigner"].shape == (S, 969)
    for name, k in kinds.items():
        per_row = parity[torch.from_numpy(SYSIDX)] if k["o3_lambda"] % 2 else parity
        f = torch.where(per_row < 0, torch.tensor(float(k["o3_sigma"] * (-1) ** k["o3_lambda"])), torch.tensor(1.0))[:, None]
        if (k["o3_lambda"], k["o3_sigma"]) == (0, 1):
            assert out[name] is batch[name]  # an invariant is not touched at all
        else:
            assert torch.equal(out[name].cpu(), f * batch[name].cpu()), name


# ---- determinism ----------------------------------------------------------------------------------------------------------------------
def test_the_same_rows_give_the_same_bits_whatever_else_is_in_the_call(rt, device_tables):
    table, parity = device_tables
    mats = torch.from_numpy(MATRICES32[:S]).to(DEV)
    table5, parity5 = rt.o3_wigner(mats, 8)
    assert torch.equal(table5, table[:S]) and torch.equal(parity5, parity[:S])  # a system's table does not depend on the batch
    assert torch.equal(rt.o3_wigner(mats, 8)[0], table5)
    sysidx = torch.from_numpy(SYSIDX.astype(np.int32)).to(DEV)
    dev = [(x.to(DEV), l, sigma, sysidx if per_atom else None) for x, l, sigma, per_atom in _arrays()[30:46]]
    first = rt.o3_apply_spherical(table5, parity5, 8, dev)
    again = rt.o3_apply_spherical(table5, parity5, 8, dev)
    backwards = rt.o3_apply_spherical(table5, parity5, 8, dev[::-1])[::-1]
    for a, b, c in zip(first, again, backwards):
        assert torch.equal(a, b) and torch.equal(a, c)
    # a smaller batch: the first three systems (66 atoms) alone, so rows sit in other lanes, waves and workgroups' company
    n3 = sum(SIZES[:3])
    table3, parity3 = rt.o3_wigner(mats[:3], 8)
    small = [(x[:n3 if sor is not None else 3].contiguous(), l, sigma, None if sor is None else sor[:n3].contiguous())
             for x, l, sigma, sor in dev]
    for a, want in zip(rt.o3_apply_spherical(table3, parity3, 8, small), first):
        assert a.shape[0] in (3, n3) and torch.equal(a, want[:a.shape[0]])


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
E2E_KINDS = {"energy": "scalar", "forces": "vector",
             "mp_l0": {"kind": "spherical", "o3_lambda": 0, "o3_sigma": 1}, "mp_l1": {"kind": "spherical", "o3_lambda": 1, "o3_sigma": 1},
             "mp_l2": {"kind": "spherical", "o3_lambda": 2, "o3_sigma": 1}, "mp_l3": {"kind": "spherical", "o3_lambda": 3, "o3_sigma": 1},
             "chirality": {"kind": "spherical", "o3_lambda": 0, "o3_sigma": -1}}
E2E_SIZES = (6, 1, 9)
E2E_WEIGHTS = np.random.default_rng(21).standard_normal((sum(E2E_SIZES), 2))  # two properties


def _multipoles(positions: np.ndarray, l: int) -> np.ndarray:
    """``t_l[s, m, p] = sum_j w[j, p] |r_j - r_0|^l Y_l(r_j - r_0)`` over the atoms of system ``s``, in fp64: an equivariant
    function of the positions, of parity ``(-1)^l`` (``o3_sigma = +1``)."""
    out, first = [], 0
    for k in E2E_SIZES:
        r = positions[first:first + k] - positions[first]
        out.append(np.einsum("jm,jp->mp", wo.solid_harmonics(l, r), E2E_WEIGHTS[first:first + k]))
        first += k
    return np.stack(out)


@pytest.fixture(scope="module")
def multipole_batch(rt):
    from metatrain_amd import data

    rng = np.random.default_rng(22)
    systems, first = [], 0
    for k in E2E_SIZES:
        pos = torch.from_numpy(rng.uniform(1.0, 3.0, (k, 3))).float()
        systems.append((pos.to(DEV), torch.full((k,), 6, dtype=torch.int32, device=DEV), torch.eye(3) * 9.0, [True] * 3))
    pos64 = torch.cat([s[0] for s in systems]).double().cpu().numpy()
    g = torch.Generator().manual_seed(23)
    targets = {"energy": [torch.randn(1, generator=g) for _ in E2E_SIZES], "forces": [torch.randn((k, 3), generator=g) for k in E2E_SIZES],
               "chirality": [torch.randn((1, 1), generator=g) for _ in E2E_SIZES]}
    for l in range(4):
        t = _multipoles(pos64, l).astype(np.float32)  # rounded once: the stored target
        targets[f"mp_l{l}"] = [torch.from_numpy(t[s:s + 1]) for s in range(len(E2E_SIZES))]
    return data.collate(systems, float(opet.DEFAULT_HYPERS["cutoff"]), targets)


def test_end_to_end_multipoles_follow_the_positions(rt, multipole_batch):
    from metatrain_amd.augmentation import O3Augmenter

    batch = multipole_batch
    aug = O3Augmenter(E2E_KINDS, seed=6, stream=1)
    assert aug.l_max == 3
    state = aug.state_dict()
    rt.profile(True)
    out = aug.apply_random_augmentations(batch)
    calls = {r["name"]: r["calls"] for r in rt.profile_report()}
    rt.profile(False)
    assert calls == {"o3_draw": 1, "o3_apply": 1, "o3_wigner": 1, "o3_apply_spherical": 1}, calls  # two launches more
    assert aug.counter == 1 and set(out) == set(batch) | {"o3_matrices", "o3_wigner", "o3_parity"}
    assert out["o3_wigner"].shape == (3, wo.width(3)) and out["mp_l0"] is batch["mp_l0"] and out["energy"] is batch["energy"]
    second = aug.apply_random_augmentations(batch)
    assert aug.counter == 2 and not torch.equal(second["o3_matrices"], out["o3_matrices"])
    resumed = O3Augmenter(E2E_KINDS)
    resumed.load_state_dict(state)
    for want in (out, second):
        got = resumed.apply_random_augmentations(batch)
        for k in ("o3_matrices", "o3_wigner", "o3_parity", "positions", "forces", "mp_l1", "mp_l2", "mp_l3", "chirality"):
            assert torch.equal(got[k], want[k]), k
    assert resumed.counter == 2

    mats = out["o3_matrices"].double().cpu().numpy()
    dets = out["o3_parity"].double().cpu().numpy()
    assert np.array_equal(dets, np.sign(np.linalg.det(mats)))
    assert float(np.abs(mats - np.eye(3)).max()) > 0.1
    assert torch.equal(out["chirality"].cpu(), batch["chirality"].cpu() * out["o3_parity"].cpu()[:, None])
    pos0, pos1 = batch["positions"].double().cpu().numpy(), out["positions"].double().cpu().numpy()
    defect = np.abs(np.einsum("sji,sjk->sik", mats, mats) - np.eye(3)).max()
    for l in range(1, 4):
        stored = batch[f"mp_l{l}"].double().cpu().numpy()  # the fp32 targets the kernel read
        exact0 = _multipoles(pos0, l)
        d_exact = np.stack([wo.wigner_d(l, det * m) for m, det in zip(mats, dets)])
        f = np.where(dets < 0, (-1.0) ** l, 1.0)[:, None, None]
        image = f * np.einsum("smk,skp->smp", d_exact, exact0)  # the exact target, exactly rotated
        from_positions = _multipoles(pos1, l)  # the target of the rotated fp32 positions
        position_term = np.abs(from_positions - image)  # what rounding the positions to fp32 costs: measured, not guessed
        bound = _kernel_bound(d_exact, exact0, l, _table_bound(l, defect))
        err = np.abs(out[f"mp_l{l}"].double().cpu().numpy() - from_positions)
        print(f"l = {l}: max |augmented target - target of augmented positions| = {err.max():.3e}, kernel bound up to {bound.max():.3e}, "
              f"position term up to {position_term.max():.3e}, |target| up to {np.abs(stored).max():.3e}")
        assert (err <= bound + position_term).all(), l
        assert float(np.abs(out[f"mp_l{l}"].double().cpu().numpy() - stored)[[0, 2]].max()) > 1e-2  # it did move
    assert bool((out["mp_l2"][1] == 0).all())  # the one-atom system: r_0 - r_0, a zero multiplet

    # the same through given matrices, improper ones included; the counter does not move
    given = aug.apply_augmentations(batch, out["o3_matrices"])
    for k in ("positions", "forces", "mp_l1", "mp_l2", "mp_l3", "chirality", "o3_wigner", "o3_parity"):
        assert torch.equal(given[k], out[k]), k
    assert aug.counter == 2


def test_a_batch_without_spherical_kinds_is_as_before(rt, multipole_batch):
    from metatrain_amd.augmentation import O3Augmenter

    batch = {k: v for k, v in multipole_batch.items() if not k.startswith("mp_") and k != "chirality"}
    rt.profile(True)
    out = O3Augmenter({"energy": "scalar", "forces": "vector"}, seed=6, stream=1).apply_random_augmentations(batch)
    calls = {r["name"]: r["calls"] for r in rt.profile_report()}
    rt.profile(False)
    assert calls == {"o3_draw": 1, "o3_apply": 1}, calls
    assert set(out) == set(batch) | {"o3_matrices"}
    # scalars under the new spelling pass through too, and need no table
    kinds = {"energy": {"kind": "spherical", "o3_lambda": 0, "o3_sigma": 1}, "forces": "vector"}
    again = O3Augmenter(kinds, seed=6, stream=1).apply_random_augmentations(batch)
    assert set(again) == set(out) and torch.equal(again["forces"], out["forces"]) and again["energy"] is batch["energy"]
