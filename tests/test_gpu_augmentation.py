"""GPU tests of the device augmenter (``metatrain_amd/augmentation.py``; ``csrc/augment.hip``: ``pet_o3_draw``,
``pet_o3_apply``) against fp64 torch written here -- ``x @ R.T`` is the whole reference -- and, end to end, against the CPU
oracle at the project's standing 1e-5 bar.

Tolerances of the apply tests: ``|out - ref| <= 1e-6 x (largest row norm of the array)`` for vectors (fp32 rounding of the
matrix, three products and two sums), ``2e-6 x`` for rank-2 tensors (two such contractions). Bounds of the distribution
tests: 5 sigma of each statistic under the Haar measure at the sample size used; the seed is fixed, so they are
deterministic.
"""
import math

import numpy as np
import pytest
import torch

from oracle import nl as onl
from oracle import pet as opet

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CUTOFF = float(opet.DEFAULT_HYPERS["cutoff"])
SIZES = (1, 2, 63, 65, 300)  # 431 atoms: system boundaries inside a wave, a one-atom system, more than one workgroup
N, S = sum(SIZES), len(SIZES)


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from metatrain_amd import runtime

    return runtime


def _orthogonal(seed: int, proper: bool) -> torch.Tensor:
    """A fixed orthogonal matrix made in fp64 on the CPU (QR of a seeded matrix), of the requested determinant."""
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))
    if (torch.linalg.det(q) > 0) != proper:
        q = -q
    assert abs(float(torch.linalg.det(q)) - (1.0 if proper else -1.0)) < 1e-12
    return q


MATRICES = torch.stack([_orthogonal(11, True), _orthogonal(12, False), _orthogonal(13, True), _orthogonal(14, False),
                        _orthogonal(15, True)])  # three proper, two improper


def _apply_batch():
    g = torch.Generator().manual_seed(3)
    sysidx = torch.cat([torch.full((k,), i, dtype=torch.int32) for i, k in enumerate(SIZES)])
    cells = torch.stack([torch.zeros(3, 3),  # not periodic
                         torch.tensor([[9.0, 0.0, 0.0], [2.5, 8.0, 0.0], [-1.5, 3.0, 7.0]]),  # triclinic
                         torch.eye(3) * 11.0, torch.eye(3) * 12.5, torch.diag(torch.tensor([15.0, 17.0, 19.0]))])
    batch = {
        "positions": torch.rand((N, 3), generator=g) * 20 - 4,
        "cells": cells,
        "centers": torch.arange(10, dtype=torch.int32),
        "neighbors": torch.arange(10, dtype=torch.int32).flip(0).contiguous(),
        "cell_shifts": torch.zeros((10, 3), dtype=torch.int32),
        "species": torch.ones(N, dtype=torch.int32),
        "system_indices": sysidx,
        "energy": torch.randn((S, 1), generator=g),
        "f1": torch.randn((N, 3), generator=g),
        "f4": torch.randn((N, 12), generator=g) * 3,
        "stress": torch.randn((S, 3, 3), generator=g),
        "t2": torch.randn((N, 18), generator=g),
        "f1_mask": torch.ones((N, 3), dtype=torch.bool),
    }
    return {k: v.to(DEV) for k, v in batch.items()}


KINDS = {"energy": "scalar", "f1": "vector", "f4": "vector", "stress": "tensor2", "t2": "tensor2"}


def _ref_vector(x, mats_of_row):
    r = x.shape[0]
    return torch.einsum("rab,rbp->rap", mats_of_row, x.double().cpu().reshape(r, 3, -1)).reshape(x.shape)


def _ref_tensor2(x, mats_of_row):
    r = x.shape[0]
    return torch.einsum("rab,rbdp,rcd->racp", mats_of_row, x.double().cpu().reshape(r, 3, 3, -1), mats_of_row).reshape(x.shape)


def _check(name, out, ref, factor):
    rows = ref.reshape(ref.shape[0], -1)
    scale = float(rows.norm(dim=1).max())
    err = float((out.double().cpu() - ref).abs().max())
    print(f"{name}: max |out - ref| = {err:.3e}, bound {factor * scale:.3e}")
    assert err <= factor * scale, name


def test_apply_matches_fp64(rt):
    from metatrain_amd.augmentation import O3Augmenter

    batch = _apply_batch()
    before = {k: v.clone() for k, v in batch.items()}
    aug = O3Augmenter(KINDS)
    out = aug.apply_augmentations(batch, MATRICES)
    per_atom = MATRICES[batch["system_indices"].long().cpu()]
    _check("positions", out["positions"], _ref_vector(batch["positions"], per_atom), 1e-6)
    _check("cells", out["cells"].reshape(3 * S, 3), _ref_vector(batch["cells"].reshape(3 * S, 3), MATRICES.repeat_interleave(3, 0)),
           1e-6)
    assert torch.allclose(out["cells"].double().cpu(), batch["cells"].double().cpu() @ MATRICES.transpose(1, 2), atol=2e-5)
    _check("f1", out["f1"], _ref_vector(batch["f1"], per_atom), 1e-6)
    _check("f4", out["f4"], _ref_vector(batch["f4"], per_atom), 1e-6)
    _check("stress", out["stress"], _ref_tensor2(batch["stress"], MATRICES), 2e-6)
    _check("t2", out["t2"], _ref_tensor2(batch["t2"], per_atom), 2e-6)
    assert out["positions"].shape == batch["positions"].shape and out["cells"].shape == (S, 3, 3)
    assert bool((out["cells"][0] == 0).all()), "the zero cell of a non-periodic system must stay exactly zero"
    for k, v in before.items():  # the cached batch survives
        assert torch.equal(batch[k], v), k
    for k in ("centers", "neighbors", "cell_shifts", "species", "system_indices", "energy", "f1_mask"):
        assert out[k] is batch[k], k
    for k in ("positions", "cells", "f1", "f4", "stress", "t2"):
        assert out[k].data_ptr() != batch[k].data_ptr(), k
    assert torch.equal(out["o3_matrices"].cpu(), MATRICES.float())
    assert aug.counter == 0


def test_a_nan_takes_its_whole_vector_or_tensor_and_nothing_else(rt):
    from metatrain_amd.augmentation import O3Augmenter

    batch = _apply_batch()
    clean = O3Augmenter(KINDS).apply_augmentations(batch, MATRICES)
    batch["f4"] = batch["f4"].clone()
    batch["f4"][100, 1 * 4 + 2] = float("nan")  # row 100, component y of property 2
    batch["t2"] = batch["t2"].clone()
    batch["t2"][7, (3 * 2 + 0) * 2 + 1] = float("nan")  # row 7, component zx of property 1
    out = O3Augmenter(KINDS).apply_augmentations(batch, MATRICES)
    f4, c4 = out["f4"].reshape(N, 3, 4).cpu(), clean["f4"].reshape(N, 3, 4).cpu()
    assert bool(torch.isnan(f4[100, :, 2]).all())
    f4[100, :, 2] = c4[100, :, 2]
    assert torch.equal(f4, c4)  # every other vector, the other properties of row 100 included, is untouched
    t2, c2 = out["t2"].reshape(N, 9, 2).cpu(), clean["t2"].reshape(N, 9, 2).cpu()
    assert bool(torch.isnan(t2[7, :, 1]).all())
    t2[7, :, 1] = c2[7, :, 1]
    assert torch.equal(t2, c2)
    for k in ("positions", "cells", "f1", "stress"):
        assert torch.equal(out[k], clean[k]), k


# ---- the generator ------------------------------------------------------------------------------------------------------
def _philox4x32_10(counter, key):
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k[0]) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k[1]) & 0xFFFFFFFF, p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def _host_matrix(key, counter, system, group):
    """The documented recipe in Python floats (fp64): Philox block (counter low, counter high, system, 0) -> Shoemake."""
    w = _philox4x32_10([counter & 0xFFFFFFFF, counter >> 32, system, 0], [key & 0xFFFFFFFF, key >> 32])
    sign = -1.0 if w[3] >> 31 else 1.0
    if group == "inversions":
        return sign * np.eye(3)
    u1, u2, u3 = [(v + 0.5) / 2.0**32 for v in w[:3]]
    a, b = math.sqrt(1 - u1), math.sqrt(u1)
    x, y, z, q = a * math.sin(2 * math.pi * u2), a * math.cos(2 * math.pi * u2), b * math.sin(2 * math.pi * u3), b * math.cos(2 * math.pi * u3)
    return sign * np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * q), 2 * (x * z + y * q)],
                            [2 * (x * y + z * q), 1 - 2 * (x * x + z * z), 2 * (y * z - x * q)],
                            [2 * (x * z - y * q), 2 * (y * z + x * q), 1 - 2 * (x * x + y * y)]])


def test_the_generator_is_the_documented_one(rt):
    """Philox-4x32-10 known answers (the Random123 test vectors), then the device's matrices against the recipe on the host:
    a matrix depends on (key, counter, system ordinal) and nothing else."""
    assert _philox4x32_10([0] * 4, [0] * 2) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert _philox4x32_10([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert _philox4x32_10([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0]) == [
        0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    key, counter = (5 << 32) | 1234, (3 << 32) | 17
    got = rt.o3_draw(300, key, counter, "O3", DEV).double().cpu().numpy()
    for s in (0, 1, 63, 64, 255, 256, 299):
        assert np.abs(got[s] - _host_matrix(key, counter, s, "O3")).max() <= 1e-7, s
    got = rt.o3_draw(70, key, counter, "inversions", DEV).double().cpu().numpy()
    for s in (0, 1, 63, 64, 69):
        assert np.array_equal(got[s], _host_matrix(key, counter, s, "inversions")), s


def _entry_and_share_checks(m, scale):
    det = torch.linalg.det(m)
    share = float((det < 0).double().mean())
    means = m.mean(0)
    print(f"improper share {share:.4f}, largest entry mean {float(means.abs().max()):.4f}")
    assert abs(share - 0.5) <= 0.028 * scale
    assert float(means.abs().max()) <= 0.032 * scale


def test_drawn_matrices_are_orthogonal_and_haar(rt):
    n = 8192
    m = rt.o3_draw(n, 2024, 0, "O3", DEV).double().cpu()
    eye = torch.eye(3, dtype=torch.float64)
    ortho = float((m.transpose(1, 2) @ m - eye).abs().max())
    det = torch.linalg.det(m)
    print(f"max |R^T R - I| = {ortho:.3e}, max ||det| - 1| = {float((det.abs() - 1).abs().max()):.3e}")
    assert ortho <= 1e-6
    assert float((det.abs() - 1).abs().max()) <= 1e-6
    _entry_and_share_checks(m, 1.0)
    sq = (m ** 2).mean(0)
    print(f"largest |mean of a squared entry - 1/3| = {float((sq - 1 / 3).abs().max()):.4f}")
    assert float((sq - 1.0 / 3.0).abs().max()) <= 0.0165
    proper = m[det > 0]
    trace = float(torch.diagonal(proper, dim1=1, dim2=2).sum(1).mean())
    print(f"mean trace over {proper.shape[0]} proper matrices = {trace:.4f}")
    assert abs(trace) <= 0.08  # uniform-angle sampling gives 1


def test_successive_calls_are_uncorrelated_along_the_counter(rt):
    first = torch.stack([rt.o3_draw(3, 2024, c, "O3", DEV)[0] for c in range(2048)]).double().cpu()
    _entry_and_share_checks(first, 2.0)


def test_inversions_are_plus_or_minus_identity(rt):
    m = rt.o3_draw(8192, 2024, 0, "inversions", DEV).cpu()
    eye = torch.eye(3)
    plus, minus = (m == eye).all(dim=(1, 2)), (m == -eye).all(dim=(1, 2))
    assert bool((plus | minus).all())
    assert abs(float(minus.double().mean()) - 0.5) <= 0.028
    # the sign bit is the one the O3 group uses: the same systems are improper
    assert torch.equal(minus, torch.linalg.det(rt.o3_draw(8192, 2024, 0, "O3", DEV).cpu()) < 0)


def test_determinism_and_independence(rt):
    from metatrain_amd.augmentation import O3Augmenter

    small = {k: v for k, v in _apply_batch().items()}
    base = O3Augmenter(KINDS, seed=9, stream=2)
    assert base.key == (2 << 32) | 9
    a = rt.o3_draw(5, base.key, 0, "O3", DEV)
    assert torch.equal(a, rt.o3_draw(5, base.key, 0, "O3", DEV))  # the same (seed, stream, counter): the same bits
    assert torch.equal(a, rt.o3_draw(8192, base.key, 0, "O3", DEV)[:5])  # whatever else is drawn
    assert torch.equal(a, base.apply_random_augmentations(small)["o3_matrices"])
    assert base.counter == 1

    def differs_everywhere(b):
        return bool((a != b).any(dim=(1, 2)).all())

    assert differs_everywhere(rt.o3_draw(5, base.key, 1, "O3", DEV))  # another counter
    assert differs_everywhere(O3Augmenter(KINDS, seed=9, stream=3).apply_random_augmentations(small)["o3_matrices"])
    assert differs_everywhere(O3Augmenter(KINDS, seed=10, stream=2).apply_random_augmentations(small)["o3_matrices"])
    # seed and stream are different words of the key: (seed 2, stream 9) is not (seed 9, stream 2)
    assert differs_everywhere(O3Augmenter(KINDS, seed=2, stream=9).apply_random_augmentations(small)["o3_matrices"])
    # resume: the saved state reproduces the next three draws
    for _ in range(4):
        base.apply_random_augmentations(small)
    state = base.state_dict()
    assert state["counter"] == 5
    ahead = [base.apply_random_augmentations(small) for _ in range(3)]
    resumed = O3Augmenter(KINDS)
    resumed.load_state_dict(state)
    for want in ahead:
        got = resumed.apply_random_augmentations(small)
        for k in ("o3_matrices", "positions", "cells", "f4", "t2"):
            assert torch.equal(got[k], want[k]), k
    assert not torch.equal(ahead[0]["o3_matrices"], ahead[1]["o3_matrices"])


# ---- the pair list is reusable; end to end ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box64(rt):
    """A 64-atom periodic box of the synthetic generator, perturbed until no pair distance (periodic images included) lies
    within 1e-3 A of the cutoff -- asserted here on the CPU -- and collated once with an energy and a force target."""
    from metatrain_amd import data

    pos, z, cell = opet.random_box(64, 21)
    gen = torch.Generator().manual_seed(77)

    def closest(p):
        _, _, _, d = onl.neighbor_list(p.double().numpy(), cell.double().numpy(), [True] * 3, CUTOFF + 0.05)
        return float(np.abs(np.linalg.norm(d, axis=1) - CUTOFF).min())

    for _ in range(50):
        if closest(pos) > 1e-3:
            break
        pos = pos + 0.01 * torch.randn(pos.shape, generator=gen)
    gap = closest(pos)
    assert gap > 1e-3, gap
    forces = torch.randn((64, 3), generator=gen)
    batch = data.collate([(pos.to(DEV), z.to(DEV), cell, [True] * 3)], CUTOFF,
                         {"energy": [torch.tensor([-3.5])], "forces": [forces.to(DEV)]})
    return batch


def _sorted_rows(centers, neighbors, shifts):
    rows = torch.cat([centers.reshape(-1, 1), neighbors.reshape(-1, 1), shifts.reshape(-1, 3)], 1).cpu().numpy()
    return rows[np.lexsort((rows[:, 4], rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))]


@pytest.mark.parametrize("proper", [True, False])
def test_the_pair_list_of_the_original_serves_the_rotated_structure(rt, box64, proper):
    from metatrain_amd.augmentation import O3Augmenter

    out = O3Augmenter({"energy": "scalar", "forces": "vector"}).apply_augmentations(box64, _orthogonal(31, proper)[None])
    assert out["centers"] is box64["centers"] and out["cell_shifts"] is box64["cell_shifts"]
    pairs, _ = rt.neighbor_list_batch(out["positions"], out["cells"].cpu(), [[True] * 3], [0, 64], CUTOFF, want_vectors=False)
    cached = _sorted_rows(box64["centers"], box64["neighbors"], box64["cell_shifts"])
    fresh = _sorted_rows(pairs[:, 0], pairs[:, 1], pairs[:, 2:5])
    assert cached.shape[0] > 64 * 10
    assert np.array_equal(fresh, cached)


def test_end_to_end_at_the_parity_bar(rt, box64):
    from metatrain_amd import data
    from metatrain_amd.augmentation import O3Augmenter
    from metatrain_amd.pet.trainer import TrainStep

    hypers, types = dict(opet.DEFAULT_HYPERS), [1, 6, 7, 8]
    params = opet.synthetic_params(hypers, types, {"energy": 1}, 0, torch.float32)
    model = rt.HipModel(hypers, types)
    model.load({k: v.to(DEV) for k, v in params.items()}, "energy")
    aug = O3Augmenter({"energy": "scalar", "forces": "vector"}, seed=5)
    out = aug.apply_random_augmentations(box64)
    R = out["o3_matrices"][0].double().cpu()
    assert float((R - torch.eye(3, dtype=torch.float64)).abs().max()) > 0.1  # a real rotation, not a near-identity draw

    graph = data.graph_of(model, out)  # the cached pair list, the rotated geometry
    fw = rt.HipForward(model, graph)
    atomic = fw.forward()
    grad = fw.backward(torch.ones_like(atomic))

    p64 = {k: (v if k == "species_to_species_index" else v.double()) for k, v in params.items()}
    pos = out["positions"].double().cpu().requires_grad_(True)
    ref = opet.pet_atomic_energies(p64, hypers, pos, out["cells"].double().cpu(), out["centers"].long().cpu(),
                                   out["neighbors"].long().cpu(), out["cell_shifts"].long().cpu(), out["species"].cpu(),
                                   out["system_indices"].long().cpu())[:, 0]
    (ref_grad,) = torch.autograd.grad(ref.sum(), pos)
    e_err = float((atomic.double().cpu().reshape(-1) - ref.detach()).abs().max() / ref.detach().abs().max())
    g_err = float((grad.double().cpu() - ref_grad).abs().max() / ref_grad.abs().max())
    print(f"per-atom energies relmax {e_err:.3e}, dE/dR relmax {g_err:.3e}")
    assert e_err < 1e-5 and g_err < 1e-5

    want_forces = box64["forces"].double().cpu() @ R.T
    assert float((out["forces"].double().cpu() - want_forces).abs().max()) <= 1e-6 * float(want_forces.norm(dim=1).max())
    assert out["energy"] is box64["energy"]

    # an augmenter that silently does nothing would leave the (not invariant) model's energies where they were
    g0 = data.graph_of(model, box64)
    atomic0 = rt.HipForward(model, g0).forward()
    assert float((atomic - atomic0).abs().max()) > 1e-4

    train_fw = rt.HipForward(model, graph, train=True)
    step = TrainStep(model, {"learning_rate": 1e-4, "warmup_fraction": 0.0, "num_epochs": 10**9})
    res = step(graph, train_fw, out["energy"].reshape(-1), torch.tensor([64.0], device=DEV), target_gradients=-out["forces"])
    assert math.isfinite(float(res["loss"])) and math.isfinite(float(res["grad_norm"]))
