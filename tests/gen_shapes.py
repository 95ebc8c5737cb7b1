"""Sizes of the size-generic PET pass (``csrc/gen_common.h``, ``gen.hip``, ``gen_train.hip``) chosen for the boundaries
its kernels tile by, two inputs, and ONE fp64 / fp32 oracle evaluation per (case, input) that returns everything
``tests/test_gpu_gen_shapes.py`` and ``tests/test_gen_shapes_cpu.py`` compare with.

The kernels dispatch at run time: ``attn_dispatch`` on the head dimension (buckets ``HDM`` = 4, 16, 32, 64, 128; a lane owns
a slice of 16 features, the last one may be partial, ``v4`` loads need head dimension and ``d_pet`` divisible by 4),
``k_gen_lin`` / ``k_gt_wgrad`` on ``K % 4``, ``NO % 4``, 32-wide K chunks and 64-wide output tiles, the norm kernels on four
rows per block. Each case below names the boundary it is here for.

Bar (``test_gpu_hvp.py``, ``test_gpu_fp32_floor.py``): ``relmax = max|got - ref| / max|ref| <= max(1e-5, 2 y)`` with ``y`` the
relmax of the fp32 oracle against the fp64 oracle for the same quantity and input; a pair pins something only if
``y <= 1e-3``. For parameter gradients: per parameter tensor, tensors whose reference maximum is below 1e-12 absolutely."""
import functools
import os

import numpy as np
import torch

from oracle import nl as onl
from oracle import pet as opet
from test_gpu_hvp import dense_cluster

from _memo import memo_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TYPES = [1, 6, 7, 8]
Y_CAP = 1e-3
FLOOR = 1e-5


def _size(d_pet, d_node, d_ff, d_head, heads, **extra):
    return dict(d_pet=d_pet, d_node=d_node, d_feedforward=d_ff, d_head=d_head, num_heads=heads, **extra)


LEGACY = dict(normalization="LayerNorm", activation="SiLU", transformer_type="PostLN", featurizer_type="residual")
CASES = {
    # head dimension 3 -> HDM 4: partial slice in the smallest bucket; every linear on the scalar path
    "hd3": _size(6, 10, 7, 5, 2),
    # 11 -> 16: scalar k_gen_lin in both orientations; K = 32 + 1; no v4 slice loads
    "odd33": _size(33, 35, 37, 29, 3),
    # the same tails through the tied [W; W] input projection, PostLN buffers and two read-out layers
    "odd33_legacy": _size(33, 35, 37, 29, 3, **LEGACY),
    # 12 -> 16: v4 slice loads with a partial slice; K = 36 and 20 on the V4 path; the Cosine second derivative in the HVP
    "hd12": _size(36, 72, 20, 12, 3, num_gnn_layers=1, num_attention_layers=3, cutoff_function="Cosine"),
    # 13 -> 16: tiles crossed by one column (65, 130, 195); conditioning kernels at DN = 130
    "k65": _size(65, 130, 65, 65, 5, system_conditioning=True),
    # 24 -> 32: first launch of the 32 bucket, nv = 8; d_node unrelated to d_pet; K = 72
    "hd24": _size(48, 80, 72, 36, 2),
    # 32 -> 32: full 32 bucket; d_node == d_pet
    "hd32": _size(64, 64, 96, 40, 2),
    # 48 -> 64: 64 bucket with an idle slice; first training launch at HDM = 64; d_node < d_pet
    "hd48": _size(96, 48, 40, 24, 2, num_gnn_layers=3, num_attention_layers=1),
    # 96 -> 128: first launch of the 128 bucket, 6 of 8 slices live; NO = 68 and 200; one head
    "hd96": _size(96, 96, 100, 68, 1),
    # 128 -> 128: the largest head dimension pet_hypers_supported admits, at a size that is not the compiled one
    "hd128": _size(128, 128, 64, 32, 1),
}
ON_CLUSTER = ("hd3", "hd24", "hd48", "hd96", "odd33_legacy", "k65")   # one per bucket, the legacy variant, the conditioned model
PAIRS = [(tag, "a") for tag in CASES] + [(tag, "b") for tag in ON_CLUSTER]
BUCKETS = (4, 16, 32, 64, 128)


def head_dim(tag):
    return CASES[tag]["d_pet"] // CASES[tag]["num_heads"]


def hdm_bucket(hd):
    """The thresholds of ``attn_dispatch`` (gen_common.h)."""
    return next(b for b in BUCKETS if hd <= b)


def widths(tag):
    """Every K / NO the linears of a case see: the four sizes, the fused QKV projection and the SwiGLU input projection."""
    c = CASES[tag]
    return {c["d_pet"], c["d_node"], c["d_feedforward"], c["d_head"], 3 * c["d_pet"], 2 * c["d_feedforward"]}


def cluster_properties(inp):
    n, e = inp["positions"].shape[0], inp["centers"].shape[0]
    pos = inp["positions"].numpy()
    d = np.linalg.norm(pos[inp["centers"].numpy()] - pos[inp["neighbors"].numpy()], axis=1)
    tokens = np.bincount(inp["centers"].numpy(), minlength=n) + 1
    return {"n": n, "e": e, "min_distance": float(d.min()), "tokens_over_32": int((tokens > 32).sum()),
            "tokens_over_64": int((tokens > 64).sum()), "central_neighbours": int(tokens[0] - 1)}


def check_cluster(inp):
    """Input (b) reaches the partly filled last block of the four-rows-per-block kernels and the multi-pass / chunk loops of
    every attention bucket (a pass serves 32 tokens at HDM = 32, 16 at 64, 8 at 128; the training attention chunks by 64)."""
    p = cluster_properties(inp)
    n, e = p["n"], p["e"]
    assert (n, e) == (73, 3124), (n, e)
    assert n % 4 == 1 and (e + n) % 4 == 1 and (e + n) % 64 == 61
    assert abs(p["min_distance"] - 1.05) < 0.01, p
    assert p["tokens_over_32"] == 69 and p["tokens_over_64"] == 3 and p["central_neighbours"] == 72, p
    return p


@functools.lru_cache(maxsize=None)
def _input(which):
    if which == "a":   # 104 atoms, 1 908 edges, at most 27 neighbours, two periodic systems
        g = dict(np.load(os.path.join(GOLDEN, "batch_two_systems.npz")))
        return {k[3:]: torch.tensor(v) for k, v in g.items() if k.startswith("in_")}
    pos, z = dense_cluster(n_atoms=73)
    i, j, s, _ = onl.neighbor_list(pos.numpy(), np.zeros((3, 3)), [False] * 3, opet.DEFAULT_HYPERS["cutoff"])
    inp = {"positions": pos, "cells": torch.zeros(1, 3, 3, dtype=torch.float64), "centers": torch.tensor(i).long(),
           "neighbors": torch.tensor(j).long(), "cell_shifts": torch.tensor(s).long(), "species": z,
           "system_indices": torch.zeros(len(z), dtype=torch.long)}
    check_cluster(inp)
    return inp


@functools.lru_cache(maxsize=None)
def case(tag, which):
    """(hypers, params, inp, nu, u, w) of one pair; shared, never modified."""
    hypers = dict(opet.DEFAULT_HYPERS, **CASES[tag])
    params = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    inp = dict(_input(which))
    n, s = inp["positions"].shape[0], inp["cells"].shape[0]
    if hypers["system_conditioning"]:
        inp["charge"], inp["spin_multiplicity"] = torch.tensor([-2, 3])[:s], torch.tensor([1, 4])[:s]
    gen = torch.Generator().manual_seed(11)
    nu = torch.rand(n, generator=gen) - 0.5
    u = torch.randn(n, 3, generator=gen)
    w = torch.rand(n, generator=gen) + 0.5
    return hypers, params, inp, nu, u, w


@memo_oracle
def oracle(params, hypers, inp, nu, u, w, dtype):
    """Everything the tests compare with, from one evaluation of the oracle in ``dtype`` (all returned in fp64). With
    ``E_i`` the per-atom energies and ``g = dE/dR`` of ``sum_i E_i``:

    atomic, grad (g), cell_grad; ``energy_grads``: d/dtheta ``sum_i w_i E_i``; ``force_grads``: d/dtheta
    ``[sum_i nu_i E_i + <u, g>]``; ``hvp``: ``d<u, g>/dR``; ``tangent``: ``<u, dE_i/dR>`` (d/d(weight_i) of ``<u, g>``)."""
    p = {k: (v if k == "species_to_species_index" else v.to(dtype).clone().requires_grad_(True)) for k, v in params.items()}
    keys = [k for k in p if k != "species_to_species_index"]
    leaves = [p[k] for k in keys]
    pos = inp["positions"].to(dtype).clone().requires_grad_(True)
    cells = inp["cells"].to(dtype).clone().requires_grad_(True)
    ones = torch.ones(pos.shape[0], dtype=dtype, requires_grad=True)
    kw = {k: inp[k] for k in ("charge", "spin_multiplicity") if k in inp}
    atomic = opet.pet_atomic_energies(p, hypers, pos, cells, inp["centers"], inp["neighbors"], inp["cell_shifts"],
                                      inp["species"], inp["system_indices"].long(), "energy", **kw)[:, 0]
    g, g_cell = torch.autograd.grad((ones * atomic).sum(), [pos, cells], create_graph=True)
    phi = (u.to(dtype) * g).sum()
    energy_grads = torch.autograd.grad((w.to(dtype) * atomic).sum(), leaves, retain_graph=True, allow_unused=True)
    hvp, tangent = torch.autograd.grad(phi, [pos, ones], retain_graph=True)
    force_grads = torch.autograd.grad((nu.to(dtype) * atomic).sum() + phi, leaves, allow_unused=True)

    def named(grads):
        return {k: (torch.zeros_like(p[k]) if gr is None else gr).detach().double() for k, gr in zip(keys, grads)}

    return {"atomic": atomic.detach().double(), "grad": g.detach().double(), "cell_grad": g_cell.detach().double(),
            "energy_grads": named(energy_grads), "force_grads": named(force_grads), "hvp": hvp.double(),
            "tangent": tangent.double()}


def relmax(got, ref):
    got, ref = got.detach().cpu().double(), ref.double()
    return float((got - ref).abs().max() / ref.abs().max())


def tensor_err(got, ref):
    """Per parameter tensor: relmax, or the absolute error where the reference carries no signal. Tied SiLU halves
    (the model holds ``[W; W]``) are summed: d/dW is the sum of the halves' gradients."""
    got, ref = got.detach().cpu().double(), ref.double()
    if got.shape != ref.shape:
        assert got.shape[0] == 2 * ref.shape[0], (got.shape, ref.shape)
        got = got[: ref.shape[0]] + got[ref.shape[0]:]
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    return err / scale if scale > 1e-12 else err


def bar(y):
    assert y <= Y_CAP, f"fp32 yardstick {y:.2e}: this input pins nothing"
    return max(FLOOR, 2.0 * y)


QUANTITIES = ("atomic", "grad", "cell_grad", "hvp", "tangent")
GRAD_SETS = ("energy_grads", "force_grads")


@functools.lru_cache(maxsize=None)
def reference(tag, which):
    """(fp64 reference, yardsticks) of a pair. ``ys[q]`` is a float for the quantities and a dict per parameter tensor for
    the two gradient sets; ``cell_grad`` only on input (a) (the cluster is not periodic: its cell gradient is zero)."""
    hypers, params, inp, nu, u, w = case(tag, which)
    ref = oracle(params, hypers, inp, nu, u, w, torch.float64)
    f32 = oracle(params, hypers, inp, nu, u, w, torch.float32)
    ys = {q: relmax(f32[q], ref[q]) for q in QUANTITIES if q != "cell_grad" or which == "a"}
    for q in GRAD_SETS:
        ys[q] = {k: tensor_err(f32[q][k], r) for k, r in ref[q].items()}
    return ref, ys


def worst(ys):
    return max(ys.values()) if isinstance(ys, dict) else ys
