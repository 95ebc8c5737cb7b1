"""GPU tests of the ZBL Hessian-vector product (``pet_zbl_hessian_vector``, ``csrc/zbl.hip``;
``ZBLHip.hessian_vector_product``, ``pet/hessian.py::hessian(..., zbl=)``, the differentiable ZBL node of the exported
energy op) against the fp64 fixtures ``tests/golden/zbl_hvp_<case>.npz`` -- the reference's ``get_pairwise_zbl``
differentiated twice by torch (``make_golden_zbl_hvp.py``) -- and against the fp64 restatement ``tests/zbl_hvp_ref.py``.
Graphs are those of a default PET model (cutoff 4.5, as ``test_gpu_zbl.py::env`` builds them): most listed edges are
outside ``rc``.

Bar (the fp32-floor rule of ``tests/test_gpu_hvp.py``): ``relmax = max|got - ref| / max|ref| <= max(1e-5, 2 y)`` with ``y`` the
relmax of the SAME double backward evaluated by torch with fp32 geometry on the same inputs, computed here per quantity.
Measured ``(case, y, relmax)``: DESIGN.md section 12."""
import os

import numpy as np
import pytest
import torch

import zbl_hvp_ref as R
import zbl_ref
from oracle import pet as opet
from test_gpu_zbl import _cluster, env  # noqa: F401  (the fixture that builds graphs at cutoff 4.5)

from _memo import memo_oracle

pytestmark = pytest.mark.gpu
NAMES = ("positions", "cells", "tangent")
SMALL = dict(d_pet=32, d_node=32, d_feedforward=48, d_head=24, num_heads=2)  # as test_hvp_cpu.py


def _setup(env, name, which=None):
    f = R.fixture(name)
    z = env.zbl(env.fixture(name))
    g = env.graph(env.graph_model(z.atomic_types), env.systems(env.fixture(name), which))
    return f, z, g


def _direction(env, f):
    return f["u"].float().to(env.dev), f["u_cell"].float().to(env.dev), f["lambda"].float().to(env.dev)


def _same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", R.CASES)
def test_hvp_matches_the_reference_fixture(env, name):
    """1. hvp_positions, hvp_cells and tangent_atomic for a cell direction and non-uniform weights, all five fixtures."""
    f, z, g = _setup(env, name)
    u, uc, lam = _direction(env, f)
    ref = (f["hvp_positions"], f["hvp_cells"], f["tangent_atomic"])
    ys = [R.relmax(a, b) for a, b in zip(R.of_fixture(name, dtype=torch.float32), ref)]
    got = z.hessian_vector_product(g, u, uc, lam, want_cells=True, want_tangent=True)
    errs = [R.relmax(a, b) for a, b in zip(got, ref)]
    print(f"zbl hvp {name}: (y, relmax) " + " ".join(f"{w} ({y:.2e}, {e:.2e})" for w, y, e in zip(NAMES, ys, errs)))
    for what, e, y in zip(NAMES, errs, ys):
        assert e <= R.bar(y), (name, what, e, y)
    if name == "one_atom":  # six self-image edges: no position enters, the cell block is all there is
        assert torch.equal(got[0], torch.zeros_like(got[0])) and float(got[1].abs().max()) > 0.1
    if name == "qm9_compressed":  # five molecules, no cell
        assert torch.equal(got[1], torch.zeros_like(got[1]))


def test_null_arguments_and_optional_outputs(env):
    """2. Weights NULL = ones, u_cell NULL = zeros, and every optional output left out: the same bits in what remains."""
    f, z, g = _setup(env, "box_a_sheared")
    u, uc, lam = _direction(env, f)
    full = z.hessian_vector_product(g, u, uc, lam, True, True)
    assert _same_bits(z.hessian_vector_product(g, u, uc, None, True, True),
                      z.hessian_vector_product(g, u, uc, torch.ones_like(lam), True, True))
    assert _same_bits(z.hessian_vector_product(g, u, None, lam, True, True),
                      z.hessian_vector_product(g, u, torch.zeros_like(uc), lam, True, True))
    assert _same_bits([z.hessian_vector_product(g, u, uc, lam)], full[:1])
    assert _same_bits(z.hessian_vector_product(g, u, uc, lam, want_cells=True), full[:2])
    assert _same_bits(z.hessian_vector_product(g, u, uc, lam, want_tangent=True), (full[0], full[2]))


@pytest.mark.parametrize("n_atoms", [142, 37])
def test_rows_of_every_length(env, n_atoms):
    """3. The cluster of ``test_gpu_zbl.py``: 141 atoms inside one ZBL range of the central one (a row of 140 hits, more
    than two 64-slot queue flushes inside one row) plus an atom with no edge, and its first 36 atoms plus that atom (no
    row fills the queue: only the final flush runs); 142 and 37 atoms, neither a multiple of the 16 atoms of a wave."""
    from metatrain_amd.zbl import ZBLHip

    radii = {1: 2.0, 6: 2.1}  # ZBL cutoff 4.2 inside the model's 4.5
    pos = torch.cat([_cluster(n_atoms - 1, 4.1, 0.9, seed=2), torch.tensor([[50.0, 50.0, 50.0]], dtype=torch.float64)])
    numbers = torch.tensor([1, 6])[torch.randint(0, 2, (142,), generator=torch.Generator().manual_seed(4))][:n_atoms]
    z = ZBLHip([1, 6], covalent_radii=radii)
    g = env.graph(env.graph_model([1, 6]), [(pos.float().to(env.dev), numbers.to(env.dev), torch.zeros(3, 3), (False,) * 3)])
    rows = g.csr()["rowptr"].cpu()
    assert int(rows[1] - rows[0]) == n_atoms - 2 and int(rows[n_atoms] - rows[n_atoms - 1]) == 0
    radii_of = torch.zeros(7, dtype=torch.float64)
    radii_of[1], radii_of[6] = 2.0, 2.1
    pairs = zbl_ref.brute_force_pairs(pos, torch.zeros(3, 3, dtype=torch.float64), 4.5, periodic=False)
    r = (pos[pairs[:, 1]] - pos[pairs[:, 0]]).norm(dim=1)
    inside_row0 = int(((pairs[:, 0] == 0) & (r <= radii_of[numbers[0]] + radii_of[numbers[pairs[:, 1]]])).sum())
    assert inside_row0 > (130 if n_atoms == 142 else 18), inside_row0
    gen = torch.Generator().manual_seed(1)
    u = torch.randn(n_atoms, 3, generator=gen, dtype=torch.float64)
    lam = 0.5 + torch.rand(n_atoms, generator=gen, dtype=torch.float64)
    args = (pos, torch.zeros(1, 3, 3, dtype=torch.float64), torch.zeros(n_atoms, dtype=torch.long), numbers, radii_of, pairs,
            u, torch.zeros(1, 3, 3, dtype=torch.float64), lam)
    ref = R.double_backward(*args)
    ys = [R.relmax(a, b) for a, b in zip(R.double_backward(*args, dtype=torch.float32), ref)]
    hp, hc, tan = z.hessian_vector_product(g, u.float().to(env.dev), None, lam.float().to(env.dev), True, True)
    errs = [R.relmax(hp, ref[0]), R.relmax(tan, ref[2])]
    print(f"zbl hvp cluster of {n_atoms}: (y, relmax) positions ({ys[0]:.2e}, {errs[0]:.2e}) tangent ({ys[2]:.2e}, {errs[1]:.2e})")
    assert errs[0] <= R.bar(ys[0]) and errs[1] <= R.bar(ys[2]), (errs, ys)
    assert torch.equal(hp[-1], torch.zeros(3, device=env.dev)) and float(tan[-1]) == 0.0  # the atom with no edge
    assert torch.equal(hc, torch.zeros_like(hc))  # no periodic image: no cell term
    if n_atoms == 37:  # no edge at all: zeros, nothing launched on an empty array
        far = torch.tensor([[0.0, 0.0, 0.0], [20.0, 0.0, 0.0]])
        g0 = env.graph(env.graph_model([1, 6]), [(far.to(env.dev), torch.tensor([1, 6]).to(env.dev), torch.zeros(3, 3), (False,) * 3)])
        assert g0.n_edges == 0
        outs = z.hessian_vector_product(g0, torch.ones(2, 3, device=env.dev), torch.ones(1, 3, 3, device=env.dev), None, True, True)
        assert [tuple(o.shape) for o in outs] == [(2, 3), (1, 3, 3), (2,)]
        assert all(torch.equal(o, torch.zeros_like(o)) for o in outs)


def test_outputs_repeat_and_are_linear_bitwise(env):
    """4a. No atomics, fixed summation orders: two calls give the same bits; every operation on the direction is a product
    with or a sum of terms that scale with it, so ``H (2 u) = 2 H u`` bit for bit, and ``H 0`` is exactly zero."""
    f, z, g = _setup(env, "box_a_sheared")
    u, uc, lam = _direction(env, f)
    first = z.hessian_vector_product(g, u, uc, lam, True, True)
    assert _same_bits(first, z.hessian_vector_product(g, u, uc, lam, True, True))
    twice = z.hessian_vector_product(g, 2 * u, 2 * uc, lam, True, True)
    assert all(torch.equal(a, 2 * b) for a, b in zip(twice, first))
    zero = z.hessian_vector_product(g, torch.zeros_like(u), torch.zeros_like(uc), lam, True, True)
    assert all(torch.equal(a, torch.zeros_like(a)) for a in zero)


def test_a_system_gives_the_same_bits_alone_and_in_a_batch(env):
    """4b. A periodic system and one with a zero cell in one batch: every output equals, bit for bit, the system alone."""
    f, z, _ = _setup(env, "box_b")
    model = env.graph_model(z.atomic_types)
    periodic = env.systems(env.fixture("box_b"))[0]
    molecule = (periodic[0][:9].clone(), periodic[1][:9].clone(), torch.zeros(3, 3), (False,) * 3)
    gen = torch.Generator().manual_seed(8)
    u = torch.randn(33, 3, generator=gen).to(env.dev)
    uc = (0.1 * torch.randn(2, 3, 3, generator=gen)).to(env.dev)
    lam = (0.5 + torch.rand(33, generator=gen)).to(env.dev)
    for systems, slots in (([periodic, molecule], [(0, 24), (24, 33)]), ([molecule, periodic], [(24, 33), (0, 24)])):
        order = torch.cat([torch.arange(lo, hi) for lo, hi in slots]).to(env.dev)
        which = [0 if lo == 0 else 1 for lo, _ in slots]
        hp, hc, tan = z.hessian_vector_product(env.graph(model, systems), u[order], uc[which], lam[order], True, True)
        first = 0
        for s, (lo, hi) in enumerate(slots):
            one = z.hessian_vector_product(env.graph(model, [systems[s]]), u[lo:hi], uc[which[s]][None], lam[lo:hi], True, True)
            n = hi - lo
            assert _same_bits((hp[first:first + n], hc[s], tan[first:first + n]), (one[0], one[1][0], one[2]))
            first += n
    assert float(hc.abs().max()) > 0.1


def test_a_rigid_translation_gives_exact_zeros(env):
    """5. One direction for all atoms of a system and no cell direction: every ``D'`` is exactly zero, and so is the result."""
    rigid = torch.tensor([[0.3, -1.2, 0.7], [-2.0, 0.1, 0.4], [1.1, 1.3, -0.2], [0.0, 2.5, 0.0], [-0.7, 0.0, 0.9]])
    for name in ("qm9_compressed", "box_a_sheared"):  # five molecules with a direction each; a periodic box
        f, z, g = _setup(env, name)
        u = rigid[f["system_indices"].long()].to(env.dev)
        out = z.hessian_vector_product(g, u, None, f["lambda"].float().to(env.dev), True, True)
        assert float(z.hessian_vector_product(g, _direction(env, f)[0]).abs().max()) > 1.0  # (the inputs do pin something)
        assert all(torch.equal(o, torch.zeros_like(o)) for o in out), name


def test_the_product_is_symmetric(env):
    """6. ``w^T H u`` against ``u^T H w`` over (positions, cells) on the sheared box (a general cell, non-uniform weights, the
    heaviest elements), accumulated in fp64 from the fp32 outputs. The quantity is the bilinear form; ``y`` is its relative
    error when torch evaluates it with fp32 geometry (``w^T (H u)`` of that arm against fp64), and the two evaluations
    here may differ by at most ``2 y`` of the larger. Also printed: the difference of the fp32 arm's own two evaluations,
    which is rounding noise of the same kind as the kernel's (CPU, 6e-9 for this input; fp32 outputs alone allow 6e-8 of
    ``sum |w_k| |(H u)_k|``) and therefore no bound."""
    name = "box_a_sheared"
    f, z, g = _setup(env, name)
    n, s = f["positions"].shape[0], f["cells"].shape[0]
    gen = torch.Generator().manual_seed(7)
    w = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    wc = 0.1 * torch.randn(s, 3, 3, generator=gen, dtype=torch.float64)
    u, uc, lam = f["u"], f["u_cell"], f["lambda"]

    def form(hvp_of):
        hu, hw = hvp_of(u, uc), hvp_of(w, wc)
        return (float((w * hu[0].cpu().double()).sum() + (wc * hu[1].cpu().double()).sum()),
                float((u * hw[0].cpu().double()).sum() + (uc * hw[1].cpu().double()).sum()))

    ref = form(lambda a, b: R.of_fixture(name, a, b))
    arm = form(lambda a, b: R.of_fixture(name, a, b, dtype=torch.float32))
    got = form(lambda a, b: z.hessian_vector_product(g, a.float().to(env.dev), b.float().to(env.dev),
                                                     lam.float().to(env.dev), want_cells=True))
    y = abs(arm[0] - ref[0]) / abs(ref[0])
    asym = abs(got[0] - got[1]) / max(abs(got[0]), abs(got[1]))
    print(f"zbl hvp symmetry: w^T H u {got[0]:.9g} against u^T H w {got[1]:.9g} (fp64 {ref[0]:.9g}): difference {asym:.2e}, "
          f"y {y:.2e}; fp32 arm's own difference {abs(arm[0] - arm[1]) / max(abs(arm[0]), abs(arm[1])):.2e}")
    assert 0 < y <= 1e-3
    assert asym <= 2 * y, (got, y)


def test_refusals(env):
    """7. A graph below the ZBL cutoff, a graph built under an adaptive cutoff and a ``from_batch`` handle each raise."""
    f, z, g = _setup(env, "box_a")
    u, uc, lam = _direction(env, f)
    systems = env.systems(env.fixture("box_a"))
    short = env.graph(env.graph_model(z.atomic_types, cutoff=2.0, cutoff_width=0.4), systems)
    adaptive = env.graph(env.graph_model(z.atomic_types, num_neighbors_adaptive=8.0), systems)
    for bad, message in ((short, "below the ZBL cutoff"), (adaptive, "adaptive")):
        with pytest.raises(env.rt.PetHipError, match=message):
            z.hessian_vector_product(bad, u, uc, lam, True, True)
    handle = env.rt.HipGraph.from_batch(g.model, g.export_batch())
    with pytest.raises(env.rt.PetHipError):
        z.hessian_vector_product(handle, u)
    own = z.graph_for(short, pbcs=[[True, True, True]])  # the graph ZBLHip builds for itself at its own cutoff serves
    got = z.hessian_vector_product(own, u, uc, lam, True, True)
    for a, what in zip(got, ("hvp_positions", "hvp_cells", "tangent_atomic")):
        assert R.relmax(a, f[what]) <= 1e-5, what


# ---- composition and the exported model ------------------------------------------------------------------------------
def _methane(golden_dir):
    q = dict(np.load(os.path.join(golden_dir, "qm9_first5.npz")))
    return torch.tensor(q["pos0"]) * 0.8, torch.tensor(q["z0"]).long()


def _dense_zbl(pos, numbers, radii_of, cutoff, dtype):
    pairs = zbl_ref.brute_force_pairs(pos, torch.zeros(3, 3, dtype=torch.float64), cutoff, periodic=False)
    n = pos.shape[0]

    def energy(flat):
        return R.atomic_energies(flat.reshape(n, 3), torch.zeros(1, 3, 3, dtype=dtype), torch.zeros(n, dtype=torch.long),
                                 numbers, radii_of, pairs).sum()

    return torch.autograd.functional.hessian(energy, pos.to(dtype).reshape(-1)).double()


def test_dense_hessian_of_a_zbl_model(env, golden_dir):
    """8. ``hessian(model, system, zbl=table)`` of a small ``zbl: true`` model on the first QM9 molecule compressed to 0.8 =
    the network's own block (``zbl=False``) + the dense ZBL block of the fp64 restatement, within the bar; symmetric to
    twice the network-only block's own ``max|H - H^T| / max|H|``; one and four columns per launch agree; without ``zbl=``
    the call raises; with a neighbour list shorter than the ZBL range the term runs on a graph of its own."""
    from metatrain_amd.pet.hessian import hessian
    from metatrain_amd.zbl import DEFAULT_COVALENT_RADII, ZBLHip

    types = [1, 6, 7, 8]
    hypers = dict(opet.DEFAULT_HYPERS, **SMALL)
    params = opet.synthetic_params(hypers, types, {"energy": 1}, 0, torch.float32)
    model = env.rt.HipModel(dict(hypers, zbl=True), types)
    model.load({k: v.to(env.dev) for k, v in params.items()}, "energy")
    pos, numbers = _methane(golden_dir)
    n = len(numbers)
    system = (pos.float().to(env.dev), numbers.to(env.dev), torch.zeros(3, 3), [False] * 3)
    table = ZBLHip(types)
    with pytest.raises(env.rt.PetHipError, match="zbl="):
        hessian(model, system)
    net = hessian(model, system, zbl=False, columns_per_launch=4).cpu().double()
    h4 = hessian(model, system, zbl=table, columns_per_launch=4).cpu().double()
    h1 = hessian(model, system, zbl=table, columns_per_launch=1).cpu().double()
    assert torch.equal(hessian(model, system, zbl=True, columns_per_launch=4).cpu().double(), h4)  # the default radii
    radii_of = torch.zeros(9, dtype=torch.float64)
    for t in types:
        radii_of[t] = DEFAULT_COVALENT_RADII[t]
    ref = _dense_zbl(pos.float().double(), numbers, radii_of, table.cutoff, torch.float64)
    y = R.relmax(_dense_zbl(pos.float().double(), numbers, radii_of, table.cutoff, torch.float32), ref)
    assert float(ref.abs().max()) > 1.0 and float(net.abs().max()) > 0  # pairs inside rc: the term is there to be added
    e4, e1 = R.relmax(h4, net + ref), R.relmax(h1, net + ref)
    scale = float(h4.abs().max())
    asym_net = float((net - net.T).abs().max() / net.abs().max())
    asym = float((h4 - h4.T).abs().max()) / scale
    print(f"dense Hessian with ZBL: y {y:.2e}, relmax K=4 {e4:.2e}, K=1 {e1:.2e}, asymmetry {asym:.2e} (network alone {asym_net:.2e})")
    assert h4.shape == (3 * n, 3 * n) and e4 <= R.bar(y) and e1 <= R.bar(y)
    assert float((h1 - h4).abs().max()) <= R.bar(y) * scale
    assert asym <= 2 * asym_net
    # a list shorter than the ZBL range (1.2 A against 1.52 A): the term runs on a graph of its own at the ZBL cutoff
    short_net = hessian(model, system, cutoff=1.2, zbl=False, columns_per_launch=4).cpu().double()
    short = hessian(model, system, cutoff=1.2, zbl=table, columns_per_launch=4).cpu().double()
    assert table.cutoff > 1.2 and R.relmax(short, short_net + ref, "dense Hessian, short list") <= R.bar(y)


@memo_oracle
def _oracle_pet_hvp(params, hypers, inp, u, u_cell, weights, dtype):
    p = {k: (v if k == "species_to_species_index" else v.to(dtype)) for k, v in params.items()}
    pos = inp["positions"].to(dtype).clone().requires_grad_(True)
    cells = inp["cells"].to(dtype).clone().requires_grad_(True)
    w = weights.to(dtype).clone().requires_grad_(True)
    atomic = opet.pet_atomic_energies(p, hypers, pos, cells, inp["centers"], inp["neighbors"], inp["cell_shifts"],
                                      inp["species"], inp["system_indices"].long(), "energy")[:, 0]
    g_pos, g_cell = torch.autograd.grad((w * atomic).sum(), [pos, cells], create_graph=True)
    hp, hc, tan = torch.autograd.grad((g_pos * u.to(dtype)).sum() + (g_cell * u_cell.to(dtype)).sum(), [pos, cells, w])
    return hp.double(), hc.double(), tan.double()


def test_exported_model_with_zbl_differentiates_twice(env, tmp_path):
    """9. ``ExportedEnergyModel(core, scale = 1.7, composition, zbl = table)`` on box B, eager and scripted, saved and
    re-loaded: ``grad(<dE/dR, u> + <dE/dcell, u_cell>, [positions, cells, weights])`` of ``1.7 PET + ZBL`` per atom equals
    ``1.7 x`` the network's product ``+`` the ZBL product of the direct calls (the scaler multiplies the network column
    only) to 1e-6 of the largest entry -- fp32 rounding of the two sums torch forms; the measured difference is printed --
    and the fp64 oracle (``oracle.pet`` + ``zbl_hvp_ref``) within the bar. ``torch.autograd.functional.hvp`` works on it."""
    from metatrain_amd import data
    from metatrain_amd.pet import script

    f = R.fixture("box_b")
    raw = env.fixture("box_b")
    z = env.zbl(raw)
    types = z.atomic_types
    hypers = dict(opet.DEFAULT_HYPERS, **SMALL)
    params = opet.synthetic_params(hypers, types, {"energy": 1}, 0, torch.float32)
    parts = script.make_core_and_zbl(dict(hypers, zbl=True), types, params, "energy", zbl=z)
    comp = torch.zeros(30)
    comp[types] = torch.tensor([-0.5, -37.8, -75.1])
    eager = script.ExportedEnergyModel(parts.core, 1.7, comp, zbl=parts.zbl)
    path = str(tmp_path / "energy_zbl.pt")
    torch.jit.save(torch.jit.script(eager), path)
    loaded = torch.jit.load(path)
    b = data.collate(env.systems(raw), hypers["cutoff"])
    model = env.rt.HipModel(hypers, types)
    model.load({k: v.to(env.dev) for k, v in params.items()}, "energy")
    graph = data.graph_of(model, b)
    u, uc, lam = _direction(env, f)
    net = env.rt.hessian_vector_product(model, graph, u, uc, lam, True, True)
    rep = z.hessian_vector_product(graph, u, uc, lam, True, True)
    want = [1.7 * a + c for a, c in zip(net, rep)]
    idx = [b[k] for k in ("centers", "neighbors", "cell_shifts", "species", "system_indices")]

    def per_atom(mod, pos, cells):
        out = mod.pet(pos, cells, *idx)
        assert out.shape[1] == 2
        return 1.7 * out[:, 0] + out[:, 1]

    got = None
    for mod in (loaded, eager):
        pos = b["positions"].clone().requires_grad_(True)
        cells = b["cells"].clone().requires_grad_(True)
        w = lam.clone().requires_grad_(True)
        g_pos, g_cell = torch.autograd.grad((w * per_atom(mod, pos, cells)).sum(), [pos, cells], create_graph=True)
        got = torch.autograd.grad((g_pos * u).sum() + (g_cell * uc).sum(), [pos, cells, w])
        diffs = [float((a - c).abs().max() / c.abs().max()) for a, c in zip(got, want)]
        print("exported model against the direct calls: " + " ".join(f"{n} {d:.2e}" for n, d in zip(NAMES, diffs)))
        assert max(diffs) <= 1e-6, diffs
    pos0, cells0 = b["positions"], b["cells"]
    _, hv = torch.autograd.functional.hvp(lambda p: per_atom(loaded, p, cells0).sum(), pos0, u)
    ones = 1.7 * env.rt.hessian_vector_product(model, graph, u) + z.hessian_vector_product(graph, u)
    assert float((hv - ones).abs().max()) <= 1e-6 * float(ones.abs().max())
    # the fp64 oracle of both terms on the same inputs
    inp = {k: (v.cpu() if v.is_floating_point() else v.cpu().long()) for k, v in b.items()}
    zargs = (inp["positions"].double(), inp["cells"].double(), f["system_indices"].long(), f["numbers"].long(),
             f["radii_table"], f["pairs"], f["u"].float(), f["u_cell"].float(), f["lambda"].float())
    both = []
    for dtype in (torch.float64, torch.float32):
        o = _oracle_pet_hvp(params, hypers, inp, f["u"].float(), f["u_cell"].float(), f["lambda"].float(), dtype)
        both.append([1.7 * a + c for a, c in zip(o, R.double_backward(*zargs, dtype=dtype))])
    ys = [R.relmax(a, c) for a, c in zip(both[1], both[0])]
    errs = [R.relmax(a, c) for a, c in zip(got, both[0])]
    print("exported model against the fp64 oracle: (y, relmax) " + " ".join(f"{n} ({y:.2e}, {e:.2e})" for n, y, e in zip(NAMES, ys, errs)))
    for what, e, y in zip(NAMES, errs, ys):
        assert e <= R.bar(y), (what, e, y)
