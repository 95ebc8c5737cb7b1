"""GPU tests of the SOAP-BPNN Hessian-vector product (``soap_hessian_vector``, ``csrc/soap_hvp.hip``;
``SoapBpnnHip.hessian_vector_product``, ``soap_bpnn/hessian.py``) and of the stress term of its training step
(``soap_train_gradients_cell``, ``SoapTrainStep(target_strain_gradients=...)``) against torch's double backward through the
fp64 oracle ``oracle/soap.py``.

Bar of the product (the fp32-floor rule, as ``tests/test_gpu_hvp.py`` states it): ``relmax = max|got - ref| / max|ref| <=
max(1e-5, 2 y)`` with ``y`` the relmax of the SAME oracle evaluated by torch in fp32 on the same inputs, per quantity; an
input with ``y > 1e-3`` pins nothing and fails. Parameter gradients of the stress term: 1e-5 relmax per tensor and
``rtol = 2e-5`` on the losses, as ``tests/test_gpu_soap_train.py``. Measured ``(case, y, relmax)``: DESIGN §26."""
import os

import numpy as np
import pytest
import torch

from oracle import nl as onl
from oracle import pet as opet
from oracle import soap as osoap

from _memo import memo_oracle

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
BOX_TYPES, ETHANOL_TYPES = [1, 6, 7, 8], [1, 6, 8]
PC = 32  # pairs per LDS chunk of the per-atom kernels (csrc/soap.h)


def relmax(got, ref):
    ref = ref.double()
    return float((got.detach().cpu().double().reshape(ref.shape) - ref).abs().max() / ref.abs().max())


def bar(y):
    assert y <= 1e-3, f"fp32 yardstick {y:.2e}: this input pins nothing"
    return max(1e-5, 2.0 * y)


# ---- inputs -------------------------------------------------------------------------------------------------------
def _ethanol(n_frames=10):
    d = np.load(os.path.join(GOLD, "ethanol_first10.npz"))
    pos_l, z_l, i_l, j_l, sys_l, off = [], [], [], [], [], 0
    for k in range(n_frames):
        xyz = d["positions"][k]
        i, j, _, _ = onl.neighbor_list(xyz, np.zeros((3, 3)), [False] * 3, 5.0)
        pos_l.append(torch.tensor(xyz)); z_l.append(torch.tensor(d["species"][k]))
        i_l.append(torch.tensor(i) + off); j_l.append(torch.tensor(j) + off)
        sys_l.append(torch.full((len(xyz),), k, dtype=torch.long))
        off += len(xyz)
    ci = torch.cat(i_l)
    return (torch.cat(pos_l), torch.cat(z_l), torch.zeros((n_frames, 3, 3), dtype=torch.float64), ci, torch.cat(j_l),
            torch.zeros((len(ci), 3), dtype=torch.long), torch.cat(sys_l))


def _boxes(n_atoms=(60, 24), seed=3):
    """Two periodic boxes. (40, 24) has no atom above 30 pairs; 60 atoms at seed 3 reach 33, i.e. two PC chunks."""
    pos_l, z_l, cell_l, i_l, j_l, s_l, sys_l, off = [], [], [], [], [], [], [], 0
    for k, n in enumerate(n_atoms):
        pos, z, cell = opet.random_box(n, seed=seed + k, dtype=torch.float64)
        i, j, s, _ = onl.neighbor_list(pos.numpy(), cell.numpy(), [True] * 3, 5.0)
        pos_l.append(pos); z_l.append(z); cell_l.append(cell)
        i_l.append(torch.tensor(i) + off); j_l.append(torch.tensor(j) + off); s_l.append(torch.tensor(s).long())
        sys_l.append(torch.full((n,), k, dtype=torch.long))
        off += n
    batch = (torch.cat(pos_l), torch.cat(z_l), torch.stack(cell_l), torch.cat(i_l), torch.cat(j_l), torch.cat(s_l),
             torch.cat(sys_l))
    counts = torch.bincount(batch[3], minlength=off)
    assert int(counts.max()) > PC and int(counts.min()) < PC, (int(counts.min()), int(counts.max()))
    return batch


def _directions(batch, seed=1):
    gen = torch.Generator().manual_seed(seed)
    u = torch.randn(batch[0].shape[0], 3, generator=gen, dtype=torch.float64)
    u_cell = torch.randn(batch[2].shape[0], 3, 3, generator=gen, dtype=torch.float64) * 0.1
    return u, u_cell


HYPERS = {
    "legacy": {},
    "alchemical": {"legacy": False},
    "no_layernorm": {"bpnn": {"layernorm": False}},
    "one_hidden_layer": {"bpnn": {"num_hidden_layers": 1}},
    "four_hidden_layers": {"bpnn": {"num_hidden_layers": 4}},
    "48_neurons": {"bpnn": {"num_hidden_layers": 3, "num_neurons_per_layer": 48}},
    "mlp_head": {"heads": {"energy": "mlp"}},
    "alchemical_mlp_head": {"legacy": False, "heads": {"energy": "mlp"}},
    "small_basis": {"soap": {"max_angular": 2, "max_radial": 2}},
    "ethanol": {},
}


def _hypers(case):
    h = {k: (dict(v) if isinstance(v, dict) else v) for k, v in osoap.DEFAULT_HYPERS.items()}
    for key, val in HYPERS[case].items():
        if isinstance(val, dict) and key in h:
            h[key] = dict(h[key], **val)
        else:
            h[key] = val
    return h


def _case(case):
    hypers = _hypers(case)
    types = ETHANOL_TYPES if case == "ethanol" else BOX_TYPES
    batch = _ethanol() if case == "ethanol" else _boxes()
    params = osoap.synthetic_params(hypers, len(types), osoap.basis(hypers)[0], 1, torch.float32)
    return hypers, types, batch, params


# ---- oracle -------------------------------------------------------------------------------------------------------
@memo_oracle
def _oracle_hvp(params, hypers, types, batch, u, u_cell, dtype):
    """(H u [N,3], d/dcell [S,3,3], e'_i [N], <u, dE/dR> + <u_cell, dE/dcell>) of the oracle in ``dtype``: ``grad(E, [R, cells],
    create_graph)``, then ``grad(<g_R, u> + <g_cell, u_cell>, [R, cells, w])`` with ``E = sum_i w_i e_i`` at ``w = 1``."""
    pos, z, cells, ci, cj, cs, sysidx = batch
    p = {k: v.to(dtype) for k, v in params.items()}
    r = pos.to(dtype).clone().requires_grad_(True)
    c = cells.to(dtype).clone().requires_grad_(True)
    w = torch.ones(pos.shape[0], dtype=dtype, requires_grad=True)
    atomic = osoap.soap_bpnn_atomic_energies(p, hypers, types, r, c, ci, cj, cs, z, sysidx)
    g_pos, g_cell = torch.autograd.grad((w * atomic).sum(), [r, c], create_graph=True)
    phi = (g_pos * u.to(dtype)).sum() + (g_cell * u_cell.to(dtype)).sum()
    hp, hc, tan = torch.autograd.grad(phi, [r, c, w])
    return hp.double(), hc.double(), tan.double(), float(phi.detach())


def _reference(params, hypers, types, batch, u, u_cell):
    ref = _oracle_hvp(params, hypers, types, batch, u, u_cell, torch.float64)
    f32 = _oracle_hvp(params, hypers, types, batch, u, u_cell, torch.float32)
    return ref, [float((a - b).abs().max() / b.abs().max()) if float(b.abs().max()) > 0 else 0.0
                 for a, b in zip(f32[:3], ref[:3])]


def _model(dev, types, hypers, params, **kw):
    from metatrain_amd.soap_bpnn import SoapBpnnHip

    m = SoapBpnnHip(hypers, types, **kw)
    m.load({k: v.to(dev) for k, v in params.items()})
    return m


def _graph(m, dev, batch):
    pos, z, cells, ci, cj, cs, sysidx = batch[:7]
    return m.graph(pos.float().to(dev), cells.float().to(dev), ci.to(dev), cj.to(dev), cs.to(dev), z.to(dev),
                   sysidx.int().to(dev))


# ---- 1. H u against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(HYPERS))
def test_hvp_matches_the_oracle_double_backward(case):
    dev = torch.device("cuda:0")
    hypers, types, batch, params = _case(case)
    u, u_cell = _directions(batch)
    periodic = case != "ethanol"
    if not periodic:
        u_cell = torch.zeros_like(u_cell)  # open boundaries: no shift, the cell direction moves nothing
    ref, ys = _reference(params, hypers, types, batch, u, u_cell)
    m = _model(dev, types, hypers, params)
    g = _graph(m, dev, batch)
    hp, hc, tan = m.hessian_vector_product(g, u.to(dev), u_cell.to(dev), want_cells=True, want_tangent=True)
    errs = [relmax(hp, ref[0]), relmax(hc, ref[1]) if periodic else 0.0, relmax(tan, ref[2])]
    print(f"soap hvp {case}: (y, relmax) positions ({ys[0]:.2e}, {errs[0]:.2e}) cells ({ys[1]:.2e}, {errs[1]:.2e}) "
          f"tangent ({ys[2]:.2e}, {errs[2]:.2e})")
    for what, e, y in zip(("positions", "cells", "tangent"), errs, ys):
        assert e <= bar(y), (case, what, e, y)
    if not periodic:
        assert not bool(hc.any())
    # self-check: sum_i e'_i = <u, dE/dR> + <u_cell, dE/dcell>. Both sides are sums with cancellation of fp32 terms, each
    # term pinned to 1e-5 of the largest (the bar above; dE/dR likewise, tests/test_gpu_soap.py): the sums agree to 1e-5 of
    # the sum of the terms' magnitudes (the 1e-2: the right side's magnitudes overstate |u . g| per atom, as in
    # tests/test_gpu_soap_train.py)
    atomic = m.forward(g)
    gpos, gcell = m.backward(g, torch.ones_like(atomic), want_cell_grad=True)
    rhs = float((u.to(dev) * gpos.double()).sum() + (u_cell.to(dev) * gcell.double()).sum())
    size = float((u.to(dev).abs() * gpos.double().abs()).sum() + (u_cell.to(dev).abs() * gcell.double().abs()).sum())
    tol = 1e-5 * max(float(tan.double().abs().sum()), 1e-2 * size)
    assert abs(float(tan.double().sum()) - rhs) < tol
    assert abs(rhs - ref[3]) < tol
    # u_cell = None is a zero cell direction, bit for bit
    one = m.hessian_vector_product(g, u.to(dev), want_cells=True, want_tangent=True)
    same = m.hessian_vector_product(g, u.to(dev), torch.zeros_like(u_cell).to(dev), want_cells=True, want_tangent=True)
    for a, b in zip(one, same):
        assert torch.equal(a, b)


# ---- 2. dense Hessian of one ethanol molecule --------------------------------------------------------------------------
@memo_oracle
def _oracle_hessian(params, hypers, types, mol, dtype):
    pos, z, cells, ci, cj, cs, sysidx = mol
    p = {k: v.to(dtype) for k, v in params.items()}

    def energy(flat):
        return osoap.soap_bpnn_atomic_energies(p, hypers, types, flat.reshape(-1, 3), cells.to(dtype), ci, cj, cs, z,
                                               sysidx).sum()

    return torch.autograd.functional.hessian(energy, pos.to(dtype).reshape(-1), vectorize=True).double()  # (vmap: 1 s, not 9)


def _one_ethanol():
    return _ethanol(1)


def test_dense_hessian_of_one_ethanol_molecule():
    from metatrain_amd.soap_bpnn.hessian import hessian

    dev = torch.device("cuda:0")
    hypers, types = _hypers("legacy"), ETHANOL_TYPES
    params = osoap.synthetic_params(hypers, len(types), osoap.basis(hypers)[0], 1, torch.float32)
    mol = _one_ethanol()
    ref = _oracle_hessian(params, hypers, types, mol, torch.float64)
    y = float((_oracle_hessian(params, hypers, types, mol, torch.float32) - ref).abs().max() / ref.abs().max())
    m = _model(dev, types, hypers, params)
    system = (mol[0].float().to(dev), mol[1].to(dev), torch.zeros(3, 3, device=dev), [False] * 3)
    h = hessian(m, system, columns_per_launch=8).cpu().double()  # 27 rows: launches of 8, 8, 8 and 3 replicas
    assert h.shape == (27, 27)
    scale = float(h.abs().max())
    err, asym = relmax(h, ref), float((h - h.T).abs().max()) / scale
    shift = torch.eye(3, dtype=torch.float64).repeat(9, 1)  # [27, 3]: the three uniform translations
    trans = float((h @ shift).abs().max()) / scale
    print(f"soap dense Hessian: y {y:.2e}, relmax {err:.2e}, asymmetry {asym:.2e}, translations {trans:.2e}")
    assert err <= bar(y)
    assert asym <= bar(y)
    assert trans <= bar(y)
    # rows of a subset of the atoms: the same numbers
    part = hessian(m, system, atoms=[2, 7], columns_per_launch=4).cpu().double()
    assert torch.equal(part, torch.cat([h[6:9], h[21:24]]))


# ---- 3. structural edges ------------------------------------------------------------------------------------------------
def _with_isolated_atom():
    """One ethanol molecule and a one-atom system without any pair."""
    pos, z, cells, ci, cj, cs, sysidx = _ethanol(1)
    pos = torch.cat([pos, torch.tensor([[0.3, -0.2, 0.1]], dtype=torch.float64)])
    z = torch.cat([z, torch.tensor([8], dtype=z.dtype)])
    sysidx = torch.cat([sysidx, torch.tensor([1])])
    return pos, z, torch.zeros((2, 3, 3), dtype=torch.float64), ci, cj, cs, sysidx


def test_isolated_atom_beside_a_normal_system():
    dev = torch.device("cuda:0")
    hypers, types = _hypers("legacy"), ETHANOL_TYPES
    params = osoap.synthetic_params(hypers, len(types), osoap.basis(hypers)[0], 1, torch.float32)
    batch = _with_isolated_atom()
    u, u_cell = _directions(batch)
    ref, ys = _reference(params, hypers, types, batch, u, torch.zeros_like(u_cell))
    m = _model(dev, types, hypers, params)
    hp, hc, tan = m.hessian_vector_product(_graph(m, dev, batch), u.to(dev), want_cells=True, want_tangent=True)
    assert relmax(hp, ref[0]) <= bar(ys[0]) and relmax(tan, ref[2]) <= bar(ys[2])
    assert not bool(hp[-1].any()) and float(tan[-1]) == 0.0 and not bool(hc.any())


def test_no_pair_at_all_returns_zeros():
    dev = torch.device("cuda:0")
    hypers, types = _hypers("legacy"), ETHANOL_TYPES
    params = osoap.synthetic_params(hypers, len(types), osoap.basis(hypers)[0], 1, torch.float32)
    none = torch.zeros(0, dtype=torch.long)
    batch = (torch.tensor([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]], dtype=torch.float64), torch.tensor([1, 6]),
             torch.zeros((2, 3, 3), dtype=torch.float64), none, none, torch.zeros((0, 3), dtype=torch.long), torch.tensor([0, 1]))
    m = _model(dev, types, hypers, params)
    u = torch.ones(2, 3, device=dev)
    hp, hc, tan = m.hessian_vector_product(_graph(m, dev, batch), u, torch.ones(2, 3, 3, device=dev), want_cells=True,
                                           want_tangent=True)
    assert hp.shape == (2, 3) and hc.shape == (2, 3, 3) and tan.shape == (2,)
    assert not bool(hp.any()) and not bool(hc.any()) and not bool(tan.any())


def test_empty_system_index_batches_repeats_and_alone():
    """An empty system index in the middle of a batch; two calls give the same bits; a system alone gives the same bits as
    inside a batch."""
    dev = torch.device("cuda:0")
    hypers, types, batch, params = _case("legacy")
    pos, z, cells, ci, cj, cs, sysidx = batch
    u, u_cell = _directions(batch)
    m = _model(dev, types, hypers, params)
    g = _graph(m, dev, batch)
    first = m.hessian_vector_product(g, u.to(dev), u_cell.to(dev), want_cells=True, want_tangent=True)
    again = m.hessian_vector_product(g, u.to(dev), u_cell.to(dev), want_cells=True, want_tangent=True)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    # system index 1 left empty: the second box becomes system 2
    gap = (pos, z, torch.stack([cells[0], torch.eye(3, dtype=torch.float64), cells[1]]), ci, cj, cs, sysidx * 2)
    uc_gap = torch.stack([u_cell[0], torch.ones(3, 3, dtype=torch.float64), u_cell[1]])
    hp, hc, tan = m.hessian_vector_product(_graph(m, dev, gap), u.to(dev), uc_gap.to(dev), want_cells=True, want_tangent=True)
    assert torch.equal(hp, first[0]) and torch.equal(tan, first[2])
    assert torch.equal(hc[0], first[1][0]) and torch.equal(hc[2], first[1][1]) and not bool(hc[1].any())
    # the first box alone
    n0 = int((sysidx == 0).sum())
    e0 = int((ci < n0).sum())
    assert bool((ci[:e0] < n0).all()) and bool((ci[e0:] >= n0).all())
    alone = (pos[:n0], z[:n0], cells[:1], ci[:e0], cj[:e0], cs[:e0], sysidx[:n0])
    hp, hc, tan = m.hessian_vector_product(_graph(m, dev, alone), u[:n0].to(dev), u_cell[:1].to(dev), want_cells=True,
                                           want_tangent=True)
    assert torch.equal(hp, first[0][:n0]) and torch.equal(tan, first[2][:n0]) and torch.equal(hc[0], first[1][0])


def test_product_behind_a_packed_inference_forward():
    """The default forward of a legacy model stores the packed (upper-triangle) power spectrum; the product reads the full
    layout, rebuilt from the expansion coefficients as in training. Same numbers as behind a full-layout forward."""
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    hypers, types, batch, params = _case("legacy")
    u, u_cell = _directions(batch)
    ref, ys = _reference(params, hypers, types, batch, u, u_cell)
    m = _model(dev, types, hypers, params)
    g = _graph(m, dev, batch)
    m.forward(g)  # packed
    hp = m.hessian_vector_product(g, u.to(dev), u_cell.to(dev))
    assert relmax(hp, ref[0]) <= bar(ys[0])
    try:
        rt.config_set("soap_packed", 0)
        m.forward(g)  # full layout
        full = m.hessian_vector_product(g, u.to(dev), u_cell.to(dev))
    finally:
        rt.config_set("soap_packed", 1)
    assert relmax(full, ref[0]) <= bar(ys[0])
    assert relmax(hp, full.cpu()) <= 1e-6


# ---- 4. ZBL -----------------------------------------------------------------------------------------------------------
def test_zbl_total_and_dense_hessian_rule():
    from metatrain_amd._lib import PetHipError
    from metatrain_amd.soap_bpnn.hessian import hessian

    dev = torch.device("cuda:0")
    hypers, types, batch, params = _case("legacy")
    u, _ = _directions(batch)
    m = _model(dev, types, hypers, params, zbl=True)
    g = _graph(m, dev, batch)
    pbcs = [[True] * 3] * 2
    total = m.hessian_vector_product_total(g, u.to(dev), pbcs=pbcs)
    net = m.hessian_vector_product(g, u.to(dev))
    pair = m.zbl.hessian_vector_product(m.zbl.graph_for(g, pbcs), u.float().to(dev))
    assert bool(pair.any())
    assert torch.equal(total, net + pair)
    mol = _one_ethanol()
    me = _model(dev, ETHANOL_TYPES, hypers, osoap.synthetic_params(hypers, 3, osoap.basis(hypers)[0], 1, torch.float32), zbl=True)
    system = (mol[0].float().to(dev), mol[1].to(dev), torch.zeros(3, 3, device=dev), [False] * 3)
    with pytest.raises(PetHipError, match="zbl"):
        hessian(me, system)
    bare = hessian(me, system, zbl=False)
    with_pair = hessian(me, system, zbl=me.zbl)
    assert bare.shape == with_pair.shape == (27, 27) and not torch.equal(bare, with_pair)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    from ctypes import byref, c_void_p

    from metatrain_amd import _lib
    from metatrain_amd import runtime as rt
    from metatrain_amd._lib import PetHipError, check
    from metatrain_amd.soap_bpnn import SoapTrainStep, radial

    dev = torch.device("cuda:0")
    hypers, types, batch, params = _case("small_basis")
    m = _model(dev, types, hypers, params)
    g = _graph(m, dev, batch)
    n, s = g.n_nodes, g.n_systems
    # a model created through the C ABI without the curvature table
    lib = m.lib
    h = _lib.SoapHypers()
    h.cutoff, h.cutoff_width, h.max_angular = m.cutoff, m.width, hypers["soap"]["max_angular"]
    n_per_l, zeros, norms = radial.laplacian_eigenstates(m.cutoff, hypers["soap"]["max_radial"], hypers["soap"]["max_angular"])
    for l, k in enumerate(n_per_l):
        h.n_per_l[l] = k
    h.n_species = h.n_channels = len(types)
    h.legacy, h.layernorm, h.num_hidden_layers, h.num_neurons_per_layer = 1, 1, 2, 32
    handle = c_void_p()
    check(lib.soap_model_create(byref(h), byref(handle)))
    try:
        table = torch.from_numpy(radial.spline_table(m.cutoff, zeros, norms, 2049)).to(dev).contiguous()
        check(lib.soap_model_set_radial_table(handle, rt._ptr(table), 2049, rt._stream()))
        for key, t in params.items():
            src = t.to(dev).contiguous()
            check(lib.soap_model_set_param(handle, key.encode(), rt._ptr(src), src.numel(), rt._stream()))
            torch.cuda.synchronize()
        check(lib.soap_model_finalize(handle, rt._stream()))
        ws = torch.empty(int(lib.soap_workspace_bytes(handle, n, g.n_edges)), dtype=torch.uint8, device=dev)
        hws = torch.empty(int(lib.soap_hvp_workspace_bytes(handle, n, g.n_edges)), dtype=torch.uint8, device=dev)
        atomic = torch.empty(n, device=dev)
        check(lib.soap_forward(handle, g.handle, rt._ptr(ws), ws.numel(), rt._ptr(atomic), None, rt._stream()))
        uu, hp = torch.ones(n, 3, device=dev), torch.empty(n, 3, device=dev)
        with pytest.raises(PetHipError, match="soap_model_set_radial_curvature"):
            check(lib.soap_hessian_vector(handle, g.handle, rt._ptr(ws), ws.numel(), rt._ptr(hws), hws.numel(), rt._ptr(uu),
                                          None, rt._ptr(hp), None, None, rt._stream()))
        torch.cuda.synchronize()
    finally:
        lib.soap_model_destroy(handle)
    # u_cell on a graph without cell shifts
    bare = rt.HipGraph.from_batch(m._graph_model, g.export_batch())  # the NEF tensors alone: no shifts, no system indices
    with pytest.raises(PetHipError, match="d_u_cell.*cell shifts"):
        m.hessian_vector_product(bare, torch.ones(n, 3, device=dev), torch.ones(s, 3, 3, device=dev))
    u = _directions(batch)[0].float().to(dev)
    hp = m.hessian_vector_product(bare, u)  # without a cell direction such a graph serves
    assert relmax(hp, m.hessian_vector_product(g, u).cpu()) <= 1e-6
    # a strain target without positions / cells
    step = SoapTrainStep(m)
    with pytest.raises(ValueError, match="target_strain_gradients"):
        step(g, torch.zeros(s, device=dev), torch.ones(s, device=dev), target_strain_gradients=torch.zeros(s, 3, 3, device=dev))


# ---- 6. stress term of the training step ---------------------------------------------------------------------------------
def _targets(batch, seed=3):
    gen = torch.Generator().manual_seed(seed)
    n, s = batch[0].shape[0], batch[2].shape[0]
    return (torch.randn(s, generator=gen, dtype=torch.float64) * 3, torch.randn(n, 3, generator=gen, dtype=torch.float64) * 0.3,
            torch.randn(s, 3, 3, generator=gen, dtype=torch.float64) * 2)


def _oracle_step(p, hypers, types, batch, targets):
    """MSE(E / atom) + MSE(dE/dR) + MSE(dE/dstrain), the strain entering as in ``utils/evaluate_model.py:305-321``:
    ``positions @ strain``, ``cells @ strain``, gradient at the identity."""
    pos, z, cells, ci, cj, cs, sysidx = batch
    te, tg, ts = targets
    n_sys = cells.shape[0]
    r = pos.clone().requires_grad_(True)
    strain = torch.eye(3, dtype=torch.float64).repeat(n_sys, 1, 1).requires_grad_(True)
    r_s = (r[:, None, :] @ strain[sysidx]).squeeze(1)
    atomic = osoap.soap_bpnn_atomic_energies(p, hypers, types, r_s, cells @ strain, ci, cj, cs, z, sysidx)
    energies = torch.zeros(n_sys, dtype=torch.float64).index_add(0, sysidx, atomic)
    n_atoms = torch.bincount(sysidx, minlength=n_sys).double()
    g_r, g_s = torch.autograd.grad(energies.sum(), [r, strain], create_graph=True)
    return (((energies - te) / n_atoms) ** 2).mean() + ((g_r - tg) ** 2).mean() + ((g_s - ts) ** 2).mean()


@memo_oracle
def _oracle_strain_grads(params64, hypers, types, batch, targets):
    p = {k: v.clone().requires_grad_(True) for k, v in params64.items()}
    loss = _oracle_step(p, hypers, types, batch, targets)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in p.items()}


@pytest.mark.parametrize("case", ["legacy", "alchemical"])
def test_stress_term_parameter_gradients(case):
    from metatrain_amd.pet.trainer import energy_loss_and_seeds, force_loss_and_seeds, strain_loss_and_seeds

    dev = torch.device("cuda:0")
    hypers, types, batch, params = _case(case)
    targets = _targets(batch)
    loss_ref, g_ref = _oracle_strain_grads({k: v.double() for k, v in params.items()}, hypers, types, batch, targets)
    m = _model(dev, types, hypers, params)
    g = _graph(m, dev, batch)
    te, tg, ts = [t.float().to(dev) for t in targets]
    n_atoms = torch.bincount(batch[6], minlength=len(te)).float().to(dev)
    m.zero_grad()
    atomic = m.forward(g)
    loss, seeds = energy_loss_and_seeds(m.sum_over_atoms(g, atomic), te, n_atoms, g.system_of_atom())
    gpos, gcell = m.backward(g, torch.ones_like(atomic), want_cell_grad=True)
    loss_f, u = force_loss_and_seeds(gpos, tg)
    loss_s, u_s, u_cell = strain_loss_and_seeds(batch[0].float().to(dev), batch[2].float().to(dev), g.system_of_atom().long(),
                                                gpos, gcell, ts)
    tangent = m.train_gradients(g, seeds, u + u_s, u_cell)
    total = float(loss + loss_f + loss_s)
    assert abs(total - loss_ref) < 1e-5 * abs(loss_ref), (total, loss_ref)
    lhs = float(tangent.double().sum())
    rhs = float(((u + u_s).double() * gpos.double()).sum() + (u_cell.double() * gcell.double()).sum())
    size = float(((u + u_s).double().abs() * gpos.double().abs()).sum() + (u_cell.double().abs() * gcell.double().abs()).sum())
    assert abs(lhs - rhs) < 1e-5 * max(abs(rhs), 1e-2 * size)
    got = m.grads()
    assert set(got) == set(g_ref)
    worst = {key: relmax(got[key], ref) for key, ref in g_ref.items()}
    print(f"soap stress {case}: loss {total:.6e} (oracle {loss_ref:.6e}), worst parameter-gradient error {max(worst.values()):.2e}")
    bad = {k: v for k, v in worst.items() if not v < 1e-5}
    assert not bad, bad


def test_three_adam_steps_with_a_strain_target_follow_torch():
    from torch.optim.lr_scheduler import LambdaLR

    from metatrain_amd.pet.trainer import lr_lambda
    from metatrain_amd.soap_bpnn import SoapTrainStep

    dev = torch.device("cuda:0")
    hypers, types, batch, params = _case("legacy")
    targets = _targets(batch)
    p = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.Adam(list(p.values()), lr=1e-3)
    sched = LambdaLR(opt, lr_lambda=lambda k: lr_lambda(k, 5 * 2, 0.2))  # two warm-up steps: lr 0, 1/2, then the cosine
    ref_losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = _oracle_step(p, hypers, types, batch, targets)
        loss.backward()
        opt.step()
        sched.step()
        ref_losses.append(float(loss.detach()))
    m = _model(dev, types, hypers, params)
    g = _graph(m, dev, batch)
    step = SoapTrainStep(m, {"num_epochs": 5, "warmup_fraction": 0.2}, 2)
    te, tg, ts = [t.float().to(dev) for t in targets]
    n_atoms = torch.bincount(batch[6], minlength=len(te)).float().to(dev)
    pos, cells = batch[0].float().to(dev), batch[2].float().to(dev)
    losses = [float(step(g, te, n_atoms, tg, target_strain_gradients=ts, positions=pos, cells=cells)["loss"]) for _ in range(3)]
    print("soap strain steps:", losses, ref_losses)
    np.testing.assert_allclose(losses, ref_losses, rtol=2e-5)
    assert losses[1] == pytest.approx(losses[0], rel=1e-6) and losses[2] != losses[1]  # step 0 ran at lr 0, step 1 did not


# ---- 7. nothing existing moved -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["legacy", "alchemical"])
def test_zero_cell_seeds_leave_the_training_gradients(case):
    dev = torch.device("cuda:0")
    hypers, types, batch, params = _case(case)
    u, u_cell = _directions(batch)
    m = _model(dev, types, hypers, params)
    g = _graph(m, dev, batch)
    seeds = torch.linspace(-1.0, 1.0, g.n_nodes, device=dev)
    out = []
    for uc in (None, torch.zeros_like(u_cell).to(dev)):
        m.zero_grad()
        m.forward(g)
        tangent = m.train_gradients(g, seeds, u.float().to(dev), uc)
        out.append((tangent, m.grads()))
    assert relmax(out[1][0], out[0][0].cpu()) <= 1e-7
    for key, ref in out[0][1].items():
        assert relmax(out[1][1][key], ref.cpu()) <= 1e-7, key
