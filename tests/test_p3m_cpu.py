"""P3M evaluation of the long-range operator, the parts that need no GPU: the fp64 oracle of the definition
(``tests/_p3m_oracle.py``) against the Ewald oracle it approximates and against the NaCl Madelung constant, the product's host
mesh shape and influence function against the oracle's, ``method=`` resolution with every refusal by name, and the premises
of the GPU cases (``tests/p3m_cases.py``)."""
import ctypes

import pytest
import torch

import _ewald_oracle as eo
import _p3m_oracle as po
import p3m_cases as pc
from metatrain_amd.long_range import P3M_CONVENTIONS  # the table the oracle restates
from oracle import pet as opet

MADELUNG = -1.7475646


def _cells():
    g = torch.Generator().manual_seed(2)
    cubic = torch.eye(3, dtype=torch.float64) * 9.5
    return {"cubic": cubic, "triclinic": cubic + 0.3 * torch.randn(3, 3, generator=g, dtype=torch.float64),
            "elongated": torch.tensor(pc.ANISOTROPIC, dtype=torch.float64), "sub_spacing": torch.eye(3, dtype=torch.float64) * 1.0}


def test_oracle_converges_to_the_ewald_oracle():
    """The 43-atom triclinic box of test_oracle_converges_in_the_kset, sigma = 1.4, p = 5, against the Ewald k-sum to |k| <= 8:
    the mesh k-space term differs by 1.19e-3 / 1.20e-5 / 2.08e-7 of the largest value on meshes 8^3 / 16^3 / 32^3 (measured;
    gains 99 and 58 per halving of the spacing). Asserted: one decade either side of those, and a gain of at least 16."""
    torch.manual_seed(0)
    cell = torch.eye(3, dtype=torch.float64) * 9.5 + 0.3 * torch.randn(3, 3, dtype=torch.float64)
    pos = torch.rand(43, 3, dtype=torch.float64) @ cell
    q = torch.randn(43, 5, dtype=torch.float64)
    ref = eo.kspace_self_background(pos, cell, q, 1.4, None, kmax=8.0)
    rel = {}
    for n in (8, 16, 32):
        v = po.kspace_self_background(pos, cell, q, 1.4, None, 5, shape=[n] * 3)
        rel[n] = float((v - ref).abs().max() / ref.abs().max())
    print(rel)
    measured = {8: 1.19e-3, 16: 1.20e-5, 32: 2.08e-7}
    for n, m in measured.items():
        assert m / 10.0 < rel[n] < m * 10.0, rel
    assert rel[8] / rel[16] >= 16.0 and rel[16] / rel[32] >= 16.0, rel


@pytest.mark.parametrize("smearing, measured", [(0.3, 3.7e-7), (0.5, 1.0e-8)])
def test_oracle_gives_the_nacl_madelung_constant(smearing, measured):
    """Real-space erfc term + mesh k-space + self + background on a 32^3 mesh (spacing 1/16 of the nearest distance):
    -1.7475646 within 3.7e-7 (sigma = 0.3) / 1.0e-8 (sigma = 0.5), the discretisation errors measured at this mesh (the coarser
    meshes 16^3 and 8^3 leave 2.7e-5 / 3.1e-7 and 3.3e-3 / 2.2e-5). Asserted: within one decade above the measured error."""
    assert po.mesh_shape(eo.nacl_system()[1], 0.0625) == [32, 32, 32]
    err = abs(po.madelung_nacl(smearing, 0.0625) - MADELUNG)
    print(smearing, err)
    assert err < 10.0 * measured + 1e-7  # (the constant is quoted to 1e-7)


@pytest.mark.parametrize("kind", ["cubic", "triclinic", "elongated", "sub_spacing"])
def test_product_mesh_shape_equals_the_oracle(kind):
    from metatrain_amd import long_range as lr

    cell = _cells()[kind]
    got = lr.mesh_shape(cell, 1.33)
    assert got == po.mesh_shape(cell, 1.33)
    assert got == {"cubic": [8, 8, 8], "triclinic": [8, 8, 8], "elongated": [8, 16, 4], "sub_spacing": [1, 1, 1]}[kind]
    with pytest.raises(lr.PetHipError, match="singular cell"):
        lr.mesh_shape(torch.zeros(3, 3), 1.33)


@pytest.mark.parametrize("kind", ["cubic", "triclinic"])
@pytest.mark.parametrize("nodes", [1, 2, 3, 4, 5])
def test_product_influence_function_equals_the_oracle(kind, nodes):
    from metatrain_amd import long_range as lr

    cell = _cells()[kind]
    got = lr.influence(cell, 1.4, 1.33, nodes)
    ref = po.influence(cell, po.mesh_shape(cell, 1.33), 1.4, nodes)
    assert got.shape == ref.shape == (8, 8, 5)
    assert float(got[0, 0, 0]) == 0.0 and float(ref[0, 0, 0]) == 0.0
    assert float(ref.max()) > 0.0
    assert bool(((got - ref).abs() <= 1e-12 * ref.abs()).all()), float(((got - ref).abs() / ref.abs().clamp_min(1e-300)).max())


def test_method_resolution_and_refusals():
    from metatrain_amd import long_range as lr

    default = dict(opet.DEFAULT_HYPERS)
    default["long_range"] = {"enable": True}  # the reference's defaults: use_ewald false, interpolation_nodes 5
    with pytest.raises(lr.PetHipError, match="p3m_as_ewald=True"):
        lr.LongRangeFeaturizerHip(default)  # None: unchanged
    with pytest.raises(lr.PetHipError, match="method='p3m'"):
        lr.LongRangeFeaturizerHip(default)
    f = lr.LongRangeFeaturizerHip(default, method="p3m")
    assert isinstance(f.ewald, lr.P3MHip) and f.ewald.interpolation_nodes == 5
    state = eo.featurizer_params(default["d_node"], 0)
    g = lr.LongRangeFeaturizerHip.from_state_dict(default, state, method="p3m")
    assert isinstance(g.ewald, lr.P3MHip) and all(torch.equal(g.state_dict()[k], state[k]) for k in state)
    e = lr.LongRangeFeaturizerHip(default, method="ewald")
    assert type(e.ewald) is lr.EwaldHip and type(lr.LongRangeFeaturizerHip(default, p3m_as_ewald=True).ewald) is lr.EwaldHip
    # method="p3m" evaluates with P3M whatever use_ewald says; None follows the hypers
    assert isinstance(lr.LongRangeFeaturizerHip(pc.lr_hypers(3, use_ewald=True), method="p3m").ewald, lr.P3MHip)
    assert type(lr.LongRangeFeaturizerHip(pc.lr_hypers(3, use_ewald=True)).ewald) is lr.EwaldHip
    assert lr.LongRangeFeaturizerHip(pc.lr_hypers(3), method="p3m").ewald.interpolation_nodes == 3
    for bad in (0, 6, 2.5):
        with pytest.raises(lr.PetHipError, match="interpolation_nodes must be an integer in 1..5"):
            lr.LongRangeFeaturizerHip(pc.lr_hypers(bad), method="p3m")
        with pytest.raises(lr.PetHipError, match="interpolation_nodes"):
            lr.P3MHip(interpolation_nodes=bad)
    lr.LongRangeFeaturizerHip(pc.lr_hypers(6), method="ewald")  # the Ewald sum does not read it
    with pytest.raises(lr.PetHipError, match="method must be one of None, 'ewald', 'p3m'"):
        lr.LongRangeFeaturizerHip(default, method="pme")
    with pytest.raises(lr.PetHipError, match="long_range.enable is false"):
        lr.LongRangeFeaturizerHip(dict(opet.DEFAULT_HYPERS), method="p3m")
    with pytest.raises(lr.PetHipError, match="num_neighbors_adaptive"):
        lr.LongRangeFeaturizerHip(dict(default, num_neighbors_adaptive=16.0), method="p3m")
    with pytest.raises(lr.PetHipError, match="mixed pbc"):
        lr.P3MHip().plan(torch.eye(3)[None] * 10.0, [[True, True, False]], [0, 4])
    with pytest.raises(lr.PetHipError, match="no CPU path"):
        lr.P3MHip().potential(None, torch.zeros(2, 3), torch.zeros(2, 4))
    with pytest.raises(lr.PetHipError, match="no CPU path"):
        lr.P3MHip().backward(None, torch.zeros(2, 3), torch.zeros(2, 4), torch.zeros(2, 4))
    assert lr.P3M_CONVENTIONS is P3M_CONVENTIONS
    assert set(P3M_CONVENTIONS) == {"mesh", "assignment", "nodes", "influence", "mesh_potential", "gather"}
    assert "{-2..2}^3" in P3M_CONVENTIONS["influence"] and po.ALIASES == (-2, -1, 0, 1, 2)


def test_entry_points_refuse_the_other_mode():
    """Host-side checks that come before any launch: interpolation_nodes outside 1..5, a P3M entry point on an Ewald-mode
    handle and the Ewald workspace query on a P3M-mode handle."""
    from metatrain_amd import _lib
    from metatrain_amd import long_range as lr

    lib = _lib.load()
    ew = lr.EwaldHip()
    assert lib.pet_p3m_filter(ew.handle, 4, None, None) == _lib.PET_ERR_ARGUMENT
    assert b"Ewald-mode handle" in lib.pet_last_error()
    assert lib.pet_p3m_spread(ew.handle, None, None, None, 4, None, None, 0, None) == _lib.PET_ERR_ARGUMENT
    assert lib.pet_p3m_workspace_bytes(ew.handle, 4) == -1 and lib.pet_p3m_mesh_elements(ew.handle, 4) == -1
    for bad in (0, 6, -1):
        assert lib.pet_ewald_set_p3m(ew.handle, bad) == _lib.PET_ERR_ARGUMENT
        assert b"interpolation_nodes must be 1..5" in lib.pet_last_error()
    p3m = lr.P3MHip()
    assert lib.pet_ewald_workspace_bytes(p3m.handle, 4) == -1 and lib.pet_ewald_num_kvectors(p3m.handle, 0) == -1
    assert lib.pet_ewald_potential(p3m.handle, None, None, None, 4, None, None, 0, None) == _lib.PET_ERR_ARGUMENT
    assert b"P3M-mode handle" in lib.pet_last_error()
    out = (ctypes.c_int32 * 3)()
    assert lib.pet_p3m_mesh_shape(p3m.handle, 0, out) == _lib.PET_ERR_ARGUMENT  # no plan yet


@pytest.mark.parametrize("name", pc.ALL_CASES)
def test_case_premises(name):
    """Every case is what it says: its mesh shapes, fp32-exact positions, and the property it is named for."""
    from metatrain_amd import long_range as lr

    c = pc.case(name)
    assert pc.meshes(name) == pc.EXPECTED_MESHES[name]
    for pos, cell, pbc in c.systems:
        assert torch.equal(pos, pos.float().double())
        if all(pbc):
            assert lr.mesh_shape(cell, pc.SPACING) == po.mesh_shape(cell, pc.SPACING)
    if name == "small_mesh":
        assert max(pc.meshes(name)[0]) == 4 < max(c.nodes) and len(c.systems[1][0]) == 1
    if name == "on_nodes":
        pos, cell, _ = c.systems[0]
        u = pos @ torch.linalg.inv(cell) * 8.0
        assert torch.equal(u, pos)  # mesh units are Angstrom here, exactly
        frac = u - torch.floor(u)
        assert bool((frac[0] == 0.0).all()) and bool((frac[1] == 0.5).all())  # on nodes; half-way
        assert float(u[2, 0]) == 0.0 and float(u[3, 0]) == 8.0  # both faces
        assert bool(((frac == 0.0) | (frac == 0.5)).all())
    if name == "anisotropic":
        (p0, c0, _), (p1, c1, _) = c.systems
        assert torch.equal(p0, p1) and float(torch.det(c0)) > 0.0 > float(torch.det(c1))
        assert float((c0 - torch.diag(c0.diagonal())).abs().max()) >= 1.0  # sheared
    if name == "unwrapped":
        pos, cell, _ = c.systems[0]
        s = pos @ torch.linalg.inv(cell)
        assert float(s.min()) < -2.0 and float(s.max()) > 3.0
    if name == "bins":
        pos, cell, _ = c.systems[0]
        assert len(pos) == 33
        for p in c.nodes:
            idx, _ = po.stencil(pos, cell, [16, 16, 16], p)
            assert len({tuple(r.tolist()) for r in idx[:, :, 0]}) == 1  # one stencil origin: one bin of 33 atoms
    if name == "mixed":
        sizes = [len(p) for p, _, _ in c.systems]
        assert sizes == [43, 0, 17, 1] and [all(pbc) for _, _, pbc in c.systems] == [True, True, False, True]
    if name == "supercell":
        (p0, c0, _), (p1, c1, _) = c.systems
        assert torch.equal(c1[0], 2.0 * c0[0]) and len(p1) == 2 * len(p0)
        m0, m1 = pc.meshes(name)
        assert m1 == [2 * m0[0], m0[1], m0[2]]  # commensurate: the same mesh spacing
    if name == "nodes":
        assert c.nodes == (1, 2, 3, 4, 5) and len(c.systems[0][0]) == 20
