"""The attention kernels at the per-atom token counts they switch by (the cases of ``attn_token_cases.py``; the dispatch table is
in DESIGN.md): per-atom energies and dE/dR of every first-order route against the fp64 oracle ``oracle/pet.py``, which kernels
ran, the fused block's 64 | 65 refusal, the general kernels behind ``trr = 0``, and the training passes at the second-order
pass's limit (T_max = 121: the first size whose ``k_attn_rev`` needs the large-LDS opt-in; 128: the largest served; 129: the
size-generic pass).

First-order bar, per cluster (an m-atom cluster is m atoms of exactly m tokens): ``max |got - ref|`` over the cluster's rows
divided by ``max |ref|`` over those rows (the batch-wide scale where the cluster's own is below 1e-9 of it: the one-atom
cluster, whose dE/dR is exactly zero) must stay below ``max(1e-5, 3 y)``, y the same figure of the oracle evaluated by torch in
fp32 on the same inputs -- the rule of ``test_fused_block_operand_ranges``. Every ``(case, cluster size, quantity, y, device
error)`` is printed before it is asserted; the figures of one run are in DESIGN.md.

The switches a test needs are set here and restored in ``try / finally``."""
import functools

import numpy as np
import pytest
import torch

import attn_token_cases as ac
from _memo import memo_oracle
from oracle import pet as opet
from test_gpu_gen_train import _compare, _oracle_param_grads, _oracle_second_order
from test_gpu_hvp import _reference as _hvp_reference
from test_gpu_hvp import bar as hvp_bar
from test_gpu_hvp import relmax as hvp_relmax

pytestmark = pytest.mark.gpu
TOL = 1e-5
TYPES = ac.TYPES
DEFAULT = {"emlp_s": 1, "attn_fused": 3, "trr": 1}
FORCED = {"emlp_s": 2, "attn_fused": 7}
GENERAL = {"trr": 0}
THREE_KERNEL = {"qkv", "attn_fwd", "attn_bwd"}
FUSED = {"attn_blk", "attn_blk_bwd"}
ORDERS = pytest.mark.parametrize("shuffled", [False, True], ids=["ordered", "shuffled"])


def _hypers():
    return dict(opet.DEFAULT_HYPERS)


def _params():
    return opet.synthetic_params(_hypers(), TYPES, {"energy": 1}, 0, torch.float32)


def _seed_vector(n):
    return torch.rand(n, generator=torch.Generator().manual_seed(7)) + 0.5


@memo_oracle
def _oracle_first_order(params, hypers, inp, w, dtype):
    """(per-atom energies, d(sum_i w_i e_i)/dR) of the oracle in ``dtype``, as fp64 arrays"""
    p = {k: (v if k == "species_to_species_index" else v.to(dtype)) for k, v in params.items()}
    pos = inp["positions"].to(dtype).clone().requires_grad_(True)
    a = opet.pet_atomic_energies(p, hypers, pos, inp["cells"].to(dtype), inp["centers"], inp["neighbors"], inp["cell_shifts"],
                                 inp["species"], inp["system_indices"], "energy")[:, 0]
    (g,) = torch.autograd.grad((a * w.to(dtype)).sum(), pos)
    return a.detach().double().numpy(), g.double().numpy()


def _reference(case):
    """fp64 reference and fp32 yardstick of a case: the shuffled list describes the same system, so both orders share them"""
    inp = ac.inputs(case)
    w = _seed_vector(len(inp["species"]))
    return (_oracle_first_order(_params(), _hypers(), inp, w, torch.float64),
            _oracle_first_order(_params(), _hypers(), inp, w, torch.float32))


def cluster_errors(got, ref, cluster):
    """{cluster index: max |got - ref| / max |ref| over the cluster's rows}; batch-wide scale under a vanishing own scale"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    batch = np.abs(ref).max()
    out = {}
    for k in np.unique(cluster):
        rows = cluster == k
        scale = np.abs(ref[rows]).max()
        out[int(k)] = np.abs(got[rows] - ref[rows]).max() / (scale if scale >= 1e-9 * batch else batch)
    return out


@functools.lru_cache(maxsize=None)
def _model():
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    model = rt.HipModel(_hypers(), TYPES)
    model.load({k: v.to(dev) for k, v in _params().items()}, "energy")
    return model


def _graph(case, shuffled=False):
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    s = ac.system(case, shuffled)
    return rt.HipGraph(_model(), s.positions.to(dev), s.cells.to(dev), s.centers.int().to(dev), s.neighbors.int().to(dev),
                       s.cell_shifts.int().to(dev), s.species.int().to(dev), s.system_indices.int().to(dev))


class _Switches:
    def __init__(self, switches):
        self.switches = dict(switches)

    def __enter__(self):
        from metatrain_amd import runtime as rt

        for k, v in self.switches.items():
            rt.config_set(k, v)

    def __exit__(self, *exc):
        from metatrain_amd import runtime as rt

        for k, v in DEFAULT.items():
            rt.config_set(k, v)


@functools.lru_cache(maxsize=None)
def _device(case, shuffled, policy):
    """Two forward + dE/dR runs of the case under the switches ``policy`` (a tuple of items; () is the default policy): the
    first run's arrays, whether the second gave the same bits, the stages that ran and the graph's largest neighbour count.
    Cached: the tests below look at the same run from several sides."""
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    w = _seed_vector(sum(ac.CASES[case])).to(dev)
    with _Switches(dict(policy)):
        graph = _graph(case, shuffled)
        fw = rt.HipForward(_model(), graph)
        runs = []
        rt.profile(True)
        try:
            for _ in range(2):
                atomic = fw.forward().clone()
                grad = fw.backward(w).clone()
                torch.cuda.synchronize()
                runs.append((atomic.cpu().numpy().reshape(-1), grad.cpu().numpy()))
            stages = {r["name"] for r in rt.profile_report()}
        finally:
            rt.profile(False)
    same = np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    return {"atomic": runs[0][0], "grad": runs[0][1], "same_bits": same, "stages": stages, "max_neighbors": graph.max_neighbors}


def _fused_stages(stages):
    return {s for s in stages if s.startswith("attn_blk")}


def _check_bars(case, tag, got):
    """Print every (case, cluster size, quantity, fp32-oracle error, device error), then assert the bars."""
    (a64, g64), (a32, g32) = _reference(case)
    cluster = ac.system(case).cluster
    sizes = ac.CASES[case]
    assert np.isfinite(got["atomic"]).all() and np.isfinite(got["grad"]).all()
    rows, bad = [], []
    for what, dev, ref, f32 in (("energy", got["atomic"], a64, a32), ("dE/dR", got["grad"], g64, g32)):
        y, e = cluster_errors(f32, ref, cluster), cluster_errors(dev, ref, cluster)
        for k, m in enumerate(sizes):
            rows.append((case + tag, m, what, y[k], e[k]))
            if not e[k] < max(TOL, 3.0 * y[k]):
                bad.append(rows[-1])
    for r in rows:
        print("attn-token-edges: %s  m = %3d  %-6s  fp32 oracle %.2e  device %.2e" % r)
    assert not bad, f"beyond max(1e-5, 3 x fp32 oracle): {bad}"
    for k, m in enumerate(sizes):
        if m == 1:  # no neighbour, no geometry: dE/dR of the lone atom is exactly zero
            assert not g64[cluster == k].any() and not got["grad"][cluster == k].any()


# ---- 1. first order, default policy ---------------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("case", ac.FIRST_ORDER)
def test_first_order_against_the_oracle(case, shuffled):
    got = _device(case, shuffled, ())
    _check_bars(case, " shuffled" if shuffled else "", got)
    assert got["same_bits"], "two runs of the same graph differ"


# ---- 2. which kernels ran ------------------------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("case,max_neighbors", [("t64", 63), ("t96", 95), ("t128", 127), ("t129", 128)])
def test_the_stated_kernels_ran(case, max_neighbors, shuffled):
    got = _device(case, shuffled, ())
    assert got["max_neighbors"] == max_neighbors
    stages = got["stages"]
    assert not _fused_stages(stages), stages
    if case == "t129":  # the size-generic pass: none of the tuned pass's attention stages
        assert not stages & THREE_KERNEL, stages
    else:
        assert THREE_KERNEL <= stages, stages


# ---- 3. the fused block's limit ------------------------------------------------------------------------------------------
@ORDERS
def test_the_fused_block_serves_64_tokens(shuffled):
    got = _device("t64", shuffled, tuple(FORCED.items()))
    assert FUSED <= got["stages"] and not got["stages"] & (THREE_KERNEL | {"oproj", "qkv_bwd"}), got["stages"]
    _check_bars("t64", " fused" + (" shuffled" if shuffled else ""), got)
    assert got["same_bits"]


@ORDERS
def test_the_fused_block_refuses_65_tokens_and_falls_back(shuffled):
    """One atom of more than 64 tokens takes the whole graph off the fused block even when it is forced
    (``emlp_s = 2, attn_fused = 7``): the three-kernel form runs, all of it, within the bars, and forcing the block changes no
    bit. ``emlp_s = 2`` also sends every row stage of this small graph through the ring kernels, which sum in another order
    than the default policy's (measured: the forced run differs from the default one in energies and dE/dR, with or without
    ``attn_fused = 7``). The bits are therefore compared under equal row kernels, both ways: ``attn_fused = 7`` against 3 with
    ``emlp_s = 2``, and ``attn_fused = 7`` alone against the default policy."""
    forced, default = _device("t96", shuffled, tuple(FORCED.items())), _device("t96", shuffled, ())
    assert not _fused_stages(forced["stages"]) and THREE_KERNEL <= forced["stages"], forced["stages"]
    _check_bars("t96", " forced" + (" shuffled" if shuffled else ""), forced)
    assert forced["same_bits"]
    rows_only = _device("t96", shuffled, (("emlp_s", FORCED["emlp_s"]),))
    assert np.array_equal(forced["atomic"], rows_only["atomic"]) and np.array_equal(forced["grad"], rows_only["grad"])
    block_only = _device("t96", shuffled, (("attn_fused", FORCED["attn_fused"]),))
    assert not _fused_stages(block_only["stages"]) and THREE_KERNEL <= block_only["stages"], block_only["stages"]
    assert np.array_equal(block_only["atomic"], default["atomic"]) and np.array_equal(block_only["grad"], default["grad"])


# ---- 4. the general kernels ----------------------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("case", ["t64", "t128"])
def test_general_kernels_behind_trr_0(case, shuffled):
    """``trr = 0``: no preload kernels, k_attn_fwd / k_attn_bwd <1..4> serve nt <= 4 (and <8> runs beside the LDS-tile row
    kernels at nt = 8). The stage names of the attention are those of the default policy; that the switch took is seen from
    ``dxf``, the separate kernel the adjoint only launches without the pipelined row kernels (pet_plan.hip dxf_fused)."""
    got = _device(case, shuffled, tuple(GENERAL.items()))
    assert {"attn_fwd", "attn_bwd", "dxf"} <= got["stages"] and not _fused_stages(got["stages"]), got["stages"]
    assert "dxf" not in _device(case, shuffled, ())["stages"]
    _check_bars(case, " trr=0" + (" shuffled" if shuffled else ""), got)
    assert got["same_bits"]


# ---- 5. training at the limit --------------------------------------------------------------------------------------------
def _train_inputs(case):
    inp = ac.inputs(case)
    n = len(inp["species"])
    gen = torch.Generator().manual_seed(11)
    nu = torch.rand(n, generator=gen) - 0.5
    u = torch.randn(n, 3, generator=gen)
    return inp, n, _seed_vector(n), nu, u


def _energy_term(case):
    """parameter gradients of sum_i w_i e_i from backward_train against the oracle's backward; the stages that ran"""
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    inp, n, w, _, _ = _train_inputs(case)
    ref = _oracle_param_grads(_params(), _hypers(), inp, w)
    model = _model()
    with _Switches({}):
        fw = rt.HipForward(model, _graph(case), train=True)
        model.zero_grad()
        rt.profile(True)
        try:
            fw.forward()
            fw.backward_train(w.to(dev))
            torch.cuda.synchronize()
            stages = {r["name"] for r in rt.profile_report()}
        finally:
            rt.profile(False)
    worst = _compare(model.grads(), ref, model, f"{case} energy term")
    print(f"attn-token-edges: {case}  energy-term parameter gradients  worst {worst:.2e}")
    return stages


@pytest.mark.parametrize("case", ac.SECOND_ORDER)
def test_training_energy_term_at_the_second_order_limit(case):
    stages = _energy_term(case)
    assert {"attn_fwd", "attn_bwd"} <= stages, stages  # the tuned pass's <8> instantiations


@pytest.mark.parametrize("case", ac.SECOND_ORDER)
def test_training_force_loss_term_at_the_second_order_limit(case):
    """``backward_train2`` at T_max = 121 (k_attn_rev's first size under the LDS opt-in) and 128 (the largest served): tangent
    energies and the parameter gradients of sum_i nu_i e_i + <u, dE/dR> against the oracle's double backward."""
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    inp, n, _, nu, u = _train_inputs(case)
    ref, tan_ref, g_ref = _oracle_second_order(_params(), _hypers(), inp, nu, u)
    model = _model()
    with _Switches({}):
        graph = _graph(case)
        assert graph.max_neighbors + 1 == ac.STATED[case][0]
        fw = rt.HipForward(model, graph, train=True)
        model.zero_grad()
        ones = torch.ones(n, device=dev)
        rt.profile(True)
        try:
            fw.forward()
            gpos = fw.backward(ones)
            tan = fw.backward_train2(ones, nu.to(dev), u.to(dev), want_tangent=True)
            torch.cuda.synchronize()
            stages = {r["name"] for r in rt.profile_report()}
        finally:
            rt.profile(False)
    assert {"so_attn_jvp", "so_attn_rev"} <= stages, stages
    e_g = np.abs(gpos.cpu().numpy() - g_ref.numpy()).max() / np.abs(g_ref.numpy()).max()
    e_t = np.abs(tan.cpu().numpy() - tan_ref.numpy()).max() / np.abs(tan_ref.numpy()).max()
    print(f"attn-token-edges: {case}  dE/dR {e_g:.2e}  tangent energies {e_t:.2e}")
    assert e_g < TOL and e_t < TOL
    worst = _compare(model.grads(), ref, model, f"{case} force-loss term")
    print(f"attn-token-edges: {case}  force-loss parameter gradients  worst {worst:.2e}")


def test_hessian_vector_product_at_128_tokens():
    from metatrain_amd import runtime as rt

    dev = torch.device("cuda:0")
    inp = ac.inputs("so128")
    n = len(inp["species"])
    gen = torch.Generator().manual_seed(1)
    u = torch.randn(n, 3, generator=gen)
    weights = torch.rand(n, generator=gen) + 0.5
    ref, ys = _hvp_reference(_params(), _hypers(), inp, u, torch.zeros(1, 3, 3), weights)
    with _Switches({}):
        graph = _graph("so128")
        assert graph.max_neighbors == 127
        hp, tan = rt.hessian_vector_product(_model(), graph, u.to(dev), None, weights.to(dev), want_tangent=True)
    errs = [hvp_relmax(hp, ref[0]), hvp_relmax(tan, ref[2])]
    print(f"attn-token-edges: so128  hvp (y, relmax) positions ({ys[0]:.2e}, {errs[0]:.2e}) tangent ({ys[2]:.2e}, {errs[1]:.2e})")
    assert errs[0] <= hvp_bar(ys[0]) and errs[1] <= hvp_bar(ys[2]), (errs, ys)


# ---- 6. one neighbour too many for the tuned training pass -----------------------------------------------------------------
def test_training_with_128_neighbours_runs_the_size_generic_pass():
    stages = _energy_term("t129")
    assert not stages & (THREE_KERNEL | {"so_attn_jvp", "so_attn_rev"}), stages
