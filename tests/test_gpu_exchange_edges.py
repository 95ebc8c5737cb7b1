"""The per-layer exchange of ONE PET box over several ranks (``pet_graph_set_exchange``,
``partition.energy_and_gradient_exchange``) at its slab, peer and stage-plan edges: the cases of ``exchange_cases.py`` (premises:
``test_exchange_cases_cpu.py``) on the device against the fp64 oracle ``oracle/pet.py`` on the WHOLE box.

Harness. The ranks of a run are threads of this process with the in-process all-to-all of ``test_gpu_exchange.ThreadWorld``
(``side_stream`` = 0 while they run: the threads share the process' streams; the barrier's timeout and the abort on error end
the test if a rank fails). The threaded run RECORDS, per rank, the rows that arrived in every all-to-all (forward: ``ghost_buf``,
reverse: ``export_buf``; call k is layer k of the forward for k < L and layer 2 L - 1 - k of the reverse after that) and the
rows it SENT. A rank can then be REPLAYED alone in the main thread with a callback that copies the recording into its receive
buffer on the current stream and holds the rows the rank sends to the bits of those it sent before: deterministic, thread-free,
and free to run with ``side_stream`` = 1, the configuration of a real multi-process run (a gather that read its rows before
they were complete would show in what is sent, a scatter out of order in what the rank returns). A spy in place of the
``runtime`` argument hands back the rank's per-atom energies, which the library call sums away. ``side_stream`` goes back to 1,
the library's default, afterwards (``pet_config_set`` has no getter; every suite here leaves the switches at their defaults).

  1. oracle        every case and world: per-atom energies of the owned atoms gathered over the ranks, the sum of the ranks'
                   gradients and of their energies against the oracle; ``owned`` sums to N; an empty rank returns zeros;
  2. per rank      ``slab`` (world 3) and ``surface``: rank r's own gradient, halo atoms included, against the oracle's statement
                   of it: the part of dE/dR that flows through the rows r owns (``exchange_cases.rank_gradients``; with the
                   exchange the adjoints of ghost rows go home, so a rank does NOT return the gradient of its owned energies
                   -- the halo scheme does, and section 6 holds it to that). A ghost adjoint sent to the wrong row, twice, or
                   not zeroed shows on the rank where it happens; ``slab`` again under the forced ring kernels;
  3. stage forms   ``slab`` (world 3) and ``dense`` (world 2) under each setting of ``STAGE_FORMS`` (set before the graphs are
                   built), the same assertions. That a form was reached: the profiled stage names and declared bytes of a
                   replayed rank (the forced form), dE/dR differing in bits from the default switches (``trr=0``, the forced
                   form, ``node_planes=0``, ``trr_compress=0``), the number of ``center`` launches (``center_fused=0``).
                   ``attn_fused=0`` changes nothing on graphs this small, which the plan does not fuse by default: it is run
                   and held to the bits of the default switches, and is not counted as a form of its own;
  4. side stream   every rank of ``slab`` (world 3) replayed with ``side_stream`` = 1: the bits of the threaded run; a rank
                   replayed twice: the same bits;
  5. refusals      by message, nothing launched that could fault; the graph's exchange is cleared afterwards;
  6. halo scheme   ``partition.energy_and_gradient`` (exact hops, ranks looped, no threads) on the same cases and oracle.

Bar: ``relmax`` = max |got - oracle| / max |oracle| per quantity below 1e-5 (``test_gpu_exchange.TOL``, the bar of
``test_gpu_parity.py``) in every case but ``unwrapped``, the one case measured to miss it (dE/dR: the device 1.67e-5, the fp32
oracle 1.70e-5 on the same machine): there the bar of dE/dR is max(1e-5, 3 x the fp32 oracle's own distance from the fp64
oracle), about 5.1e-5 (``_bars``). Every ``(case, world, rank or "sum", quantity, relmax)`` is printed before it is asserted;
the figures of one run, beside the fp32 oracle's own distance from the fp64 oracle, are in DESIGN.md."""
import collections
import functools
import threading

import numpy as np
import pytest
import torch

import exchange_cases as X
from test_gpu_exchange import TOL, ThreadWorld
from test_gpu_stage_plan import digests

pytestmark = pytest.mark.gpu

Rank = collections.namedtuple("Rank", "energy grad n_sub n_owned n_rows n_ghost atomic index owned")
THREE_KERNEL = {"qkv", "attn_fwd", "oproj", "qkv_bwd", "attn_bwd", "oproj_bwd"}
FUSED = {"attn_blk", "attn_blk_bwd"}
# every form: with an exchange in place dXF is never folded into the combination adjoint ("dxf" is a stage of its own)
REF32_CASES = ("unwrapped",)  # the cases measured to miss 1e-5 in dE/dR by fp32 rounding of the INPUT (``_bars``)
# the settings that put another kernel in some stage of graphs this small: dE/dR must NOT have the bits of the default switches
OTHER_BITS = ("trr=0", X.FORCED, "node_planes=0", "trr_compress=0")
SAME_BITS = ("default", "attn_fused=0")  # a small graph is not fused by default: the switch changes nothing here
COMMON = {"center", "center_bwd", "comb", "comb_bwd", "compress", "compress_bwd", "dxf", "emlp", "emlp_bwd", "head_edge",
          "head_edge_bwd", "head_node", "head_node_bwd", "node", "node_bwd"}


def _dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _model(**delta):
    from metatrain_amd import runtime as rt

    model = rt.HipModel(X.hypers(**delta), X.TYPES)
    model.load({k: v.to(_dev()) for k, v in X.params(**delta).items()}, "energy")
    return model


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = X.CASES.get(name) or X.REFUSALS[name]
    return c.positions.to(_dev()), c.species.to(_dev()), c.cell.to(_dev()), list(c.pbc)


class _Spy:
    """``metatrain_amd.runtime`` as ``energy_and_gradient_exchange`` sees it, keeping what the call does not return: the graph,
    what it was built from and the per-atom energies. ``train`` / ``forward``: another pass in place of the inference forward
    (the refusals)."""

    def __init__(self, train=False, forward=None):
        from metatrain_amd import runtime as rt

        self._rt, self._train, self._forward = rt, train, forward
        self.graph = self.graph_args = self.atomic = None

    def __getattr__(self, key):
        return getattr(self._rt, key)

    def HipGraph(self, *args):
        self.graph_args = args
        self.graph = self._rt.HipGraph(*args)
        return self.graph

    def HipForward(self, model, graph):
        fw = self._rt.HipForward(model, graph, train=self._train)
        inner, spy = fw.forward, self

        def forward():
            out = spy._forward(model, graph) if spy._forward else inner()
            spy.atomic = out.reshape(-1).clone()
            return out

        fw.forward = forward
        return fw


def _run_rank(name, world, rank, all_to_all, model=None, spy=None):
    from metatrain_amd.partition import slab_partition
    from metatrain_amd.pet import partition

    pos, z, cell, pbc = _inputs(name)
    spy = spy or _Spy()
    out = partition.energy_and_gradient_exchange(model or _model(), pos, z, cell, pbc, world, rank, all_to_all, runtime=spy)
    index, owned, _ = slab_partition(pos, cell, pbc, X.CUTOFF, world, rank)
    return Rank(*out, spy.atomic, index, owned)


@functools.lru_cache(maxsize=None)
def _threaded(name, world, spec="default"):
    """``(ranks, tapes, sent)`` of one threaded run: per rank its :class:`Rank`, the rows that arrived in each of its all-to-alls
    and the rows it sent in each"""
    from metatrain_amd import runtime as rt

    dev = _dev()
    rt.config_set("side_stream", 0)   # the rank threads share this process' streams
    try:
        with digests.switches(spec):  # before the graphs are built: a small graph plans its attention tiles only then
            tw = ThreadWorld(world)
            ranks, tapes, sent, errors = [None] * world, [[] for _ in range(world)], [[] for _ in range(world)], []

            def run(rank):
                try:
                    torch.cuda.set_device(dev)
                    inner = tw.all_to_all(rank)

                    def recording(out, inp, out_splits, in_splits):
                        sent[rank].append(inp.clone())  # (behind the library's gather on this stream)
                        inner(out, inp, out_splits, in_splits)
                        tapes[rank].append(out.clone())

                    ranks[rank] = _run_rank(name, world, rank, recording)
                except BaseException as exc:  # noqa: BLE001
                    errors.append(exc)
                    tw.barrier.abort()

            threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
            [t.start() for t in threads]
            [t.join() for t in threads]
            assert not errors, errors
            torch.cuda.synchronize()
    finally:
        rt.config_set("side_stream", 1)
    assert all(len(t) == 2 * X.N_LAYERS for t in tapes + sent)
    return ranks, tapes, sent


def _replay(name, world, rank, spec="default", side_stream=0, profile=False, tamper=None):
    """rank ``rank`` alone in this thread, fed from the recording: ``(Rank, profile report or None)``. ``tamper(k, rows)``:
    what arrives in call k instead (the tests of the checks themselves)."""
    from metatrain_amd import runtime as rt

    run = _threaded(name, world, spec)
    tape, sent, used = run[1][rank], run[2][rank], [0]

    def all_to_all(out, inp, out_splits, in_splits):
        k = used[0]
        rows = tape[k] if tamper is None else tamper(k, tape[k])
        used[0] += 1
        assert rows.shape == out.shape and sum(out_splits) == out.shape[0] and sum(in_splits) == inp.shape[0]
        # what the rank sends has the bits of what it sent among the threads: the gather found its rows complete
        assert tamper is not None or torch.equal(inp, sent[k]), f"call {k}: the rows this rank sends differ from the recording"
        out.copy_(rows)  # on the current stream, where the library's scatter follows

    report = None
    rt.config_set("side_stream", side_stream)
    try:
        with digests.switches(spec):
            if profile:
                rt.profile(True)
            try:
                res = _run_rank(name, world, rank, all_to_all)
                torch.cuda.synchronize()
                if profile:
                    report = {r["name"]: r for r in rt.profile_report()}
            finally:
                if profile:
                    rt.profile(False)
    finally:
        rt.config_set("side_stream", 1)
    assert used[0] == len(tape)
    return res, report


def _say(name, world, who, quantity, value):
    print(f"exchange-edges: {name} world {world} {who} {quantity} relmax {value:.2e}")
    return value


@functools.lru_cache(maxsize=None)
def _bars(name):
    """``(per-atom energies, dE/dR)``: 1e-5. One case was measured to miss it in dE/dR, ``unwrapped``: positions of up to 108 A
    carry 7.6e-6 A of fp32 rounding into every edge vector. There, and there alone, the bar of dE/dR is max(1e-5, three times
    the fp32 ORACLE's own distance from the fp64 oracle on the case): the rule of ``test_gpu_parity.py`` for its large box,
    never the device's own output."""
    if name not in REF32_CASES:
        return TOL, TOL
    _, g32 = X.ref32(name)
    print(f"exchange-edges: {name} fp32 oracle against fp64: dE/dR {g32:.2e}")
    return TOL, max(TOL, 3.0 * g32)


def _against_oracle(name, world, spec="default"):
    ranks = _threaded(name, world, spec)[0]
    atomic_ref, grad_ref = X.oracle(name)
    n = len(atomic_ref)
    atomic = np.full(n, np.nan)
    grad = np.zeros((n, 3))
    for rank, r in enumerate(ranks):
        if r.n_owned == 0 and r.n_sub == 0:  # an empty slab: nothing was launched, exact zeros come back
            assert (r.n_sub, r.n_owned, r.n_rows, r.n_ghost) == (0, 0, 0, 0) and r.atomic is None
            assert float(r.energy) == 0.0 and float(r.grad.abs().max()) == 0.0
            continue
        assert r.atomic.shape == (r.n_sub,) and r.index.numel() == r.n_sub and int(r.owned.sum()) == r.n_owned
        own = r.index[r.owned].cpu().numpy()
        assert np.isnan(atomic[own]).all()
        atomic[own] = r.atomic[r.owned].double().cpu().numpy()
        grad += r.grad.double().cpu().numpy()
        rest = torch.ones(n, dtype=torch.bool)
        rest[r.index.cpu()] = False
        assert float(r.grad.cpu()[rest].abs().sum()) == 0.0  # nothing outside the rank's sub-system
    assert sum(r.n_owned for r in ranks) == n and not np.isnan(atomic).any()
    who = "sum" if spec == "default" else f"sum [{spec}]"
    energy = sum(float(r.energy) for r in ranks)
    figures = (_say(name, world, who, "per-atom energies", X.relmax(atomic, atomic_ref)),
               _say(name, world, who, "dE/dR", X.relmax(grad, grad_ref)),
               _say(name, world, who, "energy", X.relmax([energy], [atomic_ref.sum()])))
    bar_e, bar_g = _bars(name)
    assert figures[0] < bar_e and figures[1] < bar_g and figures[2] < TOL, (figures, bar_e, bar_g)
    return ranks


# ---- 1. every case and world against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,world", X.CASE_WORLDS)
def test_ranks_add_up_to_the_oracle(name, world):
    ranks = _against_oracle(name, world)
    if name == "clustered":
        assert [r.n_owned for r in ranks] == [0, 40, 0, 0] and [r.n_sub for r in ranks] == [0, 40, 0, 0]
    if name == "gap":
        assert [r.n_ghost for r in ranks] == [0, 0] and all(r.n_rows > 0 for r in ranks)
    if name == "isolated_alone":
        assert ranks[2].n_owned == 1 and ranks[2].n_rows == 0 and ranks[2].n_sub > 1


# ---- 2. a rank's own gradient ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,world,spec", [(n, w, "default") for n, w in X.PER_RANK] + [("slab", 3, X.FORCED)])
def test_each_rank_against_its_own_share_of_the_gradient(name, world, spec):
    """Rank r's result against the oracle's statement of it (``exchange_cases.rank_gradients``): the part of dE/dR that flows
    through the rows r owns -- NOT the gradient of the energies r owns, which only the halo scheme returns (section 6; printed
    here for information: the two differ by several per cent of the largest entry). Under the forced form too: the ring
    combination adjoint, ``k_dxf`` and the reverse exchange behind them, where a mis-routed adjoint could cancel in the sum."""
    ranks = _threaded(name, world, spec)[0]
    want, owned = X.rank_gradients(name, world), X.owned_energy_gradients(name, world)
    got = [r.grad.double().cpu().numpy() for r in ranks]
    tag = "" if spec == "default" else f" [{spec}]"
    figures = [_say(name, world, f"rank {k}{tag}", "share of dE/dR", X.relmax(got[k], want[k])) for k in range(world)]
    for k in range(world):
        _say(name, world, f"rank {k}{tag}", "(information) against d(owned energies)/dR", X.relmax(got[k], owned[k]))
    assert max(figures) < _bars(name)[1], figures


@pytest.mark.parametrize("fault", ["forward rows one row off", "reverse rows added twice"])
def test_the_per_rank_checks_can_tell(fault):
    """The checks have teeth: rank 1 of ``slab`` (world 3) replayed with a tampered recording -- every arriving edge token one
    ghost row off in layer 0, or the last layer's arriving adjoints doubled -- misses its oracle by more than a hundred bars."""
    name, world, rank = "slab", 3, 1
    call = 0 if fault.startswith("forward") else X.N_LAYERS  # (the reverse pass starts with the last layer)

    def tamper(k, rows):
        if k != call:
            return rows
        return torch.roll(rows, 1, 0) if call == 0 else 2.0 * rows

    res, _ = _replay(name, world, rank, tamper=tamper)
    own = res.index[res.owned].cpu().numpy()
    e = _say(name, world, f"rank {rank} [{fault}]", "per-atom energies",
             X.relmax(res.atomic[res.owned].double().cpu().numpy(), X.oracle(name)[0][own]))
    g = _say(name, world, f"rank {rank} [{fault}]", "share of dE/dR",
             X.relmax(res.grad.double().cpu().numpy(), X.rank_gradients(name, world)[rank]))
    assert g > 100 * TOL and (call != 0 or e > 100 * TOL), (e, g)


# ---- 3. the stage forms around the callback ----------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", X.STAGE_FORMS)
@pytest.mark.parametrize("name,world", X.STAGE_FORM_CASES)
def test_stage_forms_add_up_to_the_oracle(name, world, spec):
    ranks = _against_oracle(name, world, spec)
    base = _threaded(name, world)[0]
    same = [torch.equal(a.grad, b.grad) for a, b in zip(ranks, base)]
    print(f"exchange-edges: {name} world {world} [{spec}] bits of the default switches per rank: {same}")
    # the switch took effect: another kernel in some stage rounds differently on EVERY rank; ``attn_fused=0`` is no form of its
    # own on graphs this small (not fused by default) and must change nothing. ``center_fused=0`` launches the same arithmetic
    # from another kernel: ``test_stage_names_per_form`` counts its launches.
    if spec in OTHER_BITS:
        assert not any(same), (spec, same)
    if spec in SAME_BITS:
        assert all(same), (spec, same)


@pytest.mark.parametrize("spec", X.STAGE_FORMS)
@pytest.mark.parametrize("name,world,rank", [("slab", 3, 1), ("dense", 2, 0)])
def test_stage_names_per_form(name, world, rank, spec):
    """The form was reached with the exchange in place: the profiled stage names of the rank replayed alone. The names tell the
    fused attention block from the three-kernel form and show ``dxf`` as a stage of its own in EVERY form (no graph without an
    exchange reaches it behind the ring combination adjoint); that the forced form runs the ring kernels shows in the bytes
    the edge MLP declares: its [v; g] is not stored, which only the recomputing ring adjoint allows."""
    res, report = _replay(name, world, rank, spec, profile=True)
    thr = _threaded(name, world, spec)[0][rank]
    assert torch.equal(res.grad, thr.grad) and torch.equal(res.atomic, thr.atomic) and torch.equal(res.energy, thr.energy)
    stages = sorted(report)
    print(f"exchange-edges: {name} world {world} rank {rank} [{spec}] stages {stages}")
    assert set(stages) == COMMON | (FUSED if spec == X.FORCED else THREE_KERNEL), stages
    hy = X.hypers()
    d, dff, layers = hy["d_pet"], hy["d_feedforward"], hy["num_gnn_layers"] * hy["num_attention_layers"]
    emlp = report["emlp"]
    assert emlp["calls"] == layers and report["dxf"]["calls"] == report["comb_bwd"]["calls"] == hy["num_gnn_layers"]
    stored = 0 if spec == X.FORCED else 2 * dff
    assert emlp["bytes"] == layers * res.n_rows * 4.0 * (2 * d + stored), (emlp, res.n_rows)
    # the centre tokens: written by the 32-row node kernel of the layer before (one ``center`` launch, the first layer's) unless
    # ``center_fused=0`` launches ``k_center`` in every layer, or the node stage runs another kernel (``node_planes=0``: the
    # LDS-tile one; the forced form: the ring chain), which writes none
    print(f"exchange-edges: {name} world {world} rank {rank} [{spec}] center launches {report['center']['calls']}")
    by_node = spec not in ("center_fused=0", "node_planes=0", X.FORCED)
    assert report["center"]["calls"] == (1 if by_node else layers), (spec, report["center"])


# ---- 4. the side stream; the same bits twice ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", range(3))
def test_side_stream_changes_no_bit(rank):
    thr = _threaded("slab", 3)[0][rank]
    for side in (1, 1, 0):
        res, _ = _replay("slab", 3, rank, side_stream=side)
        for what in ("energy", "grad", "atomic"):
            assert torch.equal(getattr(res, what), getattr(thr, what)), (rank, side, what)
        assert (res.n_sub, res.n_owned, res.n_rows, res.n_ghost) == (thr.n_sub, thr.n_owned, thr.n_rows, thr.n_ghost)


@pytest.mark.parametrize("name,world,rank,spec", [("dense", 2, 1, X.FORCED), ("slab", 12, 5, "default")])
def test_a_replayed_rank_gives_the_same_bits_twice(name, world, rank, spec):
    a, _ = _replay(name, world, rank, spec, side_stream=1)
    b, _ = _replay(name, world, rank, spec, side_stream=1)
    thr = _threaded(name, world, spec)[0][rank]
    for what in ("energy", "grad", "atomic"):
        assert torch.equal(getattr(a, what), getattr(b, what)) and torch.equal(getattr(a, what), getattr(thr, what)), what


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def _counting():
    calls = []

    def all_to_all(out, inp, out_splits, in_splits):
        calls.append((tuple(out.shape), tuple(inp.shape)))

    return calls, all_to_all


@pytest.mark.parametrize("name,message", [("two_images", "wider than two cutoffs"), ("crowded", "127 neighbours")])
def test_a_box_the_exchange_cannot_serve_is_refused_while_it_sets_up(name, message):
    calls, all_to_all = _counting()
    spy = _Spy()
    with pytest.raises(ValueError, match=message):
        _run_rank(name, 2, 0, all_to_all, spy=spy)
    assert not calls and spy.atomic is None  # no collective entered, no pass launched


def test_an_adaptive_cutoff_model_is_refused():
    from metatrain_amd import runtime as rt

    calls, all_to_all = _counting()
    spy = _Spy()
    model = rt.HipModel(X.hypers(num_neighbors_adaptive=12.0), X.TYPES)
    with pytest.raises(ValueError, match="built for the fixed cutoff"):
        _run_rank("slab", 3, 0, all_to_all, model=model, spy=spy)
    assert not calls and spy.graph is None


def _hessian_vector(model, graph):
    from metatrain_amd import runtime as rt

    return rt.hessian_vector_product(model, graph, torch.ones((graph.n_nodes, 3), device=_dev()))


@pytest.mark.parametrize("what,message", [("size", "tuned path"), ("train", "inference and forces"),
                                          ("hessian", "per-layer exchange")])
def test_a_pass_the_exchange_is_not_built_for_is_refused_and_the_graph_stays_usable(what, message):
    """Refused by the library with the graph's exchange in place (``PET_ERR_UNSUPPORTED``); the call still enters its
    collectives (its peers would be waiting) and clears the exchange: an ordinary forward on the same graph then gives the
    bits of a graph that never had one."""
    from metatrain_amd import runtime as rt
    from metatrain_amd._lib import PET_ERR_UNSUPPORTED

    calls, all_to_all = _counting()
    small = dict(d_pet=64, d_node=128, d_feedforward=128, d_head=64, num_heads=4)  # the "s64" sizes of test_gpu_gen_train.py
    model = _model(**small) if what == "size" else _model()
    spy = _Spy(train=what == "train", forward=_hessian_vector if what == "hessian" else None)
    with pytest.raises(rt.PetHipError, match=message) as err:
        _run_rank("slab", 3, 0, all_to_all, model=model, spy=spy)
    assert f"error {PET_ERR_UNSUPPORTED}:" in str(err.value), err.value
    assert len(calls) == 2 * X.N_LAYERS and spy.graph is not None
    used = rt.HipForward(model, spy.graph).forward()
    fresh = rt.HipForward(model, rt.HipGraph(*spy.graph_args)).forward()
    torch.cuda.synchronize()
    assert torch.equal(used, fresh) and bool(torch.isfinite(used).all())
    if what != "size":  # and the Hessian-vector product is served again
        assert bool(torch.isfinite(_hessian_vector(model, spy.graph)).all())


# ---- 6. the halo scheme on the same cases ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,world", X.HALO)
def test_halo_scheme_adds_up_to_the_oracle(name, world):
    from metatrain_amd.pet import partition

    pos, z, cell, pbc = _inputs(name)
    atomic_ref, grad_ref = X.oracle(name)
    n = len(atomic_ref)
    parts = [partition.energy_and_gradient(_model(), pos, z, cell, pbc, world, rank) for rank in range(world)]
    assert sum(p[3] for p in parts) == n
    if (name, world) == ("slab", 2):  # the 13.5 A halos of an 18 A slab in a 36 A box wrap onto each other
        assert [p[2] for p in parts] == [n, n]
    if name == "clustered":  # the 13.5 A halos of ranks 0 and 2 hold the cluster, which they do not own; rank 3 sees nothing
        assert [p[3] for p in parts] == [0, 40, 0, 0] and [p[2] for p in parts] == [40, 40, 40, 0]
        assert all(float(parts[r][0]) == 0.0 and float(parts[r][1].abs().max()) == 0.0 for r in (0, 2, 3))
    figures = (_say(name, world, "sum [halo]", "dE/dR", X.relmax(sum(p[1] for p in parts).double().cpu().numpy(), grad_ref)),
               _say(name, world, "sum [halo]", "energy", X.relmax([sum(float(p[0]) for p in parts)], [atomic_ref.sum()])))
    bar_g = _bars(name)[1]
    assert figures[0] < bar_g and figures[1] < TOL, figures
    if (name, world) in X.PER_RANK:  # here a rank's own result IS the gradient of the energies it owns
        want = X.owned_energy_gradients(name, world)
        own = [_say(name, world, f"rank {k} [halo]", "d(owned energies)/dR", X.relmax(p[1].double().cpu().numpy(), want[k]))
               for k, p in enumerate(parts)]
        assert max(own) < bar_g, own
