"""Fine-tuning on the GPU (``-m gpu``): LoRA adapters folded into the kernels' weights, their gradients, and frozen
parameters in the native step.

Bars: energies, forces and adapter gradients within 1e-5 relative of the reference (``pet_lora_box64.npz``, made by the
reference's own ``inject_lora_layers``) or of the fp64 oracle; a LoRA model against a plain model with the fold done on
the host within 1e-6; frozen parameters and their Adam moments bit-identical.
"""
import os

import numpy as np
import pytest
import torch

from oracle import pet as opet

pytestmark = pytest.mark.gpu

TOL = 1e-5
TYPES = [1, 6, 7, 8]
PLACES_ALL = ("attention.input_linear", "attention.output_linear", "mlp.w_in", "mlp.w_out", "center_mlp.w_in",
              "center_mlp.w_out", "center_contraction", "center_expansion")


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from metatrain_amd import runtime

    return runtime


DEV = torch.device("cuda:0")


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / np.abs(b).max()


def _inputs(golden_dir, name):
    g = dict(np.load(os.path.join(golden_dir, name)))
    return {k[3:]: torch.tensor(v) for k, v in g.items() if k.startswith("in_")}


def _graph(rt, model, inp):
    if "centers" not in inp:  # a box stored without its neighbour list (pet_default_box10000.npz)
        pos = inp["positions"].float().to(DEV)
        pairs, _ = rt.neighbor_list(pos, inp["cell"].float(), [True] * 3, model.hypers["cutoff"])
        return rt.HipGraph(model, pos, inp["cell"].float()[None].to(DEV), pairs[:, 0].contiguous(), pairs[:, 1].contiguous(),
                           pairs[:, 2:5].contiguous(), inp["species"].int().to(DEV),
                           torch.zeros(pos.shape[0], dtype=torch.int32, device=DEV))
    return rt.HipGraph(model, inp["positions"].float().to(DEV), inp["cells"].float().to(DEV), inp["centers"].to(DEV),
                       inp["neighbors"].to(DEV), inp["cell_shifts"].to(DEV), inp["species"].to(DEV),
                       inp["system_indices"].int().to(DEV))


def _lins(hypers, places):
    return [f"gnn_layers.{g}.trans.layers.{a}.{p}" for g in range(hypers["num_gnn_layers"])
            for a in range(hypers["num_attention_layers"]) for p in places
            if not (p.startswith("center") and hypers["d_node"] == hypers["d_pet"])]


def _inject(params, lins, rank=4, seed=5, adapters=None):
    """The state dict after LoRA injection (keys in the reference's order), A / B seeded or taken from `adapters`."""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in params.items():
        lin = k.rsplit(".", 1)[0]
        if lin not in lins:
            out[k] = v
            continue
        leaf = k.rsplit(".", 1)[1]
        out[f"{lin}.linear.{leaf}"] = v
        if leaf == "bias":
            n_out, k_in = params[lin + ".weight"].shape
            for name, shape in (("lora_A", (rank, k_in)), ("lora_B", (n_out, rank))):
                key = f"{lin}.{name}.weight"
                out[key] = (adapters[key] if adapters is not None
                            else 0.05 * torch.randn(shape, generator=gen)).float()
    return out


def _host_fold(injected, lins, s):
    out = {}
    for k, v in injected.items():
        if ".lora_" in k:
            continue
        lin = k.rsplit(".", 2)[0]
        if lin in lins and k.endswith(".linear.weight"):
            a, b = injected[lin + ".lora_A.weight"].double(), injected[lin + ".lora_B.weight"].double()
            v = (v.double() + s * b @ a).float()
        out[k.replace(".linear.", ".") if lin in lins else k] = v
    return out


def _model(rt, hypers, params, scaling=None):
    m = rt.HipModel(hypers, TYPES)
    m.load({k: v.to(DEV) for k, v in params.items()}, "energy", lora_scaling=scaling)
    return m


def _fixture(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "pet_lora_box64.npz")))
    keys = [str(k) for k in g["lora_keys"]]
    lins = sorted({k.rsplit(".", 2)[0] for k in keys})
    hypers = dict(opet.DEFAULT_HYPERS)
    base = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    adapters = {k: torch.tensor(g["lora::" + k]) for k in keys}
    return g, keys, lins, hypers, _inject(base, lins, adapters=adapters), float(g["scaling"])


# ---- 1. inference against the reference ------------------------------------------------------------------------
def test_lora_inference_matches_the_reference(rt, golden_dir):
    g, keys, lins, hypers, params, s = _fixture(golden_dir)
    model = _model(rt, hypers, params, s)
    fw = rt.HipForward(model, _graph(rt, model, _inputs(golden_dir, "pet_lora_box64.npz")))
    atomic = fw.forward()
    grad = fw.backward(torch.ones_like(atomic))
    assert relmax(atomic.cpu().numpy(), g["atomic"].ravel()) < TOL
    assert abs(float(atomic.double().sum()) - g["energies"][0, 0]) < TOL * abs(g["energies"][0, 0])
    assert relmax(grad.cpu().numpy(), g["grad"]) < TOL
    # the base weight reads back as uploaded, not as W_eff
    k = lins[0] + ".linear.weight"
    assert torch.equal(model.param(k).cpu(), params[k])


# ---- 2. the fold on every kernel path -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["box10000", "s64", "postln"])
def test_lora_fold_matches_host_fold(rt, golden_dir, case):
    hypers = dict(opet.DEFAULT_HYPERS)
    name = "pet_default_box64.npz"
    if case == "box10000":
        name = "pet_default_box10000.npz"
    elif case == "s64":
        hypers.update(d_pet=64, d_node=128, d_feedforward=128, d_head=64, num_heads=4)
        name = "pet_size_s64_box64.npz"
    else:
        hypers.update(transformer_type="PostLN")
    base = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    lins = _lins(hypers, PLACES_ALL)
    s = 0.75
    inj = _inject(base, lins, rank=8)
    inp = _inputs(golden_dir, name)
    out = []
    for params, scaling in ((inj, s), (_host_fold(inj, lins, s), None)):
        model = _model(rt, hypers, params, scaling)
        fw = rt.HipForward(model, _graph(rt, model, inp))
        a = fw.forward()
        out.append((a.cpu().numpy(), fw.backward(torch.ones_like(a)).cpu().numpy()))
    assert relmax(out[0][0], out[1][0]) < 1e-6
    assert relmax(out[0][1], out[1][1]) < 1e-6


# ---- 3. adapter gradients -----------------------------------------------------------------------------------------
def test_lora_gradients_match_the_reference(rt, golden_dir):
    g, keys, lins, hypers, params, s = _fixture(golden_dir)
    model = _model(rt, hypers, params, s)
    fw = rt.HipForward(model, _graph(rt, model, _inputs(golden_dir, "pet_lora_box64.npz")), train=True)
    model.zero_grad()
    fw.forward()
    n = g["seed_w"].shape[0]
    fw.backward_train2(torch.ones(n, device=DEV), torch.tensor(g["seed_w"]).float().to(DEV),
                       torch.tensor(g["seed_u"]).float().to(DEV))
    bad = {}
    for k in keys:
        r = relmax(model.grad(k).cpu().numpy(), g["dL::" + k])
        if not r < TOL:
            bad[k] = r
    assert not bad, bad


def _oracle_lora_grads(params, lins, s, hypers, inp, nu, u, ucell):
    p64 = {k: (v if k == "species_to_species_index" else v.double().clone().requires_grad_(True))
           for k, v in params.items()}
    eff = {}
    for k, v in p64.items():
        if ".lora_" in k:
            continue
        lin = k.rsplit(".", 2)[0]
        if lin in lins and k.endswith(".linear.weight"):
            v = v + s * p64[lin + ".lora_B.weight"] @ p64[lin + ".lora_A.weight"]  # differentiable W + s B A
        eff[k.replace(".linear.", ".") if lin in lins else k] = v
    pos = inp["positions"].double().clone().requires_grad_(True)
    cells = inp["cells"].double().clone().requires_grad_(True)
    atomic = opet.pet_atomic_energies(eff, hypers, pos, cells, inp["centers"], inp["neighbors"], inp["cell_shifts"],
                                      inp["species"], inp["system_indices"].long(), "energy")[:, 0]
    gp, gc = torch.autograd.grad(atomic.sum(), [pos, cells], create_graph=True)
    phi = (nu.double() * atomic).sum() + (u.double() * gp).sum()
    if ucell is not None:
        phi = phi + (ucell.double() * gc).sum()
    keys = [k for k in p64 if k != "species_to_species_index"]
    grads = torch.autograd.grad(phi, [p64[k] for k in keys], allow_unused=True)
    return {k: (torch.zeros_like(p64[k]) if gr is None else gr) for k, gr in zip(keys, grads)}


@pytest.mark.parametrize("case", ["tuned_cell", "s64"])
def test_lora_gradients_match_the_oracle(rt, golden_dir, case):
    """The gradients of the adapters and of the adapted base Linears of a LoRA model against fp64 autograd through the
    oracle with W + s B A in the parameters: the tuned path with a stress term (cell tangent), and a size-generic model."""
    hypers = dict(opet.DEFAULT_HYPERS)
    name = "pet_default_box64.npz"
    if case == "s64":
        hypers.update(d_pet=64, d_node=128, d_feedforward=128, d_head=64, num_heads=4)
        name = "pet_size_s64_box64.npz"
    base = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    lins = _lins(hypers, ("attention.input_linear", "mlp.w_out", "center_mlp.w_in", "center_expansion"))
    s = 1.5
    params = _inject(base, lins, rank=4)
    inp = _inputs(golden_dir, name)
    n = inp["positions"].shape[0]
    gen = torch.Generator().manual_seed(3)
    nu = torch.rand(n, generator=gen) - 0.5
    u = torch.randn(n, 3, generator=gen)
    ucell = torch.randn(1, 3, 3, generator=gen) if case == "tuned_cell" else None
    ref = _oracle_lora_grads(params, lins, s, hypers, inp, nu, u, ucell)
    model = _model(rt, hypers, params, s)
    fw = rt.HipForward(model, _graph(rt, model, inp), train=True)
    model.zero_grad()
    fw.forward()
    fw.backward_train2(torch.ones(n, device=DEV), nu.to(DEV), u.to(DEV),
                       u_cell=None if ucell is None else ucell.to(DEV))
    bad = {}
    for k, r in ref.items():
        if k.rsplit(".", 2)[0] not in lins:
            continue
        r = r.numpy()
        got = model.grad(k).cpu().numpy().astype(np.float64)
        scale = np.abs(r).max()
        err = np.abs(got - r).max() / scale if scale > 1e-12 else np.abs(got - r).max()
        if not err < TOL:
            bad[k] = err
    assert not bad, bad


# ---- 4. / 5. frozen parameters in the native step, the fold follows the optimizer --------------------------------
def _step_setup(rt, golden_dir, mode):
    from metatrain_amd.pet.finetuning import DEFAULT_HEADS_CONFIG

    hypers = dict(opet.DEFAULT_HYPERS)
    base = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    lins = _lins(hypers, ("attention.input_linear", "attention.output_linear"))
    params = _inject(base, lins) if mode == "lora" else dict(base)
    model = _model(rt, hypers, params, 2.0 if mode == "lora" else None)
    keys = list(model._ckeys)
    if mode == "lora":
        trainable = [k for k in keys if "lora_" in k]
    elif mode == "heads":
        pre = DEFAULT_HEADS_CONFIG["head_modules"] + DEFAULT_HEADS_CONFIG["last_layer_modules"]
        trainable = [k for k in keys if any(k.startswith(p) for p in pre)]
    else:
        trainable = keys
    if mode != "full":
        model.set_trainable(trainable)
    return hypers, params, model, keys, trainable


def _grads_of_one_pass(rt, model, inp, nu, u):
    fw = rt.HipForward(model, _graph(rt, model, inp), train=True)
    model.zero_grad()
    fw.forward()
    fw.backward_train2(torch.ones(nu.shape[0], device=DEV), nu, u)
    return model.grads()


@pytest.mark.parametrize("mode", ["lora", "heads"])
def test_frozen_parameters_stay_put_under_adamw(rt, golden_dir, mode):
    hypers, params, model, keys, trainable = _step_setup(rt, golden_dir, mode)
    inp = _inputs(golden_dir, "pet_default_box64.npz")
    n = inp["positions"].shape[0]
    gen = torch.Generator().manual_seed(9)
    before = {k: model.param(k).clone() for k in keys}
    # the torch side: AdamW + clip_grad_norm_ over the trainable set, fed the library's own gradients
    ref = {k: before[k].clone().double().requires_grad_(True) for k in trainable}
    opt = torch.optim.AdamW(list(ref.values()), lr=1e-3, weight_decay=0.01)
    for step in range(1, 4):
        nu = (torch.rand(n, generator=gen) - 0.5).to(DEV)
        u = torch.randn(n, 3, generator=gen).to(DEV)
        state0 = model.optimizer_state() if step > 1 else None
        grads = _grads_of_one_pass(rt, model, inp, nu, u)
        for k in keys:
            if k not in trainable:
                assert not grads[k].any(), f"frozen {k} received a gradient"
        for k in trainable:
            ref[k].grad = grads[k].double().clone()
        torch.nn.utils.clip_grad_norm_(list(ref.values()), 0.5)
        opt.step()
        model.adam_step(1e-3, step, weight_decay=0.01, max_grad_norm=0.5)
        state1 = model.optimizer_state()
        if state0 is not None:  # frozen entries of the moments do not move
            off = 0
            for k, numel in state1["layout"]:
                if k not in trainable:
                    for mom in ("exp_avg", "exp_avg_sq"):
                        assert torch.equal(state0[mom][off:off + numel], state1[mom][off:off + numel]), k
                off += numel
    for k in keys:
        now = model.param(k)
        if k in trainable:
            r = ref[k].detach().cpu()
            assert relmax(now.cpu().numpy(), r.numpy()) < 1e-6 or (now.double().cpu() - r).abs().max() < 1e-7, k
        else:
            assert torch.equal(now, before[k]), f"frozen {k} moved"
    if mode == "heads":  # the head gradients do not depend on freezing the backbone
        _, _, full, _, _ = _step_setup(rt, golden_dir, "full")
        _, _, heads, _, tr = _step_setup(rt, golden_dir, "heads")
        nu = (torch.rand(n, generator=gen) - 0.5).to(DEV)
        u = torch.randn(n, 3, generator=gen).to(DEV)
        gf, gh = _grads_of_one_pass(rt, full, inp, nu, u), _grads_of_one_pass(rt, heads, inp, nu, u)
        for k in tr:
            assert relmax(gh[k].cpu().numpy(), gf[k].cpu().numpy()) < 1e-6, k


def test_fold_follows_the_optimizer(rt, golden_dir):
    hypers, params, model, keys, trainable = _step_setup(rt, golden_dir, "lora")
    inp = _inputs(golden_dir, "pet_default_box64.npz")
    n = inp["positions"].shape[0]
    gen = torch.Generator().manual_seed(4)
    _grads_of_one_pass(rt, model, inp, (torch.rand(n, generator=gen) - 0.5).to(DEV), torch.randn(n, 3, generator=gen).to(DEV))
    model.adam_step(1e-2, 1)
    updated = {k: model.param(k).cpu() for k in keys}
    assert any(not torch.equal(updated[k], params[k]) for k in trainable)
    fresh = _model(rt, hypers, {**params, **updated}, 2.0)
    a = rt.HipForward(model, _graph(rt, model, inp)).forward()
    b = rt.HipForward(fresh, _graph(rt, fresh, inp)).forward()
    assert torch.equal(a, b)


# ---- 6. skipped work is not launched ------------------------------------------------------------------------------
def _stage_calls(rt, model, inp):
    n = inp["positions"].shape[0]
    fw = rt.HipForward(model, _graph(rt, model, inp), train=True)
    model.zero_grad()
    fw.forward()
    torch.cuda.synchronize()
    rt.profile(True)
    try:
        fw.backward_train2(torch.ones(n, device=DEV), torch.ones(n, device=DEV), torch.ones(n, 3, device=DEV))
        torch.cuda.synchronize()
        return {r["name"]: r["calls"] for r in rt.profile_report()}
    finally:
        rt.profile(False)


def test_frozen_work_is_not_launched(rt, golden_dir):
    inp = _inputs(golden_dir, "pet_default_box64.npz")
    calls = {mode: _stage_calls(rt, _step_setup(rt, golden_dir, mode)[2], inp) for mode in ("full", "lora", "heads")}
    assert calls["full"].get("so_attn_rev", 0) > 0
    assert calls["heads"].get("so_attn_rev", 0) == 0
    assert 0 < calls["lora"].get("wgrad", 0) < calls["full"]["wgrad"]
    _, _, explicit, keys, _ = _step_setup(rt, golden_dir, "full")
    explicit.set_trainable(keys)
    assert _stage_calls(rt, explicit, inp) == calls["full"]


# ---- refusals ----------------------------------------------------------------------------------------------------
def test_refused_adapters(rt):
    from metatrain_amd._lib import PetHipError

    hypers = dict(opet.DEFAULT_HYPERS)
    base = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    comb = _inject(base, ["combination_mlps.0.0"])
    with pytest.raises(PetHipError, match=r"combination_mlps\.0\.0\.linear\.weight"):
        _model(rt, hypers, comb, 1.0)
    lin = "gnn_layers.0.trans.layers.0.attention.input_linear"
    with pytest.raises(PetHipError, match="rank 65"):
        _model(rt, hypers, _inject(base, [lin], rank=65), 1.0)
    with pytest.raises(PetHipError, match="no scaling"):
        _model(rt, hypers, _inject(base, [lin]), None)
    silu = dict(hypers, activation="SiLU")
    sb = opet.synthetic_params(silu, TYPES, {"energy": 1}, 0, torch.float32)
    with pytest.raises(PetHipError, match="SiLU"):
        _model(rt, silu, _inject(sb, ["gnn_layers.0.trans.layers.0.mlp.w_in"]), 1.0)


def test_finalize_refuses_adapters_that_do_not_fit(rt):
    from metatrain_amd._lib import PetHipError

    hypers = dict(opet.DEFAULT_HYPERS)
    base = opet.synthetic_params(hypers, TYPES, {"energy": 1}, 0, torch.float32)
    lin = "gnn_layers.1.trans.layers.0.mlp.w_out"
    bad = _inject(base, [lin], rank=4)
    bad[lin + ".lora_B.weight"] = torch.zeros(bad[lin + ".lora_B.weight"].shape[0], 5)  # rank 5 against A's 4
    with pytest.raises(PetHipError, match="do not fit the base Linear"):
        _model(rt, hypers, bad, 1.0)
    # an adapter on a Linear the model does not have: d_node == d_pet has no centre modules
    flat = dict(hypers, d_pet=32, d_node=32, d_feedforward=48, d_head=24, num_heads=2)
    fb = opet.synthetic_params(flat, TYPES, {"energy": 1}, 0, torch.float32)
    cc = "gnn_layers.0.trans.layers.0.center_contraction"
    gen = torch.Generator().manual_seed(1)
    for key, shape in ((".linear.weight", (32, 32)), (".linear.bias", (32,)), (".lora_A.weight", (2, 32)),
                       (".lora_B.weight", (32, 2))):
        fb[cc + key] = torch.randn(shape, generator=gen)
    with pytest.raises(PetHipError, match="on a Linear this model does not have"):
        _model(rt, flat, fb, 1.0)


def test_optimizer_state_round_trip_with_adapters(rt, golden_dir):
    """Adam moments of a LoRA model (adapters in the flat layout) saved after one step and loaded into a fresh model:
    the next step equals the uninterrupted one bit for bit."""
    inp = _inputs(golden_dir, "pet_default_box64.npz")
    n = inp["positions"].shape[0]
    gen = torch.Generator().manual_seed(21)
    seeds = [((torch.rand(n, generator=gen) - 0.5).to(DEV), torch.randn(n, 3, generator=gen).to(DEV)) for _ in range(2)]
    hypers, params, model, keys, trainable = _step_setup(rt, golden_dir, "lora")
    _grads_of_one_pass(rt, model, inp, *seeds[0])
    model.adam_step(1e-3, 1, weight_decay=0.01, max_grad_norm=0.5)
    state = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in model.optimizer_state().items()}
    assert any(".lora_A." in k for k, _ in state["layout"])
    weights = {k: model.param(k).cpu() for k in keys}
    _grads_of_one_pass(rt, model, inp, *seeds[1])
    model.adam_step(1e-3, 2, weight_decay=0.01, max_grad_norm=0.5)
    fresh = _model(rt, hypers, {"species_to_species_index": params["species_to_species_index"], **weights}, 2.0)
    fresh.set_trainable(trainable)
    fresh.load_optimizer_state(state)
    _grads_of_one_pass(rt, fresh, inp, *seeds[1])
    fresh.adam_step(1e-3, 2, weight_decay=0.01, max_grad_norm=0.5)
    for k in keys:
        assert torch.equal(fresh.param(k), model.param(k)), k


# ---- the mirror (metatrain_amd.pet.PETBackend) after LoRA injection --------------------------------------------------
def _lora_mirror(golden_dir):
    from metatrain_amd.pet import PETBackend
    from metatrain_amd.pet.finetuning import inject_lora

    g, keys, lins, hypers, params, s = _fixture(golden_dir)
    be = PETBackend(hypers, TYPES)
    be.add_output("energy", {"energy": [1]})
    inject_lora(be, rank=4, alpha=8)
    be.load_state_dict(params, strict=True)
    return g, keys, be.to(DEV)


def _mirror_run(module, inp, create_graph=False):
    pos = inp["positions"].float().to(DEV).requires_grad_(True)
    cells = inp["cells"].float().to(DEV)
    sysidx = inp["system_indices"].long().to(DEV)
    batch = module.preprocess(pos, inp["centers"].long().to(DEV), inp["neighbors"].long().to(DEV),
                              inp["species"].long().to(DEV), cells, inp["cell_shifts"].long().to(DEV), sysidx, 1.0)
    nodes, edges = module.calculate_features(batch)
    pred, _, _ = module.predict(nodes, edges, batch, cells, sysidx, ["energy"])
    atomic = pred["energy"][0][:, 0]
    (grad,) = torch.autograd.grad([atomic.sum()], [pos], create_graph=create_graph)
    return atomic, grad


def test_lora_inference_through_the_mirror_eager_and_scripted(golden_dir):
    import io

    g, keys, be = _lora_mirror(golden_dir)
    be.eval()
    inp = _inputs(golden_dir, "pet_lora_box64.npz")
    atomic, grad = _mirror_run(be, inp)
    assert relmax(atomic.detach().cpu().numpy(), g["atomic"].ravel()) < TOL
    assert relmax(grad.cpu().numpy(), g["grad"]) < TOL
    buf = io.BytesIO()
    torch.jit.save(torch.jit.script(be), buf)
    buf.seek(0)
    mod = torch.jit.load(buf, map_location=DEV)
    a1, g1 = _mirror_run(mod, inp)
    assert torch.equal(atomic.detach(), a1.detach()) and torch.equal(grad, g1)


def test_lora_training_through_the_mirror(golden_dir):
    """loss.backward() on an injected mirror under the `lora` strategy fills .grad of the adapters only, equal to the
    reference's gradients of the fixture."""
    from metatrain_amd.pet.finetuning import apply_finetuning

    g, keys, be = _lora_mirror(golden_dir)
    apply_finetuning(be, {"method": "lora", "config": {"rank": 4, "alpha": 8}})
    be.train()
    inp = _inputs(golden_dir, "pet_lora_box64.npz")
    atomic, grad = _mirror_run(be, inp, create_graph=True)
    w = torch.tensor(g["seed_w"]).float().to(DEV)
    u = torch.tensor(g["seed_u"]).float().to(DEV)
    ((w * atomic).sum() + (u * grad).sum()).backward()
    named = dict(be.named_parameters())
    for k, p in named.items():
        if ".lora_" in k:
            assert relmax(p.grad.cpu().numpy(), g["dL::" + k]) < TOL, k
        else:
            assert p.grad is None, k
    model = next(iter(be._train_models.values()))  # the fused node's model got requires_grad as its trainable set
    assert {k for k, on in model._mirror_flags.items() if on} == {k for k in named if ".lora_" in k}
