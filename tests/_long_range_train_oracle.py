"""CPU oracle of what a long-range PET's training step and Hessian-vector product compute: ``_ewald_oracle.model_reference``'s
lines restated so that the parameters are leaves of the graph, the six featuriser tensors included.

With ``e`` the per-atom energies and ``g = dE/dR`` of ``sum_i e_i`` (``create_graph=True``):

    J   = <nu, e> + <u, g>                the quantity a force loss differentiates (nu = dL_E/de, u = dL_F/dg)
    dJ/dtheta                             per parameter tensor (model and featuriser keys in one dictionary)
    e'  = d/d(w_i) <u, grad_R sum_i w_i e_i>   the per-atom tangents along u (sum e' = <u, g>)
    H u = grad_R <u, g>

evaluated in fp64 for the reference and in fp32 for the yardstick of the fp32-floor rule (``gen_shapes.bar``)."""
import functools
import math

import torch

import _ewald_oracle as eo
import ewald_cases as ec
import gen_shapes as gs
from oracle import pet as opet

SMEARING, RESOLUTION, CUTOFF = 1.4, 1.33, 4.5
MODELS = {"default": {}, "odd33": gs.CASES["odd33"], "residual": dict(featurizer_type="residual")}
PRE = "long_range_featurizer."


def atomic_energies(p, hypers, batch, pos, cells):
    """Per-atom energies ``[N]`` of the long-range PET for the parameters ``p`` (model and featuriser keys) at ``pos``."""
    ctr_in, nbr_in, sh_in, sysidx = batch["centers"], batch["neighbors"], batch["cell_shifts"], batch["system_indices"]
    _, nfs, efs, graph = opet.pet_atomic_energies(p, hypers, pos, cells, ctr_in, nbr_in, sh_in, batch["species"], sysidx,
                                                  "energy", return_features="all")
    lr = hypers["long_range"]
    x = sum(nfs) / math.sqrt(len(nfs))
    lin = torch.nn.functional.linear
    q = lin(x, p[PRE + "charges_map.weight"], p[PRE + "charges_map.bias"])
    v = eo.potential_batch(pos, cells, batch["pbcs"], batch["first_atom"], q, ctr_in, nbr_in, sh_in, float(lr["smearing"]),
                           float(lr["kspace_resolution"]), float(hypers["cutoff"]))
    hid = torch.nn.functional.silu(lin(v, p[PRE + "out_projection.0.weight"], p[PRE + "out_projection.0.bias"]))
    feat = lin(hid, p[PRE + "out_projection.2.weight"], p[PRE + "out_projection.2.bias"])
    hs = [(h + feat) * math.sqrt(0.5) for h in nfs]
    ctr = torch.as_tensor(graph.centers)
    silu = torch.nn.functional.silu
    atomic = None
    if len(graph.order):
        _, d_all = opet.edge_geometry(pos, cells, ctr_in, nbr_in, sh_in, sysidx)
        d0 = d_all[torch.as_tensor(graph.order)]
        cut = opet.cutoff_bump if hypers["cutoff_function"].lower() == "bump" else opet.cutoff_cosine
        fc = cut(d0, float(hypers["cutoff"]), float(hypers["cutoff_width"]))
    for l, (h, m) in enumerate(zip(hs, efs)):
        nl = silu(opet._linear(silu(opet._linear(h, p, f"node_heads.energy.{l}.0")), p, f"node_heads.energy.{l}.2"))
        contrib = opet._linear(nl, p, f"node_last_layers.energy.{l}.energy")
        if len(graph.order):
            el = silu(opet._linear(silu(opet._linear(m, p, f"edge_heads.energy.{l}.0")), p, f"edge_heads.energy.{l}.2"))
            edge_pred = opet._linear(el, p, f"edge_last_layers.energy.{l}.energy") * fc[:, None]
            contrib = contrib.index_add(0, ctr, edge_pred)
        atomic = contrib if atomic is None else atomic + contrib
    return atomic[:, 0]


def leaves_of(params, dtype):
    """The parameters as leaves in ``dtype``; the species table stays as it is."""
    return {k: (v if k == "species_to_species_index" else v.to(dtype).clone().requires_grad_(True)) for k, v in params.items()}


def evaluate(params, hypers, batch, nu, u, dtype):
    """One evaluation in ``dtype``, everything returned in fp64: ``atomic`` (e), ``grad`` (g), ``grads`` (dJ/dtheta per
    tensor, J = <nu, e> + <u, g>; ``u = None``: J = <nu, e>), and with a direction ``tangent`` (e') and ``hvp`` (H u)."""
    p = leaves_of(params, dtype)
    keys = [k for k in p if k != "species_to_species_index"]
    pos = batch["positions"].to(dtype).clone().requires_grad_(True)
    cells = batch["cells"].to(dtype)
    ones = torch.ones(pos.shape[0], dtype=dtype, requires_grad=True)
    e = atomic_energies(p, hypers, batch, pos, cells)
    (g,) = torch.autograd.grad((ones * e).sum(), pos, create_graph=True)
    out = {"atomic": e.detach().double(), "grad": g.detach().double()}
    J = (nu.to(dtype) * e).sum()
    if u is not None:
        phi = (u.to(dtype) * g).sum()
        hvp, tangent = torch.autograd.grad(phi, [pos, ones], retain_graph=True)
        out.update(hvp=hvp.detach().double(), tangent=tangent.detach().double())
        J = J + phi
    grads = torch.autograd.grad(J, [p[k] for k in keys], allow_unused=True)
    out["grads"] = {k: (torch.zeros_like(p[k]) if gr is None else gr).detach().double() for k, gr in zip(keys, grads)}
    return out


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_case(tag):
    """(hypers, one state dict: the model's synthetic parameters and the six featuriser tensors)."""
    hypers = ec.lr_hypers(SMEARING, RESOLUTION, **MODELS[tag])
    params = dict(opet.synthetic_params(hypers, eo.TYPES, {"energy": 1}, 0, torch.float32))
    params.update(eo.featurizer_params(hypers["d_node"], 0))
    return hypers, params


def three_atoms():
    """Three open atoms about 6 A apart: no pair inside the 4.5 A cutoff, so the model's graph has no edge at all."""
    pos = torch.tensor([[0.0, 0.0, 0.0], [5.9, 0.3, -0.2], [2.8, 5.4, 0.4]], dtype=torch.float64)
    return (pos, torch.zeros(3, 3, dtype=torch.float64), [False] * 3), torch.tensor([6, 8, 1], dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def batch_of(which):
    if which == "box":
        return eo.periodic_box_batch(64, 3, CUTOFF)
    if which == "qm9":
        return eo.qm9_batch(3, CUTOFF)
    if which == "model_batch":
        return ec.model_batch()
    if which == "box_alone":   # the box of model_batch() by itself
        systems, species = ec.model_systems()
        b = eo.collate([systems[1]], CUTOFF)
        b["species"] = species[40:104]
        return b
    tri, z = three_atoms()
    if which == "three":
        b = eo.collate([tri], CUTOFF)
        b["species"] = z
        return b
    assert which == "qm9_three", which
    q = eo.qm9_batch(1, CUTOFF)
    b = eo.collate([(q["positions"], torch.zeros(3, 3, dtype=torch.float64), [False] * 3), tri], CUTOFF)
    b["species"] = torch.cat([q["species"].to(torch.int32), z])
    return b


@functools.lru_cache(maxsize=None)
def seeds(which, seed=0):
    """``nu`` uniform in [-0.5, 0.5] and a random normal direction ``u`` (and a second one, ``v``) for a batch."""
    n = batch_of(which)["positions"].shape[0]
    g = torch.Generator().manual_seed(4100 + seed)
    return (torch.rand(n, generator=g, dtype=torch.float64) - 0.5, torch.randn(n, 3, generator=g, dtype=torch.float64),
            torch.randn(n, 3, generator=g, dtype=torch.float64))


@functools.lru_cache(maxsize=None)
def reference(tag, which, second_order=True, direction="u"):
    """(fp64 evaluation, fp32 evaluation) of a case, shared by the tests that need it and left unchanged."""
    hypers, params = model_case(tag)
    nu, u, v = seeds(which)
    d = None if not second_order else (u if direction == "u" else v)
    b = batch_of(which)
    return evaluate(params, hypers, b, nu, d, torch.float64), evaluate(params, hypers, b, nu, d, torch.float32)
