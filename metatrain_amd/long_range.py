"""Long-range (Ewald) features of a ``long_range: {enable: true}`` PET on the HIP path (``utils/long_range.py:108-195``,
``pet/model.py:505-518, 664-695``).

With ``L`` readout layers and node features ``h_l [N, d_node]`` the reference computes

    x    = (sum_l h_l) / sqrt(L)
    q    = charges_map(x)                        Linear(d_node, d_node)
    V    = potential(q; positions, cell, NL)     per system, [n, d_node]
    lr   = out_projection(V)                     Linear -> SiLU -> Linear
    h_l <- (h_l + lr) / sqrt(2)   for every l,   then predict as usual

``potential`` is torch-pme's ``CoulombPotential`` / ``EwaldCalculator``. torch-pme is not part of the reference tree and its
tests pin no values, so the operator is fixed HERE by definition (the formulas are in ``include/pet_hip.h``, block
``pet_ewald_*``, and DESIGN.md section 18) and pinned to an independent fp64 oracle (``tests/_ewald_oracle.py``). **Parity
with torch-pme is not pinned.** Every convention constant of that definition is in :data:`CONVENTIONS` below (and, as the
same table); the kernels hold them as ``EW_PREFACTOR`` and the three coefficients ``ew_local_forward``
passes to ``k_ew_finish`` (``csrc/long_range.h``: the local terms and their adjoints, which both operators below launch) and
the weight ``pet_ewald_plan`` gives every k-vector (``csrc/ewald.hip``).

:class:`EwaldHip` is the operator (``csrc/ewald.hip``: structure factors, the gather back to atoms and the open all-pairs sum
as fp32 matrix-core GEMMs with a generated operand; fixed summation orders, no atomics), :class:`LongRangeFeaturizerHip` the
featuriser under the reference's state-dict keys, :func:`energy_and_gradient` the whole model: energies, dE/dR and dE/dcell.

Second derivatives are built at the OPERATOR level for the Ewald sum: :meth:`EwaldHip.second`
(``pet_ewald_second``) differentiates the adjoint -- ``dL/dq`` and ``dL/dR`` -- with respect to charges, ``dL/dV`` and positions,
and torch double backward (``create_graph=True``) through :class:`LongRangeFeaturizerHip` runs on it, which is what a force loss
and a Hessian-vector product need from the operator. At the MODEL level the size-generic dual pass
carries the featuriser between the backbone and the heads (``pet_backward_train2_long_range``,
``pet_hessian_vector_long_range``): :class:`LongRangeForward` and :class:`LongRangeTrainStep` are the training step on
energies and forces, :func:`hessian_vector_product` is ``H u``. The six featuriser tensors then live in the model's own
parameter table (:meth:`LongRangeFeaturizerHip.bind`). Behind ``LongRangeFeaturizerHip(...,
cell_tangents=True)`` the loss may hold a stress term (``EwaldHip.second_cell`` / ``P3MHip.second_cell``,
``pet_backward_train2_long_range_cell``). Not built, each raising by name: a stress / strain-gradient loss without that
opt-in, the position result under a cell tangent and every cell result of the second-order operation (cell directions of a
Hessian-vector product, cells that require grad in a double backward), further targets in the long-range step.

The reference takes its Ewald branch only under ``use_ewald and training`` (``utils/long_range.py:153-170``): with its default
hypers (``use_ewald: false``) a periodic long-range model goes through P3M in training and in evaluation alike.
:class:`P3MHip` is that operator (``csrc/p3m.hip``: binning, spread, filter, gather and the
adjoints as HIP kernels in stages around ``torch.fft.rfftn`` / ``irfftn``), fixed by definition like the Ewald one
(:data:`P3M_CONVENTIONS`, DESIGN.md section 19, oracle ``tests/_p3m_oracle.py``; parity with torch-pme unpinned). It is an
explicit opt-in: ``LongRangeFeaturizerHip(hypers, method="p3m")`` evaluates periodic systems with P3M whatever ``use_ewald``
says, ``method="ewald"`` (the earlier ``p3m_as_ewald=True``) with the Ewald sum P3M approximates, and without either a
``use_ewald: false`` model is refused.

Second derivatives through the mesh operator are a further opt-in, ``second_order=True`` on
:class:`P3MHip` and on a ``method="p3m"`` :class:`LongRangeFeaturizerHip`: the operator's stages run around ``torch.fft``, which
this library does not link, so ``pet_p3m_second`` and the dual pass call the transforms back through a hook the operator
installs (``pet_p3m_set_transform``). With it :meth:`P3MHip.second`, torch double backward, :class:`LongRangeTrainStep`,
:class:`LongRangeForward` and :func:`hessian_vector_product` serve a P3M featuriser; without it they raise as before.
"""
import logging
import math
import weakref
from ctypes import byref, c_double, c_int32, c_int64, c_void_p
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib
from . import runtime as rt
from ._lib import PetHipError, check

# The convention table (sigma = smearing, lambda = kspace_resolution, Omega = |det cell|, R = the model cutoff).
CONVENTIONS = {
    "prefactor": "P = 1/2 on every term (torch-pme's Calculator halves the pair sum)",
    "kernel": "G(k) = 4 pi exp(-sigma^2 k^2 / 2) / k^2, summed over k != 0 and divided by Omega",
    "self": "- q_i sqrt(2 / pi) / sigma",
    "background": "- (2 pi sigma^2 / Omega) sum_j q_j  (= pi / (Omega a^2) with a = 1 / (sqrt(2) sigma))",
    "k_set": "the sphere |k| <= 2 pi / lambda of the reciprocal lattice 2 pi n cell^{-T} (torch-pme: the box of a mesh)",
    "exclusion": "- sum over the model's edges of q_j erf(d / (sqrt(2) sigma)) / d * (1 + cos(pi d / R)) / 2",
    "open": "P sum_{j != i} q_j (1 - (1 + cos(pi d / R)) / 2 [d < R]) / d over all pairs of a system without pbc",
}
PREFACTOR = 0.5

# The mesh operator's conventions (h = kspace_resolution, the reference's mesh_spacing; p = interpolation_nodes in 1..5). The
# self, background, exclusion and open-system terms and the prefactor are those of CONVENTIONS.
P3M_CONVENTIONS = {
    "mesh": "N_a = 2^ceil(log2(|cell row a| / h)), at least 1 (believed to be torch-pme's get_ns_mesh; unpinned)",
    "assignment": "the order-p P3M (Hockney-Eastwood) charge-assignment function: the centred cardinal B-spline "
                  "W(x) = M_p(x + p/2), separable over the fractional axes, in mesh units u_a = s_a N_a, s = r cell^{-1} in [0, 1)",
    "nodes": "odd p: around floor(u + 1/2), offsets -(p-1)/2 .. (p-1)/2; even p: around floor(u), offsets -(p/2-1) .. p/2; "
             "indices mod N_a (N_a < p: several nodes fall on one mesh point and their weights add)",
    "influence": "G^(n) = sum_m U_m^2 G(|k_{n+mN}|) / (sum_m U_m^2)^2, G^(0) = 0, G as in CONVENTIONS, k_nu = 2 pi nu cell^{-T}, "
                 "U_m = prod_a sinc^p((n_a + m_a N_a) / N_a), aliases m in {-2..2}^3, n_a in [-N_a/2, N_a/2)",
    "mesh_potential": "Phi = (1/Omega) sum_n G^(n) rho^(n) e^{2 pi i n.j/N}: unnormalised transforms, G^/Omega is the filter",
    "gather": "sum over the same nodes of W_i(node) Phi(node)",
}
METHODS = (None, "ewald", "p3m")

REFERENCE_KEYS = ("long_range_featurizer.charges_map.weight", "long_range_featurizer.charges_map.bias",
                  "long_range_featurizer.out_projection.0.weight", "long_range_featurizer.out_projection.0.bias",
                  "long_range_featurizer.out_projection.2.weight", "long_range_featurizer.out_projection.2.bias")

_warned_kset = False


def truncation_factor(smearing: float, kspace_resolution: float) -> float:
    """``exp(-(sigma 2 pi / lambda)^2 / 2)``: the size of the first k-space terms left out, relative to the largest."""
    return math.exp(-0.5 * (float(smearing) * 2.0 * math.pi / float(kspace_resolution)) ** 2)


def resolve_hypers(hypers: dict, p3m_as_ewald: bool = False, method: Optional[str] = None) -> dict:
    """The ``long_range`` block of a model's hypers with the reference's defaults filled in, checked for what this package
    serves. Raises for a model without ``long_range.enable``, for ``use_ewald: false`` without an explicit choice
    (``method="p3m"``, ``method="ewald"`` or the earlier ``p3m_as_ewald=True``), for an unknown ``method``, for
    ``interpolation_nodes`` outside 1..5 under ``method="p3m"`` and for an adaptive cutoff together with long range."""
    from .pet.hypers import long_range_hypers

    if method not in METHODS:
        raise PetHipError(f"method must be one of None, 'ewald', 'p3m': got {method!r}")
    lr = long_range_hypers(hypers)
    if not lr["enable"]:
        raise PetHipError("long_range.enable is false: this model has no long-range featuriser")
    if not lr["use_ewald"] and not p3m_as_ewald and method is None:
        raise PetHipError("long_range.use_ewald is false: the reference evaluates this model with P3M, which is an explicit "
                          "opt-in here: pass method='p3m' to evaluate with it. Ewald summation is the sum P3M approximates: "
                          "pass p3m_as_ewald=True (or method='ewald') to evaluate with that")
    if method == "p3m":
        _check_nodes(lr["interpolation_nodes"])
    if hypers.get("num_neighbors_adaptive"):
        raise PetHipError("long_range together with num_neighbors_adaptive: the adaptive cutoff drops edges inside the "
                          "exclusion radius, on which the long-range exclusion term relies")
    return lr


def _check_nodes(interpolation_nodes) -> int:
    if isinstance(interpolation_nodes, bool) or int(interpolation_nodes) != interpolation_nodes or not 1 <= int(interpolation_nodes) <= 5:
        raise PetHipError(f"interpolation_nodes must be an integer in 1..5: got {interpolation_nodes!r}")
    return int(interpolation_nodes)


def _cell9(cell):
    flat = [float(x) for x in torch.as_tensor(cell, dtype=torch.float64).reshape(-1).tolist()]
    if len(flat) != 9:
        raise ValueError("cell must be [3, 3]")
    return (c_double * 9)(*flat)


def mesh_shape(cell, spacing: float) -> List[int]:
    """The P3M mesh ``[N_0, N_1, N_2]`` of one ``cell [3, 3]`` at mesh spacing ``spacing`` (``pet_p3m_mesh_shape_host``).
    Needs no GPU."""
    out = (c_int32 * 3)()
    if _lib.load().pet_p3m_mesh_shape_host(_cell9(cell), float(spacing), out) != 0:
        raise PetHipError("singular cell or non-positive spacing")
    return [int(x) for x in out]


def influence(cell, smearing: float, spacing: float, interpolation_nodes: int = 5) -> torch.Tensor:
    """The filter ``G^(n) / Omega`` (fp64, host) on the half spectrum ``[N_0, N_1, N_2 / 2 + 1]`` of one cell's mesh, from the
    function the device evaluates at plan time (``pet_p3m_influence_host``). Needs no GPU."""
    lib = _lib.load()
    p = _check_nodes(interpolation_nodes)
    h = _cell9(cell)
    n = int(lib.pet_p3m_influence_host(h, float(smearing), float(spacing), p, None, 0))
    if n < 0:
        raise PetHipError("singular cell, or non-positive smearing or spacing")
    buf = (c_double * n)()
    lib.pet_p3m_influence_host(h, float(smearing), float(spacing), p, buf, n)
    shape = mesh_shape(cell, spacing)
    return torch.tensor(list(buf), dtype=torch.float64).reshape(shape[0], shape[1], shape[2] // 2 + 1)


def kvectors(cell, kspace_resolution: float) -> torch.Tensor:
    """The k-set ``[K, 3]`` (fp64, host) the plan builds for one ``cell [3, 3]``: every ``k = 2 pi n cell^{-T} != 0`` with
    ``|k| <= 2 pi / kspace_resolution`` (``pet_ewald_kvectors_host``; the kernels walk one of every pair ``(k, -k)``).
    Needs no GPU."""
    lib = _lib.load()
    h = _cell9(cell)
    n = int(lib.pet_ewald_kvectors_host(h, float(kspace_resolution), None, 0))
    if n < 0:
        raise PetHipError("singular cell or non-positive kspace_resolution")
    buf = (c_double * (3 * max(n, 1)))()
    lib.pet_ewald_kvectors_host(h, float(kspace_resolution), buf, n)
    return torch.tensor(list(buf)[: 3 * n], dtype=torch.float64).reshape(n, 3)


def _first_atoms(system_indices: torch.Tensor, n_systems: int) -> List[int]:
    counts = torch.bincount(system_indices.long(), minlength=n_systems).cpu().tolist()
    first = [0]
    for c in counts:
        first.append(first[-1] + int(c))
    return first


class EwaldHip:
    """``pet_ewald_t``: the operator ``q [N, C] -> V [N, C]`` and its adjoints on device tensors."""

    _warns_kset = True  # the k-set warning is the Ewald sum's: a mesh operator walks no k-set
    _entry = "pet_ewald"  # the prefix of this mode's entry points

    def __init__(self, smearing: float = 1.4, kspace_resolution: float = 1.33, cutoff: float = 4.5):
        global _warned_kset
        self.lib = _lib.load()
        self.smearing, self.kspace_resolution, self.cutoff = float(smearing), float(kspace_resolution), float(cutoff)
        self._handle = c_void_p()
        check(self.lib.pet_ewald_create(self.smearing, self.kspace_resolution, self.cutoff, byref(self._handle)))
        t = truncation_factor(self.smearing, self.kspace_resolution)
        if self._warns_kset and t > 1e-7 and not _warned_kset:
            _warned_kset = True
            logging.warning(f"long range: exp(-(smearing 2 pi / kspace_resolution)^2 / 2) = {t:.1e} exceeds 1e-7: the k-space "
                            "sum has not converged inside the k-set, so the result depends on the SHAPE of the k-set (a "
                            "sphere here, the box of a mesh in torch-pme), which is not pinned")
        self.n_systems = -1
        self._workspace: Optional[torch.Tensor] = None  # first order: one buffer that only grows
        self._workspaces: Dict[str, Dict[int, torch.Tensor]] = {}  # second order: by size-query name, then by channel count

    def __del__(self):
        h = getattr(self, "_handle", None)
        try:
            if h is not None and h.value:
                self.lib.pet_ewald_destroy(h)
                self._handle = c_void_p()
        except Exception:
            pass

    @property
    def handle(self) -> c_void_p:
        return self._handle

    def plan(self, cells, pbcs: Sequence[Sequence[bool]], first_atom: Sequence[int]) -> "EwaldHip":
        """Build the per-system k-vector lists (host fp64) for ``cells [S, 3, 3]``, ``pbcs [S][3]`` and the batch layout
        ``first_atom [S + 1]`` (``pet_ewald_plan``). Valid for as long as the cells do not change. Mixed ``pbc`` raises."""
        cells_t = torch.as_tensor(cells).detach().to("cpu", torch.float64).reshape(-1, 3, 3)
        n_sys = int(cells_t.shape[0])
        if len(pbcs) != n_sys or len(first_atom) != n_sys + 1:
            raise PetHipError(f"{n_sys} cells, {len(pbcs)} pbc entries and {len(first_atom)} first_atom entries do not "
                              "describe one batch")
        h_cells = (c_double * (9 * max(n_sys, 1)))(*[float(x) for x in cells_t.reshape(-1).tolist()])
        h_pbc = (c_int32 * (3 * max(n_sys, 1)))(*[int(bool(x)) for p in pbcs for x in p])
        h_first = (c_int64 * (n_sys + 1))(*[int(x) for x in first_atom])
        check(self.lib.pet_ewald_plan(self._handle, h_cells, h_pbc, h_first, n_sys))
        self.n_systems = n_sys
        self._workspace = None
        self._workspaces = {}
        return self

    def num_kvectors(self, system: int) -> int:
        n = int(self.lib.pet_ewald_num_kvectors(self._handle, int(system)))
        if n < 0:
            raise PetHipError("no plan, or no such system")
        return n

    def _ws(self, channels: int, device) -> torch.Tensor:
        nbytes = int(getattr(self.lib, self._entry + "_workspace_bytes")(self._handle, channels))
        if nbytes < 0:
            raise PetHipError(f"{self._entry}_workspace_bytes failed: call plan() first")
        if self._workspace is None or self._workspace.numel() < nbytes or self._workspace.device != device:
            self._workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        return self._workspace

    def _inputs(self, positions, *rows):
        rt._require_cuda(positions, *rows)
        pos = positions.detach().to(torch.float32).contiguous()
        return (pos,) + tuple(r.detach().to(torch.float32).reshape(pos.shape[0], -1).contiguous() for r in rows)

    def potential(self, graph: rt.HipGraph, positions: torch.Tensor, charges: torch.Tensor) -> torch.Tensor:
        """``V [N, C]`` for ``charges [N, C]`` (``pet_ewald_potential``)."""
        pos, q = self._inputs(positions, charges)
        out = torch.empty_like(q)
        ws = self._ws(q.shape[1], q.device)
        check(self.lib.pet_ewald_potential(self._handle, graph.handle, rt._ptr(pos), rt._ptr(q), int(q.shape[1]),
                                           rt._ptr(out), rt._ptr(ws), ws.numel(), rt._stream()))
        return out

    def backward(self, graph: rt.HipGraph, positions: torch.Tensor, charges: torch.Tensor, grad_potential: torch.Tensor,
                 want_cell_grad: bool = False):
        """``(dL/dq [N, C], dL/dR [N, 3])`` and on request ``dL/dcell [S, 3, 3]`` (fixed Cartesian positions) for
        ``dL/dV = grad_potential`` (``pet_ewald_backward``)."""
        pos, q, g = self._inputs(positions, charges, grad_potential)
        gq = torch.empty_like(q)
        gpos = torch.empty_like(pos)
        gcell = torch.empty((graph.n_systems, 3, 3), dtype=torch.float32, device=q.device) if want_cell_grad else None
        ws = self._ws(q.shape[1], q.device)
        check(self.lib.pet_ewald_backward(self._handle, graph.handle, rt._ptr(pos), rt._ptr(q), rt._ptr(g), int(q.shape[1]),
                                          rt._ptr(gq), rt._ptr(gpos), rt._ptr(gcell), rt._ptr(ws), ws.numel(), rt._stream()))
        return (gq, gpos, gcell) if want_cell_grad else (gq, gpos)

    def second(self, graph: rt.HipGraph, positions: torch.Tensor, charges: torch.Tensor, grad_potential: torch.Tensor,
               u_charges: Optional[torch.Tensor] = None, u_positions: Optional[torch.Tensor] = None):
        """The derivative of the adjoint (``pet_ewald_second``): for cotangents ``u_charges [N, C]`` of ``dL/dq`` and
        ``u_positions [N, 3]`` of ``dL/dR`` as :meth:`backward` returns them, the gradient of
        ``<u_charges, dL/dq> + <u_positions, dL/dR>`` with respect to ``(charges, grad_potential, positions)``:
        ``(out_charges [N, C], out_grad_potential [N, C], out_positions [N, 3])``. Either cotangent may be ``None`` (zero; its
        work is skipped), not both. No cell tangent is taken and no cell result returned."""
        return self._second_order("second", graph, positions, charges, grad_potential, (u_charges, u_positions), (True, True, True))

    def second_cell(self, graph: rt.HipGraph, positions: torch.Tensor, charges: torch.Tensor, grad_potential: torch.Tensor,
                    u_charges: Optional[torch.Tensor] = None, u_positions: Optional[torch.Tensor] = None,
                    u_cells: Optional[torch.Tensor] = None, results: Sequence[bool] = (True, True)):
        """:meth:`second` with a cotangent ``u_cells [S, 3, 3]`` of ``dL/dcell`` beside the other two (``pet_ewald_second_cell``;
        DESIGN.md section 23): ``(out_charges, out_grad_potential)``, the gradient of ``<u_charges, dL/dq> + <u_positions, dL/dR>
        + <u_cells, dL/dcell>`` with respect to ``(charges, grad_potential)`` -- the two results that feed parameter gradients.
        Any cotangent may be ``None`` (zero), not all three; rows of ``u_cells`` of open systems are ignored. ``results``: which
        of the two to form (the other comes back ``None``, the one formed has the bits of the full call). The position and
        cell results (mixed and second cell derivatives) are not built."""
        return self._second_order("second_cell", graph, positions, charges, grad_potential, (u_charges, u_positions, u_cells), results)

    def _with_hook(self, workspace: Optional[torch.Tensor], call) -> None:
        """``check(call())`` for an entry point that runs on ``workspace``; :class:`P3MHip` serves its transform hook there."""
        check(call())

    @property
    def _second_workspaces(self) -> Dict[int, torch.Tensor]:
        """The workspaces of :meth:`second` by channel count: its part of the one cache."""
        return self._workspaces.setdefault(self._entry + "_second_workspace_bytes", {})

    def _second_order(self, what: str, graph, positions, charges, grad_potential, cotangents, results):
        """Behind :meth:`second` (``what = "second"``: two cotangents, three results) and :meth:`second_cell` (three and two): the
        cotangents as fp32 device rows, the results asked for, the cached workspace of the entry's size query, the call."""
        cell = what == "second_cell"
        if all(t is None for t in cotangents):
            raise PetHipError("second_cell: u_charges, u_positions and u_cells are all None" if cell
                              else "second: u_charges and u_positions are both None")
        results = tuple(bool(x) for x in results)
        if len(results) != (2 if cell else 3) or not any(results):
            raise PetHipError("second_cell: results names two flags (out_charges, out_grad_potential), at least one set" if cell
                              else "second: results names three flags (out_charges, out_grad_potential, out_positions), at least one set")
        rt._require_cuda(*[t for t in cotangents if t is not None])
        pos, q, g = self._inputs(positions, charges, grad_potential)
        shapes = (q.shape, pos.shape, (graph.n_systems, 3, 3))
        us = [None if t is None else t.detach().to(torch.float32).reshape(shape).contiguous() for t, shape in zip(cotangents, shapes)]
        C = int(q.shape[1])
        entry_name = f"{self._entry}_{what}"
        nbytes = int(getattr(self.lib, entry_name + "_workspace_bytes")(self._handle, C))
        if nbytes < 0:
            raise PetHipError(f"{entry_name}_workspace_bytes failed: call plan() first")
        cache = self._workspaces.setdefault(entry_name + "_workspace_bytes", {})
        ws = cache.get(C)
        if ws is None or ws.numel() < nbytes or ws.device != q.device:
            ws = cache[C] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=q.device)
        outs = tuple(torch.empty_like(t) if want else None for t, want in zip((q, q, pos), results))
        entry = getattr(self.lib, entry_name)
        self._with_hook(ws, lambda: entry(self._handle, graph.handle, rt._ptr(pos), rt._ptr(q), rt._ptr(g), *[rt._ptr(u) for u in us],
                                          C, *[rt._ptr(t) for t in outs], rt._ptr(ws), ws.numel(), rt._stream()))
        return outs


class P3MHip(EwaldHip):
    """The same operator with the reciprocal-space sum on a mesh (a ``pet_ewald_t`` after ``pet_ewald_set_p3m``): ``plan``,
    ``potential`` and ``backward`` as :class:`EwaldHip`, and ``mesh_shape(system)``. One application is
    ``pet_p3m_spread -> torch.fft.rfftn -> pet_p3m_filter -> torch.fft.irfftn -> pet_p3m_finish`` on the current stream; the
    meshes are channel-first ``[C, N_x, N_y, N_z]`` per periodic system, packed in batch order.

    ``second_order=True`` installs the TRANSFORM HOOK (``pet_p3m_set_transform``): a ctypes callback that
    runs the same ``torch.fft`` calls between two offsets of the workspace of whichever entry point is running. That enables
    :meth:`second` (``pet_p3m_second``), torch double backward through a P3M featuriser, and the handle's place in the
    long-range training sweep and Hessian-vector product. Without it all of those raise as before."""

    _warns_kset = False
    _entry = "pet_p3m"

    def __init__(self, smearing: float = 1.4, kspace_resolution: float = 1.33, cutoff: float = 4.5, interpolation_nodes: int = 5,
                 second_order: bool = False):
        self.interpolation_nodes = _check_nodes(interpolation_nodes)
        super().__init__(smearing, kspace_resolution, cutoff)
        check(self.lib.pet_ewald_set_p3m(self._handle, self.interpolation_nodes))
        self._meshes: List[tuple] = []  # (shape, first mesh point, first half-spectrum point) per system with a mesh
        self._mesh_points = self._spec_points = 0
        self.second_order = bool(second_order)
        self.transform_calls = 0  # hook invocations (a batch without a mesh makes none)
        self._hook = self._hook_error = self._hook_workspace = None
        if self.second_order:
            self._install_hook()

    def _install_hook(self) -> None:
        me = weakref.ref(self)  # (the callback must not keep the handle's owner alive)

        def hook(user, inverse, mesh_byte_offset, spectrum_byte_offset, n_channels):
            # ctypes swallows an exception raised here: keep it for _with_hook and tell the C side by the return value
            op = me()
            try:
                op._transform(op._hook_workspace, int(inverse), int(mesh_byte_offset), int(spectrum_byte_offset), int(n_channels))
                return 0
            except BaseException as exc:  # noqa: BLE001
                if op is not None:
                    op._hook_error = exc
                return 1

        self._hook = _lib.P3M_TRANSFORM_FN(hook)  # (kept: the handle holds the raw pointer)
        check(self.lib.pet_p3m_set_transform(self._handle, self._hook, None))

    def _transform(self, ws: Optional[torch.Tensor], inverse: int, mesh_off: int, spec_off: int, C: int) -> None:
        """``rfftn`` (``inverse = 0``) / ``irfftn(norm="forward")`` of every mesh of the plan between the packed mesh buffer at
        byte ``mesh_off`` and the packed half spectrum at byte ``spec_off`` of ``ws`` (uint8), on the current stream, without a
        copy: the calls of :meth:`_mesh_potential`."""
        if ws is None:
            raise PetHipError("the P3M transform hook ran outside an entry point that named its workspace (P3MHip._with_hook)")
        self.transform_calls += 1
        for n, moff, soff in self._meshes:
            m, mh = n[0] * n[1] * n[2], n[0] * n[1] * (n[2] // 2 + 1)
            real = ws[mesh_off + 4 * moff * C:mesh_off + 4 * (moff + m) * C].view(torch.float32).view(C, *n)
            half = ws[spec_off + 8 * soff * C:spec_off + 8 * (soff + mh) * C].view(torch.complex64).view(C, n[0], n[1], n[2] // 2 + 1)
            if inverse:
                torch.fft.irfftn(half, s=n, dim=(1, 2, 3), norm="forward", out=real)
            else:
                torch.fft.rfftn(real, dim=(1, 2, 3), out=half)

    def _with_hook(self, workspace: Optional[torch.Tensor], call) -> None:
        """Run an entry point whose transforms come back through the hook on ``workspace``; an exception raised inside the hook
        is re-raised here, in place of the C side's error that names the hook."""
        self._hook_workspace, self._hook_error = workspace, None
        try:
            rc = call()
        finally:
            self._hook_workspace = None
        err, self._hook_error = self._hook_error, None
        if err is not None:
            raise err
        check(rc)

    def plan(self, cells, pbcs: Sequence[Sequence[bool]], first_atom: Sequence[int]) -> "P3MHip":
        """Mesh descriptors and influence functions for the batch (``pet_ewald_plan`` in P3M mode). Valid while the cells and
        the batch layout do not change. Mixed ``pbc`` and a mesh axis above 512 raise."""
        super().plan(cells, pbcs, first_atom)
        self._meshes = []
        moff = soff = 0
        out = (c_int32 * 3)()
        for s in range(self.n_systems):
            check(self.lib.pet_p3m_mesh_shape(self._handle, s, out))
            n = (int(out[0]), int(out[1]), int(out[2]))
            if n[0] == 0:
                continue
            self._meshes.append((n, moff, soff))
            moff += n[0] * n[1] * n[2]
            soff += n[0] * n[1] * (n[2] // 2 + 1)
        self._mesh_points, self._spec_points = moff, soff
        return self

    def num_kvectors(self, system: int) -> int:
        raise PetHipError("a P3M operator has no k-vector list: see mesh_shape(system)")

    def mesh_shape(self, system: int) -> List[int]:
        """``[N_0, N_1, N_2]`` of a planned system; zeros for a non-periodic or empty one, which has no mesh."""
        out = (c_int32 * 3)()
        check(self.lib.pet_p3m_mesh_shape(self._handle, int(system), out))
        return [int(x) for x in out]

    def second(self, graph: rt.HipGraph, positions: torch.Tensor, charges: torch.Tensor, grad_potential: torch.Tensor,
               u_charges: Optional[torch.Tensor] = None, u_positions: Optional[torch.Tensor] = None,
               results: Sequence[bool] = (True, True, True)):
        """:meth:`EwaldHip.second` through the mesh operator (``pet_p3m_second``), for an operator built with
        ``second_order=True``. ``results``: which of ``(out_charges, out_grad_potential, out_positions)`` to form; the others
        come back ``None`` and the meshes, transforms and launches that serve them alone are skipped (the ones formed have the
        bits of the full call)."""
        if not self.second_order:
            raise PetHipError("second derivatives through P3M are not built on this operator: second_order=True "
                              "(P3MHip(..., second_order=True), LongRangeFeaturizerHip(..., method='p3m', second_order=True)) "
                              "installs the transform hook they need and trains through the mesh operator; method='ewald' "
                              "trains by Ewald summation")
        return self._second_order("second", graph, positions, charges, grad_potential, (u_charges, u_positions), results)

    def second_cell(self, graph: rt.HipGraph, positions: torch.Tensor, charges: torch.Tensor, grad_potential: torch.Tensor,
                    u_charges: Optional[torch.Tensor] = None, u_positions: Optional[torch.Tensor] = None,
                    u_cells: Optional[torch.Tensor] = None, results: Sequence[bool] = (True, True)):
        """:meth:`EwaldHip.second_cell` through the mesh operator (``pet_p3m_second_cell``), for an operator built with
        ``second_order=True``: the filter's cell tangent rides on the transforms of the position tangent, four hook calls per
        result formed."""
        if not self.second_order:
            raise PetHipError("cell tangents through P3M are not built on this operator: second_order=True "
                              "(P3MHip(..., second_order=True)) installs the transform hook they need")
        return super().second_cell(graph, positions, charges, grad_potential, u_charges, u_positions, u_cells, results)

    def _mesh_potential(self, graph, pos, x, ws, keep_spectrum: bool = False):
        """spread -> rfftn -> filter -> irfftn of ``x [N, C]``: the mesh potential (packed, channel-first) and, on request, the
        unfiltered half spectrum. Leaves the weights and bins of ``pos`` in the workspace."""
        C = int(x.shape[1])
        mesh = torch.empty(max(self._mesh_points * C, 1), dtype=torch.float32, device=x.device)
        check(self.lib.pet_p3m_spread(self._handle, graph.handle, rt._ptr(pos), rt._ptr(x), C, rt._ptr(mesh), rt._ptr(ws),
                                      ws.numel(), rt._stream()))
        spec = torch.empty(max(self._spec_points * C, 1), dtype=torch.complex64, device=x.device)
        views = []
        for n, moff, soff in self._meshes:
            m, mh = n[0] * n[1] * n[2], n[0] * n[1] * (n[2] // 2 + 1)
            real = mesh[moff * C:(moff + m) * C].view(C, *n)
            half = spec[soff * C:(soff + mh) * C].view(C, n[0], n[1], n[2] // 2 + 1)
            torch.fft.rfftn(real, dim=(1, 2, 3), out=half)
            views.append((n, real, half))
        raw = spec.clone() if keep_spectrum else None
        check(self.lib.pet_p3m_filter(self._handle, C, rt._ptr(spec), rt._stream()))
        for n, real, half in views:
            torch.fft.irfftn(half, s=n, dim=(1, 2, 3), norm="forward", out=real)
        return mesh, raw

    def _finish(self, graph, pos, x, phi, ws):
        out = torch.empty_like(x)
        check(self.lib.pet_p3m_finish(self._handle, graph.handle, rt._ptr(pos), rt._ptr(x), int(x.shape[1]), rt._ptr(phi),
                                      rt._ptr(out), rt._ptr(ws), ws.numel(), rt._stream()))
        return out

    def potential(self, graph: rt.HipGraph, positions: torch.Tensor, charges: torch.Tensor) -> torch.Tensor:
        """``V [N, C]`` for ``charges [N, C]``."""
        pos, q = self._inputs(positions, charges)
        ws = self._ws(q.shape[1], q.device)
        phi, _ = self._mesh_potential(graph, pos, q, ws)
        return self._finish(graph, pos, q, phi, ws)

    def backward(self, graph: rt.HipGraph, positions: torch.Tensor, charges: torch.Tensor, grad_potential: torch.Tensor,
                 want_cell_grad: bool = False):
        """``(dL/dq [N, C], dL/dR [N, 3])`` and on request ``dL/dcell [S, 3, 3]`` (fixed Cartesian positions) for
        ``dL/dV = grad_potential``: the forward path applied to ``grad_potential`` (the operator is symmetric), then
        ``pet_p3m_backward`` on the two mesh potentials and the two unfiltered spectra."""
        pos, q, g = self._inputs(positions, charges, grad_potential)
        C = int(q.shape[1])
        ws = self._ws(C, q.device)
        phi_q, spec_q = self._mesh_potential(graph, pos, q, ws, keep_spectrum=want_cell_grad)
        phi_g, spec_g = self._mesh_potential(graph, pos, g, ws, keep_spectrum=want_cell_grad)
        gq = self._finish(graph, pos, g, phi_g, ws)
        gpos = torch.empty_like(pos)
        gcell = torch.empty((graph.n_systems, 3, 3), dtype=torch.float32, device=q.device) if want_cell_grad else None
        check(self.lib.pet_p3m_backward(self._handle, graph.handle, rt._ptr(pos), rt._ptr(q), rt._ptr(g), C, rt._ptr(phi_q),
                                        rt._ptr(phi_g), rt._ptr(spec_q), rt._ptr(spec_g), rt._ptr(gpos), rt._ptr(gcell),
                                        rt._ptr(ws), ws.numel(), rt._stream()))
        return (gq, gpos, gcell) if want_cell_grad else (gq, gpos)


_MIXED_SECOND = ("mixed position / cell second derivatives of the long-range operator are not built: the second-order "
                 "operation (pet_ewald_second) takes no cell tangent and returns no cell result (a stress loss needs them); "
                 "differentiate the first-order gradients with respect to charges, dL/dV and positions only, with cells that "
                 "do not require grad")


class _EwaldAdjointFn(torch.autograd.Function):
    """The operator's adjoint as an autograd node of its own: ``forward`` is the first-order ``backward`` call, ``backward`` the
    second-order operation (:meth:`EwaldHip.second`), with respect to charges, positions and the incoming gradient."""

    @staticmethod
    def forward(ctx, charges, positions, cells, grad, ewald, graph):
        ctx.set_materialize_grads(False)
        ctx.ewald, ctx.graph = ewald, graph
        ctx.save_for_backward(charges, positions, grad)
        gq, gpos, gcell = ewald.backward(graph, positions, charges, grad, want_cell_grad=True)
        return gq, gpos, gcell.reshape(cells.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable  # (third derivatives are not built)
    def backward(ctx, u_charges, u_positions, u_cells):
        if u_cells is not None or ctx.needs_input_grad[2]:
            raise PetHipError(_MIXED_SECOND)
        if u_charges is None and u_positions is None:
            return None, None, None, None, None, None
        charges, positions, grad = ctx.saved_tensors
        out_q, out_g, out_r = ctx.ewald.second(ctx.graph, positions, charges, grad, u_charges, u_positions)
        return out_q, out_r, None, out_g, None, None


class _EwaldFn(torch.autograd.Function):
    """The operator as an autograd node over the HIP calls: gradients for charges, positions and cells, and (no cells; P3M
    under ``second_order=True``) their derivatives once more under ``create_graph`` through :class:`_EwaldAdjointFn`."""

    @staticmethod
    def forward(ctx, charges, positions, cells, ewald, graph):
        ctx.ewald, ctx.graph = ewald, graph
        ctx.save_for_backward(charges, positions, cells)
        return ewald.potential(graph, positions, charges)

    @staticmethod
    def backward(ctx, grad):
        charges, positions, cells = ctx.saved_tensors
        gq, gpos, gcell = _EwaldAdjointFn.apply(charges, positions, cells, grad, ctx.ewald, ctx.graph)
        return gq, gpos, gcell, None, None


class LongRangeFeaturizerHip:
    """``LongRangeFeaturizer`` (``utils/long_range.py``) on the device: ``charges_map`` and ``out_projection`` under the
    reference's state-dict keys (fp32 torch ops on the device; there is no TF32 on gfx950) around :class:`EwaldHip` or, with
    ``method="p3m"``, :class:`P3MHip` (``interpolation_nodes`` from the hypers). ``method=None`` follows the hypers and refuses
    ``use_ewald: false``; ``method="ewald"`` is ``p3m_as_ewald=True``."""

    def __init__(self, hypers: dict, device=None, p3m_as_ewald: bool = False, method: Optional[str] = None,
                 second_order: bool = False, cell_tangents: bool = False):
        self.long_range = resolve_hypers(hypers, p3m_as_ewald, method)
        if second_order and method != "p3m":
            raise PetHipError("second_order=True is the switch of the P3M operator (method='p3m'): the Ewald operator has its "
                              f"second derivatives without it, got method={method!r}")
        if cell_tangents and method == "p3m" and not second_order:
            raise PetHipError("cell_tangents=True with method='p3m' needs second_order=True as well: the mesh operator's cell "
                              "tangents run their transforms through the hook that second_order=True installs")
        # the opt-in of the stress term: LongRangeForward.backward_train2(u_cell=...) and
        # LongRangeTrainStep(target_strain_gradients=...) run the cell-tangent sweep; without it they refuse as before
        self.cell_tangents = bool(cell_tangents)
        self.method = method
        self.d = int(hypers["d_node"])
        self.cutoff = float(hypers["cutoff"])
        lr = self.long_range
        # (the attribute keeps its name: whichever operator evaluates the periodic systems)
        self.ewald = (P3MHip(lr["smearing"], lr["kspace_resolution"], self.cutoff, lr["interpolation_nodes"], second_order)
                      if method == "p3m"
                      else EwaldHip(lr["smearing"], lr["kspace_resolution"], self.cutoff))
        dev = torch.device("cpu") if device is None else torch.device(device)
        d = self.d
        self.params: Dict[str, torch.Tensor] = {}
        for name in ("charges_map", "out_projection.0", "out_projection.2"):
            lin = torch.nn.Linear(d, d)
            self.params[name + ".weight"] = lin.weight.detach().to(dev, torch.float32)
            self.params[name + ".bias"] = lin.bias.detach().to(dev, torch.float32)

    def state_dict(self, prefix: str = "long_range_featurizer.") -> Dict[str, torch.Tensor]:
        return {prefix + k: v for k, v in self.params.items()}

    def load_state_dict(self, state: Dict[str, torch.Tensor], prefix: str = "long_range_featurizer.") -> None:
        d = self.d
        dev = next(iter(self.params.values())).device
        for k in list(self.params):
            if prefix + k not in state:
                raise PetHipError(f"the state dict has no '{prefix + k}': not a long-range checkpoint")
            t = state[prefix + k].detach().to(dev, torch.float32).contiguous()
            want = (d, d) if k.endswith("weight") else (d,)
            if tuple(t.shape) != want:
                raise PetHipError(f"'{prefix + k}' has shape {tuple(t.shape)}, expected {want}")
            self.params[k] = t

    @classmethod
    def from_state_dict(cls, hypers: dict, state: Dict[str, torch.Tensor], device=None, p3m_as_ewald: bool = False,
                        prefix: str = "long_range_featurizer.", method: Optional[str] = None,
                        second_order: bool = False, cell_tangents: bool = False) -> "LongRangeFeaturizerHip":
        self = cls(hypers, device, p3m_as_ewald, method, second_order, cell_tangents)
        self.load_state_dict(state, prefix)
        return self

    def bind(self, model: rt.HipModel, prefix: str = "long_range_featurizer.") -> "LongRangeFeaturizerHip":
        """Make ``model``'s parameter table the single source of the six tensors (training: the model holds their storage,
        gradient slots and Adam moments; ``HipModel.load`` uploads them with every other key of a long-range checkpoint).
        ``params`` become copies of the model's and :meth:`refresh` renews them after an optimizer step, so that
        ``state_dict()`` of model and featuriser agree to the bit. A tensor the model was loaded without raises by key."""
        keys = getattr(model, "_ckeys", {})
        for k in self.params:
            if prefix + k not in keys:
                raise PetHipError(f"the model was loaded without '{prefix + k}': load the long-range checkpoint's featuriser "
                                  "tensors with the model (one state dict) to train them")
        self._bound = (model, prefix)
        return self.refresh()

    def refresh(self) -> "LongRangeFeaturizerHip":
        """Copy the six tensors from the bound model (six small device copies); a no-op without :meth:`bind`."""
        bound = getattr(self, "_bound", None)
        if bound is not None:
            model, prefix = bound
            self.params = {k: model.param(prefix + k) for k in self.params}
        return self

    def to(self, device) -> "LongRangeFeaturizerHip":
        self.params = {k: v.to(device) for k, v in self.params.items()}
        return self

    def plan(self, cells, pbcs, first_atom) -> "LongRangeFeaturizerHip":
        self.ewald.plan(cells, pbcs, first_atom)
        return self

    def __call__(self, features: torch.Tensor, positions: torch.Tensor, cells: torch.Tensor, graph: rt.HipGraph):
        """``out_projection(potential(charges_map(features)))`` ``[N, d_node]``, differentiable by torch autograd with
        respect to ``features``, ``positions`` and ``cells``, and with the Ewald operator twice (``create_graph=True``) with
        respect to ``features``, ``positions`` and the six parameter tensors once a caller sets ``requires_grad_`` on them;
        a P3M featuriser without ``second_order=True`` and cells that require grad are refused there."""
        rt._require_cuda(features, positions)
        p = self.params
        q = torch.nn.functional.linear(features, p["charges_map.weight"], p["charges_map.bias"])
        v = _EwaldFn.apply(q, positions, cells, self.ewald, graph)
        hid = torch.nn.functional.silu(torch.nn.functional.linear(v, p["out_projection.0.weight"], p["out_projection.0.bias"]))
        return torch.nn.functional.linear(hid, p["out_projection.2.weight"], p["out_projection.2.bias"])


def energy_and_gradient(model: rt.HipModel, featurizer: LongRangeFeaturizerHip, graph: rt.HipGraph, pbcs, target: str = "energy",
                        want_cell_grad: bool = False, outputs: Sequence[str] = (), replan: bool = True):
    """The whole long-range model on one batch: ``(per-atom energies [N], per-system energies [S], dE/dR [N, 3])`` and, on
    request, ``dE/dcell [S, 3, 3]`` (fixed Cartesian positions) of the summed energy.

    ``features_layers -> featuriser -> (h_l + lr) / sqrt(2) -> predict`` per readout layer, summed; back through
    ``predict_backward``, the featuriser's adjoint (torch autograd over the HIP operator), ``backward_features_layers`` and
    ``backward_geometry``, plus the operator's own position and cell gradients. ``pbcs [S][3]``: a graph does not record
    them. ``replan=False`` reuses the featuriser's plan (fixed-cell MD: the k-vectors depend on the cells alone)."""
    if outputs:
        raise PetHipError(f"auxiliary outputs {list(outputs)} ('feature', last-layer features) of a long-range model are not "
                          "built: the long-range entry point returns energies and their gradients")
    if not bool((model.hypers.get("long_range") or {}).get("enable")):
        raise PetHipError("this model has no long_range.enable: use the ordinary entry points")
    if model.hypers.get("num_neighbors_adaptive"):
        raise PetHipError("long_range together with num_neighbors_adaptive is not served (the adaptive cutoff drops edges "
                          "inside the exclusion radius)")
    if getattr(graph, "_sys", None) is None:
        raise PetHipError("the long-range model needs a HipGraph built from positions (not from batch_data)")
    dev = graph.workspace.device
    if replan or featurizer.ewald.n_systems != graph.n_systems:
        featurizer.plan(graph._cells, pbcs, _first_atoms(graph._sys, graph.n_systems))
    fw = rt.HipForward(model, graph)
    nfs, efs = fw.features_layers()
    n_l = len(nfs)
    leaves = [t.detach().requires_grad_(True) for t in nfs]
    pos = graph._pos.detach().clone().requires_grad_(True)
    cells = graph._cells.detach().clone().requires_grad_(True)
    x = leaves[0]
    for t in leaves[1:]:
        x = x + t
    lr = featurizer(x * (1.0 / math.sqrt(n_l)), pos, cells, graph)
    mixed = [(t + lr) * math.sqrt(0.5) for t in leaves]
    hs = [t.detach().contiguous() for t in mixed]
    atomic = None
    for l in range(n_l):
        a = rt.predict(model, graph, hs[l], efs[l], target, readout_layer=l)
        atomic = a if atomic is None else atomic + a
    if atomic.shape[1] != 1:
        raise PetHipError(f"target '{target}' has {atomic.shape[1]} properties: energies have one")
    atomic = atomic.reshape(-1)
    energies = torch.zeros(graph.n_systems, dtype=torch.float32, device=dev)
    check(model.lib.pet_sum_over_atoms(graph.handle, rt._ptr(atomic), rt._ptr(energies), rt._stream()))
    ones = torch.ones((graph.n_nodes, 1), dtype=torch.float32, device=dev)
    g_h, g_ef, g_fc = [], [], None
    for l in range(n_l):
        a, b, c = rt.predict_backward(model, graph, hs[l], efs[l], ones, target, readout_layer=l)
        g_h.append(a)
        g_ef.append(b)
        g_fc = c if g_fc is None else g_fc + c
    torch.autograd.backward(mixed, g_h)
    geo, gfc = fw.backward_features_layers([t.grad for t in leaves], g_ef)
    out = fw.backward_geometry(geo, gfc + g_fc, want_cell_grad=want_cell_grad)
    if want_cell_grad:
        gpos, gcell = out
        return atomic, energies, gpos + pos.grad, gcell + cells.grad
    return atomic, energies, out + pos.grad


# ---- training on energies and forces, Hessian-vector products --------------------------------------------
def _check_trainable(model, featurizer, what: str) -> None:
    """What the long-range sweeps refuse before anything is launched, by name."""
    hypers = getattr(model, "hypers", None) or {}
    if not bool((hypers.get("long_range") or {}).get("enable")):
        raise PetHipError(f"{what}: this model has no long_range.enable: use the ordinary entry points")
    if hypers.get("num_neighbors_adaptive"):
        raise PetHipError(f"{what}: long_range together with num_neighbors_adaptive is not served (the adaptive cutoff drops "
                          "edges inside the exclusion radius)")
    op = getattr(featurizer, "ewald", None)
    if isinstance(op, P3MHip) and not op.second_order:
        raise PetHipError(f"{what} with a P3M featuriser is not built without second_order=True: second derivatives through "
                          "P3M are not built on an operator without the transform hook. Build the featuriser with "
                          "method='p3m', second_order=True to train through the mesh operator, or with method='ewald' "
                          "(p3m_as_ewald=True) to train by Ewald summation")


class LongRangeForward:
    """What :class:`metatrain_amd.pet.trainer.TrainStep` calls on a ``HipForward``, for a long-range model: ``forward``,
    ``sum_over_atoms``, ``backward(ones, want_cell_grad=True)``, ``backward_train(seeds)``, ``backward_train2(ones, seeds, u)``
    and ``rebind``. The first-order pair is :func:`energy_and_gradient` (``forward`` runs it and keeps dE/dR and dE/dcell of
    the summed energy for ``backward``, whose seeds are therefore ones); the two training calls are
    ``pet_backward_train2_long_range``, which needs no forward. ``pbcs [S][3]``: a graph does not record them."""

    train = True

    def __init__(self, model: rt.HipModel, featurizer: LongRangeFeaturizerHip, graph: rt.HipGraph, pbcs, target: str = "energy"):
        _check_trainable(model, featurizer, "LongRangeForward")
        self.model, self.featurizer, self.graph, self.pbcs, self.target = model, featurizer, graph, pbcs, target
        self.lib = model.lib
        self._first = None
        self._planned_for = None
        self.workspace2: Optional[torch.Tensor] = None

    def rebind(self, graph: rt.HipGraph, pbcs=None) -> "LongRangeForward":
        """Another batch (``pbcs``: its periodicities, unchanged if None); the plan follows at the next call."""
        self.graph = graph
        self.pbcs = self.pbcs if pbcs is None else pbcs
        self._first = None
        return self

    def _plan(self) -> None:
        g = self.graph
        if getattr(g, "_sys", None) is None:
            raise PetHipError("the long-range model needs a HipGraph built from positions (not from batch_data)")
        if self._planned_for is not g or self.featurizer.ewald.n_systems != g.n_systems:
            self.featurizer.plan(g._cells, self.pbcs, _first_atoms(g._sys, g.n_systems))
            self._planned_for = g

    def forward(self, want_features: bool = False, want_atomic: bool = True):
        if want_features or not want_atomic:
            raise PetHipError("LongRangeForward.forward returns the per-atom energies of the fused target only (features and a "
                              "model without a fused target belong to further targets, which the long-range step does not serve)")
        self._plan()
        atomic, _, gpos, gcell = energy_and_gradient(self.model, self.featurizer, self.graph, self.pbcs, self.target,
                                                     want_cell_grad=True, replan=False)
        self._first = (gpos, gcell)
        return atomic

    def sum_over_atoms(self, atomic: torch.Tensor) -> torch.Tensor:
        out = torch.zeros(self.graph.n_systems, dtype=torch.float32, device=atomic.device)
        check(self.lib.pet_sum_over_atoms(self.graph.handle, rt._ptr(atomic), rt._ptr(out), rt._stream()))
        return out

    def backward(self, grad_atomic: torch.Tensor, want_cell_grad: bool = False):
        """dE/dR (and dE/dcell) of the summed energy from the last :meth:`forward`: ``grad_atomic`` is ones by contract."""
        if self._first is None:
            raise PetHipError("LongRangeForward.backward follows forward() on the same graph")
        if grad_atomic is not None and not bool((grad_atomic == 1).all()):
            raise PetHipError("LongRangeForward.backward returns the gradients of the summed energy: grad_atomic must be ones "
                              "(weighted sums: hessian_vector_product / backward_train2 take lambda_atomic)")
        return self._first if want_cell_grad else self._first[0]

    def _sweep(self, lam, nu, u, want_tangent, u_cell=None):
        self._plan()
        g, dev = self.graph, self.graph.workspace.device
        cell = "" if u_cell is None else "_cell"  # the entry with a cell tangent has one argument more
        bytes_name = f"pet_train2_long_range{cell}_workspace_bytes"
        need = int(getattr(self.lib, bytes_name)(self.model.handle, g.handle, self.featurizer.ewald.handle))
        if need < 0:
            raise PetHipError(self.lib.pet_last_error().decode(errors="replace") or f"{bytes_name} failed")
        if self.workspace2 is None or self.workspace2.numel() < need:
            self.workspace2 = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        f32 = lambda t: None if t is None else t.detach().to(dev, torch.float32).contiguous()  # noqa: E731
        lam, nu, u = f32(lam), f32(nu), f32(u)
        pos = g._pos.detach().to(torch.float32).contiguous()
        tan = torch.empty(g.n_nodes, dtype=torch.float32, device=dev) if want_tangent else None
        op, ws = self.featurizer.ewald, self.workspace2
        uc = () if u_cell is None else (rt._ptr(f32(u_cell).reshape(g.n_systems, 3, 3)),)
        entry = getattr(self.lib, f"pet_backward_train2_long_range{cell}")
        op._with_hook(ws, lambda: entry(self.model.handle, g.handle, op.handle, rt._ptr(pos), rt._ptr(ws), ws.numel(), rt._ptr(lam),
                                        rt._ptr(nu), rt._ptr(u), *uc, rt._ptr(tan), rt._stream()))
        return tan

    def backward_train(self, grad_atomic: Optional[torch.Tensor], want_position_grad: bool = False, want_cell_grad: bool = False,
                       seed_features=None):
        """Energy-only loss: ADDS dL/dtheta for ``dL/de = grad_atomic`` to the model's gradient slots, the six featuriser
        tensors' among them."""
        if seed_features is not None:
            raise PetHipError("seed_features (further targets) in the long-range training step are not built")
        if want_position_grad or want_cell_grad:
            raise PetHipError("LongRangeForward.backward_train forms parameter gradients only: dE/dR and dE/dcell come from "
                              "forward() / backward()")
        if grad_atomic is None:
            raise PetHipError("the long-range training step trains the fused energy target: grad_atomic is None")
        self._sweep(None, grad_atomic, None, False)
        return None

    def backward_train2(self, lambda_atomic: torch.Tensor, nu_atomic: Optional[torch.Tensor], u: torch.Tensor,
                        want_tangent: bool = False, u_cell: Optional[torch.Tensor] = None, seed_features=None):
        """Force loss: ADDS d/dtheta ``[sum_i nu_i e_i + <u, dE/dR>]`` (gradient taken with seeds ``lambda_atomic``) to the
        gradient slots; on request returns ``e'_i`` along ``u``. With a featuriser built under ``cell_tangents=True``, ``u_cell
        [S, 3, 3] = dL/d(dE/dcell)`` adds ``<u_cell, dE/dcell>`` (``pet_backward_train2_long_range_cell``; ``u`` may then be
        ``None``)."""
        if u_cell is not None and not getattr(self.featurizer, "cell_tangents", False):
            raise PetHipError("u_cell (a cell tangent: the stress / strain-gradient loss) of a long-range model is not built: "
                              "the operator's second-order entry takes no cell tangent")
        if seed_features is not None:
            raise PetHipError("seed_features (further targets) in the long-range training step are not built")
        return self._sweep(lambda_atomic, nu_atomic, u, want_tangent, u_cell)


from .pet.trainer import TrainStep  # noqa: E402  (trainer imports runtime only: no cycle)


class LongRangeTrainStep(TrainStep):
    """:class:`TrainStep` for a long-range model: energy and position-gradient terms, by ``loss_weights`` (MSE) or the
    ``loss`` hyper (MSE / MAE / Huber), with a :class:`LongRangeForward` in place of the ``HipForward``. ``featurizer`` is
    bound to the model (:meth:`LongRangeFeaturizerHip.bind`): the model's table holds the six tensors, the optimizer step
    updates them there and the featuriser's copies are refreshed after it. With a featuriser built under ``cell_tangents=True``
    the step takes ``target_strain_gradients`` (with ``positions`` and ``cells``) on both loss paths, in ``microbatched`` and in
    ``begin`` / ``end``: the seeds are the base class's (``strain_loss_and_seeds``; ``u_cell = cell @ g``), the sweep is
    ``pet_backward_train2_long_range_cell``. Refused by name: ``target_strain_gradients`` without that opt-in,
    ``extra_targets``, a P3M featuriser built without ``second_order=True``."""

    _serves_long_range = True

    def __init__(self, model: rt.HipModel, featurizer: LongRangeFeaturizerHip, hypers: Optional[dict] = None,
                 steps_per_epoch: int = 1):
        _check_trainable(model, featurizer, "LongRangeTrainStep")
        super().__init__(model, hypers, steps_per_epoch)
        self.featurizer = featurizer.bind(model)

    @staticmethod
    def _refuse(fw, target_strain_gradients, extra_targets) -> None:
        if target_strain_gradients is not None and not getattr(getattr(fw, "featurizer", None), "cell_tangents", False):
            raise PetHipError("target_strain_gradients (the stress loss) of a long-range model are not built: the operator's "
                              "second-order entry takes no cell tangent")
        if extra_targets:
            raise PetHipError(f"extra_targets {sorted(extra_targets)} in the long-range training step are not built")
        if not isinstance(fw, LongRangeForward):
            raise PetHipError("LongRangeTrainStep needs a LongRangeForward (a HipForward leaves the long-range features out)")

    def _accumulate(self, graph, fw, target_energies, n_atoms, target_gradients, target_strain_gradients, positions, cells,
                    share_e, share_f, share_s, extra_targets=None, extra_counts=None):
        self._refuse(fw, target_strain_gradients, extra_targets)
        return super()._accumulate(graph, fw, target_energies, n_atoms, target_gradients, target_strain_gradients, positions,
                                   cells, share_e, share_f, share_s, None, extra_counts)

    def _term_arrays(self, b):
        self._refuse(b["fw"], b.get("target_strain_gradients"), b.get("extra_targets"))
        return super()._term_arrays(b)

    def _finish(self, trained=None):
        norm = super()._finish(trained)
        self.featurizer.refresh()
        return norm


def hessian_vector_product(model: rt.HipModel, featurizer: LongRangeFeaturizerHip, graph: rt.HipGraph, pbcs, u: torch.Tensor,
                           lambda_atomic: Optional[torch.Tensor] = None, want_tangent: bool = False, replan: bool = True,
                           workspace: Optional[torch.Tensor] = None):
    """``H u`` of a long-range model (``pet_hessian_vector_long_range``): ``grad_R sum_i lambda_i e'_i`` ``[N, 3]`` with ``e'_i``
    the derivative of the per-atom energies along ``dR = u [N, 3]`` (``lambda_atomic = None``: ones, the total energy's
    Hessian), then on request ``e'_i [N]``. The model holds the six featuriser tensors (one state dict); ``featurizer``
    supplies the planned operator. Needs no forward pass and touches no gradient slot. No cell direction and no cell result."""
    _check_trainable(model, featurizer, "the long-range Hessian-vector product")
    rt._require_cuda(u)
    if getattr(graph, "_sys", None) is None:
        raise PetHipError("the long-range model needs a HipGraph built from positions (not from batch_data)")
    if replan or featurizer.ewald.n_systems != graph.n_systems:
        featurizer.plan(graph._cells, pbcs, _first_atoms(graph._sys, graph.n_systems))
    dev, n = u.device, graph.n_nodes
    need = int(model.lib.pet_hvp_long_range_workspace_bytes(model.handle, graph.handle, featurizer.ewald.handle))
    if need < 0:
        raise PetHipError(model.lib.pet_last_error().decode(errors="replace") or "pet_hvp_long_range_workspace_bytes failed")
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    uu = u.detach().to(torch.float32).reshape(n, 3).contiguous()
    lam = None if lambda_atomic is None else lambda_atomic.detach().to(dev, torch.float32).reshape(n).contiguous()
    pos = graph._pos.detach().to(torch.float32).contiguous()
    hp = torch.empty((n, 3), dtype=torch.float32, device=dev)
    tan = torch.empty(n, dtype=torch.float32, device=dev) if want_tangent else None
    op = featurizer.ewald
    op._with_hook(workspace, lambda: model.lib.pet_hessian_vector_long_range(
        model.handle, graph.handle, op.handle, rt._ptr(pos), rt._ptr(workspace), workspace.numel(), rt._ptr(lam), rt._ptr(uu),
        rt._ptr(hp), rt._ptr(tan), rt._stream()))
    return (hp, tan) if want_tangent else hp
