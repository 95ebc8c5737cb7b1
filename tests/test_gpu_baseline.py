"""Composition baselines and target scales on the device (``csrc/baseline.hip``, ``metatrain_amd/baseline.py``) against the
fp64 restatement of the reference (``tests/_baseline_oracle.py``).

Shapes: systems of 1, 63, 64, 65 and 300 atoms in one batch (a wave's 64-atom slices; 493 atoms cross a 256-atom chunk),
S in {1, 3, 257} (257 crosses a 256-system chunk), T in {1, 4, 9} with a type absent from the data, P in {1, 3, 5}, fp32 and
fp64 targets, a per-atom target whose NaNs sit in one type, one call against the same data in three calls.

Bounds, with u = 2^-53 (none is tuned to what the kernels give):
  counts, n_atoms, XTX, N     equal to the oracle's.
  XTY, Y2                     |gpu - oracle| <= 2 n u sum|term|, n the number of summed terms: n - 1 additions and one rounding
                              of the term on either side, whatever the order, so the same bound serves the one-call and the
                              three-call form. For Y2 the terms are r^2 of the residual r; the data of the moment tests are
                              dyadic (multiples of 2^-6 below 2^11, weights multiples of 2^-4), so y - sum c w is exact on both
                              sides and the one or two divisions that follow are correctly rounded from the same operands: r is
                              the same number on both sides and the bound is the pure summation bound it is stated as.
  fitted weights              10 cond (accumulator bound / |XTY| + 2u) max|w|, cond of XTX + reg on the types that occur: a type
                              that never occurs is a zero row and column, its equation is reg w = 0 on both sides (asserted:
                              exactly 0) and the rest of the system does not see it. cond < 1e4 is asserted for every case.
  pet_targets_remove          |out - r| <= 2^-24 |r| + 2^-50 (|y| + sum_i |w_i|) / scale against the oracle residual r in fp64.
  gradient arrays             |out - g / scale| <= 2^-24 |g / scale| (fp32 gradients are widened exactly, so the relative
                              2^-24 the issue allows for them is not needed).
"""
import numpy as np
import pytest
import torch

import _baseline_oracle as oracle

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
TOL = 1e-5  # the exported classes' tolerance (tests/test_gpu_zbl.py)
NINE = [1, 3, 6, 7, 8, 9, 14, 16, 17]

# name: sizes, atomic types, the types that occur, target shape, dtype
CASES = {
    "sizes": dict(sizes=[1, 63, 64, 65, 300], types=[1, 6, 7, 8], present=[1, 6, 8], shape=[1], dtype=torch.float64),
    "chunks": dict(sizes=[1 + (k % 3) for k in range(257)], types=NINE, present=[1, 3, 6, 7, 8, 9, 14, 17], shape=[3],
                   dtype=torch.float32),
    "three": dict(sizes=[2, 5, 3], types=[6], present=[6], shape=[5], dtype=torch.float64),
    "one": dict(sizes=[7], types=[1, 6, 7, 8], present=[6], shape=[3, 1], dtype=torch.float32),
    "components": dict(sizes=[2, 3, 4], types=[1, 8], present=[1, 8], shape=[3, 2], dtype=torch.float64),  # components x properties
}


def _width(shape):
    return int(np.prod(shape)) if shape else 1


def make_case(name):
    """numpy only: species with a composition of its own per system (a Dirichlet draw, so that XTX is well conditioned),
    positions on a jittered 1.5 A lattice, dyadic targets."""
    c = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    species, positions = [], []
    for n in c["sizes"]:
        p = rng.dirichlet(np.full(len(c["present"]), 0.7))
        species.append(rng.choice(c["present"], size=n, p=p))
        side = int(np.ceil(n ** (1 / 3)))
        grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
        positions.append(1.5 * grid + rng.uniform(-0.2, 0.2, size=(n, 3)))
    sysidx = np.concatenate([np.full(n, s) for s, n in enumerate(c["sizes"])])
    S, N, P = len(c["sizes"]), int(sysidx.size), _width(c["shape"])
    dyadic = lambda size, scale: np.round(rng.normal(size=size) * scale * 64) / 64  # noqa: E731
    y = dyadic((S, P), 30.0)                       # per structure
    q = dyadic((N, P), 4.0)                        # per atom
    nan_type = c["present"][0]
    q[(np.concatenate(species) == nan_type) & (rng.random(N) < 0.5)] = np.nan  # NaNs confined to one type
    if name == "sizes":
        q[0] = np.nan  # the one-atom system is of the NaN type: a whole system without a value
        species[0][:] = nan_type
    w = np.round(rng.normal(size=(len(c["types"]), P)) * 16) / 16  # weights handed to the moment kernels
    return dict(c, name=name, species=species, positions=positions, all_species=np.concatenate(species), sysidx=sysidx, S=S, N=N,
                P=P, y=y, q=q, w=w, nan_type=nan_type)


def conditioning(case):
    """cond of XTX + reg on the types that occur (the oracle alone; no GPU)."""
    X, _ = oracle.counts_per_structure(case["types"], case["all_species"], case["sysidx"], case["S"])
    seen = [k for k, z in enumerate(case["types"]) if z in case["present"] and X[:, k].any()]
    xtx = (X.T @ X).astype(np.float64)
    reg = 1e-14 * np.mean(np.abs(np.diag(xtx)))
    return float(np.linalg.cond((xtx + reg * np.eye(len(case["types"])))[np.ix_(seen, seen)])), seen


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from metatrain_amd import baseline, data

    class Env:
        dev = torch.device("cuda:0")
        bl = baseline
        _cases = {}

        def systems(self, case, which=None):
            which = range(case["S"]) if which is None else which
            return [(torch.tensor(case["positions"][s], dtype=torch.float32).to(self.dev),
                     torch.tensor(case["species"][s]).to(self.dev), torch.zeros(3, 3), (False, False, False)) for s in which]

        def batch(self, case, which=None, y=None, q=None):
            """collate of the systems ``which`` with the per-structure target "y" and the per-atom target "q"."""
            which = list(range(case["S"])) if which is None else list(which)
            y = case["y"] if y is None else y
            q = case["q"] if q is None else q
            first = np.concatenate([[0], np.cumsum(case["sizes"])])
            shape = tuple(case["shape"])
            targets = {"y": [torch.tensor(y[s].reshape((1,) + shape), dtype=case["dtype"]) for s in which],
                       "q": [torch.tensor(q[first[s]:first[s + 1]].reshape((-1,) + shape), dtype=case["dtype"]) for s in which]}
            return data.collate(self.systems(case, which), 2.0, targets)

        def case(self, name):
            if name not in self._cases:
                c = make_case(name)
                c["batch"] = self.batch(c)
                c["X"], c["n_atoms"] = oracle.counts_per_structure(c["types"], c["all_species"], c["sysidx"], c["S"])
                c["tix"] = oracle.type_indices(c["types"], c["all_species"])
                self._cases[name] = c
            return self._cases[name]

        def specs(self, case):
            return {"y": {"per_atom": False, "shape": case["shape"]}, "q": {"per_atom": True, "shape": case["shape"]}}

    return Env()


def sum_bound(terms, axis):
    """2 n u sum|term| over ``axis``; NaN terms (a NaN accumulator is compared by position) count as 0."""
    t = np.nan_to_num(np.abs(terms))
    return 2.0 * terms.shape[axis] * U * t.sum(axis=axis)


def comp_oracle(case):
    Y, Q = case["y"].reshape(case["S"], -1), case["q"].reshape(case["N"], -1)
    xtx_s, xty_s = oracle.composition_accumulate(False, case["X"], Y)
    xtx_a, xty_a = oracle.composition_accumulate(True, oracle.one_hot(case["types"], case["all_species"]), Q)
    b_s = sum_bound(case["X"][:, :, None] * Y[:, None, :], 0)
    b_a = np.stack([sum_bound(Q[case["tix"] == t], 0) if (case["tix"] == t).any() else np.zeros(case["P"])
                    for t in range(len(case["types"]))])
    return (xtx_s, xty_s, b_s), (xtx_a, xty_a, b_a)


def accumulated(env, case, parts):
    comp = env.bl.CompositionHip(case["types"], env.specs(case))
    for which in parts:
        comp.accumulate(case["batch"] if which is None else env.batch(case, which))
    return comp


def check_composition(case, comp):
    (xtx_s, xty_s, b_s), (xtx_a, xty_a, b_a) = comp_oracle(case)
    assert np.array_equal(comp.XTX["y"]["y"].cpu().numpy(), xtx_s)
    assert np.array_equal(comp.XTX["q"]["q"].cpu().numpy(), xtx_a)  # the diagonal: the types' atom counts
    got = comp.XTY["y"]["y"].cpu().numpy()
    print("XTY per structure: max err / bound", np.max(np.abs(got - xty_s) / np.maximum(b_s, 1e-300)))
    assert np.all(np.abs(got - xty_s) <= b_s)
    got = comp.XTY["q"]["q"].cpu().numpy()
    k = case["types"].index(case["nan_type"])
    assert np.isnan(xty_a[k]).any() and np.array_equal(np.isnan(got), np.isnan(xty_a))  # a NaN stays inside its own type
    ok = ~np.isnan(xty_a)  # (nothing left where the NaN type is the only type)
    assert np.all(np.abs(got - xty_a)[ok] <= b_a[ok])


@pytest.mark.parametrize("name", list(CASES))
def test_species_counts_are_exact(env, name):
    case = env.case(name)
    b = case["batch"]
    tix = env.bl.CompositionHip(case["types"], env.specs(case)).type_index(env.dev)
    counts, n_atoms, flag = env.bl.species_counts(b["species"], b["system_indices"], case["S"], tix, len(case["types"]))
    assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), case["X"])
    assert np.array_equal(n_atoms.cpu().numpy(), case["n_atoms"]) and int(flag) == 0
    absent = [k for k, z in enumerate(case["types"]) if z not in case["present"]]
    assert int(counts[:, absent].abs().sum()) == 0
    again = env.bl.species_counts(b["species"], b["system_indices"], case["S"], tix, len(case["types"]))
    assert torch.equal(again[0], counts) and torch.equal(again[1], n_atoms)


@pytest.mark.parametrize("name", list(CASES))
def test_composition_accumulate_in_one_call(env, name):
    case = env.case(name)
    comp = accumulated(env, case, [None])
    check_composition(case, comp)
    twice = accumulated(env, case, [None])
    for n in ("y", "q"):  # two runs: the same bits (NaN positions included)
        assert torch.equal(twice.XTX[n][n], comp.XTX[n][n])
        assert torch.equal(torch.nan_to_num(twice.XTY[n][n], nan=12345.0), torch.nan_to_num(comp.XTY[n][n], nan=12345.0))


@pytest.mark.parametrize("name", ["sizes", "chunks", "three", "components"])
def test_composition_accumulate_in_three_calls(env, name):
    case = env.case(name)
    cut = [0, case["S"] // 3, max(2 * case["S"] // 3, case["S"] // 3 + 1), case["S"]]
    comp = accumulated(env, case, [range(cut[k], cut[k + 1]) for k in range(3)])
    check_composition(case, comp)  # += across calls, the same bound


@pytest.mark.parametrize("name", list(CASES))
def test_fitted_weights_against_the_oracle_solve(env, name):
    case = env.case(name)
    cond, seen = conditioning(case)
    assert cond < 1e4, cond
    # a target the composition explains (plus noise), so that the fit is of something: y = X w0 + noise
    rng = np.random.default_rng(5)
    w0 = -rng.uniform(10.0, 2000.0, size=(len(case["types"]), case["P"]))
    y = case["X"] @ w0 + rng.normal(size=(case["S"], case["P"]))
    if case["dtype"] == torch.float32:
        y = y.astype(np.float32).astype(np.float64)
    comp = env.bl.CompositionHip(case["types"], {"y": {"per_atom": False, "shape": case["shape"]}})
    comp.accumulate(env.batch(case, y=y.reshape((case["S"],) + tuple(case["shape"]))), names=["y"])
    comp.fit()
    xtx, xty = oracle.composition_accumulate(False, case["X"], y)
    want = oracle.composition_fit(case["types"], False, xtx, xty)
    got = comp.weights("y").numpy()
    xty_bound = sum_bound(case["X"][:, :, None] * y[:, None, :], 0)
    assert np.all(np.abs(comp.XTY["y"]["y"].cpu().numpy() - xty) <= xty_bound)  # XTY again, on numbers that are not dyadic
    acc = xty_bound.max() / np.abs(xty).max()
    bound = 10 * cond * (acc + 2 * U) * np.abs(want).max()
    print(f"{name}: cond {cond:.3g}, weights max err {np.abs(got - want).max():.3g}, bound {bound:.3g}")
    assert np.abs(got - want).max() <= bound
    for k in range(len(case["types"])):
        if k not in seen:
            assert np.all(got[k] == 0.0) and np.all(want[k] == 0.0)  # a type never seen: exactly 0


@pytest.mark.parametrize("name", list(CASES))
def test_target_moments(env, name):
    """N and Y2 of the residual (composition weights ``w`` removed, per-structure values divided by the atom count), summed
    over everything and, after the fitted per-target scale is divided out, per property."""
    case = env.case(name)
    T, P, S = len(case["types"]), case["P"], case["S"]
    nprop = case["shape"][-1]
    comp = env.bl.CompositionHip(case["types"], env.specs(case))
    comp._weights = {"y": {"y": torch.tensor(case["w"])}, "q": {"q": torch.tensor(case["w"])}}  # as if fitted

    def run(per_structure_targets=(), with_comp=True):
        sc = env.bl.ScalerHip(case["types"], {"y": {"per_atom": False, "shape": case["shape"]},
                                              "q": {"per_atom": True, "shape": [1]}} if P == 1 else
                              {"y": {"per_atom": False, "shape": case["shape"]}}, per_structure_targets)
        sc.accumulate(case["batch"], composition=comp if with_comp else None)
        return sc

    for pst, with_comp in (((), True), (("y",), True), ((), False)):
        sc = run(pst, with_comp)
        r = oracle.residual(False, case["y"].reshape(S, P), case["w"] if with_comp else None, case["X"], case["n_atoms"],
                            divide=not pst)
        n, y2 = oracle.n_and_y2(False, r, False)
        assert int(sc.N["y"][0]) == int(n[0, 0]) == S * P
        err, bound = abs(float(sc.Y2["y"][0]) - y2[0, 0]), 2 * r.size * U * np.sum(r * r)
        print(f"{name} Y2 (per_structure_targets={pst}, composition={with_comp}): err {err:.3g} bound {bound:.3g}")
        assert err <= bound
        assert torch.equal(run(pst, with_comp).Y2["y"], sc.Y2["y"])  # two runs: the same bits
    if P == 1:  # a per-atom scalar: one row per type, NaNs out of N
        sc = run()
        r = oracle.residual(True, case["q"].reshape(case["N"], 1), case["w"], oracle.one_hot(case["types"], case["all_species"]))
        n, y2 = oracle.n_and_y2(True, r, False, case["tix"], T)
        assert np.array_equal(sc.N["q"].cpu().numpy(), n[:, 0]) and n[:, 0].sum() < case["N"]
        for t in range(T):
            rt_ = np.nan_to_num(r[case["tix"] == t])
            assert abs(float(sc.Y2["q"][t]) - y2[t, 0]) <= 2 * max(rt_.size, 1) * U * np.sum(rt_ * rt_)
    if nprop > 1:  # per property, on top of the per-target scale (accumulate_per_property)
        sc = run()
        sc.fit()
        sc.accumulate_per_property(case["batch"], composition=comp)
        sc.fit_per_property()
        r = oracle.residual(False, case["y"].reshape((S,) + tuple(case["shape"])), case["w"].reshape((T,) + tuple(case["shape"])),
                            case["X"], case["n_atoms"])
        n0, y20 = oracle.n_and_y2(False, r, False)
        scale = oracle.scaler_fit(n0, y20)[0, 0]
        assert abs(sc.scale("y") - scale) <= (r.size + 4) * U * scale  # Y2 to 2 n u relatively, halved by the root; N equal
        rs = oracle.remove_scale(False, r, [sc.scale("y")])  # the product's own scale: the same operand on both sides
        n, y2 = oracle.n_and_y2(False, rs, True)
        assert np.array_equal(sc.per_property_N["y"]["y"].cpu().numpy(), n)
        terms = (rs * rs).reshape(-1, nprop)
        assert np.all(np.abs(sc.per_property_Y2["y"]["y"].cpu().numpy() - y2) <= sum_bound(terms, 0)[None, :])
        want = oracle.scaler_fit(n, y2)[0]
        assert np.allclose(sc.property_scales("y")["y"].numpy(), want, rtol=1e-12, atol=0)
        assert np.allclose(sc.full_scales("y")["y"].numpy(), oracle.full_scales(sc.scale("y"), want), rtol=1e-12, atol=0)


def remove_bound(r, y, w_sum, scale):
    return 2.0 ** -24 * np.abs(r) + 2.0 ** -50 * (np.abs(y) + w_sum) / scale


@pytest.mark.parametrize("name", list(CASES))
def test_targets_remove(env, name):
    """(y - baseline) / scale for the per-structure and the per-atom target of every case, real (not dyadic) numbers."""
    case = env.case(name)
    T, P, S, N = len(case["types"]), case["P"], case["S"], case["N"]
    rng = np.random.default_rng(9)
    w = -rng.uniform(10.0, 2000.0, size=(T, P))
    f32 = case["dtype"] == torch.float32
    cast = (lambda a: a.astype(np.float32).astype(np.float64)) if f32 else (lambda a: a)
    y = cast(case["X"] @ w + rng.normal(size=(S, P)))
    q = cast(w[case["tix"]] + rng.normal(size=(N, P)))
    q[np.isnan(case["q"]).reshape(N, P)] = np.nan
    shape = tuple(case["shape"])
    batch = env.batch(case, y=y.reshape((S,) + shape), q=q.reshape((N,) + shape))
    comp = env.bl.CompositionHip(case["types"], env.specs(case))
    comp._weights = {"y": {"y": torch.tensor(w)}, "q": {"q": torch.tensor(w)}}
    sc = env.bl.ScalerHip(case["types"], {"y": {"per_atom": False, "shape": case["shape"]}} if P > 1 else
                          {"y": {"per_atom": False, "shape": [1]}, "q": {"per_atom": True, "shape": [1]}})
    sc._scales = {"y": torch.tensor([0.37], dtype=torch.float64), "q": torch.tensor(rng.uniform(0.5, 3.0, size=T))}
    sc._scales = {k: v for k, v in sc._scales.items() if k in sc.targets}
    sc._property_scales = {n: {n: torch.ones(case["shape"][-1], dtype=torch.float64)} for n in sc.multi_property}
    tr = env.bl.TargetTransform(comp, sc)
    out = tr(batch, {"extra": ["y", "q"]})
    got_y = out["extra_targets"]["y"]["values"]
    assert got_y.dtype == torch.float32 and tuple(got_y.shape) == (S,) + shape
    r = oracle.remove_scale(False, oracle.residual(False, y, w, case["X"], divide=False), [0.37])
    bound = remove_bound(r, y, case["X"] @ np.abs(w), 0.37)
    err = np.abs(got_y.cpu().numpy().reshape(S, P).astype(np.float64) - r)
    print(f"{name} remove per structure: max err / bound {np.max(err / bound):.3g}")
    assert np.all(err <= bound)
    got_q = out["extra_targets"]["q"]["values"].cpu().numpy().reshape(N, P).astype(np.float64)
    s_q = sc._scales["q"].numpy() if "q" in sc.targets else np.ones(T)
    rq = oracle.remove_scale(True, oracle.residual(True, q, w, oracle.one_hot(case["types"], case["all_species"])), s_q, case["tix"])
    assert np.array_equal(np.isnan(got_q), np.isnan(rq)) and np.isnan(rq).any()  # NaN stays NaN, and only there
    ok = ~np.isnan(rq)
    bq = remove_bound(rq, q, np.abs(w)[case["tix"]], s_q[case["tix"]][:, None])
    assert np.all(np.abs(got_q - rq)[ok] <= bq[ok])
    assert torch.equal(out["n_atoms"].cpu(), torch.tensor(case["n_atoms"], dtype=torch.float32))
    again = tr(batch, {"extra": ["y", "q"]})  # two runs: the same bits
    assert torch.equal(again["extra_targets"]["y"]["values"], got_y)
    assert torch.equal(torch.nan_to_num(again["extra_targets"]["q"]["values"]), torch.nan_to_num(out["extra_targets"]["q"]["values"]))
    assert batch["y"].dtype == case["dtype"] and got_y.data_ptr() != batch["y"].data_ptr()  # out of place


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.float64])
def test_raw_dft_energies_and_their_gradients(env, grad_dtype):
    """The case the fp64 path is for: energies near -1e5 eV whose residual after the baseline is near 1e-2 eV.

    What rounding y to fp32 FIRST would cost: 2^16 <= 1e5 < 2^17, so fp32 spaces such numbers 2^(16-23) = 2^-7 = 7.8e-3
    apart and rounds by up to 3.9e-3 (a quarter of that, 2e-3, on average) -- 20 to 40 % of the 1e-2 residual itself. The
    bound here is 2^-24 x 1e-2 + 2^-50 x (1e5 + 1e5) / scale = 6e-10 + 1.8e-10 / scale, i.e. about 8e-10 at scale 1: the
    fp32-first error of 2e-3 misses it by more than SIX orders of magnitude (by two orders it would miss even a bound a
    thousand times as wide). The control at the end forms that fp32-first version and checks that it does miss."""
    case = env.case("sizes")
    rng = np.random.default_rng(21)
    S, N, T = case["S"], case["N"], 4
    w = np.array([[-16.5], [-1030.1], [-1485.3], [-2041.7]]) * rng.uniform(0.9, 1.1, size=(T, 1))
    y = case["X"] @ w + 1e-2 * rng.normal(size=(S, 1))  # the 300-atom system: about -3e5 eV
    assert np.abs(y).max() > 1e5 and np.abs(y - case["X"] @ w).max() < 0.1
    grads = rng.normal(size=(N, 3))
    strain = rng.normal(size=(S, 3, 3))
    if grad_dtype == torch.float32:
        grads, strain = grads.astype(np.float32).astype(np.float64), strain.astype(np.float32).astype(np.float64)
    batch = env.batch(case, y=y.reshape(S, 1))
    batch["dE_dR"] = torch.tensor(grads, dtype=grad_dtype).to(env.dev)
    batch["dE_deps"] = torch.tensor(strain, dtype=grad_dtype).to(env.dev)
    spec = {"y": {"per_atom": False, "shape": [1]}}
    comp, sc = env.bl.CompositionHip(case["types"], spec), env.bl.ScalerHip(case["types"], spec)
    comp._weights = {"y": {"y": torch.tensor(w)}}
    for scale in (1.0, 0.0123):
        sc._scales = {"y": torch.tensor([scale], dtype=torch.float64)}
        out = env.bl.TargetTransform(comp, sc)(batch, {"energies": "y", "gradients": "dE_dR", "strain_gradients": "dE_deps"})
        r = oracle.remove_scale(False, oracle.residual(False, y, w, case["X"], divide=False), [scale])[:, 0]
        bound = remove_bound(r, y[:, 0], (case["X"] @ np.abs(w))[:, 0], scale)
        got = out["target_energies"]
        assert got.dtype == torch.float32 and tuple(got.shape) == (S,)
        err = np.abs(got.cpu().numpy().astype(np.float64) - r)
        print(f"raw energies, scale {scale}: max err / bound {np.max(err / bound):.3g}; residuals {np.abs(r * scale).max():.3g}")
        assert np.all(err <= bound)
        for key, g in (("target_gradients", grads), ("target_strain_gradients", strain)):
            assert out[key].dtype == torch.float32 and tuple(out[key].shape) == g.shape
            assert np.all(np.abs(out[key].cpu().numpy().astype(np.float64) - g / scale) <= 2.0 ** -24 * np.abs(g / scale))
        fp32_first = (y[:, 0].astype(np.float32).astype(np.float64) - (case["X"] @ w)[:, 0]) / scale
        big = np.abs(y[:, 0]) > 6e4
        assert np.max(np.abs(fp32_first - r)[big] / bound[big]) > 100.0  # the control: fp32 first misses, by far


def test_unexpected_species_and_cpu_tensors_raise(env):
    from metatrain_amd._lib import PetHipError

    case = env.case("sizes")
    spec = {"y": {"per_atom": False, "shape": case["shape"]}}
    comp, sc = env.bl.CompositionHip([1, 8], spec), env.bl.ScalerHip([1, 8], spec)  # carbon is not a model type
    with pytest.raises(PetHipError, match="unexpected atom types.*found: \\[1, 6, 8\\]"):
        comp.accumulate(case["batch"])
    assert int(comp.XTX["y"]["y"].abs().sum()) == 0  # a refused batch leaves nothing behind
    with pytest.raises(PetHipError, match="unexpected atom types"):
        sc.accumulate(case["batch"])
    sc._scales = {"y": torch.ones(1, dtype=torch.float64)}
    with pytest.raises(PetHipError, match="unexpected atom types"):
        env.bl.TargetTransform(None, sc)(case["batch"], {"extra": ["y"]})
    cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in case["batch"].items()}
    for call in (lambda: env.bl.CompositionHip([1, 6, 8], spec).accumulate(cpu),
                 lambda: env.bl.ScalerHip([1, 6, 8], spec).accumulate(cpu)):
        with pytest.raises(PetHipError, match="MI355X only"):
            call()


@pytest.fixture(scope="module")
def two_systems(env):
    """Two small systems of H, C, O with raw fp64 energies, dE/dR targets, a fitted composition model and scaler."""
    rng = np.random.default_rng(33)
    types = [1, 6, 8]
    species = [np.array([6, 1, 1, 1, 1, 8]), np.array([8, 1, 1, 6, 6, 1, 1, 1])]
    positions = [rng.uniform(0.0, 1.0, size=(len(z), 3)) * 0.3 + 1.1 * np.stack(np.unravel_index(np.arange(len(z)), (2, 2, 2)), -1)
                 for z in species]
    case = dict(sizes=[6, 8], types=types, species=species, positions=positions, S=2, shape=[1], dtype=torch.float64)
    X, n_atoms = oracle.counts_per_structure(types, np.concatenate(species), np.repeat([0, 1], [6, 8]), 2)
    w = np.array([[-13.7], [-1029.4], [-2042.9]])
    y = X @ w + np.array([[0.8], [-1.3]])
    grads = rng.normal(size=(14, 3))
    batch = env.batch(case, y=y, q=np.zeros((14, 1)))
    batch["dE_dR"] = torch.tensor(grads).to(env.dev)
    spec = {"y": {"per_atom": False, "shape": [1]}}
    comp, sc = env.bl.CompositionHip(types, spec), env.bl.ScalerHip(types, spec)
    comp._weights = {"y": {"y": torch.tensor(w)}}
    sc.accumulate(batch, composition=comp, names=["y"])
    sc.fit()
    return dict(types=types, batch=batch, X=X, n_atoms=n_atoms, w=w, y=y, grads=grads, comp=comp, sc=sc)


def test_exported_model_applies_what_the_transform_removes(env, two_systems):
    """``ExportedEnergyModel(core, scale, table)`` returns scale x core + sum_i w[Z_i]: removal and re-application use one
    convention."""
    from metatrain_amd.pet import default_hypers, script
    from metatrain_amd.synthetic import synthetic_params

    t = two_systems
    hypers = default_hypers()
    params = synthetic_params(hypers, t["types"], {"energy": 1}, 0, torch.float32)
    scale, table = t["sc"].scale("y"), t["comp"].table("y")
    assert isinstance(scale, float) and 0.0 < scale < 10.0
    b = t["batch"]
    args = (b["positions"], b["cells"], b["centers"], b["neighbors"], b["cell_shifts"], b["species"], b["system_indices"])
    core = script.ExportedEnergyModel(script.make_core(hypers, t["types"], params, "energy")).to(env.dev)
    full = script.ExportedEnergyModel(script.make_core(hypers, t["types"], params, "energy"), scale, table).to(env.dev)
    e0, f0, _, a0 = core(*args)
    e1, f1, _, a1 = full(*args)
    want = scale * e0.cpu().double().numpy() + (t["X"] @ t["w"])[:, 0]
    assert np.max(np.abs(e1.cpu().double().numpy() - want)) / np.max(np.abs(want)) < TOL
    assert np.max(np.abs(f1.cpu().double().numpy() - scale * f0.cpu().double().numpy())) <= TOL * np.max(np.abs(scale * f0.cpu().numpy()))
    # and the round trip: what the transform takes out of a target, the exported model puts back
    out = env.bl.TargetTransform(t["comp"], t["sc"])(b, {"energies": "y"})
    back = scale * out["target_energies"].cpu().double().numpy() + (t["X"] @ t["w"])[:, 0]
    assert np.max(np.abs(back - t["y"][:, 0])) <= 2.0 ** -23 * np.max(np.abs(t["y"] - t["X"] @ t["w"])) + 2.0 ** -48 * np.max(np.abs(t["y"]))


def test_train_step_on_transformed_targets_matches_the_oracle_residuals(env, two_systems):
    """One ``TrainStep`` on ``TargetTransform``'s output against one on the oracle's fp64 residuals rounded to fp32.

    Tolerance. L = w_e mean_s ((E_s - t_s) / n_s)^2 + w_f mean (g - t_g)^2. For targets that differ by dt, dt_g, the
    gradient of L and Cauchy-Schwarz give |dL| <= 2 sqrt(L_e) sqrt(w_e mean (dt / n)^2) + w_e mean (dt / n)^2, likewise for
    the force term, and L_e, L_f <= L. The loss itself is evaluated in fp32: a mean of S + 3 N squares, each a few
    roundings, so 16 x 2^-24 L is added for the two evaluations. dt and dt_g are measured from the two target tensors."""
    from metatrain_amd import data
    from metatrain_amd.pet import default_hypers
    from metatrain_amd.pet.trainer import TrainStep
    from metatrain_amd.synthetic import synthetic_params

    t = two_systems
    hypers = default_hypers()
    params = {k: v.to(env.dev) for k, v in synthetic_params(hypers, t["types"], {"energy": 1}, 0, torch.float32).items()}
    scale = t["sc"].scale("y")
    out = env.bl.TargetTransform(t["comp"], t["sc"])(t["batch"], {"energies": "y", "gradients": "dE_dR"})
    r_e = oracle.remove_scale(False, oracle.residual(False, t["y"], t["w"], t["X"], divide=False), [scale])[:, 0]
    r_g = t["grads"] / scale
    hand_e = torch.tensor(r_e, dtype=torch.float32).to(env.dev)
    hand_g = torch.tensor(r_g, dtype=torch.float32).to(env.dev)

    def step(te, tg):
        from metatrain_amd import runtime as rt

        model = rt.HipModel(hypers, t["types"])
        model.load(params, "energy")
        g = data.graph_of(model, t["batch"])
        ts = TrainStep(model, {"learning_rate": 1e-3, "warmup_fraction": 0.0, "num_epochs": 10**9})
        res = ts(g, rt.HipForward(model, g, train=True), te, out["n_atoms"], tg)
        return float(res["loss"]), ts.hypers["loss_weights"]

    loss_a, lw = step(out["target_energies"], out["target_gradients"])
    loss_b, _ = step(hand_e, hand_g)
    n = torch.tensor(t["n_atoms"], dtype=torch.float64)
    dt = (out["target_energies"].cpu().double() - hand_e.cpu().double()) / n
    dg = out["target_gradients"].cpu().double() - hand_g.cpu().double()
    me, mf = lw["energy"] * float((dt * dt).mean()), lw["forces"] * float((dg * dg).mean())
    big = max(loss_a, loss_b)
    tol = 2 * np.sqrt(big) * (np.sqrt(me) + np.sqrt(mf)) + me + mf + 16 * 2.0 ** -24 * big
    print(f"losses {loss_a:.9g} {loss_b:.9g}, |difference| {abs(loss_a - loss_b):.3g}, tolerance {tol:.3g}")
    assert loss_a > 0 and abs(loss_a - loss_b) <= tol


def test_transform_with_zbl_follows_the_reference_order(env, two_systems):
    """composition, then ZBL, then the scale: against the composition removed by the oracle in fp64 and
    ``ZBLHip.remove_from_targets`` applied by hand. Both sides round the composition-free energies to fp32 (what the ZBL
    energies are) and divide once: 4 x 2^-24 of the magnitudes involved covers the roundings that may differ."""
    from metatrain_amd._lib import PetHipError
    from metatrain_amd.zbl import ZBLHip

    t = two_systems
    b = t["batch"]
    z = ZBLHip(t["types"])
    spec = {"y": {"per_atom": False, "shape": [1]}}
    sc = env.bl.ScalerHip(t["types"], spec)
    ze, zg, _ = z.remove_from_targets(b, b["positions"], b["cells"], torch.zeros(2, device=env.dev),
                                      torch.zeros((14, 3), device=env.dev))
    zbl_e, zbl_g = -ze.cpu().double().numpy(), -zg.cpu().double().numpy()
    no_comp = oracle.residual(False, t["y"], t["w"], t["X"], divide=False)[:, 0]
    pre = dict(b)
    pre["y"] = torch.tensor(no_comp - zbl_e).to(env.dev)
    sc.accumulate(pre, composition=None, zbl_removed=True, names=["y"])
    sc.fit()
    with pytest.raises(PetHipError, match="the other way"):
        env.bl.TargetTransform(t["comp"], sc)  # fitted with ZBL removed, set up without
    out = env.bl.TargetTransform(t["comp"], sc, zbl=z)(b, {"energies": "y", "gradients": "dE_dR"})
    scale = sc.scale("y")
    he, hg, _ = z.remove_from_targets(b, b["positions"], b["cells"], torch.tensor(no_comp, dtype=torch.float32).to(env.dev),
                                      b["dE_dR"])
    hand_e, hand_g = he.cpu().double().numpy() / scale, hg.cpu().double().numpy() / scale
    tol_e = 4 * 2.0 ** -24 * (np.abs(no_comp) + np.abs(zbl_e)) / scale
    tol_g = 4 * 2.0 ** -24 * (np.abs(t["grads"]) + np.abs(zbl_g)) / scale
    assert np.all(np.abs(out["target_energies"].cpu().double().numpy() - hand_e) <= tol_e)
    assert np.all(np.abs(out["target_gradients"].cpu().double().numpy() - hand_g) <= tol_g)
    assert np.abs(zbl_e).max() > 1e-3  # the ZBL term is there


def test_target_of_two_blocks(env):
    """A per-structure target given as ``{block: tensor}``: N and Y2 pooled over the blocks (``accumulate`` :417-429), per-block
    per-property scales on top, and the transform's ``extra_targets`` entry in the form ``TrainStep`` takes."""
    case = env.case("components")
    S, T = case["S"], len(case["types"])
    rng = np.random.default_rng(8)
    shapes = {"a": [3, 2], "b": [4]}
    vals = {b: np.round(rng.normal(size=(S,) + tuple(s)) * 8 * 64) / 64 for b, s in shapes.items()}  # dyadic, as above
    batch = dict(case["batch"])
    batch["nc"] = {b: torch.tensor(v).to(env.dev) for b, v in vals.items()}
    spec = {"nc": {"per_atom": False, "shape": shapes}}
    sc = env.bl.ScalerHip(case["types"], spec)
    sc.accumulate(batch, names=["nc"])
    r = {b: oracle.residual(False, v, None, case["X"], case["n_atoms"]) for b, v in vals.items()}
    moments = [oracle.n_and_y2(False, r[b], False) for b in shapes]
    n, y2 = sum(m[0][0, 0] for m in moments), sum(m[1][0, 0] for m in moments)
    terms = np.concatenate([(r[b] * r[b]).reshape(-1) for b in shapes])
    assert int(sc.N["nc"][0]) == n == terms.size
    assert abs(float(sc.Y2["nc"][0]) - y2) <= 2 * terms.size * U * terms.sum()
    sc.fit()
    sc.accumulate_per_property(batch)
    sc.fit_per_property()
    pp = sc.property_scales("nc")
    for b, s in shapes.items():
        rs = oracle.remove_scale(False, r[b], [sc.scale("nc")])
        nb, y2b = oracle.n_and_y2(False, rs, True)
        assert np.array_equal(sc.per_property_N["nc"][b].cpu().numpy(), nb)
        assert np.all(np.abs(sc.per_property_Y2["nc"][b].cpu().numpy() - y2b) <= sum_bound((rs * rs).reshape(-1, s[-1]), 0)[None, :])
        assert np.allclose(pp[b].numpy(), oracle.scaler_fit(nb, y2b)[0], rtol=1e-12, atol=0)
    out = env.bl.TargetTransform(None, sc)(batch, {"extra": ["nc"]})["extra_targets"]["nc"]
    assert out["per_atom"] is False and set(out["values"]) == {"a", "b"} and set(out["scales"]) == {"a", "b"}
    for b, v in vals.items():
        want = v / sc.scale("nc")
        got = out["values"][b]
        assert got.dtype == torch.float32 and tuple(got.shape) == v.shape
        assert np.all(np.abs(got.cpu().numpy().astype(np.float64) - want) <= remove_bound(want, v, 0.0, sc.scale("nc")))
        assert torch.equal(out["scales"][b], pp[b])
