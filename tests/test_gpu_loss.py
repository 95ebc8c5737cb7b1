"""GPU tests of ``csrc/loss.hip`` through ``metatrain_amd.loss.PointwiseLoss`` against the fp64 oracle ``_loss_oracle.py``
(torch's MSELoss / L1Loss / HuberLoss after the reference's flatten - mask - drop-NaN, seeds from ``torch.autograd.grad``).

Data. Every operand is dyadic, so the residual ``d = p rs cs - t rs`` is exact on both sides and never within rounding of
a kink: ``|d|`` is a multiple of 2^-4 in [2^-4, 2^3] other than the two deltas under test (0.25 and 1.0), with exact zeros
and exact +-delta placed on purpose at valid entries (there both sides follow the table of ``include/pet_hip.h``; torch's
agreement on the host is asserted in ``test_loss_cpu.py``). About 30 % of the targets are NaN.

Bounds, with u = 2^-53 and n the number of valid entries: counts equal; loss, sum d^2 and sum |d| within ``2 n u sum|term|``
(two summation orders of n non-negative terms, each within ``n u sum`` of the exact sum to first order); seeds within
``2^-24 |ref| + 2^-50 |ref|`` (one rounding to fp32 of a value a few fp64 roundings from the oracle's); seeds at invalid
entries exactly 0."""
import numpy as np
import pytest
import torch

import _loss_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
DELTAS = (0.25, 1.0)
ROWS = (0, 1, 255, 256, 257, 513)   # an empty term, both sides of one and of two chunk boundaries (256 rows per chunk)
WIDTHS = (1, 3, 5, 9)               # 5: no power of two; 9 with three column scales: properties innermost
N_CS = {1: 1, 3: 3, 5: 5, 9: 3}
KINDS = (("mse", 1.0), ("mae", 1.0), ("huber", 0.25), ("huber", 1.0))


def make_case(rows, width, seed, rs_on=False, cs_on=False, mask_on=False, nan_fraction=0.3):
    """fp32 ``p, t [rows, width]`` (NaN targets included), fp64 ``rs [rows]``, ``cs [N_CS[width]]``, boolean ``mask`` (or
    None each) with the exact residuals described in the module docstring."""
    gen = torch.Generator().manual_seed(seed)
    n = rows * width
    allowed = torch.tensor([m for m in range(1, 129) if m / 16.0 not in DELTAS], dtype=torch.float64) / 16.0
    d = allowed[torch.randint(len(allowed), (n,), generator=gen)] * (torch.randint(2, (n,), generator=gen) * 2.0 - 1.0)
    placed = [0.0, 0.0, 0.25, -0.25, 1.0, -1.0][:n]
    d[:len(placed)] = torch.tensor(placed, dtype=torch.float64)
    d = d.reshape(rows, width)
    rs = 2.0 ** -torch.randint(0, 3, (rows,), generator=gen).double() if rs_on else None
    cs = 2.0 ** (torch.randint(0, 3, (N_CS[width],), generator=gen).double() - 1.0) if cs_on else None
    t = (torch.randint(-32, 33, (rows, width), generator=gen) / 8.0).double()
    rs_full = rs[:, None] if rs_on else torch.ones(rows, 1, dtype=torch.float64)
    cs_full = cs.repeat(width // N_CS[width])[None, :] if cs_on else torch.ones(1, width, dtype=torch.float64)
    p = (d / rs_full + t) / cs_full          # p rs cs - t rs = d, every step exact in fp32 and fp64
    assert torch.equal(p.float().double(), p) and torch.equal(p * rs_full * cs_full - t * rs_full, d)
    invalid = torch.rand(n, generator=gen) < nan_fraction
    mask = None
    if mask_on:
        mask = torch.rand(n, generator=gen) < 0.7
        mask[:len(placed)] = True
        mask = mask.reshape(rows, width)
    invalid[:len(placed)] = False
    t = t.clone()
    t[invalid.reshape(rows, width)] = float("nan")
    return p.float(), t.float(), rs, cs, mask


def run(term, case, kind, delta, reduction, weight, dev, count=True, **kw):
    p, t, rs, cs, mask = case
    dv = lambda x: None if x is None else x.to(dev)  # noqa: E731
    if count:
        term.reset()
        term.count(dv(p), dv(t), dv(mask))
    loss, seed = term(dv(p), dv(t), kind=kind, delta=delta, weight=weight, reduction=reduction, row_scale=dv(rs),
                      col_scale=dv(cs), mask=dv(mask), **kw)
    return loss, seed


def check(term, loss, seed, ref, what):
    from metatrain_amd.loss import read_stats

    st = read_stats(term.stats())
    n = ref["count"]
    assert st["count"] == n, what
    d = ref["d"]
    for name, got, want, terms in (("loss", float(loss), float(ref["loss"]), abs(float(ref["loss"]))),
                                   ("stats.loss", st["loss"], float(ref["loss"]), abs(float(ref["loss"]))),
                                   ("sum_sq", st["sum_sq"], float(ref["sum_sq"]), float((d * d).sum())),
                                   ("sum_abs", st["sum_abs"], float(ref["sum_abs"]), float(d.abs().sum()))):
        assert abs(got - want) <= 2 * n * U * terms, (what, name, got, want)
    if seed is not None:
        got = seed.cpu().double()
        want = ref["seed"]
        assert got.shape == want.shape
        assert bool((got[~ref["valid"]] == 0).all()), what
        err = (got - want).abs()
        bound = (2.0 ** -24 + 2.0 ** -50) * want.abs()
        assert bool((err <= bound).all()), (what, float((err - bound).max()))


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("rows", ROWS)
def test_kernel_matches_the_oracle(rows, width):
    from metatrain_amd.loss import PointwiseLoss

    dev = torch.device("cuda:0")
    term = PointwiseLoss()
    variants = [dict(), dict(rs_on=True), dict(cs_on=True), dict(mask_on=True), dict(rs_on=True, cs_on=True, mask_on=True)]
    for vi, variant in enumerate(variants):
        case = make_case(rows, width, 1000 * rows + 10 * width + vi, **variant)
        p, t, rs, cs, mask = case
        for kind, delta in KINDS:
            for reduction, weight in (("mean", 0.7), ("sum", 1.0)):
                what = (rows, width, variant, kind, delta, reduction)
                ref = O.term(p, t, kind, reduction, delta, weight, rs, cs, mask)
                loss, seed = run(term, case, kind, delta, reduction, weight, dev)
                check(term, loss, seed, ref, what)
        # the evaluation form: no seeds, the same sums
        term.reset()
        term.count(p.to(dev), t.to(dev), None if mask is None else mask.to(dev))
        loss, seed = run(term, case, "huber", 1.0, "mean", 0.7, dev, count=False, want_seed=False)
        assert seed is None
        check(term, loss, None, O.term(p, t, "huber", "mean", 1.0, 0.7, rs, cs, mask), (rows, width, variant, "evaluation"))


@pytest.mark.parametrize("how", ["all_nan", "all_masked"])
def test_a_term_without_valid_entries_is_zero(how):
    from metatrain_amd.loss import PointwiseLoss, read_stats

    dev = torch.device("cuda:0")
    p, t, rs, cs, _ = make_case(257, 3, 5, rs_on=True, cs_on=True)
    mask = None
    if how == "all_nan":
        t = torch.full_like(t, float("nan"))
    else:
        mask = torch.zeros(t.shape, dtype=torch.bool)
    term = PointwiseLoss()
    for kind, delta in KINDS:
        for reduction in ("mean", "sum"):
            loss, seed = run(term, (p, t, rs, cs, mask), kind, delta, reduction, 0.7, dev)
            assert float(loss) == 0.0 and bool((seed == 0).all())
            assert read_stats(term.stats()) == {"loss": 0.0, "sum_sq": 0.0, "sum_abs": 0.0, "count": 0}


def test_two_identical_calls_are_bitwise_equal_and_a_nan_prediction_spreads():
    from metatrain_amd.loss import PointwiseLoss

    dev = torch.device("cuda:0")
    case = make_case(513, 5, 77, rs_on=True, cs_on=True, mask_on=True)
    # (no dyadic luck here: weights and scales with full mantissas, so the sums do round)
    gen = torch.Generator().manual_seed(1)
    p = case[0] + torch.randn(case[0].shape, generator=gen) * 0.1
    case = (p, case[1], torch.rand(513, generator=gen).double() + 0.5, torch.rand(5, generator=gen).double() + 0.5, case[4])
    results = []
    for _ in range(2):
        term = PointwiseLoss()
        loss, seed = run(term, case, "huber", 0.25, "mean", 0.37, dev)
        results.append((loss.clone(), seed.clone(), term.stats().clone()))
    for a, b in zip(*results):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a.view(torch.int32),
                           b.view(torch.int64) if b.dtype == torch.float64 else b.view(torch.int32))
    # a NaN prediction at a valid entry is not dropped
    valid = ~torch.isnan(case[1]) & case[4]
    r, c = [int(v) for v in torch.nonzero(valid)[-1]]
    p = case[0].clone()
    p[r, c] = float("nan")
    for kind, delta in KINDS:
        loss, _ = run(PointwiseLoss(), (p,) + case[1:], kind, delta, "mean", 1.0, dev)
        assert bool(torch.isnan(loss)), kind


def test_counting_in_parts_then_one_call_per_part_reproduces_the_one_call_loss():
    """The micro-batched order: count every part, then the pointwise calls; the mean is over the whole."""
    from metatrain_amd.loss import PointwiseLoss, read_stats

    dev = torch.device("cuda:0")
    case = make_case(513, 3, 9, rs_on=True, cs_on=True, mask_on=True)
    p, t, rs, cs, mask = case
    for kind, delta in KINDS:
        ref = O.term(p, t, kind, "mean", delta, 0.7, rs, cs, mask)
        term = PointwiseLoss()
        parts = [slice(0, 100), slice(100, 400), slice(400, 513)]
        for s in parts:
            term.count(p[s].to(dev), t[s].to(dev), mask[s].to(dev))
        total = torch.zeros((), dtype=torch.float64, device=dev)
        seeds = []
        for s in parts:
            _, seed = run(term, (p[s], t[s], rs[s], cs, mask[s]), kind, delta, "mean", 0.7, dev, count=False, loss_out=total)
            seeds.append(seed)
        check(term, total, torch.cat(seeds), ref, (kind, delta, "three parts"))
        assert read_stats(term.stats())["count"] == ref["count"]
        assert np.isfinite(float(total))
