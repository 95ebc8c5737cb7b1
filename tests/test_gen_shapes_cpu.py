"""The case table of ``tests/gen_shapes.py`` does what it claims (no GPU): every case is a size the library accepts, the
table reaches every head-dimension bucket of ``attn_dispatch`` and the width classes the linears and slice loads branch
on, input (b) has the row counts and token counts the tails need, and every (case, input, quantity) is pinned by the
fp32 yardstick (``y <= 1e-3``)."""
import pytest

import gen_shapes as gs


def test_every_case_is_a_supported_size():
    """The size rule of ``pet_hypers_supported`` (abi.hip): d_pet a multiple of num_heads, head dimension at most 128."""
    for tag, c in gs.CASES.items():
        assert all(c[k] >= 1 for k in ("d_pet", "d_node", "d_feedforward", "d_head", "num_heads")), tag
        assert c["d_pet"] % c["num_heads"] == 0 and gs.head_dim(tag) <= 128, tag
        assert (c["d_pet"], c["d_node"], c["d_feedforward"], c["d_head"], c["num_heads"]) != (128, 256, 256, 128, 8), tag


def test_the_table_reaches_every_bucket_and_width_class():
    hd = {tag: gs.head_dim(tag) for tag in gs.CASES}
    assert hd == {"hd3": 3, "odd33": 11, "odd33_legacy": 11, "hd12": 12, "k65": 13, "hd24": 24, "hd32": 32, "hd48": 48,
                  "hd96": 96, "hd128": 128}
    assert {gs.hdm_bucket(h) for h in hd.values()} == {4, 16, 32, 64, 128}
    # the pairs on input (b) keep one case per bucket
    assert {gs.hdm_bucket(hd[tag]) for tag, which in gs.PAIRS if which == "b"} == {4, 16, 32, 64, 128}
    assert len(gs.PAIRS) == 16 and len(set(gs.PAIRS)) == 16
    assert any(h % 16 != 0 and gs.hdm_bucket(h) > 16 for h in hd.values())            # partial slice above one slice
    assert any(h % 4 == 0 and h % 16 != 0 and gs.CASES[t]["d_pet"] % 4 == 0 for t, h in hd.items())   # v4, partial slice
    assert any(c["d_pet"] % 2 == 1 for c in gs.CASES.values())
    assert any(64 < w < 68 or w % 64 == 1 for tag in gs.CASES for w in gs.widths(tag))
    assert any(c["d_node"] == c["d_pet"] for c in gs.CASES.values())
    assert any(c["d_node"] > c["d_pet"] for c in gs.CASES.values())
    assert any(c["d_node"] < c["d_pet"] for c in gs.CASES.values())


def test_the_cluster_has_the_tails_it_is_here_for():
    inp = gs.case("hd3", "b")[2]
    p = gs.check_cluster(inp)
    print("cluster", p)
    a = gs.case("hd3", "a")[2]
    n, e = a["positions"].shape[0], a["centers"].shape[0]
    assert (n, e) == (104, 1908) and n % 4 == 0 and (e + n) % 4 == 0   # what input (a) alone never reaches


@pytest.mark.parametrize("tag,which", gs.PAIRS)
def test_every_pair_is_pinned_by_the_fp32_yardstick(tag, which):
    ref, ys = gs.reference(tag, which)
    assert ("cell_grad" in ys) == (which == "a")
    print(f"{tag} {which}: y", {q: f"{gs.worst(y):.2e}" for q, y in ys.items()})
    for q, y in ys.items():
        assert gs.worst(y) <= gs.Y_CAP, (tag, which, q, y)
        if q in gs.QUANTITIES:
            assert float(ref[q].abs().max()) > 0, (tag, which, q)
    for q in gs.GRAD_SETS:   # the parameter gradients carry signal: nothing is compared absolutely by accident
        assert sum(float(r.abs().max()) > 1e-12 for r in ref[q].values()) >= len(ref[q]) - 1, (tag, which, q)
