"""The slot -> row map of the fused attention tiles (``csrc/ablk_rows.h``), compiled by the host compiler into a stand-alone
program (``tests/ablk_rows_host_main.cpp``) that prints it exhaustively, against the plain definition of a tile restated here:
slot 0 is atom A's centre token, slots 1 .. TA - 1 its neighbours (CSR rows startA ..), slot TA atom B's centre token, the slots
behind it B's neighbours (CSR rows startB ..), and slots past the last token repeat the last token. No GPU call is made."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = (1 << 33) + 12345


def fields(TA, TB):
    """the descriptor the host program gives tile (TA, TB): atomA, startA, atomB, startB"""
    return 1000 + 7 * TA + TB, 100000 + 64 * TA, 5000 + 11 * TB + TA, 300 + 3 * TB


def plain(TA, TB, s):
    """(centre, atom, CSR row or None, row of the token stream) of slot s, branch by branch"""
    atomA, startA, atomB, startB = fields(TA, TB)
    T = TA + TB
    if s >= T:
        s = T - 1
    if s < TA:
        atom, local, start = atomA, s, startA
    else:
        atom, local, start = atomB, s - TA, startB
    if local == 0:
        return 1, atom, None, E + atom
    return 0, atom, start + local - 1, start + local - 1


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ to build the host program with")
    exe = str(tmp_path_factory.mktemp("ablk_rows") / "ablk_rows_host")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "metatrain_amd", "csrc"),
                    os.path.join(ROOT, "tests", "ablk_rows_host_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return np.array([[int(v) for v in line.split()] for line in out.strip().split("\n")], dtype=np.int64)


def _check(rows):
    for TA, TB, s, centre, atom, edge, row in rows.tolist():
        c, a, e, r = plain(TA, TB, s)
        assert (centre, atom, row) == (c, a, r), (TA, TB, s)
        if e is not None:
            assert edge == e, (TA, TB, s)


def test_every_32_slot_tile(table):
    rows = table[table[:, 0] <= 32]
    shapes = {(TA, TB) for TA in range(1, 33) for TB in range(0, 33 - TA)}
    assert {(int(a), int(b)) for a, b in rows[:, :2]} == shapes and len(rows) == 32 * len(shapes)
    assert len({tuple(r) for r in rows[:, :3].tolist()}) == len(rows)  # every slot of every shape, once
    _check(rows)


def test_every_64_slot_tile(table):
    rows = table[table[:, 0] > 32]
    assert {int(a) for a in rows[:, 0]} == set(range(33, 65)) and (rows[:, 1] == 0).all() and len(rows) == 64 * 32
    assert len({tuple(r) for r in rows[:, :3].tolist()}) == len(rows)
    _check(rows)


def test_centre_rows_and_ranges_of_a_tile(table):
    """what the kernels rely on: exactly the slots 0 and TA (if B is there) are centre tokens, and the neighbour rows of each atom
    are one contiguous ascending CSR range"""
    for TA, TB in [(1, 0), (1, 31), (16, 16), (15, 17), (2, 17), (32, 0), (33, 0), (64, 0)]:
        rows = table[(table[:, 0] == TA) & (table[:, 1] == TB)]
        T = TA + TB
        live = rows[rows[:, 2] < T]
        assert live[live[:, 3] == 1][:, 2].tolist() == ([0, TA] if TB else [0])
        _, startA, _, startB = fields(TA, TB)
        assert live[(live[:, 3] == 0) & (live[:, 2] < TA)][:, 5].tolist() == list(range(startA, startA + TA - 1))
        assert live[(live[:, 3] == 0) & (live[:, 2] > TA)][:, 5].tolist() == list(range(startB, startB + max(TB - 1, 0)))
        dead = rows[rows[:, 2] >= T]
        assert (dead[:, 3:] == live[-1, 3:]).all()  # slots past the last token repeat it
