"""The geometry oracle checks itself (CPU only): `ptv3_ref.subm_neighbors` (packed keys + searchsorted) against a
brute-force dict of (b, x, y, z) tuples that uses no packing arithmetic, on the cases of oracle/geometry_cases.py --
the corners of the 16-bit coordinate range, several batches, full 27-neighbourhoods, the smallest hash tables.

This is the comparison that caught the key packing at coordinate 65535: with x + 1, y + 1, z + 1 in 16-bit fields,
65536 carried into the next field and `range_corners` reported neighbours in another row, column or batch.  The GPU
kernel packed its keys the same way, so kernel-vs-oracle comparisons agreed with the wrong answer."""
import numpy as np
import pytest
import torch

from oracle import geometry_cases as gc
from oracle import ptv3_ref


@pytest.fixture(scope="module")
def cases():
    """Every builder runs its own assertions (wrap partners present, the last table slot collided, interior rows
    with all 27 neighbours) when it builds its case."""
    return {c.name: c for c in gc.all_cases()}


CASE_NAMES = [c.name for c in gc.all_cases()]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_bruteforce_equals_packed_oracle(cases, name):
    c = cases[name]
    ref = ptv3_ref.subm_neighbors(torch.from_numpy(c.grid), torch.from_numpy(c.batch0).long()).numpy()
    bad = np.argwhere(ref != c.nbr)
    assert bad.shape[0] == 0, (
        f"{name}: {bad.shape[0]} entries differ; first (row, k) = {bad[0].tolist()}: packed oracle "
        f"{ref[bad[0][0], bad[0][1]]} vs brute force {c.nbr[bad[0][0], bad[0][1]]} "
        f"(point {c.grid[bad[0][0]].tolist()} batch {int(c.batch0[bad[0][0]])})")


def test_issue_example_has_no_false_neighbours():
    """The four points that showed the carry: no neighbour across the range edge, none in another batch."""
    grid = np.array([[5, 7, 65535], [5, 8, 0], [65535, 3, 3], [0, 3, 3]], np.int32)
    batch = np.array([0, 0, 0, 1], np.int32)
    want = np.full((4, 27), -1, np.int64)
    want[np.arange(4), 13] = np.arange(4)
    assert np.array_equal(gc.subm_neighbors_bruteforce(grid, batch), want)
    ref = ptv3_ref.subm_neighbors(torch.from_numpy(grid), torch.from_numpy(batch).long()).numpy()
    assert np.array_equal(ref, want)


def test_bruteforce_known_answers():
    grid = np.array([[5, 5, 5], [5, 5, 5], [6, 5, 5], [5, 5, 5], [0, 0, 0], [5, 5, 6]], np.int32)
    batch = np.array([0, 0, 0, 0, 0, 1], np.int32)
    nbr = gc.subm_neighbors_bruteforce(grid, batch)
    assert nbr[3, 13] == 0 and nbr[0, 22] == 2 and nbr[2, 4] == 0  # lowest duplicate; +x; -x
    assert (nbr[4, :13] == -1).all() and nbr[4, 13] == 4  # negative coordinates never match
    assert nbr[0, 14] == -1 and (nbr[5] >= 0).sum() == 1  # (5,5,6) is in another batch
    assert np.array_equal(gc.subm_neighbors_bruteforce(grid[:5], None), nbr[:5])


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("centre", [False, True])
def test_pair_lists_ref_agrees_with_map(cases, name, centre):
    c = cases[name]
    nbr, n = c.nbr, c.n
    pl = gc.pair_lists_ref(nbr, centre)
    off, pin, pout, pos, cpos = pl["pair_off"], pl["pair_in"], pl["pair_out"], pl["pair_pos"], pl["cpos"]
    present = nbr >= 0
    if not centre:
        present = present.copy()
        present[:, 13] = False
    assert off[0] == 0 and off[27] == present.sum() == len(pin) == len(pout)
    assert off[27] <= (27 if centre else 26) * n  # the documented capacity of pair_in / pair_out
    assert np.array_equal(np.diff(off), present.sum(0))
    for k in range(27):
        rows = pout[off[k]:off[k + 1]]
        assert np.array_equal(rows, np.nonzero(present[:, k])[0])  # ascending output rows
        assert np.array_equal(pin[off[k]:off[k + 1]], nbr[rows, k])
        assert np.array_equal(pos[rows, k], np.arange(off[k], off[k + 1]))
    assert np.array_equal(pos >= 0, present)
    assert np.array_equal(cpos[:, 31], present.sum(1))
    for i in range(n):
        cnt = cpos[i, 31]
        assert np.array_equal(cpos[i, :cnt], pos[i][pos[i] >= 0]) and (cpos[i, cnt:31] == -1).all()
    if name.startswith("dense_cube"):  # the rows that reach the per-row capacity
        assert (cpos[c.info["interior"], 31] == (27 if centre else 26)).all()


def test_pooling_ref_small():
    """Two clusters at stride 2: codes >> 3, members in index order, heads, pooled orders."""
    codes = torch.tensor([[9, 1, 8, 15, 0], [1, 9, 2, 8, 7]])
    r = gc.pooling_ref(codes, 2, 2)
    assert r["pd"] == 1 and r["cluster"].tolist() == [1, 0, 1, 1, 0] and r["counts"].tolist() == [2, 3]
    assert r["indices"].tolist() == [1, 4, 0, 2, 3] and r["ptr"].tolist() == [0, 2, 5] and r["head"].tolist() == [1, 0]
    assert r["code_h"].tolist() == [[0, 1], [1, 0]] and r["order"].tolist() == [[0, 1], [1, 0]]
    assert r["inverse"].tolist() == [[0, 1], [1, 0]]
    assert gc.pooling_ref(codes, 4, 1)["pd"] == 0  # a pooling depth beyond the serialized depth pools nothing


def test_slot_of_restates_table_size():
    assert [gc.table_log2(n) for n in (0, 1, 8, 9, 16, 17)] == [4, 4, 4, 5, 5, 6]
    wrap = [c for c in gc.tiny() if c.name.endswith("wrap]")]
    assert len(wrap) == 8
    for c in wrap:
        assert c.info["home"] == (1 << c.info["log2cap"]) - 1 and c.info["homed"] >= 2
        assert sum(gc.slot_of(0, *v, c.info["log2cap"]) == c.info["home"] for v in c.grid.tolist()) == c.info["homed"]
