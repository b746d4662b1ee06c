"""Independent references and seeded edge cases for the refiner's integer geometry.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

The SubM neighbour map has two restatements that share their key packing (the HIP kernel in csrc/subm.hip and
`ptv3_ref.subm_neighbors`), so a packing error agrees with itself.  `subm_neighbors_bruteforce` below shares nothing
with either: a Python dict keyed by (b, x, y, z) tuples, 27 lookups per point, no packing arithmetic at all.
`pair_lists_ref` states the offset-major pair lists of a map, `pooling_ref` the integer half of Pointcept's
SerializedPooling.  The case builders put a few thousand points at most on the edges the kernels can get wrong
(the 16-bit coordinate range, several batches, full 27-neighbourhoods, the smallest hash tables, depth 1), and each
asserts that its points really reach the edge it is named for.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

COORD_MAX = 65535  # largest coordinate of a depth-16 grid (16-bit key fields)


def _offset(k: int):
    return k // 9 - 1, (k // 3) % 3 - 1, k % 3 - 1


def subm_neighbors_bruteforce(grid, batch=None) -> np.ndarray:
    """nbr [n][27] (int64): nbr[i][k] = the lowest point index in voxel grid[i] + (dx, dy, dz) of i's batch,
    k = 9 (dx + 1) + 3 (dy + 1) + (dz + 1); -1 when no point is there or a neighbour coordinate is negative."""
    g = np.asarray(grid).astype(np.int64).reshape(-1, 3).tolist()
    n = len(g)
    b = [0] * n if batch is None else np.asarray(batch).astype(np.int64).reshape(-1).tolist()
    assert len(b) == n
    first: Dict[tuple, int] = {}
    for i in range(n):
        first.setdefault((b[i], g[i][0], g[i][1], g[i][2]), i)  # ascending i: the lowest index stays
    nbr = np.full((n, 27), -1, dtype=np.int64)
    for i in range(n):
        x, y, z = g[i]
        for k in range(27):
            dx, dy, dz = _offset(k)
            xx, yy, zz = x + dx, y + dy, z + dz
            if xx < 0 or yy < 0 or zz < 0:
                continue
            nbr[i, k] = first.get((b[i], xx, yy, zz), -1)
    return nbr


def pair_lists_ref(nbr, with_centre: bool) -> Dict[str, np.ndarray]:
    """Offset-major pair lists of a neighbour map: pair_in / pair_out (output rows ascending within an offset; the
    centre k = 13 only `with_centre`), pair_off [28] (pair_off[k] = first pair of offset k, pair_off[27] = count),
    pair_pos [n][27] (index of pair (k, row), -1: none) and cpos [n][32] (a row's present pair indices in ascending
    offset order, then -1, their count in column 31)."""
    nbr = np.asarray(nbr)
    n = nbr.shape[0]
    pin: List[int] = []
    pout: List[int] = []
    off = np.zeros(28, dtype=np.int64)
    pos = np.full((n, 27), -1, dtype=np.int64)
    for k in range(27):
        off[k] = len(pin)
        if k == 13 and not with_centre:
            continue
        for i in range(n):
            if nbr[i, k] >= 0:
                pos[i, k] = len(pin)
                pout.append(i)
                pin.append(int(nbr[i, k]))
    off[27] = len(pin)
    cpos = np.full((n, 32), -1, dtype=np.int64)
    for i in range(n):
        present = [int(p) for p in pos[i] if p >= 0]
        cpos[i, :len(present)] = present
        cpos[i, 31] = len(present)
    return dict(pair_in=np.asarray(pin, dtype=np.int64), pair_out=np.asarray(pout, dtype=np.int64), pair_off=off,
                pair_pos=pos, cpos=cpos)


def pooling_ref(codes, stride: int, depth: int) -> dict:
    """The integer half of Pointcept's SerializedPooling on serialized codes [R][n] (torch int64, rows in logical
    order): torch.unique(code[0] >> 3pd), a stable sort of the clusters, the argsort of the pooled codes."""
    import torch
    pd = (stride - 1).bit_length()
    if pd > depth:
        pd = 0
    code = codes >> 3 * pd
    _, cluster, counts = torch.unique(code[0], sorted=True, return_inverse=True, return_counts=True)
    indices = torch.sort(cluster, stable=True).indices
    ptr = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])
    head = indices[ptr[:-1]]
    code_h = code[:, head]
    order = torch.argsort(code_h, stable=True)
    inverse = torch.zeros_like(order).scatter_(1, order, torch.arange(code_h.shape[1]).repeat(code_h.shape[0], 1))
    return dict(pd=pd, code=code, cluster=cluster, counts=counts, indices=indices, ptr=ptr, head=head,
                code_h=code_h, order=order, inverse=inverse)


# ---- cases ------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    grid: np.ndarray                 # [n][3] int32
    batch: Optional[np.ndarray]      # [n] int32, or None (one batch)
    depth: int                       # serialization depth the case is meant for
    info: dict = field(default_factory=dict)
    _nbr: Optional[np.ndarray] = None

    @property
    def n(self) -> int:
        return self.grid.shape[0]

    @property
    def batch0(self) -> np.ndarray:
        return np.zeros(self.n, np.int32) if self.batch is None else self.batch

    @property
    def nbr(self) -> np.ndarray:
        """The brute-force map, computed once per case."""
        if self._nbr is None:
            self._nbr = subm_neighbors_bruteforce(self.grid, self.batch)
            self._nbr.setflags(write=False)
        return self._nbr

    def sorted_by_batch(self, dense: bool = True) -> "Case":
        """The same points with each batch's points contiguous (a stable sort by batch), the way offsets describe
        them; dense: batch indices renumbered 0 .. B-1 in ascending order."""
        o = np.argsort(self.batch0, kind="stable")
        b = self.batch0[o]
        if dense:
            b = np.unique(b, return_inverse=True)[1].astype(np.int32)
        return Case(self.name + "/by-batch", np.ascontiguousarray(self.grid[o]), np.ascontiguousarray(b), self.depth,
                    dict(self.info))


def _finish(name, pts, depth, rng, info=None, shuffle=True, batched=True) -> Case:
    a = np.asarray(pts, dtype=np.int64).reshape(-1, 4)
    if shuffle:
        a = a[rng.permutation(a.shape[0])]
    grid = np.ascontiguousarray(a[:, 1:4], dtype=np.int32)
    batch = np.ascontiguousarray(a[:, 0], dtype=np.int32) if batched else None
    assert grid.min() >= 0 and grid.max() < (1 << depth), name
    return Case(name, grid, batch, depth, info or {})


def range_corners(seed: int = 0) -> Case:
    """About 2000 points at depth 16: a 3x3x3 block at each of the eight corners of [0, 65535]^3 in every batch of
    {0, 1, 16383}, points on the upper faces, and every point a key field's carry could be confused with -- for
    (x, y, 65535) the point (x, y+1, 0), for (x, 65535, z) the point (x+1, 0, z), for (65535, y, z) of batch b the
    point (0, y, z) of batch b + 1 -- plus random points of the whole range."""
    rng = np.random.default_rng(seed)
    M = COORD_MAX
    batches = (0, 1, 16383)
    pts = set()
    ends = ((0, 1, 2), (M - 2, M - 1, M))
    for b in batches:
        for cx in ends:
            for cy in ends:
                for cz in ends:
                    pts.update((b, x, y, z) for x in cx for y in cy for z in cz)
    for axis in range(3):  # points on each upper face away from the corners
        for _ in range(100):
            c = rng.integers(3, M - 3, size=3).tolist()
            c[axis] = M
            pts.add((int(rng.choice(batches)), *c))
    partners = {"x": 0, "y": 0, "z": 0}
    for (b, x, y, z) in sorted(pts):
        if z == M and y + 1 <= M:
            pts.add((b, x, y + 1, 0))
            partners["z"] += 1
        if y == M and x + 1 <= M:
            pts.add((b, x + 1, 0, z))
            partners["y"] += 1
        if x == M and (b + 1) in batches:
            pts.add((b + 1, 0, y, z))
            partners["x"] += 1
    # the edge this case is named for: at least one wrap partner per axis is really among the points
    assert any(z == M and (b, x, y + 1, 0) in pts for (b, x, y, z) in pts)
    assert any(y == M and (b, x + 1, 0, z) in pts for (b, x, y, z) in pts)
    assert any(x == M and (b + 1, 0, y, z) in pts for (b, x, y, z) in pts)
    assert min(partners.values()) > 0
    pts = sorted(pts)
    fill = [(int(rng.choice(batches)), *rng.integers(0, M + 1, size=3).tolist()) for _ in range(2000 - len(pts))]
    dup = [pts[i] for i in rng.integers(0, len(pts), size=20)]  # a few duplicate voxels, corners included
    case = _finish("range_corners", pts + fill + dup, 16, rng, dict(partners=partners, batches=batches))
    assert int(case.grid.max()) == M and int(case.grid.min()) == 0 and int(case.batch.max()) == 16383
    return case


def batched_twins(B: int = 3, seed: int = 1) -> Case:
    """The same ~983 voxels in each of B batches at shuffled indices, plus 50 duplicate voxels inside batch 1: a
    map that ignores the batch, or resolves a voxel to another batch's twin, differs on nearly every row."""
    rng = np.random.default_rng(seed)
    side = 20  # 983 of 8000 cells: most points have a few neighbours
    cells = rng.choice(side ** 3, size=983, replace=False)
    vox = np.stack([cells // (side * side), (cells // side) % side, cells % side], 1)
    pts = [(b, *v) for b in range(B) for v in vox.tolist()]
    pts += [(1, *vox[i]) for i in rng.integers(0, len(vox), size=50).tolist()]
    case = _finish(f"batched_twins[B={B}]", pts, 5, rng, dict(B=B, voxels=len(vox)))
    for b in range(B):  # every batch holds the whole voxel set
        assert len({tuple(v) for v in case.grid[case.batch == b].tolist()}) == len(vox)
    assert case.n == B * len(vox) + 50
    return case


def dense_cube(twice: bool = False, seed: int = 2) -> Case:
    """A full 16x16x16 block in shuffled point order (twice: every voxel present twice): every interior point has
    all 27 neighbours, which is where the pair lists reach their documented capacity per row."""
    rng = np.random.default_rng(seed + (10 if twice else 0))
    o = (7, 0, 11)  # one face on the coordinate 0 boundary
    r = np.arange(16)
    vox = np.stack(np.meshgrid(r + o[0], r + o[1], r + o[2], indexing="ij"), -1).reshape(-1, 3)
    pts = [(0, *v) for v in vox.tolist()] * (2 if twice else 1)
    case = _finish("dense_cube" + ("[twice]" if twice else ""), pts, 5, rng, batched=False)
    g = case.grid.astype(np.int64) - np.asarray(o)
    interior = ((g >= 1) & (g <= 14)).all(1)
    case.info.update(interior=interior)
    assert int(interior.sum()) == 14 ** 3 * (2 if twice else 1)
    assert bool((case.nbr[interior] >= 0).all()), "an interior row lacks one of its 27 neighbours"
    assert bool((case.nbr[~interior] < 0).any(1).all())
    return case


_GOLDEN = 0x9E3779B97F4A7C15


def table_log2(n: int) -> int:
    """csrc/subm.hip sfx_subm_table_log2 restated: the smallest table of 2^l >= 2n slots, l >= 4."""
    l = 4
    while (1 << l) < 2 * max(n, 1):
        l += 1
    return l


def slot_of(b: int, x: int, y: int, z: int, log2cap: int) -> int:
    """csrc/subm.hip pack + slot_of restated: the home slot of voxel (b, x, y, z) in a 2^log2cap-slot table."""
    key = (b << 48) | (x << 32) | (y << 16) | z
    return ((key * _GOLDEN) & 0xFFFFFFFFFFFFFFFF) >> (64 - log2cap)


def tiny() -> List[Case]:
    """n = 1 .. 9 points: the 16-slot table up to its 2n bound (n = 8) and the first 32-slot one (n = 9).  Three
    layouts per n: all points in one voxel; a touching clump with one duplicate; and voxels whose home slot is the
    table's LAST slot, so every probe chain but the first wraps past the end of the table."""
    rng = np.random.default_rng(3)
    cases = []
    for n in range(1, 10):
        l2 = table_log2(n)
        last = (1 << l2) - 1
        assert l2 == (4 if n <= 8 else 5)
        cases.append(_finish(f"tiny[n={n},one-voxel]", [(0, 4, 5, 6)] * n, 3, rng, batched=False))
        clump = [(0, 1 + (i % 2), 1 + (i // 2) % 2, (i // 4) % 2) for i in range(n)]
        if n > 2:
            clump[-1] = clump[0]
        cases.append(_finish(f"tiny[n={n},clump]", clump, 2, rng, batched=False))
        if n < 2:
            continue
        # ceil(n / 2) (at least 2) voxels of [0, 32)^3 homed at the last slot, then +z neighbours of them (a
        # multiplicative hash never homes two adjacent voxels at one slot), so hits are found through wrapped chains
        home = [(x, y, z) for x in range(32) for y in range(32) for z in range(0, 32, 3)
                if slot_of(0, x, y, z, l2) == last]
        nh = max(2, (n + 1) // 2)
        pick = home[:nh] + [(v[0], v[1], v[2] + 1) for v in home[:n - nh]]
        # the edge: distinct keys whose home is the last slot collide there, and all but the first wrap to slot 0
        assert len(set(pick)) == n and sum(slot_of(0, *v, l2) == last for v in pick) >= 2
        c = _finish(f"tiny[n={n},wrap]", [(0, *v) for v in pick], 6, rng,
                    dict(log2cap=l2, home=last, homed=nh), batched=False)
        assert n < 3 or bool((c.nbr[:, [12, 14]] >= 0).any()), "no adjacent pair among the wrapped keys"
        cases.append(c)
    return cases


def depth_one(seed: int = 4) -> Case:
    """257 points of {0, 1}^3: each of the 8 codes is shared by about 32 points, which only a stable sort orders
    like the reference."""
    rng = np.random.default_rng(seed)
    pts = [(0, *rng.integers(0, 2, size=3).tolist()) for _ in range(257)]
    case = _finish("depth_one", pts, 1, rng, batched=False)
    assert len({tuple(v) for v in case.grid.tolist()}) == 8 and int(case.grid.max()) == 1
    return case


def all_cases() -> List[Case]:
    """Every case the SubM map is compared on."""
    return [range_corners(), batched_twins(), dense_cube(False), dense_cube(True), *tiny(), depth_one()]
