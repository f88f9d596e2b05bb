"""How many distinct rows the free-slip K of a box mesh has once every cell
adds the same element matrix -- on the CPU, with the oracle's element matrix
of cell 0 (oracle.Element.kle) planted in every cell and the oracle's
assembly order (kle_oracle.c orc_assemble_fs: ascending cells, every Dirichlet
row and column left out of K).

This is the ground for the meshes of tests/test_gpu_brick_dedup.py: the cap
`rows stored <= 2 D` proves something only where D, the number of distinct
upper-triangle node rows (lattice offsets of the blocks and the bits of their
values), lies well below the number of rows the bricks hold (free rows with
more than one stored block).  The library shares a K's rows only where that
saves half of the bricked bytes (9 doubles per block, rows padded to 16):

  * [8,8,4] ngl 3 and [8,8,2] ngl 5 repeat enough: the distinct rows' bytes
    are at most a quarter of all (so even with every row in both roles of a
    unit the sharing is taken);
  * [4,3,3] ngl 3, [4,4,2] ngl 3, [3,3,2] ngl 5 and [2,2,2] ngl 5, the small
    meshes, do not: more than a quarter, so there the library may keep every
    row's own storage and the GPU tests check the bitwise product and the
    refusal instead.  [4,3,3] still has translated interior rows: D below the
    bricked rows; [2,2,2] has no interior element and no two rows equal.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as O

SHARED = {"8x8x4-p2": ([8, 8, 4], 3), "8x8x2-p4": ([8, 8, 2], 5)}
SMALL = {"4x3x3-p2": ([4, 3, 3], 3), "4x4x2-p2": ([4, 4, 2], 3), "3x3x2-p4": ([3, 3, 2], 5),
         "2x2x2-p4": ([2, 2, 2], 5)}


@functools.lru_cache(maxsize=None)
def distinct(name):
    """(D, bricked rows, bytes of the distinct rows, bytes of all) of the K
    with cell 0's matrix planted, every boundary node a Dirichlet node."""
    nelem, ngl = {**SHARED, **SMALL}[name]
    m = O.BoxMesh(3, nelem, [0, 0, 0], [1, 1, 1], ngl)
    L = np.array([n * (ngl - 1) + 1 for n in nelem])
    nn, N = ngl ** 3, m.N
    ke = O.Element(ngl, 3).kle(m.corners()[0])[0].reshape(nn, 3, nn, 3).transpose(0, 2, 1, 3).reshape(nn, nn, 9)
    lat = np.rint(m.coords() * (L - 1)).astype(np.int64)
    assert len(np.unique(lat, axis=0)) == N
    free = ((lat > 0) & (lat < L - 1)).all(axis=1)
    conn = m.conn()
    gi = np.repeat(conn, nn, axis=1).ravel()  # (cells ascending, li, lj: the oracle's add order)
    gj = np.tile(conn, (1, nn)).ravel()
    blk = np.tile(ke.reshape(nn * nn, 9), (m.E, 1))
    keep = free[gi] & free[gj] & (gj >= gi)
    gi, gj, blk = gi[keep], gj[keep], blk[keep]
    pairs, inv = np.unique(gi * N + gj, return_inverse=True)
    val = np.zeros((len(pairs), 9))
    np.add.at(val, inv, blk)  # (unbuffered: in the order given)
    pi, pj = pairs // N, pairs % N
    start = np.searchsorted(pi, np.arange(N + 1))
    seen = {}
    rows = total = 0
    for i in np.nonzero(free)[0]:
        s, e = start[i], start[i + 1]
        if e - s <= 1:
            continue  # (a one-block row: formed by the gather, not by the bricks)
        size = 8 * ((9 * (e - s) + 15) // 16 * 16)
        rows += 1
        total += size
        seen[((lat[pj[s:e]] - lat[i]).tobytes(), val[s:e].tobytes())] = size
    return len(seen), rows, sum(seen.values()), total


@pytest.mark.parametrize("name", list(SHARED))
def test_the_meshes_the_sharing_is_tested_on_repeat_their_rows(name):
    D, rows, dbytes, total = distinct(name)
    print(f"DEDUP-TRUTH {name}: D {D} of {rows} bricked rows, {dbytes} of {total} B")
    assert 0 < D and 4 * D <= rows and 4 * dbytes <= total


@pytest.mark.parametrize("name", list(SMALL))
def test_the_small_meshes_repeat_too_little_to_share(name):
    D, rows, dbytes, total = distinct(name)
    print(f"DEDUP-TRUTH {name}: D {D} of {rows} bricked rows, {dbytes} of {total} B")
    assert 4 * dbytes > total
    if name == "4x3x3-p2":
        assert D < rows  # (the two interior elements along x: translated rows)
    if name == "2x2x2-p4":
        assert D == rows
