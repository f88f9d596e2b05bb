"""tests/mat_ref.py against dense longdouble arithmetic, and its power to see
the errors the GPU tests (test_gpu_mat_ref.py) are there for: each planted
error on the oracle's K of the smallest box case (fs2d_p2: box [3,2], ngl 3,
2x2 node blocks, Dirichlet boundary) must give err / bound > 1 on some row,
the unaltered data restated in plain fp64 numpy <= 1.  No GPU.

The restatement's own figures are printed (MATREF cpu ...): the baseline the
device figures of DESIGN.md are read against."""
import numpy as np
import pytest

import mat_ref as M
from krylov_ref import LD, Csr

LOWER, STEP = [-1.5, 0.25], [0.7, 0.05]


def _random_csr(m, n, seed, empty_every=0):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, min(n, 9) + 1, m)
    if empty_every:
        lens[::empty_every] = 0
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rng.choice(n, ln, replace=False)) for ln in lens] + [np.zeros(0, np.int64)])
    data = rng.uniform(-1.0, 1.0, int(indptr[-1])) * 10.0 ** rng.uniform(-3, 3, int(indptr[-1]))
    if len(data) > 2:
        data[1] = 0.0  # an explicit zero
    return Csr(indptr, indices.astype(np.int64), data, n)


def _dense(A, data=None, dtype=LD):
    D = np.zeros((A.m, A.n), dtype=dtype)
    D[M.rows_of(A), A.indices] = A.data if data is None else data
    return D


CASES = {"square": (12, 12, 0), "empty_rows": (15, 11, 3), "one": (1, 1, 0), "wide": (5, 40, 0), "tall": (30, 4, 4)}


@pytest.mark.parametrize("case", list(CASES))
def test_restatements_match_dense_longdouble(case):
    m, n, ee = CASES[case]
    A = _random_csr(m, n, 100 + m * n, ee)
    if case == "one":
        A = Csr([0, 1], [0], [-0.3], 1)
    rng = np.random.default_rng(7)
    D = _dense(A)
    absD = np.abs(D)
    x = rng.uniform(-1, 1, n)
    ref, bound = M.product(A, x)
    # (the reference against dense longdouble: to longdouble rounding of the row's scale)
    scale = absD @ np.abs(x.astype(LD))
    assert (np.abs(ref - D @ x.astype(LD)) <= 16 * np.finfo(LD).eps * scale).all()
    np.testing.assert_allclose(bound, (1.01 * M.U * A.row_lengths() * scale).astype(np.float64), rtol=1e-14)
    empty = A.row_lengths() == 0
    assert (ref[empty] == 0).all() and (bound[empty] == 0).all()
    y = rng.uniform(-1, 1, m)
    z, zb = M.mult_add(ref, bound, y)
    assert (z == y.astype(LD) + ref).all()
    np.testing.assert_allclose(zb, bound + (1.01 * M.U * np.abs(z)).astype(np.float64), rtol=1e-14)
    # scaled: a L R on the same pattern, zeros stay zeros
    L = rng.uniform(0.5, 2, m) * rng.choice([-1, 1], m)
    R = rng.uniform(0.5, 2, n) * rng.choice([-1, 1], n)
    L[0] = 0.0
    R[-1] = 0.0
    for l, r, k in ((L, None, 1), (None, R, 1), (L, R, 2)):
        v, b = M.scaled(A, l, r)
        want = D * (1 if l is None else l.astype(LD)[:, None]) * (1 if r is None else r.astype(LD)[None, :])
        got = _dense(A, v)
        assert (np.abs(got - want) <= 4 * np.finfo(LD).eps * np.abs(want)).all()
        np.testing.assert_allclose(b, (k * 1.01 * M.U * np.abs(v)).astype(np.float64), rtol=1e-14)
        assert (v[A.data == 0] == 0).all() and (b[v == 0] == 0).all()
        assert M.worst(M.scaled64(A, l, r), v, b)[0] <= 1
    # axpy: X a strict subset of Y's pattern (every other entry), and X = Y's pattern
    keep = np.arange(len(A.data)) % 2 == 0
    lens = np.add.reduceat(keep.astype(np.int64), A.indptr[:-1][A.row_lengths() > 0]) if keep.size else []
    xl = np.zeros(m, np.int64)
    xl[A.row_lengths() > 0] = lens
    X = Csr(np.concatenate([[0], np.cumsum(xl)]), A.indices[keep], rng.uniform(-1, 1, int(keep.sum())), n)
    for a in (-0.75, 1.0):
        ref_v, b = M.axpy(A, a, X)
        want = D + LD(a) * _dense(X)
        assert (np.abs(_dense(A, ref_v) - want) <= 4 * np.finfo(LD).eps * (np.abs(D) + np.abs(_dense(X)))).all()
        assert (ref_v[~keep] == A.data[~keep]).all() and (b[~keep] == 0).all()
        assert M.worst(M.axpy64(A, a, X), ref_v, b)[0] <= 1
    assert M.is_subset(A, X) and (M.is_subset(X, A) == bool(keep.all()))
    # union sum with a matrix of another pattern
    B = _random_csr(m, n, 900 + m * n)
    ip, ix, sv, sb = M.union_sum(A, B)
    S = Csr(ip, ix, sv.astype(np.float64), n)
    DB = _dense(B)
    in_a, in_b, got_pat = (np.zeros((m, n), bool) for _ in range(3))
    in_a[M.rows_of(A), A.indices] = True
    in_b[M.rows_of(B), B.indices] = True
    got_pat[M.rows_of(S), S.indices] = True
    np.testing.assert_array_equal(got_pat, in_a | in_b)
    assert (_dense(S, sv) == D + DB).all()
    Sb = _dense(S, sb, np.float64)
    assert (Sb[in_a ^ in_b] == 0).all()
    np.testing.assert_allclose(Sb[in_a & in_b], (1.01 * M.U * np.abs(D + DB)).astype(np.float64)[in_a & in_b], rtol=1e-14)
    # diagonal: stored entries, 0 elsewhere and beyond min(m, n)
    d = M.diagonal(A)
    for i in range(m):
        assert d[i] == (float(D[i, i]) if i < n and in_a[i, i] else 0.0)


def test_worst_and_input_vectors():
    w, at = M.worst(np.array([1.0, 2.0, 3.0]), np.array([1.0, 2.0, 3.0], LD), np.zeros(3))
    assert w == 0
    w, at = M.worst(np.array([1.0, 2.0, 3.0 + 2.0 ** -50]), np.array([1.0, 2.0, 3.0], LD), np.zeros(3))
    assert w == np.inf and at == (2,)
    w, at = M.worst(np.array([1.0, 2.5]), np.array([1.0, 2.0], LD), np.array([1.0, 0.25]))
    assert w == 2.0 and at == (1,)
    assert M.worst(np.zeros(0), np.zeros(0, LD), np.zeros(0)) == (0.0, ())
    A = _random_csr(9, 14, 5, 4)
    vecs = dict(M.input_vectors(A, C=2, seed=3))
    assert set(vecs) == {"uniform", "scales", "signs_longest", "signs_shortest", "unit_first", "unit_last",
                         "unit_longest", "node"}
    r = M.longest_row(A)
    s, e = A.indptr[r], A.indptr[r + 1]
    tot = np.abs(A.data[s:e].astype(LD)).sum()  # (nothing cancels: the row sum is sum |a|)
    assert abs(M.product(A, vecs["signs_longest"])[0][r] - tot) <= 8 * np.finfo(LD).eps * tot
    assert np.abs(vecs["scales"]).min() >= 1e-6 and np.abs(vecs["scales"]).max() <= 1e6
    assert vecs["unit_first"][0] == 1 and vecs["unit_last"][-1] == 1 and vecs["unit_longest"][A.indices[e - 1]] == 1
    assert np.count_nonzero(vecs["node"]) == 2


# ------------------------------------------------------------ planted errors
@pytest.fixture(scope="module")
def K():
    """The oracle's assembled K of fs2d_p2 with the box boundary Dirichlet."""
    from oracle import oracle as O
    nel = [3, 2]
    hi = [a + n * h for a, n, h in zip(LOWER, nel, STEP)]
    om = O.BoxMesh(2, nel, LOWER, hi, 3)
    xy = om.coords()
    flag = np.zeros(om.N, np.uint8)
    for d in range(2):
        flag |= (np.abs(xy[:, d] - LOWER[d]) < 1e-12) | (np.abs(xy[:, d] - hi[d]) < 1e-12)
    Kc = om.assemble_fs(flag)[0]
    Kf = om.assemble_fs(np.zeros(om.N, np.uint8))[0]  # no Dirichlet rows (planted error 3)
    return Csr(Kc.indptr, Kc.indices, Kc.data, om.N * 2), Csr(Kf.indptr, Kf.indices, Kf.data, om.N * 2)


def _interior_row(A):
    return M.longest_row(A)


def test_clean_restatement_is_within_every_bound(K):
    A, Afree = K
    worst = {}
    for nm, x in M.input_vectors(A, C=2, seed=11):
        ref, b = M.product(A, x)
        worst["mult " + nm] = M.worst(M.product64(A, x), ref, b)
        y = M.x_uniform(A.m, 12)
        z, zb = M.mult_add(ref, b, y)
        worst["multAdd " + nm] = M.worst(y + M.product64(A, x), z, zb)
    rng = np.random.default_rng(13)
    L = rng.uniform(0.5, 2, A.m) * rng.choice([-1, 1], A.m)
    R = rng.uniform(0.5, 2, A.n) * rng.choice([-1, 1], A.n)
    L[3], R[5] = 0.0, 0.0
    for nm, l, r in (("L", L, None), ("R", None, R), ("LR", L, R)):
        v, b = M.scaled(A, l, r)
        worst["scale " + nm] = M.worst(M.scaled64(A, l, r), v, b)
    X = Csr(A.indptr, A.indices, rng.uniform(-1, 1, len(A.data)), A.n)
    for a in (-0.75, 1.0):
        v, b = M.axpy(A, a, X)
        worst[f"axpy {a}"] = M.worst(M.axpy64(A, a, X), v, b)
    for k, (w, at) in worst.items():
        print(f"MATREF cpu fs2d_p2 K {k}: worst err/bound {w:.3g} at {at}")
        assert w <= 1, (k, w, at)
    print(f"MATREF cpu fs2d_p2 K all: worst err/bound {max(w for w, _ in worst.values()):.3g}")


def test_planted_errors_are_flagged(K):
    A, Afree = K
    r = _interior_row(A)
    s, e = int(A.indptr[r]), int(A.indptr[r + 1])
    assert (e - s) % 2 == 0 and e - s >= 18  # 2x2 blocks, an interior node row
    out = {}

    # 1. one entry of one row off by 4 ulp: the entrywise export check, and the
    # product of a Dirichlet row (one stored entry: the bound is one rounding)
    k = s + int(np.argmax(np.abs(A.data[s:e])))
    bad = A.data.copy()
    for _ in range(4):
        bad[k] = np.nextafter(bad[k], np.inf)
    v, b = M.scaled(A, np.ones(A.m), None)
    assert M.worst(A.data, v, b)[0] == 0
    out["4ulp entry"] = M.worst(bad, v, b)
    dr = int(np.flatnonzero(A.row_lengths() == 1)[0])
    bad = A.data.copy()
    for _ in range(4):
        bad[A.indptr[dr]] = np.nextafter(bad[A.indptr[dr]], np.inf)
    x = M.x_signs(A, dr, 21)
    ref, bb = M.product(A, x)
    out["4ulp product"] = M.worst(Csr(A.indptr, A.indices, bad, A.n).mult(x), ref, bb)
    assert out["4ulp product"][1] == (dr,)

    # 2. the last block of a row dropped (its two columns, both component rows of the node)
    node_rows = [r - r % 2, r - r % 2 + 1]
    bad = A.data.copy()
    for rr in node_rows:
        bad[A.indptr[rr + 1] - 2:A.indptr[rr + 1]] = 0.0
    assert np.abs(A.data[e - 2:e]).max() > 0
    for nm, x in (("signs", M.x_signs(A, r, 22)), ("unit", dict(M.x_units(A))["longest"])):
        ref, bb = M.product(A, x)
        out["dropped block " + nm] = M.worst(Csr(A.indptr, A.indices, bad, A.n).mult(x), ref, bb)
        assert out["dropped block " + nm][1][0] in node_rows

    # 3. entries (a,b) and (b,a) of one block swapped.  With the whole boundary
    # fixed every block of K is symmetric to rounding (the antisymmetric part
    # of a block is a boundary term, and every free row is interior): the swap
    # is no error there.  The same mesh's K without Dirichlet rows has
    # boundary-node rows whose blocks are not symmetric; the block whose two
    # off-diagonal entries differ most is swapped.
    F = Afree
    gap, r0, kb = max((abs(F.data[F.indptr[q] + k + 1] - F.data[F.indptr[q + 1] + k]), q, k)
                      for q in range(0, F.m, 2) for k in range(0, int(F.indptr[q + 1] - F.indptr[q]), 2))
    ab, ba = F.indptr[r0] + kb + 1, F.indptr[r0 + 1] + kb
    assert gap > 1e-3 * np.abs(F.data).max(), "no block with a_ab != a_ba"
    bad = F.data.copy()
    bad[ab], bad[ba] = F.data[ba], F.data[ab]
    x = M.x_node(F.n, 2, int(F.indices[F.indptr[r0] + kb]) // 2, 23)
    ref, bb = M.product(F, x)
    assert M.worst(M.product64(F, x), ref, bb)[0] <= 1
    out["swapped block entries"] = M.worst(Csr(F.indptr, F.indices, bad, F.n).mult(x), ref, bb)
    assert out["swapped block entries"][1][0] in (r0, r0 + 1)

    # 4. a value left unscaled after diagonalScale
    rng = np.random.default_rng(24)
    L = rng.uniform(0.5, 2, A.m) * rng.choice([-1, 1], A.m)
    R = rng.uniform(0.5, 2, A.n) * rng.choice([-1, 1], A.n)
    v, b = M.scaled(A, L, R)
    bad = M.scaled64(A, L, R)
    assert M.worst(bad, v, b)[0] <= 1
    bad[e - 1] = A.data[e - 1]
    out["unscaled value"] = M.worst(bad, v, b)
    assert out["unscaled value"][1] == (e - 1,)

    # 5. an entry outside the exported pattern contributing to a product
    missing = np.setdiff1d(np.arange(A.n), A.indices[s:e])
    x = M.x_uniform(A.n, 25)
    ref, bb = M.product(A, x)
    dev = M.product64(A, x)
    assert M.worst(dev, ref, bb)[0] <= 1
    dev[r] += 1e-3 * np.abs(A.data[s:e]).max() * x[missing[0]]
    out["hidden entry"] = M.worst(dev, ref, bb)
    # ... and on a Dirichlet row, whose export is the diagonal alone
    dev = M.product64(A, x)
    dev[dr] += 1e-9 * x[(dr + 1) % A.n]
    out["hidden entry, Dirichlet row"] = M.worst(dev, ref, bb)

    for k, (wv, at) in out.items():
        print(f"MATREF cpu fs2d_p2 K planted {k}: err/bound {wv:.3g} at {at}")
        assert wv > 1, (k, wv, at)
