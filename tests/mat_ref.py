"""Longdouble restatements of the Mat surface (kle_mat.hip: mult, multAdd,
diagonalScale, axpy, Mat + Mat, getDiagonal) on an exported CSR, no GPU and no
project import.

Everything starts from the fp64 data of an export (indptr, indices, data) and
is evaluated in ``np.longdouble`` (64-bit mantissa); every function returns
the reference together with a bound on what fp64 evaluation may differ from
it by, counted in roundings of u = 2^-53 with the 1.01 slack of elem_ref and
sym_ref (it covers the second-order terms and the reference's own 2^-64):

  product    row sums; 1.01 n_i u sum_k |a_ik| |x_k|, n_i the stored entries
             of row i (explicit zeros included): n_i products and n_i - 1
             additions in any order, fused or not, are n_i roundings at most
             on every term.  A stored zero adds an exact 0, so kernels that
             also sum stored zeros outside the export stay inside it; an empty
             row is exactly 0.
  mult_add   y + ref: one more rounding of the result.
  scaled     a_ij L_i R_j per entry: the kernels form s = L_i R_j (exact with
             one factor, one rounding with both), then a s (one rounding).
  axpy       y + a x per entry of Y's pattern, X's a subset: a x and the sum,
             one rounding each (or one in all when fused); an entry X does not
             hold stays exactly y.
  union_sum  Mat + Mat on different patterns: y + x, one rounding, on the
             union; an entry only one holds is exact.
  diagonal   the stored diagonal, 0 where a row holds none or beyond min(m, n).
  worst      largest err / bound and where (bound 0: must be equal).

The x_* functions build the input vectors of the GPU tests; each class exists
because a kind of kernel error hides from a uniform random x in a max-norm:

  x_uniform  U(-1, 1): the baseline.
  x_scales   +-10^U(-6, 6): a small row next to large ones -- an error
             relative to the largest row passes a norm, not a row bound.
  x_signs    x_k = sign(a_ik) on a chosen row, random signs elsewhere: that
             row's sum is sum |a|, nothing cancels, so a lost or doubled term
             cannot hide in the cancellation.
  x_units    unit vectors at the first column, the last column and the last
             column of the longest row: one entry per row, the bound collapses
             to n_i u |a_ij| -- a wrong column or a lost tail block shows.
  x_node     zero except one node's C components: block-internal transposes.

The *64 functions restate the same operations in plain fp64 numpy: the
"device" of the CPU test, whose err / bound is the baseline the device
figures are read against.
"""
import numpy as np

from krylov_ref import LD, Csr

U = 2.0 ** -53
SLACK = 1.01


def as_csr(csr, ncols=None):
    """A krylov_ref.Csr from a Csr or an (indptr, indices, data) triple."""
    if isinstance(csr, Csr):
        return csr
    return Csr(csr[0], csr[1], csr[2], ncols)


def rows_of(csr):
    """Row index of every stored entry."""
    A = as_csr(csr)
    return np.repeat(np.arange(A.m), A.row_lengths())


def product(csr, x):
    """(A x in longdouble, per-row bound)."""
    A = as_csr(csr)
    x = np.asarray(x, dtype=LD)
    ref = A.mult(x)
    bound = (SLACK * U * A.row_lengths().astype(LD) * A.abs_mult(x)).astype(np.float64)
    return ref, bound


def mult_add(ref, bound, y):
    """z = y + A x from product()'s pair: one more rounding, of the result."""
    z = np.asarray(y, dtype=LD) + ref
    return z, bound + (SLACK * U * np.abs(z)).astype(np.float64)


def scaled(csr, L=None, R=None):
    """(a_ij L_i R_j in longdouble, per-entry bound) on the pattern of csr."""
    A = as_csr(csr)
    v = A.data.astype(LD)
    if L is not None:
        v = v * np.asarray(L, dtype=LD)[rows_of(A)]
    if R is not None:
        v = v * np.asarray(R, dtype=LD)[A.indices]
    roundings = 2 if (L is not None and R is not None) else 1
    return v, (roundings * SLACK * U * np.abs(v)).astype(np.float64)


def _positions(Y, X):
    """Index into Y's entries of every entry of X (X's pattern within Y's)."""
    assert Y.m == X.m
    stride = max(Y.n, X.n, int(Y.indices.max(initial=0)) + 1, int(X.indices.max(initial=0)) + 1)
    ky = rows_of(Y) * stride + Y.indices
    kx = rows_of(X) * stride + X.indices
    pos = np.searchsorted(ky, kx)  # (columns ascend within a row: ky is sorted)
    ok = (pos < len(ky)) & (ky[np.minimum(pos, max(len(ky) - 1, 0))] == kx) if len(ky) else np.zeros(len(kx), bool)
    return pos, ok


def is_subset(csrY, csrX):
    """Whether X's pattern lies within Y's."""
    return bool(_positions(as_csr(csrY), as_csr(csrX))[1].all())


def axpy(csrY, a, csrX):
    """(y + a x in longdouble, per-entry bound) on Y's pattern; X's pattern
    equal to Y's or a subset of it."""
    Y, X = as_csr(csrY), as_csr(csrX)
    pos, ok = _positions(Y, X)
    assert ok.all(), "X's pattern is not within Y's"
    ax = np.zeros(len(Y.data), dtype=LD)
    ax[pos] = LD(a) * X.data.astype(LD)
    held = np.zeros(len(Y.data), bool)
    held[pos] = True
    ref = Y.data.astype(LD) + ax
    bound = np.where(held, (SLACK * U * (np.abs(ax) + np.abs(ref))).astype(np.float64), 0.0)
    return ref, bound


def union_sum(csrY, csrX):
    """Mat + Mat on the union pattern: (indptr, indices, y + x in longdouble,
    per-entry bound); Y's entry first, then X's, one rounding."""
    Y, X = as_csr(csrY), as_csr(csrX)
    assert Y.m == X.m
    stride = max(Y.n, X.n, int(Y.indices.max(initial=0)) + 1, int(X.indices.max(initial=0)) + 1)
    ky = rows_of(Y) * stride + Y.indices
    kx = rows_of(X) * stride + X.indices
    keys = np.union1d(ky, kx)
    vy = np.zeros(len(keys), dtype=LD)
    vx = np.zeros(len(keys), dtype=LD)
    both = np.zeros(len(keys), np.int64)
    py, px = np.searchsorted(keys, ky), np.searchsorted(keys, kx)
    vy[py] = Y.data
    vx[px] = X.data
    both[py] += 1
    both[px] += 1
    ref = vy + vx
    bound = np.where(both == 2, (SLACK * U * np.abs(ref)).astype(np.float64), 0.0)
    indptr = np.zeros(Y.m + 1, np.int64)
    np.add.at(indptr, keys // stride + 1, 1)
    return np.cumsum(indptr), keys % stride, ref, bound


def diagonal(csr):
    """The stored diagonal (fp64, exact): 0 where the row holds none, 0 beyond min(m, n)."""
    return as_csr(csr).diagonal()


def worst(dev, ref, bound):
    """Largest |dev - ref| / bound and its position; entries with bound 0 must
    be equal (their ratio counts as inf when they are not)."""
    err = np.abs(np.asarray(dev).astype(LD) - ref).astype(np.float64)
    b = np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1), np.where(err > 0, np.inf, 0.0))
    k = np.unravel_index(np.argmax(ratio), ratio.shape) if ratio.size else ()
    return (float(ratio[k]) if ratio.size else 0.0), tuple(int(i) for i in k)


# ------------------------------------------------------------ input vectors
def x_uniform(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def x_scales(n, seed):
    rng = np.random.default_rng(seed)
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6.0, 6.0, n)


def x_signs(csr, row, seed):
    A = as_csr(csr)
    x = np.random.default_rng(seed).choice([-1.0, 1.0], A.n)
    s, e = A.indptr[row], A.indptr[row + 1]
    x[A.indices[s:e]] = np.where(A.data[s:e] < 0, -1.0, 1.0)
    return x


def longest_row(csr):
    A = as_csr(csr)
    return int(np.argmax(A.row_lengths())) if A.m else 0


def x_units(csr):
    """[(name, e_j)]: first column, last column, last column of the longest row."""
    A = as_csr(csr)
    cols = [("first", 0), ("last", A.n - 1)]
    r = longest_row(A)
    if A.m and A.indptr[r + 1] > A.indptr[r]:
        cols.append(("longest", int(A.indices[A.indptr[r + 1] - 1])))
    out = []
    for name, j in cols:
        x = np.zeros(A.n)
        x[j] = 1.0
        out.append((name, x))
    return out


def x_node(n, C, node, seed):
    x = np.zeros(n)
    x[node * C:(node + 1) * C] = np.random.default_rng(seed).uniform(0.5, 2.0, C) * np.array([1.0, -1.0, 1.0, -1.0, 1.0, -1.0])[:C]
    return x


def input_vectors(csr, C=1, seed=0):
    """[(class name, x)] of classes (a)-(e) for one matrix; the sign vector is
    built for the longest row and for the shortest non-empty one."""
    A = as_csr(csr)
    lens = A.row_lengths()
    out = [("uniform", x_uniform(A.n, seed)), ("scales", x_scales(A.n, seed + 1))]
    if A.m and lens.max() > 0:
        short = int(np.flatnonzero(lens > 0)[np.argmin(lens[lens > 0])])
        out.append(("signs_longest", x_signs(A, longest_row(A), seed + 2)))
        out.append(("signs_shortest", x_signs(A, short, seed + 3)))
    out += [("unit_" + nm, x) for nm, x in x_units(A)]
    nodes = A.n // C
    out.append(("node", x_node(A.n, C, (seed * 7 + nodes // 2) % max(nodes, 1), seed + 4)))
    return out


# ------------------------------------------------- fp64 restatements ("device")
def product64(csr, x):
    return as_csr(csr).mult(np.asarray(x, dtype=np.float64))


def scaled64(csr, L=None, R=None):
    A = as_csr(csr)
    s = np.ones(len(A.data))
    if L is not None:
        s = s * np.asarray(L, np.float64)[rows_of(A)]
    if R is not None:
        s = s * np.asarray(R, np.float64)[A.indices]
    return A.data * s


def axpy64(csrY, a, csrX):
    Y, X = as_csr(csrY), as_csr(csrX)
    pos, ok = _positions(Y, X)
    assert ok.all()
    out = Y.data.copy()
    out[pos] = out[pos] + float(a) * X.data
    return out
