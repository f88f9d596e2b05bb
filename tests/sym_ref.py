"""Host references for the symmetric-storage SpMV (kle_brick.hip, kle_sym.hip,
kle_gbrick.hip), no GPU.

Everything works on a K exported by ``getValuesCSR()`` (3 dofs per node, dof
3 j + b of node j) wrapped in ``krylov_ref.Csr``.  The reference of a product
is ``A.mult(x.astype(longdouble))``; its rows are scaled by
``den = A.abs_mult(x)`` = (|K||x|)_i, the scale of every rounding bound of a
row sum, so one wrong stored entry shows in its own row however small that
row is against the rest of y.

The symmetric storages keep the blocks B_ij = K[3i:3i+3, 3j:3j+3], j >= i.
Row i's *direct* sum, sum_{j >= i} B_ij x_j, is fp64.  Its *transposed* sum,
sum_{j < i} B_ji^T x_j, is an int64 fixed-point sum: each term
t = B_ji^T x_j (three fp64 products) enters as rint(t / q), q = 2^(E-61), with
2^E > bound x max|x| per brick / tile / group.  A term is therefore off by at
most q/2 and row i, into which nT_i node blocks are transposed, by nT_i q/2
on top of the fp64 roundings.

  scaled_err / restatement    the component-wise error and its fp64 yardstick
  brick_quantum               q and nT_i of a one-brick decomposition
                              (k_brick_bound restated)
  apriori_quantum             q <= 2^-57 ||K||inf ||x||inf for every storage
  uniform / ramp / spike / sign_adversarial / subnormal / comb / comb_greedy
                              seeded inputs
"""
import numpy as np

from krylov_ref import LD, Csr

U = 2.0 ** -53  # unit roundoff of fp64
DBL_MAX = np.finfo(np.float64).max


# ------------------------------------------------------------------ errors
def abs_mult(A, x):
    """(|K||x|)_i in longdouble (Csr.abs_mult with the cached longdouble data)."""
    if A._data_ld is None:
        A._data_ld = A.data.astype(LD)
    return A._rowsum(np.abs(A._data_ld * np.asarray(x, dtype=LD)[A.indices]))


def _rows(A):
    if getattr(A, "_row_of", None) is None:
        A._row_of = np.repeat(np.arange(A.m), np.diff(A.indptr))
    return A._row_of


def reference(A, x):
    """(ref, den): K x in longdouble and (|K||x|)_i.  (A mostly zero x, the
    combs: only the entries that meet a nonzero.)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        if 8 * np.count_nonzero(x) > len(x):
            return A.mult(x.astype(LD)), abs_mult(A, x)
        sel = np.flatnonzero(x[A.indices] != 0)
        prod = A.data[sel].astype(LD) * x[A.indices[sel]].astype(LD)
        ref, den = np.zeros(A.m, LD), np.zeros(A.m, LD)
        np.add.at(ref, _rows(A)[sel], prod)
        np.add.at(den, _rows(A)[sel], np.abs(prod))
        return ref, den


def scaled_err(y, ref, den):
    """max_i |y_i - ref_i| / den_i over the rows with den_i > 0.  Rows with
    den_i == 0 (every product of the row vanishes) must hold y_i == 0 exactly."""
    y = np.asarray(y)
    on = den > 0
    assert not np.any(y[~on] != 0), "a row without a nonzero product is not exactly 0"
    if not on.any():
        return 0.0
    return float((np.abs(y[on].astype(LD) - ref[on]) / den[on]).max())


def restatement(A, x, ref=None, den=None):
    """scaled_err of the fp64 ``A.mult(x)``: how far fp64 rounding alone moves
    the product -- the yardstick of the device's direct sums."""
    if ref is None:
        ref, den = reference(A, x)
    with np.errstate(all="ignore"):
        return scaled_err(A.mult(np.asarray(x, dtype=np.float64)), ref, den)


def asymmetry(A):
    """(pattern symmetric, entries with K_ij != K_ji, max |K_ij - K_ji| / max(|K_ij|, |K_ji|))."""
    rows = _rows(A)
    o = np.lexsort((rows, A.indices))  # the transpose's entries in CSR order
    if not (A.m == A.n and np.array_equal(A.indices[o], rows) and np.array_equal(rows[o], A.indices)):
        return False, -1, np.inf
    d, t = A.data, A.data[o]
    ne = d != t
    rel = float((np.abs(d[ne] - t[ne]) / np.maximum(np.abs(d[ne]), np.abs(t[ne]))).max()) if ne.any() else 0.0
    return True, int(ne.sum()), rel


def is_symmetric(A):
    """K == K^T entry for entry (pattern and bits)."""
    return asymmetry(A)[:2] == (True, 0)


def identity_rows(A):
    """Dirichlet rows: one entry, on the diagonal, equal to 1."""
    one = np.flatnonzero(np.diff(A.indptr) == 1)
    p = A.indptr[one]
    return one[(A.indices[p] == one) & (A.data[p] == 1.0)]


def norm_inf(A):
    return float(A._rowsum(np.abs(A.data)).max())


# ------------------------------------------------------------ the quantum
def _lower_blocks(A):
    """The entries K[3j+b, 3i+a] = B_ij[a][b] of the node blocks below the
    diagonal (i < j) -- the blocks transposed into node j.  Returns
    (sel, pid, pj, npairs): the entries, each entry's pair (j, i) and every
    pair's node j."""
    rows = _rows(A)
    nj, ni = rows // 3, A.indices // 3
    sel = np.flatnonzero(ni < nj)
    nn = (A.m + 2) // 3
    key, pid = np.unique(nj[sel] * nn + ni[sel], return_inverse=True)
    return sel, pid, key // nn, len(key)


def transposed_bound(A):
    """Per node j: (lower_j, upper_j, nT_j) with
    lower_j = sum over the lower-neighbour nodes i of max_b sum_a |B_ij[a][b]|
              (each transposed term's component is <= that x max|x|),
    upper_j = max_a of the abs sum of row 3j+a's stored entries (its direct sum),
    nT_j    = the number of node blocks transposed into node j."""
    if getattr(A, "_tbound", None) is not None:
        return A._tbound
    nn = (A.m + 2) // 3
    rows = _rows(A)
    sel, pid, pj, npairs = _lower_blocks(A)
    s = np.zeros((npairs, 3))
    np.add.at(s, (pid, rows[sel] % 3), np.abs(A.data[sel]))
    lower = np.bincount(pj, weights=s.max(axis=1), minlength=nn)
    nT = np.bincount(pj, minlength=nn)
    up = np.flatnonzero(A.indices // 3 >= rows // 3)
    rs = np.bincount(rows[up], weights=np.abs(A.data[up]), minlength=3 * nn)
    upper = rs.reshape(nn, 3).max(axis=1)
    A._tbound = (lower, upper, nT)
    return A._tbound


def _pow2(e):
    return np.ldexp(LD(1), int(e))  # (longdouble: exponents down to -16445)


def brick_quantum(A, x):
    """(q, nT_i) of a one-brick decomposition: k_brick_bound restated.  The
    brick's bound is max_j (lower_j + upper_j) (transposed_bound), the kernel
    takes E = frexp(bound) + frexp(max|x|) clamped to [-1070, 1020] and sums
    rint(t 2^(61-E)); q = 2^(E-61).  nT_i per row (dof) of K."""
    lower, upper, nT = transposed_bound(A)
    bound = float((lower + upper).max())
    xm = float(np.abs(x).max())
    if not (bound > 0 and xm > 0):
        return LD(0), np.repeat(nT, 3)[: A.m]
    E = int(np.frexp(bound)[1]) + int(np.frexp(xm)[1])
    E = min(max(E, -1070), 1020)
    return _pow2(E - 61), np.repeat(nT, 3)[: A.m]


def apriori_quantum(A, x):
    """(q, nT_i) with q an upper bound of every storage's quantum, for planned
    decompositions whose per-part scales the test does not know.

    Box bricks (k_brick_bound): the bound of a brick is, over its region nodes
    j, sum_i max_b sum_a |B_ij[a][b]| over some lower neighbours i, plus the
    largest abs row sum of j's stored entries.  By symmetry
    sum_a |B_ij[a][b]| is the part of row 3j+b of |K| in node i's columns, so
    sum_i max_b (.) <= sum_b sum_i (.) <= 3 ||K||inf, and the direct part is
    <= ||K||inf: bound <= 4 ||K||inf.
    128-row tiles (k_sym_bound) and 64-row groups (k_gsym_bound): the same sum
    over the tile's / group's rows, without the direct part: <= 3 ||K||inf.
    Graph bricks (k_gbrick_bound): that sum with every term rounded up to a
    multiple of 2^-sh, 3 max|K_ij| < 2^(50-sh), and one ulp for the
    conversion: <= 3 ||K||inf (1 + n 2^-50 + 2^-50) with n < 2^12 terms
    per entry, < 4 ||K||inf.
    Every kernel then takes 2^eb > bound by frexp, so 2^eb <= 2 bound
    <= 8 ||K||inf, and 2^em > max|x| over (a part of) x the same way,
    2^em <= 2 ||x||inf.  E = eb + em: 2^E <= 16 ||K||inf ||x||inf and
    q = 2^(E-61) <= 2^-57 ||K||inf ||x||inf.
    (The kernels clamp E to an exponent range; inside it the bound holds, and
    below it the storage would flush sums that fp64 keeps -- the subnormal
    inputs test that it does not.)"""
    _, _, nT = transposed_bound(A)
    q = _pow2(-57) * LD(norm_inf(A)) * LD(np.abs(x).max())
    return q, np.repeat(nT, 3)[: A.m]


# ---------------------------------------------------------------- inputs
def uniform(n, seed=0):
    return np.random.default_rng(1000 + seed).uniform(-1.0, 1.0, n)


def ramp(n, decades=6, seed=0):
    """|x| falling `decades` decades along the index, random signs and
    mantissas: the quantum follows the largest entries, the small ones' rows
    see it."""
    rng = np.random.default_rng(2000 + seed)
    return rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n) * 10.0 ** (-decades * np.arange(n) / max(n - 1, 1))


def spike(n, at=None, big=1e8, seed=0):
    """O(1) entries and one of size `big` at index `at` (default: the middle)."""
    x = np.random.default_rng(3000 + seed).uniform(-1.0, 1.0, n)
    x[n // 2 if at is None else at] = big
    return x


def sign_adversarial(A, seed=0):
    """x = the signs of the lower part of the row with the largest lower abs
    sum in the node with the largest transposed bound (random signs
    elsewhere): that row's transposed sum is sum |K_ij|, the most a region sum
    can reach with max|x| = 1."""
    lower, _, _ = transposed_bound(A)
    j = int(np.argmax(lower))
    rows = np.repeat(np.arange(A.m), np.diff(A.indptr))
    low = (A.indices // 3 < rows // 3)
    ls = np.bincount(rows[low], weights=np.abs(A.data[low]), minlength=A.m)
    r = 3 * j + int(np.argmax(ls[3 * j:3 * j + 3]))
    x = np.random.default_rng(4000 + seed).choice([-1.0, 1.0], A.n)
    p = np.arange(A.indptr[r], A.indptr[r + 1])
    p = p[A.indices[p] // 3 < j]
    x[A.indices[p]] = np.where(A.data[p] < 0, -1.0, 1.0)
    return x


def subnormal(n, seed=0):
    """Entries k x 5e-324 (the smallest subnormal), |k| in [1, 2^20]."""
    rng = np.random.default_rng(5000 + seed)
    k = rng.integers(1, 1 << 20, n) * rng.choice([-1, 1], n)
    return k.astype(np.float64) * 5e-324


def comb(dims, P, offset, comp, seed=0):
    """A box lattice (dims = nodes per axis, x fastest) of elements of order
    P: component `comp` of the nodes offset + (2P+1) Z^3, magnitudes in
    [0.5, 2], 0 elsewhere.  A node couples to nodes at most P away per axis,
    so no row meets two comb nodes: y_i is the single product K_ij x_j."""
    Lx, Ly, Lz = dims
    s = 2 * P + 1
    ox, oy, oz = (int(o) % s for o in offset)
    gx, gy, gz = np.meshgrid(np.arange(ox, Lx, s), np.arange(oy, Ly, s), np.arange(oz, Lz, s), indexing="ij")
    nodes = (gx + Lx * (gy + Ly * gz)).ravel()
    rng = np.random.default_rng(6000 + seed)
    x = np.zeros(3 * Lx * Ly * Lz)
    x[3 * nodes + comp] = rng.uniform(0.5, 2.0, len(nodes)) * rng.choice([-1.0, 1.0], len(nodes))
    return x


def comb_greedy(A, comp, seed=0):
    """The comb of a mesh without a lattice: nodes taken in a seeded random
    order, each kept if none of its rows (= its columns, K symmetric) meets a
    node kept before."""
    nn = A.m // 3
    rng = np.random.default_rng(7000 + seed)
    taken = np.zeros(nn, bool)
    x = np.zeros(A.n)
    for j in rng.permutation(nn):
        nb = A.indices[A.indptr[3 * j]:A.indptr[3 * j + 3]] // 3
        if not taken[nb].any():
            taken[nb] = True
            x[3 * j + comp] = rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0])
    return x


def terms_per_row(A, x):
    """The number of nonzero products K_ij x_j of each row."""
    return A._rowsum((np.asarray(x)[A.indices] != 0).astype(np.int64) * (A.data != 0))


COMB_CASES = 6
COMB_ALL = 125  # up to this many offsets, (2P+1)^3: every one of them


def comb_inputs(A, dims=None, P=None, seed=0):
    """The combs of a mesh: on a lattice of order P <= 2 one comb per offset
    (27 or 125: every node is in one of them, so no stored block escapes),
    otherwise COMB_CASES combs with seeded random offsets (a lattice where
    dims is given, the greedy comb otherwise); the components cycle first,
    then are random."""
    rng = np.random.default_rng(8000 + seed)
    out = {}
    if dims is not None and (2 * P + 1) ** 3 <= COMB_ALL:
        s = 2 * P + 1
        for k in range(s ** 3):
            out[f"comb{k}"] = comb(dims, P, (k % s, (k // s) % s, k // (s * s)), k % 3, seed=seed + k)
        return out
    for k in range(COMB_CASES):
        comp = k % 3 if k < 3 else int(rng.integers(3))
        if dims is not None:
            off = rng.integers(0, 2 * P + 1, 3)
            out[f"comb{k}"] = comb(dims, P, off, comp, seed=seed + k)
        else:
            out[f"comb{k}"] = comb_greedy(A, comp, seed=seed + k)
    return out


def inputs(A, dims=None, P=None, seed=0):
    """Every input maker on K, by name."""
    n = A.n
    out = {"uniform": uniform(n, seed), "ramp": ramp(n, 6, seed), "spike": spike(n, None, 1e8, seed),
           "sign_adversarial": sign_adversarial(A, seed), "subnormal": subnormal(n, seed)}
    out.update(comb_inputs(A, dims, P, seed))
    return out


# ------------------------------------------------- the brick arithmetic
def emulate_one_brick(A, x, q):
    """The arithmetic of one brick on the host: the direct part (stored
    entries, j >= i) as an fp64 row sum, every transposed term
    t = sum_a B_ij[a][b] x_i[a] in fp64, rint(t / q) summed in int64, the sum
    back to fp64 (one rounding) times q, added to the direct part."""
    x = np.asarray(x, dtype=np.float64)
    rows = np.repeat(np.arange(A.m), np.diff(A.indptr))
    with np.errstate(all="ignore"):
        prod = A.data * x[A.indices]
        up = A.indices // 3 >= rows // 3
        direct = np.zeros(A.m)
        # (sequential fp64 sums per row, in column order)
        np.add.at(direct, rows[up], prod[up])
        sel, pid, pj, npairs = _lower_blocks(A)
        t = np.zeros((npairs, 3))
        np.add.at(t, (pid, rows[sel] % 3), prod[sel])
        if q == 0:
            return direct
        ti = np.rint(t.astype(LD) / q)
        assert np.abs(ti).max() < 2.0 ** 61
        acc = np.zeros((A.m + 2) // 3 * 3, np.int64).reshape(-1, 3)
        np.add.at(acc, pj, ti.astype(np.int64))
        assert np.abs(acc).max() < 2 ** 61, "a region sum past 2^61: the bound is too small"
        tr = (acc.ravel()[: A.m].astype(np.float64).astype(LD) * q).astype(np.float64)
        return direct + tr


def as_csr(ip, ix, d):
    return Csr(ip, ix, d, len(ip) - 1)
