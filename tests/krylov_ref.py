"""Plain numpy references for the Krylov layer (kle_ksp.hip), no GPU.

Everything is generic in its dtype: run in ``np.longdouble`` (64-bit mantissa,
eps 1.1e-19) an iteration is the reference; the same code in ``np.float64`` is
an fp64 *restatement*, whose distance from the reference measures how far
fp64 rounding alone moves that recurrence -- the yardstick the GPU tests scale
their tolerances by (tests/test_gpu_krylov.py).

  Csr                      host CSR + a mat-vec in the dtype of its argument
  sym_tridiag / convdiff   the matrix families of the GPU tests (seeded)
  cg_classic / cg_single_reduction / cg_pipelined
                           the three CG recurrences of the device, zero start,
                           PC none or Jacobi; every iterate x_k and ||r_k||
  pcg_reference            cg_classic in longdouble (the three are one
                           iteration in exact arithmetic)
  gmres                    right-preconditioned GMRES(m), CGS2 + Givens, the
                           stopping decisions of solve_gmres
  thomas                   tridiagonal solve in longdouble
  gap_threshold            a threshold in a gap of a residual history
"""
import math
from functools import lru_cache

import numpy as np

LD = np.longdouble

# converged reasons (include/kle.h)
RTOL, ATOL, ITS_OK, DIV_ITS, DIV_DTOL, DIV_INDEFINITE, DIV_NAN = 2, 3, 4, -3, -4, -8, -9


class Csr:
    """Host CSR (int64 indptr / indices, float64 data)."""

    def __init__(self, indptr, indices, data, ncols=None):
        self.indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        self.indices = np.ascontiguousarray(indices, dtype=np.int64)
        self.data = np.ascontiguousarray(data, dtype=np.float64)
        self.m = len(self.indptr) - 1
        self.n = self.m if ncols is None else int(ncols)
        self._rows = np.flatnonzero(np.diff(self.indptr) > 0)
        self._data_ld = None

    @property
    def csr(self):
        return self.indptr, self.indices, self.data

    def _rowsum(self, prod):
        out = np.zeros(self.m, dtype=prod.dtype)
        if len(self._rows):
            out[self._rows] = np.add.reduceat(prod, self.indptr[self._rows])
        return out  # (an empty row: exactly 0)

    def mult(self, x):
        """A x in the dtype of x (longdouble x: every product and sum in longdouble)."""
        x = np.asarray(x)
        if x.dtype == LD:
            if self._data_ld is None:
                self._data_ld = self.data.astype(LD)
            return self._rowsum(self._data_ld * x[self.indices])
        return self._rowsum(self.data * x[self.indices])

    def abs_mult(self, x):
        """sum_j |a_ij x_j| in longdouble (the scale of a row's rounding bound)."""
        return self._rowsum(np.abs(self.data.astype(LD) * np.asarray(x, dtype=LD)[self.indices]))

    def diagonal(self):
        d = np.zeros(self.m)
        rows = np.repeat(np.arange(self.m), np.diff(self.indptr))
        on = rows == self.indices
        d[rows[on]] = self.data[on]
        return d

    def row_lengths(self):
        return np.diff(self.indptr)


def tridiag(lower, diag, upper):
    """CSR of tridiag(lower, diag, upper); lower[i] = a(i+1, i), upper[i] = a(i, i+1)."""
    n = len(diag)
    rows = np.concatenate([np.arange(1, n), np.arange(n), np.arange(n - 1)])
    cols = np.concatenate([np.arange(n - 1), np.arange(n), np.arange(1, n)])
    vals = np.concatenate([lower, diag, upper]).astype(np.float64)
    order = np.lexsort((cols, rows))
    indptr = np.zeros(n + 1, np.int64)
    np.add.at(indptr, rows + 1, 1)
    return Csr(np.cumsum(indptr), cols[order], vals[order])


def sym_tridiag(n):
    """The CG family: diagonal 3 + U(0,2), off-diagonal -1 + 0.2 U(-1,1),
    b = U(-1,1); SPD by diagonal dominance, condition < 7, and the varying
    diagonal makes Jacobi differ from PC none.  Returns (A, b)."""
    rng = np.random.default_rng(20000 + n)
    d = 3.0 + rng.uniform(0.0, 2.0, n)
    e = -1.0 + 0.2 * rng.uniform(-1.0, 1.0, max(n - 1, 0))
    b = rng.uniform(-1.0, 1.0, n)
    return tridiag(e, d, e), b


def convdiff(n, c=0.5):
    """The GMRES family: non-symmetric tridiag(-1-c, d_i, -1+c), d_i = 3 + U(0,2).
    Its symmetric part is tridiag(-1, d_i, -1) >= I, so ||A^-1||_2 <= 1.
    Returns (A, b, lower, diag, upper)."""
    rng = np.random.default_rng(30000 + n)
    d = 3.0 + rng.uniform(0.0, 2.0, n)
    lo = np.full(max(n - 1, 0), -1.0 - c)
    up = np.full(max(n - 1, 0), -1.0 + c)
    b = rng.uniform(-1.0, 1.0, n)
    return tridiag(lo, d, up), b, lo, d, up


def _dot(a, b):
    return (a * b).sum()  # (pairwise summation)


def _minv(A, pc, dtype):
    if pc == "none":
        return None
    assert pc == "jacobi", pc
    d = A.diagonal().astype(dtype)
    return np.where(d != 0, dtype(1) / np.where(d != 0, d, 1), dtype(1))  # (k_invert_diag)


def _apply(minv, r):
    return r.copy() if minv is None else minv * r


def cg_classic(A, b, pc, iters, dtype=np.float64):
    """Hestenes-Stiefel PCG, zero start.  Returns (xs, rns): x_0 .. x_K and
    ||r_0|| .. ||r_K|| (K = iters, or where the residual vanished)."""
    with np.errstate(all="ignore"):
        b = np.asarray(b, dtype=dtype)
        minv = _minv(A, pc, dtype)
        x = np.zeros_like(b)
        r = b.copy()
        z = _apply(minv, r)
        p = z.copy()
        rz = _dot(r, z)
        xs, rns = [x.copy()], [np.sqrt(_dot(r, r))]
        for _ in range(iters):
            q = A.mult(p)
            pq = _dot(p, q)
            if not pq > 0:
                break
            alpha = rz / pq
            x = x + alpha * p
            r = r - alpha * q
            xs.append(x.copy())
            rns.append(np.sqrt(_dot(r, r)))
            z = _apply(minv, r)
            rz_new = _dot(r, z)
            beta = rz_new / rz
            rz = rz_new
            p = z + beta * p
    return xs, rns


def cg_single_reduction(A, b, pc, iters, dtype=np.float64):
    """Chronopoulos-Gear CG as the device runs it (k_sr_start, k_sr_iter,
    sr_step): beta = g / rho_prev, alpha = g / (d - beta g / alpha_prev)."""
    with np.errstate(all="ignore"):
        b = np.asarray(b, dtype=dtype)
        minv = _minv(A, pc, dtype)
        x = np.zeros_like(b)
        r = b.copy()
        u = _apply(minv, r)
        w = A.mult(u)
        p = np.zeros_like(b)
        s = np.zeros_like(b)
        g, d = _dot(r, u), _dot(w, u)
        rho, alpha, beta = g, g / d, dtype(0)
        xs, rns = [x.copy()], [np.sqrt(_dot(r, r))]
        for _ in range(iters):
            if not np.isfinite(alpha):
                break
            p = u + beta * p
            s = w + beta * s
            x = x + alpha * p
            r = r - alpha * s
            u = _apply(minv, r)
            w = A.mult(u)
            xs.append(x.copy())
            rns.append(np.sqrt(_dot(r, r)))
            g, d = _dot(r, u), _dot(w, u)
            beta = g / rho
            alpha = g / (d - beta * g / alpha)
            rho = g
    return xs, rns


def cg_pipelined(A, b, pc, iters, dtype=np.float64):
    """Ghysels-Vanroose pipelined CG as the device runs it (k_pipe_init,
    k_pipe_iter): u, w, m by recurrence, the scalar stage of sr_step."""
    with np.errstate(all="ignore"):
        b = np.asarray(b, dtype=dtype)
        minv = _minv(A, pc, dtype)
        x = np.zeros_like(b)
        r = b.copy()
        u = _apply(minv, r)
        w = A.mult(u)
        g, d = _dot(r, u), _dot(w, u)
        rho, alpha, beta = g, g / d, dtype(0)
        m = _apply(minv, w)
        nv = A.mult(m)
        z, q, s, p = (np.zeros_like(b) for _ in range(4))
        xs, rns = [x.copy()], [np.sqrt(_dot(r, r))]
        for _ in range(iters):
            if not np.isfinite(alpha):
                break
            z = nv + beta * z
            q = m + beta * q
            s = w + beta * s
            p = u + beta * p
            x = x + alpha * p
            r = r - alpha * s
            u = u - alpha * q
            w = w - alpha * z
            m = _apply(minv, w)
            xs.append(x.copy())
            rns.append(np.sqrt(_dot(r, r)))
            g, d = _dot(r, u), _dot(w, u)
            nv = A.mult(m)
            beta = g / rho
            alpha = g / (d - beta * g / alpha)
            rho = g
    return xs, rns


RECURRENCES = {"cg": cg_classic, "sr": cg_single_reduction, "pipecg": cg_pipelined}


def pcg_reference(A, b, pc, iters):
    """The reference of all three device variants: PCG in longdouble."""
    return cg_classic(A, b, pc, iters, dtype=LD)


def history_error(xs, rns, ref_xs, ref_rns, rn_floor):
    """(ex, er) of a history against the reference's: the largest
    max|x_k - ref_k| / max|ref_k| over k >= 1, and the largest
    | ||r_k|| - ref | / ref over the k >= 1 whose reference norm is >= rn_floor."""
    ex = er = 0.0
    for k in range(1, min(len(xs), len(ref_xs))):
        ex = max(ex, float(np.abs(xs[k].astype(LD) - ref_xs[k]).max() / np.abs(ref_xs[k]).max()))
        if ref_rns[k] >= rn_floor:
            er = max(er, float(abs(LD(rns[k]) - ref_rns[k]) / ref_rns[k]))
    return ex, er


def gmres(A, b, pc, restart, rtol, atol=1e-50, dtol=1e5, maxit=10000, dtype=np.float64):
    """Right-preconditioned GMRES(restart), zero start, two passes of classical
    Gram-Schmidt, Givens rotations, the residual re-formed at every restart --
    statement for statement the decisions of solve_gmres: NaN/Inf, converged
    (max(rtol ||b||, atol)), dtol ||b||, at iteration 0, at every iteration's
    estimate and at every restart's true residual; hn == 0 ends the cycle.
    Returns dict(x, its, reason, rn, hist=[(its, estimate, x)])."""
    b = np.asarray(b, dtype=dtype)
    n, m = len(b), restart
    minv = _minv(A, pc, dtype)
    x = np.zeros_like(b)
    bn = np.sqrt(_dot(b, b))
    tol = max(dtype(rtol) * bn, dtype(atol))

    def stop(v):
        if not np.isfinite(v):
            return DIV_NAN
        if v <= tol:
            return ATOL if v <= atol else RTOL
        if v >= dtype(dtol) * bn:
            return DIV_DTOL
        return 0

    its, hist = 0, []
    reason, rn = stop(bn), bn
    if reason:
        return dict(x=x, its=0, reason=reason, rn=rn, hist=hist, bn=bn)
    while True:
        r = b - A.mult(x)
        rn = np.sqrt(_dot(r, r))
        reason = stop(rn)
        if reason:
            break
        V = np.zeros((m + 1, n), dtype=dtype)
        V[0] = r * (dtype(1) / rn)
        H = np.zeros((m + 1, m), dtype=dtype)
        cs, sn, gv = np.zeros(m, dtype), np.zeros(m, dtype), np.zeros(m + 1, dtype)
        gv[0] = rn
        j = 0

        def iterate(jj):
            y = np.zeros(jj, dtype=dtype)
            for i in range(jj - 1, -1, -1):
                y[i] = (gv[i] - _dot(H[i, i + 1:jj], y[i + 1:])) / H[i, i]
            z = y @ V[:jj] if jj else np.zeros_like(b)
            return x + (z if minv is None else minv * z)

        while j < m and its < maxit:
            w = A.mult(_apply(minv, V[j]))
            hcol = np.zeros(m + 1, dtype=dtype)
            for _ in range(2):
                h = np.array([_dot(V[i], w) for i in range(j + 1)], dtype=dtype)
                w = w - h @ V[:j + 1]
                hcol[:j + 1] += h
            hn = np.sqrt(_dot(w, w))
            hcol[j + 1] = hn
            if not np.isfinite(hn):
                return dict(x=x, its=its, reason=DIV_NAN, rn=hn, hist=hist, bn=bn)
            if hn > 0:
                V[j + 1] = w * (dtype(1) / hn)
            for i in range(j):
                t = cs[i] * hcol[i] + sn[i] * hcol[i + 1]
                hcol[i + 1] = -sn[i] * hcol[i] + cs[i] * hcol[i + 1]
                hcol[i] = t
            den = np.hypot(hcol[j], hcol[j + 1])
            cs[j] = hcol[j] / den if den > 0 else 1
            sn[j] = hcol[j + 1] / den if den > 0 else 0
            hcol[j], hcol[j + 1] = den, 0
            gv[j + 1] = -sn[j] * gv[j]
            gv[j] = cs[j] * gv[j]
            H[:j + 1, j] = hcol[:j + 1]
            its += 1
            rn = abs(gv[j + 1])
            hist.append((its, rn, iterate(j + 1)))
            reason = stop(rn)
            j += 1
            if reason or hn == 0:
                break
        x = iterate(j)
        if reason:
            break
        if its >= maxit:
            reason = DIV_ITS
            break
    return dict(x=x, its=its, reason=reason, rn=rn, hist=hist, bn=bn)


def thomas(lower, diag, upper, b):
    """Tridiagonal solve in longdouble (no pivoting: diagonally dominant inputs)."""
    n = len(diag)
    lo, d, up = (np.asarray(a, dtype=LD) for a in (lower, diag, upper))
    c, g = np.zeros(n, LD), np.zeros(n, LD)
    rhs = np.asarray(b, dtype=LD)
    piv = d[0]
    g[0] = rhs[0] / piv
    for i in range(1, n):
        c[i - 1] = up[i - 1] / piv
        piv = d[i] - lo[i - 1] * c[i - 1]
        g[i] = (rhs[i] - lo[i - 1] * g[i - 1]) / piv
    x = g.copy()
    for i in range(n - 2, -1, -1):
        x[i] = g[i] - c[i] * x[i + 1]
    return x


def gap_threshold(rns, k, floor=0.0):
    """The geometric mean of ||r_{k-1}|| and max(||r_k||, floor): a stopping
    threshold that iteration k is the first to meet."""
    return float(np.sqrt(LD(rns[k - 1]) * max(LD(rns[k]), LD(floor))))


def gap_ok(rns, k, thr, factor=1.5):
    """Every norm before iteration k is >= factor * thr and iteration k's is
    <= thr / factor: rounding at the 1e-15 level cannot move the stop."""
    return all(r >= factor * thr for r in rns[:k]) and rns[k] <= thr / factor


def two_prod_fsum(x, y):
    """(x, y) exactly, rounded once: Dekker's error-free products, math.fsum."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    p = x * y
    cx, cy = 134217729.0 * x, 134217729.0 * y
    xh, yh = cx - (cx - x), cy - (cy - y)
    xl, yl = x - xh, y - yh
    e = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl
    return math.fsum(np.concatenate([p, e]).tolist())


# ------------------------------------------------- inputs of the GPU tests
CG_LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 1025, 262144 + 77, 524288 + 300)
CG_ITERS = 12
FLOOR = 2.2e-16  # fp64 eps: the least a restatement error counts as


@lru_cache(maxsize=4)
def cg_case(n, pc):
    """Family matrix of length n with the reference history of 12 iterations
    and, per recurrence, the fp64 restatement's error against it."""
    A, b = sym_tridiag(n)
    K = min(CG_ITERS, n)
    xs, rns = pcg_reference(A, b, pc, K)
    bn = float(rns[0])
    err = {v: history_error(*f(A, b, pc, K), xs, rns, 1e-6 * bn) for v, f in RECURRENCES.items()}
    return dict(A=A, b=b, xs=xs, rns=rns, bn=bn, K=len(xs) - 1, err=err)


def cg_tols(case, variant):
    ex, er = case["err"][variant]
    return 16 * max(ex, FLOOR), 16 * max(er, FLOOR)


# DTOL by a residual that rises: (A, b, divtol, crossing iteration) per PC.
# none: A = diag(1, 1e4), b = (1, 0.01): ||r_1|| / ||b|| = 49.995.
# jacobi: A = D^1/2 [[1, .5], [.5, 1]] D^1/2 with D = diag(1, 1e4): Jacobi PCG
# is CG on the inner matrix, whose small second residual entry the scaling
# D^1/2 blows up (||r_1|| / ||b|| = 70.7).
def dtol_case(pc):
    if pc == "none":
        A = Csr([0, 1, 2], [0, 1], [1.0, 1e4])
        return A, np.array([1.0, 0.01]), 10.0, 1
    A = Csr([0, 2, 4], [0, 1, 0, 1], [1.0, 50.0, 50.0, 1e4])
    return A, np.array([1.0, 0.01]), 10.0, 1


def indefinite_case(n=257):
    """diag(+1 .. -1) with b weighted to the negative part: (b, A b) < 0."""
    d = np.linspace(1.0, -1.0, n)
    b = np.where(d < 0, 1.0, 0.1)
    return Csr(np.arange(n + 1), np.arange(n), d), b


GMRES_LENGTHS = (1, 65, 257, 1025)
GMRES_RESTARTS = (3, 5, 30)


@lru_cache(maxsize=None)
def gmres_case(n, pc, restart):
    """Family matrix, an rtol in a gap of the reference's residual history (the
    first iteration >= 8 whose estimate falls >= 2.25 x, or the last), the
    reference run to it and the fp64 restatement's error in x."""
    A, b, lo, d, up = convdiff(n)
    probe = gmres(A, b, pc, restart, 1e-30, maxit=40, dtype=LD)
    bn = float(probe["bn"])
    rns = [probe["bn"]] + [h[1] for h in probe["hist"]]
    floor = 1e-13 * bn
    k = next((k for k in range(min(8, len(rns) - 1), len(rns))
              if rns[k - 1] >= 2.25 * max(rns[k], LD(floor))), len(rns) - 1)
    thr = gap_threshold(rns, k, floor)
    rtol = thr / bn
    ref = gmres(A, b, pc, restart, rtol, dtype=LD)
    f64 = gmres(A, b, pc, restart, rtol, dtype=np.float64)
    ex = float(np.abs(f64["x"].astype(LD) - ref["x"]).max() / np.abs(ref["x"]).max())
    return dict(A=A, b=b, tri=(lo, d, up), rns=rns, k=k, thr=thr, rtol=rtol, ref=ref, f64=f64, ex=ex, bn=bn)


@lru_cache(maxsize=None)
def gmres_maxit_case(n, pc, restart=3, maxit=7):
    A, b, *_ = convdiff(n)
    ref = gmres(A, b, pc, restart, 1e-30, maxit=maxit, dtype=LD)
    f64 = gmres(A, b, pc, restart, 1e-30, maxit=maxit, dtype=np.float64)
    ex = float(np.abs(f64["x"].astype(LD) - ref["x"]).max() / np.abs(ref["x"]).max())
    return dict(A=A, b=b, ref=ref, ex=ex)


def lucky_case(n=257, values=(2.0, 3.0, 5.0)):
    d = np.resize(np.asarray(values, dtype=np.float64), n)
    b = np.random.default_rng(40000 + n).uniform(-1.0, 1.0, n)
    return Csr(np.arange(n + 1), np.arange(n), d), b


# the scalar-CSR product: row lengths at every offset modulo 32, across the
# 512-entry pass
SPMV_ROW_LENGTHS = (0, 1, 31, 32, 33, 511, 512, 513, 1025)


def spmv_case(m, ncols):
    """m rows cycling through SPMV_ROW_LENGTHS (clipped to ncols), random
    distinct columns, values and x in U(-1, 1)."""
    rng = np.random.default_rng(50000 + 7 * m + ncols)
    lens = np.array([min(SPMV_ROW_LENGTHS[(i + m) % len(SPMV_ROW_LENGTHS)], ncols) for i in range(m)])
    if m >= len(SPMV_ROW_LENGTHS):
        assert set(lens) == {min(v, ncols) for v in SPMV_ROW_LENGTHS}
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rng.choice(ncols, ln, replace=False)) for ln in lens] + [np.zeros(0, np.int64)])
    data = rng.uniform(-1.0, 1.0, int(indptr[-1]))
    x = rng.uniform(-1.0, 1.0, ncols)
    return Csr(indptr, indices, data, ncols), x
