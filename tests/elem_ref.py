"""First-principles reference of the KLE element matrices in np.longdouble.

Plain numpy.  Nothing here calls oracle/ or pynama_amd: the formulas of
kle_basis.hpp (1-D rules, Lagrange tables), of the multilinear geometry and of
the element matrices K_e, Rw_e, Rd_e and the collocation blocks Curl_e, SrT_e,
DivSrT_e are restated from their definitions, in libkle's tensor node order
(x fastest, as mesh.conn() and kle_element_kle use) with the corners in the
closure order mesh.corners() returns them (CORN).

    K_e(la, mb) = d_ab G + a_d D_ab + a_w (d_ab tr D - D_ba)
      G    = sum_full c grad N_l . grad N_m      D_ab = sum_red c d_a N_l d_b N_m
    Rw_e from E_d = sum_full c N_l d_d N_m  and  F_d = sum_red c d_d N_l N_m
    Rd_e(la, m) = -E_a + a_d F_a
  full = GLL(ngl) if ngl > 3 else Gauss(ngl), red = Gauss(ngl - 1), op = GLL(ngl),
  c = w det J, a_w = 1e2, a_d = 1e3.

Every value comes with an entrywise bound on what a correct fp64
implementation may differ from it:

    bound = 1.01 u (C S + P),   u = 2^-53

S is the same sum with every term replaced by its absolute value (abs_kle).
C counts the roundings one entry passes through from the rounded operands to
the stored number in the kernel that produced it (C()).  P carries the error
of the operands themselves to first order: dA^T |B| + |A|^T dB, where dA, dB
bound the error of the operand a kernel holds (c grad N, grad N, c N, N at a
Gauss point) against the exact one.  1.01 covers the second-order terms
(C u < 1e-2 throughout).

Why P and not "every factor replaced by a companion": the companion of
inv J (sum |cofactor terms| / |det| with J_kj replaced by
sum_c |dN_c| |X_cj|) is 4 on the unit cube where inv J is 2, with
off-diagonals of 4 where inv J is 0, and the product of such companions is
squared in K.  Measured at 3-D ngl 7 on the unit cube, that S is 150 (Rw_e)
to 3000 (K_e) times the plain sum of absolute terms; a relative error of
1e-10 in the full-rule weights is then 2.8 times the bound on its best Rw_e
entry (before the table and geometry roundings are added to C) and 0.03 on
K_e, against 20 and 8.6 here.  Carrying the same companions through to first
order (each J_kj error enters the inverse once, linearly) is as rigorous and
keeps S to the cancellation the sums really have.

The count, stage by stage (all in units of u; n = number of 1-D nodes):

  1-D nodes and points   premise: within EX u = 4 u of the exact value (four
                         units in the last place of a node in [0.5, 1):
                         Newton or an eigen-solver in fp64), weights within
                         EW(n) u relative,
                         EW = 4 n + 8 (the n-term Legendre recurrence, squared
                         in the weight formula).  tests/test_elem_ref.py
                         asserts the premise for the oracle's rules and, for
                         the product's GLL nodes, through the node coordinates
                         of a one-element mesh on [-1, 1].  libkle exports no
                         tables: its Gauss points, its weights and its h / dh
                         tables are held to the premise only through the
                         element matrices that are built from them.
  Lagrange tables        product form: each factor (p - x_j) one rounding plus
                         2 EX / |p - x_j| from its inputs (0 where p is x_j
                         itself: the factor is exactly 0), n - 1 products for
                         numerator and denominator, one division; the
                         derivative sums n - 1 such products (n - 1 additions)
                         over the companion sum_k prod |.| / |den|.
  tensor products        DIM - 1 products.
  geometry               f = (1 + s xi) / 2: one rounding + EX / 2;
                         dN_c: DIM - 2 roundings; J_kj: 2^DIM terms, one
                         product and at most 2^DIM - 1 additions each, over
                         sum_c |dN_c| |X_cj|; cofactor: product and
                         difference; det: product and 2 additions over
                         sum |J_0j| |cof_0j|; inv J: one division;
                         c = w det: DIM - 1 products of weights and one more.
  physical gradient      DIM products and DIM - 1 additions per entry; the
                         c_q scaling of the l side one more.
  accumulation (C)       one rounding per accumulated Gauss point (a
                         16x16x4 MFMA counted as four sequential additions)
                         plus the product:
                           mfma    K: max(DIM nqF, nqR)      Rw, Rd: max(nqF, nqR)
                           valu    K: max(nqF + DIM, nqR + 1) Rw, Rd: the same
                           oracle  K, Rw, Rd: nqF + nqR (one running sum)
  final combination      store_elem_blocks, the longest path of an entry of K:
                         tr D (DIM - 1), a_w tr (1), G + (1), val + (1):
                         DIM + 2 on top of the accumulation of G or D.  The
                         other path, a_d D_ab, a_w D_ba, their difference and
                         val +, has 4 on top of nqR: with the maximum of the
                         two accumulation lengths taken for every term, C_K
                         = max(..) + DIM + 2 covers it (4 <= DIM + 2).  a_w F
                         and two additions: 3 for Rw and Rd.  The oracle
                         forms c (a_d (..) + a_w cc) per point: DW + 4.

The collocation blocks are single products c_l sum_k invJ_dk dh_k (no
Gauss-point sum); ref_ops carries the same operand errors (c, inv J, dh; the
2 DIM - 1 roundings of the gradient) plus the product with c_l.
"""
import functools

import numpy as np

LD = np.longdouble
U = float(2.0 ** -53)
ALPHA_W, ALPHA_D = 1e2, 1e3
EX = 4.0  # 1-D node / point error premise, in units of u

CORN = {2: np.array([[0, 0], [1, 0], [1, 1], [0, 1]]),
        3: np.array([[0, 0, 0], [0, 1, 0], [1, 1, 0], [1, 0, 0],
                     [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]])}
# (row, column, derivative) of B_curl / Bw_curl, sign (-1)^t
IND3 = [(0, 2, 1), (0, 1, 2), (1, 0, 2), (1, 2, 0), (2, 1, 0), (2, 0, 1)]


def EW(n):
    return 4.0 * n + 8.0


# ------------------------------------------------------------- 1-D rules
def _legendre(n, x):
    """P_n and P_{n-1} at x (three-term recurrence, longdouble)."""
    p0, p1 = np.ones_like(x), x.copy()
    if n == 0:
        return p0, np.zeros_like(x)
    for k in range(2, n + 1):
        p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
    return p1, p0


def _symmetrise(x, w):
    x = (x - x[::-1]) / 2
    w = (w + w[::-1]) / 2
    return x, w


@functools.lru_cache(None)
def gauss(n):
    """Gauss-Legendre nodes and weights on [-1, 1], ascending."""
    i = np.arange(n, dtype=LD)
    x = -np.cos(LD(np.pi) * (i + LD(0.75)) / (n + LD(0.5)))
    for _ in range(60):
        p, pm = _legendre(n, x)
        x = x - p * (1 - x * x) / (n * (pm - x * p))
    p, pm = _legendre(n, x)
    dp = n * (pm - x * p) / (1 - x * x)
    return _symmetrise(x, 2 / ((1 - x * x) * dp * dp))


@functools.lru_cache(None)
def gll(n):
    """Gauss-Lobatto-Legendre nodes and weights on [-1, 1], ascending."""
    N = n - 1
    x = -np.cos(LD(np.pi) * np.arange(n, dtype=LD) / N)
    x[0], x[-1] = -1, 1
    xi = x[1:-1].copy()
    for _ in range(60):
        p, pm = _legendre(N, xi)
        dp = N * (pm - xi * p) / (1 - xi * xi)
        d2 = (2 * xi * dp - N * (N + 1) * p) / (1 - xi * xi)
        xi = xi - dp / d2
    x[1:-1] = xi
    p, _ = _legendre(N, x)
    return _symmetrise(x, 2 / (N * (N + 1) * p * p))


def lagrange(nodes, pts):
    """Lagrange basis of `nodes` and its derivative at `pts`, [point, node]:
    h, dh, the companion dh_abs = sum_k prod |.| / |den| (|h| is the other),
    and the error bounds eh, edh of the fp64 product form, in units of u."""
    n, P = len(nodes), len(pts)
    d = pts[:, None] - nodes[None, :]
    ad = np.abs(d)
    rho = np.where(ad > 0, 1 + 2 * EX / np.where(ad > 0, ad, 1), 0)
    dn = nodes[:, None] - nodes[None, :]
    h, dh, dha, eh, edh = (np.zeros((P, n), LD) for _ in range(5))
    for a in range(n):
        J = [j for j in range(n) if j != a]
        den = np.prod(dn[a, J])
        rden = np.sum(1 + 2 * EX / np.abs(dn[a, J])) + (n - 1)
        num = np.prod(d[:, J], axis=1)
        h[:, a] = num / den
        eh[:, a] = np.abs(h[:, a]) * (np.sum(rho[:, J], axis=1) + (n - 1) + rden + 1)
        s, sa, es = np.zeros(P, LD), np.zeros(P, LD), np.zeros(P, LD)
        for k in J:
            JJ = [j for j in J if j != k]
            t = np.prod(d[:, JJ], axis=1) if JJ else np.ones(P, LD)
            s += t
            sa += np.abs(t)
            es += np.abs(t) * (np.sum(rho[:, JJ], axis=1) + (n - 2))
        dh[:, a] = s / den
        dha[:, a] = sa / abs(den)
        edh[:, a] = (es + sa * (n - 1)) / abs(den) + dha[:, a] * (rden + 1)
    return h, dh, dha, eh, edh


class Rule:
    """One 1-D point set with the tables of the GLL(ngl) basis on it."""

    def __init__(self, nodes, x, w):
        self.x, self.w = x, w
        self.h, self.dh, self.dha, self.eh, self.edh = lagrange(nodes, x)


def rules(ngl, plant=None):
    """full / red / op point sets of the spectral element.  `plant` puts a
    known error into the tables (the discrimination tests):
      {"w_full": f}      full-rule weights times f
      {"dh_full": f}     one entry of the full derivative table times f
      {"drop_red": True} the last reduced Gauss point left out (point_sets)
      {"alpha_w": a}     another curl penalty (ref_kle)"""
    plant = plant or {}
    nodes, nw = gll(ngl)
    fx, fw = (nodes, nw) if ngl > 3 else gauss(ngl)
    rx, rw = gauss(ngl - 1)
    out = {"full": Rule(nodes, fx, fw), "red": Rule(nodes, rx, rw), "op": Rule(nodes, nodes, nw)}
    if "w_full" in plant:
        out["full"].w = out["full"].w * LD(plant["w_full"])
    if "dh_full" in plant:
        out["full"].dh = out["full"].dh.copy()
        out["full"].dh[1, 0] *= LD(plant["dh_full"])
    return out


# ------------------------------------------------------- tensor tables
def _tp(fs):
    """Tensor product of dim [point, node] tables -> [nq, ne], x fastest."""
    if len(fs) == 2:
        t = np.einsum("xa,yb->yxba", *fs)
    else:
        t = np.einsum("xa,yb,zc->zyxcba", *fs)
    P, n = fs[0].shape
    return t.reshape(P ** len(fs), n ** len(fs))


def _tp_err(vals, errs):
    """Error of the fp64 product of the tables `vals` (errors `errs`)."""
    dim = len(vals)
    av = [np.abs(v) for v in vals]
    e = (dim - 1) * _tp(av)
    for k in range(dim):
        e = e + _tp([errs[j] if j == k else av[j] for j in range(dim)])
    return e


def tensor(dim, R):
    """N [q, l], dN [q, k, l] (reference derivatives), their errors, the
    weights wq [q] with error, the points xi [q, k]."""
    hs, es = [R.h] * dim, [R.eh] * dim
    N, eN = _tp(hs), _tp_err(hs, es)
    dN, edN = [], []
    for k in range(dim):
        v = [R.dh if j == k else R.h for j in range(dim)]
        e = [R.edh if j == k else R.eh for j in range(dim)]
        dN.append(_tp(v))
        edN.append(_tp_err(v, e))
    P = len(R.x)
    g = np.meshgrid(*[np.arange(P)] * dim, indexing="ij")
    qi = np.stack([a.ravel() for a in g[::-1]], -1)  # [q, k], x fastest
    xi = R.x[qi]
    wq = np.prod(R.w[qi], axis=1)
    ewq = np.abs(wq) * (dim * EW(P) + dim - 1)
    return N, eN, np.stack(dN, 1), np.stack(edN, 1), wq, ewq, xi


# ------------------------------------------------------------- geometry
def _cof3(J, eJ):
    """Cofactors adj[i, k] (inv J = adj / det) of 3x3 J [q, 3, 3] with errors."""
    aJ = np.abs(J)

    def two(a, b, c, d):  # J_a J_b - J_c J_d
        v = J[:, a[0], a[1]] * J[:, b[0], b[1]] - J[:, c[0], c[1]] * J[:, d[0], d[1]]
        e = 0
        for p, r in ((a, b), (c, d)):
            e = e + aJ[:, p[0], p[1]] * eJ[:, r[0], r[1]] + eJ[:, p[0], p[1]] * aJ[:, r[0], r[1]] \
                + 2 * aJ[:, p[0], p[1]] * aJ[:, r[0], r[1]]
        return v, e

    adj = np.zeros_like(J)
    eadj = np.zeros_like(J)
    for i in range(3):
        for k in range(3):
            # adj[i, k] = cofactor of J[k, i]
            r = [a for a in range(3) if a != k]
            c = [a for a in range(3) if a != i]
            v, e = two((r[0], c[0]), (r[1], c[1]), (r[0], c[1]), (r[1], c[0]))
            sg = -1 if (i + k) % 2 else 1
            adj[:, i, k], eadj[:, i, k] = sg * v, e
    return adj, eadj


def geometry(dim, xi, X):
    """det J [q], inv J [q, i, k] (d xi_k / d x_i ... as J^-1[i][k] with
    J[k][j] = d x_j / d xi_k) and their error bounds, from the corners X
    [2^dim, dim] (fp64 values, widened)."""
    X = np.asarray(X, dtype=np.float64).reshape(2 ** dim, dim).astype(LD)
    nc = 2 ** dim
    s = (2 * CORN[dim] - 1).astype(LD)
    f = (1 + s[None] * xi[:, None, :]) / 2  # [q, c, k]
    ef = np.abs(f) + EX / 2
    af = np.abs(f)
    nq = len(xi)
    dn, edn = np.zeros((nq, nc, dim), LD), np.zeros((nq, nc, dim), LD)
    for k in range(dim):
        o = [d for d in range(dim) if d != k]
        v = s[None, :, k] / 2
        for d in o:
            v = v * f[:, :, d]
        dn[:, :, k] = v
        e = (dim - 2) * np.abs(v)
        for d in o:
            t = ef[:, :, d] / 2
            for d2 in o:
                if d2 != d:
                    t = t * af[:, :, d2]
            e = e + t
        edn[:, :, k] = e
    aX = np.abs(X)
    J = np.einsum("qck,cj->qkj", dn, X)
    eJ = np.einsum("qck,cj->qkj", edn, aX) + nc * np.einsum("qck,cj->qkj", np.abs(dn), aX)
    aJ = np.abs(J)
    if dim == 2:
        det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
        edet = 0
        for a, b in (((0, 0), (1, 1)), ((0, 1), (1, 0))):
            edet = edet + aJ[:, a[0], a[1]] * eJ[:, b[0], b[1]] + eJ[:, a[0], a[1]] * aJ[:, b[0], b[1]] \
                + 2 * aJ[:, a[0], a[1]] * aJ[:, b[0], b[1]]
        adj = np.stack([np.stack([J[:, 1, 1], -J[:, 0, 1]], -1), np.stack([-J[:, 1, 0], J[:, 0, 0]], -1)], 1)
        eadj = np.stack([np.stack([eJ[:, 1, 1], eJ[:, 0, 1]], -1), np.stack([eJ[:, 1, 0], eJ[:, 0, 0]], -1)], 1)
    else:
        adj, eadj = _cof3(J, eJ)
        # det = sum_j J[0][j] cofactor(0, j) = sum_j J[0][j] adj[j][0]
        det = np.einsum("qj,qj->q", J[:, 0, :], adj[:, :, 0])
        edet = np.einsum("qj,qj->q", eJ[:, 0, :], np.abs(adj[:, :, 0])) \
            + np.einsum("qj,qj->q", aJ[:, 0, :], eadj[:, :, 0]) \
            + 3 * np.einsum("qj,qj->q", aJ[:, 0, :], np.abs(adj[:, :, 0]))
    Ji = adj / det[:, None, None]
    adet = np.abs(det)[:, None, None]
    eJi = eadj / adet + np.abs(adj) * edet[:, None, None] / adet ** 2 + np.abs(Ji)
    return det, edet, Ji, eJi


class PointSet:
    """Operands of one quadrature rule on one element: c [q], g [q, i, l]
    (physical gradient), N [q, l], with error bounds e* (units of u)."""

    def __init__(self, dim, R, X, drop_last=False):
        N, eN, dN, edN, wq, ewq, xi = tensor(dim, R)
        if drop_last:
            wq = wq.copy()
            wq[-1] = 0
        det, edet, Ji, eJi = geometry(dim, xi, X)
        self.N, self.eN = N, eN
        self.det, self.Ji, self.eJi = det, Ji, eJi
        self.c = wq * det
        self.ec = np.abs(det) * ewq + np.abs(wq) * edet + np.abs(self.c)
        self.g = np.einsum("qik,qkl->qil", Ji, dN)
        aJi, adN = np.abs(Ji), np.abs(dN)
        self.eg = np.einsum("qik,qkl->qil", eJi, adN) + np.einsum("qik,qkl->qil", aJi, edN) \
            + dim * np.einsum("qik,qkl->qil", aJi, adN)
        c3 = self.c[:, None, None]
        self.cg = c3 * self.g
        self.ecg = np.abs(c3) * self.eg + np.abs(self.g) * self.ec[:, None, None] + np.abs(self.cg)
        c2 = self.c[:, None]
        self.cN = c2 * N
        self.ecN = np.abs(c2) * eN + np.abs(N) * self.ec[:, None] + np.abs(self.cN)


_X_CACHE = {}


def point_sets(dim, ngl, X, plant=None):
    key = (dim, ngl, np.asarray(X, np.float64).tobytes(), repr(sorted((plant or {}).items())))
    if key not in _X_CACHE:
        if len(_X_CACHE) > 64:
            _X_CACHE.clear()
        R = rules(ngl, plant)
        drop = bool((plant or {}).get("drop_red"))
        _X_CACHE[key] = {k: PointSet(dim, R[k], X, drop and k == "red") for k in ("full", "red", "op")}
    return _X_CACHE[key]


# ------------------------------------------------------ KLE matrices
def _products(AgF, BgF, ANF, AgR, BgR, BNR, rows):
    """G [l, m], D [l, a, m, b], E [l, d, m], F [l, d, m] for the row nodes
    `rows`: K[rows] = A[:, rows]^T A, as matrix products over (q, component).
    A*: l-side operands (scaled by c), B*: m-side operands."""
    nqF, dim, ne = BgF.shape
    nqR = BgR.shape[0]
    nr = len(rows)
    G = AgF[:, :, rows].reshape(nqF * dim, nr).T @ BgF.reshape(nqF * dim, ne)
    A2 = np.ascontiguousarray(AgR[:, :, rows].transpose(0, 2, 1)).reshape(nqR, nr * dim)
    B2 = np.ascontiguousarray(BgR.transpose(0, 2, 1)).reshape(nqR, ne * dim)
    D = (A2.T @ B2).reshape(nr, dim, ne, dim)
    E = (ANF[:, rows].T @ BgF.reshape(nqF, dim * ne)).reshape(nr, dim, ne)
    F = (A2.T @ BNR).reshape(nr, dim, ne)
    return G, D, E, F


def _combine(dim, G, D, E, F, sign, alpha_w=ALPHA_W):
    """K [l a, m b], Rw [l a, m c], Rd [l a, m] from the factored sums; with
    sign = +1 every term is added (the abs-value companions)."""
    nr, ne = G.shape
    dw = 1 if dim == 2 else 3
    sg = -1 if sign < 0 else 1
    aw, ad = G.dtype.type(alpha_w), G.dtype.type(ALPHA_D)
    K = ad * D + sg * aw * D.transpose(0, 3, 2, 1)
    tr = np.einsum("lcmc->lm", D)
    for a in range(dim):
        K[:, a, :, a] += G + aw * tr
    Rw = np.zeros((nr, dim, ne, dw), G.dtype)
    if dim == 3:
        for t, (r0, r1, d) in enumerate(IND3):
            s = sg if t & 1 else 1
            Rw[:, r0, :, r1] += s * E[:, d, :]
            Rw[:, r1, :, r0] += aw * s * F[:, d, :]
    else:
        Rw[:, 0, :, 0] += E[:, 1, :] + sg * aw * F[:, 1, :]
        Rw[:, 1, :, 0] += sg * E[:, 0, :] + aw * F[:, 0, :]
    Rd = sg * E + ad * F
    return K.reshape(nr * dim, ne * dim), Rw.reshape(nr * dim, ne * dw), Rd.reshape(nr * dim, ne)


def _rows(dim, ngl, rows):
    return np.arange(ngl ** dim) if rows is None else np.asarray(rows, dtype=np.int64)


def ref_kle(dim, ngl, X, rows=None, plant=None):
    """K_e, Rw_e, Rd_e in longdouble; with rows= only those node rows
    (dim rows each, all columns)."""
    ps = point_sets(dim, ngl, X, plant)
    f, r = ps["full"], ps["red"]
    G, D, E, F = _products(f.cg, f.g, f.cN, r.cg, r.g, r.N, _rows(dim, ngl, rows))
    return _combine(dim, G, D, E, F, -1, alpha_w=(plant or {}).get("alpha_w", ALPHA_W))


def _f64(a):
    return np.abs(a).astype(np.float64)


def abs_kle(dim, ngl, X, rows=None):
    """SK, SRw, SRd: the sums of ref_kle with every term replaced by its
    absolute value (fp64: a bound needs no more)."""
    ps = point_sets(dim, ngl, X)
    f, r = ps["full"], ps["red"]
    G, D, E, F = _products(_f64(f.cg), _f64(f.g), _f64(f.cN), _f64(r.cg), _f64(r.g), _f64(r.N),
                           _rows(dim, ngl, rows))
    return _combine(dim, G, D, E, F, +1)


def prop_kle(dim, ngl, X, rows=None):
    """PK, PRw, PRd: the operand errors carried into the sums to first order,
    dA^T |B| + |A|^T dB, in units of u."""
    ps = point_sets(dim, ngl, X)
    f, r = ps["full"], ps["red"]
    rows = _rows(dim, ngl, rows)
    a = _products(_f64(f.ecg), _f64(f.g), _f64(f.ecN), _f64(r.ecg), _f64(r.g), _f64(r.N), rows)
    b = _products(_f64(f.cg), _f64(f.eg), _f64(f.cN), _f64(r.cg), _f64(r.eg), _f64(r.eN), rows)
    return _combine(dim, *[p + q for p, q in zip(a, b)], +1)


def npoints(dim, ngl):
    return ngl ** dim, (ngl - 1) ** dim


def C(dim, ngl, kernel):
    """Roundings from the rounded operands to the stored entry (module
    docstring): (C_K, C_Rw) for kernel in mfma / valu / oracle; Rd as Rw."""
    nqF, nqR = npoints(dim, ngl)
    dw = 1 if dim == 2 else 3
    if kernel == "mfma":
        return max(dim * nqF, nqR) + dim + 2, max(nqF, nqR) + 3
    if kernel == "valu":
        return max(nqF + dim, nqR + 1) + dim + 2, max(nqF, nqR) + 3
    if kernel == "oracle":
        return nqF + nqR + dw + 4, nqF + nqR + 3
    raise ValueError(kernel)


def bound_from(S, P, dim, ngl, kernel):
    """1.01 u (C S + P) for `kernel` from abs_kle's S and prop_kle's P."""
    ck, cr = C(dim, ngl, kernel)
    return tuple(1.01 * U * (c * s + p) for c, s, p in zip((ck, cr, cr), S, P))


def bound_kle(dim, ngl, X, kernel, rows=None):
    """Entrywise bounds BK, BRw, BRd = 1.01 u (C S + P) for `kernel`."""
    return bound_from(abs_kle(dim, ngl, X, rows), prop_kle(dim, ngl, X, rows), dim, ngl, kernel)


# -------------------------------------------------- collocation blocks
def _op_coeff(dim):
    """T[name][r, c, d]: block entry (r, c) = c_l sum_d T[r, c, d] H_d."""
    dw, ds = (1, 3) if dim == 2 else (3, 6)
    Cu, S, Dv = np.zeros((dw, dim, dim)), np.zeros((ds, dim, dim)), np.zeros((dim, ds, dim))
    if dim == 3:
        for t, (r0, r1, d) in enumerate(IND3):
            Cu[r0, r1, d] = -1 if t & 1 else 1
        bdiv = [[0, 1, 5], [1, 2, 3], [5, 3, 4]]
    else:
        Cu[0, 1, 0], Cu[0, 0, 1] = 1, -1
        bdiv = [[0, 1], [1, 2]]
    for x in range(dim):
        S[2 * x, x, x] = 1
        for i in range(dim):
            Dv[i, bdiv[x][i], x] = 1
            if i != x:
                S[(x + i) if x + i != 2 or dim == 2 else 5, i, x] = 0.5
    return {"Curl": Cu, "SrT": S, "DivSrT": Dv}


def node_positions(dim, ngl, X):
    """Physical position of every element node [l, dim], tensor order."""
    X = np.asarray(X, np.float64).reshape(2 ** dim, dim).astype(LD)
    x = gll(ngl)[0]
    g = np.meshgrid(*[np.arange(ngl)] * dim, indexing="ij")
    xi = x[np.stack([a.ravel() for a in g[::-1]], -1)]
    s = (2 * CORN[dim] - 1).astype(LD)
    f = np.prod((1 + s[None] * xi[:, None, :]) / 2, axis=2)
    return f @ X


def ref_ops(dim, ngl, X):
    """Curl_e [l dw, m dim], SrT_e [l ds, m dim], DivSrT_e [l dim, m ds], c_e
    [l] in kle_element_ops' layout, and their entrywise bounds (fp64)."""
    o = point_sets(dim, ngl, X)["op"]
    ne = ngl ** dim
    H = o.g  # [q = l, d, m]; dN/dxi, and with it eg, is exactly 0 off the grid lines
    out, bnd = {}, {}
    for nm, T in _op_coeff(dim).items():
        T = T.astype(LD)
        M = np.einsum("l,rcd,ldm->lrmc", o.c, T, H)
        aT = np.abs(T)
        e = np.einsum("l,rcd,ldm->lrmc", np.abs(o.c), aT, o.eg) + np.einsum("l,rcd,ldm->lrmc", o.ec, aT, np.abs(H)) \
            + np.einsum("l,rcd,ldm->lrmc", np.abs(o.c), aT, np.abs(H))
        R, Cc = T.shape[0], T.shape[1]
        out[nm] = M.reshape(ne * R, ne * Cc)
        bnd[nm] = (1.01 * U * e).astype(np.float64).reshape(ne * R, ne * Cc)
    out["c"], bnd["c"] = o.c, (1.01 * U * o.ec).astype(np.float64)
    return out, bnd


def ops_line_mask(dim, ngl):
    """[l, m]: node m lies on a grid line through node l."""
    ne = ngl ** dim
    idx = np.arange(ne)
    co = np.stack([(idx // ngl ** d) % ngl for d in range(dim)], -1)
    diff = (co[:, None, :] != co[None, :, :]).sum(-1)
    return diff <= 1


# ------------------------------------------------------------ assembly
def assemble_ref(dim, ngl, conn, corners, dirflag, kernel="mfma", ops=True):
    """Dense longdouble K, Krhs, Rw (Dirichlet treatment of the free-slip
    assembly: free rows x free columns of K += K_e, free rows x Dirichlet
    columns of Krhs += -K_e, unit diagonal on Dirichlet rows of both, free
    rows of Rw += Rw_e, free rows of Rd += Rd_e: the no-slip assembly's Rd
    with its wall nodes as the Dirichlet set) and Curl, SrT, DivSrT (element blocks added, rows
    scaled by 1 / W_n, W_n = sum of c over the incident elements), each as
    (value, bound, pattern).  conn [E, ne] in tensor order, corners
    [E, 2^dim, dim], dirflag [N]."""
    conn = np.asarray(conn)
    E, ne = conn.shape
    N = len(dirflag)
    dw, ds = (1, 3) if dim == 2 else (3, 6)
    free = ~np.asarray(dirflag, bool)
    shp = {"K": (dim, dim), "Krhs": (dim, dim), "Rw": (dim, dw), "Rd": (dim, 1), "Curl": (dw, dim),
           "SrT": (ds, dim), "DivSrT": (dim, ds)}
    names = ["K", "Krhs", "Rw", "Rd"] + (["Curl", "SrT", "DivSrT"] if ops else [])
    val = {k: np.zeros((N * shp[k][0], N * shp[k][1]), LD) for k in names}
    bnd = {k: np.zeros((N * shp[k][0], N * shp[k][1])) for k in names}
    mag = {k: np.zeros((N * shp[k][0], N * shp[k][1])) for k in names}
    cnt = {k: np.zeros((N * shp[k][0], N * shp[k][1]), np.int32) for k in names}
    W, eW, nW = np.zeros(N, LD), np.zeros(N), np.zeros(N, np.int32)

    def dofs(nodes, r):
        return (np.asarray(nodes)[:, None] * r + np.arange(r)[None, :]).ravel()

    cache = {}
    for e in range(E):
        X = np.asarray(corners[e], np.float64)
        key = X.tobytes()
        if key not in cache:
            Ke, Rwe, Rde = ref_kle(dim, ngl, X)
            BK, BRw, BRd = bound_kle(dim, ngl, X, kernel)
            BK = np.maximum(BK, BK.T)  # K takes block (l, m), l < m, for both triangles
            cache[key] = (Ke, Rwe, Rde, BK, BRw, BRd, ref_ops(dim, ngl, X) if ops else None)
        Ke, Rwe, Rde, BK, BRw, BRd, op = cache[key]
        nd = conn[e]
        fr, dr = free[nd], ~free[nd]
        rv = dofs(nd, dim)
        rfree = np.repeat(fr, dim)
        cdir = np.repeat(dr, dim)
        for nm, blk, bb, rmask, cmask, cols, sgn in (
                ("K", Ke, BK, rfree, rfree, rv, 1), ("Krhs", Ke, BK, rfree, cdir, rv, -1),
                ("Rw", Rwe, BRw, rfree, np.ones(ne * dw, bool), dofs(nd, dw), 1),
                ("Rd", Rde, BRd, rfree, np.ones(ne, bool), nd, 1)):
            ix = np.ix_(rv[rmask], cols[cmask])
            sub = np.ix_(rmask, cmask)
            val[nm][ix] += sgn * blk[sub]
            bnd[nm][ix] += bb[sub]
            mag[nm][ix] += np.abs(blk[sub]).astype(np.float64)
            cnt[nm][ix] += 1
        if ops:
            ov, ob = op
            for nm in ("Curl", "SrT", "DivSrT"):
                ix = np.ix_(dofs(nd, shp[nm][0]), dofs(nd, shp[nm][1]))
                val[nm][ix] += ov[nm]
                bnd[nm][ix] += ob[nm]
                mag[nm][ix] += np.abs(ov[nm]).astype(np.float64)
                cnt[nm][ix] += 1
            W[nd] += ov["c"]
            eW[nd] += ob["c"]
            nW[nd] += 1
    out = {}
    dirdof = dofs(np.nonzero(~free)[0], dim)
    for nm in ("K", "Krhs"):
        val[nm][dirdof, dirdof] += 1
        cnt[nm][dirdof, dirdof] += 1
    for nm in names:
        # one rounding per incident element for the sum of the blocks
        b = bnd[nm] + 1.01 * U * cnt[nm] * mag[nm]
        v = val[nm]
        if nm in ("Curl", "SrT", "DivSrT"):
            R = shp[nm][0]
            Wr = np.repeat(W, R)[:, None]
            # 1 / W (the sum of c: one rounding per element, one division) and the scaling
            aW = np.abs(W).astype(np.float64)
            relW = np.repeat((eW + 1.01 * U * nW * aW) / aW, R)[:, None]
            b = b / np.abs(Wr).astype(np.float64) + np.abs(v / Wr).astype(np.float64) * (relW + 2 * 1.01 * U)
            v = v / Wr
        out[nm] = (v, b, cnt[nm] > 0)
    return out


def csr_of(value, pattern):
    """(indptr, indices, data) of the dense `value` on `pattern` (explicit
    zeros kept), columns ascending."""
    r, c = np.nonzero(pattern)
    indptr = np.zeros(pattern.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=pattern.shape[0]), out=indptr[1:])
    return indptr, c.astype(np.int64), value[r, c]


# ------------------------------------------------------------- checking
SUBSET_FROM = 344  # ne above which the tests compare tile_rows instead of every row: 3-D ngl 8 alone


def tile_rows(ne, seed=0):
    """First and last row of every 32-row tile and 16-row sub-tile, ne - 1,
    and 16 random rows."""
    r = set()
    for t in range(0, ne, 16):
        r.update((t, min(t + 15, ne - 1)))
    r.add(ne - 1)
    r.update(np.random.default_rng(seed).choice(ne, 16, replace=False).tolist())
    return np.array(sorted(r))


def compare_rows(dim, ngl):
    """Node rows the tests compare (None: all).  The full reference of one
    3-D element takes 6 s at ngl 7 and 32 s at ngl 8: ngl 8 alone is cut."""
    ne = ngl ** dim
    return tile_rows(ne) if ne >= SUBSET_FROM else None



def dof(p, r):
    """DoF indices p r + (0 .. r - 1) of the nodes p."""
    return (np.asarray(p)[:, None] * r + np.arange(r)[None, :]).ravel()


def worst(dev, ref, bound):
    """Largest |dev - ref| / bound and its entry; entries with bound 0 must
    be equal (their ratio counts as inf when they are not)."""
    err = np.abs(np.asarray(dev).astype(LD) - ref).astype(np.float64)
    b = np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1), np.where(err > 0, np.inf, 0.0))
    k = np.unravel_index(np.argmax(ratio), ratio.shape) if ratio.size else ()
    return (float(ratio[k]) if ratio.size else 0.0), tuple(int(i) for i in k)
