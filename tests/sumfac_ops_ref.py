"""References of the sum-factorised Rw (kle_sumfac.hip k_sumfac_rw) and of the
collocation operators with per-element geometry (kle_colloc.hip
k_colloc_elem<.., true>, k_colloc_gather_csr) in np.longdouble, with derived
bounds.

Plain numpy on top of tests/elem_ref.py, in the manner of tests/sumfac_ref.py;
nothing here calls pynama_amd or oracle/.  The mesh comes in as arrays: conn
[E, nn] (tensor node order), corners [E, 2^dim, dim], dirflag [N].

Rw
--
y_ref = sum_e S_e^T ref_kle(X_e)[1] w_e on free rows, 0 on Dirichlet rows (no
entry of w is dropped).  Bound (u = 2^-53):

    bound_i = 1.01 u [ sum_{e in i} ( C_rw (S_e |w_e|)_i + (P_e |w_e|)_i )
                       + (inc_i - 1) sum_{e in i} |(Rw_e w_e)_i| ]

S_e = abs_kle[1], P_e = prop_kle[1], inc_i the node's incidence count.
Dirichlet rows compare exactly: +0.0.

C_rw counts the roundings one ws entry passes through in k_sumfac_rw as
written, a line sum of n products counted n (sumfac_ref's convention).
n = ngl:

  full rule
    forward passes       x, y (, z) line sums over the n nodes: DIM n
    physical gradient    sum_k invJ[b][k] g[c][k]: DIM
    c curl w             3-D: one difference, one product: 2.  2-D: c G: 1 (the
                         sign is exact)
    value passes back    z, y, x (2-D: y, x) over the n points: DIM n
  reduced rule
    forward value passes DIM n
    t = c (a_w w_c)      2
    inv J^T              3-D: Ji t - Ji t, two products and a difference: 2.
                         2-D: one product: 1
    transposed passes    as k_sumfac_elem: 5 (n - 1) in 3-D, 3 (n - 1) in 2-D
  rule sum               1

  3-D  full 6 n + 5,  reduced 3 n + 4 + 5 (n - 1) = 8 n - 1
  2-D  full 4 n + 3,  reduced 2 n + 3 + 3 (n - 1) = 5 n
  C_rw = max over the rules + 1                                     -- C_rw()

Beside it the bound of the assembled product (the longdouble product of the
device's stored Rw with w): per entry elem_ref.assemble_ref's
sum_e BRw_e + 1.01 u cnt |Rw|, applied to |w| with cnt <= inc_i:

    abound_i = sum_e (BRw_e |w_e|)_i + 1.01 u inc_i sum_e (|Rw_e| |w_e|)_i

Collocation operators
---------------------
y_ref_i = (sum_e ref_ops(X_e)[nm] x_e)_i / W_i, W the longdouble sum of c over
the node's incident elements.  Before the scaling, row i carries

    b_i = sum_e ( (B_e |x_e|)_i + 1.01 u C_op (S_e |x_e|)_i )
          + 1.01 u (inc_i - 1) sum_e |(M_e x_e)_i|

B_e = ref_ops' entrywise bound (the errors of c, inv J and dh carried into the
entry), S_e the companion |c_l| sum_d |T| sum_k |invJ_dk| |dh_k|, and C_op the
roundings of k_colloc_elem as written: the line sums over n nodes (n), inv J
(DIM), the placement (at most DIM terms, the 1/2 exact: DIM), times c_l (1):

  C_op = n + 2 DIM + 1                                              -- C_op()

The gather adds inc_i numbers (inc_i - 1 roundings).  Then, as
elem_ref.assemble_ref does for its 1 / W: winv = fl(1 / W~), W~ the fp64 sum of
the rounded c in incidence order (relative error (eW + 1.01 u inc |W|) / |W|),
one division and the final product (2 * 1.01 u):

    bound_i = b_i / |W_i| + |y_ref_i| (relW_i + 2.02 u)

The assembled product's bound is assemble_ref's entry bound applied to |x|:

    abound_i = ( sum_e (B_e |x_e|)_i + 1.01 u inc_i sum_e (|M_e| |x_e|)_i ) / |W_i|
               + ( sum_e (|M_e| |x_e|)_i / |W_i| ) (relW_i + 2.02 u)

For large elements (3-D ngl >= 7) `nodes=` restricts every reference to a
sample of global node rows (sumfac_ref.sample_nodes).
"""
import numpy as np

import elem_ref as R
import sumfac_ref as SF

LD = R.LD
U = R.U
OPS = ("Curl", "SrT", "DivSrT")


def C_rw(dim, ngl):
    n = ngl
    return (max(6 * n + 5, 8 * n - 1) if dim == 3 else max(4 * n + 3, 5 * n)) + 1


def C_op(dim, ngl):
    return ngl + 2 * dim + 1


def _eps3():
    e = np.zeros((3, 3, 3))
    for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        e[a, b, c], e[a, c, b] = 1, -1
    return e


# ------------------------------------------------- the factorised Rw formula
def rw_apply(dim, ngl, X, we, dtype=LD, plant=None, flip=False):
    """Rw_e w_e by the sum-factorised formula k_sumfac_rw evaluates, in `dtype`
    (tables and geometry formed in longdouble and rounded to it).  we [nn dw]
    node-major.  plant: elem_ref.rules' plants and "alpha_w"; flip: the sign of
    one curl term flipped (a planted error)."""
    plant = plant or {}
    rl = R.rules(ngl, plant)
    ps = R.point_sets(dim, ngl, X, plant)
    aw = dtype(plant.get("alpha_w", R.ALPHA_W))
    dw = 1 if dim == 2 else 3
    comp = [2] if dim == 2 else [0, 1, 2]  # the components of w as 3-D indices
    eps = _eps3().astype(dtype)
    epc = eps.copy()  # curl_a = epc[a, b, c] d_b w_c
    if flip:
        epc[0, 2 if dim == 3 else 1, comp[0] if dim == 2 else 1] *= -1
    w = np.asarray(we, dtype=dtype).reshape((ngl,) * dim + (dw,))
    out = np.zeros((ngl ** dim, dim), dtype)
    if dim == 3:
        fw, bw = "zk,yj,xi,kjia->zyxa", "zk,yj,xi,zyxa->kjia"
    else:
        fw, bw = "yj,xi,jia->yxa", "yj,xi,yxa->jia"
    # ---- full rule: c N_l curl w
    h, dh = rl["full"].h.astype(dtype), rl["full"].dh.astype(dtype)
    P = h.shape[0]
    c, Ji = ps["full"].c.astype(dtype), ps["full"].Ji.astype(dtype)
    tabs = [(h, h, dh), (h, dh, h), (dh, h, h)] if dim == 3 else [(h, dh), (dh, h)]
    g = np.stack([np.einsum(fw, *t, w) for t in tabs], -1).reshape(P ** dim, dw, dim)  # [q, c, k]
    G = np.einsum("qbk,qck->qcb", Ji, g)  # d_b w_c
    curl = np.einsum("abc,qcb->qa", epc[:dim][:, :dim][:, :, comp], G)
    v = (c[:, None] * curl).reshape((P,) * dim + (dim,))
    out += np.einsum(bw, *([h] * dim), v).reshape(ngl ** dim, dim)
    # ---- reduced rule: a_w c sum_b d_b N_l eps_{acb} w_c
    h, dh = rl["red"].h.astype(dtype), rl["red"].dh.astype(dtype)
    P = h.shape[0]
    c, Ji = ps["red"].c.astype(dtype), ps["red"].Ji.astype(dtype)
    tabs = [(h, h, dh), (h, dh, h), (dh, h, h)] if dim == 3 else [(h, dh), (dh, h)]
    wq = np.einsum(fw, *([h] * dim), w).reshape(P ** dim, dw)
    t = c[:, None] * (aw * wq)
    F = np.einsum("acb,qc->qab", eps[:dim][:, comp][:, :, :dim], t)
    Fr = np.einsum("qbk,qab->qak", Ji, F).reshape((P,) * dim + (dim, dim))
    for k, tb in enumerate(tabs):
        out += np.einsum(bw, *tb, Fr[..., k]).reshape(ngl ** dim, dim)
    return out.ravel()


# --------------------------------------------------------- Rw on a mesh
_RW_TERMS = {}


def _rw_terms(dim, ngl, X, rows):
    key = (dim, ngl, X.tobytes(), np.asarray(rows, np.int64).tobytes())
    if key not in _RW_TERMS:
        if len(_RW_TERMS) >= 64:
            _RW_TERMS.clear()
        Sall, Pall = R.abs_kle(dim, ngl, X), R.prop_kle(dim, ngl, X)
        _RW_TERMS[key] = (R.ref_kle(dim, ngl, X, rows=rows)[1], Sall[1], Pall[1],
                          R.bound_from(Sall, Pall, dim, ngl, "mfma")[1])
    return _RW_TERMS[key]


class Reference:
    """y (longdouble), bound, abound; rows: the DoF rows they hold (all, or
    those of `nodes`), dird: which of them are Dirichlet rows."""


def rw_reference(dim, ngl, conn, corners, dirflag, w, nodes=None, apply=None, skip=None):
    """The mesh-level Rw reference and bounds (module docstring).  apply(e, X,
    we) -> Rw_e we replaces the element product of the *value* (planted
    errors); skip = (e, l): that incidence entry is left out of the gather."""
    conn = np.asarray(conn)
    E, nn = conn.shape
    N = len(dirflag)
    dw = 1 if dim == 2 else 3
    dirn = np.asarray(dirflag, bool)
    inc = SF.incidence(conn, N)
    w = np.asarray(w, np.float64)
    want = np.ones(N, bool) if nodes is None else np.isin(np.arange(N), nodes)
    y = np.zeros(N * dim, LD)
    sS, sP, sM, sB, sA = (np.zeros(N * dim) for _ in range(5))
    cr = C_rw(dim, ngl)
    for e in range(E):
        nd = conn[e]
        rows = np.nonzero(want[nd] & ~dirn[nd])[0]
        if not len(rows):
            continue
        X = np.asarray(corners[e], np.float64)
        we = w[R.dof(nd, dw)]
        aw = np.abs(we)
        rl, rg = R.dof(rows, dim), R.dof(nd[rows], dim)
        Rwe, S, Pm, BRw = _rw_terms(dim, ngl, X, rows)
        ye = Rwe @ we.astype(LD)
        val = np.asarray(apply(e, X, we), LD)[rl] if apply is not None else ye.copy()
        if skip is not None and skip[0] == e:
            val[np.repeat(rows == skip[1], dim)] = 0
        np.add.at(y, rg, val)
        np.add.at(sS, rg, S[rl] @ aw)
        np.add.at(sP, rg, Pm[rl] @ aw)
        np.add.at(sM, rg, np.abs(ye).astype(np.float64))
        np.add.at(sB, rg, BRw[rl] @ aw)
        np.add.at(sA, rg, np.abs(Rwe).astype(np.float64) @ aw)
    incd = np.repeat(inc, dim).astype(np.float64)
    dird = np.repeat(dirn, dim)
    out = Reference()
    out.rows = np.nonzero(np.repeat(want, dim))[0]
    out.dird = dird[out.rows]
    out.y = np.where(dird, LD(0), y)[out.rows]
    out.bound = np.where(dird, 0.0, 1.01 * U * (cr * sS + sP + (incd - 1) * sM))[out.rows]
    out.abound = np.where(dird, 0.0, sB + 1.01 * U * incd * sA)[out.rows]
    return out


# ------------------------------------------------- collocation operators
_OP_TERMS = {}


def _op_terms(dim, ngl, X):
    """ref_ops' blocks and bounds and the companions S of one element."""
    key = (dim, ngl, X.tobytes())
    if key not in _OP_TERMS:
        if len(_OP_TERMS) >= 64:
            _OP_TERMS.clear()
        ov, ob = R.ref_ops(dim, ngl, X)
        o = R.point_sets(dim, ngl, X)["op"]
        dN = R.tensor(dim, R.rules(ngl)["op"])[2]
        Ha = np.einsum("qik,qkl->qil", np.abs(o.Ji), np.abs(dN)).astype(np.float64)
        ne = ngl ** dim
        S = {}
        for nm, T in R._op_coeff(dim).items():
            S[nm] = np.einsum("l,rcd,ldm->lrmc", np.abs(o.c).astype(np.float64), np.abs(T), Ha).reshape(
                ne * T.shape[0], ne * T.shape[1])
        _OP_TERMS[key] = (ov, ob, S)
    return _OP_TERMS[key]


def op_shape(dim, name):
    dw, ds = (1, 3) if dim == 2 else (3, 6)
    return {"Curl": (dw, dim), "SrT": (ds, dim), "DivSrT": (dim, ds)}[name]


def ops_reference(dim, ngl, conn, corners, name, x, nodes=None, plant=None):
    """The mesh-level reference and bounds of one collocation operator (module
    docstring).  plant, errors in the *value* only:
      {"srt_half": f}   SrT's 1/2 replaced by f
      {"skip_w": (e, l)}  that incidence entry left out of the weight W
      {"skip": (e, l)}  that incidence entry left out of the gather
      {"geo0": True}    every element evaluated with element 0's corners"""
    plant = plant or {}
    conn = np.asarray(conn)
    E, nn = conn.shape
    N = int(conn.max()) + 1
    rw, cw = op_shape(dim, name)
    inc = SF.incidence(conn, N)
    x = np.asarray(x, np.float64)
    want = np.ones(N, bool) if nodes is None else np.isin(np.arange(N), nodes)
    y = np.zeros(N * rw, LD)
    sB, sS, sM, sA = (np.zeros(N * rw) for _ in range(4))
    W, Wv, eW = np.zeros(N, LD), np.zeros(N, LD), np.zeros(N)
    co = C_op(dim, ngl)
    for e in range(E):
        nd = conn[e]
        X = np.asarray(corners[e], np.float64)
        ov, ob, S = _op_terms(dim, ngl, X)
        cv = ov["c"]
        if plant.get("geo0"):
            cv = _op_terms(dim, ngl, np.asarray(corners[0], np.float64))[0]["c"]
        W[nd] += ov["c"]
        eW[nd] += ob["c"]
        keep = np.ones(nn, bool)
        if "skip_w" in plant and plant["skip_w"][0] == e:
            keep[plant["skip_w"][1]] = False
        np.add.at(Wv, nd[keep], cv[keep])
        rows = np.nonzero(want[nd])[0]
        if not len(rows):
            continue
        xe = x[R.dof(nd, cw)]
        ax = np.abs(xe)
        rl, rg = R.dof(rows, rw), R.dof(nd[rows], rw)
        M = ov[name]
        ye = M[rl] @ xe.astype(LD)
        val = ye.copy()
        if plant.get("geo0"):
            val = _op_terms(dim, ngl, np.asarray(corners[0], np.float64))[0][name][rl] @ xe.astype(LD)
        if "srt_half" in plant and name == "SrT":
            T = R._op_coeff(dim)["SrT"]
            T = np.where(T == 0.5, plant["srt_half"], T).astype(LD)
            o = R.point_sets(dim, ngl, X)["op"]
            Mp = np.einsum("l,rcd,ldm->lrmc", o.c, T, o.g).reshape(nn * rw, nn * cw)
            val = Mp[rl] @ xe.astype(LD)
        if "skip" in plant and plant["skip"][0] == e:
            val[np.repeat(rows == plant["skip"][1], rw)] = 0
        np.add.at(y, rg, val)
        np.add.at(sB, rg, ob[name][rl] @ ax)
        np.add.at(sS, rg, S[name][rl] @ ax)
        np.add.at(sM, rg, np.abs(ye).astype(np.float64))
        np.add.at(sA, rg, np.abs(M[rl]).astype(np.float64) @ ax)
    aW = np.abs(W).astype(np.float64)
    relW = np.repeat((eW + 1.01 * U * inc * aW) / aW, rw)
    Wr, aWr = np.repeat(Wv, rw), np.repeat(aW, rw)
    incd = np.repeat(inc, rw).astype(np.float64)
    out = Reference()
    out.rows = np.nonzero(np.repeat(want, rw))[0]
    yv = y / Wr
    ytrue = y / np.repeat(W, rw)  # (== yv without plants)
    b = sB + 1.01 * U * co * sS + 1.01 * U * (incd - 1) * sM
    out.y = yv[out.rows]
    out.bound = (b / aWr + np.abs(ytrue).astype(np.float64) * (relW + 2 * 1.01 * U))[out.rows]
    out.abound = ((sB + 1.01 * U * incd * sA) / aWr + (sA / aWr) * (relW + 2 * 1.01 * U))[out.rows]
    out.W = W
    return out
