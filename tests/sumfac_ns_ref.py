"""Reference of the seven sum-factorised no-slip operators (kle_sumfac.hip,
kle_mat_create_ns_sumfac: K, Krhs, Rw, Kfs, Krhsfs, Rwfs, K+Kfs) in
np.longdouble on a mesh, with derived entrywise bounds.

Plain numpy on top of tests/sumfac_ref.py (_element_terms: the dense K_e of an
element's own corners with its companions) and tests/sumfac_ops_ref.py
(_rw_terms: the same for Rw_e); nothing here calls pynama_amd or oracle/.  The
mesh comes in as arrays: conn [E, nn] (tensor node order), corners
[E, 2^dim, dim], cls [N dim] the class of every velocity DoF (F 0, T 1, N 2).

Operators.  SPECS restates MatNS.buildNS (mat_ns.py:47-145) as the table of
include/kle.h: a list of passes (column classes kept -> row classes that take
the sum; None: every vorticity column), the sign, and the rule of every other
row -- identity (y_i = x_i), zero (+0.0) -- plus the rows that also add -x_i
(the -1 on Kfs's tangential diagonal).  The mask is per DoF:

    y_i = sign sum_{e in i} (M_e x~_e)_i         i's class in the pass's rows,
    x~_e = the element's entries of x whose class the pass keeps, else 0.

Bound of a summed row, in sumfac_ref's form (u = 2^-53):

    bound_i = 1.01 u [ sum_e ( C (S_e |x~_e|)_i + (P_e |x~_e|)_i )
                       + (inc_i - 1) sum_e |(M_e x~_e)_i| ]

C = C_sf (sumfac_ref: the roundings of k_sumfac_elem, which the class mask does
not change -- a masked load is a selection) or C_rw (sumfac_ops_ref), S_e and
P_e the companions, inc_i the node's incidence count (the gather term).  A row
that adds -x_i makes one more addition, s + (-x_i), whose rounding is at most
u |s~ - x_i| <= u (sum_e |(M_e x~_e)_i| (1 + ...) + |x_i|):

    bound_i += 1.01 u ( sum_e |(M_e x~_e)_i| + |x_i| )

(inside the element-wise form's eps |x_i| + its sums).  Identity and zero rows
compare exactly.

The assembled product's bound (the longdouble product of the stored matrix with
x), as sumfac_ref / sumfac_ops_ref: abound_i = sum_e (B_e |x~_e|)_i + 1.01 u
inc_i sum_e (|M_e| |x~_e|)_i.  On a tangential diagonal the assembly stores
fl(S~ - 1) (Kfs) or fl(1 + fl(S~ - 1)) (K+Kfs, PETSc's form, where the operator
holds the element sums S); with |S| <= D_i = sum_e |K_e(i,i)| and b_S the
entry's assembled bound, ns_ref's

    Kfs   1.01 u (|S - 1| + b_S) |x_i|  <=  1.01 u (D_i + 1 + b_S) |x_i|
    K+Kfs 1.01 u (|S - 1| + |S| + 2 b_S) |x_i|  <=  1.01 u (2 D_i + 1 + 2 b_S) |x_i|

is added on those rows: the documented eps S |x_i| difference.

Diagonal (K, Kfs, K+Kfs; k_sumfac_diag gathered by class): the sum of K_e(i,i)
over the incident elements where the row's pass keeps the row's own class, with
sumfac_ref's C_diag bound; Kfs's tangential rows then add -1 (one more
rounding, u (D_i + 1)); 1 on identity rows, 0 elsewhere, exact.

plant, errors in the *value* only (the bounds stay the true operator's):
  {"cls": (dof, c)}     DoF `dof` takes class c
  {"swap_kfs": True}    Kfs's two passes swap their kept column sets
  {"no_minus_x": True}  the -x_i of Kfs's tangential rows is left out
  {"skip": (e, l)}      that incidence entry is left out of the gather
  {"sign": s}           the operator's sign replaced by s
"""
import numpy as np

import elem_ref as R
import sumfac_ops_ref as SO
import sumfac_ref as SF

LD = R.LD
U = R.U
F, T, N = 0, 1, 2
OPS = ("K", "Krhs", "Rw", "Kfs", "Krhsfs", "Rwfs", "K+Kfs")
RW = ("Rw", "Rwfs")
SPECS = {
    "K": dict(passes=[({F}, {F})], sign=1, ident={T, N}, zero=set()),
    "Krhs": dict(passes=[({T, N}, {F})], sign=-1, ident={T, N}, zero=set()),
    "Rw": dict(passes=[(None, {F})], sign=1, ident=set(), zero={T, N}),
    "Kfs": dict(passes=[({F, T}, {T}), ({T}, {F})], sign=1, ident=set(), zero={N}, minus_x={T}),
    "Krhsfs": dict(passes=[({N}, {F, T})], sign=-1, ident={N}, zero=set()),
    "Rwfs": dict(passes=[(None, {T})], sign=1, ident=set(), zero={F, N}),
    "K+Kfs": dict(passes=[({F, T}, {F, T})], sign=1, ident={N}, zero=set()),
}


def isin(cls, classes):
    return np.isin(cls, sorted(classes))


def wall_nodes(cls, dim):
    """Nodes with a DoF that is not free (sample_nodes' Dirichlet flag)."""
    return (np.asarray(cls).reshape(-1, dim) != F).any(axis=1)


class Reference:
    """y (longdouble), bound, abound for one operator and x; for K, Kfs and
    K+Kfs the diagonal with dbound and adbound; rows: the DoF rows they hold
    (all, or those of `nodes`); summed / ident / zero: their rule."""


def _sums(dim, ngl, conn, corners, cls, spec, rw, x, want, skip=None, bounds=True):
    """The gathered element sums of one operator: y, and with `bounds` the
    terms of the bounds and the diagonal's."""
    E, nn = conn.shape
    n = len(cls)
    dw = 1 if dim == 2 else 3
    cw = dw if rw else dim
    y = np.zeros(n, LD)
    z = {k: np.zeros(n) for k in ("S", "P", "M", "B", "A", "dS", "dP", "dM", "dB")}
    dg = np.zeros(n, LD)
    for e in range(E):
        nd = conn[e]
        rows = np.nonzero(want[nd])[0]
        if not len(rows):
            continue
        X = np.asarray(corners[e], np.float64)
        Me, S, Pm, BM = (SO._rw_terms if rw else SF._element_terms)(dim, ngl, X, rows)
        cols = R.dof(nd, cw)
        rl, rg = R.dof(rows, dim), R.dof(nd[rows], dim)
        k = np.arange(len(rl))
        for kc, rc in spec["passes"]:
            take = isin(cls[rg], rc)
            if not take.any():
                continue
            keepc = np.ones(len(cols), bool) if kc is None else isin(cls[cols], kc)
            xt = np.where(keepc, x[cols], 0.0)
            ax = np.abs(xt)
            ye = spec["sign"] * (Me @ xt.astype(LD))
            val = ye.copy()
            if skip is not None and skip[0] == e:
                val[np.repeat(rows == skip[1], dim)] = 0
            np.add.at(y, rg[take], val[take])
            if not bounds:
                continue
            for key, v in (("S", S[rl] @ ax), ("P", Pm[rl] @ ax), ("M", np.abs(ye).astype(np.float64)),
                           ("B", BM[rl] @ ax), ("A", np.abs(Me).astype(np.float64) @ ax)):
                np.add.at(z[key], rg[take], v[take])
            if not rw:
                own = take & keepc[rl]  # the row's own column is kept: it has a diagonal
                np.add.at(dg, rg[own], Me[k, rl][own])
                for key, v in (("dS", S[rl, rl]), ("dP", Pm[rl, rl]), ("dM", np.abs(Me[k, rl]).astype(np.float64)),
                               ("dB", BM[rl, rl])):
                    np.add.at(z[key], rg[own], v[own])
    return y, z, dg


def reference(dim, ngl, conn, corners, cls, name, x, nodes=None, plant=None, diag=True):
    """The mesh-level reference and bounds of operator `name` (module
    docstring); x the velocity, or the vorticity for Rw and Rwfs."""
    plant = plant or {}
    conn = np.asarray(conn)
    cls = np.asarray(cls, np.int64)
    n = len(cls)
    Nn = n // dim
    spec = SPECS[name]
    rw = name in RW
    x = np.asarray(x, np.float64)
    inc = SF.incidence(conn, Nn)
    want = np.ones(Nn, bool) if nodes is None else np.isin(np.arange(Nn), nodes)
    y, z, dg = _sums(dim, ngl, conn, corners, cls, spec, rw, x, want)
    vcls, vspec = cls, dict(spec)
    if plant:
        if "cls" in plant:
            vcls = cls.copy()
            vcls[plant["cls"][0]] = plant["cls"][1]
        if plant.get("swap_kfs"):
            (c0, r0), (c1, r1) = spec["passes"]
            vspec["passes"] = [(c1, r0), (c0, r1)]
        if "sign" in plant:
            vspec["sign"] = plant["sign"]
        if plant.get("no_minus_x"):
            vspec["minus_x"] = set()
        y = _sums(dim, ngl, conn, corners, vcls, vspec, rw, x, want, skip=plant.get("skip"), bounds=False)[0]
    incd = np.repeat(inc, dim).astype(np.float64)

    def rules(c, s):
        return isin(c, s["ident"]), isin(c, s["zero"]), isin(c, s.get("minus_x", set()))

    ident, zero, minus = rules(cls, spec)
    vi, vz, vm = rules(vcls, vspec)
    if not rw:
        y = np.where(vm, y - x.astype(LD), y)
        y = np.where(vi, x.astype(LD), y)
    y = np.where(vz, LD(0), y)
    summed = ~(ident | zero)
    C = SO.C_rw(dim, ngl) if rw else SF.C_sf(dim, ngl)
    bound = 1.01 * U * (C * z["S"] + z["P"] + (incd - 1) * z["M"])
    abound = z["B"] + 1.01 * U * incd * z["A"]
    out = Reference()
    out.rows = np.nonzero(np.repeat(want, dim))[0]
    tdiag = np.zeros(n)
    if not rw:
        ax = np.abs(x)
        bound = bound + np.where(minus, 1.01 * U * (z["M"] + ax), 0.0)
        bS = z["dB"] + 1.01 * U * incd * z["dM"]
        if name == "Kfs":
            tdiag = np.where(cls == T, 1.01 * U * (z["dM"] + 1 + bS), 0.0)
        elif name == "K+Kfs":
            tdiag = np.where(cls == T, 1.01 * U * (2 * z["dM"] + 1 + 2 * bS), 0.0)
        abound = abound + tdiag * ax
    out.y = y[out.rows]
    out.bound = np.where(summed, bound, 0.0)[out.rows]
    out.abound = np.where(summed, abound, 0.0)[out.rows]
    out.summed, out.ident, out.zero = summed[out.rows], ident[out.rows], zero[out.rows]
    if diag and name in ("K", "Kfs", "K+Kfs"):
        cd = SF.C_diag(dim, ngl)
        d = np.where(minus, dg - 1, dg)
        out.diag = np.where(ident, LD(1), np.where(zero, LD(0), d))[out.rows]
        db = 1.01 * U * (cd * z["dS"] + z["dP"] + (incd - 1) * z["dM"]) + np.where(minus, 1.01 * U * (z["dM"] + 1), 0.0)
        out.dbound = np.where(summed, db, 0.0)[out.rows]
        out.adbound = np.where(summed, z["dB"] + 1.01 * U * incd * z["dM"] + tdiag, 0.0)[out.rows]
    return out
