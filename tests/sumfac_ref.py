"""Reference of the sum-factorised element-wise K and Krhs (kle_sumfac.hip) in
np.longdouble, with a derived entrywise bound.

Plain numpy on top of tests/elem_ref.py; nothing here calls pynama_amd or
oracle/.  The mesh comes in as arrays: conn [E, nn] (mesh.conn(), tensor node
order), corners [E, 2^dim, dim] (mesh.corners()), dirflag [N].

Reference.  y_ref = sum_e S_e^T ref_kle(X_e) x~_e in longdouble: the dense
element matrix of elem_ref from the element's own corners, x~_e the element's
entries of x masked as the operator masks (K drops the Dirichlet columns, Krhs
keeps only them and is negated); Dirichlet rows y_i = x_i.

Bound, in elem_ref's form (u = 2^-53):

    bound_i = 1.01 u [ sum_{e in i} ( C_sf (S_e |x~_e|)_i + (P_e |x~_e|)_i )
                       + (inc_i - 1) sum_{e in i} |(K_e x~_e)_i| ]

S_e = abs_kle (every term of the factored sums replaced by its absolute value:
the companion of a factorised evaluation), P_e = prop_kle (the errors of the
operands the kernel holds -- 1-D tables, c_q, inv J -- to first order), inc_i
the number of elements the node lies in (the gather adds inc_i numbers: at most
inc_i - 1 roundings, the first addition to 0.0 being exact).  Dirichlet rows
compare exactly (bound 0).

C_sf counts the roundings one ws entry passes through in k_sumfac_elem as
written, a line sum of n products counted n (n products and n - 1 additions on
its first term, the addition to the 0.0 accumulator exact; fewer with fused
multiply-adds).  n = ngl, P the rule's 1-D points (ngl or ngl - 1):

  forward passes         x, y (, z) line sums over the n nodes: DIM n
  physical gradient      sum_k invJ[b][k] g[a][k]: DIM
  flux                   full: c G: 1.  reduced: the diagonal c (a_d div), div
                         DIM - 1 additions: DIM + 1; off the diagonal
                         c (a_w (G_ab - G_ba)): 3 <= DIM + 1
  back with invJ^T       DIM
  transposed passes      3-D: z over P, y over 2 P terms (dh c1 + h c2), x over
                         2 P terms: 5 P.  2-D: y over P, x over 2 P: 3 P
  rule sum               full + reduced: 1

  3-D  full 3n + 3 + 1 + 3 + 5n = 8n + 7, reduced 3n + 3 + 4 + 3 + 5(n - 1) = 8n + 5
  2-D  full 2n + 2 + 1 + 2 + 3n = 5n + 5, reduced 2n + 2 + 3 + 2 + 3(n - 1) = 5n + 4
  C_sf = max over the rules + 1:  8 n + 8 (3-D),  5 n + 6 (2-D)     -- C_sf()

The diagonal (k_sumfac_diag; same form with the diagonal entries of K_e, S_e,
P_e): reference derivative DIM - 1 products, physical gradient DIM, square 1,
|grad N|^2 DIM - 1 additions: 3 DIM - 1; full: c n2 and nqF additions; reduced:
n2 - ga, a_w (.), a_d ga + (.), c (.) and nqR additions; the final sum 1:
  C_diag = max(3 DIM + nqF, 3 DIM + 3 + nqR) + 1                    -- C_diag()

Beside it, the bound of the assembled product (the longdouble product of the
device's stored K with x): per entry elem_ref.assemble_ref's
sum_e max(BK_e, BK_e^T) + 1.01 u cnt |K|, applied to |x~| with cnt_ij <= inc_i:

    abound_i = sum_e (max(BK_e, BK_e^T) |x~_e|)_i + 1.01 u inc_i sum_e (|K_e| |x~_e|)_i

For large elements (3-D ngl >= 7) `nodes=` restricts the reference to a sample
of global node rows (sample_nodes: every valence class of the mesh -- vertex,
edge, face and interior nodes -- and element-local indices on both sides of
the kernel's 256-thread loop boundary); S, P and BK are fp64 and always whole.
"""
import numpy as np

import elem_ref as R

LD = R.LD
U = R.U


def C_sf(dim, ngl):
    return 8 * ngl + 8 if dim == 3 else 5 * ngl + 6


def C_diag(dim, ngl):
    nqF, nqR = R.npoints(dim, ngl)
    return max(3 * dim + nqF, 3 * dim + 3 + nqR) + 1


# ------------------------------------------------- the factorised formula
def sumfac_apply(dim, ngl, X, xe, dtype=LD, plant=None, flip=False):
    """K_e x_e by the sum-factorised formula the kernel evaluates, in `dtype`
    (tables and geometry formed in longdouble and rounded to it).  xe [nn dim]
    node-major.  plant: elem_ref.rules' plants and "alpha_w"; flip: the sign
    of the grad u^T term flipped (a planted error)."""
    plant = plant or {}
    rl = R.rules(ngl, plant)
    ps = R.point_sets(dim, ngl, X, plant)
    aw = dtype(plant.get("alpha_w", R.ALPHA_W))
    ad = dtype(R.ALPHA_D)
    u = np.asarray(xe, dtype=dtype).reshape((ngl,) * dim + (dim,))  # [(k,) j, i, a]
    out = np.zeros((ngl ** dim, dim), dtype)
    for name in ("full", "red"):
        h, dh = rl[name].h.astype(dtype), rl[name].dh.astype(dtype)
        P = h.shape[0]
        c, Ji = ps[name].c.astype(dtype), ps[name].Ji.astype(dtype)
        if dim == 3:
            fw = ["zk,yj,xi,kjia->zyxa"] * 3
            tabs = [(h, h, dh), (h, dh, h), (dh, h, h)]  # (z, y, x) tables of d/dxi_0, _1, _2
            bw = "zk,yj,xi,zyxa->kjia"
        else:
            fw = ["yj,xi,jia->yxa"] * 2
            tabs = [(h, dh), (dh, h)]
            bw = "yj,xi,yxa->jia"
        g = np.stack([np.einsum(f, *t, u) for f, t in zip(fw, tabs)], -1).reshape(P ** dim, dim, dim)  # [q, a, k]
        G = np.einsum("qbk,qak->qab", Ji, g)  # (grad u)_ab = d_b u^a
        if name == "full":
            F = c[:, None, None] * G
        else:
            div = np.einsum("qaa->q", G)
            GT = G.transpose(0, 2, 1)
            T = aw * (G + GT if flip else G - GT)
            for a in range(dim):
                T[:, a, a] = ad * div if not flip else ad * div + T[:, a, a]
            F = c[:, None, None] * T
        Fr = np.einsum("qbk,qab->qak", Ji, F).reshape((P,) * dim + (dim, dim))
        for k, t in enumerate(tabs):
            out += np.einsum(bw, *t, Fr[..., k]).reshape(ngl ** dim, dim)
    return out.ravel()


# --------------------------------------------------------- mesh reference
def incidence(conn, N):
    """inc [N]: the number of elements each node lies in."""
    return np.bincount(np.asarray(conn).ravel(), minlength=N)


def sample_nodes(conn, ngl, dim, dirflag, per_class=4, seed=0):
    """Global node rows for the large elements: `per_class` free nodes of every
    valence (interior 1, face 2, edge 4, vertex 8 on a box of hexes), interior
    nodes with an element-local index below and from 256 on, and a few
    Dirichlet nodes."""
    conn = np.asarray(conn)
    N = len(dirflag)
    inc = incidence(conn, N)
    rng = np.random.default_rng(seed)
    free = ~np.asarray(dirflag, bool)
    out = set()
    for v in np.unique(inc[free]):
        cand = np.nonzero(free & (inc == v))[0]
        out.update(rng.choice(cand, min(per_class, len(cand)), replace=False).tolist())
    loc = np.zeros(N, np.int64)
    loc[conn.ravel()] = np.tile(np.arange(conn.shape[1]), conn.shape[0])
    for sel in (loc < 256, loc >= 256):
        cand = np.nonzero(free & (inc == 1) & sel)[0]
        if len(cand):
            out.update(rng.choice(cand, min(2 * per_class, len(cand)), replace=False).tolist())
            out.update((int(cand[np.argmin(np.abs(loc[cand] - 255.5))]),))
    cand = np.nonzero(~free)[0]
    out.update(rng.choice(cand, min(per_class, len(cand)), replace=False).tolist())
    return np.array(sorted(out))


_TERMS = {}


def _element_terms(dim, ngl, X, rows):
    """K_e (longdouble, the node rows `rows`), S_e, P_e and the symmetrised
    assembly bound BK_e (fp64, whole) of one element; kept for the next
    operator on the same mesh."""
    key = (dim, ngl, X.tobytes(), np.asarray(rows, np.int64).tobytes())
    if key not in _TERMS:
        if len(_TERMS) >= 64:
            _TERMS.clear()
        Sall, Pall = R.abs_kle(dim, ngl, X), R.prop_kle(dim, ngl, X)
        BK = R.bound_from(Sall, Pall, dim, ngl, "mfma")[0]
        _TERMS[key] = (R.ref_kle(dim, ngl, X, rows=rows)[0], Sall[0], Pall[0], np.maximum(BK, BK.T))
    return _TERMS[key]


class Reference:
    """y (longdouble), bound, abound for one operator and x, the diagonal with
    its bound dbound and the assembled diagonal's bound adbound (the entry
    bound of abound on the diagonal); rows: the DoF rows they hold (all, or
    those of `nodes`), dird: which of them are Dirichlet rows."""


def reference(dim, ngl, conn, corners, dirflag, which, x, nodes=None, apply=None, skip=None, diag=True):
    """The mesh-level reference and bounds (module docstring).  apply(e, X, xt)
    -> K_e xt replaces the element product of the *value* (planted errors);
    skip = (e, l): that incidence entry is left out of the value's gather."""
    conn = np.asarray(conn)
    E, nn = conn.shape
    N = len(dirflag)
    dirn = np.asarray(dirflag, bool)
    inc = incidence(conn, N)
    keepn = ~dirn if which == "K" else dirn
    sgn = 1 if which == "K" else -1
    x = np.asarray(x, np.float64)
    want = np.ones(N, bool) if nodes is None else np.isin(np.arange(N), nodes)
    y = np.zeros(N * dim, LD)
    sS, sP, sM, sB, sKa = (np.zeros(N * dim) for _ in range(5))
    dg, dS, dP, dM, dB = np.zeros(N * dim, LD), np.zeros(N * dim), np.zeros(N * dim), np.zeros(N * dim), np.zeros(N * dim)
    cs, cd = C_sf(dim, ngl), C_diag(dim, ngl)
    for e in range(E):
        nd = conn[e]
        rows = np.nonzero(want[nd] & ~dirn[nd])[0]
        if not len(rows):
            continue
        X = np.asarray(corners[e], np.float64)
        cols = R.dof(nd, dim)
        xt = np.where(np.repeat(keepn[nd], dim), x[cols], 0.0)
        ax = np.abs(xt)
        rl, rg = R.dof(rows, dim), R.dof(nd[rows], dim)
        Ke, S, Pm, BK = _element_terms(dim, ngl, X, rows)
        ye = sgn * (Ke @ xt.astype(LD))
        if apply is not None:
            val = sgn * np.asarray(apply(e, X, xt), LD)[rl]
        else:
            val = ye.copy()
        if skip is not None and skip[0] == e:
            val[np.repeat(rows == skip[1], dim)] = 0
        np.add.at(y, rg, val)
        np.add.at(sS, rg, S[rl] @ ax)
        np.add.at(sP, rg, Pm[rl] @ ax)
        np.add.at(sM, rg, np.abs(ye).astype(np.float64))
        np.add.at(sB, rg, BK[rl] @ ax)
        np.add.at(sKa, rg, np.abs(Ke).astype(np.float64) @ ax)
        if diag and which == "K":
            k = np.arange(len(rl))
            np.add.at(dg, rg, Ke[k, rl])
            np.add.at(dS, rg, S[rl, rl])
            np.add.at(dP, rg, Pm[rl, rl])
            np.add.at(dM, rg, np.abs(Ke[k, rl]).astype(np.float64))
            np.add.at(dB, rg, BK[rl, rl])
    incd = np.repeat(inc, dim).astype(np.float64)
    dird = np.repeat(dirn, dim)
    out = Reference()
    out.rows = np.nonzero(np.repeat(want, dim))[0]
    out.dird = dird[out.rows]
    out.y = np.where(dird, x.astype(LD), y)[out.rows]
    out.bound = np.where(dird, 0.0, 1.01 * U * (cs * sS + sP + (incd - 1) * sM))[out.rows]
    out.abound = np.where(dird, 0.0, sB + 1.01 * U * incd * sKa)[out.rows]
    if which == "K":
        out.diag = np.where(dird, LD(1), dg)[out.rows]
        out.dbound = np.where(dird, 0.0, 1.01 * U * (cd * dS + dP + (incd - 1) * dM))[out.rows]
        out.adbound = np.where(dird, 0.0, dB + 1.01 * U * incd * dM)[out.rows]
    else:
        out.diag = np.where(dird, LD(1), LD(0))[out.rows]
        out.dbound = out.adbound = np.zeros(len(out.rows))
    return out


def csr_mult(csr, x):
    """Longdouble product of a CSR triple (indptr, indices, data) with x."""
    ip, ix, d = csr
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    out = np.zeros(len(ip) - 1, LD)
    np.add.at(out, rows, np.asarray(d).astype(LD) * np.asarray(x)[ix].astype(LD))
    return out


def csr_diag(csr):
    ip, ix, d = csr
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    out = np.zeros(len(ip) - 1)
    on = np.asarray(ix) == rows
    out[rows[on]] = np.asarray(d)[on]
    return out
