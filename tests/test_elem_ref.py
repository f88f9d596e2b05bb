"""The longdouble element reference (tests/elem_ref.py) against the fixtures
of the original project, the fp64 oracle inside the derived bound, and the
bound's power to tell a subtly wrong element matrix from a right one.

Figures of this file on the development host (worst |oracle - ref| / bound
over K_e, Rw_e, Rd_e; bound = 1.01 u (C S + P), elem_ref's docstring):
  unit box        2-D 0.003 (ngl 2) .. 0.119 (ngl 8), 3-D 0.002 (ngl 2) .. 0.088 (ngl 8)
  affine offset   2-D 0.006 .. 0.099, 3-D 0.005 .. 0.060
  distorted       2-D 0.015 .. 0.115, 3-D 0.008 .. 0.083
Against the plain abs-value sums, |oracle - ref| / (u S) for K_e grows from
0.5 (ngl 2) to 1.8e3 (2-D) and 1.9e3 (3-D) at ngl 8: the table cancellation
that the table error terms of P absorb.
Reference build (values and bounds of one element, all rows): 0.2 s at 3-D
ngl 5, 0.8 s at ngl 6, 6 s at ngl 7, 32 s at ngl 8 -- hence the row subset
at 3-D ngl 8 alone (4.8 s)."""
import os

import numpy as np
import pytest

import elem_ref as R
from oracle import oracle as O

G = os.path.join(os.path.dirname(__file__), "golden")
LOWER, STEP = [-1.5, 0.25, 10.0], [0.7, 0.05, 1.0]


@pytest.fixture(scope="module")
def tables():
    return np.load(os.path.join(G, "tables.npz"))


@pytest.fixture(scope="module")
def elements():
    return np.load(os.path.join(G, "elements.npz"))


def _match(a, b, tol=1e-9):
    """p with b[p[i]] == a[i] (rows of coordinates; a bijection)."""
    d = np.abs(np.asarray(a, float)[:, None, :] - np.asarray(b, float)[None, :, :]).max(-1)
    p = d.argmin(1)
    assert d.min(1).max() < tol and len(set(p.tolist())) == len(p)
    return p


def geometries(dim):
    """unit box, affine anisotropic offset box, distorted element of
    meshgen.perturbed_box -- corners in closure order."""
    from pynama_amd.meshgen import perturbed_box
    unit = R.CORN[dim].astype(float)
    aff = np.array(LOWER[:dim]) + unit * np.array(STEP[:dim])
    V, cells, _, _ = perturbed_box(dim, [2] * dim, seed=5)
    dist = O.UMesh(dim, 2, V, cells).corners()[0]
    return {"unit": unit, "affine": aff, "distorted": np.ascontiguousarray(dist)}


# ------------------------------------------------ reference vs fixtures
@pytest.mark.parametrize("n", range(1, 9))
def test_rules_match_fixture(tables, n):
    x, w = R.gauss(n)
    np.testing.assert_allclose(x.astype(float), tables[f"gauss_x_{n}"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(w.astype(float), tables[f"gauss_w_{n}"], rtol=0, atol=1e-12)
    if n >= 2:
        x, w = R.gll(n)
        np.testing.assert_allclose(x.astype(float), tables[f"lobatto_x_{n}"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(w.astype(float), tables[f"lobatto_w_{n}"], rtol=0, atol=1e-12)
        assert abs(float(w.sum()) - 2) < 1e-18 * 8 and x[0] == -1 and x[-1] == 1


@pytest.mark.parametrize("dim,ngl", [(2, n) for n in range(2, 9)] + [(3, n) for n in range(2, 6)])
def test_tables_match_fixture(tables, dim, ngl):
    """H and Hrs of the three point sets and the quadrature weights, 12
    decimals.  The fixture's node and point orders and the orientation of its
    reference frame are read from its own corner tables: HCoo* places every
    point and HCooOp every node in the element, HrsCoo gives d xi / d r."""
    Uc = (2 * R.CORN[dim] - 1).astype(float)
    rl = R.rules(ngl)
    nodes = rl["op"].x.astype(float)

    def tensor_index(pos, x1):
        idx = np.array([[int(np.argmin(np.abs(x1 - c))) for c in row] for row in pos])
        assert np.abs(x1[idx] - pos).max() < 1e-12
        return sum(idx[:, k] * len(x1) ** k for k in range(dim))

    ln = tensor_index(tables[f"HCooOp_{dim}d_{ngl}"] @ Uc, nodes)
    Pm = np.round(tables[f"HrsCoo_{dim}d_{ngl}"][0] @ Uc, 12)  # [k, d] = d xi_d / d r_k: a signed permutation
    assert np.array_equal(np.abs(Pm).sum(0), np.ones(dim)) and np.array_equal(np.abs(Pm).sum(1), np.ones(dim))
    for which, hn, hrs, coo, gps in (("full", "H", "Hrs", "HCoo", "gps"),
                                      ("red", "HRed", "HrsRed", "HCooRed", "gpsRed"),
                                      ("op", "HOp", "HrsOp", "HCooOp", "gpsOp")):
        N, _, dN, _, wq, _, _ = R.tensor(dim, rl[which])
        lq = tensor_index(tables[f"{coo}_{dim}d_{ngl}"] @ Uc, rl[which].x.astype(float))
        Hf, Hrf = tables[f"{hn}_{dim}d_{ngl}"], tables[f"{hrs}_{dim}d_{ngl}"]
        mine = N[np.ix_(lq, ln)].astype(float)
        np.testing.assert_allclose(Hf, mine, rtol=0, atol=1e-12 * max(1, np.abs(mine).max()))
        mined = np.einsum("kd,qdl->qkl", Pm, dN[np.ix_(lq, np.arange(dim), ln)].astype(float))
        np.testing.assert_allclose(Hrf, mined, rtol=0, atol=1e-12 * max(1, np.abs(mined).max()))
        np.testing.assert_allclose(tables[f"{gps}_{dim}d_{ngl}"][:, dim], wq[lq].astype(float), rtol=0, atol=1e-12)


def test_elements_match_fixture(tables, elements):
    """Every K_, Rw_, Rd_, Curl_, SrT_, DivSrT_ (and W_) entry of the
    original project's element matrices (box, skew and legacy geometries)
    inside the bound of a sequential fp64 evaluation.  The fixture's local
    node order is mapped through the geometry: HCooOp X places its nodes."""
    E = elements
    tags = sorted(k[2:] for k in E.files if k.startswith("K_"))
    assert len(tags) == 19
    worst = {}
    for tag in tags:
        dim, ngl = int(tag[0]), int(tag.split("_")[1])
        dw, ds = (1, 3) if dim == 2 else (3, 6)
        X = E["X_" + tag].reshape(2 ** dim, dim)
        p = _match(tables[f"HCooOp_{dim}d_{ngl}"] @ X, R.node_positions(dim, ngl, X))
        ref = dict(zip(("K", "Rw", "Rd"), R.ref_kle(dim, ngl, X)))
        bnd = dict(zip(("K", "Rw", "Rd"), R.bound_kle(dim, ngl, X, "oracle")))
        ov, ob = R.ref_ops(dim, ngl, X)
        ref.update(ov)
        bnd.update(ob)
        ref["W"], bnd["W"] = ref["c"], bnd["c"]
        shape = {"K": (dim, dim), "Rw": (dim, dw), "Rd": (dim, 1), "Curl": (dw, dim), "SrT": (ds, dim),
                 "DivSrT": (dim, ds), "W": None}
        for nm, rc in shape.items():
            if f"{nm}_{tag}" not in E.files:
                continue
            fix = E[f"{nm}_{tag}"]
            if rc is None:
                mine, b = ref[nm][p], bnd[nm][p]
            else:
                ix = np.ix_(R.dof(p, rc[0]), R.dof(p, rc[1]))
                mine, b = ref[nm][ix], bnd[nm][ix]
            w, at = R.worst(fix.reshape(mine.shape), mine, b)
            worst[(nm, tag)] = w
            assert w <= 1, (nm, tag, w, at)
    k = max(worst, key=worst.get)
    print(f"ELEMREF fixtures worst err/bound {worst[k]:.3g} at {k}")


# ------------------------------------------------- the oracle's premise
@pytest.mark.parametrize("ngl", range(2, 9))
def test_product_gll_nodes_meet_the_premise(ngl):
    """libkle exports no tables; its GLL nodes show in the node coordinates
    of a one-element mesh on [-1, 1] (lower + (1 + x) / 2 * 2: the map adds
    at most 2 u of its own).  They are within EX u of the longdouble nodes."""
    import pynama_amd as pa
    x = pa.BoxMesh(2, [1, 1], [-1, -1], [1, 1], ngl).coords()[:ngl, 0]
    assert float(np.abs(x - R.gll(ngl)[0]).max()) <= R.EX * R.U


@pytest.mark.parametrize("n", range(1, 9))
def test_oracle_rules_meet_the_premise(n):
    """Nodes within EX u, weights within EW(n) u relative: what the table
    error terms of the bound assume of an fp64 rule."""
    pairs = [(R.gauss(n), O.gauss(n))] + ([(R.gll(n), O.lobatto(n))] if n >= 2 else [])
    for (x, w), (xo, wo) in pairs:
        assert float(np.abs(xo - x).max()) <= R.EX * R.U
        assert float((np.abs(wo - w) / w).max()) <= R.EW(n) * R.U


def _oracle_tensor(dim, ngl, X, ops=True):
    """The oracle's K, Rw, Rd, Curl, SrT, DivSrT, W in tensor order."""
    el = O.Element(ngl, dim)
    dw, ds = (1, 3) if dim == 2 else (3, 6)
    p = _match(el.table("cooOp", 0) @ X, R.node_positions(dim, ngl, X))
    K, Rw, Rd = el.kle(X.ravel())
    mats = [("K", K, dim, dim), ("Rw", Rw, dim, dw), ("Rd", Rd, dim, 1)]
    out = {}
    if ops:
        S, D, Cu, W = el.ops(X.ravel())
        mats += [("Curl", Cu, dw, dim), ("SrT", S, ds, dim), ("DivSrT", D, dim, ds)]
        out["c"] = np.zeros_like(W)
        out["c"][p] = W
    for nm, A, r, c in mats:
        T = np.zeros_like(A)
        T[np.ix_(R.dof(p, r), R.dof(p, c))] = A
        out[nm] = T
    return out


@pytest.mark.parametrize("geom", ["unit", "affine", "distorted"])
@pytest.mark.parametrize("dim,ngl", [(d, n) for d in (2, 3) for n in range(2, 9)])
def test_oracle_within_bound(dim, ngl, geom):
    """|oracle - ref| <= 1.01 u (C S + P) entry by entry, C the oracle's own
    (sequential) count; the collocation blocks inside theirs.  At 3-D ngl 8
    the rows of tile_rows (all columns) and no collocation blocks: the
    oracle's dense loops over them take 10 s there, and the device's blocks
    are compared at that order in tests/test_gpu_elem_ref.py."""
    X = geometries(dim)[geom]
    ne = ngl ** dim
    rows = R.compare_rows(dim, ngl)
    orc = _oracle_tensor(dim, ngl, X, ops=rows is None)
    ref = R.ref_kle(dim, ngl, X, rows)
    bnd = R.bound_kle(dim, ngl, X, "oracle", rows)
    S = R.abs_kle(dim, ngl, X, rows)
    rsel = slice(None) if rows is None else R.dof(rows, dim)
    msg = []
    for nm, r, b, s in zip(("K", "Rw", "Rd"), ref, bnd, S):
        w, at = R.worst(orc[nm][rsel], r, b)
        ws, _ = R.worst(orc[nm][rsel], r, R.U * s)
        msg.append(f"{nm} {w:.3g} at {at} ({ws:.3g} u S)")
        assert w <= 1, (nm, w, at)
    ov, ob = R.ref_ops(dim, ngl, X) if rows is None else ({}, {})
    for nm in ov:
        w, at = R.worst(orc[nm], ov[nm], ob[nm])
        msg.append(f"{nm} {w:.3g}")
        assert w <= 1, (nm, w, at)
        if nm != "c":  # exact zeros of the formula are exact zeros of the oracle
            assert not orc[nm][ob[nm] == 0].any()
    print(f"ELEMREF oracle {dim}d ngl {ngl} {geom}: " + ", ".join(msg))


# ------------------------------------------------- the check discriminates
PLANTS = {"a": {"w_full": 1 + 1e-10}, "b": {"alpha_w": 1e2 * (1 + 1e-11)}, "c": {"drop_red": True},
          "d": {"dh_full": 1 + 1e-9},
          # a tenth / a twentieth of (a) and (d): below the old check on Rw_e too
          "a2": {"w_full": 1 + 1e-11}, "d2": {"dh_full": 1 + 5e-11}}


@pytest.mark.parametrize("dim,ngl", [(3, 4), (3, 5), (3, 7), (2, 8)])
def test_check_discriminates(dim, ngl):
    """The reference with a planted error in place of the implementation:
    (a) full-rule weights (1 + 1e-10), (b) alpha_w (1 + 1e-11), (c) the last
    reduced Gauss point left out, (d) one dh entry of the full table
    (1 + 1e-9) are each outside the bound of every kernel's count on at
    least one entry.

    The old check, max |diff| <= 1e-12 max |ref|: (a) and (d) pass it on K_e
    -- (d) at every order here, 3.4e-13 .. 3.9e-13; (a) with 6.8e-13 ..
    9.4e-13 except at 3-D ngl 4, where 1.3e-12 is just caught.  On Rw_e it
    catches both (4e-12 .. 1.3e-11: E is a hundredth of a_w F there), so
    (a2) = (a) / 10 and (d2) = (d) / 20 are planted too: they pass the old
    check on K_e and Rw_e alike and the bound still flags them."""
    X = R.CORN[dim].astype(float)
    ne = ngl ** dim
    # "at least one entry" is the claim: at 3-D ngl 7 the first and last 8
    # rows and 8 random ones (the seven planted references of the full matrix
    # take 36 s, these 4 s)
    rows = np.r_[0:8, ne - 8:ne, np.random.default_rng(1).choice(ne, 8)] if ne > 216 else None
    ref = R.ref_kle(dim, ngl, X, rows)
    bnds = [R.bound_kle(dim, ngl, X, kernel, rows) for kernel in ("mfma", "valu", "oracle")]

    def old_ok(bad, good):
        return float(np.abs(bad - good).max()) <= 1e-12 * float(np.abs(good).max())

    for nm, plant in PLANTS.items():
        bad = R.ref_kle(dim, ngl, X, rows, plant=plant)
        for bnd in bnds:
            w = [R.worst(b.astype(float), r, bb)[0] for b, r, bb in zip(bad[:2], ref[:2], bnd[:2])]
            assert max(w) > 1, (nm, w)
        if nm in ("a", "d") and not (nm == "a" and ngl == 4):
            assert old_ok(bad[0], ref[0]), nm
        if nm in ("a2", "d2"):
            assert old_ok(bad[0], ref[0]) and old_ok(bad[1], ref[1]), nm
        if nm == "c":
            assert not old_ok(bad[0], ref[0])
    # and the reference itself, rounded to fp64, is inside
    for r, bb in zip(ref, bnds[0]):
        assert R.worst(r.astype(float), r, bb)[0] <= 1


# ---------------------------------------------------- structure of K_e
@pytest.mark.parametrize("geom", ["unit", "affine", "distorted"])
@pytest.mark.parametrize("dim,ngl", [(2, 3), (2, 8), (3, 2), (3, 5)])
def test_structure_in_longdouble(dim, ngl, geom):
    """K_e = K_e^T; K_e applied to a rigid translation vanishes (every part
    of K_e is a derivative of the shape functions, which sum to one: zero for
    the gradient, divergence and curl parts alike); sum(c) = |element| --
    all to the longdouble rounding of the sums, 2^-11 of the fp64 bound."""
    X = geometries(dim)[geom]
    K, _, _ = R.ref_kle(dim, ngl, X)
    BK = R.bound_kle(dim, ngl, X, "oracle")[0] * 2.0 ** -11
    assert (np.abs(K - K.T).astype(float) <= BK + BK.T).all()
    for a in range(dim):
        t = np.zeros(K.shape[1], R.LD)
        t[a::dim] = 1
        assert (np.abs(K @ t).astype(float) <= BK.sum(1)).all()
    ps = R.point_sets(dim, ngl, X)
    if dim == 2:  # shoelace formula on the corners
        x, y = X[:, 0].astype(R.LD), X[:, 1].astype(R.LD)
        vol = abs(float((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())) / 2
    elif geom == "distorted":  # det J has degree 2 per direction: Gauss(2) is exact
        rg = R.Rule(R.gll(2)[0], *R.gauss(2))
        _, _, _, _, wq, _, xi = R.tensor(3, rg)
        vol = float((wq * R.geometry(3, xi, X)[0]).sum())
    else:
        vol = float(np.prod(X.max(0) - X.min(0)))
    for k in ("full", "op") if ngl >= 3 else ("full",):  # GLL(2) is exact to degree 1 only
        c = ps[k].c
        assert (c > 0).all()
        assert abs(float(c.sum()) - vol) <= 1e-15 * vol, (k, float(c.sum()), vol)


# ------------------------------------- the product's meshes, the assembly
@pytest.mark.parametrize("dim", [2, 3])
def test_product_mesh_orders(dim, tmp_path):
    """mesh.corners() (closure order) and mesh.conn() (tensor order, x
    fastest) of the product's box and Gmsh meshes are the orders the
    reference assumes: the multilinear map of an element's corners places
    its nodes where mesh.coords() has them."""
    import pynama_amd as pa
    from pynama_amd.mesh import UnstructuredMesh
    from pynama_amd.meshgen import perturbed_box, write_gmsh
    V, Cc, F, T = perturbed_box(dim, [2] * dim, seed=13)
    path = str(tmp_path / "p.msh")
    write_gmsh(path, dim, V, Cc, F, T)
    nel = [3, 1, 2] if dim == 3 else [3, 2]
    hi = [a + n * h for a, n, h in zip(LOWER, nel, STEP)]
    for ngl in (2, 4, 5):
        for m in (UnstructuredMesh.from_gmsh(path, ngl), pa.BoxMesh(dim, nel, LOWER[:dim], hi, ngl)):
            co, cn, X = m.coords(), m.conn(), m.corners()
            for e in range(len(cn)):
                pos = R.node_positions(dim, ngl, X[e]).astype(float)
                assert np.abs(pos - co[cn[e]]).max() <= 4e-16 * max(1.0, np.abs(pos).max())


def test_assemble_ref_matches_oracle():
    """assemble_ref against the oracle's assembly on a box with partial
    Dirichlet faces: patterns exact (explicit zeros kept), values inside the
    scattered bound."""
    import pynama_amd as pa
    dim, ngl, nel = 3, 3, [2, 3, 2]
    om = O.BoxMesh(dim, nel, [0, 0, 0], [1, 1, 1], ngl)
    m = pa.BoxMesh(dim, nel, [0, 0, 0], [1, 1, 1], ngl)
    flag = np.zeros(m.N, bool)
    flag[m.face_nodes(["left", "down"])] = True
    ref = R.assemble_ref(dim, ngl, m.conn(), m.corners(), flag, kernel="oracle")
    K, Kr, Rw = om.assemble_fs(flag.astype(np.uint8))
    Cu, S, D, _ = om.assemble_ops()
    for nm, A in (("K", K), ("Krhs", Kr), ("Rw", Rw), ("Curl", Cu), ("SrT", S), ("DivSrT", D)):
        v, b, pat = ref[nm]
        rp, rx, rv = R.csr_of(v, pat)
        np.testing.assert_array_equal(rp, A.indptr, err_msg=nm)
        np.testing.assert_array_equal(rx, A.indices, err_msg=nm)
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
        w, at = R.worst(A.data, rv, b[rows, rx])
        assert w <= 1, (nm, w, at)
