"""The element-wise no-slip operators (Mat.createNSElement, kle_elem.hip) and
the matrix-free no-slip KLE system (MatNS.build(nsType="element"),
-kle_ns_type element) against the assembled MatNS of the same mesh, one rank.

Reference of every product: the assembled matrix's getValuesCSR() multiplied on
the host in np.longdouble.  Bound of a product entry i (the one of
test_gpu_elem.py and test_gpu_matfree.py):

    |y_i - ref_i| <= n eps B_i + delta Kmax X_i

n = nc + 8 (nc the columns of the element matrix: the terms of one element row
plus the element sums), B_i the sum over incident elements of |M_e0| |x_e| over
the columns the operator keeps for row i's class, Kmax = max |M_e0|, X_i the
sum over incident elements of the 1-norm of the kept x_e, delta the largest
|M_e - M_e0| / Kmax over the mesh's elements (kle_element_kle), required
<= 2e-12.  Kfs's tangential rows add eps |x_i| (the -1 on their diagonal).
Identity rows are compared bit for bit, zero rows must be +0.0.

Every operator is a list of passes (column classes kept -> row classes taking
the sum) and a rule on every other row -- the table of kle.h, restated in
SPECS below from MatNS.buildNS (mat_ns.py:47-145).

Selection: a NaN in a column class a pass drops must not reach that pass's
rows, which stay bit-equal to the clean product.  Identity rows return x_i
itself, so where the dropped class is also an identity row's own (K, Krhs:
T and N; Krhsfs, K+Kfs: none dropped but N) that row returns the NaN it was
given -- bit for bit x_i, as the table says."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
G = os.path.join(os.path.dirname(__file__), "golden")
F, T, N = 0, 1, 2
OPS = ("K", "Krhs", "Rw", "Kfs", "Krhsfs", "Rwfs", "K+Kfs")
# passes: (column classes kept (None: every vorticity column), row classes taking the sum);
# ident / zero: the rule of the other rows; minus_x: rows that also add -x_i
SPECS = {
    "K": dict(passes=[({F}, {F})], sign=1, ident={T, N}, zero=set()),
    "Krhs": dict(passes=[({T, N}, {F})], sign=-1, ident={T, N}, zero=set()),
    "Rw": dict(passes=[(None, {F})], sign=1, ident=set(), zero={T, N}),
    "Kfs": dict(passes=[({F, T}, {T}), ({T}, {F})], sign=1, ident=set(), zero={N}, minus_x={T}),
    "Krhsfs": dict(passes=[({N}, {F, T})], sign=-1, ident={N}, zero=set()),
    "Rwfs": dict(passes=[(None, {T})], sign=1, ident=set(), zero={F, N}),
    "K+Kfs": dict(passes=[({F, T}, {F, T})], sign=1, ident={N}, zero=set()),
}
CAVITY = {"up": [2, 0], "down": [0, 0], "left": [0, 0], "right": [0, 0]}
SIX = {"up": [1, 0, 0.5], "down": [0, 0, 0], "left": [0, 0, 0], "right": [0, 0, 0], "front": [0, 0, 0],
       "back": [0, 0, 0]}
MESHES = {
    "cavity": dict(dim=2, nelem=[4, 4], ngl=3, walls=CAVITY),
    "three_walls": dict(dim=2, nelem=[5, 4], ngl=3, walls={"left": [0, 1], "up": [2, 0], "down": [0, 0]}),
    "four_walls": dict(dim=2, nelem=[6, 5], ngl=4,
                       walls={"down": [0, 0], "up": [1.5, 0], "right": [0, -0.5], "left": [0, 0]}),
    "ngl5_2d": dict(dim=2, nelem=[3, 2], ngl=5, walls=CAVITY),
    "six_walls": dict(dim=3, nelem=[3, 2, 2], ngl=3, walls=SIX),
    "up_down_3d": dict(dim=3, nelem=[2, 2, 2], ngl=5, walls={"up": [1, 0, 0.5], "down": [0, 0, 0]}),
    "one_free_node": dict(dim=3, nelem=[1, 1, 1], ngl=3, walls=SIX),
    "ngl7": dict(dim=3, nelem=[1, 1, 2], ngl=7, walls=SIX),
}


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


def _domain(pa, dim, nelem, ngl, walls):
    cfg = {"domain": {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": [0] * dim, "upper": [1] * dim}},
           "boundary-conditions": {"no-slip": walls}}
    dom = pa.Domain()
    dom.configure(cfg)
    dom.setUp()
    return dom


def _classes(dom, n):
    cls = np.zeros(n, np.int8)
    cls[np.asarray(sorted(dom.getTangDofs(collect=True)), np.int64)] = T
    cls[np.asarray(sorted(dom.getNormalDofs(collect=True)), np.int64)] = N  # normal wins (mat_ns.py:60-62)
    return cls


def _isin(cls, classes):
    return np.isin(cls, sorted(classes))


def _ref_mult(csr, x):
    ip, ix, d = csr
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    out = np.zeros(len(ip) - 1, np.longdouble)
    np.add.at(out, rows, d.astype(np.longdouble) * x[ix].astype(np.longdouble))
    return out


def _csr_diag(csr):
    ip, ix, d = csr
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    out = np.zeros(len(ip) - 1)
    on = ix == rows
    out[rows[on]] = d[on]
    return out


class Case:
    """One mesh: the assembled MatNS, the seven element-wise operators, x and w,
    the references and the bound's terms, computed once and left unchanged."""

    def __init__(self, pa, dim, nelem, ngl, walls):
        from pynama_amd._lib import call
        from pynama_amd.petsc import Mat
        self.dim, self.ngl = dim, ngl
        self.dw = dw = 1 if dim == 2 else 3
        self.dom = dom = _domain(pa, dim, nelem, ngl, walls)
        self.mat = mat = pa.MatNS()
        mat.setDomain(dom)
        mat.build(buildOperators=False)
        mesh = dom.mesh
        self.n, self.nw = mesh.N * dim, mesh.N * dw
        self.cls = _classes(dom, self.n)
        self.asm = {"K": mat.K, "Krhs": mat.Krhs, "Rw": mat.Rw, "Kfs": mat.Kfs, "Krhsfs": mat.Krhsfs,
                    "Rwfs": mat.Rwfs, "K+Kfs": mat.getKplusKfs()}
        self.csr = {k: A.getValuesCSR() for k, A in self.asm.items()}
        self.op = {k: Mat.createNSElement(mesh, k) for k in OPS}
        nn = ngl ** dim
        self.nd, self.ncw = nd, ncw = dim * nn, dw * nn
        ctx = pa.get_ctx()
        E = mesh.E
        Ke, Rwe = np.zeros((nd, nd)), np.zeros((nd, ncw))
        call("kle_element_kle", ctx.h, mesh._h, 0, Ke, Rwe)
        self.K0, self.R0 = Ke.copy(), Rwe.copy()
        self.Kmax, self.Rmax = np.abs(self.K0).max(), np.abs(self.R0).max()
        self.deltaK = self.deltaR = 0.0
        for e in range(1, E):
            call("kle_element_kle", ctx.h, mesh._h, e, Ke, Rwe)
            self.deltaK = max(self.deltaK, np.abs(Ke - self.K0).max() / self.Kmax)
            self.deltaR = max(self.deltaR, np.abs(Rwe - self.R0).max() / self.Rmax)
        conn = mesh.conn()
        self.gd = (conn[:, :, None] * dim + np.arange(dim)[None, None, :]).reshape(E, nd)
        self.gw = (conn[:, :, None] * dw + np.arange(dw)[None, None, :]).reshape(E, ncw)
        rng = np.random.default_rng(20241020)
        self.x = rng.uniform(-1, 1, self.n)
        self.w = rng.uniform(-1, 1, self.nw)
        self.ref = {k: _ref_mult(self.csr[k], self.w if k in ("Rw", "Rwfs") else self.x) for k in OPS}
        self.bound = {k: self._bound(k, self.w if k in ("Rw", "Rwfs") else self.x) for k in OPS}

    def _bound(self, name, x):
        S = SPECS[name]
        rw = name in ("Rw", "Rwfs")
        M0, g, delta, mmax = (self.R0, self.gw, self.deltaR, self.Rmax) if rw else \
            (self.K0, self.gd, self.deltaK, self.Kmax)
        ncols = M0.shape[1]
        B, X = np.zeros(self.n), np.zeros(self.n)
        for cols, rows in S["passes"]:
            xe = np.abs(x)[g]
            if cols is not None:
                xe = np.where(_isin(self.cls[g], cols), xe, 0.0)
            take = _isin(self.cls[self.gd], rows)
            np.add.at(B, self.gd, np.where(take, xe @ np.abs(M0).T, 0.0))
            np.add.at(X, self.gd, np.where(take, xe.sum(axis=1)[:, None], 0.0))
        b = (ncols + 8) * EPS * B + delta * mmax * X
        if "minus_x" in S:
            b = b + np.where(_isin(self.cls, S["minus_x"]), EPS * np.abs(x), 0.0)
        return b

    def product(self, name, x):
        A = self.op[name]
        xv = A.createVecRight()
        xv.setArray(x)
        return (A * xv).getArray()

    def rows(self, classes):
        return _isin(self.cls, classes)


@functools.lru_cache(maxsize=None)
def _case_cached(name):
    import pynama_amd
    return Case(pynama_amd, **MESHES[name])


def _case(pa, name):
    return _case_cached(name)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _check_product(c, name, y, x, label):
    """y = op x against the reference and the bound of (c, name); x the clean input."""
    S = SPECS[name]
    err = np.abs(y.astype(np.longdouble) - c.ref[name]).astype(np.float64)
    bound = c.bound[name]
    summed = ~c.rows(S["ident"] | S["zero"])
    worst = float(np.max(err[summed] / np.where(bound[summed] > 0, bound[summed], 1.0))) if summed.any() else 0.0
    print(f"{label} {name}: max err/bound {worst:.3g}")
    assert np.all(err[summed] <= bound[summed]), (label, name, worst)
    ident, zero = c.rows(S["ident"]), c.rows(S["zero"])
    if ident.any():  # (Rw, Rwfs have none: their x is the vorticity, of another length in 2-D)
        np.testing.assert_array_equal(_bits(y[ident]), _bits(x[ident]))
    assert np.all(y[zero] == 0.0) and not np.any(np.signbit(y[zero]))
    return worst


# ------------------------------------------------------------ 1. the products
@pytest.mark.parametrize("mesh", list(MESHES))
def test_products_equal_assembled(pa, mesh):
    c = _case(pa, mesh)
    assert c.deltaK <= 2e-12 and c.deltaR <= 2e-12, (c.deltaK, c.deltaR)
    worst = {}
    for name in OPS:
        A = c.op[name]
        rw = name in ("Rw", "Rwfs")
        ncol = c.nw if rw else c.n
        assert A.getFormat() == "elem"
        assert A.getSize() == (c.n, ncol) and A.getLocalSize() == (c.n, ncol)
        info = A.getInfo()
        assert info["format"] == "elem" and info["nz_used"] == 0 and info["spmv_bytes"] > 0
        assert "k_elem_gemm" in A.spmvKernel() and "k_elem_gather_cls" in A.spmvKernel()
        x = c.w if rw else c.x
        worst[name] = _check_product(c, name, c.product(name, x), x, mesh)
        S = SPECS[name]
        if mesh != "one_free_node" or name in ("K", "K+Kfs", "Kfs"):
            summed = ~c.rows(S["ident"] | S["zero"])
            assert np.any(c.product(name, x)[summed] != 0.0), name
    print(f"{mesh}: deltaK {c.deltaK:.2e} deltaR {c.deltaR:.2e} worst err/bound "
          f"{max(worst.values()):.3g} ({max(worst, key=worst.get)})")


def test_class_counts(pa):
    """The meshes reach what they are there for."""
    assert _case(pa, "one_free_node").rows({F}).sum() == 3
    c = _case(pa, "three_walls")
    assert c.rows({F}).sum() and c.rows({T}).sum() and c.rows({N}).sum()
    c = _case(pa, "ngl5_2d")
    assert c.nd == 50 and c.nd % 16 and c.ncw == 25 and c.ncw % 4
    assert _case(pa, "ngl7").nd == 1029


# ------------------------------------------------------------ 2. selection
@pytest.mark.parametrize("mesh", ["cavity", "three_walls", "six_walls", "up_down_3d"])
def test_dropped_columns_are_never_read(pa, mesh):
    c = _case(pa, mesh)
    for name in ("K", "Krhs", "Kfs", "Krhsfs", "K+Kfs"):
        S = SPECS[name]
        clean = c.product(name, c.x)
        for cols, rows in S["passes"]:
            dropped = ~c.rows(cols)
            if not dropped.any():
                continue
            x = np.where(dropped, np.nan, c.x)
            y = c.product(name, x)
            take = c.rows(rows)
            # a row that also adds -x_i reads its own entry: its class is a kept column here
            assert np.all(np.isfinite(y[take])), name
            np.testing.assert_array_equal(_bits(y[take]), _bits(clean[take]), err_msg=name)
            ident, zero = c.rows(S["ident"]), c.rows(S["zero"])
            np.testing.assert_array_equal(_bits(y[ident]), _bits(x[ident]), err_msg=name)
            assert np.all(y[zero] == 0.0) and not np.any(np.signbit(y[zero]))


@pytest.mark.parametrize("mesh", ["cavity", "six_walls"])
def test_all_nan_input(pa, mesh):
    c = _case(pa, mesh)
    for name in OPS:
        S = SPECS[name]
        rw = name in ("Rw", "Rwfs")
        y = c.product(name, np.full(c.nw if rw else c.n, np.nan))
        ident, zero = c.rows(S["ident"]), c.rows(S["zero"])
        assert np.all(np.isnan(y[ident])), name
        assert np.all(y[zero] == 0.0) and not np.any(np.signbit(y[zero])), name


# ------------------------------------------------ 3. repeatability, diagonal
@pytest.mark.parametrize("mesh", ["four_walls", "up_down_3d"])
def test_repeatable(pa, mesh):
    c = _case(pa, mesh)
    for name in OPS:
        x = c.w if name in ("Rw", "Rwfs") else c.x
        y = c.product(name, x)
        for _ in range(3):
            np.testing.assert_array_equal(_bits(c.product(name, x)), _bits(y), err_msg=name)


@pytest.mark.parametrize("mesh", ["cavity", "three_walls", "ngl5_2d", "six_walls", "up_down_3d", "ngl7"])
def test_diagonal(pa, mesh):
    from pynama_amd._lib import Error
    c = _case(pa, mesh)
    terms = np.zeros(c.n)  # sum over incident elements of |K_e0 diagonal|
    np.add.at(terms, c.gd, np.broadcast_to(np.abs(np.diag(c.K0))[None, :], c.gd.shape))
    for name in ("K", "K+Kfs", "Kfs"):
        S = SPECS[name]
        d = c.op[name].getDiagonal().getArray()
        ref = _csr_diag(c.csr[name])
        ident = c.rows(S["ident"])
        np.testing.assert_array_equal(d[ident], np.ones(int(ident.sum())))
        t = terms + np.where(c.rows(S.get("minus_x", set())), 1.0, 0.0)
        err = np.abs(d - ref)
        print(f"{mesh} diag {name}: max err/bound "
              f"{float(np.max(err[~ident] / ((c.nd + 8) * EPS * t[~ident]))) if (~ident).any() else 0:.3g}")
        assert np.all(err[~ident] <= (c.nd + 8) * EPS * t[~ident]), name
    for name in ("Krhs", "Krhsfs"):
        S = SPECS[name]
        d = c.op[name].getDiagonal().getArray()
        ident = c.rows(S["ident"])
        np.testing.assert_array_equal(d, np.where(ident, 1.0, 0.0))
    for name in ("Rw", "Rwfs"):
        with pytest.raises(Error) as ei:
            c.op[name].getDiagonal()
        assert ei.value.ierr == 56


def test_mult_add_and_copy_identity_rows(pa):
    c = _case(pa, "six_walls")
    y0 = np.random.default_rng(5).uniform(-1, 1, c.n)
    for name in ("K+Kfs", "Kfs", "Rwfs"):
        A = c.op[name]
        x = c.w if name == "Rwfs" else c.x
        xv, yv, zv = A.createVecRight(), A.createVecLeft(), A.createVecLeft()
        xv.setArray(x)
        yv.setArray(y0)
        A.multAdd(xv, yv, zv)
        z = zv.getArray()
        ref = y0.astype(np.longdouble) + c.ref[name]
        err = np.abs(z.astype(np.longdouble) - ref).astype(np.float64)
        assert np.all(err <= c.bound[name] + EPS * np.abs(z)), name
    src = np.random.default_rng(6).uniform(-1, 1, c.n)
    for name in OPS:
        A = c.op[name]
        sv, dv = A.createVecLeft(), A.createVecLeft()
        sv.setArray(src)
        dv.setArray(y0)
        A.copyDirichletRows(sv, dv)
        ident = c.rows(SPECS[name]["ident"])
        np.testing.assert_array_equal(_bits(dv.getArray()), _bits(np.where(ident, src, y0)), err_msg=name)


# ------------------------------------------------------------------ 4. solves
def _build_element(pa, dom, how):
    from pynama_amd.petsc import Options
    mat = pa.MatNS()
    mat.setDomain(dom)
    if how == "keyword":
        mat.build(nsType="element")
    else:
        opts = Options()
        opts.setValue("kle_ns_type", "element")
        try:
            mat.build()
        finally:
            opts.delValue("kle_ns_type")
    return mat


@pytest.mark.parametrize("how", ["keyword", "option"])
def test_solvefs_and_solve_match_golden(pa, how):
    """rhsFS = Rw w + Rwfs w + Krhsfs vel against the golden bFS: each of the
    three products lies within its product bound of the exact product, and so
    does the reference's (a sum of the same terms in another order, from
    entries assembled in fp64), so the two differ by at most twice the summed
    bounds plus the two additions' 2 eps (|t1| + |t2| + |t3|) on either side."""
    g = np.load(os.path.join(G, "case_cavity2d.npz"))
    c = _case(pa, "cavity")
    mat = _build_element(pa, c.dom, how)
    assert all(m.getFormat() == "elem" for m in (mat.K, mat.Krhs, mat.Rw, mat.Kfs, mat.Krhsfs, mat.Rwfs,
                                                 mat.getKplusKfs()))
    assert [m.getName() for m in mat.kle] == ["K", "Krhs", "Rw", "Rd", "Kfs", "Krhsfs", "Rwfs", "Rdfs"]
    assert mat.Rd.getInfo()["nz_used"] == 0 and mat.Rdfs.getInfo()["nz_used"] == 0
    sol = pa.KleSolver()
    sol.setMat(mat)
    sol.setUp()
    assert sol.isNS() and sol.solverFS.getOperators()[0] is mat.getKplusKfs()
    sol.getKSP().setTolerances(rtol=1e-13)
    sol.solverFS.setTolerances(rtol=1e-13)
    vort = mat.Rw.createVecRight()
    vort.setArray(g["vort0"])
    vel = sol.getSolution()
    vel0 = np.ascontiguousarray(g["vel0"], np.float64)
    vel.setArray(vel0)
    bfs = sol.rhsFS(vort).getArray()
    w0 = np.ascontiguousarray(g["vort0"], np.float64)
    parts = [np.abs(_ref_mult(c.csr[k], v)).astype(np.float64)
             for k, v in (("Rw", w0), ("Rwfs", w0), ("Krhsfs", vel0))]
    bound = 2 * (c._bound("Rw", w0) + c._bound("Rwfs", w0) + c._bound("Krhsfs", vel0)) + 4 * EPS * sum(parts)
    err = np.abs(bfs - g["bFS"])
    print(f"rhsFS: max err {err.max():.3e}, max err/bound {float(np.max(err / np.where(bound > 0, bound, 1.0))):.3g}")
    nrows = c.rows({N})
    np.testing.assert_array_equal(_bits(bfs[nrows]), _bits(vel0[nrows]))
    assert np.all(err[~nrows] <= bound[~nrows])
    sol.solveFS(vort)
    vfs = sol.getFreeSlipSolution().getArray()
    assert np.linalg.norm(vfs - g["velFS"]) <= 1e-9 * np.linalg.norm(g["velFS"])
    np.testing.assert_array_equal(_bits(vfs[nrows]), _bits(vel0[nrows]))
    sol.solve(vort)
    u = vel.getArray()
    assert np.linalg.norm(u - g["u"]) <= 1e-9 * np.linalg.norm(g["u"])
    wall = c.rows({T, N})
    np.testing.assert_array_equal(_bits(u[wall]), _bits(vel0[wall]))


def _problem(pa, g, nelem):
    from pynama_amd.petsc import Options
    cfg = {"name": "cavity", "material-properties": {"rho": float(g["rho"]), "mu": float(g["mu"])},
           "domain": {"ngl": 3, "box-mesh": {"nelem": nelem, "lower": [0, 0], "upper": [1, 1]}},
           "boundary-conditions": {"no-slip": CAVITY}, "initial-conditions": {"velocity": [0, 0]}}
    opts = Options()
    opts.setValue("kle_ns_type", "element")
    opts.setValue("kle_op_type", "element")
    try:
        prob = pa.BaseProblem(cfg)
        prob.setUp()
        prob.setUpSolver()
    finally:
        opts.delValue("kle_ns_type")
        opts.delValue("kle_op_type")
    # nothing assembled: the seven KLE operators and the three collocation operators
    mat, op = prob.mat, prob.operator
    for m in (mat.K, mat.Krhs, mat.Rw, mat.Kfs, mat.Krhsfs, mat.Rwfs, mat.getKplusKfs(), op.Curl, op.SrT, op.DivSrT):
        assert m.getFormat() == "elem" and m.getInfo()["nz_used"] == 0
    prob.solverKLE.getKSP().setTolerances(rtol=1e-13)
    prob.solverKLE.solverFS.setTolerances(rtol=1e-13)
    return prob


def _check_eval_rhs(prob, g):
    sol = prob.solverKLE
    sol.getSolution().setArray(g["vel0"])
    prob.vort.setArray(g["rhs_vort_in"])
    f = prob.operator.Curl.createVecLeft()
    prob.evalRHS(None, float(g["rhs_t"]), prob.vort, f)
    vfs = sol.getFreeSlipSolution().getArray()
    assert np.linalg.norm(vfs - g["rhs_velFS"]) <= 1e-9 * np.linalg.norm(g["rhs_velFS"])
    np.testing.assert_allclose(prob.vort.getArray(), g["rhs_vort_bc"], rtol=0,
                               atol=1e-9 * np.abs(g["rhs_vort_bc"]).max())
    u = sol.getSolution().getArray()
    assert np.linalg.norm(u - g["rhs_vel"]) <= 1e-9 * np.linalg.norm(g["rhs_vel"])
    scale = max(1.0, np.abs(g["rhs_f"]).max())
    assert np.abs(f.getArray() - g["rhs_f"]).max() <= 1e-6 * scale


def test_eval_rhs_noslip_nothing_assembled(pa):
    g = np.load(os.path.join(G, "case_cavity2d.npz"))
    _check_eval_rhs(_problem(pa, g, [4, 4]), g)


def test_config1_cavity_at_stated_size_nothing_assembled(pa):
    """BASELINE config 1 at its stated size ([50, 50] ngl 3) through BaseProblem
    with -kle_ns_type element -kle_op_type element: the assertions of
    test_gpu_ns.py::test_config1_cavity_at_stated_size_matches_reference
    without the K nnz check (no entry is stored)."""
    g = np.load(os.path.join(G, "case_cavity2d_full.npz"))
    prob = _problem(pa, g, [50, 50])
    dom, sol = prob.dom, prob.solverKLE
    assert sorted(dom.getTangDofs(collect=True)) == sorted(g["tang_dofs"].tolist())
    assert sorted(dom.getNormalDofs(collect=True)) == sorted(g["normal_dofs"].tolist())
    vort = prob.mat.Rw.createVecRight()
    vort.setArray(g["vort0"])
    vel = sol.getSolution()
    vel.setArray(g["vel0"])
    np.testing.assert_allclose(sol.rhsFS(vort).getArray(), g["bFS"], rtol=0, atol=1e-12 * np.abs(g["bFS"]).max())
    sol.solveFS(vort)
    vfs = sol.getFreeSlipSolution().getArray()
    assert np.linalg.norm(vfs - g["velFS"]) <= 1e-9 * np.linalg.norm(g["velFS"])
    sol.solve(vort)
    assert np.linalg.norm(vel.getArray() - g["u"]) <= 1e-9 * np.linalg.norm(g["u"])
    _check_eval_rhs(prob, g)


# --------------------------------------------------------------- 5. refusals
def _refused(fn, code=56):
    from pynama_amd._lib import Error
    with pytest.raises(Error) as ei:
        fn()
    assert ei.value.ierr == code, ei.value


def test_refusals(pa):
    from pynama_amd.petsc import KSP, Mat, Options
    c = _case(pa, "cavity")
    mesh = c.dom.mesh
    # a free-slip box, an unstructured mesh, a 2-rank mesh on a one-rank context
    fs = pa.Domain()
    fs.configure({"domain": {"ngl": 3, "box-mesh": {"nelem": [2, 2], "lower": [0, 0], "upper": [1, 1]}},
                  "boundary-conditions": {"uniform": {"velocity": [1.0, -0.5]}}})
    fs.setUp()
    _refused(lambda: Mat.createNSElement(fs.mesh, "K"))
    from pynama_amd.mesh import UnstructuredMesh
    um = UnstructuredMesh.from_gmsh(os.path.join(G, "test.msh"), 3)
    _refused(lambda: Mat.createNSElement(um, "K"))
    two = pa.BoxMesh(2, [4, 4], [0, 0], [1, 1], 3, rank=0, nranks=2)
    two.set_noslip_faces(list(CAVITY))
    _refused(lambda: Mat.createNSElement(two, "K"))
    # a bad which, a bad nsType by keyword and by option
    _refused(lambda: Mat.createNSElement(mesh, "Rd"), 62)
    _refused(lambda: Mat.createNSElement(mesh, 0), 62)
    ns = pa.MatNS()
    ns.setDomain(c.dom)
    _refused(lambda: ns.build(buildOperators=False, nsType="matrixfree"), 62)
    opts = Options()
    opts.setValue("kle_ns_type", "dense")
    try:
        _refused(lambda: ns.build(buildOperators=False), 62)
    finally:
        opts.delValue("kle_ns_type")
    assert ns.K is None
    # the old switch keeps refusing; the new one is the way in
    _refused(lambda: ns.build(buildOperators=False, kleType="element"))
    # stored-value calls
    A = c.op["K+Kfs"]
    _refused(A.getValuesCSR)
    _refused(A.convert)
    _refused(lambda: A.getRow(0))
    _refused(lambda: A.duplicate(copy=True))
    _refused(A.assemble)
    # the 2-D Rwfs is rectangular
    from pynama_amd._lib import Error
    with pytest.raises(Error):
        KSP().create().setOperators(c.op["Rwfs"])
    # every operator still multiplies within the bound
    for name in OPS:
        x = c.w if name in ("Rw", "Rwfs") else c.x
        _check_product(c, name, c.product(name, x), x, "after refusals")
