"""The element-wise Rw operator (Mat.createKLEElement(mesh, "Rw"), kle_elem.hip)
and the matrix-free KLE system (MatFS.build(kleType="element"),
-kle_mat_type element) against the assembled matrices of the same mesh.

Reference of every product comparison: mat.Rw.getValuesCSR() multiplied on the
host in np.longdouble.  Bound of a product entry i:

    |y_i - ref_i| <= n eps B_i + delta_R Rmax X_i

n = dim_w ngl^dim + 8 (the terms of one element row plus the element sums: the
standard bound of a sum in any order), B_i the sum over incident elements of
|Rw_e0| |w_e| on free rows (0 on Dirichlet rows, which must be 0.0 exactly),
Rmax = max |Rw_e0|, X_i the sum over incident elements of the 1-norm of w_e,
delta_R the largest |Rw_e - Rw_e0| / Rmax over the mesh's elements (from
kle_element_kle), required <= 2e-12."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
G = os.path.join(os.path.dirname(__file__), "golden")
RTOL = 1e-10

MESHES = {
    "one_element": dict(dim=3, nelem=[1, 1, 1], ngl=3),
    "p1": dict(dim=3, nelem=[2, 1, 1], ngl=2),
    "shared_by_8": dict(dim=3, nelem=[2, 2, 2], ngl=3),
    "whole_tiles": dict(dim=3, nelem=[5, 4, 3], ngl=4),
    "config2_element": dict(dim=3, nelem=[3, 2, 2], ngl=5),
    "config4_element": dict(dim=3, nelem=[2, 1, 1], ngl=7),
    "anisotropic": dict(dim=3, nelem=[5, 2, 3], ngl=4, lower=[-1.5, 0.25, 10.0], upper=[2.0, 0.3, 13.0]),
    "partial_dirichlet": dict(dim=3, nelem=[2, 3, 2], ngl=3, faces=["left", "down"]),
    "2d": dict(dim=2, nelem=[3, 2], ngl=5),
    "2d_one_element": dict(dim=2, nelem=[1, 1], ngl=8),
}


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


def _domain(pa, dim, nelem, ngl, lower=None, upper=None, faces=None, bc=None):
    cfg = {"domain": {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": lower or [0.0] * dim,
                                               "upper": upper or [1.0] * dim}},
           "boundary-conditions": bc or {"uniform": {"velocity": [1.0, -0.5, 0.25][:dim]}}}
    dom = pa.Domain()
    dom.configure(cfg)
    dom.setUp()
    if faces is not None:
        dom.mesh.set_dirichlet_faces(faces)
    return dom


def _host_mult(csr, x):
    ip, ix, d = csr
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    out = np.zeros(len(ip) - 1)
    np.add.at(out, rows, d * x[ix])
    return out


class Case:
    """One mesh: the assembled Rw, the element-wise Rw, w, the reference and
    the bound's terms, computed once and left unchanged."""

    def __init__(self, pa, dim, nelem, ngl, lower=None, upper=None, faces=None):
        from pynama_amd._lib import call
        self.dim, self.ngl = dim, ngl
        self.dw = dw = 1 if dim == 2 else 3
        self.dom = dom = _domain(pa, dim, nelem, ngl, lower, upper, faces)
        self.mat = mat = pa.MatFS()
        mat.setDomain(dom)
        mat.build(buildOperators=False)
        mesh = dom.mesh
        self.n, self.nw = mesh.N * dim, mesh.N * dw
        self.dir = np.zeros(mesh.N, bool)
        self.dir[mesh.face_nodes(faces if faces is not None else pa.mesh.FACES[dim])] = True
        self.dird = np.repeat(self.dir, dim)
        self.csr = mat.Rw.getValuesCSR()
        self.op = mat.getElementRw()
        # element matrices: Rw_e0, Rmax, delta_R
        nn = ngl ** dim
        nd, nc = dim * nn, dw * nn
        ctx = pa.get_ctx()
        E = mesh.E
        Ke, Rwe = np.zeros((nd, nd)), np.zeros((nd, nc))
        call("kle_element_kle", ctx.h, mesh._h, 0, Ke, Rwe)
        self.R0 = Rwe.copy()
        self.Rmax = np.abs(self.R0).max()
        self.delta = 0.0
        for e in range(1, E):
            call("kle_element_kle", ctx.h, mesh._h, e, Ke, Rwe)
            self.delta = max(self.delta, np.abs(Rwe - self.R0).max() / self.Rmax)
        conn = mesh.conn()
        self.gd = (conn[:, :, None] * dim + np.arange(dim)[None, None, :]).reshape(E, nd)
        self.gw = (conn[:, :, None] * dw + np.arange(dw)[None, None, :]).reshape(E, nc)
        self.w = np.random.default_rng(20240607).uniform(-1, 1, self.nw)
        # reference and bound of Rw w
        ip, ix, d = self.csr
        rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
        self.ref = np.zeros(len(ip) - 1, np.longdouble)
        np.add.at(self.ref, rows, d.astype(np.longdouble) * self.w[ix].astype(np.longdouble))
        we = np.abs(self.w)[self.gw]
        B, X = np.zeros(self.n), np.zeros(self.n)
        np.add.at(B, self.gd, we @ np.abs(self.R0).T)
        np.add.at(X, self.gd, np.broadcast_to(we.sum(axis=1)[:, None], self.gd.shape))
        B = np.where(self.dird, 0.0, B)
        self.bound = (dw * nn + 8) * EPS * B + self.delta * self.Rmax * X

    def product(self, w):
        xv = self.op.createVecRight()
        xv.setArray(w)
        return (self.op * xv).getArray()


@functools.lru_cache(maxsize=None)
def _case_cached(name):
    import pynama_amd
    return Case(pynama_amd, **MESHES[name])


def _case(pa, name):
    return _case_cached(name)


# ------------------------------------------------------------ 1. the product
@pytest.mark.parametrize("name", list(MESHES))
def test_rw_product_equals_assembled(pa, name):
    c = _case(pa, name)
    assert c.delta <= 2e-12, f"element matrices differ over the mesh: delta_R = {c.delta:.3e}"
    A = c.op
    assert c.csr[0].shape == (c.n + 1,)
    assert A.getFormat() == "elem"
    assert A.getSize() == (c.n, c.nw) and A.getLocalSize() == (c.n, c.nw)
    assert A.createVecRight().getLocalSize() == c.nw and A.createVecLeft().getLocalSize() == c.n
    info = A.getInfo()
    assert info["format"] == "elem" and info["nz_used"] == 0 and info["spmv_bytes"] > 0
    assert "k_elem_gemm" in A.spmvKernel()
    y = c.product(c.w)
    err = np.abs(y.astype(np.longdouble) - c.ref).astype(np.float64)
    worst = float(np.max(err / np.where(c.bound > 0, c.bound, 1.0)))
    print(f"{name} Rw: delta_R {c.delta:.2e}  max err/bound {worst:.3g}  "
          f"rel.norm {np.linalg.norm(err) / max(float(np.linalg.norm(c.ref.astype(np.float64))), 1e-300):.2e}")
    assert np.all(err <= c.bound), (name, worst)
    # Dirichlet rows hold no entry
    assert np.all(y[c.dird] == 0.0)
    assert not np.any(np.signbit(y[c.dird]))
    if name != "p1":
        assert np.any(y[~c.dird] != 0.0)


# ------------------------------------ 2. repeatability, row selection, multAdd
def test_rw_repeatable(pa):
    c = _case(pa, "config2_element")
    y = c.product(c.w)
    for _ in range(3):
        np.testing.assert_array_equal(c.product(c.w), y)


@pytest.mark.parametrize("name", ["shared_by_8", "2d", "p1"])
def test_rw_rows_are_selected(pa, name):
    c = _case(pa, name)
    y = c.product(np.full(c.nw, np.nan))
    np.testing.assert_array_equal(y[c.dird], np.zeros(int(c.dird.sum())))
    assert np.all(np.isnan(y[~c.dird]))


@pytest.mark.parametrize("name", ["config2_element", "2d", "anisotropic"])
def test_rw_mult_add(pa, name):
    c = _case(pa, name)
    A = c.op
    y0 = np.random.default_rng(5).uniform(-1, 1, c.n)
    xv, yv, zv = A.createVecRight(), A.createVecLeft(), A.createVecLeft()
    xv.setArray(c.w)
    yv.setArray(y0)
    A.multAdd(xv, yv, zv)
    z = zv.getArray()
    ref = y0.astype(np.longdouble) + c.ref
    err = np.abs(z.astype(np.longdouble) - ref).astype(np.float64)
    assert np.all(err <= c.bound + EPS * np.abs(z))


# ------------------------------------------------------ 3. matrix-free build
BUILD_CASES = {
    "3d": dict(dim=3, nelem=[3, 2, 2], ngl=5, bc={"custom-func": {"name": "taylor_green3d"}}),
    "2d": dict(dim=2, nelem=[3, 2], ngl=5),
}


class Solved:
    """One matrix-free build and KleSolver.solve, and the assembled MatFS of
    the same domain that the host checks go through; made once per case."""

    def __init__(self, pa, name, how):
        from pynama_amd.petsc import Options
        spec = BUILD_CASES[name]
        self.dim = dim = spec["dim"]
        self.dom = dom = _domain(pa, **spec)
        self.mat = mat = pa.MatFS()
        mat.setDomain(dom)
        if how == "keyword":
            mat.build(buildOperators=False, kleType="element")
        else:
            opts = Options()
            opts.setValue("kle_mat_type", "element")
            try:
                mat.build(buildOperators=False)
            finally:
                opts.delValue("kle_mat_type")
        self.sol = sol = pa.KleSolver()
        sol.setMat(mat)
        sol.setUp()
        N = dom.mesh.N
        if name == "3d":
            w = pa.fields.get("taylor_green3d").vorticity(dom.getFullCoordArray(), 1.0)
            self.w = np.asarray(w, np.float64).ravel()
        else:
            self.w = np.random.default_rng(11).uniform(-1, 1, N)
        # a second, assembled MatFS of the same domain
        self.ref = ref = pa.MatFS()
        ref.setDomain(dom)
        ref.build(buildOperators=False, kleType="assembled")
        self.u, self.ubc = self._solve(sol, mat)
        self.reason, self.its = sol.getKSP().getConvergedReason(), sol.getKSP().getIterationNumber()
        dird = np.zeros(N, bool)
        dird[dom.mesh.face_nodes(pa.mesh.FACES[dim])] = True
        self.dird = np.repeat(dird, dim)

    def _solve(self, sol, mat):
        vort = mat.Rw.createVecRight()
        vort.setArray(self.w)
        vel = sol.getSolution()
        self.dom.applyBoundaryConditions(vel, "velocity", 0.0, 0.02)
        ubc = vel.getArray().copy()
        sol.solve(vort)
        return vel.getArray().copy(), ubc


@functools.lru_cache(maxsize=None)
def _solved_cached(name, how):
    import pynama_amd
    return Solved(pynama_amd, name, how)


@pytest.mark.parametrize("how", ["keyword", "option"])
@pytest.mark.parametrize("name", list(BUILD_CASES))
def test_matrix_free_build_and_solve(pa, name, how):
    s = _solved_cached(name, how)
    mat, sol, ref = s.mat, s.sol, s.ref
    for A, nm in ((mat.K, "K"), (mat.Krhs, "Krhs"), (mat.Rw, "Rw")):
        assert A.getFormat() == "elem" and A.getInfo()["nz_used"] == 0, nm
        assert A.getName() == nm
    assert mat.getElementK() is mat.K and mat.getElementKrhs() is mat.Krhs and mat.getElementRw() is mat.Rw
    assert len(mat.kle) == 4 and mat.kle[0] is mat.K and mat.kle[1] is mat.Krhs and mat.kle[2] is mat.Rw
    assert mat.kle[3] is mat.Rd and mat.Rd.getInfo()["nz_used"] == 0
    assert sol.getKSP().getOperators()[0] is mat.K
    assert s.reason > 0, s.reason
    # b and the residual on the host through the assembled matrices
    assert ref.K.getFormat() == "nb" and ref.Rw.getFormat() == "nb"
    b = _host_mult(ref.Rw.getValuesCSR(), s.w) + _host_mult(ref.Krhs.getValuesCSR(), s.ubc)
    res = np.linalg.norm(_host_mult(ref.K.getValuesCSR(), s.u) - b)
    print(f"{name} {how}: iterations {s.its}  true residual {res / np.linalg.norm(b):.3e}")
    assert res <= 2 * RTOL * np.linalg.norm(b), res / np.linalg.norm(b)


@pytest.mark.parametrize("how", ["keyword", "option"])
@pytest.mark.parametrize("name", list(BUILD_CASES))
def test_matrix_free_dirichlet_entries_are_u_bc(pa, name, how):
    """Dirichlet entries of u equal u_bc bit for bit: after a matrix-free
    solve KleSolver copies them back (Mat.copyDirichletRows; the unit Dirichlet
    rows make u = b = u_bc there).  The Krylov iterate alone, started from 0,
    holds them to rtol only, as the assembled solve of the same domain shows
    (printed: largest |u - u_bc| / |u_bc| over the Dirichlet entries; measured
    1.111e-10 on [3,2,2] ngl 5 Taylor-Green, 9.989e-12 on the 2-D mesh, and
    1.085e-10 / 2.133e-11 matrix-free before the copy)."""
    s = _solved_cached(name, how)
    d = s.dird
    assert np.any(s.ubc[d] != 0.0)

    def worst(u, ubc):
        nz = d & (ubc != 0.0)
        return float(np.max(np.abs(u[nz] - ubc[nz]) / np.abs(ubc[nz])))

    asm = pa.KleSolver()
    asm.setMat(s.ref)
    asm.setUp()
    ua, ubca = s._solve(asm, s.ref)
    print(f"{name} {how}: Dirichlet entries, largest relative difference to u_bc: matrix-free "
          f"{worst(s.u, s.ubc):.3e}  assembled {worst(ua, ubca):.3e}")
    np.testing.assert_array_equal(s.u[d], s.ubc[d])
    assert s.u[d].tobytes() == s.ubc[d].tobytes()
    # the copy touches the Dirichlet rows only, and only of an element-wise operator
    K = s.mat.K
    src, dst = K.createVecLeft(), K.createVecLeft()
    src.setArray(np.full(len(d), 7.0))
    dst.setArray(np.arange(len(d), dtype=np.float64))
    K.copyDirichletRows(src, dst)
    np.testing.assert_array_equal(dst.getArray(), np.where(d, 7.0, np.arange(len(d), dtype=np.float64)))
    _refused(pa, lambda: s.ref.K.copyDirichletRows(src, dst))


# ------------------------------------------------------------------ 4. options
def test_k_type_element_uses_element_rw(pa):
    from pynama_amd.petsc import Options
    dom = _domain(pa, 3, [3, 2, 2], 5, bc={"custom-func": {"name": "taylor_green3d"}})
    mat = pa.MatFS()
    mat.setDomain(dom)
    mat.build(buildOperators=False)
    assert mat.Rw.getFormat() == "nb"
    opts = Options()
    opts.setValue("kle_k_type", "element")
    try:
        sol = pa.KleSolver()
        sol.setMat(mat)
        sol.setUp()
    finally:
        opts.delValue("kle_k_type")
    w = np.asarray(pa.fields.get("taylor_green3d").vorticity(dom.getFullCoordArray(), 1.0), np.float64).ravel()
    vort = mat.Rw.createVecRight()
    vort.setArray(w)
    vel = sol.getSolution()
    dom.applyBoundaryConditions(vel, "velocity", 0.0, 0.02)
    b = sol.rhs(vort).getArray().copy()
    Rw, Krhs = mat.getElementRw(), mat.getElementKrhs()
    assert Rw.getFormat() == "elem" and Rw is not mat.Rw
    expect = (Rw * vort).getArray() + (Krhs * vel).getArray()
    assert np.any(b != 0.0)
    np.testing.assert_array_equal(b, expect)


def test_problem_under_mat_type_element(pa):
    from pynama_amd.petsc import Options
    cfg = {"name": "tg", "material-properties": {"rho": 0.5, "mu": 0.01},
           "domain": {"ngl": 3, "box-mesh": {"nelem": [2, 2, 2], "lower": [0, 0, 0], "upper": [1, 1, 1]}},
           "boundary-conditions": {"custom-func": {"name": "taylor_green3d"}},
           "initial-conditions": {"custom-func": {"name": "taylor_green3d"}},
           "time-solver": {"start-time": 0.0, "end-time": 0.1, "max-steps": 2}}
    opts = Options()
    opts.setValue("kle_mat_type", "element")
    try:
        prob = pa.BaseProblem(cfg)
        prob.setUp()
        prob.setUpSolver()
    finally:
        opts.delValue("kle_mat_type")
    assert prob.mat.K.getFormat() == "elem"
    assert prob.mat.Krhs.getFormat() == "elem" and prob.mat.Rw.getFormat() == "elem"
    assert prob.solverKLE.getKSP().getOperators()[0] is prob.mat.K
    # the operators stay assembled
    assert prob.operator.Curl.getFormat() != "elem"


# ---------------------------------------------------------------- 5. refusals
def _refused(pa, fn, ierr=56):
    with pytest.raises(pa.Error) as ei:
        fn()
    assert ei.value.ierr == ierr, ei.value


def test_rw_refused_meshes(pa):
    Mat = pa.petsc.Mat
    from pynama_amd.mesh import UnstructuredMesh
    um = UnstructuredMesh.from_gmsh(os.path.join(G, "test.msh"), 3)
    _refused(pa, lambda: Mat.createKLEElement(um, "Rw"))
    cav = pa.Domain()
    cav.configure({"domain": {"ngl": 3, "box-mesh": {"nelem": [4, 4], "lower": [0, 0], "upper": [1, 1]}},
                   "boundary-conditions": {"no-slip": {"up": [2, 0], "down": [0, 0], "left": [0, 0],
                                                       "right": [0, 0]}}})
    cav.setUp()
    _refused(pa, lambda: Mat.createKLEElement(cav.getMesh(), "Rw"))
    half = pa.BoxMesh(3, [2, 2, 2], [0, 0, 0], [1, 1, 1], 3, rank=0, nranks=2)
    half.set_dirichlet_faces(pa.mesh.FACES[3])
    _refused(pa, lambda: Mat.createKLEElement(half, "Rw"))
    c = _case(pa, "shared_by_8")
    _refused(pa, lambda: Mat.createKLEElement(c.dom.mesh, "Rd"), 62)


@pytest.mark.parametrize("name", ["shared_by_8", "2d"])
def test_rw_refused_calls(pa, name):
    c = _case(pa, name)
    A = c.op
    _refused(pa, A.getDiagonal)
    _refused(pa, A.getValuesCSR)
    _refused(pa, A.convert)
    _refused(pa, lambda: A.getRow(0))
    _refused(pa, lambda: A.duplicate(copy=True))
    _refused(pa, A.assemble)
    # ... and the operator still multiplies correctly afterwards
    err = np.abs(c.product(c.w).astype(np.longdouble) - c.ref).astype(np.float64)
    assert np.all(err <= c.bound)


def test_ksp_refuses_rw(pa):
    c = _case(pa, "2d")
    A = c.op

    def solve():
        ksp = pa.petsc.KSP().create()
        ksp.setType("cg")
        pc = pa.petsc.PC().create()
        pc.setType("jacobi")
        ksp.setPC(pc)
        ksp.setOperators(A)
        ksp.setUp()
    with pytest.raises(pa.Error):
        solve()
    err = np.abs(c.product(c.w).astype(np.longdouble) - c.ref).astype(np.float64)
    assert np.all(err <= c.bound)


def test_mat_type_refusals(pa):
    from pynama_amd.petsc import Options
    opts = Options()
    cav = pa.Domain()
    cav.configure({"domain": {"ngl": 3, "box-mesh": {"nelem": [4, 4], "lower": [0, 0], "upper": [1, 1]}},
                   "boundary-conditions": {"no-slip": {"up": [2, 0], "down": [0, 0], "left": [0, 0],
                                                       "right": [0, 0]}}})
    cav.setUp()
    ns = pa.MatNS()
    ns.setDomain(cav)
    opts.setValue("kle_mat_type", "element")
    try:
        _refused(pa, ns.build)
    finally:
        opts.delValue("kle_mat_type")
    _refused(pa, lambda: ns.build(kleType="element"))
    # a bad value, by option and by keyword
    dom = _domain(pa, 3, [1, 1, 1], 3)
    mat = pa.MatFS()
    mat.setDomain(dom)
    opts.setValue("kle_mat_type", "matrixfree")
    try:
        _refused(pa, lambda: mat.build(buildOperators=False), 62)
    finally:
        opts.delValue("kle_mat_type")
    _refused(pa, lambda: mat.build(buildOperators=False, kleType="dense"), 62)
    assert mat.K is None
    # unstructured meshes have no matrix-free build
    gm = pa.Domain()
    gm.configure({"domain": {"ngl": 3, "gmsh-file": os.path.join(G, "test.msh")},
                  "boundary-conditions": {"custom-func": {"name": "taylor_green"}}})
    gm.setUp()
    mf = pa.MatFS()
    mf.setDomain(gm)
    _refused(pa, lambda: mf.build(buildOperators=False, kleType="element"))
