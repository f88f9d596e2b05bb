"""The element-wise K and Krhs operators (Mat.createKLEElement, kle_elem.hip)
against the assembled operators of the same mesh.

Reference of every comparison: mat.K.getValuesCSR() / mat.Krhs.getValuesCSR()
multiplied on the host in np.longdouble.  Bound of a product entry i:

    |y_i - ref_i| <= n eps B_i + delta Kmax X_i

n = dim ngl^dim + 8 (the terms of one element row plus the element sums: the
standard bound of a sum in any order), B_i the sum over incident elements of
|K_e0| |x_e| masked as the operator masks (max(B_i, |x_i|) on Dirichlet rows),
Kmax = max |K_e0|, X_i the sum over incident elements of the 1-norm of the
masked x_e, delta the largest |K_e - K_e0| / Kmax over the mesh's elements
(from kle_element_kle), required <= 2e-12."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
G = os.path.join(os.path.dirname(__file__), "golden")

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


class Case:
    """One mesh: assembled and element-wise operators, x, the references and
    the bound's terms, computed once and left unchanged."""

    def __init__(self, pa, dim, nelem, ngl, lower=None, upper=None, faces=None, bc=None):
        from pynama_amd._lib import call
        self.dim, self.ngl = dim, ngl
        cfg = {"domain": {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": lower or [0.0] * dim,
                                                   "upper": upper or [1.0] * dim}},
               "boundary-conditions": bc or {"uniform": {"velocity": [1.0, -0.5, 0.25][:dim]}}}
        self.dom = dom = pa.Domain()
        dom.configure(cfg)
        dom.setUp()
        if faces is not None:
            dom.mesh.set_dirichlet_faces(faces)
        self.mat = mat = pa.MatFS()
        mat.setDomain(dom)
        mat.build(buildOperators=False)
        mesh = dom.mesh
        self.n = n = mesh.N * dim
        self.dir = np.zeros(mesh.N, bool)
        self.dir[mesh.face_nodes(faces if faces is not None else pa.mesh.FACES[dim])] = True
        self.dird = np.repeat(self.dir, dim)
        self.csr = {"K": mat.K.getValuesCSR(), "Krhs": mat.Krhs.getValuesCSR()}
        self.op = {"K": mat.getElementK(), "Krhs": mat.getElementKrhs()}
        # element matrices: K_e0, Kmax, delta
        nd = dim * ngl ** dim
        dw = 1 if dim == 2 else 3
        ctx = pa.get_ctx()
        E = mesh.E
        Ke, Rwe = np.zeros((nd, nd)), np.zeros((nd, dw * ngl ** dim))
        call("kle_element_kle", ctx.h, mesh._h, 0, Ke, Rwe)
        self.K0 = Ke.copy()
        self.Kmax = np.abs(self.K0).max()
        self.delta = 0.0
        for e in range(1, E):
            call("kle_element_kle", ctx.h, mesh._h, e, Ke, Rwe)
            self.delta = max(self.delta, np.abs(Ke - self.K0).max() / self.Kmax)
        conn = mesh.conn()
        self.gd = (conn[:, :, None] * dim + np.arange(dim)[None, None, :]).reshape(E, nd)
        self.x = np.random.default_rng(20240607).uniform(-1, 1, n)

    def ref(self, which, x):
        ip, ix, d = self.csr[which]
        rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
        out = np.zeros(len(ip) - 1, np.longdouble)
        np.add.at(out, rows, d.astype(np.longdouble) * x[ix].astype(np.longdouble))
        return out

    def bound(self, which, x):
        keep = ~self.dird if which == "K" else self.dird
        xe = np.where(keep[self.gd], np.abs(x)[self.gd], 0.0)
        B, X = np.zeros(self.n), np.zeros(self.n)
        np.add.at(B, self.gd, xe @ np.abs(self.K0).T)
        np.add.at(X, self.gd, np.broadcast_to(xe.sum(axis=1)[:, None], xe.shape))
        B = np.where(self.dird, np.maximum(B, np.abs(x)), B)
        nterms = self.dim * self.ngl ** self.dim + 8
        return nterms * EPS * B + self.delta * self.Kmax * X

    def product(self, which, x):
        A = self.op[which]
        xv = A.createVecRight()
        xv.setArray(x)
        return (A * xv).getArray()


@functools.lru_cache(maxsize=None)
def _case_cached(name):
    import pynama_amd
    return Case(pynama_amd, **MESHES[name])


def _case(pa, name):
    return _case_cached(name)


@pytest.mark.parametrize("which", ["K", "Krhs"])
@pytest.mark.parametrize("name", list(MESHES))
def test_product_equals_assembled(pa, name, which):
    c = _case(pa, name)
    assert c.delta <= 2e-12, f"element matrices differ over the mesh: delta = {c.delta:.3e}"
    y = c.product(which, c.x)
    ref = c.ref(which, c.x)
    err = np.abs(y.astype(np.longdouble) - ref).astype(np.float64)
    bnd = c.bound(which, c.x)
    worst = float(np.max(err / np.where(bnd > 0, bnd, 1.0)))
    print(f"{name} {which}: delta {c.delta:.2e}  max err/bound {worst:.3g}  "
          f"rel.norm {np.linalg.norm(err) / max(float(np.linalg.norm(ref.astype(np.float64))), 1e-300):.2e}")
    assert np.all(err <= bnd), (name, which, worst)
    A = c.op[which]
    assert A.getFormat() == "elem"
    assert A.getSize() == (c.n, c.n) and A.getLocalSize() == (c.n, c.n)
    info = A.getInfo()
    assert info["format"] == "elem" and info["nz_used"] == 0 and info["spmv_bytes"] > 0
    assert "k_elem_gemm" in A.spmvKernel() and "k_elem_gather" in A.spmvKernel()


def test_repeatable(pa):
    c = _case(pa, "config2_element")
    for which in ("K", "Krhs"):
        y = c.product(which, c.x)
        for _ in range(3):
            np.testing.assert_array_equal(c.product(which, c.x), y)


def test_masking_is_selection(pa):
    c = _case(pa, "shared_by_8")
    free = ~c.dird
    # K: NaN in every Dirichlet entry
    xn = c.x.copy()
    xn[c.dird] = np.nan
    y0, y1 = c.product("K", c.x), c.product("K", xn)
    np.testing.assert_array_equal(y1[free], y0[free])
    assert np.all(np.isnan(y1[c.dird]))
    # Krhs: NaN in every free entry
    xn = c.x.copy()
    xn[free] = np.nan
    y0, y1 = c.product("Krhs", c.x), c.product("Krhs", xn)
    np.testing.assert_array_equal(y1[free], y0[free])
    np.testing.assert_array_equal(y1[c.dird], c.x[c.dird])


@pytest.mark.parametrize("which", ["K", "Krhs"])
@pytest.mark.parametrize("name", ["config2_element", "2d", "anisotropic"])
def test_mult_add_and_diagonal(pa, name, which):
    c = _case(pa, name)
    A = c.op[which]
    y0 = np.random.default_rng(5).uniform(-1, 1, c.n)
    xv, yv, zv = A.createVecRight(), A.createVecLeft(), A.createVecLeft()
    xv.setArray(c.x)
    yv.setArray(y0)
    A.multAdd(xv, yv, zv)
    z = zv.getArray()
    ref = y0.astype(np.longdouble) + c.ref(which, c.x)
    err = np.abs(z.astype(np.longdouble) - ref).astype(np.float64)
    assert np.all(err <= c.bound(which, c.x) + EPS * np.abs(z))
    # diagonal
    ip, ix, d = c.csr[which]
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    dref = np.zeros(c.n)
    on = ix == rows
    dref[rows[on]] = d[on]
    dsum = np.zeros(c.n)
    np.add.at(dsum, c.gd, np.broadcast_to(np.abs(np.diag(c.K0))[None, :], c.gd.shape))
    dg = A.getDiagonal().getArray()
    assert np.all(np.abs(dg - dref) <= 8 * EPS * dsum + c.delta * c.Kmax * 8)
    assert np.all(dg[c.dird] == 1.0)
    if which == "Krhs":
        assert np.all(dg[~c.dird] == 0.0)


def _host_mult(csr, x):
    ip, ix, d = csr
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    out = np.zeros(len(ip) - 1)
    np.add.at(out, rows, d * x[ix])
    return out


@pytest.mark.parametrize("ksp_type", ["cg", "cg_single_reduction", "gmres"])
@pytest.mark.parametrize("name", ["config2_element", "2d"])
def test_solves(pa, name, ksp_type):
    c = _case(pa, name)
    rtol = 1e-10
    xt = c.mat.K.createVecRight()
    xt.setArray(np.random.default_rng(9).uniform(-1, 1, c.n))
    b = c.mat.K * xt
    its = {}
    for label, A in (("element", c.op["K"]), ("assembled", c.mat.K)):
        ksp = pa.petsc.KSP().create()
        ksp.setType("gmres" if ksp_type == "gmres" else "cg")
        if ksp_type == "cg_single_reduction":
            ksp.setCGSingleReduction(True)
        pc = pa.petsc.PC().create()
        pc.setType("jacobi")
        ksp.setPC(pc)
        ksp.setTolerances(rtol=rtol, atol=0.0, max_it=100000)
        ksp.setOperators(A)
        ksp.setUp()
        u = A.createVecRight()
        ksp.solve(b, u)
        its[label] = ksp.getIterationNumber()
        if label == "element":
            assert ksp.getConvergedReason() > 0, ksp.getConvergedReason()
            bh = b.getArray()
            res = np.linalg.norm(bh - _host_mult(c.csr["K"], u.getArray()))
            assert res <= 2 * rtol * np.linalg.norm(bh), res / np.linalg.norm(bh)
    print(f"{name} {ksp_type}: iterations element {its['element']} assembled {its['assembled']}")


def test_kle_solver_option(pa):
    from pynama_amd.petsc import Options
    bc = {"custom-func": {"name": "taylor_green3d"}}

    def run(element):
        c = Case(pa, 3, [3, 2, 2], 5, bc=bc)
        opts = Options()
        if element:
            opts.setValue("kle_k_type", "element")
        try:
            sol = pa.KleSolver()
            sol.setMat(c.mat)
            sol.setUp()
        finally:
            opts.delValue("kle_k_type")
        return c, sol

    c, sol = run(False)
    assert sol.getKSP().getOperators()[0] is c.mat.K
    assert c.mat.K.getFormat() == "nb" and c.mat.K.spmvKernel() == "k_nb_spmv<3,3,1,true,4>"

    c, sol = run(True)
    assert sol.getKSP().getOperators()[0] is c.mat.getElementK()
    assert sol.getKSP().getOperators()[0].getFormat() == "elem"
    coords = c.dom.getFullCoordArray()
    f = pa.fields.get("taylor_green3d")
    w = f.vorticity(coords, 1.0)
    vort = c.mat.Rw.createVecRight()
    vort.setArray(w)
    vel = sol.getSolution()
    c.dom.applyBoundaryConditions(vel, "velocity", 0.0, 0.02)
    ubc = vel.getArray().copy()
    sol.solve(vort)
    u = vel.getArray()
    assert sol.getKSP().getConvergedReason() > 0
    b = _host_mult(c.mat.Rw.getValuesCSR(), np.asarray(w).ravel()) + _host_mult(c.csr["Krhs"], ubc)
    res = np.linalg.norm(_host_mult(c.csr["K"], u) - b)
    assert res <= 2 * 1e-10 * np.linalg.norm(b), res / np.linalg.norm(b)


def test_refusals(pa):
    Mat = pa.petsc.Mat

    def refused(fn):
        with pytest.raises(pa.Error) as ei:
            fn()
        assert ei.value.ierr == 56, ei.value

    # meshes
    from pynama_amd.mesh import UnstructuredMesh
    um = UnstructuredMesh.from_gmsh(os.path.join(G, "test.msh"), 3)
    refused(lambda: Mat.createKLEElement(um, "K"))
    cav = pa.Domain()
    cav.configure({"domain": {"ngl": 3, "box-mesh": {"nelem": [4, 4], "lower": [0, 0], "upper": [1, 1]}},
                   "boundary-conditions": {"no-slip": {"up": [2, 0], "down": [0, 0], "left": [0, 0],
                                                       "right": [0, 0]}}})
    cav.setUp()
    refused(lambda: Mat.createKLEElement(cav.getMesh(), "K"))
    half = pa.BoxMesh(3, [2, 2, 2], [0, 0, 0], [1, 1, 1], 3, rank=0, nranks=2)
    half.set_dirichlet_faces(pa.mesh.FACES[3])
    refused(lambda: Mat.createKLEElement(half, "Krhs"))
    # calls that need stored values
    c = _case(pa, "shared_by_8")
    A = c.op["K"]
    refused(A.getValuesCSR)
    refused(A.convert)
    refused(lambda: A.setOption(A.Option.SPD, True))
    refused(lambda: A.getRow(0))
    refused(lambda: A.duplicate(copy=True))
    refused(lambda: A.diagonalScale(A.createVecLeft()))
    refused(A.assemble)

    def lu():
        ksp = pa.petsc.KSP().create()
        pc = pa.petsc.PC().create()
        pc.setType("lu")
        ksp.setPC(pc)
        ksp.setOperators(A)
        ksp.setUp()
    refused(lu)
    # ... and the operator still works afterwards
    np.testing.assert_array_equal(c.product("K", c.x), c.product("K", c.x))
