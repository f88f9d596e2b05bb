"""The element-wise collocation operators Curl, SrT and DivSrT
(Mat.createOperatorElement, Operators.build(opType="element"), -kle_op_type
element; kle_colloc.hip) against the assembled operators of the same mesh.

Reference of every product comparison: the assembled operator's
getValuesCSR() multiplied on the host in np.longdouble.  Bound of a product
entry i (row component of node g, which is local node l of its elements e):

    |y_i - ref_i| <= n eps B_i + delta Mmax X_i winv_g + 2 delta_w B_i

n = CW (dim (ngl - 1) + 1) + 2^dim + 8 (the terms of one factored element row
over the CW column components, the element sums and the scalings),
B_i = winv_g sum_{e containing g} (|M_e0| |x_e|)_l, X_i = sum_e ||x_e||_1,
Mmax = max |M_e0|, delta = max_e max |M_e - M_e0| / Mmax,
delta_w = max_e max |c_e - c_0| / max c_0, with the element matrices and
weights from the oracle's Element.ops on the device mesh's own corners.
delta, delta_w <= 2e-12 is required of the inputs.

Largest error / bound measured per case on an MI355X: see DESIGN section 3
("Element-wise Curl, SrT and DivSrT")."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
G = os.path.join(os.path.dirname(__file__), "golden")
OPS = ("Curl", "SrT", "DivSrT")
CAVITY_BC = {"no-slip": {"up": [2, 0], "down": [0, 0], "left": [0, 0], "right": [0, 0]}}

MESHES = {
    "one_element": dict(dim=3, nelem=[1, 1, 1], ngl=3),
    "line_of_2": dict(dim=3, nelem=[2, 1, 1], ngl=2),
    "shared_by_8": dict(dim=3, nelem=[2, 2, 2], ngl=3),
    "partial_batch": dict(dim=3, nelem=[5, 4, 3], ngl=4),
    "config2_element": dict(dim=3, nelem=[3, 2, 2], ngl=5),
    "config4_element": dict(dim=3, nelem=[2, 1, 1], ngl=7),
    "largest_line": dict(dim=3, nelem=[1, 2, 1], ngl=8),
    "anisotropic": dict(dim=3, nelem=[5, 2, 3], ngl=4, lower=[-1.5, 0.25, 10.0], upper=[2.0, 0.3, 13.0]),
    "2d": dict(dim=2, nelem=[3, 2], ngl=5),
    "2d_largest_line": dict(dim=2, nelem=[1, 1], ngl=8),
    "2d_offset": dict(dim=2, nelem=[4, 3], ngl=6, lower=[-2.0, 100.0], upper=[1.0, 100.3]),
    "cavity": dict(dim=2, nelem=[4, 4], ngl=3, bc=CAVITY_BC),
}


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


def _domain(pa, dim, nelem, ngl, lower=None, upper=None, bc=None):
    cfg = {"domain": {"ngl": ngl, "box-mesh": {"nelem": list(nelem), "lower": lower or [0.0] * dim,
                                               "upper": upper or [1.0] * dim}},
           "boundary-conditions": bc or {"custom-func": {"name": "taylor_green3d" if dim == 3 else "taylor_green"}}}
    dom = pa.Domain()
    dom.configure(cfg)
    dom.setUp()
    return dom


def _shape(dim, nm):
    dw, ds = (1, 3) if dim == 2 else (3, 6)
    return {"Curl": (dw, dim), "SrT": (ds, dim), "DivSrT": (dim, ds)}[nm]


def _long_mult(csr, x):
    ip, ix, d = csr
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    out = np.zeros(len(ip) - 1, np.longdouble)
    np.add.at(out, rows, d.astype(np.longdouble) * x[ix].astype(np.longdouble))
    return out


class Case:
    """One mesh: the assembled and the element-wise operators, x, the
    reference products and the bound's terms, computed once and left
    unchanged."""

    def __init__(self, pa, dim, nelem, ngl, lower=None, upper=None, bc=None):
        self.dim, self.ngl = dim, ngl
        lower, upper = lower or [0.0] * dim, upper or [1.0] * dim
        self.dom = dom = _domain(pa, dim, nelem, ngl, lower, upper, bc)
        ns = bc is not None
        asm = (pa.MatNS if ns else pa.MatFS)()
        asm.setDomain(dom)
        asm.build(buildKLE=False)
        self.asm = asm.getOperators()
        self.mat = mat = (pa.MatNS if ns else pa.MatFS)()
        mat.setDomain(dom)
        if ns:
            mat.build(opType="element")  # the no-slip KLE matrices are assembled beside them
        else:
            mat.build(buildKLE=False, opType="element")
        self.elem = mat.getOperators()
        mesh = dom.mesh
        self.N, self.E = N, E = mesh.N, mesh.E
        nn = ngl ** dim
        conn = mesh.conn()
        self.conn = conn
        # oracle element matrices on the device mesh's corners, in libkle's tensor order
        el = O.Element(ngl, dim)
        om = O.BoxMesh(dim, nelem, lower, upper, ngl)
        ref0 = om.conn()[0]
        perm = np.array([np.where(conn[0] == c)[0][0] for c in ref0])
        corners = mesh.corners()

        def ops(e):
            SrT, Div, Curl, W = el.ops(corners[e].ravel())
            out = {}
            for nm, M in (("Curl", Curl), ("SrT", SrT), ("DivSrT", Div)):
                R, C = _shape(dim, nm)
                pr = (perm[:, None] * R + np.arange(R)[None, :]).ravel()
                pc = (perm[:, None] * C + np.arange(C)[None, :]).ravel()
                T = np.zeros_like(M)
                T[np.ix_(pr, pc)] = M
                out[nm] = T
            c = np.zeros(nn)
            c[perm] = W
            return out, c

        # (the oracle's element call takes seconds at ngl 8 and reads its
        # element tables only: the elements go through a few threads)
        with ThreadPoolExecutor(max_workers=8) as pool:
            every = list(pool.map(ops, range(E)))
        M0, c0 = every[0]
        self.M0 = M0
        self.delta = {nm: 0.0 for nm in OPS}
        self.delta_w = 0.0
        for Me, ce in every[1:]:
            for nm in OPS:
                self.delta[nm] = max(self.delta[nm], np.abs(Me[nm] - M0[nm]).max() / np.abs(M0[nm]).max())
            self.delta_w = max(self.delta_w, np.abs(ce - c0).max() / np.abs(c0).max())
        W = np.zeros(N)
        np.add.at(W, conn, np.broadcast_to(c0[None, :], conn.shape))
        self.winv = 1.0 / W
        rng = np.random.default_rng(20240611)
        self.x, self.csr, self.ref, self.bound = {}, {}, {}, {}
        for nm in OPS:
            R, C = _shape(dim, nm)
            x = rng.uniform(-1, 1, N * C)
            gr = (conn[:, :, None] * R + np.arange(R)[None, None, :]).reshape(E, nn * R)
            gc = (conn[:, :, None] * C + np.arange(C)[None, None, :]).reshape(E, nn * C)
            xe = np.abs(x)[gc]
            B, X = np.zeros(N * R), np.zeros(N * R)
            np.add.at(B, gr, xe @ np.abs(M0[nm]).T)
            np.add.at(X, gr, np.broadcast_to(xe.sum(axis=1)[:, None], gr.shape))
            wi = np.repeat(self.winv, R)
            B *= wi
            n = C * (dim * (ngl - 1) + 1) + 2 ** dim + 8
            self.bound[nm] = (n * EPS * B + self.delta[nm] * np.abs(M0[nm]).max() * X * wi
                              + 2 * self.delta_w * B)
            self.x[nm] = x
            self.csr[nm] = getattr(self.asm, nm).getValuesCSR()
            self.ref[nm] = _long_mult(self.csr[nm], x)

    def product(self, nm, x):
        A = getattr(self.elem, nm)
        xv = A.createVecRight()
        xv.setArray(x)
        return (A * xv).getArray()

    def within_bound(self, nm):
        err = np.abs(self.product(nm, self.x[nm]).astype(np.longdouble) - self.ref[nm]).astype(np.float64)
        return err, bool(np.all(err <= self.bound[nm]))


@functools.lru_cache(maxsize=None)
def _case_cached(name):
    import pynama_amd
    return Case(pynama_amd, **MESHES[name])


def _case(pa, name):
    return _case_cached(name)


def _refused(pa, fn, ierr=56):
    with pytest.raises(pa.Error) as ei:
        fn()
    assert ei.value.ierr == ierr, ei.value


# ------------------------------------------------------------ 1. the product
@pytest.mark.parametrize("name", list(MESHES))
def test_product_equals_assembled(pa, name):
    c = _case(pa, name)
    assert c.delta_w <= 2e-12, f"element weights differ over the mesh: delta_w = {c.delta_w:.3e}"
    for nm in OPS:
        assert c.delta[nm] <= 2e-12, f"{nm}: element matrices differ over the mesh: delta = {c.delta[nm]:.3e}"
        R, C = _shape(c.dim, nm)
        A = getattr(c.elem, nm)
        assert getattr(c.asm, nm).getFormat() != "elem"
        assert A.getFormat() == "elem" and A.getName() == nm
        assert A.getSize() == (c.N * R, c.N * C) and A.getLocalSize() == (c.N * R, c.N * C)
        assert A.getOwnershipRange() == (0, c.N * R)
        assert A.createVecRight().getLocalSize() == c.N * C and A.createVecLeft().getLocalSize() == c.N * R
        info = A.getInfo()
        assert info["format"] == "elem" and info["nz_used"] == 0 and info["spmv_bytes"] > 0
        assert "k_colloc_elem" in A.spmvKernel() and "k_colloc_gather" in A.spmvKernel()
        err, ok = c.within_bound(nm)
        b = c.bound[nm]
        worst = float(np.max(err / np.where(b > 0, b, 1.0)))
        print(f"{name} {nm}: delta {c.delta[nm]:.2e}  delta_w {c.delta_w:.2e}  max err/bound {worst:.3g}  "
              f"rel.norm {np.linalg.norm(err) / max(float(np.linalg.norm(c.ref[nm].astype(np.float64))), 1e-300):.2e}")
        assert ok, (name, nm, worst)
        assert np.any(c.product(nm, c.x[nm]) != 0.0)


@pytest.mark.parametrize("name", ["anisotropic", "2d"])
def test_element_ops_export_matches_oracle(pa, name):
    """kle_element_ops (the element matrices of the assembly path, which the
    creation check compares the factored tables with) against the oracle's:
    1e-12 of the largest entry, as the assembled values are held to; entries
    off the grid lines exactly 0."""
    from pynama_amd._lib import call
    c = _case(pa, name)
    mesh, dim, ngl = c.dom.mesh, c.dim, c.ngl
    nn = ngl ** dim
    out = {nm: np.zeros((nn * _shape(dim, nm)[0], nn * _shape(dim, nm)[1])) for nm in OPS}
    w = np.zeros(nn)
    call("kle_element_ops", pa.get_ctx().h, mesh._h, 0, out["Curl"], out["SrT"], out["DivSrT"], w)
    l = np.arange(nn)
    idx = np.stack([(l // ngl ** d) % ngl for d in range(dim)], 1)
    on_line = (idx[:, None, :] != idx[None, :, :]).sum(axis=2) <= 1
    for nm in OPS:
        R, C = _shape(dim, nm)
        ref = c.M0[nm]
        assert np.abs(out[nm] - ref).max() <= 1e-12 * np.abs(ref).max(), nm
        off = ~np.repeat(np.repeat(on_line, R, axis=0), C, axis=1)
        assert np.all(out[nm][off] == 0.0), nm
        assert np.count_nonzero(on_line[0]) == dim * (ngl - 1) + 1


# ---------------------------------------------------------------- 2. golden
@pytest.mark.parametrize("case", ["uniform2d", "tg2d_small", "tg3d", "cavity2d"])
def test_element_operators_match_golden(pa, case):
    g = np.load(os.path.join(G, f"case_{case}.npz"))
    dim = int(g["dim"])
    dom = _domain(pa, dim, list(g["nelem"]), int(g["ngl"]), list(g["lower"]), list(g["upper"]))
    mat = pa.MatFS()
    mat.setDomain(dom)
    mat.build(buildKLE=False, opType="element")
    op = mat.getOperators()
    rng = np.random.default_rng(5)
    for nm in OPS:
        A = getattr(op, nm)
        assert A.getFormat() == "elem"
        R = O.CSR.from_arrays(g[nm + "_indptr"], g[nm + "_indices"], g[nm + "_data"], int(g[nm + "_shape"][1]))
        x = A.createVecRight()
        xa = rng.uniform(-1, 1, x.getLocalSize())
        x.setArray(xa)
        y = (A * x).getArray()
        yr = R.mult(xa)
        print(f"{case} {nm}: {np.linalg.norm(y - yr) / np.linalg.norm(yr):.3e}")
        assert np.linalg.norm(y - yr) <= 1e-13 * np.linalg.norm(yr), nm


# ------------------------------------------------- 3. polynomial identities
def test_element_operator_polynomial_identities(pa):
    """Degree-<=p fields: Curl u, SrT u and DivSrT s are exact at the nodes."""
    dim, nelem, ngl = 3, [6, 5, 4], 5
    dom = _domain(pa, dim, nelem, ngl)
    mat = pa.MatFS()
    mat.setDomain(dom)
    mat.build(buildKLE=False, opType="element")
    op = mat.getOperators()
    assert op.Curl.getFormat() == "elem"
    X = dom.getFullCoordArray().reshape(-1, 3)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    u = np.stack([y * y * z, x * z * z, x * y * x], 1)          # degree <= 3
    curl = np.stack([x * x - 2 * x * z, y * y - 2 * x * y, z * z - 2 * y * z], 1)
    # grad[i][j] = d u_i / d x_j; strain rate 0.5 (grad u + grad u^T): xx, xy, yy, yz, zz, zx
    gr = [[0 * x, 2 * y * z, y * y], [z * z, 0 * x, 2 * x * z], [2 * x * y, x * x, 0 * x]]
    S = np.stack([gr[0][0], 0.5 * (gr[0][1] + gr[1][0]), gr[1][1], 0.5 * (gr[1][2] + gr[2][1]), gr[2][2],
                  0.5 * (gr[2][0] + gr[0][2])], 1)
    v = op.Curl.createVecRight()
    v.setArray(u.ravel())
    w = (op.Curl * v).getArray().reshape(-1, 3)
    assert np.abs(w - curl).max() <= 1e-9 * np.abs(curl).max()
    s = (op.SrT * v).getArray().reshape(-1, 6)
    assert np.abs(s - S).max() <= 1e-9 * np.abs(S).max()
    # div of a polynomial symmetric tensor: sigma = (x^2, xy, y^2, yz, z^2, zx)
    sig = np.stack([x * x, x * y, y * y, y * z, z * z, z * x], 1)
    divs = np.stack([2 * x + x + x, y + 2 * y + y, z + 2 * z + z], 1)  # d_j sigma_ij
    sv = op.DivSrT.createVecRight()
    sv.setArray(sig.ravel())
    d = (op.DivSrT * sv).getArray().reshape(-1, 3)
    assert np.abs(d - divs).max() <= 1e-9 * np.abs(divs).max()


# ---------------------------------------------------------------- 4. evalRHS
def _problem(pa, g, case):
    dim = int(g["dim"])
    bc = ({"uniform": {"velocity": [4, 0]}} if case == "uniform2d" else
          {"custom-func": {"name": "taylor_green3d" if dim == 3 else "taylor_green"}})
    cfg = {"name": case, "material-properties": {"rho": float(g["rho"]), "mu": float(g["mu"])},
           "domain": {"ngl": int(g["ngl"]), "box-mesh": {"nelem": [int(v) for v in g["nelem"]],
                                                        "lower": list(g["lower"]), "upper": list(g["upper"])}},
           "boundary-conditions": bc, "initial-conditions": {"velocity": [4, 0]} if case == "uniform2d" else bc}
    prob = pa.BaseProblem(cfg)
    prob.setUp()
    prob.setUpSolver()
    return prob


@pytest.mark.parametrize("both", [False, True], ids=["op_element", "mat_and_op_element"])
@pytest.mark.parametrize("case", ["uniform2d", "tg2d_small", "tg3d"])
def test_eval_rhs_with_element_operators(pa, case, both):
    from pynama_amd.petsc import Options
    g = np.load(os.path.join(G, f"case_{case}.npz"))
    opts = Options()
    opts.setValue("kle_op_type", "element")
    if both:
        opts.setValue("kle_mat_type", "element")
    try:
        prob = _problem(pa, g, case)
    finally:
        opts.delValue("kle_op_type")
        if both:
            opts.delValue("kle_mat_type")
    for nm in OPS:
        assert getattr(prob.operator, nm).getFormat() == "elem", nm
    assert prob.mat.K.getFormat() == ("elem" if both else "nb")
    scale = max(1.0, np.abs(g["rhs_f"]).max())
    # (1) the operator chain from the reference's KLE velocity
    vel = prob.solverKLE.getSolution().duplicate()
    vel.setArray(g["rhs_vel"])
    prob.computeVtensV(vel)
    np.testing.assert_array_equal(prob._VtensV.getArray(), g["rhs_VtensV"])
    prob.operator.SrT.mult(vel, prob._Aux1)
    prob._Aux1 *= (2.0 * prob.mu)
    prob._Aux1.axpy(-1.0 * prob.rho, prob._VtensV)
    e1 = np.abs(prob._Aux1.getArray() - g["rhs_Aux1"]).max() / max(1.0, np.abs(g["rhs_Aux1"]).max())
    rhs = vel.duplicate()
    prob.operator.DivSrT.mult(prob._Aux1, rhs)
    rhs.scale(1 / prob.rho)
    f = prob.operator.Curl.createVecLeft()
    prob.operator.Curl.mult(rhs, f)
    e2 = np.abs(f.getArray() - g["rhs_f"]).max() / scale
    # (2) the full call
    prob.solverKLE.getKSP().setTolerances(rtol=1e-13)
    prob.vort.setArray(g["rhs_vort_in"])
    f2 = prob.operator.Curl.createVecLeft()
    prob.evalRHS(None, float(g["rhs_t"]), prob.vort, f2)
    e3 = np.abs(f2.getArray() - g["rhs_f"]).max() / scale
    print(f"{case} both={both}: Aux1 {e1:.3e}  f {e2:.3e}  full call {e3:.3e}")
    assert e1 <= 1e-12
    assert e2 <= 1e-10
    assert e3 <= 1e-6


# ------------------------------------------- 5. repeatability and multAdd
@pytest.mark.parametrize("name", ["config2_element", "2d"])
def test_products_are_repeatable(pa, name):
    c = _case(pa, name)
    for nm in OPS:
        y = c.product(nm, c.x[nm])
        for _ in range(3):
            assert c.product(nm, c.x[nm]).tobytes() == y.tobytes(), nm


@pytest.mark.parametrize("name", ["config2_element", "2d", "anisotropic"])
def test_mult_add(pa, name):
    c = _case(pa, name)
    for nm in OPS:
        A = getattr(c.elem, nm)
        y0 = np.random.default_rng(5).uniform(-1, 1, A.getLocalSize()[0])
        xv, yv, zv = A.createVecRight(), A.createVecLeft(), A.createVecLeft()
        xv.setArray(c.x[nm])
        yv.setArray(y0)
        A.multAdd(xv, yv, zv)
        z = zv.getArray()
        # z = y + A x, entry by entry: one rounding on top of the product
        np.testing.assert_array_equal(z, y0 + c.product(nm, c.x[nm]))
        ref = y0.astype(np.longdouble) + c.ref[nm]
        err = np.abs(z.astype(np.longdouble) - ref).astype(np.float64)
        assert np.all(err <= c.bound[nm] + EPS * np.abs(z)), nm
        np.testing.assert_array_equal(yv.getArray(), y0)


# ---------------------------------------------- 6. inputs that must not leak
@pytest.mark.parametrize("name", ["shared_by_8", "partial_batch", "2d"])
def test_nan_stays_in_its_elements(pa, name):
    c = _case(pa, name)
    for nm in OPS:
        R, C = _shape(c.dim, nm)
        clean = c.product(nm, c.x[nm])
        node = int(c.conn[c.E // 2][0])
        x = c.x[nm].copy()
        x[node * C + (C - 1)] = np.nan
        y = c.product(nm, x)
        touched = np.zeros(c.N, bool)
        touched[c.conn[np.any(c.conn == node, axis=1)].ravel()] = True
        rows = np.repeat(touched, R)
        assert np.any(np.isnan(y)) and not np.any(np.isnan(y[~rows])), nm
        assert y[~rows].tobytes() == clean[~rows].tobytes(), nm
        assert np.any(~rows) or c.E == 1


# ---------------------------------------------------------------- 7. refusals
def test_refused_meshes_and_names(pa):
    Mat = pa.petsc.Mat
    from pynama_amd.mesh import UnstructuredMesh
    from pynama_amd.petsc import Options
    um = UnstructuredMesh.from_gmsh(os.path.join(G, "test.msh"), 3)
    half = pa.BoxMesh(3, [2, 2, 2], [0, 0, 0], [1, 1, 1], 3, rank=0, nranks=2)
    c = _case(pa, "shared_by_8")
    for nm in OPS:
        _refused(pa, lambda: Mat.createOperatorElement(um, nm))
        _refused(pa, lambda: Mat.createOperatorElement(half, nm))
    _refused(pa, lambda: Mat.createOperatorElement(c.dom.mesh, "Div"), 62)
    _refused(pa, lambda: Mat.createOperatorElement(c.dom.mesh, "K"), 62)
    mat = pa.MatFS()
    mat.setDomain(c.dom)
    _refused(pa, lambda: mat.build(buildKLE=False, opType="sumfactorised"), 62)
    opts = Options()
    opts.setValue("kle_op_type", "matrixfree")
    try:
        _refused(pa, lambda: mat.build(buildKLE=False), 62)
        _refused(pa, mat.buildOperators, 62)
    finally:
        opts.delValue("kle_op_type")
    assert mat.operator is None or mat.operator.Curl is None
    # unstructured meshes have no element-wise operators
    gm = pa.Domain()
    gm.configure({"domain": {"ngl": 3, "gmsh-file": os.path.join(G, "test.msh")},
                  "boundary-conditions": {"custom-func": {"name": "taylor_green"}}})
    gm.setUp()
    mf = pa.MatFS()
    mf.setDomain(gm)
    _refused(pa, lambda: mf.build(buildKLE=False, opType="element"))


@pytest.mark.parametrize("name", ["shared_by_8", "2d", "cavity"])
def test_refused_calls(pa, name):
    c = _case(pa, name)
    for nm in OPS:
        A = getattr(c.elem, nm)

        def set_operators():
            ksp = pa.petsc.KSP().create()
            ksp.setType("cg")
            ksp.setOperators(A)

        v = A.createVecLeft()
        for fn in (A.getDiagonal, A.getValuesCSR, A.convert, lambda: A.getRow(0), lambda: A.duplicate(copy=True),
                   A.assemble, lambda: A.diagonalScale(v), set_operators, lambda: A.copyDirichletRows(v, v)):
            _refused(pa, fn)
            _, ok = c.within_bound(nm)
            assert ok, nm
        # y must not alias x (square operators only have such a vector)
        if A.getSize()[0] == A.getSize()[1]:
            xv = A.createVecRight()
            xv.setArray(c.x[nm])
            _refused(pa, lambda: A.mult(xv, xv), 62)
        # a vector of another layout
        other = getattr(c.elem, "SrT" if nm == "DivSrT" else "DivSrT")
        assert other.getSize()[1] != A.getSize()[1]
        with pytest.raises(pa.Error) as ei:
            A.mult(other.createVecRight(), A.createVecLeft())
        assert ei.value.ierr == 60, ei.value
        _, ok = c.within_bound(nm)
        assert ok, nm


# ------------------------------------------------------ 8. defaults unchanged
def test_defaults_stay_assembled(pa):
    import ctypes as C
    from pynama_amd._lib import call
    from pynama_amd.matrices import Operators
    dom = _domain(pa, 3, [2, 2, 2], 3)
    mesh = dom.getMesh()
    op = Operators()
    op.setDimensions(dom.getDimensions())
    op.build(mesh)
    ctx = pa.get_ctx()
    h = [C.c_void_p() for _ in range(3)]
    call("kle_assemble_operators", ctx.h, mesh._h, *[C.byref(x) for x in h])
    for nm, hh in zip(OPS, h):
        A = getattr(op, nm)
        assert A.getFormat() != "elem" and A.getInfo()["nz_used"] > 0, nm
        R, Cc = _shape(3, nm)
        B = pa.petsc.Mat._wrap(hh, ctx, mesh, R, Cc)
        for a, b in zip(A.getValuesCSR(), B.getValuesCSR()):
            np.testing.assert_array_equal(a, b)
    # -kle_mat_type element alone leaves the operators assembled
    mat = pa.MatFS()
    mat.setDomain(dom)
    mat.build(kleType="element")
    assert mat.K.getFormat() == "elem" and mat.getOperators().SrT.getFormat() != "elem"
