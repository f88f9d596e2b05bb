"""The sum-factorised element-wise K and Krhs (Mat.createKLESumFactored,
kle_sumfac.hip) on unstructured and box meshes against tests/sumfac_ref.py.

Reference of every product: y_ref = sum_e S_e^T ref_kle(X_e) x~_e in
np.longdouble from mesh.corners() and mesh.conn(), with the derived bound of
sumfac_ref (C_sf roundings of the factorised evaluation over the factor-wise
absolute companion, the operand errors, the gather); beside it the longdouble
product of the assembled mat.K.getValuesCSR(), inside bound + the assembled
bound.  Shapes: the smallest that reach each edge of the kernels (SHAPES).

Worst |y - y_ref| / bound per shape, K / Krhs / diagonal, as measured on an
MI355X (printed by test_product_within_bound and test_diagonal):
see DESIGN.md, "Sum-factorised element-wise K and Krhs"."""
import functools
import os
import tempfile

import numpy as np
import pytest

import elem_ref as R
import sumfac_ref as SF
from oracle import oracle as O

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
G = os.path.join(os.path.dirname(__file__), "golden")
MSH = os.path.join(G, "test.msh")
TG = {2: {"custom-func": {"name": "taylor_green"}}, 3: {"custom-func": {"name": "taylor_green3d"}}}

# name -> list of meshes: (kind, args, ngl[, extras])
SHAPES = {
    "msh2d_gauss": [dict(msh=MSH, dim=2, ngl=3)],                       # Gauss full rule, valence != 4
    "msh2d_gll": [dict(msh=MSH, dim=2, ngl=5)],                         # GLL full rule
    "umesh3d": [dict(golden="umesh3d", dim=3, ngl=3)],                  # rotated, shuffled, distorted hexes
    "distorted_p4": [dict(pbox=(3, [2, 2, 2], 13), dim=3, ngl=5)],      # config 5's element, 2 per batch
    "partial_batch": [dict(pbox=(3, [3, 1, 1], 0), dim=3, ngl=4),      # a last batch that is not full
                      dict(pbox=(3, [3, 3, 2], 0), dim=3, ngl=2)],
    "loop_nodes": [dict(pbox=(3, [2, 2, 2], 3), dim=3, ngl=7)],         # 343 nodes: the thread loop
    "ngl8": [dict(pbox=(3, [1, 1, 1], 0), dim=3, ngl=8),               # 512 nodes; line length 8
             dict(pbox=(2, [3, 2], 0), dim=2, ngl=8)],
    "partial_dirichlet": [dict(pbox=(3, [2, 2, 2], 13), dim=3, ngl=5, faces=["left", "down"])],
    "box": [dict(box=([3, 2, 2], [-1.5, 0.25, 10.0], [2.0, 0.3, 13.0]), dim=3, ngl=5)],
}
CASES = [(n, k) for n, ms in SHAPES.items() for k in range(len(ms))]
_TMP = tempfile.TemporaryDirectory(prefix="sumfac_msh_")


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


def _mesh_file(spec, tag):
    from pynama_amd.meshgen import perturbed_box, write_gmsh
    if "msh" in spec:
        return spec["msh"]
    p = os.path.join(_TMP.name, tag + ".msh")
    if "golden" in spec:
        g = np.load(os.path.join(G, f"case_{spec['golden']}.npz"))
        write_gmsh(p, int(g["dim"]), g["mesh_vertices"], g["mesh_cells"], g["mesh_facets"], g["mesh_tags"])
    else:
        dim, nelem, seed = spec["pbox"]
        write_gmsh(p, dim, *perturbed_box(dim, nelem, seed=seed))
    return p


class Case:
    """One mesh: the assembled and the sum-factorised operators, x, and per
    operator the reference with its bounds, computed once and left unchanged."""

    def __init__(self, pa, name, k):
        spec = SHAPES[name][k]
        self.name, self.dim, self.ngl = f"{name}[{k}]", spec["dim"], spec["ngl"]
        dim, ngl = self.dim, self.ngl
        if "box" in spec:
            nelem, lo, hi = spec["box"]
            domain = {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": lo, "upper": hi}}
        else:
            domain = {"ngl": ngl, "gmsh-file": _mesh_file(spec, f"{name}_{k}")}
        self.dom = dom = pa.Domain()
        dom.configure({"domain": domain, "boundary-conditions": TG[dim]})
        dom.setUp()
        self.mesh = mesh = dom.getMesh()
        faces = spec.get("faces")
        if faces is not None:
            mesh.set_dirichlet_faces(faces)
        self.mat = mat = pa.MatFS()
        mat.setDomain(dom)
        mat.build(buildOperators=False)
        self.N, self.n = mesh.N, mesh.N * dim
        self.dir = np.zeros(mesh.N, bool)
        self.dir[mesh.face_nodes(faces if faces is not None else pa.mesh.FACES[dim])] = True
        self.dird = np.repeat(self.dir, dim)
        self.conn, self.corners = mesh.conn(), mesh.corners()
        self.csr = {"K": mat.K.getValuesCSR(), "Krhs": mat.Krhs.getValuesCSR()}
        self.op = {w: pa.petsc.Mat.createKLESumFactored(mesh, w) for w in ("K", "Krhs")}
        self.x = np.random.default_rng(20241020).uniform(-1, 1, self.n)
        # 3-D ngl >= 7: a sample of node rows (sumfac_ref.sample_nodes)
        self.nodes = SF.sample_nodes(self.conn, ngl, dim, self.dir) if dim == 3 and ngl >= 7 else None
        self._ref = {}

    def ref(self, which):
        if which not in self._ref:
            self._ref[which] = SF.reference(self.dim, self.ngl, self.conn, self.corners, self.dir, which, self.x,
                                            nodes=self.nodes)
        return self._ref[which]

    def product(self, which, x):
        A = self.op[which]
        xv = A.createVecRight()
        xv.setArray(x)
        return (A * xv).getArray()


@functools.lru_cache(maxsize=None)
def _case_cached(name, k):
    import pynama_amd
    return Case(pynama_amd, name, k)


def _case(pa, name, k=0):
    return _case_cached(name, k)


@pytest.mark.parametrize("which", ["K", "Krhs"])
@pytest.mark.parametrize("name,k", CASES)
def test_product_within_bound(pa, name, k, which):
    c = _case(pa, name, k)
    r = c.ref(which)
    y = c.product(which, c.x)
    w, at = R.worst(y[r.rows], r.y, r.bound)
    ya = SF.csr_mult(c.csr[which], c.x)[r.rows]
    wa, ata = R.worst(y[r.rows], ya, r.bound + r.abound)
    print(f"{c.name} {which}: C_sf {SF.C_sf(c.dim, c.ngl)}  rows {len(r.rows)}  worst err/bound {w:.3g} at {at}  "
          f"vs assembled err/(bound + assembled bound) {wa:.3g}")
    # Dirichlet rows: x bit for bit
    np.testing.assert_array_equal(y[c.dird], c.x[c.dird])
    assert w <= 1.0, (c.name, which, w, at)
    assert wa <= 1.0, (c.name, which, wa, ata)
    A = c.op[which]
    assert A.getFormat() == "elem"
    assert A.getSize() == (c.n, c.n) and A.getLocalSize() == (c.n, c.n)
    assert A.getOwnershipRange() == (0, c.n)
    info = A.getInfo()
    assert info["format"] == "elem" and info["nz_used"] == 0 and info["spmv_bytes"] > 0
    assert A.spmvKernel() == f"k_sumfac_elem<{c.dim}>+k_sumfac_gather<{c.dim}>"


@pytest.mark.parametrize("name,k", CASES)
def test_repeatable_and_masking_is_selection(pa, name, k):
    c = _case(pa, name, k)
    free = ~c.dird
    for which, masked in (("K", c.dird), ("Krhs", free)):
        y = c.product(which, c.x)
        for _ in range(2):
            np.testing.assert_array_equal(c.product(which, c.x), y)
        xn = c.x.copy()
        xn[masked] = np.nan
        yn = c.product(which, xn)
        # every summed row is unchanged bit for bit; a Dirichlet row hands back its own x_i
        np.testing.assert_array_equal(yn[free], y[free])
        np.testing.assert_array_equal(yn[c.dird], xn[c.dird])


@pytest.mark.parametrize("name,k", CASES)
def test_diagonal(pa, name, k):
    c = _case(pa, name, k)
    r = c.ref("K")
    dg = c.op["K"].getDiagonal().getArray()
    w, at = R.worst(dg[r.rows], r.diag, r.dbound)
    da = SF.csr_diag(c.csr["K"])
    wa, _ = R.worst(dg[r.rows], da[r.rows].astype(R.LD), r.dbound + r.adbound)
    print(f"{c.name} diagonal: C_diag {SF.C_diag(c.dim, c.ngl)}  worst err/bound {w:.3g} at {at}  vs assembled {wa:.3g}")
    assert np.all(dg[c.dird] == 1.0)
    assert w <= 1.0 and wa <= 1.0
    dk = c.op["Krhs"].getDiagonal().getArray()
    assert np.all(dk[c.dird] == 1.0) and np.all(dk[~c.dird] == 0.0)
    np.testing.assert_array_equal(dk, SF.csr_diag(c.csr["Krhs"]))


@pytest.mark.parametrize("which", ["K", "Krhs"])
def test_mult_add_and_local_timing(pa, which):
    c = _case(pa, "distorted_p4")
    A = c.op[which]
    r = c.ref(which)
    y0 = np.random.default_rng(5).uniform(-1, 1, c.n)
    xv, yv, zv = A.createVecRight(), A.createVecLeft(), A.createVecLeft()
    xv.setArray(c.x)
    yv.setArray(y0)
    A.multAdd(xv, yv, zv)
    z = zv.getArray()
    ref = y0.astype(R.LD)[r.rows] + r.y
    err = np.abs(z[r.rows].astype(R.LD) - ref).astype(np.float64)
    assert np.all(err <= r.bound + EPS * np.abs(z[r.rows]))
    y = c.product(which, c.x)
    ms = A.timeLocalSpmv(xv, zv, reps=3)
    assert ms > 0
    np.testing.assert_array_equal(zv.getArray(), y)


def test_box_equals_element_operator(pa):
    """Kind 0 through the new creator: beside the reference, the product lies
    inside the sum of both operators' bounds of Mat.createKLEElement's
    (tests/test_gpu_elem.py: n eps B_i + delta Kmax X_i around the assembled
    product, n = dim ngl^dim + 8)."""
    from pynama_amd._lib import call
    c = _case(pa, "box")
    dim, ngl, mesh = c.dim, c.ngl, c.mesh
    nd = dim * ngl ** dim
    ctx = pa.get_ctx()
    Ke, Rwe = np.zeros((nd, nd)), np.zeros((nd, 3 * ngl ** dim))
    call("kle_element_kle", ctx.h, mesh._h, 0, Ke, Rwe)
    K0 = Ke.copy()
    Kmax, delta = np.abs(K0).max(), 0.0
    for e in range(1, mesh.E):
        call("kle_element_kle", ctx.h, mesh._h, e, Ke, Rwe)
        delta = max(delta, np.abs(Ke - K0).max() / Kmax)
    assert delta <= 2e-12
    gd = (c.conn[:, :, None] * dim + np.arange(dim)[None, None, :]).reshape(mesh.E, nd)
    for which in ("K", "Krhs"):
        keep = ~c.dird if which == "K" else c.dird
        xe = np.where(keep[gd], np.abs(c.x)[gd], 0.0)
        B, X = np.zeros(c.n), np.zeros(c.n)
        np.add.at(B, gd, xe @ np.abs(K0).T)
        np.add.at(X, gd, np.broadcast_to(xe.sum(axis=1)[:, None], xe.shape))
        ebound = np.where(c.dird, 0.0, (nd + 8) * EPS * B + delta * Kmax * X)
        E = pa.petsc.Mat.createKLEElement(mesh, which)
        xv = E.createVecRight()
        xv.setArray(c.x)
        ye = (E * xv).getArray()
        y = c.product(which, c.x)
        r = c.ref(which)
        # both lie around the assembled product: |y - ye| <= (bound + abound) + ebound
        w, at = R.worst(y, ye.astype(R.LD), r.bound + r.abound + ebound)
        print(f"box {which}: sum-factorised vs dense-GEMM element operator, err / (sum of bounds) {w:.3g}")
        assert w <= 1.0, (which, w, at)


def _vec_to_ours(v, mp, bs):
    return np.asarray(v).reshape(-1, bs)[mp].ravel()


@pytest.mark.parametrize("case", ["gmsh2d", "umesh3d"])
def test_kle_solver_option_matches_golden(pa, case):
    """-kle_k_type sumfac on the golden cases: u to the golden u at the
    tolerance of tests/test_gpu_umesh.py (1e-9 relative at rtol 1e-13), the
    iteration count within 2 of the assembled solve's."""
    from pynama_amd.petsc import Options
    g = np.load(os.path.join(G, f"case_{case}.npz"))
    dim, ngl = int(g["dim"]), int(g["ngl"])
    dw = 1 if dim == 2 else 3
    path = MSH if case == "gmsh2d" else _mesh_file(dict(golden=case), "golden_" + case)
    cfg = {"name": case, "material-properties": {"rho": float(g["rho"]), "mu": float(g["mu"])},
           "domain": {"ngl": ngl, "gmsh-file": path}, "boundary-conditions": TG[dim], "initial-conditions": TG[dim]}
    its = {}
    for ktype in ("assembled", "sumfac"):
        opts = Options()
        if ktype == "sumfac":
            opts.setValue("kle_k_type", "sumfac")
        try:
            prob = pa.BaseProblem(cfg)
            prob.setUp()
            prob.setUpSolver()
        finally:
            opts.delValue("kle_k_type")
        sol = prob.solverKLE
        A = sol.getKSP().getOperators()[0]
        if ktype == "sumfac":
            assert A is prob.mat.getSumFactoredK() and A.getFormat() == "elem" and "k_sumfac_elem" in A.spmvKernel()
            assert prob.mat.getSumFactoredKrhs() is prob.mat.getSumFactoredKrhs()
        else:
            assert A is prob.mat.K
        mp = O.node_map(prob.dom.getFullCoordArray().reshape(-1, dim), g["coords"])
        sol.getKSP().setTolerances(rtol=1e-13)
        vort = prob.vort.duplicate()
        vort.setArray(_vec_to_ours(g["vort0"], mp, dw))
        vel = sol.getSolution()
        vel.setArray(_vec_to_ours(g["vel0"], mp, dim))
        b = sol.rhs(vort)
        np.testing.assert_allclose(b.getArray(), _vec_to_ours(g["b"], mp, dim), rtol=0, atol=1e-12 * np.abs(g["b"]).max())
        sol.solve(vort)
        assert sol.getKSP().getConvergedReason() > 0
        its[ktype] = sol.getKSP().getIterationNumber()
        u = vel.getArray()
        ref = _vec_to_ours(g["u"], mp, dim)
        assert np.linalg.norm(u - ref) <= 1e-9 * np.linalg.norm(ref), ktype
    print(f"{case}: iterations assembled {its['assembled']} sumfac {its['sumfac']}")
    assert abs(its["sumfac"] - its["assembled"]) <= 2, its


@pytest.mark.parametrize("pc", ["none", "jacobi"])
@pytest.mark.parametrize("variant", ["cg", "sr", "pipecg", "gmres"])
def test_krylov_types_converge(pa, variant, pc):
    c = _case(pa, "distorted_p4")
    rtol = 1e-10
    xt = c.mat.K.createVecRight()
    xt.setArray(np.random.default_rng(9).uniform(-1, 1, c.n))
    b = c.mat.K * xt
    A = c.op["K"]
    ksp = pa.petsc.KSP().create()
    ksp.setType({"cg": "cg", "sr": "cg", "pipecg": "pipecg", "gmres": "gmres"}[variant])
    ksp.setCGSingleReduction(variant == "sr")
    p = pa.petsc.PC().create()
    p.setType(pc)
    ksp.setPC(p)
    ksp.setTolerances(rtol=rtol, atol=0.0, max_it=100000)
    ksp.setOperators(A)
    ksp.setUp()
    u = A.createVecRight()
    ksp.solve(b, u)
    assert ksp.getConvergedReason() > 0, ksp.getConvergedReason()
    bh = b.getArray()
    res = np.linalg.norm(bh.astype(R.LD) - SF.csr_mult(c.csr["K"], u.getArray()))
    print(f"{variant} / {pc}: {ksp.getIterationNumber()} iterations, true residual {float(res / np.linalg.norm(bh)):.2e}")
    assert res <= 10 * rtol * np.linalg.norm(bh)


def test_refusals(pa):
    Mat = pa.petsc.Mat

    def refused(fn, code=56):
        with pytest.raises(pa.Error) as ei:
            fn()
        assert ei.value.ierr == code, ei.value

    c = _case(pa, "distorted_p4")
    refused(lambda: Mat.createKLESumFactored(c.mesh, "Rw"))
    refused(lambda: Mat.createKLESumFactored(c.mesh, "Rd"), 62)
    cav = pa.Domain()
    cav.configure({"domain": {"ngl": 3, "box-mesh": {"nelem": [4, 4], "lower": [0, 0], "upper": [1, 1]}},
                   "boundary-conditions": {"no-slip": {"up": [2, 0], "down": [0, 0], "left": [0, 0],
                                                       "right": [0, 0]}}})
    cav.setUp()
    refused(lambda: Mat.createKLESumFactored(cav.getMesh(), "K"))
    half = pa.BoxMesh(3, [2, 2, 2], [0, 0, 0], [1, 1, 1], 3, rank=0, nranks=2)
    half.set_dirichlet_faces(pa.mesh.FACES[3])
    refused(lambda: Mat.createKLESumFactored(half, "K"))
    # calls that need stored values
    A = c.op["K"]
    v = A.createVecLeft()
    refused(A.getValuesCSR)
    refused(A.convert)
    refused(lambda: A.setOption(A.Option.SPD, True))
    refused(lambda: A.getRow(0))
    refused(lambda: A.duplicate(copy=True))
    refused(lambda: A.diagonalScale(v))
    refused(A.assemble)
    refused(lambda: A.copyDirichletRows(v, A.createVecLeft()))

    def lu():
        ksp = pa.petsc.KSP().create()
        p = pa.petsc.PC().create()
        p.setType("lu")
        ksp.setPC(p)
        ksp.setOperators(A)
        ksp.setUp()
    refused(lu)
    # y aliasing x
    xv = A.createVecRight()
    xv.setArray(c.x)
    with pytest.raises(pa.Error):
        A.mult(xv, xv)
    # the solver option: any other value still raises 62 and names the three
    from pynama_amd.petsc import Options
    opts = Options()
    opts.setValue("kle_k_type", "bogus")
    try:
        sol = pa.KleSolver()
        sol.setMat(c.mat)
        with pytest.raises(pa.Error) as ei:
            sol.setUp()
        assert ei.value.ierr == 62
        assert all(w in str(ei.value) for w in ("assembled", "element", "sumfac"))
    finally:
        opts.delValue("kle_k_type")
    # ... and the operator still works afterwards
    np.testing.assert_array_equal(c.product("K", c.x), c.product("K", c.x))
