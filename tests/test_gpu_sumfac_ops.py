"""The sum-factorised Rw (Mat.createRwSumFactored, kle_sumfac.hip) and the
collocation operators with per-element geometry (Mat.createOperatorSumFactored,
kle_colloc.hip) on unstructured and box meshes against tests/sumfac_ops_ref.py,
and the matrix-free build -kle_mat_type sumfac -kle_op_type sumfac.

Reference of every product: the longdouble sums of sumfac_ops_ref from
mesh.corners() and mesh.conn() with their derived bounds (C_rw / C_op roundings
over the factor-wise absolute companions, the operand errors, the gather, the
weight); beside it the longdouble product of the assembled matrix's
getValuesCSR(), inside bound + the assembled bound.  Shapes: those of
tests/test_gpu_sumfac.py (SHAPES), the smallest that reach each edge.

Worst |y - y_ref| / bound per shape as measured on an MI355X (printed by
test_product_within_bound): see DESIGN.md, "Matrix-free evalRHS on
unstructured meshes"."""
import functools
import os

import numpy as np
import pytest

import elem_ref as R
import sumfac_ops_ref as SO
import sumfac_ref as SF
from oracle import oracle as O
from test_gpu_sumfac import CASES, G, MSH, SHAPES, TG, _mesh_file

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NAMES = ("Rw",) + SO.OPS


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


def _domain(pa, spec, tag, bc=None):
    dim, ngl = spec["dim"], spec["ngl"]
    if "box" in spec:
        nelem, lo, hi = spec["box"]
        domain = {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": lo, "upper": hi}}
    else:
        domain = {"ngl": ngl, "gmsh-file": _mesh_file(spec, tag)}
    dom = pa.Domain()
    dom.configure({"domain": domain, "boundary-conditions": bc or TG[dim]})
    dom.setUp()
    faces = spec.get("faces")
    if faces is not None:
        dom.getMesh().set_dirichlet_faces(faces)
    return dom


class Case:
    """One mesh: the assembled Rw, Curl, SrT, DivSrT and the sum-factorised
    ones, one x per operator, and the references, computed once."""

    def __init__(self, pa, name, k):
        spec = SHAPES[name][k]
        self.name, self.dim, self.ngl = f"{name}[{k}]", spec["dim"], spec["ngl"]
        dim, ngl = self.dim, self.ngl
        self.dom = dom = _domain(pa, spec, f"ops_{name}_{k}")
        self.mesh = mesh = dom.getMesh()
        self.mat = mat = pa.MatFS()
        mat.setDomain(dom)
        mat.build()
        faces = spec.get("faces")
        self.N = mesh.N
        self.dir = np.zeros(mesh.N, bool)
        self.dir[mesh.face_nodes(faces if faces is not None else pa.mesh.FACES[dim])] = True
        self.conn, self.corners = mesh.conn(), mesh.corners()
        asm = {"Rw": mat.Rw, **{nm: getattr(mat.getOperators(), nm) for nm in SO.OPS}}
        self.csr = {nm: A.getValuesCSR() for nm, A in asm.items()}
        Mat = pa.petsc.Mat
        self.op = {"Rw": Mat.createRwSumFactored(mesh), **{nm: Mat.createOperatorSumFactored(mesh, nm) for nm in SO.OPS}}
        rng = np.random.default_rng(20261020)
        self.x = {nm: rng.uniform(-1, 1, A.getSize()[1]) for nm, A in self.op.items()}
        self.nodes = SF.sample_nodes(self.conn, ngl, dim, self.dir) if dim == 3 and ngl >= 7 else None
        self._ref = {}

    def rbs(self, nm):
        return self.dim if nm == "Rw" else SO.op_shape(self.dim, nm)[0]

    def ref(self, nm):
        if nm not in self._ref:
            if nm == "Rw":
                self._ref[nm] = SO.rw_reference(self.dim, self.ngl, self.conn, self.corners, self.dir, self.x[nm],
                                                nodes=self.nodes)
            else:
                self._ref[nm] = SO.ops_reference(self.dim, self.ngl, self.conn, self.corners, nm, self.x[nm],
                                                 nodes=self.nodes)
        return self._ref[nm]

    def product(self, nm, x, A=None):
        A = A or self.op[nm]
        xv = A.createVecRight()
        xv.setArray(x)
        return (A * xv).getArray()


@functools.lru_cache(maxsize=None)
def _case_cached(name, k):
    import pynama_amd
    return Case(pynama_amd, name, k)


def _case(pa, name, k=0):
    return _case_cached(name, k)


@pytest.mark.parametrize("nm", NAMES)
@pytest.mark.parametrize("name,k", CASES)
def test_product_within_bound(pa, name, k, nm):
    c = _case(pa, name, k)
    r = c.ref(nm)
    x = c.x[nm]
    y = c.product(nm, x)
    w, at = R.worst(y[r.rows], r.y, r.bound)
    ya = SF.csr_mult(c.csr[nm], x)[r.rows]
    wa, ata = R.worst(y[r.rows], ya, r.bound + r.abound)
    cc = SO.C_rw(c.dim, c.ngl) if nm == "Rw" else SO.C_op(c.dim, c.ngl)
    print(f"{c.name} {nm}: C {cc}  rows {len(r.rows)}  worst err/bound {w:.3g} at {at}  "
          f"vs assembled err/(bound + assembled bound) {wa:.3g}")
    assert w <= 1.0, (c.name, nm, w, at)
    assert wa <= 1.0, (c.name, nm, wa, ata)
    if nm == "Rw":  # Dirichlet rows: +0.0 in bytes
        dird = np.repeat(c.dir, c.dim)
        assert dird.any() and y[dird].tobytes() == np.zeros(int(dird.sum())).tobytes()
    # three products bit-equal
    for _ in range(2):
        np.testing.assert_array_equal(c.product(nm, x), y)
    A = c.op[nm]
    m, n = c.N * c.rbs(nm), len(x)
    assert A.getFormat() == "elem"
    assert A.getSize() == (m, n) and A.getLocalSize() == (m, n) and A.getOwnershipRange() == (0, m)
    info = A.getInfo()
    assert info["format"] == "elem" and info["nz_used"] == 0 and info["spmv_bytes"] > 0
    want = (f"k_sumfac_rw<{c.dim}>+k_sumfac_gather_rw<{c.dim}>" if nm == "Rw" else
            f"k_colloc_elem<{c.dim},{nm},geo>+k_colloc_gather_csr<{c.rbs(nm)}>")
    assert A.spmvKernel() == want


@pytest.mark.parametrize("nm", NAMES)
@pytest.mark.parametrize("name", ["msh2d_gauss", "distorted_p4"])
def test_mult_add_and_local_timing(pa, name, nm):
    c = _case(pa, name)
    A, r, x = c.op[nm], c.ref(nm), c.x[nm]
    y0 = np.random.default_rng(5).uniform(-1, 1, A.getSize()[0])
    xv, yv, zv = A.createVecRight(), A.createVecLeft(), A.createVecLeft()
    xv.setArray(x)
    yv.setArray(y0)
    A.multAdd(xv, yv, zv)
    z = zv.getArray()
    ref = y0.astype(R.LD)[r.rows] + r.y
    err = np.abs(z[r.rows].astype(R.LD) - ref).astype(np.float64)
    assert np.all(err <= r.bound + EPS * np.abs(z[r.rows]))
    y = c.product(nm, x)
    assert A.timeLocalSpmv(xv, zv, reps=3) > 0
    np.testing.assert_array_equal(zv.getArray(), y)


@pytest.mark.parametrize("ngl_case", ["msh2d_gauss", "msh2d_gll"])
def test_weighted_rows_at_valence_3_and_5(pa, ngl_case):
    """test.msh has nodes in 3 and in 5 elements, which the box operators'
    padded [N][2^dim] table cannot hold: their rows, checked explicitly."""
    c = _case(pa, ngl_case)
    inc = SF.incidence(c.conn, c.N)
    for nm in SO.OPS:
        r, rb = c.ref(nm), c.rbs(nm)
        y = c.product(nm, c.x[nm])
        for v in (3, 5):
            nodes = np.nonzero(inc == v)[0]
            assert len(nodes), v
            rows = R.dof(nodes, rb)
            w, at = R.worst(y[rows], r.y[rows], r.bound[rows])
            wa, _ = R.worst(y[rows], SF.csr_mult(c.csr[nm], c.x[nm])[rows], (r.bound + r.abound)[rows])
            print(f"{c.name} {nm}: valence {v}, {len(nodes)} nodes, worst err/bound {w:.3g}, vs assembled {wa:.3g}")
            assert w <= 1.0 and wa <= 1.0 and np.all(y[rows] != 0)


def test_shared_geometry_does_not_change_bits(pa):
    """ngl 5: the full rule is GLL(5), so the operators' nodal table is the
    full-rule table of K, Krhs and Rw.  Whichever is created first, and after
    the others are destroyed, every product is the same bits."""
    Mat = pa.petsc.Mat
    spec = SHAPES["distorted_p4"][0]
    c = _case(pa, "distorted_p4")
    xk = np.random.default_rng(1).uniform(-1, 1, c.N * c.dim)

    def products(first):
        dom = _domain(pa, spec, "ops_shared_" + first)
        mesh = dom.getMesh()
        ops = {}
        order = ("K", "Krhs", "Rw") + SO.OPS if first == "K" else SO.OPS[::-1] + ("Rw", "Krhs", "K")
        for nm in order:
            ops[nm] = (Mat.createKLESumFactored(mesh, nm) if nm in ("K", "Krhs") else
                       Mat.createRwSumFactored(mesh) if nm == "Rw" else Mat.createOperatorSumFactored(mesh, nm))
        x = {nm: (xk if nm in ("K", "Krhs") else c.x[nm]) for nm in ops}
        y = {nm: c.product(nm, x[nm], A) for nm, A in ops.items()}
        return ops, x, y

    opsK, x, yK = products("K")
    opsO, _, yO = products("ops")
    for nm in yK:
        np.testing.assert_array_equal(yK[nm], yO[nm], err_msg=nm)
        if nm in NAMES:  # ... and the bits of the operators that were created alone per mesh order
            np.testing.assert_array_equal(yK[nm], c.product(nm, c.x[nm]), err_msg=nm)
    # destroy all but one holder of each set, in both orders
    for ops, keep in ((opsK, "Curl"), (opsO, "K")):
        for nm, A in ops.items():
            if nm != keep:
                A.destroy()
        np.testing.assert_array_equal(c.product(keep, x[keep], ops[keep]), yK[keep], err_msg=keep)
        ops[keep].destroy()


def _refused(pa, fn, ierr=56):
    with pytest.raises(pa.Error) as ei:
        fn()
    assert ei.value.ierr == ierr, ei.value


def test_refusals(pa):
    Mat = pa.petsc.Mat
    from pynama_amd.mesh import UnstructuredMesh
    c = _case(pa, "distorted_p4")
    c2 = _case(pa, "msh2d_gauss")
    half = pa.BoxMesh(3, [2, 2, 2], [0, 0, 0], [1, 1, 1], 3, rank=0, nranks=2)
    half.set_dirichlet_faces(pa.mesh.FACES[3])
    _refused(pa, lambda: Mat.createRwSumFactored(half))
    for nm in SO.OPS:
        _refused(pa, lambda: Mat.createOperatorSumFactored(half, nm))
    _refused(pa, lambda: Mat.createOperatorSumFactored(c.mesh, "Div"), 62)
    _refused(pa, lambda: Mat.createOperatorSumFactored(c.mesh, "K"), 62)
    # the pinned refusals stay
    _refused(pa, lambda: Mat.createKLESumFactored(c.mesh, "Rw"))
    um = UnstructuredMesh.from_gmsh(MSH, 3)
    _refused(pa, lambda: Mat.createOperatorElement(um, "Curl"))
    # a no-slip mesh: Rw refused, the operators accepted (test_noslip_operators)
    cav = pa.Domain()
    cav.configure({"domain": {"ngl": 3, "box-mesh": {"nelem": [4, 4], "lower": [0, 0], "upper": [1, 1]}},
                   "boundary-conditions": {"no-slip": {"up": [2, 0], "down": [0, 0], "left": [0, 0],
                                                       "right": [0, 0]}}})
    cav.setUp()
    _refused(pa, lambda: Mat.createRwSumFactored(cav.getMesh()))
    ns = pa.MatNS()
    ns.setDomain(cav)
    _refused(pa, lambda: ns.build(kleType="sumfac"))
    _refused(pa, lambda: ns.build(kleType="element"))
    for bad in ("matrixfree", "", "Element", "dense", "sumfactorised"):
        mf = pa.MatFS()
        mf.setDomain(c.dom)
        _refused(pa, lambda: mf.build(kleType=bad), 62)
        _refused(pa, lambda: mf.build(buildKLE=False, opType=bad), 62)
    # calls that need stored values, the diagonal, the Dirichlet copy
    for nm in NAMES:
        A = c.op[nm]
        v = A.createVecLeft()
        for fn in (A.getValuesCSR, A.convert, lambda: A.setOption(A.Option.SPD, True), lambda: A.getRow(0),
                   lambda: A.duplicate(copy=True), lambda: A.diagonalScale(v), A.assemble, A.getDiagonal,
                   lambda: A.copyDirichletRows(v, A.createVecLeft())):
            _refused(pa, fn)
        if nm != "Rw":
            _refused(pa, lambda: pa.petsc.KSP().create().setOperators(A))
    # y aliasing x (the square operators have such a vector)
    A = c.op["Rw"]
    xv = A.createVecRight()
    xv.setArray(c.x["Rw"])
    with pytest.raises(pa.Error):
        A.mult(xv, xv)
    # the non-square 2-D Rw is no KSP operator
    with pytest.raises(pa.Error):
        pa.petsc.KSP().create().setOperators(c2.op["Rw"])
    # ... and everything still works afterwards
    for nm in NAMES:
        np.testing.assert_array_equal(c.product(nm, c.x[nm]), c.product(nm, c.x[nm]))


def _vec_to_ours(v, mp, bs):
    return np.asarray(v).reshape(-1, bs)[mp].ravel()


@pytest.mark.parametrize("case", ["gmsh2d", "umesh3d"])
def test_matrix_free_problem_matches_golden(pa, case):
    """-kle_mat_type sumfac -kle_op_type sumfac through BaseProblem: nothing is
    assembled, and the assertions of tests/test_gpu_umesh.py
    test_umesh_solve_and_eval_rhs_match_golden hold with its tolerances."""
    from pynama_amd.petsc import Options
    g = np.load(os.path.join(G, f"case_{case}.npz"))
    dim, ngl = int(g["dim"]), int(g["ngl"])
    dw = 1 if dim == 2 else 3
    path = MSH if case == "gmsh2d" else _mesh_file(dict(golden=case), "ops_golden_" + case)
    cfg = {"name": case, "material-properties": {"rho": float(g["rho"]), "mu": float(g["mu"])},
           "domain": {"ngl": ngl, "gmsh-file": path}, "boundary-conditions": TG[dim], "initial-conditions": TG[dim]}
    opts = Options()
    opts.setValue("kle_mat_type", "sumfac")
    opts.setValue("kle_op_type", "sumfac")
    try:
        prob = pa.BaseProblem(cfg)
        prob.setUp()
        prob.setUpSolver()
    finally:
        opts.delValue("kle_mat_type")
        opts.delValue("kle_op_type")
    mat, op = prob.mat, prob.mat.getOperators()
    six = [mat.K, mat.Krhs, mat.Rw, op.Curl, op.SrT, op.DivSrT]
    for A in six:
        assert A.getFormat() == "elem" and A.getInfo()["nz_used"] == 0, A.getName()
    assert mat.kle[:3] == [mat.K, mat.Krhs, mat.Rw] and mat.kle[3] is mat.Rd and mat.Rd.getInfo()["nz_used"] == 0
    assert mat.Rw is mat.getSumFactoredRw() and "k_sumfac_rw" in mat.Rw.spmvKernel()
    mp = O.node_map(prob.dom.getFullCoordArray().reshape(-1, dim), g["coords"])
    sol = prob.solverKLE
    assert sol.getKSP().getOperators()[0] is mat.K
    sol.getKSP().setTolerances(rtol=1e-13)
    vort = prob.vort.duplicate()
    vort.setArray(_vec_to_ours(g["vort0"], mp, dw))
    vel = sol.getSolution()
    vel.setArray(_vec_to_ours(g["vel0"], mp, dim))
    b = sol.rhs(vort)
    np.testing.assert_allclose(b.getArray(), _vec_to_ours(g["b"], mp, dim), rtol=0,
                               atol=1e-12 * np.abs(g["b"]).max())
    sol.solve(vort)
    assert sol.getKSP().getConvergedReason() > 0
    u = vel.getArray()
    ref = _vec_to_ours(g["u"], mp, dim)
    assert np.linalg.norm(u - ref) <= 1e-9 * np.linalg.norm(ref)
    ex = _vec_to_ours(g["u_exact"], mp, dim)
    assert abs(np.linalg.norm(u - ex) - float(g["err_l2"])) <= 1e-8 * max(1.0, float(g["err_l2"]))
    prob.vort.setArray(_vec_to_ours(g["rhs_vort_in"], mp, dw))
    f = prob.operator.Curl.createVecLeft()
    prob.evalRHS(None, float(g["rhs_t"]), prob.vort, f)
    np.testing.assert_allclose(prob.vort.getArray(), _vec_to_ours(g["rhs_vort_bc"], mp, dw), rtol=0,
                               atol=1e-12 * max(1.0, np.abs(g["rhs_vort_bc"]).max()))
    uu = sol.getSolution().getArray()
    rv = _vec_to_ours(g["rhs_vel"], mp, dim)
    assert np.linalg.norm(uu - rv) <= 1e-9 * max(1.0, np.linalg.norm(rv))
    rf = _vec_to_ours(g["rhs_f"], mp, dw)
    assert np.abs(f.getArray() - rf).max() <= 1e-6 * max(1.0, np.abs(rf).max())


def test_matrix_free_solve_agrees_with_assembled(pa):
    """Taylor-Green on perturbed_box(3, [3, 3, 3], seed=5), ngl 5: the
    matrix-free solve and the assembled solve at rtol 1e-13 agree to 1e-9."""
    from pynama_amd.petsc import Options
    path = _mesh_file(dict(pbox=(3, [3, 3, 3], 5)), "ops_tg333")
    cfg = {"name": "tg333", "material-properties": {"rho": 1.0, "mu": 0.01},
           "domain": {"ngl": 5, "gmsh-file": path}, "boundary-conditions": TG[3], "initial-conditions": TG[3]}
    u = {}
    for form in ("assembled", "sumfac"):
        opts = Options()
        if form == "sumfac":
            opts.setValue("kle_mat_type", "sumfac")
            opts.setValue("kle_op_type", "sumfac")
        try:
            prob = pa.BaseProblem(cfg)
            prob.setUp()
            prob.setUpSolver()
        finally:
            opts.delValue("kle_mat_type")
            opts.delValue("kle_op_type")
        assert prob.mat.K.getFormat() == ("elem" if form == "sumfac" else "nb")
        sol = prob.solverKLE
        sol.getKSP().setTolerances(rtol=1e-13)
        sol.solve(prob.vort)  # (vort and the Dirichlet values of vel: the initial conditions)
        assert sol.getKSP().getConvergedReason() > 0
        u[form] = sol.getSolution().getArray().copy()
    assert np.linalg.norm(u["assembled"]) > 0
    assert np.linalg.norm(u["sumfac"] - u["assembled"]) <= 1e-9 * np.linalg.norm(u["assembled"])


def test_noslip_operators(pa):
    """A no-slip Gmsh case (case_gmsh2d_ns: a wall on test.msh): MatNS with
    opType="sumfac" keeps the NS matrices assembled and builds the three
    operators matrix-free; their products lie inside bound + assembled bound of
    the assembled operators'."""
    g = np.load(os.path.join(G, "case_gmsh2d_ns.npz"))
    dim, ngl = int(g["dim"]), int(g["ngl"])
    dom = pa.Domain()
    dom.configure({"domain": {"ngl": ngl, "gmsh-file": MSH}, "boundary-conditions": {"no-slip": {"down": [1, 0]}}})
    dom.setUp()
    mesh = dom.getMesh()
    mat = pa.MatNS()
    mat.setDomain(dom)
    mat.build(opType="sumfac")
    assert mat.K.getFormat() == "nb" and mat.getKplusKfs().getFormat() == "nb"
    asm = pa.Operators()
    asm.setDimensions(dom.getDimensions())
    asm.build(mesh, "assembled")
    conn, corners = mesh.conn(), mesh.corners()
    for nm in SO.OPS:
        A = getattr(mat.getOperators(), nm)
        assert A.getFormat() == "elem" and A.getInfo()["nz_used"] == 0
        x = np.random.default_rng(31).uniform(-1, 1, A.getSize()[1])
        xv = A.createVecRight()
        xv.setArray(x)
        y = (A * xv).getArray()
        r = SO.ops_reference(dim, ngl, conn, corners, nm, x)
        w, at = R.worst(y, r.y, r.bound)
        wa, _ = R.worst(y, SF.csr_mult(getattr(asm, nm).getValuesCSR(), x), r.bound + r.abound)
        print(f"gmsh2d_ns {nm}: worst err/bound {w:.3g}, vs assembled err/(bound + assembled bound) {wa:.3g}")
        assert w <= 1.0 and wa <= 1.0, (nm, w, wa)
