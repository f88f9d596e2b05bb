"""The sum-factorised no-slip operators (Mat.createNSSumFactored,
kle_sumfac.hip) and the matrix-free no-slip KLE system on any mesh
(MatNS.build(nsType="sumfac"), -kle_ns_type sumfac) on one rank, against
tests/sumfac_ns_ref.py.

Reference of every product: the longdouble mesh-level sum of sumfac_ns_ref
from mesh.conn(), mesh.corners() and the domain's DoF classes, with its derived
bound (C_sf / C_rw roundings over the factor-wise companions, the operand
errors, the gather, one more addition on Kfs's tangential rows); beside it the
longdouble product of the assembled MatNS matrix's getValuesCSR(), inside
bound + assembled bound.  Identity rows are compared bit for bit, zero rows
must be +0.0.  Shapes: the smallest that reach each edge of the kernels
(SHAPES).

Selection: a NaN in a column class a pass drops must not reach that pass's
rows, which stay bit-equal to the clean product (an identity row hands back the
x_i it was given, NaN included).

Worst |y - y_ref| / bound per shape, as measured on an MI355X (printed by
test_products_within_bound and test_diagonal): see DESIGN.md, "Sum-factorised
no-slip operators"."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest

import elem_ref as R
import sumfac_ns_ref as SN
import sumfac_ref as SF
from oracle import oracle as O

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
G = os.path.join(os.path.dirname(__file__), "golden")
MSH = os.path.join(G, "test.msh")
F, T, N = SN.F, SN.T, SN.N
OPS, SPECS = SN.OPS, SN.SPECS
SIX = {"up": [1, 0, 0.5], "down": [0, 0, 0], "left": [0, 0, 0], "right": [0, 0, 0], "front": [0, 0, 0],
       "back": [0, 0, 0]}
UPDOWN = {"up": [1, 0, 0.5], "down": [0, 0, 0]}
SHAPES = {
    "msh2d_gauss": dict(msh=MSH, dim=2, ngl=3, walls={"down": [1, 0]}),      # Gauss full rule, valence != 4
    "msh2d_gll": dict(msh=MSH, dim=2, ngl=5, walls={"down": [1, 0]}),        # GLL full rule
    "umesh3d": dict(golden="umesh3d_ns", dim=3, ngl=3, walls=SIX),           # rotated, shuffled, distorted hexes
    "ftn_element": dict(pbox=(3, [2, 2, 2], 13), dim=3, ngl=5, walls=UPDOWN),  # F, T and N on one element
    "partial_batch": dict(pbox=(3, [3, 1, 1], 0), dim=3, ngl=4, walls=SIX),  # a last batch that is not full
    "one_free_node": dict(pbox=(3, [1, 1, 1], 0), dim=3, ngl=3, walls=SIX),
    "loop_nodes": dict(pbox=(3, [1, 1, 2], 0), dim=3, ngl=7, walls=SIX),     # 343 nodes: the thread loop, sampled rows
    "box": dict(box=[3, 2, 2], dim=3, ngl=3, walls=SIX),                     # kind 0, beside createNSElement
}
_TMP = tempfile.TemporaryDirectory(prefix="sumfac_ns_msh_")


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


def _domain_cfg(spec, tag):
    dim, ngl = spec["dim"], spec["ngl"]
    if "box" in spec:
        return {"ngl": ngl, "box-mesh": {"nelem": spec["box"], "lower": [0] * dim, "upper": [1] * dim}}
    return {"ngl": ngl, "gmsh-file": _mesh_file(spec, tag)}


def _domain(pa, spec, tag):
    dom = pa.Domain()
    dom.configure({"domain": _domain_cfg(spec, tag), "boundary-conditions": {"no-slip": spec["walls"]}})
    dom.setUp()
    return dom


def _classes(dom, n):
    cls = np.zeros(n, np.int64)
    cls[np.asarray(sorted(dom.getTangDofs(collect=True)), np.int64)] = T
    cls[np.asarray(sorted(dom.getNormalDofs(collect=True)), np.int64)] = N  # normal wins (mat_ns.py:60-62)
    return cls


def _gdof(conn, bs):
    """[E, nn bs]: the global DoFs of every element, node-major."""
    return (conn[:, :, None] * bs + np.arange(bs)[None, None, :]).reshape(conn.shape[0], -1)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


class Case:
    """One mesh: the assembled MatNS, the seven sum-factorised operators, x and
    w, and per operator the reference with its bounds, computed once and left
    unchanged."""

    def __init__(self, pa, name):
        from pynama_amd.petsc import Mat
        spec = SHAPES[name]
        self.name, self.dim, self.ngl = name, spec["dim"], spec["ngl"]
        dim = self.dim
        self.dw = dw = 1 if dim == 2 else 3
        self.dom = dom = _domain(pa, spec, name)
        self.mesh = mesh = dom.getMesh()
        self.mat = mat = pa.MatNS()
        mat.setDomain(dom)
        mat.build(buildOperators=False)
        self.n, self.nw = mesh.N * dim, mesh.N * dw
        self.cls = _classes(dom, self.n)
        self.conn, self.corners = mesh.conn(), mesh.corners()
        self.asm = {"K": mat.K, "Krhs": mat.Krhs, "Rw": mat.Rw, "Kfs": mat.Kfs, "Krhsfs": mat.Krhsfs,
                    "Rwfs": mat.Rwfs, "K+Kfs": mat.getKplusKfs()}
        self.csr = {k: A.getValuesCSR() for k, A in self.asm.items()}
        self.op = {k: Mat.createNSSumFactored(mesh, k) for k in OPS}
        rng = np.random.default_rng(20241020)
        self.x = rng.uniform(-1, 1, self.n)
        self.w = rng.uniform(-1, 1, self.nw)
        # 3-D ngl >= 7: a sample of node rows (sumfac_ref.sample_nodes; wall nodes as its Dirichlet nodes)
        self.nodes = SF.sample_nodes(self.conn, self.ngl, dim, SN.wall_nodes(self.cls, dim), per_class=6) \
            if dim == 3 and self.ngl >= 7 else None
        self._ref = {}

    def input(self, name):
        return self.w if name in SN.RW else self.x

    def ref(self, name):
        if name not in self._ref:
            self._ref[name] = SN.reference(self.dim, self.ngl, self.conn, self.corners, self.cls, name,
                                           self.input(name), nodes=self.nodes)
        return self._ref[name]

    def product(self, name, x):
        A = self.op[name]
        xv = A.createVecRight()
        xv.setArray(x)
        return (A * xv).getArray()

    def rows(self, classes):
        return SN.isin(self.cls, classes)


@functools.lru_cache(maxsize=None)
def _case_cached(name):
    import pynama_amd
    return Case(pynama_amd, name)


def _case(pa, name):
    return _case_cached(name)


def _check_product(c, name, y, label):
    """y = op x (x the clean input) against the reference, the assembled product
    and the exact rows; -> worst err/bound."""
    r = c.ref(name)
    x = c.input(name)
    s = r.summed
    w, at = R.worst(y[r.rows][s], r.y[s], r.bound[s])
    ya = SF.csr_mult(c.csr[name], x)[r.rows]
    wa, ata = R.worst(y[r.rows][s], ya[s], (r.bound + r.abound)[s])
    print(f"{label} {name}: rows {int(s.sum())}  worst err/bound {w:.3g} at {at}  "
          f"vs assembled err/(bound + assembled bound) {wa:.3g}")
    assert w <= 1.0, (label, name, w, at)
    assert wa <= 1.0, (label, name, wa, ata)
    S = SPECS[name]
    ident, zero = c.rows(S["ident"]), c.rows(S["zero"])
    if ident.any():  # (Rw, Rwfs have none: their x is the vorticity, of another length in 2-D)
        np.testing.assert_array_equal(_bits(y[ident]), _bits(x[ident]), err_msg=name)
    assert np.all(y[zero] == 0.0) and not np.any(np.signbit(y[zero])), name
    return w


# ------------------------------------------------------------ 1. the products
@pytest.mark.parametrize("shape", list(SHAPES))
def test_products_within_bound(pa, shape):
    c = _case(pa, shape)
    worst = {}
    for name in OPS:
        A = c.op[name]
        rw = name in SN.RW
        ncol = c.nw if rw else c.n
        assert A.getFormat() == "elem"
        assert A.getSize() == (c.n, ncol) and A.getLocalSize() == (c.n, ncol)
        assert A.getOwnershipRange() == (0, c.n)
        info = A.getInfo()
        assert info["format"] == "elem" and info["nz_used"] == 0 and info["spmv_bytes"] > 0
        d = c.dim
        want = (f"k_sumfac_rw<{d}>" if rw else f"k_sumfac_elem<{d},cls>" + ("x2" if name == "Kfs" else "")) + \
            f"+k_sumfac_gather_cls<{d}>"
        assert A.spmvKernel() == want
        y = c.product(name, c.input(name))
        worst[name] = _check_product(c, name, y, shape)
        if shape != "one_free_node" or name in ("K", "K+Kfs", "Kfs"):
            assert np.any(y[~c.rows(SPECS[name]["ident"] | SPECS[name]["zero"])] != 0.0), name
        # repeated: identical bits
        for _ in range(2):
            np.testing.assert_array_equal(_bits(c.product(name, c.input(name))), _bits(y), err_msg=name)
    print(f"{shape}: C_sf {SF.C_sf(c.dim, c.ngl)}  worst err/bound {max(worst.values()):.3g} "
          f"({max(worst, key=worst.get)})  " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_class_counts(pa):
    """The meshes reach what they are there for."""
    assert _case(pa, "one_free_node").rows({F}).sum() == 3
    c = _case(pa, "ftn_element")
    gd = _gdof(c.conn, c.dim)
    assert any(set(np.unique(c.cls[g])) == {F, T, N} for g in gd)
    c = _case(pa, "partial_batch")
    assert c.conn.shape == (3, 64) and 256 // 64 > 3 % (256 // 64) > 0  # 4 elements per workgroup, 3 in the only one
    assert _case(pa, "loop_nodes").conn.shape[1] == 343
    inc = SF.incidence(_case(pa, "msh2d_gauss").conn, _case(pa, "msh2d_gauss").mesh.N)
    assert {3, 5} <= set(np.unique(inc))
    c = _case(pa, "msh2d_gll")
    assert c.rows({F}).any() and c.rows({T}).any() and c.rows({N}).any()


# ------------------------------------------------------------ 2. selection
@pytest.mark.parametrize("shape", list(SHAPES))
def test_dropped_columns_are_never_read(pa, shape):
    c = _case(pa, shape)
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


@pytest.mark.parametrize("shape", ["msh2d_gauss", "umesh3d"])
def test_all_nan_input(pa, shape):
    c = _case(pa, shape)
    for name in OPS:
        S = SPECS[name]
        y = c.product(name, np.full(c.nw if name in SN.RW else c.n, np.nan))
        ident, zero = c.rows(S["ident"]), c.rows(S["zero"])
        assert np.all(np.isnan(y[ident])), name
        assert np.all(y[zero] == 0.0) and not np.any(np.signbit(y[zero])), name


# ------------------------------------------------ 3. diagonal, multAdd, copies
@pytest.mark.parametrize("shape", list(SHAPES))
def test_diagonal(pa, shape):
    c = _case(pa, shape)
    worst = {}
    for name in ("K", "Kfs", "K+Kfs"):
        r = c.ref(name)
        S = SPECS[name]
        d = c.op[name].getDiagonal().getArray()
        ident, zero = c.rows(S["ident"]), c.rows(S["zero"])
        np.testing.assert_array_equal(d[ident], np.ones(int(ident.sum())))
        assert np.all(d[zero] == 0.0) and not np.any(np.signbit(d[zero]))
        w, at = R.worst(d[r.rows], r.diag, r.dbound)
        da = SF.csr_diag(c.csr[name])
        wa, ata = R.worst(d[r.rows], da[r.rows].astype(R.LD), r.dbound + r.adbound)
        print(f"{shape} diagonal {name}: C_diag {SF.C_diag(c.dim, c.ngl)}  worst err/bound {w:.3g} at {at}  "
              f"vs assembled {wa:.3g}")
        assert w <= 1.0 and wa <= 1.0, (name, w, at, wa, ata)
        worst[name] = w
    for name in ("Krhs", "Krhsfs"):
        d = c.op[name].getDiagonal().getArray()
        np.testing.assert_array_equal(_bits(d), _bits(np.where(c.rows(SPECS[name]["ident"]), 1.0, 0.0)))
    for name in SN.RW:
        with pytest.raises(pa.Error) as ei:
            c.op[name].getDiagonal()
        assert ei.value.ierr == 56
    print(f"{shape}: diagonal worst err/bound {max(worst.values()):.3g}")


def test_mult_add_local_timing_and_copy_identity_rows(pa):
    c = _case(pa, "ftn_element")
    y0 = np.random.default_rng(5).uniform(-1, 1, c.n)
    for name in ("K+Kfs", "Kfs", "Rwfs", "Krhs"):
        A = c.op[name]
        r = c.ref(name)
        x = c.input(name)
        xv, yv, zv = A.createVecRight(), A.createVecLeft(), A.createVecLeft()
        xv.setArray(x)
        yv.setArray(y0)
        A.multAdd(xv, yv, zv)
        z = zv.getArray()
        ref = y0.astype(R.LD)[r.rows] + r.y
        err = np.abs(z[r.rows].astype(R.LD) - ref).astype(np.float64)
        assert np.all(err <= r.bound + EPS * np.abs(z[r.rows])), name
        y = c.product(name, x)
        assert A.timeLocalSpmv(xv, zv, reps=3) > 0
        np.testing.assert_array_equal(_bits(zv.getArray()), _bits(y), err_msg=name)
    src = np.random.default_rng(6).uniform(-1, 1, c.n)
    for name in OPS:
        A = c.op[name]
        sv, dv = A.createVecLeft(), A.createVecLeft()
        sv.setArray(src)
        dv.setArray(y0)
        A.copyDirichletRows(sv, dv)
        ident = c.rows(SPECS[name]["ident"])
        np.testing.assert_array_equal(_bits(dv.getArray()), _bits(np.where(ident, src, y0)), err_msg=name)


def test_spmv_bytes_count_the_class_table_and_the_passes(pa):
    c = _case(pa, "ftn_element")
    E, nn = c.conn.shape
    dim, ngl = c.dim, c.ngl
    nq = ngl ** dim + (ngl - 1) ** dim
    elem = 4 * E * nn + 8 * E * nq * (1 + dim * dim) + 8 * 4 * ngl * ngl + 8 * c.n + 2 * 8 * E * nn * dim
    rest = 4 * (c.mesh.N + 1) + 4 * E * nn + c.n + 8 * c.n  # incidence list, class bytes, y
    got = {k: c.op[k].getInfo()["spmv_bytes"] for k in OPS}
    assert got["K"] == elem + E * nn + rest
    assert got["Kfs"] == 2 * (elem + E * nn) + rest
    assert got["Rw"] == elem + rest  # (3-D: the vorticity has the velocity's length; no class table)
    fs = pa.Domain()
    fs.configure({"domain": _domain_cfg(SHAPES["ftn_element"], "ftn_element"),
                  "boundary-conditions": {"custom-func": {"name": "taylor_green3d"}}})
    fs.setUp()
    kfs = pa.petsc.Mat.createKLESumFactored(fs.getMesh(), "K")
    # against the free-slip K of the same mesh: the class table, and a class byte per DoF for a flag per node
    assert got["K"] - kfs.getInfo()["spmv_bytes"] == E * nn + c.n - c.mesh.N


def test_box_equals_element_operator(pa):
    """Kind 0 through the new creator: beside the reference, every product lies
    inside the sum of both operators' bounds of Mat.createNSElement's
    (tests/test_gpu_ns_elem.py: n eps B_i + delta Mmax X_i around the assembled
    product, n = the element matrix's columns + 8; Kfs's T rows eps |x_i| more)."""
    from pynama_amd._lib import call
    c = _case(pa, "box")
    dim, dw, mesh = c.dim, c.dw, c.mesh
    nn = c.ngl ** dim
    nd, ncw = dim * nn, dw * nn
    ctx = pa.get_ctx()
    Ke, Rwe = np.zeros((nd, nd)), np.zeros((nd, ncw))
    call("kle_element_kle", ctx.h, mesh._h, 0, Ke, Rwe)
    K0, R0 = Ke.copy(), Rwe.copy()
    dK = dR = 0.0
    for e in range(1, mesh.E):
        call("kle_element_kle", ctx.h, mesh._h, e, Ke, Rwe)
        dK = max(dK, np.abs(Ke - K0).max() / np.abs(K0).max())
        dR = max(dR, np.abs(Rwe - R0).max() / np.abs(R0).max())
    assert dK <= 2e-12 and dR <= 2e-12
    gd, gw = _gdof(c.conn, dim), _gdof(c.conn, dw)
    for name in OPS:
        S = SPECS[name]
        rw = name in SN.RW
        M0, g, delta = (R0, gw, dR) if rw else (K0, gd, dK)
        x = c.input(name)
        B, X = np.zeros(c.n), np.zeros(c.n)
        for cols, rows in S["passes"]:
            xe = np.abs(x)[g]
            if cols is not None:
                xe = np.where(SN.isin(c.cls[g], cols), xe, 0.0)
            take = SN.isin(c.cls[gd], rows)
            np.add.at(B, gd, np.where(take, xe @ np.abs(M0).T, 0.0))
            np.add.at(X, gd, np.where(take, xe.sum(axis=1)[:, None], 0.0))
        ebound = (M0.shape[1] + 8) * EPS * B + delta * np.abs(M0).max() * X
        if "minus_x" in S:
            ebound = ebound + np.where(c.rows(S["minus_x"]), EPS * np.abs(x), 0.0)
        A = pa.petsc.Mat.createNSElement(mesh, name)
        xv = A.createVecRight()
        xv.setArray(x)
        ye = (A * xv).getArray()
        y = c.product(name, x)
        r = c.ref(name)
        s = r.summed
        w, at = R.worst(y[s], ye.astype(R.LD)[s], (r.bound + r.abound + ebound)[s])
        print(f"box {name}: sum-factorised vs dense-GEMM element operator, err / (sum of bounds) {w:.3g}")
        assert w <= 1.0, (name, w, at)
        np.testing.assert_array_equal(_bits(y[~s]), _bits(ye[~s]), err_msg=name)


def _free_bytes(pa):
    """Free device memory as the HIP runtime the library itself is linked to
    sees it: the symbol is looked up through libkle's own handle (a bare
    "libamdhip64.so" may name another copy of the runtime in the process,
    which has not opened the device)."""
    f, t = C.c_size_t(), C.c_size_t()
    rc = C.CDLL(pa._lib.LIBPATH).hipMemGetInfo(C.byref(f), C.byref(t))
    assert rc == 0, f"hipMemGetInfo: hipError {rc}"
    return f.value


def test_seven_operators_share_one_geometry_set(pa):
    """perturbed_box(3, [8, 8, 8]), ngl 5: a geometry set is 8 E (5^3 + 4^3) 10
    bytes = 7.7 MB, an operator's own tables (connectivity, incidence, class
    table, result arrays: Kfs two) about a third of that.  The first operator
    brings the set; the six after it together hold their own tables, about 1.9
    sets' worth, where private sets would make it 7.9: below 3."""
    spec = dict(pbox=(3, [8, 8, 8], 5), dim=3, ngl=5, walls=SIX)
    dom = _domain(pa, spec, "share_888")
    mesh = dom.getMesh()
    E, ngl = mesh.E, 5
    geo = 8 * E * (ngl ** 3 + (ngl - 1) ** 3) * 10
    Mat = pa.petsc.Mat
    m0 = _free_bytes(pa)
    first = Mat.createNSSumFactored(mesh, "K")
    m1 = _free_bytes(pa)
    rest = [Mat.createNSSumFactored(mesh, k) for k in OPS[1:]]
    m2 = _free_bytes(pa)
    print(f"geometry set {geo} B; first operator holds {m0 - m1} B, the six after it {m1 - m2} B")
    assert m0 - m1 >= geo
    assert m1 - m2 < 3 * geo
    # the shared set outlives its first holder
    x = np.random.default_rng(2).uniform(-1, 1, mesh.N * 3)
    xv = rest[-1].createVecRight()
    xv.setArray(x)
    y = (rest[-1] * xv).getArray()
    first.destroy()
    np.testing.assert_array_equal(_bits((rest[-1] * xv).getArray()), _bits(y))


# ------------------------------------------------------------------ 4. solves
@pytest.mark.parametrize("pc", ["none", "jacobi"])
@pytest.mark.parametrize("variant", ["cg", "sr", "pipecg", "gmres"])
@pytest.mark.parametrize("name", ["K", "K+Kfs"])
def test_krylov_types_converge(pa, name, variant, pc):
    c = _case(pa, "ftn_element")
    rtol = 1e-10
    xt = c.asm[name].createVecRight()
    xt.setArray(np.random.default_rng(9).uniform(-1, 1, c.n))
    b = c.asm[name] * xt
    A = c.op[name]
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
    res = np.linalg.norm(bh.astype(R.LD) - SF.csr_mult(c.csr[name], u.getArray()))
    print(f"{name} {variant} / {pc}: {ksp.getIterationNumber()} iterations, true residual "
          f"{float(res / np.linalg.norm(bh)):.2e}")
    assert res <= 10 * rtol * np.linalg.norm(bh)


def _vec_to_ours(v, mp, bs):
    return np.asarray(v).reshape(-1, bs)[mp].ravel()


def _build_sumfac(pa, dom, how):
    from pynama_amd.petsc import Options
    mat = pa.MatNS()
    mat.setDomain(dom)
    if how == "keyword":
        mat.build(nsType="sumfac", opType="sumfac")
    else:
        opts = Options()
        opts.setValue("kle_ns_type", "sumfac")
        opts.setValue("kle_op_type", "sumfac")
        try:
            mat.build()
        finally:
            opts.delValue("kle_ns_type")
            opts.delValue("kle_op_type")
    return mat


def _nothing_assembled(mat):
    op = mat.getOperators()
    for m in (mat.K, mat.Krhs, mat.Rw, mat.Kfs, mat.Krhsfs, mat.Rwfs, mat.getKplusKfs(), op.Curl, op.SrT, op.DivSrT):
        assert m.getFormat() == "elem" and m.getInfo()["nz_used"] == 0, m.getName()
    assert [m.getName() for m in mat.kle] == ["K", "Krhs", "Rw", "Rd", "Kfs", "Krhsfs", "Rwfs", "Rdfs"]
    assert mat.Rd.getInfo()["nz_used"] == 0 and mat.Rdfs.getInfo()["nz_used"] == 0
    assert "k_sumfac_gather_cls" in mat.getKplusKfs().spmvKernel()


@pytest.mark.parametrize("case,shape,how", [("gmsh2d_ns", "msh2d_gauss", "keyword"), ("umesh3d_ns", "umesh3d", "option")])
def test_solvefs_and_solve_match_golden(pa, case, shape, how):
    """MatNS.build(nsType="sumfac", opType="sumfac") on the golden no-slip Gmsh
    cases: solveFS and solve at rtol 1e-13 within 1e-9 relative of the golden
    velFS and u (the tolerances of test_gpu_umesh.py::test_umesh_noslip_matches_golden)."""
    g = np.load(os.path.join(G, f"case_{case}.npz"))
    c = _case(pa, shape)
    dim, dw = c.dim, c.dw
    assert int(g["ngl"]) == c.ngl
    mat = _build_sumfac(pa, c.dom, how)
    _nothing_assembled(mat)
    mp = O.node_map(c.dom.getFullCoordArray().reshape(-1, dim), g["coords"])
    sol = pa.KleSolver()
    sol.setMat(mat)
    sol.setUp()
    assert sol.isNS() and sol.solverFS.getOperators()[0] is mat.getKplusKfs()
    sol.getKSP().setTolerances(rtol=1e-13)
    sol.solverFS.setTolerances(rtol=1e-13)
    vort = mat.Rw.createVecRight()
    vort.setArray(_vec_to_ours(g["vort0"], mp, dw))
    vel = sol.getSolution()
    vel0 = _vec_to_ours(g["vel0"], mp, dim)
    vel.setArray(vel0)
    sol.solveFS(vort)
    assert sol.solverFS.getConvergedReason() > 0
    vfs = sol.getFreeSlipSolution().getArray()
    rfs = _vec_to_ours(g["velFS"], mp, dim)
    print(f"{case}: solveFS {sol.solverFS.getIterationNumber()} iterations, "
          f"|velFS - golden| {np.linalg.norm(vfs - rfs):.2e} (|golden| {np.linalg.norm(rfs):.2e})")
    assert np.linalg.norm(vfs - rfs) <= 1e-9 * np.linalg.norm(rfs)
    nrows = c.rows({N})
    np.testing.assert_array_equal(_bits(vfs[nrows]), _bits(vel0[nrows]))
    sol.solve(vort)
    assert sol.getKSP().getConvergedReason() > 0
    u = vel.getArray()
    ru = _vec_to_ours(g["u"], mp, dim)
    print(f"{case}: solve {sol.getKSP().getIterationNumber()} iterations, "
          f"rel. diff {np.linalg.norm(u - ru) / max(1.0, np.linalg.norm(ru)):.2e}")
    assert np.linalg.norm(u - ru) <= 1e-9 * max(1.0, np.linalg.norm(ru))
    wall = c.rows({T, N})
    np.testing.assert_array_equal(_bits(u[wall]), _bits(vel0[wall]))


def test_eval_rhs_noslip_gmsh_nothing_assembled(pa):
    """BaseProblem on the no-slip test.msh with -kle_ns_type sumfac -kle_op_type
    sumfac: nothing is assembled, and one evalRHS agrees with the assembled
    build of the same mesh to 1e-9."""
    from pynama_amd.petsc import Options
    g = np.load(os.path.join(G, "case_gmsh2d_ns.npz"))
    cfg = {"name": "gmsh2d_ns", "material-properties": {"rho": float(g["rho"]), "mu": float(g["mu"])},
           "domain": {"ngl": 3, "gmsh-file": MSH}, "boundary-conditions": {"no-slip": {"down": [1, 0]}},
           "initial-conditions": {"velocity": [0, 0]}}
    out = {}
    for form in ("assembled", "sumfac"):
        opts = Options()
        if form == "sumfac":
            opts.setValue("kle_ns_type", "sumfac")
            opts.setValue("kle_op_type", "sumfac")
        try:
            prob = pa.BaseProblem(cfg)
            prob.setUp()
            prob.setUpSolver()
        finally:
            opts.delValue("kle_ns_type")
            opts.delValue("kle_op_type")
        if form == "sumfac":
            _nothing_assembled(prob.mat)
        else:
            assert prob.mat.K.getFormat() == "nb"
        dim = 2
        mp = O.node_map(prob.dom.getFullCoordArray().reshape(-1, dim), g["coords"])
        sol = prob.solverKLE
        sol.getKSP().setTolerances(rtol=1e-13)
        sol.solverFS.setTolerances(rtol=1e-13)
        sol.getSolution().setArray(_vec_to_ours(g["vel0"], mp, dim))
        prob.vort.setArray(_vec_to_ours(g["rhs_vort_in"], mp, 1))
        f = prob.operator.Curl.createVecLeft()
        prob.evalRHS(None, float(g["rhs_t"]), prob.vort, f)
        out[form] = dict(velFS=sol.getFreeSlipSolution().getArray().copy(), vort=prob.vort.getArray().copy(),
                         vel=sol.getSolution().getArray().copy(), f=f.getArray().copy())
    for k, a in out["assembled"].items():
        d = np.linalg.norm(out["sumfac"][k] - a) / max(1.0, np.linalg.norm(a))
        print(f"evalRHS {k}: |sumfac - assembled| / max(1, |assembled|) = {d:.2e}")
    for k, a in out["assembled"].items():
        assert np.linalg.norm(a) > 0, k
        assert np.linalg.norm(out["sumfac"][k] - a) <= 1e-9 * max(1.0, np.linalg.norm(a)), k


# --------------------------------------------------------------- 5. refusals
def _refused(pa, fn, code=56):
    with pytest.raises(pa.Error) as ei:
        fn()
    assert ei.value.ierr == code, ei.value


def test_refusals(pa):
    from pynama_amd._lib import call
    from pynama_amd.mesh import UnstructuredMesh
    from pynama_amd.petsc import KSP, Mat
    c = _case(pa, "msh2d_gauss")
    mesh = c.mesh
    # a free-slip mesh (Gmsh and box), a 2-rank mesh on a one-rank context
    _refused(pa, lambda: Mat.createNSSumFactored(UnstructuredMesh.from_gmsh(MSH, 3), "K"))
    fs = pa.Domain()
    fs.configure({"domain": {"ngl": 3, "box-mesh": {"nelem": [2, 2], "lower": [0, 0], "upper": [1, 1]}},
                  "boundary-conditions": {"uniform": {"velocity": [1.0, -0.5]}}})
    fs.setUp()
    _refused(pa, lambda: Mat.createNSSumFactored(fs.getMesh(), "K"))
    two = pa.BoxMesh(2, [4, 4], [0, 0], [1, 1], 3, rank=0, nranks=2)
    two.set_noslip_faces(["up", "down", "left", "right"])
    _refused(pa, lambda: Mat.createNSSumFactored(two, "K"))
    # a bad which: by name, and at the C ABI
    _refused(pa, lambda: Mat.createNSSumFactored(mesh, "Rd"), 62)
    _refused(pa, lambda: Mat.createNSSumFactored(mesh, 0), 62)
    h = C.c_void_p()
    for bad in (-1, 7):
        _refused(pa, lambda: call("kle_mat_create_ns_sumfac", pa.get_ctx().h, mesh._h, bad, C.byref(h)), 62)
        assert not h.value
    # the other switches keep refusing: the element-wise form on a Gmsh mesh, the free-slip forms on MatNS
    ns = pa.MatNS()
    ns.setDomain(c.dom)
    _refused(pa, lambda: ns.build(buildOperators=False, nsType="element"))
    _refused(pa, lambda: ns.build(buildOperators=False, kleType="sumfac"))
    _refused(pa, lambda: ns.build(buildOperators=False, nsType="matrixfree"), 62)
    _refused(pa, lambda: Mat.createKLESumFactored(mesh, "K"))
    _refused(pa, lambda: Mat.createRwSumFactored(mesh))
    # stored-value calls
    A = c.op["K+Kfs"]
    v = A.createVecLeft()
    _refused(pa, A.getValuesCSR)
    _refused(pa, A.convert)
    _refused(pa, lambda: A.setOption(A.Option.SPD, True))
    _refused(pa, lambda: A.getRow(0))
    _refused(pa, lambda: A.duplicate(copy=True))
    _refused(pa, lambda: A.diagonalScale(v))
    _refused(pa, A.assemble)
    # the 2-D Rwfs is rectangular; y aliasing x
    with pytest.raises(pa.Error):
        KSP().create().setOperators(c.op["Rwfs"])
    xv = A.createVecRight()
    xv.setArray(c.x)
    with pytest.raises(pa.Error):
        A.mult(xv, xv)
    # every operator still multiplies within the bound
    for name in OPS:
        _check_product(c, name, c.product(name, c.input(name)), "after refusals")
