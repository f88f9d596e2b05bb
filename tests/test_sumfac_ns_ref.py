"""The reference of the sum-factorised no-slip operators
(tests/sumfac_ns_ref.py) checks itself, and the host side of the new entry
point: no GPU.

1. On the golden no-slip Gmsh cases (case_gmsh2d_ns, case_umesh3d_ns) the
   mesh-level reference of every operator equals the product of the golden
   assembled matrix inside bound + assembled bound (the fixtures come from the
   reference code's running sum: the assembled bound at elem_ref.C "oracle").
   K+Kfs has no fixture of its own: K x + Kfs x in longdouble is its product.
2. The bounds are not vacuous: each planted error -- a wrong class on one DoF,
   Kfs's passes swapped, a missing -x_i, a dropped incidence entry, a sign
   error on Krhsfs -- leaves the bound on at least one row.
3. The C ABI export, the option parsing and the null-argument refusal."""
import ctypes as C
import os

import numpy as np
import pytest

import elem_ref as R
import ns_ref as NS
import sumfac_ns_ref as SN
import sumfac_ref as SF
from oracle import oracle as O

G = os.path.join(os.path.dirname(__file__), "golden")
LD = R.LD
F, T, N = SN.F, SN.T, SN.N


def _golden_mesh(case, tmp_path):
    """The host mesh of a golden no-slip case in our numbering: conn, corners,
    classes (from the fixture's DoF sets) and the node map to the fixture."""
    from pynama_amd.mesh import UnstructuredMesh
    from pynama_amd.meshgen import write_gmsh
    g = np.load(os.path.join(G, f"case_{case}.npz"))
    dim, ngl = int(g["dim"]), int(g["ngl"])
    path = os.path.join(G, "test.msh")
    if "mesh_cells" in g:
        path = str(tmp_path / "mesh.msh")
        write_gmsh(path, dim, g["mesh_vertices"], g["mesh_cells"], g["mesh_facets"], g["mesh_tags"])
    m = UnstructuredMesh.from_gmsh(path, ngl)
    mp = O.node_map(m.coords(), g["coords"])  # our node -> the fixture's
    cf = np.zeros(m.N * dim, np.int64)
    cf[g["tang_dofs"]] = T
    cf[g["normal_dofs"]] = N  # normal wins (mat_ns.py:60-62)
    cls = cf[R.dof(mp, dim)]
    return g, dim, ngl, m.conn(), m.corners(), cls, mp


@pytest.mark.parametrize("case", ["gmsh2d_ns", "umesh3d_ns"])
def test_mesh_references_equal_golden_assembled_products(case, tmp_path):
    g, dim, ngl, conn, corners, cls, mp = _golden_mesh(case, tmp_path)
    dw = 1 if dim == 2 else 3
    Nn = len(cls) // dim
    assert (cls == F).any() and (cls == T).any() and (cls == N).any()
    if case == "gmsh2d_ns":
        assert {3, 5} <= set(np.unique(SF.incidence(conn, Nn))), "the fixture has nodes of valence 3 and 5"
    rng = np.random.default_rng(11)
    x, w = rng.uniform(-1, 1, Nn * dim), rng.uniform(-1, 1, Nn * dw)

    def golden(nm, v, cbs):
        vf = np.zeros_like(v)
        vf[R.dof(mp, cbs)] = v
        y = SF.csr_mult((g[nm + "_indptr"], g[nm + "_indices"], g[nm + "_data"]), vf)
        return y[R.dof(mp, dim)]

    for name in SN.OPS:
        rw = name in SN.RW
        v, cbs = (w, dw) if rw else (x, dim)
        ref = SN.reference(dim, ngl, conn, corners, cls, name, v)
        ya = golden("K", v, cbs) + golden("Kfs", v, cbs) if name == "K+Kfs" else golden(name, v, cbs)
        i = 1 if rw else 0
        ratio = max(1.0, R.C(dim, ngl, "oracle")[i] / R.C(dim, ngl, "mfma")[i])
        s = ref.summed
        assert s.any() and np.any(ref.bound[s] > 0)  # (a row no kept column reaches is exactly 0: bound 0)
        wv, at = R.worst(ya.astype(np.float64)[s], ref.y[s], (ref.bound + ref.abound * ratio)[s])
        print(f"{case} {name}: golden product vs mesh reference, err / (bound + assembled bound) {wv:.3g} at {at}")
        assert wv <= 1.0, (name, wv, at)
        # identity rows hold x_i itself, zero rows nothing
        if ref.ident.any():
            np.testing.assert_array_equal(ref.y[ref.ident].astype(np.float64), v[ref.ident])
            np.testing.assert_array_equal(ya[ref.ident].astype(np.float64), v[ref.ident])
        assert np.all(ref.y[ref.zero] == 0) and np.all(ya[ref.zero] == 0)
        if name in ("K", "Kfs"):
            da = SF.csr_diag((g[name + "_indptr"], g[name + "_indices"], g[name + "_data"]))[R.dof(mp, dim)]
            nz = ~ref.zero  # (a zero row stores no diagonal)
            wd, at = R.worst(da[nz], ref.diag[nz], (ref.dbound + ref.adbound * ratio)[nz])
            print(f"{case} {name}: golden diagonal vs reference, err / (bound + assembled bound) {wd:.3g}")
            assert wd <= 1.0, (name, wd, at)


def _planted_mesh(dim):
    """A box whose walls leave F, T and N DoFs, corner rule included."""
    import pynama_amd as pa
    nelem, walls = ([3, 4], ["up", "down", "left"]) if dim == 2 else ([2, 2, 2], ["up", "down", "left"])
    ngl = 3
    m = pa.BoxMesh(dim, nelem, [0] * dim, [1] * dim, ngl)
    conn, corners, coords = m.conn(), m.corners(), m.coords()
    return ngl, conn, corners, NS.classes(coords, walls)


@pytest.mark.parametrize("dim", [2, 3])
def test_bounds_hold_the_rounded_reference_and_catch_planted_errors(dim):
    ngl, conn, corners, cls = _planted_mesh(dim)
    Nn = len(cls) // dim
    dw = 1 if dim == 2 else 3
    rng = np.random.default_rng(3)
    x, w = rng.uniform(-1, 1, Nn * dim), rng.uniform(-1, 1, Nn * dw)
    refs = {nm: SN.reference(dim, ngl, conn, corners, cls, nm, w if nm in SN.RW else x) for nm in SN.OPS}
    for nm, r in refs.items():
        assert np.any(r.bound[r.summed] > 0), nm
        assert R.worst(r.y.astype(np.float64), r.y, r.bound)[0] <= 1.0  # (the longdouble value rounded to fp64)

    def worst(nm, plant):
        v = w if nm in SN.RW else x
        r = SN.reference(dim, ngl, conn, corners, cls, nm, v, plant=plant)
        ref = refs[nm]
        # a planted class moves a row between rules: every row is compared, exact rows with bound 0
        return R.worst(r.y.astype(np.float64), ref.y, ref.bound)[0]

    # a free DoF of an element that also holds T DoFs, and a T DoF
    gd = R.dof(conn[0], dim)
    fdof = int(gd[cls[gd] == F][0])
    tdof = int(np.nonzero(cls == T)[0][0])
    shared = np.nonzero(SF.incidence(conn, Nn) > 1)[0]
    node = int(shared[(cls.reshape(Nn, dim)[shared] == F).all(axis=1)][0])  # a free node of several elements
    e1 = int(np.nonzero((conn == node).any(axis=1))[0][1])
    skip = (e1, int(np.nonzero(conn[e1] == node)[0][0]))
    tnode = int(tdof // dim)
    et = int(np.nonzero((conn == tnode).any(axis=1))[0][0])
    skip_t = (et, int(np.nonzero(conn[et] == tnode)[0][0]))
    cases = []
    for nm in ("K", "Krhs", "Kfs"):
        cases += [(nm, "free DoF classed tangential", {"cls": (fdof, T)}),
                  (nm, "tangential DoF classed free", {"cls": (tdof, F)})]
    # (Krhsfs and K+Kfs treat F and T alike: their table tells N from the rest)
    ndof = int(np.nonzero(cls == N)[0][0])
    for nm in ("Krhsfs", "K+Kfs"):
        cases += [(nm, "normal DoF classed tangential", {"cls": (ndof, T)}),
                  (nm, "tangential DoF classed normal", {"cls": (tdof, N)})]
    cases += [("Rw", "free DoF classed tangential", {"cls": (fdof, T)}),
              ("Rwfs", "tangential DoF classed free", {"cls": (tdof, F)}),
              ("Kfs", "passes swapped", {"swap_kfs": True}),
              ("Kfs", "missing -x_i", {"no_minus_x": True}),
              ("Krhsfs", "sign", {"sign": 1}),
              ("Krhs", "sign", {"sign": 1})]
    cases += [(nm, "dropped incidence entry", {"skip": skip}) for nm in ("K", "Krhs", "Rw", "Krhsfs", "K+Kfs")]
    cases += [(nm, "dropped incidence entry (T row)", {"skip": skip_t}) for nm in ("Kfs", "Rwfs", "K+Kfs")]
    for nm, what, plant in cases:
        wv = worst(nm, plant)
        print(f"dim {dim} {nm}: planted {what}: err/bound {wv:.3g}")
        assert wv > 1.0, (nm, what)


def test_diagonal_rules():
    ngl, conn, corners, cls = _planted_mesh(2)
    x = np.random.default_rng(4).uniform(-1, 1, len(cls))
    rk = SN.reference(2, ngl, conn, corners, cls, "K", x)
    rf = SN.reference(2, ngl, conn, corners, cls, "Kfs", x)
    rs = SN.reference(2, ngl, conn, corners, cls, "K+Kfs", x)
    f, t, n = cls == F, cls == T, cls == N
    assert np.all(rk.diag[t | n] == 1) and np.all(rk.diag[f] > 0)
    assert np.all(rf.diag[n | f] == 0)
    # Kfs's tangential diagonal is the element sums - 1: K+Kfs's - 1
    assert np.all(rs.diag[n] == 1)
    np.testing.assert_array_equal(rf.diag[t], rs.diag[t] - 1)
    np.testing.assert_array_equal(rs.diag[f], rk.diag[f])
    assert np.all(rf.dbound[t] > rs.dbound[t]) and np.all(rs.dbound[f | t] > 0)
    assert not hasattr(SN.reference(2, ngl, conn, corners, cls, "Krhs", x), "diag")


# ------------------------------------------------------------ host surface
@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


def test_new_symbol_is_exported_and_bound(pa):
    lib = C.CDLL(pa._lib.LIBPATH)
    assert hasattr(lib, "kle_mat_create_ns_sumfac")
    assert "kle_mat_create_ns_sumfac" in set(pa._lib.exported_symbols())


def test_null_arguments_are_refused_before_the_device(pa):
    lib = C.CDLL(pa._lib.LIBPATH)
    out = C.c_void_p()
    lib.kle_mat_create_ns_sumfac.restype = C.c_int
    assert lib.kle_mat_create_ns_sumfac(None, None, 0, C.byref(out)) != 0 and not out.value


def test_ns_type_option_values_parse(pa):
    from pynama_amd.matrices import kle_ns_type
    from pynama_amd.petsc import Options
    assert kle_ns_type("sumfac") == "sumfac" and kle_ns_type("element") == "element"
    opts = Options()
    opts.setValue("kle_ns_type", "sumfac")
    try:
        assert kle_ns_type() == "sumfac"
        assert kle_ns_type("assembled") == "assembled"  # the keyword wins
    finally:
        opts.delValue("kle_ns_type")
    assert kle_ns_type() == "assembled"
    for bad in ("matrixfree", "", "Sumfac", "dense", "sumfactorised"):
        with pytest.raises(pa.Error) as ei:
            kle_ns_type(bad)
        assert ei.value.ierr == 62
        assert all(v in str(ei.value) for v in ("assembled", "element", "sumfac"))
    with pytest.raises(pa.Error) as ei:
        pa.petsc.Mat.createNSSumFactored(None, "Rd")
    assert ei.value.ierr == 62
