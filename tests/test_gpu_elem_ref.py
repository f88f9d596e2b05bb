"""Device element matrices entry by entry against the longdouble reference
(tests/elem_ref.py): K_e and Rw_e of k_geometry + k_element_mfma (default,
and the 2-wave instantiation) and k_element (VALU) through kle_element_kle,
Curl_e / SrT_e / DivSrT_e / c_e of k_ops_element through kle_element_ops,
Rd through the assembled no-slip Rd, and the assembled K, Krhs, Rw, Curl,
SrT, DivSrT of MatFS.build() against the scatter-added reference.

Every entry must satisfy |device - ref| <= 1.01 u (C S + P) with the count C
of the kernel that produced it (elem_ref's docstring); entries whose bound is
0 (exact zeros of the formula) must be exactly 0.  Each test prints one
ELEMREF line with the worst err / bound and where it occurs.

Reference build on the development host (one element, values + S + P): all
rows 0.2 s at 3-D ngl 5, 0.8 s at ngl 6, 6 s at ngl 7, 32 s at ngl 8.  Every
row is compared up to 3-D ngl 7; at 3-D ngl 8 alone the row subset of
elem_ref.tile_rows (first and last row of every 16-row sub-tile, ne - 1, 16
random rows; all columns): 4.8 s.  References are built once per (dim, ngl,
element geometry) and shared by the kernels."""
import os

import numpy as np
import pytest

import elem_ref as R

pytestmark = pytest.mark.gpu

LOWER, STEP = [-1.5, 0.25, 10.0], [0.7, 0.05, 1.0]
KERNELS = {"mfma": ("mfma", {}), "waves2": ("mfma", {"KLE_ELEMENT_WAVES": "2"}),
           "valu": ("valu", {"KLE_ELEMENT_VALU": "1"})}
ORDERS = [(d, n) for d in (2, 3) for n in range(2, 9)]
OPS_ORDERS = [(2, n) for n in range(2, 9)] + [(3, n) for n in (2, 4, 5, 7, 8)]
GUARD = 64
_REF, _OPS = {}, {}


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


def _ref(dim, ngl, X):
    key = (dim, ngl, np.asarray(X, np.float64).tobytes())
    if key not in _REF:
        rows = R.compare_rows(dim, ngl)
        _REF[key] = (R.ref_kle(dim, ngl, X, rows), R.abs_kle(dim, ngl, X, rows), R.prop_kle(dim, ngl, X, rows))
    return _REF[key]


def _ref_ops(dim, ngl, X):
    key = (dim, ngl, np.asarray(X, np.float64).tobytes())
    if key not in _OPS:
        _OPS[key] = R.ref_ops(dim, ngl, X)
    return _OPS[key]


def _box(pa, dim, ngl):
    nel = [3, 1, 2] if dim == 3 else [3, 2]
    lo = LOWER[:dim]
    hi = [a + n * h for a, n, h in zip(lo, nel, STEP)]
    return pa.BoxMesh(dim, nel, lo, hi, ngl)


def _gmsh(pa, dim, ngl, tmp_path, nel=(2, 2, 1)):
    from pynama_amd.meshgen import perturbed_box, write_gmsh
    V, Cc, F, T = perturbed_box(dim, list(nel)[:dim], seed=13)
    path = str(tmp_path / "p.msh")
    write_gmsh(path, dim, V, Cc, F, T)
    from pynama_amd.mesh import UnstructuredMesh
    return UnstructuredMesh.from_gmsh(path, ngl)


def _mesh_and_elements(pa, which, dim, ngl, tmp_path):
    if which == "box":
        mesh = _box(pa, dim, ngl)
        E = mesh.elem_range[1] - mesh.elem_range[0]
        return mesh, [0, E // 2, E - 1]  # blockIdx.z stride: first, interior, batch end
    # perturbed_box moves interior vertices only: [2,2,1] has none in 3-D
    # (rotated and shuffled cells with constant Jacobians), [2,2,2] has one
    mesh = _gmsh(pa, dim, ngl, tmp_path, (2, 2, 2) if which == "gmsh222" else (2, 2, 1))
    return mesh, list(range(mesh.elem_range[1] - mesh.elem_range[0]))


def _element_kle(pa, mesh, e, env):
    """K_e, Rw_e of element e, written into buffers with guard values past
    their ends.  The guards see only the host side of kle_element_kle (its
    re-layout loop): the kernels write to internal device buffers, where a
    write beyond ne would land in the next (l, m) block or the next element.
    That is what the entrywise comparison of all columns on elements 0,
    interior and last is for."""
    from pynama_amd._lib import call
    dim, n = mesh.dim, mesh.nn
    dw = 1 if dim == 2 else 3
    nk, nr = (dim * n) ** 2, dim * n * dw * n
    kb, rb = np.full(nk + GUARD, -7.25), np.full(nr + GUARD, -7.25)
    old = {k: os.environ.get(k) for k in ("KLE_ELEMENT_VALU", "KLE_ELEMENT_WAVES")}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        call("kle_element_kle", pa.get_ctx().h, mesh._h, e, kb[:nk], rb[:nr])
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert (kb[nk:] == -7.25).all() and (rb[nr:] == -7.25).all(), "host copy wrote past its arrays"
    assert np.isfinite(kb[:nk]).all() and np.isfinite(rb[:nr]).all()
    return kb[:nk].reshape(dim * n, dim * n), rb[:nr].reshape(dim * n, dw * n)


DISTORTED = [(3, n, "gmsh222") for n in (3, 4, 5)]  # non-constant Jacobians in 3-D, every element


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("dim,ngl,which", [(d, n, w) for d, n in ORDERS for w in ("box", "gmsh")] + DISTORTED)
def test_element_matrices(pa, dim, ngl, which, kernel, tmp_path):
    """K_e and Rw_e entrywise inside the bound on the anisotropic offset box
    mesh [3,1,2] / [3,2] (elements 0, interior, last) and on every element of
    a Gmsh mesh written from perturbed_box [2,2,1] / [2,2] (and [2,2,2] at
    3-D ngl 3, 4, 5: distorted hexes); K_e = K_e^T to the
    rounding of the two evaluations (block (l, m) scales the l side by c_q,
    block (m, l) the m side: the same exact terms, C roundings each, hence
    |K_e - K_e^T| <= 1.01 u C (S + S^T) -- see sym_elem_entry); the host
    copy stays inside its arrays (_element_kle)."""
    count, env = KERNELS[kernel]
    mesh, elems = _mesh_and_elements(pa, which, dim, ngl, tmp_path)
    corners = mesh.corners()
    rows = R.compare_rows(dim, ngl)
    rsel = slice(None) if rows is None else R.dof(rows, dim)
    ck = R.C(dim, ngl, count)[0]
    worst = (0.0, None)
    for e in elems:
        Ke, Rwe = _element_kle(pa, mesh, e, env)
        ref, S, P = _ref(dim, ngl, corners[e])
        bnd = R.bound_from(S, P, dim, ngl, count)
        for nm, dev, r, b in (("K", Ke, ref[0], bnd[0]), ("Rw", Rwe, ref[1], bnd[1])):
            w, at = R.worst(dev[rsel], r, b)
            if w > worst[0]:
                worst = (w, (nm, e) + at)
            assert w <= 1, (nm, e, w, at)
        Ks = Ke[rsel][:, rsel]
        Ss = S[0][:, rsel]
        assert (np.abs(Ks - Ks.T) <= 1.01 * R.U * ck * (Ss + Ss.T)).all(), e
    print(f"ELEMREF elem {dim}d ngl {ngl} {which} {kernel}: worst err/bound {worst[0]:.3g} at {worst[1]}")


@pytest.mark.parametrize("dim,ngl,which", [(d, n, w) for d, n in OPS_ORDERS for w in ("box", "gmsh")] + DISTORTED)
def test_collocation_blocks(pa, dim, ngl, which, tmp_path):
    """Curl_e, SrT_e, DivSrT_e and c_e of kle_element_ops entrywise inside
    their bounds; entries that are exactly zero in the formula (dN/dxi is
    nonzero only along grid lines, and the blocks' own zero pattern) are
    exactly zero on the device."""
    from pynama_amd._lib import call
    mesh, elems = _mesh_and_elements(pa, which, dim, ngl, tmp_path)
    corners = mesh.corners()
    n = mesh.nn
    dw, ds = (1, 3) if dim == 2 else (3, 6)
    line = R.ops_line_mask(dim, ngl)
    worst = (0.0, None)
    for e in elems:
        out = {"Curl": np.full((dw * n, dim * n), np.nan), "SrT": np.full((ds * n, dim * n), np.nan),
               "DivSrT": np.full((dim * n, ds * n), np.nan), "c": np.full(n, np.nan)}
        call("kle_element_ops", pa.get_ctx().h, mesh._h, e, out["Curl"], out["SrT"], out["DivSrT"], out["c"])
        ref, bnd = _ref_ops(dim, ngl, corners[e])
        for nm in out:
            assert np.isfinite(out[nm]).all()
            w, at = R.worst(out[nm], ref[nm], bnd[nm])
            if w > worst[0]:
                worst = (w, (nm, e) + at)
            assert w <= 1, (nm, e, w, at)
            assert not out[nm][bnd[nm] == 0].any(), (nm, e)
        # off the grid lines the bound is 0: the claim above struct OpsOut
        for nm, r, c in (("Curl", dw, dim), ("SrT", ds, dim), ("DivSrT", dim, ds)):
            off = np.kron(~line, np.ones((r, c), bool))
            assert (bnd[nm][off] == 0).all() and not out[nm][off].any(), (nm, e)
    print(f"ELEMREF ops {dim}d ngl {ngl} {which}: worst err/bound {worst[0]:.3g} at {worst[1]}")


def _check_csr(A, ref, name):
    v, b, pat = ref
    ip, ix, d = A.getValuesCSR()
    rp, rx, rv = R.csr_of(v, pat)
    np.testing.assert_array_equal(ip, rp, err_msg=name)
    np.testing.assert_array_equal(ix, rx, err_msg=name)
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    w, at = R.worst(d, rv, b[rows, ix])
    assert w <= 1, (name, w, (int(rows[at[0]]), int(ix[at[0]])))
    return w, (name, int(rows[at[0]]), int(ix[at[0]])) if len(d) else (name,)


ASSEMBLED = {
    "box222_ngl3": (3, 3, {"box-mesh": {"nelem": [2, 2, 2], "lower": [0, 0, 0], "upper": [1, 1, 1]}}, None),
    "box211_ngl7": (3, 7, {"box-mesh": {"nelem": [2, 1, 1], "lower": [0, 0, 0], "upper": [1, 1, 1]}}, None),
    "box32_ngl8": (2, 8, {"box-mesh": {"nelem": [3, 2], "lower": LOWER[:2],
                                       "upper": [LOWER[0] + 3 * STEP[0], LOWER[1] + 2 * STEP[1]]}}, None),
    "perturbed221_ngl4": (3, 4, "gmsh", None),
    "box232_ngl3_left_down": (3, 3, {"box-mesh": {"nelem": [2, 3, 2], "lower": [0, 0, 0], "upper": [1, 1, 1]}},
                              ["left", "down"]),
}


@pytest.mark.parametrize("case", list(ASSEMBLED))
def test_assembled_matrices(pa, case, tmp_path):
    """K, Krhs, Rw, Curl, SrT, DivSrT of MatFS.build(): patterns exactly the
    reference's, values entrywise within the scattered element bounds plus
    one rounding per incident element (and the 1 / W_n scaling of the
    operators); K == K^T bit for bit."""
    import scipy.sparse as sp
    dim, ngl, dom_cfg, faces = ASSEMBLED[case]
    if dom_cfg == "gmsh":
        from pynama_amd.meshgen import perturbed_box, write_gmsh
        V, Cc, F, T = perturbed_box(dim, [2, 2, 1], seed=13)
        path = str(tmp_path / "p.msh")
        write_gmsh(path, dim, V, Cc, F, T)
        dom_cfg = {"gmsh-file": path}
    cfg = {"domain": dict(ngl=ngl, **dom_cfg),
           "boundary-conditions": {"custom-func": {"name": "taylor_green3d" if dim == 3 else "taylor_green"}}}
    dom = pa.Domain()
    dom.configure(cfg)
    dom.setUp()
    mesh = dom.getMesh()
    dirn = np.asarray(sorted(dom.getNodesDirichlet()), dtype=np.int64)
    if faces is not None:
        dirn = mesh.face_nodes(faces)
        mesh.set_dirichlet_nodes(dirn)
    flag = np.zeros(mesh.N, bool)
    flag[dirn] = True
    mat = pa.MatFS()
    mat.setDomain(dom)
    mat.build()
    ref = R.assemble_ref(dim, ngl, mesh.conn(), mesh.corners(), flag)
    op = mat.getOperators()
    worst = (0.0, None)
    for nm, A in (("K", mat.K), ("Krhs", mat.Krhs), ("Rw", mat.Rw), ("Curl", op.Curl), ("SrT", op.SrT),
                  ("DivSrT", op.DivSrT)):
        w, at = _check_csr(A, ref[nm], nm)
        if w > worst[0]:
            worst = (w, at)
    ip, ix, d = mat.K.getValuesCSR()
    K = sp.csr_matrix((d, ix, ip), shape=(len(ip) - 1,) * 2)
    KT = K.T.tocsr()
    KT.sort_indices()
    assert np.array_equal(KT.indptr, ip) and np.array_equal(KT.indices, ix) and np.array_equal(KT.data, d)
    print(f"ELEMREF assembled {case}: worst err/bound {worst[0]:.3g} at {worst[1]}")


def test_rd_through_noslip_assembly(pa):
    """Rd_e has no export of its own: the assembled Rd of a tiny no-slip case
    (box [2,1,1], ngl 3, one wall) is the scatter of Rd_e over the rows of
    the nodes off the wall -- pattern exact, values inside the bound."""
    cfg = {"domain": {"ngl": 3, "box-mesh": {"nelem": [2, 1, 1], "lower": LOWER, "upper": [
        LOWER[0] + 2 * STEP[0], LOWER[1] + STEP[1], LOWER[2] + STEP[2]]}},
        "boundary-conditions": {"no-slip": {"down": [0, 0, 0]}}}
    dom = pa.Domain()
    dom.configure(cfg)
    dom.setUp()
    mat = pa.MatNS()
    mat.setDomain(dom)
    mat.build()
    mesh = dom.getMesh()
    flag = np.zeros(mesh.N, bool)
    flag[mesh.face_nodes(["down"])] = True
    ref = R.assemble_ref(3, 3, mesh.conn(), mesh.corners(), flag, ops=False)
    w, at = _check_csr(mat.Rd, ref["Rd"], "Rd")
    assert mat.Rd.getInfo()["nz_used"] > 0
    print(f"ELEMREF Rd no-slip [2,1,1] ngl 3: worst err/bound {w:.3g} at {at}")
