"""The petsc4py-shaped Mat surface of kle_mat.hip on stored-value matrices
(node-block "nb" and scalar "aij") against the longdouble restatements of
tests/mat_ref.py: mult, multAdd, getDiagonal, getRow, getValuesCSR, convert,
duplicate, diagonalScale, axpy, +, setValues / assemble.

The invariant under test: what a matrix multiplies by is what it exports,
after any operation that changes values.  Every check starts from one export
E0 = A.getValuesCSR() (tied to first principles by test_gpu_elem_ref.py and
test_gpu_ns.py) and is rowwise (products) or entrywise (values) against a
bound counted in roundings (mat_ref's docstring), never a norm; exact where
the operation is a copy.  Each test prints MATREF lines with the worst
err / bound and where it occurs.

Meshes (one rank; node-row block counts in brackets, the chunk / tail edges
of vofs): fs2d_p2 box [3,2] ngl 3 (9/15/25; 2x2, 2x1, 3x2, 2x3 blocks),
fs2d_p3 [2,2] ngl 4 (16/28/49), fs2d_p4 [2,2] ngl 5 (25/45/81), fs2d_p7 [2,2]
ngl 8 (64/120/225), fs3d_p2 [2,2,2] ngl 3 (3x3, 6x3, 3x6), all_dirichlet
[1,1] ngl 2 (every row diagonal-only), partial_dirichlet [2,3,2] ngl 3 with
faces left + down fixed, gmsh3d (perturbed_box(3, [2,2,1], seed 13), ngl 4,
dictionaries built), ns2d (cavity [4,4] ngl 3) and ns3d (six walls, [3,2,2]
ngl 3) with MatNS's DoF masks.  The free-slip and Gmsh cases run under value
layout 0 with row padding 1 and 16 and under layout 1; the no-slip cases
under the default."""
import numpy as np
import pytest

import mat_ref as M
from krylov_ref import Csr, spmv_case

pytestmark = pytest.mark.gpu

LOWER, STEP = [-1.5, 0.25, 10.0], [0.7, 0.05, 1.0]
CAVITY = {"up": [2, 0], "down": [0, 0], "left": [0, 0], "right": [0, 0]}
SIXWALLS = {"up": [1, 0, 0.5], "down": [0, 0, 0], "left": [0, 0, 0], "right": [0, 0, 0], "front": [0, 0, 0],
            "back": [0, 0, 0]}
# case: (kind, dim, nelem, ngl, extra)
CASES = {
    "fs2d_p2": ("fs", 2, [3, 2], 3, None),
    "fs2d_p3": ("fs", 2, [2, 2], 4, None),
    "fs2d_p4": ("fs", 2, [2, 2], 5, None),
    "fs2d_p7": ("fs", 2, [2, 2], 8, None),
    "fs3d_p2": ("fs", 3, [2, 2, 2], 3, None),
    "all_dirichlet": ("fs", 2, [1, 1], 2, None),
    "partial_dirichlet": ("fs", 3, [2, 3, 2], 3, ["left", "down"]),
    "gmsh3d": ("gmsh", 3, [2, 2, 1], 4, None),
    "ns2d": ("ns", 2, [4, 4], 3, CAVITY),
    "ns3d": ("ns", 3, [3, 2, 2], 3, SIXWALLS),
}
LAYOUTS = {"lay0_pad1": (0, 1), "lay0_pad16": (0, 16), "lay1": (1, 16)}
PARAMS = [(c, l) for c, v in CASES.items() if v[0] != "ns" for l in LAYOUTS] + \
         [(c, "default") for c, v in CASES.items() if v[0] == "ns"]
SENTINEL = -7.25
_BUILDS = {}


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


def _build(pa, case, layout, tmp_path_factory):
    """{name: Mat} of one build, made once per (case, layout) and never
    changed: every operation that writes runs on a duplicate."""
    key = (case, layout)
    if key in _BUILDS:
        return _BUILDS[key]
    from pynama_amd.runtime import (get_row_padding, get_tuning, get_value_layout, set_row_padding, set_tuning,
                                    set_value_layout)
    kind, dim, nel, ngl, extra = CASES[case]
    old = (get_value_layout(), get_row_padding(), get_tuning("spmv_dict_min_rows"))
    try:
        if layout != "default":
            set_value_layout(LAYOUTS[layout][0])
            set_row_padding(LAYOUTS[layout][1])
        if kind == "gmsh":
            from pynama_amd.meshgen import perturbed_box, write_gmsh
            set_tuning("spmv_dict_min_rows", 0)
            V, Cc, F, T = perturbed_box(dim, nel, seed=13)
            path = str(tmp_path_factory.mktemp("matref") / "p.msh")
            write_gmsh(path, dim, V, Cc, F, T)
            dom_cfg = {"gmsh-file": path}
        elif kind == "ns":
            dom_cfg = {"box-mesh": {"nelem": nel, "lower": [0] * dim, "upper": [1] * dim}}
        else:
            dom_cfg = {"box-mesh": {"nelem": nel, "lower": LOWER[:dim],
                                    "upper": [a + n * h for a, n, h in zip(LOWER, nel, STEP)]}}
        bc = {"no-slip": extra} if kind == "ns" else \
            {"custom-func": {"name": "taylor_green3d" if dim == 3 else "taylor_green"}}
        dom = pa.Domain()
        dom.configure({"domain": dict(ngl=ngl, **dom_cfg), "boundary-conditions": bc})
        dom.setUp()
        if kind == "ns":
            mat = pa.MatNS()
            mat.setDomain(dom)
            mat.build(buildOperators=False)
            mats = {n: getattr(mat, n) for n in ("K", "Krhs", "Rw", "Rd", "Kfs", "Krhsfs", "Rwfs", "Rdfs")}
            mats["K+Kfs"] = mat.getKplusKfs()
        else:
            if extra is not None:
                mesh = dom.getMesh()
                mesh.set_dirichlet_nodes(mesh.face_nodes(extra))
            mat = pa.MatFS()
            mat.setDomain(dom)
            mat.build()
            op = mat.getOperators()
            mats = {"K": mat.K, "Krhs": mat.Krhs, "Rw": mat.Rw, "Rd": mat.Rd, "Curl": op.Curl, "SrT": op.SrT,
                    "DivSrT": op.DivSrT}
    finally:
        set_value_layout(old[0])
        set_row_padding(old[1])
        set_tuning("spmv_dict_min_rows", old[2])
    _BUILDS[key] = {"mats": mats, "keep": (dom, mat), "E0": {}}
    return _BUILDS[key]


def _export(A):
    ip, ix, d = A.getValuesCSR()
    return Csr(ip, ix, d, A.getSize()[1])


def _e0(build, name):
    if name not in build["E0"]:
        build["E0"][name] = _export(build["mats"][name])
    return build["E0"][name]


def _is_nb(A):
    return A.getFormat() == "nb"


def _mult(A, xa):
    x = A.createVecRight()
    x.setArray(xa)
    y = A.createVecLeft()
    y.set(SENTINEL)  # (a row the kernel does not write stays visible)
    A.mult(x, y)
    return y.getArray()


def _variants(pa, A):
    """Tuning states under which A's product must be bitwise the same:
    (label, structured, {tuning})."""
    out = []
    if not _is_nb(A):
        return out
    if A.isStructured():
        out.append(("streamed", False, {}))
    if A._rbs == 3 and A._cbs == 3 and "k_nb_spmv<3,3,1" in A.spmvKernel():
        for wv in (4, 8):
            for xl in (0, 1):
                out.append((f"waves{wv}_xlds{xl}", True, {"spmv_waves": wv, "spmv_x_lds": xl}))
        out.append(("waves8_nodict", True, {"spmv_waves": 8, "spmv_dict": 0}))
        out.append(("waves8_streamed", False, {"spmv_waves": 8}))
    return out


class _Tuned:
    def __init__(self, A, structured, tune):
        self.A, self.structured, self.tune = A, structured, tune

    def __enter__(self):
        from pynama_amd.runtime import get_tuning, set_tuning
        self.old = {k: get_tuning(k) for k in self.tune}
        self.was = self.A.isStructured() if _is_nb(self.A) else False
        for k, v in self.tune.items():
            set_tuning(k, v)
        if _is_nb(self.A) and self.was:
            self.A.setSpmvStructured(self.structured)

    def __exit__(self, *exc):
        from pynama_amd.runtime import set_tuning
        for k, v in self.old.items():
            set_tuning(k, v)
        if _is_nb(self.A) and self.was:
            self.A.setSpmvStructured(True)


def _product_check(A, E, tag, vectors=None, seed=0):
    """Every row of A x within product()'s bound of the export E, for the
    input classes of mat_ref; returns (worst, where) and the products."""
    worst, prods = (0.0, None), {}
    for nm, xa in (vectors or M.input_vectors(E, C=getattr(A, "_cbs", 1), seed=seed)):
        dev = _mult(A, xa)
        ref, b = M.product(E, xa)
        w, at = M.worst(dev, ref, b)
        assert w <= 1, (tag, nm, w, at, float(dev[at]), float(ref[at]))
        if w >= worst[0]:
            worst = (w, (at[0] if at else None, nm))
        prods[nm] = (xa, dev)
    return worst, prods


def _line(case, layout, name, op, worst):
    print(f"MATREF {case}/{layout} {name} {op}: worst err/bound {worst[0]:.3g} at {worst[1]}")


def _rows_equal(A, E, tag):
    """getRow of every owned row == the CSR slice, columns and values."""
    lo, hi = A.getOwnershipRange()
    assert hi - lo == E.m
    for r in range(E.m):
        cols, vals = A.getRow(lo + r)
        s, e = E.indptr[r], E.indptr[r + 1]
        np.testing.assert_array_equal(cols, E.indices[s:e], err_msg=f"{tag} row {r}")
        np.testing.assert_array_equal(vals, E.data[s:e], err_msg=f"{tag} row {r}")


def _diag_check(pa, A, E, tag):
    if _is_nb(A) and A._rbs != A._cbs:
        with pytest.raises(pa.petsc.Error) as ei:
            A.getDiagonal()
        assert ei.value.ierr == 62, tag
        return
    np.testing.assert_array_equal(A.getDiagonal().getArray(), M.diagonal(E), err_msg=tag)


def _same_pattern(E, F, tag):
    np.testing.assert_array_equal(E.indptr, F.indptr, err_msg=tag)
    np.testing.assert_array_equal(E.indices, F.indices, err_msg=tag)


# ------------------------------------------------------------------- mult
@pytest.mark.parametrize("case,layout", PARAMS)
def test_mult_rowwise(pa, case, layout, tmp_path_factory):
    """mult: every row inside the bound for the five input classes; structured
    and streamed columns, spmv_x_lds 0/1 and spmv_waves 4/8 (and the
    dictionary kernel of the Gmsh K) bitwise the same; multAdd with z distinct
    and with z the Vec y."""
    build = _build(pa, case, layout, tmp_path_factory)
    kernels = set()
    for name, A in build["mats"].items():
        E = _e0(build, name)
        tag = (case, layout, name)
        worst, prods = _product_check(A, E, tag, seed=len(name))
        kernels.add(A.spmvKernel())
        _line(case, layout, name, "mult", worst)
        for label, st, tune in _variants(pa, A):
            with _Tuned(A, st, tune):
                kernels.add(A.spmvKernel())
                for nm, (xa, dev) in prods.items():
                    np.testing.assert_array_equal(_mult(A, xa), dev, err_msg=f"{tag} {label} {nm}")
        wa = (0.0, None)
        for nm in ("uniform", "scales"):
            xa, _ = prods[nm]
            ref, b = M.product(E, xa)
            ya = M.x_uniform(E.m, 77) * (1.0 if nm == "uniform" else 1e3)
            zr, zb = M.mult_add(ref, b, ya)
            x, y, z = A.createVecRight(), A.createVecLeft(), A.createVecLeft()
            x.setArray(xa)
            y.setArray(ya)
            z.set(SENTINEL)
            A.multAdd(x, y, z)
            np.testing.assert_array_equal(y.getArray(), ya)
            for which, got in (("z", z.getArray()), ("z=y", None)):
                if got is None:
                    A.multAdd(x, y, y)
                    got = y.getArray()
                w, at = M.worst(got, zr, zb)
                assert w <= 1, (tag, "multAdd", which, nm, w, at)
                if w >= wa[0]:
                    wa = (w, (at[0] if at else None, nm, which))
        _line(case, layout, name, "multAdd", wa)
    if case == "gmsh3d" and layout == "lay1":
        assert "k_nb_spmv_dict" in kernels, kernels
    if case in ("fs3d_p2", "partial_dirichlet") and layout == "lay1":
        assert "k_nb_spmv_xl<8>" in kernels, kernels


def test_block_counts_cover_chunk_and_tail_edges(pa, tmp_path_factory):
    """The node-row block counts of the free-slip cases' matrices (K drops the
    Dirichlet columns; Rw and the collocation operators keep every node of a
    row's elements: n^2, n (2n - 1), (2n - 1)^2 in 2-D) include the edges of
    the chunked value layout (vofs): below 16, exactly 16, 17-63, exactly 64,
    a single block beyond a multiple of 16, above 128.  If not, the meshes
    were changed and those paths are no longer exercised."""
    counts = set()
    for case in ("fs2d_p2", "fs2d_p3", "fs2d_p4", "fs2d_p7", "fs3d_p2"):
        build = _build(pa, case, "lay1", tmp_path_factory)
        for name, A in build["mats"].items():
            if not _is_nb(A):
                continue
            lens = _e0(build, name).row_lengths()[::A._rbs]
            full = lens[lens % A._cbs == 0] // A._cbs
            assert (lens[lens % A._cbs != 0] == 1).all()  # (diagonal-only rows)
            counts |= {int(v) for v in full}
    print("MATREF block counts:", sorted(counts))
    assert any(c < 16 for c in counts)
    assert 16 in counts and 64 in counts
    assert any(17 <= c <= 63 for c in counts)
    assert any(c > 16 and c % 16 == 1 for c in counts)
    assert any(c > 128 for c in counts)


# --------------------------------------------------- exports and copies
@pytest.mark.parametrize("case,layout", PARAMS)
def test_exports_and_copies(pa, case, layout, tmp_path_factory):
    """getDiagonal == the export's diagonal (error 62 on rectangular blocks);
    getRow of every row == the CSR slice; convert("aij") exports E0 exactly
    and multiplies inside the same bound; duplicate(copy=True) is bitwise A;
    duplicate(copy=False) has E0's pattern, zero values and a zero product,
    also under symmetric storage (3-D box K)."""
    build = _build(pa, case, layout, tmp_path_factory)
    for name, A in build["mats"].items():
        E = _e0(build, name)
        tag = (case, layout, name)
        _diag_check(pa, A, E, tag)
        _rows_equal(A, E, tag)
        vectors = M.input_vectors(E, C=A._cbs, seed=len(name))
        # convert
        B = A.convert("aij")
        assert B.getFormat() == "aij"
        EB = _export(B)
        _same_pattern(E, EB, tag)
        np.testing.assert_array_equal(EB.data, E.data, err_msg=str(tag))
        worst, _ = _product_check(B, E, tag + ("convert",), vectors)
        _line(case, layout, name, "convert.mult", worst)
        np.testing.assert_array_equal(B.getDiagonal().getArray(), M.diagonal(E))
        # duplicate(copy=True)
        D = A.duplicate(copy=True)
        ED = _export(D)
        _same_pattern(E, ED, tag)
        np.testing.assert_array_equal(ED.data, E.data, err_msg=str(tag))
        for nm, xa in vectors[:3]:
            np.testing.assert_array_equal(_mult(D, xa), _mult(A, xa), err_msg=f"{tag} duplicate {nm}")
        _diag_check(pa, D, E, tag)
        # duplicate(copy=False)
        Z = A.duplicate(copy=False)
        sym_states = [False]
        if name == "K" and CASES[case][0] in ("fs", "ns") and CASES[case][1] == 3 and layout in ("lay1", "default"):
            sym_states.append(True)
        for sym in sym_states:
            if sym:
                Z.setOption(Z.Option.SPD, True)
                assert Z.isSymmetricStorage()
            EZ = _export(Z)
            _same_pattern(E, EZ, tag)
            assert not EZ.data.any(), tag
            for nm, xa in vectors[:2]:
                got = _mult(Z, xa)
                assert not got.any(), (tag, "zero duplicate", nm, sym)
        _line(case, layout, name, "export/getRow/duplicate", (0.0, "exact"))


# ---------------------------------------------------------- diagonalScale
def _scale_vectors(E, seed):
    rng = np.random.default_rng(seed)
    L = rng.uniform(0.5, 2.0, E.m) * rng.choice([-1.0, 1.0], E.m)
    R = rng.uniform(0.5, 2.0, E.n) * rng.choice([-1.0, 1.0], E.n)
    if E.m and E.row_lengths().max() > 0:
        r = M.longest_row(E)
        L[r] = 0.0  # one L entry and one R entry exactly 0, on the longest row and one of its columns
        R[E.indices[(E.indptr[r] + E.indptr[r + 1]) // 2]] = 0.0
    else:
        L[0], R[0] = 0.0, 0.0
    return L, R


@pytest.mark.parametrize("case,layout", PARAMS)
def test_diagonal_scale(pa, case, layout, tmp_path_factory):
    """diagonalScale with L only, R only (an A.createVecRight()) and both, on
    copies: the export keeps E0's pattern, every entry is inside scaled()'s
    bound (zeros stay zeros), and the scaled matrix's product, diagonal and
    rows agree with its own new export."""
    build = _build(pa, case, layout, tmp_path_factory)
    for name, A in build["mats"].items():
        E = _e0(build, name)
        tag = (case, layout, name)
        La, Ra = _scale_vectors(E, 300 + len(name))
        for which, l, r in (("L", La, None), ("R", None, Ra), ("LR", La, Ra)):
            B = A.duplicate(copy=True)
            lv = rv = None
            if l is not None:
                lv = B.createVecLeft()
                lv.setArray(l)
            if r is not None:
                rv = B.createVecRight()
                rv.setArray(r)
            B.diagonalScale(L=lv, R=rv)
            E1 = _export(B)
            _same_pattern(E, E1, tag + (which,))
            ref, b = M.scaled(E, l, r)
            w, at = M.worst(E1.data, ref, b)
            rows = M.rows_of(E)
            where = (int(rows[at[0]]), int(E.indices[at[0]])) if at else None
            assert w <= 1, (tag, which, w, where)
            assert not E1.data[E.data == 0].any(), (tag, which)
            _line(case, layout, name, f"diagonalScale[{which}]", (w, where))
            worst, _ = _product_check(B, E1, tag + (which, "mult"), seed=len(name) + 1)
            _line(case, layout, name, f"diagonalScale[{which}].mult", worst)
            _diag_check(pa, B, E1, tag + (which,))
            _rows_equal(B, E1, tag + (which,))
            # the original is untouched
        np.testing.assert_array_equal(_export(A).data, E.data)


# ------------------------------------------------------------------- axpy
AXPY_PAIRS = {}


@pytest.mark.parametrize("case,layout", PARAMS)
def test_axpy_and_add(pa, case, layout, tmp_path_factory):
    """axpy(a, X), a = -0.75 and 1, for every ordered pair (Y, X) of node-block
    matrices of one build with equal block shape.  Accepted: X's exported
    pattern lies within Y's (the sum shows every entry it holds), the export is
    inside axpy()'s bound of E0(Y) + a E0(X), and the sum's product agrees
    with its own export.  Refused: error 56, and Y + X is the union-pattern
    AIJ sum of union_sum()."""
    build = _build(pa, case, layout, tmp_path_factory)
    mats = {n: A for n, A in build["mats"].items() if _is_nb(A)}
    accepted, refused, by_rule = [], [], []
    worst_v, worst_p, worst_u = (0.0, None), (0.0, None), (0.0, None)
    for yn, Y in mats.items():
        for xn, X in mats.items():
            if yn == xn or (Y._rbs, Y._cbs) != (X._rbs, X._cbs):
                continue
            EY, EX = _e0(build, yn), _e0(build, xn)
            tag = (case, layout, yn, xn)
            ok = None
            for a in (-0.75, 1.0):
                S = Y.duplicate(copy=True)
                try:
                    S.axpy(a, X)
                    assert ok in (None, True)
                    ok = True
                except pa.petsc.Error as e:
                    assert e.ierr == 56, (tag, e.ierr)
                    assert ok in (None, False)
                    ok = False
                    if "export rules differ" in str(e) and a == 1.0:
                        by_rule.append(f"{yn}+={xn}")  # (the same blocks, another mask rule or other Dirichlet rows)
                    np.testing.assert_array_equal(_export(S).data, EY.data)  # a refused call changes nothing
                    continue
                assert M.is_subset(EY, EX), (tag, "accepted, but X's exported entries are not all in Y's export: "
                                             "the sum multiplies by entries it does not show")
                ES = _export(S)
                _same_pattern(EY, ES, tag)
                ref, b = M.axpy(EY, a, EX)
                w, at = M.worst(ES.data, ref, b)
                assert w <= 1, (tag, a, w, at)
                if w >= worst_v[0]:
                    worst_v = (w, (yn, xn, a, int(M.rows_of(EY)[at[0]]), int(EY.indices[at[0]])))
                wp, _ = _product_check(S, ES, tag + (a, "mult"), seed=len(yn) + len(xn))
                if wp[0] >= worst_p[0]:
                    worst_p = (wp[0], (yn, xn, a) + wp[1])
            (accepted if ok else refused).append(f"{yn}+={xn}")
            if not ok:
                T = Y + X
                assert T.getFormat() == "aij"
                ET = _export(T)
                ip, ix, ref, b = M.union_sum(EY, EX)
                np.testing.assert_array_equal(ET.indptr, ip, err_msg=str(tag))
                np.testing.assert_array_equal(ET.indices, ix, err_msg=str(tag))
                w, at = M.worst(ET.data, ref, b)
                assert w <= 1, (tag, "+", w, at)
                if w >= worst_u[0]:
                    worst_u = (w, (yn, xn))
                _product_check(T, ET, tag + ("+", "mult"), M.input_vectors(ET, C=Y._cbs, seed=5)[:3])
            else:
                T = Y + X  # the same-pattern path of Mat.__add__
                ref, b = M.axpy(EY, 1.0, EX)
                assert M.worst(_export(T).data, ref, b)[0] <= 1, tag
    AXPY_PAIRS[(case, layout)] = (accepted, refused)
    print(f"MATREF {case}/{layout} axpy accepted: {' '.join(accepted) or '-'}")
    print(f"MATREF {case}/{layout} axpy refused: {' '.join(refused) or '-'}")
    print(f"MATREF {case}/{layout} axpy refused for the export rule alone: {' '.join(by_rule) or '-'}")
    _line(case, layout, "pairs", "axpy", worst_v)
    _line(case, layout, "pairs", "axpy.mult", worst_p)
    _line(case, layout, "pairs", "+ (union)", worst_u)


def test_axpy_equal_blocks_other_export_rule(pa):
    """Within one build every block pattern has one export rule, so the pairs
    above never meet the case.  Across builds they do: the pattern of K + Kfs
    (every node sharing a cell, whatever the walls) is the same for the cavity
    and for the same box with the "down" wall alone, while the DoF classes its
    mask reads differ -- the second matrix holds full rows where the first
    exports the diagonal of a normal DoF.  Added in storage the sum would keep
    Y's rule and multiply by entries it does not export.  Either answer is
    checked: a refusal (error 56, Y unchanged, Y + X the union-pattern sum), or
    an accepted sum whose export holds every entry of both and agrees with its
    own product."""
    sums = []
    for walls in (CAVITY, {"down": [0, 0]}):
        dom = pa.Domain()
        dom.configure({"domain": {"ngl": 3, "box-mesh": {"nelem": [4, 4], "lower": [0, 0], "upper": [1, 1]}},
                       "boundary-conditions": {"no-slip": walls}})
        dom.setUp()
        mat = pa.MatNS()
        mat.setDomain(dom)
        mat.build(buildOperators=False)
        sums.append((dom, mat, mat.getKplusKfs()))
    Y, X = sums[0][2], sums[1][2]
    EY, EX = _export(Y), _export(X)
    assert not M.is_subset(EY, EX)  # X shows entries Y's rule hides
    tag = ("ns2d cavity K+Kfs", "ns2d down K+Kfs")
    S = Y.duplicate(copy=True)
    try:
        S.axpy(1.0, X)
        accepted = True
    except pa.petsc.Error as e:
        assert e.ierr == 56, e.ierr
        accepted = False
    ES = _export(S)
    if accepted:
        worst, _ = _product_check(S, ES, tag + ("axpy", "mult"), seed=2)
        _line("ns2d", "two builds", "K+Kfs", "axpy.mult", worst)
        ip, ix, ref, b = M.union_sum(EY, EX)
        np.testing.assert_array_equal(ES.indptr, ip)
        np.testing.assert_array_equal(ES.indices, ix)
    else:
        np.testing.assert_array_equal(ES.data, EY.data)
    T = Y + X
    ET = _export(T)
    ip, ix, ref, b = M.union_sum(EY, EX)
    np.testing.assert_array_equal(ET.indptr, ip)
    np.testing.assert_array_equal(ET.indices, ix)
    w, at = M.worst(ET.data, ref, b)
    assert w <= 1, (tag, "+", w, at)
    worst, _ = _product_check(T, ET, tag + ("+", "mult"), seed=3)
    _line("ns2d", "two builds", "K+Kfs", "+ (union).mult", worst)
    print(f"MATREF ns2d/two builds K+Kfs axpy: {'accepted' if accepted else 'refused (error 56)'}")


# ------------------------------------------------------------ generic AIJ
AIJ_CASES = {"1x1": (1, 1), "5x1100": (5, 1100), "129x1100": (129, 1100), "300x40": (300, 40)}


def _aij(pa, E):
    return pa.petsc.Mat().createAIJ(((E.m, E.m), (E.n, E.n)), csr=E.csr)


def _thin(E, rng, keep_every=2):
    """A matrix whose pattern is a strict subset of E's (every keep_every-th
    entry), with its own values."""
    keep = np.arange(len(E.data)) % keep_every == 0
    lens = np.zeros(E.m, np.int64)
    np.add.at(lens, M.rows_of(E)[keep], 1)
    return Csr(np.concatenate([[0], np.cumsum(lens)]), E.indices[keep], _values(rng, int(keep.sum())), E.n)


def _values(rng, k):
    """U(-1, 1) * 10^U(-1, 1): off the 2^-52 grid of uniform(-1, 1), whose sums are exact."""
    return rng.uniform(-1.0, 1.0, k) * 10.0 ** rng.uniform(-1.0, 1.0, k)


@pytest.mark.parametrize("case", list(AIJ_CASES))
def test_generic_aij(pa, case):
    """createAIJ(csr=) matrices of krylov_ref.spmv_case (rows of 0..1025
    entries; 300x40: tall, with empty rows): mult, getRow of every row,
    getDiagonal (rectangular included), diagonalScale L / R / both, duplicate
    with both flags, axpy with X a strict subset (and not a subset: error
    56), + on different patterns."""
    m, n = AIJ_CASES[case]
    E, _ = spmv_case(m, n)
    if case == "300x40":
        assert (E.row_lengths() == 0).any()
    A = _aij(pa, E)
    tag = ("aij", case)
    EA = _export(A)
    _same_pattern(E, EA, tag)
    np.testing.assert_array_equal(EA.data, E.data)
    worst, _ = _product_check(A, E, tag, seed=3)
    _line("aij", case, "A", "mult", worst)
    _rows_equal(A, E, tag)
    _diag_check(pa, A, E, tag)
    La, Ra = _scale_vectors(E, 41)
    for which, l, r in (("L", La, None), ("R", None, Ra), ("LR", La, Ra)):
        B = A.duplicate(copy=True)
        np.testing.assert_array_equal(_export(B).data, E.data)
        lv = rv = None
        if l is not None:
            lv = B.createVecLeft()
            lv.setArray(l)
        if r is not None:
            rv = B.createVecRight()
            rv.setArray(r)
        B.diagonalScale(L=lv, R=rv)
        E1 = _export(B)
        _same_pattern(E, E1, tag + (which,))
        ref, b = M.scaled(E, l, r)
        w, at = M.worst(E1.data, ref, b)
        assert w <= 1, (tag, which, w, at)
        _line("aij", case, "A", f"diagonalScale[{which}]", (w, at))
        worst, _ = _product_check(B, E1, tag + (which, "mult"), seed=4)
        _diag_check(pa, B, E1, tag + (which,))
        _rows_equal(B, E1, tag + (which,))
        # a later setValues + assemble starts from the scaled values (the host mirror is in step)
        if len(E1.data):
            r0 = int(np.flatnonzero(E.row_lengths() > 0)[0])
            c0 = int(E.indices[E.indptr[r0]])
            B.setValues([r0], [c0], [[0.5]], addv=True)
            B.assemble()
            want = E1.data.copy()
            want[E.indptr[r0]] += 0.5
            np.testing.assert_array_equal(_export(B).data, want)
    np.testing.assert_array_equal(_export(A).data, E.data)
    Z = A.duplicate(copy=False)
    EZ = _export(Z)
    _same_pattern(E, EZ, tag)
    assert not EZ.data.any()
    assert not _mult(Z, M.x_uniform(n, 1)).any()
    # axpy
    rng = np.random.default_rng(43)
    if len(E.data) >= 2:
        X = _thin(E, rng)
        XA = _aij(pa, X)
        for a in (-0.75, 1.0):
            Y = A.duplicate(copy=True)
            Y.axpy(a, XA)
            EY = _export(Y)
            _same_pattern(E, EY, tag)
            ref, b = M.axpy(E, a, X)
            w, at = M.worst(EY.data, ref, b)
            assert w <= 1, (tag, "axpy", a, w, at)
            _line("aij", case, "A", f"axpy[{a}]", (w, at))
            _product_check(Y, EY, tag + ("axpy", "mult"), seed=6)
        if not M.is_subset(X, E):
            with pytest.raises(pa.petsc.Error) as ei:
                XA.axpy(1.0, A)  # Y's pattern lacks entries of X
            assert ei.value.ierr == 56
            np.testing.assert_array_equal(_export(XA).data, X.data)
        # + on different patterns: X (a subset) + A, and a shifted pattern
        T = XA + A
        ip, ix, ref, b = M.union_sum(X, E)
        ET = _export(T)
        np.testing.assert_array_equal(ET.indptr, ip)
        np.testing.assert_array_equal(ET.indices, ix)
        w, at = M.worst(ET.data, ref, b)
        assert w <= 1, (tag, "+", w, at)
        _line("aij", case, "X+A", "+ (union)", (w, at))
        _product_check(T, ET, tag + ("+", "mult"), seed=7)
    F = Csr(E.indptr, E.indices, _values(rng, len(E.data)), n)
    T = A + _aij(pa, F)  # (equal patterns: the axpy path of Mat.__add__)
    ref, b = M.axpy(E, 1.0, F)
    assert M.worst(_export(T).data, ref, b)[0] <= 1


# ------------------------------------------------------------------ state
def _state_matrix(pa):
    """createAIJ(nnz=) + setValues + assemble, then setValues(addv=True) on an
    existing entry with no second assemble(); returns (A, dense before, the
    pending dense)."""
    P = pa.petsc
    n = 6
    A = P.Mat().createAIJ(((n, None), (n, None)), nnz=([3] * n, None))
    dense = np.zeros((n, n))
    for i in range(n):
        for j in (i - 1, i, i + 1):
            if 0 <= j < n:
                v = 4.0 + i if i == j else -1.0 - 0.125 * j
                A.setValues([i], [j], [[v]])
                dense[i, j] = v
    return A, dense


def _pend(A, dense):
    A.setValues([2], [3], [[0.25]], addv=True)
    after = dense.copy()
    after[2, 3] += 0.25
    return after


def _state_ops(pa, A, other):
    P = pa.petsc
    n = A.getSize()[0]

    def ksp():
        k = P.KSP().create()
        k.setOperators(A)
        k.setUp()

    def vec():
        v = P.Vec().createSeq(n)
        v.set(1.0)
        return v

    return {
        "mult": lambda: A.mult(vec(), vec()),
        "multAdd": lambda: A.multAdd(vec(), vec(), vec()),
        "getDiagonal": lambda: A.getDiagonal(vec()),
        "getRow": lambda: A.getRow(2),
        "getValuesCSR": lambda: A.getValuesCSR(),
        "duplicate": lambda: A.duplicate(copy=True),
        "convert": lambda: A.convert("aij"),
        "diagonalScale": lambda: A.diagonalScale(L=vec()),
        "axpy as Y": lambda: A.axpy(1.0, other),
        "axpy as X": lambda: other.axpy(1.0, A),
        "KSP.setOperators + setUp": ksp,
    }


def test_unassembled_matrix_is_refused(pa):
    """A matrix that was never assembled: every entry point that reads its
    arrays returns error 73 from its first statement (kle.h), before any
    device work."""
    A, dense = _state_matrix(pa)
    other, d2 = _state_matrix(pa)
    other.assemble()
    for name, op in _state_ops(pa, A, other).items():
        with pytest.raises(pa.petsc.Error) as ei:
            op()
        assert ei.value.ierr == 73, (name, ei.value.ierr)
    with pytest.raises(pa.petsc.Error) as ei:
        A + other
    assert ei.value.ierr == 73
    A.assemble()
    E = _export(A)
    D = np.zeros_like(dense)
    D[M.rows_of(E), E.indices] = E.data
    np.testing.assert_array_equal(D, dense)
    np.testing.assert_array_equal(_export(other).data, E.data)  # the refused axpy changed nothing


def test_values_set_after_assembly_need_assemble(pa):
    """setValues on an assembled matrix leaves it unassembled, as PETSc's:
    every reader and every writer returns error 73 (the same answer from all
    of them) and loses nothing; after assemble() the new value is there and
    nothing else changed; an insert outside the pattern is still error 77."""
    P = pa.petsc
    A, dense = _state_matrix(pa)
    A.assemble()
    other, _ = _state_matrix(pa)
    other.assemble()
    np.testing.assert_array_equal(_export(A).data, dense[dense != 0])
    ksp = P.KSP().create()
    ksp.setType("gmres")  # (the matrix is not symmetric)
    ksp.setOperators(A)
    ksp.setUp()
    after = _pend(A, dense)
    for name, op in _state_ops(pa, A, other).items():
        with pytest.raises(P.Error) as ei:
            op()
        assert ei.value.ierr == 73, (name, ei.value.ierr)
    b = P.Vec().createSeq(6)
    b.set(1.0)
    with pytest.raises(P.Error) as ei:
        ksp.solve(b, P.Vec().createSeq(6))  # (set up before the setValues)
    assert ei.value.ierr == 73
    with pytest.raises(P.Error) as ei:
        A.setValues([0], [4], [[1.0]], addv=True)
    assert ei.value.ierr == 77
    A.assemble()
    E = _export(A)
    D = np.zeros_like(dense)
    D[M.rows_of(E), E.indices] = E.data
    np.testing.assert_array_equal(D, after)
    xa = M.x_uniform(6, 9)
    ref, bnd = M.product(E, xa)
    assert M.worst(_mult(A, xa), ref, bnd)[0] <= 1
    np.testing.assert_array_equal(A.getDiagonal().getArray(), np.diag(after))
    np.testing.assert_array_equal(A.getRow(2)[1], after[2, 1:4])
    np.testing.assert_array_equal(_export(A.duplicate(copy=True)).data, E.data)
    np.testing.assert_array_equal(_export(other).data, dense[dense != 0])
    # the writers see it too: scale and axpy start from the assembled value
    v = P.Vec().createSeq(6)
    v.set(2.0)
    A.diagonalScale(L=v)
    np.testing.assert_array_equal(_export(A).data, 2.0 * E.data)
    ksp.solve(b, P.Vec().createSeq(6))
    assert ksp.getConvergedReason() > 0
