"""The longdouble no-slip reference (tests/ns_ref.py) against the oracle's
restatement of MatNS.buildNS and the original project's fixtures, its DoF
classes against oracle.noslip_dofs and the fixtures' sets, and the power of its
comparison to tell a subtly wrong assembly from a right one.

Values: <= 1e-13 of the matrix's scale against the fp64 sources (DESIGN 4:
the oracle against the fixtures); patterns equal, explicit zeros included.
K + Kfs of a source is PETSc's: the union pattern, the entrywise fp64 sum.

Planted errors (test_planted_errors): each is put into the reference, the
result is rounded as a correct fp64 assembly would round it
(ns_ref.fp64_image) and compared with the unplanted reference exactly as the
device exports are (ns_ref.compare, ns_ref.tdiag_identity).  Each must break
a pattern, push an entry past its bound, or break the T-diagonal identity."""
import itertools
import os

import numpy as np
import pytest

import ns_ref as NS
from oracle import oracle as O

G = os.path.join(os.path.dirname(__file__), "golden")
CAVITY = ["up", "down", "left", "right"]
SIX = ["up", "down", "left", "right", "front", "back"]
ORACLE_CASES = [(2, [6, 5], 4, ["down", "up", "right", "left"]), (2, [5, 4], 3, ["left", "up", "down"]),
                (3, [3, 2, 2], 3, SIX)]


def box(dim, nelem, ngl, upper=None):
    import pynama_amd as pa
    m = pa.BoxMesh(dim, nelem, [0] * dim, upper or [1] * dim, ngl)
    return m.conn(), m.corners(), m.coords()


def _keys(ip, ix, n):
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    return rows * n + np.asarray(ix, np.int64)


def petsc_sum(a, b, n):
    """K + Kfs as PETSc forms it from two CSR triples: union pattern, fp64 sum."""
    ka, kb = _keys(a[0], a[1], n), _keys(b[0], b[1], n)
    keys = np.union1d(ka, kb)
    d = np.zeros(len(keys))
    d[np.searchsorted(keys, ka)] += a[2]
    d[np.searchsorted(keys, kb)] += b[2]
    ip = np.zeros(len(a[0]), np.int64)
    np.cumsum(np.bincount(keys // n, minlength=len(a[0]) - 1), out=ip[1:])
    return ip, keys % n, d


def check_source(ref, src, tag):
    """src: {name: (indptr, indices, data)} of the eight matrices."""
    src = dict(src)
    src["KplusKfs"] = petsc_sum(src["K"], src["Kfs"], ref["K"].n)
    for nm in NS.NAMES:
        A = ref[nm]
        ip, ix, d = src[nm]
        np.testing.assert_array_equal(ip, A.indptr, err_msg=f"{tag} {nm}")
        np.testing.assert_array_equal(ix, A.indices, err_msg=f"{tag} {nm}")
        scale = max(1.0, float(np.abs(d).max()))
        err = float(np.abs(d - A.value).max())
        assert err <= 1e-13 * scale, (tag, nm, err / scale)
        assert (A.bound >= 0).all() and np.isfinite(A.bound).all()
        # exact entries of the formula are exact in the source too
        assert np.array_equal(d[A.bound == 0], A.value[A.bound == 0].astype(float)), (tag, nm)


# ------------------------------------------------------------------ classes
@pytest.mark.parametrize("walls", [list(p) for p in itertools.permutations(["left", "up", "down"])]
                         + [CAVITY, ["down", "up", "right", "left"], ["left", "right", "up", "down"]])
def test_classes_match_oracle_2d(walls):
    _, _, coords = box(2, [3, 2], 3)
    om = O.BoxMesh(2, [3, 2], [0, 0], [1, 1], 3)
    t, n = O.noslip_dofs(om, walls)
    assert NS.class_sets(NS.classes(coords, walls)) == (t - n, n)


@pytest.mark.parametrize("walls", [SIX, ["left", "right", "up", "down", "front", "back"], ["down"]])
def test_classes_match_oracle_3d(walls):
    _, _, coords = box(3, [2, 1, 2], 3)
    om = O.BoxMesh(3, [2, 1, 2], [0, 0, 0], [1, 1, 1], 3)
    t, n = O.noslip_dofs(om, walls)
    assert NS.class_sets(NS.classes(coords, walls)) == (t - n, n)


# ------------------------------------------------------------------- oracle
@pytest.mark.parametrize("dim,nelem,ngl,walls", ORACLE_CASES)
def test_reference_matches_oracle(dim, nelem, ngl, walls):
    conn, corners, coords = box(dim, nelem, ngl)
    cls, ref = NS.reference(dim, ngl, conn, corners, coords, walls, kernel="oracle")
    om = O.BoxMesh(dim, nelem, [0] * dim, [1] * dim, ngl)
    t, n = O.noslip_dofs(om, walls)
    assert NS.class_sets(cls) == (t - n, n)
    orc = O.assemble_ns(om, t, n)
    check_source(ref, {k: (A.indptr, A.indices, A.data) for k, A in orc.items()}, "oracle")
    # and inside the bound of the oracle's own rounding count
    for nm in NS.NAMES[:-1]:
        ok, w, at = NS.compare((orc[nm].indptr, orc[nm].indices, orc[nm].data), ref[nm])
        assert ok and w <= 1, (nm, w, at)


# ----------------------------------------------------------------- fixtures
def _fixture_src(g):
    return {k: (g[k + "_indptr"], g[k + "_indices"], g[k + "_data"]) for k in NS.NAMES[:-1]}


def _fixture_sets(g, cls):
    t, n = NS.class_sets(cls)
    assert n == set(g["normal_dofs"].tolist())
    assert t == set(g["tang_dofs"].tolist()) - n


def test_reference_matches_cavity_fixture():
    g = np.load(os.path.join(G, "case_cavity2d.npz"))
    conn, corners, coords = box(2, [4, 4], 3)
    cls, ref = NS.reference(2, 3, conn, corners, coords, CAVITY, kernel="oracle")
    _fixture_sets(g, cls)
    check_source(ref, _fixture_src(g), "cavity2d")


@pytest.mark.parametrize("case,walls", [("gmsh2d_ns", ["down"]), ("umesh3d_ns", SIX)])
def test_reference_matches_gmsh_fixtures(case, walls, tmp_path):
    """The product's host mesh gives cells and corners; the reference is built
    in the fixture's numbering (oracle.node_map by coordinates)."""
    from pynama_amd.mesh import UnstructuredMesh
    from pynama_amd.meshgen import write_gmsh
    g = np.load(os.path.join(G, f"case_{case}.npz"))
    dim, ngl = int(g["dim"]), int(g["ngl"])
    path = os.path.join(G, "test.msh")
    if "mesh_cells" in g:
        path = str(tmp_path / "mesh.msh")
        write_gmsh(path, dim, g["mesh_vertices"], g["mesh_cells"], g["mesh_facets"], g["mesh_tags"])
    m = UnstructuredMesh.from_gmsh(path, ngl)
    mp = O.node_map(m.coords(), g["coords"])
    members = None
    if case == "gmsh2d_ns":  # test.msh tags its whole boundary 1 = "down"
        _, verts, _, facets, tags = O.read_gmsh(path)
        members = {"down": NS.segment_nodes(g["coords"], verts, facets[tags == 1])}
        assert len(members["down"]) == 40
    cls, ref = NS.reference(dim, ngl, mp[m.conn()], m.corners(), g["coords"], walls, kernel="oracle",
                            members=members)
    _fixture_sets(g, cls)
    check_source(ref, _fixture_src(g), case)


# ----------------------------------------------------------- planted errors
@pytest.fixture(scope="module")
def planted_case():
    """2-D [3,4] ngl 3 (the lattice of the two-rank three-wall run), walls up,
    down, left: both outcomes of the corner rule are within reach (left after
    up / down drops the corner's x normal; left first keeps it)."""
    dim, ngl, walls = 2, 3, ["up", "down", "left"]
    conn, corners, coords = box(dim, [3, 4], ngl)
    cls = NS.classes(coords, walls)
    good = NS.assemble(dim, ngl, conn, corners, cls)
    return dim, ngl, walls, conn, corners, coords, cls, good


def _verdict(img, good):
    """How the comparison of the device exports sees an image: the matrices
    whose pattern breaks, those with an entry past its bound, the T diagonals
    off the identity."""
    broken, past = [], []
    for nm in NS.NAMES:
        A = good[nm]
        bad = img[nm]
        ok, w, _ = NS.compare(bad if isinstance(bad, tuple) else (A.indptr, A.indices, bad), A)
        if not ok:
            broken.append(nm)
        elif w > 1:
            past.append(nm)
    ident = [] if ("Kfs" in broken or "KplusKfs" in broken) else \
        NS.tdiag_identity(_data(img["Kfs"]), _data(img["KplusKfs"]), good).tolist()
    return broken, past, ident


def _data(x):
    return x[2] if isinstance(x, tuple) else x


def _image_of(bad):
    """fp64 image of a planted reference, with its own pattern."""
    img = NS.fp64_image(bad)
    return {nm: (bad[nm].indptr, bad[nm].indices, img[nm]) for nm in NS.NAMES}


def test_unplanted_image_passes(planted_case):
    *_, good = planted_case
    assert _verdict(NS.fp64_image(good), good) == ([], [], [])


def test_planted_errors(planted_case):
    dim, ngl, walls, conn, corners, coords, cls, good = planted_case
    seen = {}
    # the corner rule skipped: the corner's x DoF stays normal
    c = NS.classes(coords, walls, plant={"corner": "skip"})
    assert (c != cls).sum() == 2  # the two left corners
    seen["corner rule skipped"] = _verdict(_image_of(NS.assemble(dim, ngl, conn, corners, c)), good)
    # the corner rule whatever the order: right on up, down, left -- so plant it where left comes first
    w2 = ["left", "up", "down"]
    cls2 = NS.classes(coords, w2)
    good2 = NS.assemble(dim, ngl, conn, corners, cls2)
    c = NS.classes(coords, w2, plant={"corner": "always"})
    assert (c != cls2).sum() == 2 and np.array_equal(NS.classes(coords, walls, plant={"corner": "always"}), cls)
    seen["corner rule whatever the order"] = _verdict(_image_of(NS.assemble(dim, ngl, conn, corners, c)), good2)
    # one wall DoF on an interface plane of the two-rank slabs classed free: the
    # left wall's node at mid height (a ghost of the upper rank's lower neighbour)
    L = [3 * (ngl - 1) + 1, 4 * (ngl - 1) + 1]
    node = (L[1] // 2) * L[0]
    assert coords[node, 0] == 0 and 0 < coords[node, 1] < 1
    for a, what in ((0, "normal"), (1, "tangential")):
        assert cls[node * dim + a] == (NS.N if a == 0 else NS.T)
        c = NS.classes(coords, walls, plant={"free": node * dim + a})
        seen[f"one {what} wall DoF classed free"] = _verdict(_image_of(NS.assemble(dim, ngl, conn, corners, c)), good)
    seen["Krhsfs without its minus"] = _verdict(
        _image_of(NS.assemble(dim, ngl, conn, corners, cls, plant={"krhsfs_sign": 1})), good)
    td = good["tdiag"][0]
    seen["-1 missing from one Kfs diagonal"] = _verdict(
        _image_of(NS.assemble(dim, ngl, conn, corners, cls, plant={"no_minus1": int(td[len(td) // 2])})), good)
    seen["one element's block twice"] = _verdict(
        _image_of(NS.assemble(dim, ngl, conn, corners, cls, plant={"twice": len(conn) // 2})), good)
    # a plain S on K+Kfs's T diagonals.  fl(1 + fl(S - 1)) is S itself for S >= 1/2 (both steps are
    # exact), and the diagonals of the unit meshes are hundreds: the two forms differ only on small
    # elements, so this one is planted on a 3-D box of edge 1e-3 (S = 0.03 .. 0.34)
    tiny = box(3, [1, 1, 2], 3, upper=[1e-3, 1e-3, 2e-3])
    _, gt = NS.reference(3, 3, *tiny, ["down"])
    assert _verdict(NS.fp64_image(gt), gt) == ([], [], [])
    right, plain = NS.fp64_image(gt), NS.fp64_image(gt, plain_S=True)
    differ = np.nonzero(right["KplusKfs"] != plain["KplusKfs"])[0]
    assert len(differ) >= 1
    # (by the rounding of S - 1 alone: half a last bit of a number below 1)
    assert (np.abs(right["KplusKfs"][differ] - plain["KplusKfs"][differ]) <= NS.U / 2).all()
    seen["plain S for 1 + (S - 1)"] = v = _verdict(plain, gt)
    # the bound cannot see a last bit (b_S is many u |S|): the identity alone catches it
    assert v[0] == [] and v[1] == [] and len(v[2]) == len(differ)
    for what, (broken, past, ident) in seen.items():
        print(f"NSREF planted {what}: pattern broken {broken}, past bound {past}, "
              f"T diagonals off the identity {len(ident)}")
        assert broken or past or ident, what
    # what the old check (1e-12 of the matrix's scale) would have made of the value errors
    for what in ("-1 missing from one Kfs diagonal", "one element's block twice", "Krhsfs without its minus"):
        assert seen[what][1], what
