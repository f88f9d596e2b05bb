"""The nine assembled no-slip matrices of MatNS.build() (kle_assemble_ns: K,
Krhs, Rw, Rd, Kfs, Krhsfs, Rwfs, Rdfs, K+Kfs) on one rank, entry by entry
against the longdouble restatement of tests/ns_ref.py.

Patterns bit-exact, the explicit zeros of the DoF-level patterns included;
every entry within its bound (ns_ref's docstring: the scattered element
bounds of elem_ref with the kernel's count C, one rounding per incident
element, the forms of the T diagonals; 0 where the formula gives an exact 0 or
1); K+Kfs's T diagonals equal to fl(1 + Kfs's) bit for bit; the DoF classes
equal to the reference's.  Each case runs under both element kernels (MFMA
and KLE_ELEMENT_VALU=1) and prints one NSREF line per matrix with the worst
err / bound and where it occurs.

The shapes are the smallest that reach every rule, and each case asserts what
it was chosen for (REACH)."""
import os

import numpy as np
import pytest

import ns_ref as NS
from oracle import oracle as O

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
LOWER, STEP = [-1.5, 0.25, 10.0], [0.7, 0.05, 1.0]  # (tests/test_gpu_elem_ref.py)
KERNELS = {"mfma": {}, "valu": {"KLE_ELEMENT_VALU": "1"}}
SIX = ["up", "down", "left", "right", "front", "back"]


def _unit(nelem):
    return {"nelem": nelem, "lower": [0] * len(nelem), "upper": [1] * len(nelem)}


def _offset(nelem):
    d = len(nelem)
    return {"nelem": nelem, "lower": LOWER[:d], "upper": [a + n * h for a, n, h in zip(LOWER, nelem, STEP)]}


# name -> (dim, ngl, box-mesh | "test.msh" | "perturbed222", walls in configuration order, what it reaches)
CASES = {}
for _n in (3, 4):
    CASES[f"box32_ngl{_n}_left_first"] = (2, _n, _unit([3, 2]), ["left", "up", "down"], "corner_kept")
    CASES[f"box32_ngl{_n}_cavity"] = (2, _n, _unit([3, 2]), ["up", "down", "left", "right"], "corner_dropped")
CASES["box212_ngl3_six"] = (3, 3, _unit([2, 1, 2]), SIX, "six")
CASES["box221_ngl4_down"] = (3, 4, _unit([2, 2, 1]), ["down"], "partial")
CASES["offset32_ngl3_cavity"] = (2, 3, _offset([3, 2]), ["up", "down", "left", "right"], "corner_dropped")
CASES["offset212_ngl3_six"] = (3, 3, _offset([2, 1, 2]), SIX, "six")
CASES["testmsh_ngl3_down"] = (2, 3, "test.msh", ["down"], "tagged")
CASES["perturbed222_ngl3_six"] = (3, 3, "perturbed222", SIX, "moved_vertex")


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


def _build(pa, dim, ngl, dom_cfg, walls, env):
    cfg = {"domain": dict(ngl=ngl, **dom_cfg), "boundary-conditions": {"no-slip": {w: [0.0] * dim for w in walls}}}
    dom = pa.Domain()
    dom.configure(cfg)
    dom.setUp()
    mat = pa.MatNS()
    mat.setDomain(dom)
    old = {k: os.environ.get(k) for k in ("KLE_ELEMENT_VALU", "KLE_ELEMENT_WAVES")}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        mat.build(buildOperators=False, nsType="assembled")
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return dom, mat


def exports_of(mat):
    ms = dict(zip(NS.NAMES[:-1], mat.kle))
    ms["KplusKfs"] = mat.getKplusKfs()
    return {k: A.getValuesCSR() for k, A in ms.items()}


def _reach(what, dim, coords, cls, corners):
    """The property a case was chosen for."""
    c = cls.reshape(-1, dim)
    lo, hi = coords.min(0), coords.max(0)
    ext = (hi - lo).max()
    on = [(np.abs(coords[:, a] - lo[a]) <= 1e-9 * ext, np.abs(coords[:, a] - hi[a]) <= 1e-9 * ext) for a in range(dim)]
    if what in ("corner_kept", "corner_dropped"):
        left_corners = on[0][0] & (on[1][0] | on[1][1])
        assert left_corners.sum() == 2
        want = [NS.N, NS.N] if what == "corner_kept" else [NS.T, NS.N]
        assert (c[left_corners] == want).all()
        if what == "corner_kept":  # and a free right side
            assert (c[on[0][1] & ~on[1][0] & ~on[1][1]] == NS.F).all()
    if what == "six":
        assert all((c[s][:, a] != NS.F).all() for a in range(dim) for s in on[a])
        assert (c == NS.F).all(axis=1).any()
    if what == "partial":
        assert (c[on[1][0]] == [NS.T, NS.N, NS.T]).all() and (c[~on[1][0]] == NS.F).all()
    if what == "tagged":
        bnd = on[0][0] | on[0][1] | on[1][0] | on[1][1]
        assert (c[bnd] == [NS.T, NS.N]).all() and (c[~bnd] == NS.F).all()
    if what == "moved_vertex":  # a cell set with non-constant Jacobians
        X = np.asarray(corners)
        edges = X[:, [3, 2, 6, 5], :] - X[:, [0, 1, 7, 4], :]  # the four x-edges of the closure order differ
        assert np.abs(edges - edges[:, :1]).max() > 1e-3
    assert all((cls == k).any() for k in (NS.F, NS.T, NS.N))


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("case", list(CASES))
def test_noslip_matrices_match_longdouble(pa, case, kernel, tmp_path):
    dim, ngl, where, walls, what = CASES[case]
    members = None
    if where == "test.msh":
        dom_cfg = {"gmsh-file": os.path.join(G, "test.msh")}
    elif where == "perturbed222":
        from pynama_amd.meshgen import perturbed_box, write_gmsh
        path = str(tmp_path / "p.msh")
        write_gmsh(path, 3, *perturbed_box(3, [2, 2, 2], seed=13))
        dom_cfg = {"gmsh-file": path}
    else:
        dom_cfg = {"box-mesh": where}
    dom, mat = _build(pa, dim, ngl, dom_cfg, walls, KERNELS[kernel])
    mesh = dom.getMesh()
    coords = np.asarray(mesh.coords(), float).reshape(-1, dim)
    if where == "test.msh":  # the file tags its whole boundary 1 = "down"
        _, verts, _, facets, tags = O.read_gmsh(dom_cfg["gmsh-file"])
        members = {"down": NS.segment_nodes(coords, verts, facets[tags == 1])}
    cls, ref = NS.reference(dim, ngl, mesh.conn(), mesh.corners(), coords, walls, kernel=kernel, members=members)
    _reach(what, dim, coords, cls, mesh.corners())
    t, n = NS.class_sets(cls)
    normal = set(int(i) for i in dom.getNormalDofs(collect=True))
    assert normal == n
    assert set(int(i) for i in dom.getTangDofs(collect=True)) - normal == t
    bad, _ = NS.check_exports(f"{case} {kernel}", exports_of(mat), ref)
    assert not bad, (case, kernel, bad)
