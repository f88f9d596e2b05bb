"""The reference of the sum-factorised K (tests/sumfac_ref.py) checks itself:
host only, no GPU.

1. The factorised formula the kernel evaluates, in longdouble, equals the
   dense ref_kle(X) @ x of elem_ref on jittered single elements.
2. The bound is not vacuous: the same formula evaluated in fp64 lies inside
   it, and each planted error leaves it on at least one row of every shape.
3. The mesh-level reference on the reference's test.msh equals the product of
   the golden assembled K, within the assembled bound."""
import os

import numpy as np
import pytest

import elem_ref as R
import sumfac_ref as SF
from oracle import oracle as O

G = os.path.join(os.path.dirname(__file__), "golden")
LD = R.LD

# (dim, ngl): both kinds of full rule (Gauss for ngl <= 3, GLL above) in 2-D and 3-D
SHAPES = [(2, 3), (2, 4), (2, 8), (3, 2), (3, 3), (3, 5)]


def _jittered(dim, seed):
    rng = np.random.default_rng(seed)
    X = R.CORN[dim].astype(np.float64) * np.array([1.0, 0.7, 1.3][:dim]) + np.array([0.2, -1.0, 3.0][:dim])
    return X + rng.uniform(-0.12, 0.12, X.shape)


@pytest.mark.parametrize("dim,ngl", SHAPES)
def test_factorised_formula_equals_dense_reference(dim, ngl):
    X = _jittered(dim, 10 * dim + ngl)
    x = np.random.default_rng(ngl).uniform(-1, 1, dim * ngl ** dim)
    K = R.ref_kle(dim, ngl, X)[0]
    want = K @ x.astype(LD)
    got = SF.sumfac_apply(dim, ngl, X, x)
    scale = (np.abs(K).astype(np.float64) @ np.abs(x))
    rel = float(np.max(np.abs(got - want).astype(np.float64) / scale))
    print(f"dim {dim} ngl {ngl}: max |sumfac - dense| / (|K||x|) = {rel:.2e}")
    assert rel <= 64 * float(np.finfo(LD).eps) * ngl ** dim


def _two_element_mesh(dim, ngl, seed):
    """Two jittered cells whose i = 0 faces share their nodes, so the gather has
    something to add (the algebra needs no geometric conformity); Dirichlet on
    both i = ngl - 1 faces."""
    X0, X1 = _jittered(dim, seed), _jittered(dim, seed + 1)
    nn = ngl ** dim
    idx = np.arange(nn).reshape((ngl,) * dim)  # [(k,) j, i]
    conn0 = idx.ravel()
    idx1 = idx + nn
    shared = idx[..., 0]
    idx1 = idx1.copy()
    idx1[..., 0] = shared
    conn1 = idx1.ravel()
    # renumber compactly
    used = np.unique(np.concatenate([conn0, conn1]))
    mp = -np.ones(2 * nn, np.int64)
    mp[used] = np.arange(len(used))
    conn = np.stack([mp[conn0], mp[conn1]])
    N = len(used)
    dirflag = np.zeros(N, bool)
    dirflag[mp[idx[..., -1].ravel()]] = True
    dirflag[mp[idx1[..., -1].ravel()]] = True
    return conn, np.stack([X0, X1]), dirflag


@pytest.mark.parametrize("which", ["K", "Krhs"])
@pytest.mark.parametrize("dim,ngl", [(2, 3), (2, 5), (3, 3), (3, 4)])
def test_bound_holds_the_fp64_formula_and_catches_planted_errors(dim, ngl, which):
    conn, corners, dirflag = _two_element_mesh(dim, ngl, 7 * dim + ngl)
    for X in corners:  # both cells are valid (positive Jacobians)
        assert np.all(R.point_sets(dim, ngl, X)["full"].det > 0)
    N = len(dirflag)
    x = np.random.default_rng(3).uniform(-1, 1, N * dim)
    ref = SF.reference(dim, ngl, conn, corners, dirflag, which, x)
    assert np.all(ref.bound[~ref.dird] > 0)

    def worst(**kw):
        r = SF.reference(dim, ngl, conn, corners, dirflag, which, x, diag=False, **kw)
        return R.worst(r.y.astype(np.float64), ref.y, ref.bound)[0]

    def planted(**kw):
        return lambda e, X, xt: SF.sumfac_apply(dim, ngl, X, xt, **kw)

    # the reference alone: the factorised formula in fp64 (and rounded to fp64 on return)
    w0 = worst(apply=planted(dtype=np.float64))
    print(f"dim {dim} ngl {ngl} {which}: fp64 formula err/bound {w0:.3g}")
    assert w0 <= 1.0
    free_l = int(np.nonzero(~dirflag[conn[1]])[0][0])
    cases = {"alpha_w": dict(apply=planted(plant={"alpha_w": R.ALPHA_W * (1 + 1e-9)})),
             "grad_T_sign": dict(apply=planted(flip=True)),
             "drop_red": dict(apply=planted(plant={"drop_red": True})),
             "skip_incidence": dict(skip=(1, free_l))}
    for name, kw in cases.items():
        w = worst(**kw)
        print(f"  planted {name}: err/bound {w:.3g}")
        assert w > 1.0, name


def test_mesh_reference_equals_golden_assembled_product():
    from pynama_amd.mesh import FACES, UnstructuredMesh
    g = np.load(os.path.join(G, "case_gmsh2d.npz"))
    dim, ngl = int(g["dim"]), int(g["ngl"])
    assert (dim, ngl) == (2, 3)
    m = UnstructuredMesh.from_gmsh(os.path.join(G, "test.msh"), ngl)
    conn, corners = m.conn(), m.corners()
    inc = SF.incidence(conn, m.N)
    assert set(np.unique(inc)) - {1, 2, 4}, "the fixture has nodes of valence other than 4"
    dirflag = np.zeros(m.N, bool)
    dirflag[m.face_nodes(FACES[dim])] = True
    mp = O.node_map(m.coords(), g["coords"])  # our node -> the fixture's
    np.testing.assert_array_equal(np.sort(mp[np.nonzero(dirflag)[0]]), np.sort(g["dir_nodes"]))
    x = np.random.default_rng(11).uniform(-1, 1, m.N * dim)
    xg = np.zeros_like(x)
    dofs = R.dof(mp, dim)  # our DoF k -> the fixture's DoF dofs[k]
    xg[dofs] = x
    for which in ("K", "Krhs"):
        ref = SF.reference(dim, ngl, conn, corners, dirflag, which, x)
        yg = SF.csr_mult((g[which + "_indptr"], g[which + "_indices"], g[which + "_data"]), xg)[dofs]
        # the fixture's K is the reference code's: one running sum over the Gauss points
        # (elem_ref.C "oracle") where abound counts the device's MFMA order -- the longer of the two
        k_or, k_mf = R.C(dim, ngl, "oracle")[0], R.C(dim, ngl, "mfma")[0]
        w, at = R.worst(yg.astype(np.float64), ref.y, ref.abound * max(1.0, k_or / k_mf))
        print(f"{which}: golden product vs mesh reference, err / assembled bound {w:.3g} at {at}")
        assert w <= 1.0
