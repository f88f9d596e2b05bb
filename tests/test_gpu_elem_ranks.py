"""The element-wise operators on several ranks: K, Krhs, Rw (kle_elem.hip) and
Curl, SrT, DivSrT (kle_colloc.hip) on slab-partitioned uniform box meshes, the
Krylov solve on the element-wise K and the fully matrix-free evalRHS.

Ranks are spawned as tests/test_gpu_multirank.py does (torch.multiprocessing
spawn, gloo, KLE_TRANSPORT=host, all ranks on one GPU); one spawned run per
configuration is cached and shared by the assertions on it.

x of every product is sin(arange) over each rank's ownership range of the
column space.  The concatenated owned rows must be the one-rank product of
the same operator (made in the parent) bit for bit, and within these bounds:

K, Krhs (tests/test_gpu_elem.py), reference the oracle's assembled CSR product
in np.longdouble:

    |y_i - ref_i| <= n eps B_i + delta Kmax X_i

n = dim ngl^dim + 8, B_i the sum over incident elements of |K_e0| |x_e| masked
as the operator masks (max(B_i, |x_i|) on Dirichlet rows), Kmax = max |K_e0|,
X_i the sum over incident elements of the 1-norm of the masked x_e, delta the
largest |K_e - K_e0| / Kmax over the mesh's elements (kle_element_kle),
required <= 2e-12.

Rw (tests/test_gpu_matfree.py): the same with n = dim_w ngl^dim + 8, Rw_e0,
Rmax, delta_R, w unmasked, B_i = 0 on Dirichlet rows (which must be 0.0).

Curl, SrT, DivSrT (tests/test_gpu_colloc.py), reference the assembled
operator's CSR product in np.longdouble:

    |y_i - ref_i| <= n eps B_i + delta Mmax X_i winv_g + 2 delta_w B_i

n = CW (dim (ngl - 1) + 1) + 2^dim + 8, B_i = winv_g sum_e (|M_e0| |x_e|)_l,
X_i = sum_e ||x_e||_1, delta and delta_w from the oracle's Element.ops on the
device mesh's corners, required <= 2e-12.

K's selection test: the issue asks that NaN in every Dirichlet entry of x
"leaves no NaN in any row".  A Dirichlet row of K is the unit row y_i = x_i
(tests/test_gpu_elem.py::test_masking_is_selection asserts NaN there), so the
test asks it of every free row -- bit-equal to the product without the NaN --
and NaN on the Dirichlet rows."""
import functools
import os
import socket
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
EPS = np.finfo(np.float64).eps
KLE = ("K", "Krhs", "Rw")
OPS = ("Curl", "SrT", "DivSrT")
CAVITY_BC = {"no-slip": {"up": [2, 0], "down": [0, 0], "left": [0, 0], "right": [0, 0]}}

# Each the smallest shape that reaches the edge named (nd = dim ngl^dim rows per
# element in groups of 128; a ghost-layer element launches the groups holding
# its top-plane rows [nd - nd / ngl, nd) alone).
SHAPES = {
    # two layers per rank: rank 1 has a ghost layer, an interior layer and no
    # upper ghost; nd = 192, top-plane rows 144..191 in the second of two groups
    "r2_3x2x4_p4": dict(size=2, nelem=[3, 2, 4], ngl=4, solve="cg", refusals=True),
    # one layer per rank: the middle rank has no interior element and both
    # neighbours; nd = 81 is a single partial group
    "r3_2x3x3_p3": dict(size=3, nelem=[2, 3, 3], ngl=3, solve="pipecg", variants=True),
    "r3_2x2x5_p4": dict(size=3, nelem=[2, 2, 5], ngl=4),  # uneven layers 1 / 2 / 2
    "r8_2x2x8_p4": dict(size=8, nelem=[2, 2, 8], ngl=4, solve="cg"),  # config 3's decomposition
    # nd = 1029: top-plane rows 882..1028 start inside a group and span three
    "r2_1x1x2_p7": dict(size=2, nelem=[1, 1, 2], ngl=7),
    "r2_2x2x2_p5": dict(size=2, nelem=[2, 2, 2], ngl=5),  # nd = 375: the last of three groups partial
    # 2-D, partition axis y; Rw has nc = 25: a padding column next to ghosts
    "r2_2d_3x4_p5": dict(size=2, nelem=[3, 4], ngl=5),
    "r2_2d_cavity": dict(size=2, nelem=[4, 4], ngl=3, bc=CAVITY_BC),  # no-slip: the collocation operators alone
}


# Krylov methods x preconditioners on the element-wise K.  Bound of a converged
# solve's true residual |b - K u| / |b|, formed here through the operator: CG
# and pipelined CG are held to rtol on the true residual by libkle's correction
# solves and GMRES without a preconditioner stops on it, so 2 rtol (the factor
# for the rounding of this second evaluation, as tests/test_gpu_elem.py::
# test_solves allows); GMRES with Jacobi stops on the left-preconditioned
# residual |D^-1 r| <= rtol |D^-1 b|, which bounds |r| <= rtol |b| max(d) / min(d).
VARIANTS = [(kt, pct) for kt in ("cg", "cg_single_reduction", "pipecg", "gmres") for pct in ("none", "jacobi")]
VARIANT_RTOL = 1e-10


def _names(spec):
    return OPS if "bc" in spec else KLE + OPS


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _cfg(spec):
    dim = len(spec["nelem"])
    tg = {"custom-func": {"name": "taylor_green3d" if dim == 3 else "taylor_green"}}
    return {"domain": {"ngl": spec["ngl"], "box-mesh": {"nelem": list(spec["nelem"]), "lower": [0.0] * dim,
                                                        "upper": [1.0] * dim}},
            "boundary-conditions": spec.get("bc") or tg}


def _build(pa, spec):
    """The domain and its element-wise operators, nothing assembled (the
    no-slip KLE matrices, which have no element-wise form, aside)."""
    dom = pa.Domain()
    dom.configure(_cfg(spec))
    dom.setUp()
    if "bc" in spec:
        mat = pa.MatNS()
        mat.setDomain(dom)
        mat.build(opType="element")
        ops = {}
    else:
        mat = pa.MatFS()
        mat.setDomain(dom)
        mat.build(kleType="element", opType="element")
        assert mat.getElementK() is mat.K and mat.getElementKrhs() is mat.Krhs and mat.getElementRw() is mat.Rw
        ops = {"K": mat.K, "Krhs": mat.Krhs, "Rw": mat.Rw}
    ops.update({nm: getattr(mat.getOperators(), nm) for nm in OPS})
    return dom, mat, ops


def _product(A, x):
    xv = A.createVecRight()
    xv.setArray(x)
    return (A * xv).getArray().copy()


def _refused(pa, fn):
    try:
        fn()
    except pa.Error as e:
        return e.ierr
    return 0


def _worker(rank, size, port, spec, q, transport):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), KLE_TRANSPORT=transport,
                      RANK=str(rank), WORLD_SIZE=str(size))
    import torch  # noqa: F401
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=size)
    try:
        import pynama_amd as pa
        dom, mat, ops = _build(pa, spec)
        mesh = dom.getMesh()
        dim = mesh.dim
        lo, hi = mesh.node_range
        dirn = np.zeros(hi - lo, bool)
        dirn[mesh.face_nodes(pa.mesh.FACES[dim]) - lo] = True
        res = {"rank": rank, "transport": pa.get_ctx().device_info()["transport"], "node_range": (lo, hi), "ops": {}}
        for nm, A in ops.items():
            assert A.getFormat() == "elem", nm
            xv = A.createVecRight()
            clo, chi = xv.getOwnershipRange()
            x = np.sin(np.arange(clo, chi, dtype=np.float64))
            y = _product(A, x)
            A.setHaloOverlap(False)
            y_plain = _product(A, x)
            A.setHaloOverlap(True)
            reps = [_product(A, x) for _ in range(3)]
            r = {"y": y, "plain_equal": y_plain.tobytes() == y.tobytes(),
                 "repeat_equal": all(v.tobytes() == y.tobytes() for v in reps),
                 "size": A.getSize(), "local": A.getLocalSize(), "rows": A.getOwnershipRange(), "cols": (clo, chi),
                 "left": A.createVecLeft().getLocalSize(), "kernel": A.spmvKernel(), "bytes": A.spmvBytes(),
                 "nz": A.getInfo()["nz_used"]}
            if nm == "K":
                xn = x.copy()
                xn[np.repeat(dirn, dim)] = np.nan  # (every rank's: the halo carries them into the ghosts)
                r["y_nan"] = _product(A, xn)
                r["diag"] = A.getDiagonal().getArray().copy()
            if nm == "Rw":
                r["y_nan"] = _product(A, np.full(chi - clo, np.nan))
            res["ops"][nm] = r
        res["dird"] = np.repeat(dirn, dim)
        if spec.get("solve"):
            sol = pa.KleSolver()
            sol.setMat(mat)
            sol.setUp()
            ksp = sol.getKSP()
            assert ksp.getOperators()[0] is mat.K
            if spec["solve"] != "cg":
                ksp.setType(spec["solve"])
            ksp.setTolerances(rtol=1e-11)
            f = pa.fields.get("taylor_green3d")
            vort = mat.Rw.createVecRight()
            vort.setArray(f.vorticity(dom.getFullCoordArray(), 1.0))
            vel = sol.getSolution()
            dom.applyBoundaryConditions(vel, "velocity", 0.0, 0.02)
            ubc = vel.getArray().copy()
            sol.solve(vort)
            res["solve"] = {"u": vel.getArray().copy(), "ubc": ubc, "its": ksp.getIterationNumber(),
                            "corr": ksp.getCorrectionIterations(), "true": ksp.getTrueRelativeResidual(),
                            "reason": ksp.getConvergedReason(), "range": vel.getOwnershipRange()}
        if spec.get("variants"):
            # every Krylov method and both preconditioners on the element-wise K:
            # K u = K xt, the true residual through the operator itself
            K = mat.K
            xt = K.createVecRight()
            xt.setArray(np.cos(np.arange(*xt.getOwnershipRange(), dtype=np.float64)))
            b = K * xt
            res["variants"] = {}
            for kt, pct in VARIANTS:
                ksp = pa.petsc.KSP().create()
                ksp.setType("cg" if kt == "cg_single_reduction" else kt)
                if kt.startswith("cg"):
                    ksp.setCGSingleReduction(kt == "cg_single_reduction")
                pc = pa.petsc.PC().create()
                pc.setType(pct)
                ksp.setPC(pc)
                ksp.setTolerances(rtol=VARIANT_RTOL, atol=0.0, max_it=100000)
                ksp.setOperators(K)
                ksp.setUp()
                u = K.createVecRight()
                ksp.solve(b, u)
                r = K * u
                r.aypx(-1.0, b)
                res["variants"][kt, pct] = {"reason": ksp.getConvergedReason(), "its": ksp.getIterationNumber(),
                                            "res": r.norm() / b.norm()}
        if spec.get("refusals"):
            from pynama_amd.mesh import UnstructuredMesh
            Mat = pa.petsc.Mat
            um = UnstructuredMesh.from_gmsh(os.path.join(G, "test.msh"), 3, rank, size, partitioner="inertial")
            res["refused"] = {"gmsh_kle": _refused(pa, lambda: Mat.createKLEElement(um, "K")),
                              "gmsh_op": _refused(pa, lambda: Mat.createOperatorElement(um, "Curl"))}
        q.put(res)
    except Exception:  # report instead of hanging the peers
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc()})
    finally:
        dist.destroy_process_group()


def _collect(procs, q, size, timeout=100):
    """Start the ranks and gather their results; the first rank that reports
    an error fails the test at once (its peers are killed, not waited for)."""
    import queue
    import time
    for p in procs:
        p.start()
    res = []
    t_end = time.time() + timeout
    try:
        while len(res) < size:
            try:
                r = q.get(timeout=2)
            except queue.Empty:
                missing = sorted(set(range(size)) - {x["rank"] for x in res})
                dead = [(i, procs[i].exitcode) for i in missing if procs[i].exitcode is not None]
                assert not dead, f"ranks died without a result (rank, exit code): {dead}"
                assert time.time() < t_end, f"ranks {missing} sent nothing within {timeout} s"
                continue
            assert "error" not in r, f"rank {r['rank']}: {r['error']}"
            res.append(r)
    except BaseException:
        for p in procs:
            p.kill()
        raise
    for p in procs:
        p.join(timeout=60)
    return sorted(res, key=lambda r: r["rank"])


def _spawn(target, size, args):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, size, port) + args(q)) for r in range(size)]
    return _collect(procs, q, size)


@functools.lru_cache(maxsize=None)
def _run(name, transport="host"):
    spec = SHAPES[name]
    return _spawn(_worker, spec["size"], lambda q: (spec, q, transport))


def _cat(res, nm, key="y"):
    return np.concatenate([r["ops"][nm][key] for r in res])


def _long_mult(indptr, indices, data, x):
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    out = np.zeros(len(indptr) - 1, np.longdouble)
    np.add.at(out, rows, np.asarray(data).astype(np.longdouble) * x[indices].astype(np.longdouble))
    return out


class Ref:
    """One shape on one rank, in the parent: the one-rank products of the same
    element-wise operators, the long double references and the bounds;
    computed once and left unchanged."""

    def __init__(self, name):
        import pynama_amd as pa
        from pynama_amd._lib import call
        pa.load()
        self.spec = spec = SHAPES[name]
        nelem, ngl = spec["nelem"], spec["ngl"]
        self.dim = dim = len(nelem)
        dw, ds = (1, 3) if dim == 2 else (3, 6)
        self.shape = {"K": (dim, dim), "Krhs": (dim, dim), "Rw": (dim, dw), "Curl": (dw, dim), "SrT": (ds, dim),
                      "DivSrT": (dim, ds)}
        self.dom, self.mat, self.ops = dom, mat, ops = _build(pa, spec)
        mesh = dom.getMesh()
        self.N, E, nn = mesh.N, mesh.E, ngl ** dim
        N = self.N
        self.x = {nm: np.sin(np.arange(N * self.shape[nm][1], dtype=np.float64)) for nm in _names(spec)}
        self.y = {nm: _product(ops[nm], self.x[nm]) for nm in _names(spec)}
        conn = mesh.conn()
        dirn = np.zeros(N, bool)
        dirn[mesh.face_nodes(pa.mesh.FACES[dim])] = True
        self.dird = dird = np.repeat(dirn, dim)
        self.ref, self.bound, self.delta = {}, {}, {}
        if "bc" not in spec:
            self.diag = ops["K"].getDiagonal().getArray().copy()
            # element matrices of the one-rank mesh: K_e0, Rw_e0 and the deltas
            nd, nc = dim * nn, dw * nn
            ctx = pa.get_ctx()
            Ke, Rwe = np.zeros((nd, nd)), np.zeros((nd, nc))
            call("kle_element_kle", ctx.h, mesh._h, 0, Ke, Rwe)
            K0, R0 = Ke.copy(), Rwe.copy()
            dK = dR = 0.0
            for e in range(1, E):
                call("kle_element_kle", ctx.h, mesh._h, e, Ke, Rwe)
                dK = max(dK, np.abs(Ke - K0).max() / np.abs(K0).max())
                dR = max(dR, np.abs(Rwe - R0).max() / np.abs(R0).max())
            self.delta.update(K=dK, Krhs=dK, Rw=dR)
            gd = (conn[:, :, None] * dim + np.arange(dim)[None, None, :]).reshape(E, nd)
            gw = (conn[:, :, None] * dw + np.arange(dw)[None, None, :]).reshape(E, nc)
            # the oracle's assembled system on the same numbering
            om = O.BoxMesh(dim, nelem, [0] * dim, [1] * dim, ngl)
            self.om = om
            self.okle = dict(zip(KLE, om.assemble_fs(dirn.astype(np.uint8))))
            for nm in KLE:
                A = self.okle[nm]
                x = self.x[nm]
                self.ref[nm] = _long_mult(A.indptr, A.indices, A.data, x)
                M0, gc = (R0, gw) if nm == "Rw" else (K0, gd)
                if nm == "Rw":
                    xe = np.abs(x)[gc]
                else:
                    keep = ~dird if nm == "K" else dird
                    xe = np.where(keep[gc], np.abs(x)[gc], 0.0)
                B, X = np.zeros(N * dim), np.zeros(N * dim)
                np.add.at(B, gd, xe @ np.abs(M0).T)
                np.add.at(X, gd, np.broadcast_to(xe.sum(axis=1)[:, None], gd.shape))
                B = np.where(dird, 0.0 if nm == "Rw" else np.maximum(B, np.abs(x)), B)
                n = (dw if nm == "Rw" else dim) * nn + 8
                self.bound[nm] = n * EPS * B + self.delta[nm] * np.abs(M0).max() * X
        # the collocation operators: assembled on one rank, the oracle's element matrices
        asm = (pa.MatNS if "bc" in spec else pa.MatFS)()
        asm.setDomain(dom)
        asm.build(buildKLE=False)
        el = O.Element(ngl, dim)
        om = O.BoxMesh(dim, nelem, [0] * dim, [1] * dim, ngl)
        perm = np.array([np.where(conn[0] == c)[0][0] for c in om.conn()[0]])
        corners = mesh.corners()

        def elops(e):
            SrT, Div, Curl, W = el.ops(corners[e].ravel())
            out = {}
            for nm, M in (("Curl", Curl), ("SrT", SrT), ("DivSrT", Div)):
                R, C = self.shape[nm]
                pr = (perm[:, None] * R + np.arange(R)[None, :]).ravel()
                pc = (perm[:, None] * C + np.arange(C)[None, :]).ravel()
                T = np.zeros_like(M)
                T[np.ix_(pr, pc)] = M
                out[nm] = T
            c = np.zeros(nn)
            c[perm] = W
            return out, c

        with ThreadPoolExecutor(max_workers=8) as pool:
            every = list(pool.map(elops, range(E)))
        M0, c0 = every[0]
        self.delta_w = 0.0
        for nm in OPS:
            self.delta[nm] = 0.0
        for Me, ce in every[1:]:
            for nm in OPS:
                self.delta[nm] = max(self.delta[nm], np.abs(Me[nm] - M0[nm]).max() / np.abs(M0[nm]).max())
            self.delta_w = max(self.delta_w, np.abs(ce - c0).max() / np.abs(c0).max())
        W = np.zeros(N)
        np.add.at(W, conn, np.broadcast_to(c0[None, :], conn.shape))
        for nm in OPS:
            R, C = self.shape[nm]
            x = self.x[nm]
            gr = (conn[:, :, None] * R + np.arange(R)[None, None, :]).reshape(E, nn * R)
            gc = (conn[:, :, None] * C + np.arange(C)[None, None, :]).reshape(E, nn * C)
            xe = np.abs(x)[gc]
            B, X = np.zeros(N * R), np.zeros(N * R)
            np.add.at(B, gr, xe @ np.abs(M0[nm]).T)
            np.add.at(X, gr, np.broadcast_to(xe.sum(axis=1)[:, None], gr.shape))
            wi = np.repeat(1.0 / W, R)
            B *= wi
            n = C * (dim * (ngl - 1) + 1) + 2 ** dim + 8
            self.bound[nm] = n * EPS * B + self.delta[nm] * np.abs(M0[nm]).max() * X * wi + 2 * self.delta_w * B
            self.ref[nm] = _long_mult(*getattr(asm.getOperators(), nm).getValuesCSR(), x)


@functools.lru_cache(maxsize=None)
def _ref(name):
    return Ref(name)


# ------------------------------------------------------------ 1. the products
@pytest.mark.parametrize("name", list(SHAPES))
def test_products_on_ranks(name):
    spec = SHAPES[name]
    res = _run(name)
    ref = _ref(name)
    assert [r["transport"] for r in res] == ["host"] * spec["size"]
    assert res[0]["node_range"][0] == 0 and res[-1]["node_range"][1] == ref.N
    assert all(a["node_range"][1] == b["node_range"][0] for a, b in zip(res, res[1:]))
    assert ref.delta_w <= 2e-12, f"element weights differ over the mesh: delta_w = {ref.delta_w:.3e}"
    for nm in _names(spec):
        R, C = ref.shape[nm]
        for r in res:
            o, (lo, hi) = r["ops"][nm], r["node_range"]
            # the layout: sizes, ownership and the vectors the matrix makes
            assert o["size"] == (ref.N * R, ref.N * C), (nm, r["rank"])
            assert o["local"] == ((hi - lo) * R, (hi - lo) * C), (nm, r["rank"])
            assert o["rows"] == (lo * R, hi * R) and o["cols"] == (lo * C, hi * C), (nm, r["rank"])
            assert o["left"] == (hi - lo) * R and o["nz"] == 0 and o["bytes"] > 0, (nm, r["rank"])
            assert ("k_elem_gemm" if nm in KLE else "k_colloc_elem") in o["kernel"], o["kernel"]
            # 3. both schedules and three repeated products give the same bits
            assert o["plain_equal"], (nm, r["rank"])
            assert o["repeat_equal"], (nm, r["rank"])
        # 1. the owned rows are the one-rank product's, bit for bit
        y = _cat(res, nm)
        assert y.shape == ref.y[nm].shape
        diff = np.nonzero(y != ref.y[nm])[0]
        assert y.tobytes() == ref.y[nm].tobytes(), (nm, len(diff), diff[:8].tolist())
        # 2. the error bound
        assert ref.delta[nm] <= 2e-12, f"{nm}: element matrices differ over the mesh: delta = {ref.delta[nm]:.3e}"
        err = np.abs(y.astype(np.longdouble) - ref.ref[nm]).astype(np.float64)
        b = ref.bound[nm]
        worst = float(np.max(err / np.where(b > 0, b, 1.0)))
        print(f"{name} {nm}: delta {ref.delta[nm]:.2e}  max err/bound {worst:.3g}")
        assert np.all(err <= b), (name, nm, worst)
        assert np.any(y != 0.0), nm


@pytest.mark.parametrize("name", [n for n in SHAPES if "bc" not in SHAPES[n]])
def test_masking_and_diagonal_on_ranks(name):
    res = _run(name)
    ref = _ref(name)
    dird = np.concatenate([r["dird"] for r in res])
    np.testing.assert_array_equal(dird, ref.dird)
    # 4. selection, not multiplication.  K: NaN in every Dirichlet entry of x
    # (ghosts included) reaches no free row; the Dirichlet rows are y_i = x_i
    yk, yn = _cat(res, "K"), _cat(res, "K", "y_nan")
    assert not np.any(np.isnan(yn[~dird]))
    assert yn[~dird].tobytes() == yk[~dird].tobytes()
    assert np.all(np.isnan(yn[dird]))
    # Rw: an all-NaN w leaves the Dirichlet rows exactly 0.0
    yr = _cat(res, "Rw", "y_nan")
    np.testing.assert_array_equal(yr[dird], np.zeros(int(dird.sum())))
    assert not np.any(np.signbit(yr[dird]))
    assert np.all(np.isnan(yr[~dird]))
    # 5. the diagonal of K
    dg = _cat(res, "K", "diag")
    assert dg.tobytes() == ref.diag.tobytes()
    assert np.all(dg[dird] == 1.0)


def test_ipc_transport_same_bits():
    """6. KLE_TRANSPORT=ipc: the owned rows are the host transport's bit for
    bit (the product does not depend on how its halo travels)."""
    name = "r3_2x3x3_p3"
    res, host = _run(name, "ipc"), _run(name)
    assert [r["transport"] for r in res] == ["ipc"] * 3
    for nm in KLE + OPS:
        assert _cat(res, nm).tobytes() == _cat(host, nm).tobytes(), nm
        for r in res:
            assert r["ops"][nm]["plain_equal"] and r["ops"][nm]["repeat_equal"], (nm, r["rank"])
    assert _cat(res, "K", "diag").tobytes() == _cat(host, "K", "diag").tobytes()


# ----------------------------------------------------------------- 2. the solve
@pytest.mark.parametrize("name", [n for n in SHAPES if SHAPES[n].get("solve")])
def test_matrix_free_solve_on_ranks(name):
    """MatFS.build(kleType="element") + KleSolver on Taylor-Green at rtol
    1e-11, checked as test_gpu_multirank.py::_check_box_run checks the
    assembled path; the Dirichlet entries of u are u_bc bit for bit."""
    import pynama_amd as pa
    spec = SHAPES[name]
    ksp_type = spec["solve"]
    res = _run(name)
    ref = _ref(name)
    om, (K, Kr, Rw) = ref.om, (ref.okle[nm] for nm in KLE)
    coords = om.coords()
    bn = np.nonzero(ref.dird[::3])[0]
    f = pa.fields.get("taylor_green3d")
    vel0 = np.zeros(om.N * 3)
    idx = (bn[:, None] * 3 + np.arange(3)).ravel()
    vel0[idx] = f.velocity(coords[bn], 1.0)
    b = Rw.mult(f.vorticity(coords, 1.0)) + Kr.mult(vel0)
    xs, its, _ = K.cg(b, rtol=1e-11)
    sv = [r["solve"] for r in res]
    u = np.concatenate([s["u"] for s in sv])
    ubc = np.concatenate([s["ubc"] for s in sv])
    assert sv[0]["range"][0] == 0 and sv[-1]["range"][1] == len(xs)
    rel = np.linalg.norm(u - xs) / np.linalg.norm(xs)
    print(f"{name} {ksp_type}: |u - x_serial| / |x_serial| {rel:.3e}  iterations "
          f"{[s['its'] - s['corr'] for s in sv]} (oracle {its})  true residual {max(s['true'] for s in sv):.3e}")
    assert rel <= 1e-8
    tol = 3 if ksp_type == "cg" else 6
    for s in sv:
        assert s["reason"] > 0, s["reason"]
        assert -tol <= s["its"] - s["corr"] - its <= tol, (s["its"], s["corr"], its)
        assert s["true"] <= 1e-11, s["true"]
    d = ref.dird
    assert np.any(ubc[d] != 0.0)
    assert u[d].tobytes() == ubc[d].tobytes()


def test_krylov_variants_on_ranks():
    """cg (classic and single reduction), pipecg and gmres with PC none and
    jacobi on the element-wise K of 3 ranks."""
    res = _run("r3_2x3x3_p3")
    d = _cat(res, "K", "diag")
    assert d.min() > 0.0
    for key in VARIANTS:
        v = [r["variants"][key] for r in res]
        bound = 2 * VARIANT_RTOL * (d.max() / d.min() if key == ("gmres", "jacobi") else 1.0)
        print(f"{key}: iterations {v[0]['its']}  true residual {v[0]['res']:.3e}  bound {bound:.3e}")
        for a in v:
            assert a["reason"] > 0, (key, a["reason"])
            assert a["res"] <= bound, (key, a["res"], bound)
            assert a["its"] == v[0]["its"] and a["res"] == v[0]["res"], key  # (allreduced: the same on every rank)


# --------------------------------------------------------------- 3. evalRHS
EVAL_SPEC = dict(nelem=[3, 2, 4], ngl=4)


def _eval_rhs(pa):
    from pynama_amd.petsc import Options
    spec = EVAL_SPEC
    tg = {"custom-func": {"name": "taylor_green3d"}}
    cfg = {"name": "tg", "material-properties": {"rho": 0.5, "mu": 0.01},
           "domain": {"ngl": spec["ngl"], "box-mesh": {"nelem": spec["nelem"], "lower": [0, 0, 0],
                                                       "upper": [1, 1, 1]}},
           "boundary-conditions": tg, "initial-conditions": tg}
    opts = Options()
    opts.setValue("kle_mat_type", "element")
    opts.setValue("kle_op_type", "element")
    try:
        prob = pa.BaseProblem(cfg)
        prob.setUp()
        prob.setUpSolver()
    finally:
        opts.delValue("kle_mat_type")
        opts.delValue("kle_op_type")
    for A in (prob.mat.K, prob.mat.Krhs, prob.mat.Rw, prob.operator.Curl, prob.operator.SrT, prob.operator.DivSrT):
        assert A.getFormat() == "elem", A.getName()
    prob.solverKLE.getKSP().setTolerances(rtol=1e-13)
    f = prob.operator.Curl.createVecLeft()
    prob.evalRHS(None, 0.25, prob.vort, f)
    return f.getArray().copy(), f.getOwnershipRange()


def _eval_worker(rank, size, port, q):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), KLE_TRANSPORT="host",
                      RANK=str(rank), WORLD_SIZE=str(size))
    import torch  # noqa: F401
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=size)
    try:
        import pynama_amd as pa
        fa, rng = _eval_rhs(pa)
        q.put({"rank": rank, "f": fa, "range": rng})
    except Exception:
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc()})
    finally:
        dist.destroy_process_group()


def test_eval_rhs_on_two_ranks():
    """-kle_mat_type element -kle_op_type element: the whole evalRHS on 2 ranks
    against the one-rank run of the same options, 1e-8 relative (the solves
    differ by allreduce rounding, the operators do not)."""
    import pynama_amd as pa
    pa.load()
    res = _spawn(_eval_worker, 2, lambda q: (q,))
    one, rng = _eval_rhs(pa)
    two = np.concatenate([r["f"] for r in res])
    assert res[0]["range"][0] == 0 and res[0]["range"][1] == res[1]["range"][0] and res[1]["range"][1] == rng[1]
    assert np.any(one != 0.0)
    rel = np.linalg.norm(two - one) / np.linalg.norm(one)
    print(f"evalRHS 2 ranks vs 1: relative difference {rel:.3e}")
    assert rel <= 1e-8


# ---------------------------------------------------------------- 4. refusals
def test_refusals_on_ranks():
    import pynama_amd as pa
    pa.load()
    Mat = pa.petsc.Mat
    # a mesh partitioned for two ranks in a one-rank context
    half = pa.BoxMesh(3, [2, 2, 2], [0, 0, 0], [1, 1, 1], 3, rank=0, nranks=2)
    half.set_dirichlet_faces(pa.mesh.FACES[3])
    for which in KLE:
        assert _refused(pa, lambda: Mat.createKLEElement(half, which)) == 56, which
    for which in OPS:
        assert _refused(pa, lambda: Mat.createOperatorElement(half, which)) == 56, which
    # a Gmsh mesh on two ranks
    for r in _run("r2_3x2x4_p4"):
        assert r["refused"] == {"gmsh_kle": 56, "gmsh_op": 56}, r["rank"]
    # no-slip KLE matrices have no element-wise form
    cav = pa.Domain()
    cav.configure(_cfg(SHAPES["r2_2d_cavity"]))
    cav.setUp()
    ns = pa.MatNS()
    ns.setDomain(cav)
    assert _refused(pa, lambda: ns.build(kleType="element")) == 56
    assert _refused(pa, lambda: Mat.createKLEElement(cav.getMesh(), "K")) == 56
