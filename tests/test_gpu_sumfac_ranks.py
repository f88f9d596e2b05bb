"""The sum-factorised K, Krhs, Rw (kle_sumfac.hip) and the per-element-geometry
Curl, SrT, DivSrT (kle_colloc.hip, geo) on partitioned meshes: Gmsh slab and
inertial partitions and box slabs, all ranks on one GPU.

Ranks are spawned as tests/test_gpu_sym_ranks_ref.py does (torch.multiprocessing
spawn, gloo, every worker under _collect's time limit); one spawned run per
configuration and one of the same mesh on one rank, cached and shared by the
assertions.  The parent never opens the GPU: the host meshes, the partitions,
the inputs, the conditions on the configurations and the references are formed
on the CPU (tests/sumfac_ranks_ref.py: CONFIGS, conditions).

References: tests/sumfac_ref.py (K, Krhs, the diagonal) and
tests/sumfac_ops_ref.py (Rw, Curl, SrT, DivSrT), the longdouble sums and derived
bounds of the one-rank tests, formed on the global one-rank mesh; rank rows are
mapped into it by oracle.node_map on coordinates (Gmsh partitions number their
nodes by owner).  3-D ngl 7: sumfac_ref.sample_nodes' rows, as on one rank.

a. Products: mult of the six operators on two different x in turn (a stale halo
   fails the second): every owned row inside the reference's bound, the
   stitched rows bit-equal to the one-rank product of the same operator,
   multAdd = y0 + the product's bits rounded once, halo overlap on / off and
   three repeats the same bits.  Worst error / bound per configuration printed
   (SUMFAC-RANKS lines; DESIGN.md records them).
b. Selection: NaN in every Dirichlet entry of x on every rank (so it arrives in
   ghost slots) leaves every free row of K bit-equal; Krhs likewise with NaN in
   the free entries; Rw's Dirichlet rows are +0.0 in bytes.
c. getDiagonal of K and Krhs: the one-rank diagonal's owned rows bit for bit.
d. Solves: the Krylov variants of test_gpu_elem_ranks.VARIANTS with its bound
   on the true residual formed through the operator; KleSolver with
   -kle_k_type sumfac on 2 and 3 ranks against the same code on one rank at
   1e-8 relative, the figure of test_gpu_elem_ranks.py's comparisons; one
   BaseProblem.evalRHS with kleType = opType = "sumfac" on 2 ranks of test.msh
   against the one-rank matrix-free evalRHS, 1e-8 relative (its figure for f).
e. Refusals: Error 56 for a mesh partitioned for another rank count, a no-slip
   mesh, stored-value calls, copyDirichletRows and PC lu; names and getInfo as
   documented.
f. timeLocalSpmv on ranks (3 inertial ranks, 2 box slabs), every rank in turn:
   the six partitioned operators (both lists, no halo) and a rank's part of
   the assembled Rw and K (node-block; graph symmetric storage on the Gmsh
   partition) return a positive time and leave the next mult's bits alone; the
   box symmetric tiles are refused with Error 62.

inertial2_p6: the issue asks for empty inner lists on every rank.  A node
belongs to the highest rank whose cells touch it, so the last rank's own cells
read owned nodes alone on any mesh; the condition asserted is that every other
rank's inner list is empty (sumfac_ranks_ref.conditions)."""
import os

import numpy as np
import pytest

import elem_ref as R
import sumfac_ops_ref as SO
import sumfac_ranks_ref as SR
import sumfac_ref as SF
import test_gpu_sym_ranks_ref as SRK
from test_gpu_elem_ranks import VARIANT_RTOL, VARIANTS

pytestmark = pytest.mark.gpu
KLE = ("K", "Krhs", "Rw")
OPS = SO.OPS
NAMES = KLE + OPS
CAVITY = {"up": [2, 0], "down": [0, 0], "left": [0, 0], "right": [0, 0]}
LOCAL_TIMING = ("inertial3_p2", "box2_p3")  # a graph partition; box slabs, whose symmetric tiles refuse
_RUNS, _PARTS, _REFS = {}, {}, {}


def _shape(dim, nm):
    dw = 1 if dim == 2 else 3
    return {"K": (dim, dim), "Krhs": (dim, dim), "Rw": (dim, dw)}.get(nm) or SO.op_shape(dim, nm)


def _domain_cfg(cfg, msh):
    dim = SR.dim_of(cfg)
    tg = {"custom-func": {"name": "taylor_green3d" if dim == 3 else "taylor_green"}}
    if msh is not None:
        d = {"ngl": cfg["ngl"], "gmsh-file": msh}
        if cfg["size"] > 1:
            d["partitioner"] = cfg["part"]
    else:
        d = {"ngl": cfg["ngl"], "box-mesh": {"nelem": cfg["box"], "lower": [0] * dim, "upper": [1] * dim}}
    return {"name": "sumfac_ranks", "material-properties": {"rho": 0.5, "mu": 0.01}, "domain": d,
            "boundary-conditions": tg, "initial-conditions": tg}


def _refused(pa, fn):
    try:
        fn()
    except pa.Error as e:
        return e.ierr
    return 0


def _product(A, x, add=None):
    xv = A.createVecRight()
    lo, hi = xv.getOwnershipRange()
    xv.setArray(x[lo:hi])
    if add is None:
        return (A * xv).getArray().copy()
    yv, zv = A.createVecLeft(), A.createVecLeft()
    rlo, rhi = yv.getOwnershipRange()
    yv.setArray(add[rlo:rhi])
    A.multAdd(xv, yv, zv)
    return zv.getArray().copy()


def _local_timing(pa, dist, rank, size, dom, ops, cfg):
    """timeLocalSpmv, every rank in turn behind barriers: the partitioned
    sum-factorised operators (both element lists, no halo) and this rank's
    part of the assembled K (graph symmetric storage, then plain node-block)
    and Rw.  Each returns a positive time and leaves the next mult's bits as
    they were."""
    asm = pa.MatFS()
    asm.setDomain(dom)
    asm.build(buildOperators=False)
    res = {}

    def check(tag, A, nm):
        x = cfg["x"][nm][0]
        before = _product(A, x)
        xv, yv = A.createVecRight(), A.createVecLeft()
        lo, hi = xv.getOwnershipRange()
        xv.setArray(x[lo:hi])
        ms = refused = None
        for t in range(size):
            dist.barrier()
            if t == rank:
                try:
                    ms = A.timeLocalSpmv(xv, yv, 3)
                except pa.Error as e:
                    refused = e.ierr
        dist.barrier()
        res[tag] = {"ms": ms, "refused": refused, "same": _product(A, x).tobytes() == before.tobytes(),
                    "kernel": A.spmvKernel(), "finite": bool(np.isfinite(yv.getArray()).all())}

    for nm in NAMES:
        check("sumfac_" + nm, ops[nm], nm)
    check("assembled_Rw", asm.Rw, "Rw")
    asm.K.setOption(asm.K.Option.SPD, False)
    check("assembled_K_nb", asm.K, "K")
    # symmetric storage: the graph groups / bricks of a Gmsh partition; on box slabs the 128-row tiles
    # (bricks off), whose local product is refused
    keep = pa.runtime.get_tuning("spmv_sym_brick")
    pa.runtime.set_tuning("spmv_sym_brick", 0)
    try:
        asm.K.setOption(asm.K.Option.SPD, True)
        res["sym"] = asm.K.isSymmetricStorage()
        check("assembled_K_sym", asm.K, "K")
    finally:
        pa.runtime.set_tuning("spmv_sym_brick", keep)
    return res


def _worker(rank, size, port, cfg, msh, q):
    dist = SRK.rank_setup(rank, size, port, cfg)
    try:
        import pynama_amd as pa
        from pynama_amd.petsc import Options
        dcfg = _domain_cfg(cfg, msh)
        dom = pa.Domain()
        dom.configure(dcfg)
        dom.setUp()
        mesh = dom.getMesh()
        dim = mesh.dim
        mat = pa.MatFS()
        mat.setDomain(dom)
        mat.build(kleType="sumfac", opType="sumfac")
        assert mat.getSumFactoredK() is mat.K and mat.getSumFactoredRw() is mat.Rw
        ops = {"K": mat.K, "Krhs": mat.Krhs, "Rw": mat.Rw}
        ops.update({nm: getattr(mat.getOperators(), nm) for nm in OPS})
        lo, hi = mesh.node_range
        dirn = np.zeros(hi - lo, bool)
        dirn[mesh.face_nodes(pa.mesh.FACES[dim]) - lo] = True
        out = {"rank": rank, "transport": pa.get_ctx().device_info()["transport"], "node_range": (lo, hi),
               "coords": mesh.coords(), "dirn": dirn, "ops": {}}
        for nm, A in ops.items():
            R_, C_ = _shape(dim, nm)
            xs, y0 = cfg["x"][nm], cfg["y0"][nm]
            r = {"y": [], "z": [], "plain_equal": True, "repeat_equal": True, "format": A.getFormat(),
                 "size": A.getSize(), "local": A.getLocalSize(), "rows": A.getOwnershipRange(),
                 "cols": A.createVecRight().getOwnershipRange(), "left": A.createVecLeft().getLocalSize(),
                 "kernel": A.spmvKernel(), "bytes": A.spmvBytes(), "info": A.getInfo()}
            for x in xs:  # in turn: the second product finds the first's ghosts in place
                A.setHaloOverlap(True)
                y = _product(A, x)
                r["y"].append(y)
                r["z"].append(_product(A, x, y0))
                A.setHaloOverlap(False)
                r["plain_equal"] &= _product(A, x).tobytes() == y.tobytes()
                A.setHaloOverlap(True)
                r["repeat_equal"] &= all(_product(A, x).tobytes() == y.tobytes() for _ in range(3))
            x = xs[1]
            dfull = np.repeat(cfg["dirflag"], dim)  # (this run's numbering)
            if nm in ("K", "Krhs"):
                xn = x.copy()
                xn[dfull if nm == "K" else ~dfull] = np.nan  # (every rank's: the halo carries them into the ghosts)
                r["y_nan"] = _product(A, xn)
                r["diag"] = A.getDiagonal().getArray().copy()
            if nm == "Rw":
                r["y_nan"] = _product(A, np.full(len(x), np.nan))
            out["ops"][nm] = r
        if cfg.get("variants"):
            K = mat.K
            xt = K.createVecRight()
            xt.setArray(np.cos(np.arange(*xt.getOwnershipRange(), dtype=np.float64)))
            b = K * xt
            out["variants"] = {}
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
                res = K * u
                res.aypx(-1.0, b)
                out["variants"][kt, pct] = {"reason": ksp.getConvergedReason(), "its": ksp.getIterationNumber(),
                                            "res": res.norm() / b.norm()}
        if cfg.get("solve"):
            opts = Options()
            opts.setValue("kle_k_type", "sumfac")
            try:
                sol = pa.KleSolver()
                sol.setMat(mat)
                sol.setUp()
            finally:
                opts.delValue("kle_k_type")
            ksp = sol.getKSP()
            assert ksp.getOperators()[0] is mat.getSumFactoredK()
            ksp.setTolerances(rtol=1e-11)
            f = pa.fields.get("taylor_green3d")
            vort = mat.Rw.createVecRight()
            vort.setArray(f.vorticity(dom.getFullCoordArray(), 1.0))
            vel = sol.getSolution()
            dom.applyBoundaryConditions(vel, "velocity", 0.0, 0.02)
            sol.solve(vort)
            out["solve"] = {"u": vel.getArray().copy(), "its": ksp.getIterationNumber(),
                            "reason": ksp.getConvergedReason(), "true": ksp.getTrueRelativeResidual()}
        if cfg.get("eval_rhs"):
            opts = Options()
            opts.setValue("kle_mat_type", "sumfac")
            opts.setValue("kle_op_type", "sumfac")
            try:
                prob = pa.BaseProblem(dcfg)
                prob.setUp()
                prob.setUpSolver()
            finally:
                opts.delValue("kle_mat_type")
                opts.delValue("kle_op_type")
            for A in (prob.mat.K, prob.mat.Krhs, prob.mat.Rw, prob.operator.Curl, prob.operator.SrT,
                      prob.operator.DivSrT):
                assert A.getFormat() == "elem" and A.getInfo()["nz_used"] == 0, A.getName()
            prob.solverKLE.getKSP().setTolerances(rtol=1e-13)
            fv = prob.operator.Curl.createVecLeft()
            prob.evalRHS(None, 0.25, prob.vort, fv)
            out["eval"] = {"f": fv.getArray().copy(), "range": tuple(fv.getOwnershipRange())}
        if cfg.get("local_timing"):
            out["local"] = _local_timing(pa, dist, rank, size, dom, ops, cfg)
        if cfg.get("refusals"):
            Mat = pa.petsc.Mat
            other = pa.BoxMesh(3, [2, 2, 6], [0, 0, 0], [1, 1, 1], 3, rank=rank, nranks=size + 1)
            other.set_dirichlet_faces(pa.mesh.FACES[3])
            cav = pa.Domain()
            cav.configure({"domain": {"ngl": 3, "box-mesh": {"nelem": [4, 4], "lower": [0, 0], "upper": [1, 1]}},
                           "boundary-conditions": {"no-slip": CAVITY}})
            cav.setUp()
            K = mat.K
            v = K.createVecLeft()

            def lu():
                ksp = pa.petsc.KSP().create()
                p = pa.petsc.PC().create()
                p.setType("lu")
                ksp.setPC(p)
                ksp.setOperators(K)
                ksp.setUp()

            ref = {"other_count_K": lambda: Mat.createKLESumFactored(other, "K"),
                   "other_count_Rw": lambda: Mat.createRwSumFactored(other),
                   "other_count_Curl": lambda: Mat.createOperatorSumFactored(other, "Curl"),
                   "noslip_K": lambda: Mat.createKLESumFactored(cav.getMesh(), "K"),
                   "noslip_Rw": lambda: Mat.createRwSumFactored(cav.getMesh()),
                   "csr": K.getValuesCSR, "convert": K.convert, "row": lambda: K.getRow(K.getOwnershipRange()[0]),
                   "spd": lambda: K.setOption(K.Option.SPD, True), "scale": lambda: K.diagonalScale(v),
                   "copy_dirichlet": lambda: K.copyDirichletRows(v, K.createVecLeft()), "lu": lu,
                   "rw_diag": lambda: mat.Rw.getDiagonal(),
                   "op_ksp": lambda: pa.petsc.KSP().create().setOperators(mat.getOperators().Curl)}
            out["refused"] = {k: _refused(pa, fn) for k, fn in ref.items()}
            x = cfg["x"]["K"][0]
            out["after"] = _product(K, x).tobytes() == out["ops"]["K"]["y"][0].tobytes()
        q.put(out)
    except Exception:  # report instead of hanging the peers
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc()})
    finally:
        dist.destroy_process_group()


def _msh(name, tmp_path_factory):
    if "dir" not in _PARTS:
        _PARTS["dir"] = tmp_path_factory.mktemp("sumfac_ranks")
    return SR.mesh_file(SR.CONFIGS[name], _PARTS["dir"])


def _partition(name, tmp_path_factory):
    """The host partition of a configuration with its conditions asserted (CPU)."""
    cfg = SR.CONFIGS[name]
    key = cfg.get("host", name)
    if key not in _PARTS:
        P = SR.Partition(cfg, _msh(name, tmp_path_factory))
        P.cond = SR.conditions(key, P)
        rng = np.random.default_rng(20241021)
        P.x = {nm: [rng.uniform(-1, 1, P.N * _shape(P.dim, nm)[1]) for _ in range(2)] for nm in NAMES}
        P.y0 = {nm: rng.uniform(-1, 1, P.N * _shape(P.dim, nm)[0]) for nm in NAMES}
        _PARTS[key] = P
    return _PARTS[key]


def _run(name, tmp_path_factory, one=False):
    """The spawned run of a configuration, or of its mesh on one rank (inputs
    in that run's numbering)."""
    cfg = SR.CONFIGS[name]
    P = _partition(name, tmp_path_factory)
    key = ("one", cfg.get("host", name)) if one else name
    if key not in _RUNS:
        c = dict(cfg)
        if one:
            c.update(size=1, transport="host", refusals=False)
            c["x"] = {nm: [P.to_one(x, _shape(P.dim, nm)[1]) for x in xs] for nm, xs in P.x.items()}
            c["y0"] = {nm: P.to_one(y, _shape(P.dim, nm)[0]) for nm, y in P.y0.items()}
            c["dirflag"] = P.one_dir
        else:
            c.update(x=P.x, y0=P.y0, dirflag=P.dirflag, refusals=name == "slab2_p2",
                     local_timing=name in LOCAL_TIMING)
        res = SRK.spawn(_worker, c, _msh(name, tmp_path_factory))
        assert one or all(r["transport"] == c.get("transport", "host") for r in res)
        if not one:  # the workers' partition is the host's
            assert [r["node_range"] for r in res] == P.ranges
            assert np.array_equal(np.concatenate([r["coords"] for r in res]), P.coords)
            assert np.array_equal(np.concatenate([r["dirn"] for r in res]), P.dirflag)
        _RUNS[key] = res
    return _RUNS[key]


def _reference(name, tmp_path_factory):
    """Per operator and x: the longdouble reference with its bound, in the
    one-rank numbering; computed once and left unchanged."""
    P = _partition(name, tmp_path_factory)
    key = SR.CONFIGS[name].get("host", name)
    if key not in _REFS:
        dim, ngl, conn, corners, dirn = P.dim, P.ngl, P.one_conn, P.one_corners, P.one_dir
        nodes = SF.sample_nodes(conn, ngl, dim, dirn) if dim == 3 and ngl >= 7 else None
        ref = {}
        for nm in NAMES:
            ref[nm] = []
            for x in P.x[nm]:
                xo = P.to_one(x, _shape(dim, nm)[1])
                if nm in ("K", "Krhs"):
                    r = SF.reference(dim, ngl, conn, corners, dirn, nm, xo, nodes=nodes, diag=False)
                elif nm == "Rw":
                    r = SO.rw_reference(dim, ngl, conn, corners, dirn, xo, nodes=nodes)
                else:
                    r = SO.ops_reference(dim, ngl, conn, corners, nm, xo, nodes=nodes)
                ref[nm].append(r)
        _REFS[key] = ref
    return _REFS[key]


def _cat(res, nm, key, k=None):
    return np.concatenate([r["ops"][nm][key] if k is None else r["ops"][nm][key][k] for r in res])


# ---------------------------------------------------------------- a. products
@pytest.mark.parametrize("name", list(SR.CONFIGS))
def test_products_on_ranks(name, tmp_path_factory):
    cfg = SR.CONFIGS[name]
    P = _partition(name, tmp_path_factory)
    print(f"SUMFAC-RANKS {name}: neb {P.cond['neb']}  inner {P.cond['inner']}  outer {P.cond['outer']}  "
          f"peers {P.cond['peers']}")
    res = _run(name, tmp_path_factory)
    one = _run(name, tmp_path_factory, one=True)[0]
    ref = _reference(name, tmp_path_factory)
    dim = P.dim
    for nm in NAMES:
        R_, C_ = _shape(dim, nm)
        kern = {"K": f"k_sumfac_elem<{dim}>+k_sumfac_gather<{dim}>", "Krhs": f"k_sumfac_elem<{dim}>+k_sumfac_gather<{dim}>",
                "Rw": f"k_sumfac_rw<{dim}>+k_sumfac_gather_rw<{dim}>"}.get(
                    nm, f"k_colloc_elem<{dim},{nm},geo>+k_colloc_gather_csr<{R_}>")
        for r, (lo, hi) in zip(res, P.ranges):
            o = r["ops"][nm]
            # sizes, ownership, names and getInfo: as the box element-wise operators on ranks
            assert o["format"] == "elem" and o["kernel"] == kern == one["ops"][nm]["kernel"], (nm, o["kernel"])
            assert o["size"] == (P.N * R_, P.N * C_) and o["local"] == ((hi - lo) * R_, (hi - lo) * C_), (nm, r["rank"])
            assert o["rows"] == (lo * R_, hi * R_) and o["cols"] == (lo * C_, hi * C_), (nm, r["rank"])
            assert o["left"] == (hi - lo) * R_ and o["bytes"] > 0, (nm, r["rank"])
            assert o["info"]["format"] == "elem" and o["info"]["nz_used"] == 0 and o["info"]["spmv_bytes"] == o["bytes"]
            assert o["plain_equal"], (name, nm, r["rank"], "halo overlap on / off differ")
            assert o["repeat_equal"], (name, nm, r["rank"], "repeated products differ")
        worst = 0.0
        for k in range(2):
            y = _cat(res, nm, "y", k)
            yo = P.to_one(y, R_)
            y1 = one["ops"][nm]["y"][k]
            diff = np.nonzero(yo != y1)[0]
            assert yo.tobytes() == y1.tobytes(), (name, nm, k, len(diff), diff[:8].tolist())
            r = ref[nm][k]
            w, at = R.worst(yo[r.rows], r.y, r.bound)
            worst = max(worst, w)
            assert w <= 1.0, (name, nm, k, w, at)
            assert np.any(yo != 0.0)
            # multAdd: y0 + the product, rounded once
            z = _cat(res, nm, "z", k)
            assert z.tobytes() == (P.y0[nm] + y).tobytes(), (name, nm, k, "multAdd")
            assert P.to_one(z, R_).tobytes() == one["ops"][nm]["z"][k].tobytes()
        print(f"SUMFAC-RANKS {name} {nm}: worst err/bound {worst:.3g} over {len(ref[nm][0].rows)} rows x 2 inputs")


def test_ipc_transport_same_bits(tmp_path_factory):
    name = "inertial3_p2_ipc"
    res, host = _run(name, tmp_path_factory), _run(SR.CONFIGS[name]["host"], tmp_path_factory)
    assert [r["transport"] for r in res] == ["ipc"] * 3 and [r["transport"] for r in host] == ["host"] * 3
    for nm in NAMES:
        for k in range(2):
            assert _cat(res, nm, "y", k).tobytes() == _cat(host, nm, "y", k).tobytes(), (nm, k)


# -------------------------------------------------- b. selection, c. diagonal
@pytest.mark.parametrize("name", list(SR.CONFIGS))
def test_selection_and_diagonal_on_ranks(name, tmp_path_factory):
    P = _partition(name, tmp_path_factory)
    res = _run(name, tmp_path_factory)
    one = _run(name, tmp_path_factory, one=True)[0]
    dim = P.dim
    dird = np.repeat(P.dirflag, dim)
    assert any(p.dir[p.ghosts].any() for p in P.parts) and any((~p.dir[p.ghosts]).any() for p in P.parts)
    for nm in ("K", "Krhs"):
        y, yn = _cat(res, nm, "y", 1), _cat(res, nm, "y_nan")
        assert not np.isnan(yn[~dird]).any(), (name, nm)
        assert yn[~dird].tobytes() == y[~dird].tobytes(), (name, nm)
        # a Dirichlet row is y_i = x_i: NaN where x was poisoned (K), x_i bit for bit (Krhs)
        if nm == "K":
            assert np.isnan(yn[dird]).all()
        else:
            assert yn[dird].tobytes() == P.x[nm][1][dird].tobytes()
        dg = P.to_one(_cat(res, nm, "diag"), dim)
        assert dg.tobytes() == one["ops"][nm]["diag"].tobytes(), (name, nm, "diagonal")
        assert np.all(dg[np.repeat(P.one_dir, dim)] == 1.0)
    assert np.all(_cat(res, "K", "diag")[~dird] > 0.0) and np.all(_cat(res, "Krhs", "diag")[~dird] == 0.0)
    yr = _cat(res, "Rw", "y_nan")
    assert yr[dird].tobytes() == np.zeros(int(dird.sum())).tobytes()  # +0.0 in bytes
    assert np.isnan(yr[~dird]).all()


# ------------------------------------------------------------------ d. solves
def test_krylov_variants_on_ranks(tmp_path_factory):
    name = "slab2_p2"
    res = _run(name, tmp_path_factory)
    d = _cat(res, "K", "diag")
    assert d.min() > 0.0
    for key in VARIANTS:
        v = [r["variants"][key] for r in res]
        bound = 2 * VARIANT_RTOL * (d.max() / d.min() if key == ("gmres", "jacobi") else 1.0)
        print(f"SUMFAC-RANKS {name} {key}: iterations {v[0]['its']}  true residual {v[0]['res']:.3e}  bound {bound:.3e}")
        for a in v:
            assert a["reason"] > 0, (key, a["reason"])
            assert a["res"] <= bound, (key, a["res"], bound)
            assert a["its"] == v[0]["its"] and a["res"] == v[0]["res"], key  # (allreduced: the same on every rank)


@pytest.mark.parametrize("name", [n for n, c in SR.CONFIGS.items() if c.get("solve")])
def test_kle_solver_on_ranks_matches_one_rank(name, tmp_path_factory):
    P = _partition(name, tmp_path_factory)
    sv = [r["solve"] for r in _run(name, tmp_path_factory)]
    o = _run(name, tmp_path_factory, one=True)[0]["solve"]
    u = P.to_one(np.concatenate([s["u"] for s in sv]), P.dim)
    for s in sv + [o]:
        assert s["reason"] > 0 and s["true"] <= 1e-11, (s["reason"], s["true"])
    rel = np.linalg.norm(u - o["u"]) / np.linalg.norm(o["u"])
    print(f"SUMFAC-RANKS {name} -kle_k_type sumfac: |u - one rank| / |.| {rel:.3e}  iterations "
          f"{[s['its'] for s in sv]} (one rank {o['its']})  true residual {max(s['true'] for s in sv):.3e}")
    assert np.linalg.norm(o["u"]) > 0 and rel <= 1e-8


def test_eval_rhs_on_two_ranks(tmp_path_factory):
    name = "msh2d_r2_p4"
    P = _partition(name, tmp_path_factory)
    ev = [r["eval"] for r in _run(name, tmp_path_factory)]
    one = _run(name, tmp_path_factory, one=True)[0]["eval"]
    assert ev[0]["range"][0] == 0 and ev[0]["range"][1] == ev[1]["range"][0] and ev[1]["range"][1] == one["range"][1]
    two = P.to_one(np.concatenate([e["f"] for e in ev]), 1)
    assert np.any(one["f"] != 0.0)
    rel = np.linalg.norm(two - one["f"]) / np.linalg.norm(one["f"])
    print(f"SUMFAC-RANKS {name} evalRHS 2 ranks vs 1: relative difference {rel:.3e}")
    assert rel <= 1e-8


@pytest.mark.parametrize("name", LOCAL_TIMING)
def test_local_timing_on_ranks(name, tmp_path_factory):
    """timeLocalSpmv on ranks: the sum-factorised operators' local product
    (both lists, no halo) and a rank's part of an assembled node-block matrix;
    every call gives a positive time, a finite y and leaves mult's bits alone."""
    for r in _run(name, tmp_path_factory):
        loc = r["local"]
        want = ["sumfac_" + nm for nm in NAMES] + ["assembled_Rw", "assembled_K_nb"]
        k = loc["assembled_K_sym"]
        assert loc["sym"], (name, r["rank"])
        if name == "inertial3_p2":
            assert "gsym" in k["kernel"], k
            want.append("assembled_K_sym")
        else:  # the box symmetric tiles of a slab: refused (Error 62) before any launch, the product untouched
            assert "brick" not in k["kernel"], k
            assert k["refused"] == 62 and k["ms"] is None and k["same"], k
        for tag in want:
            v = loc[tag]
            assert v["refused"] is None and v["ms"] is not None and v["ms"] > 0.0, (name, r["rank"], tag, v)
            assert v["same"] and v["finite"], (name, r["rank"], tag, v)


# --------------------------------------------------------------- e. refusals
def test_refusals_on_ranks(tmp_path_factory):
    for r in _run("slab2_p2", tmp_path_factory):
        assert r["refused"] == {k: 56 for k in r["refused"]}, (r["rank"], r["refused"])
        assert len(r["refused"]) == 14 and r["after"]
