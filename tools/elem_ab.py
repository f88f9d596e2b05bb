"""In-process A/B of the element-wise K (Mat.createKLEElement, kle_elem.hip)
against the assembled K as bench.py configures it (symmetric storage, bricks),
on one GPU: per mesh, legs alternate round by round in ONE process --

  product   --reps products y = K x            (assembled, element)
  cg        --its fixed iterations of classic Jacobi-CG on each

each timed with HIP events recorded on the context's stream after a warm-up
of the same leg; the median over --rounds and the rounds' spread are reported.
The device memory each operator holds is hipMemGetInfo before / after its
creation.  With --check (first mesh): the product bound of
tests/test_gpu_elem.py on a 4096-row sample covering every Dirichlet / free
boundary class (reference rows from the assembled K, np.longdouble; delta
from the 27 first / middle / last elements per axis), and one converged
classic-CG solve with the element operator whose true residual is formed
through the assembled K.  One JSON line per leg is appended to --out.

With --matfree the legs are those of the matrix-free KLE system instead
(records to profiles/elem/matfree.jsonl), per mesh and in one process:

  build       wall time of MatFS.build(buildOperators=False) and the device
              memory its K, Krhs, Rw (and the empty Rd) hold (hipMemGetInfo
              before / after), kleType assembled and element alternating,
              after one untimed build of each
  product_Rw  --reps products y = Rw w      (assembled, element), timed as above

and with --check (first mesh) the Rw product bound of
tests/test_gpu_matfree.py on the row sample (reference rows from the
assembled Rw) and one KleSolver.solve on Taylor-Green from the matrix-free
build, its true residual K u - (Rw w + Krhs u_bc) formed through the assembled
matrices.

With --operators the legs are those of the element-wise collocation operators
(Mat.createOperatorElement, kle_colloc.hip; records to
profiles/elem/operators.jsonl), per mesh and in one process, opType assembled
and element alternating:

  build_operators  wall time of Operators.build and the device memory Curl, SrT
                   and DivSrT hold (hipMemGetInfo before / after), after one
                   untimed build of each kind
  product_<op>     --reps products of Curl, SrT and DivSrT, timed as above
  chain            the evalRHS chain without the KLE solve: computeVtensV, SrT,
                   scale, axpy, DivSrT, scale, Curl

and with --check (first mesh) the product bound of tests/test_gpu_colloc.py on
the row sample over all incidence classes (reference rows from the assembled
operators, element matrices from the oracle's Element.ops on the mesh's own
corners, delta over the 27 first / middle / last elements per axis).  With
--config4 instead: one BaseProblem at config 4's stated size ([18,18,18],
ngl 7) under -kle_mat_type element -kle_op_type element, one evalRHS, its time
and the device memory held.

With --noslip the legs are those of the matrix-free no-slip system
(Mat.createNSElement, MatNS.build(nsType="element"); records to
profiles/elem/noslip.jsonl) on a six-wall lid-driven box at the first mesh (if
the assembled set cannot be built there, the next smaller of --fallback-meshes
on which it can, named in every record), in one process:

  build_ns      wall time of MatNS.build(buildOperators=False) and the device
                memory the eight KLE matrices and K + Kfs hold, nsType assembled
                and element alternating, after one untimed build of each
  product_<op>  --reps products of K, K+Kfs, Krhsfs and Rwfs (assembled, element)
  product_K_dof_vs_node  the per-DoF K against the free-slip element-wise K of
                the same lattice (all faces Dirichlet): the cost of the [E][nc]
                index table over the [E][nn] one
  solve_ns      one solveFS + solve from the element build (wall time,
                iterations, reasons)

With --sumfac the legs are those of the sum-factorised K
(Mat.createKLESumFactored, kle_sumfac.hip; records to
profiles/elem/sumfac.jsonl), in one process, legs alternating round by round:

  (a) unstructured  the mesh bench.py --mesh unstructured generates
                    (perturbed_box(3, nelem, seed=5) of the first mesh, written
                    as a Gmsh file): K as the bench configures it (mat.build's
                    defaults: symmetric storage, graph bricks) against the
                    sum-factorised K -- --reps products and --its fixed
                    iterations of classic Jacobi-CG on each
  (b) box           the box mesh of the same size: the dense-GEMM element K
                    (Mat.createKLEElement) against the sum-factorised K,
                    --reps products

each with the build wall time and the device memory held (hipMemGetInfo before
/ after).  With --check: KleSolver.solve on Taylor-Green on (a) with the
assembled and with the sum-factorised operators (-kle_k_type sumfac) to rtol
1e-10, iterations and the true residual K u - (Rw w + Krhs u_bc) through the
assembled matrices.

With --sumfac-system the legs are those of the whole matrix-free set on an
unstructured mesh (-kle_mat_type sumfac -kle_op_type sumfac: K, Krhs, Rw,
Curl, SrT, DivSrT; records to profiles/elem/sumfac_system.jsonl), one process,
the forms alternating round by round, on perturbed_box(3, nelem, seed=5) of
the first mesh and on the box of the same size (there also the `element`
forms):

  build_system   wall time and device memory (hipMemGetInfo before / after) of
                 MatFS.build per form
  product_<op>   --reps products of Rw, Curl, SrT, DivSrT per form, with the
                 algorithmic bytes (spmv_bytes)
  chain          the evalRHS chain without the KLE solve
  eval_rhs       one whole BaseProblem.evalRHS per form (wall time, iterations)

With --check: Taylor-Green with the matrix-free set to rtol 1e-10, the true
residual K u - (Rw w + Krhs u_bc) formed through the assembled K, Krhs and Rw.

With --sumfac-noslip the legs are those of the matrix-free no-slip system on
an unstructured mesh (Mat.createNSSumFactored, MatNS.build(nsType="sumfac");
records to profiles/elem/sumfac_noslip.jsonl), one process, on
perturbed_box(3, nelem, seed=5) of the first mesh with six no-slip walls:

  build_ns        wall time and device memory (hipMemGetInfo before / after) of
                  MatNS.build(buildOperators=False) per nsType; where the
                  assembled set cannot be built the record says so and the legs
                  against it are left out
  product_<op>    --reps products of the seven operators, sum-factorised and
                  assembled, with the algorithmic bytes (spmv_bytes)
  product_K_cls_vs_node   the class-masked K against the free-slip
                  sum-factorised K of the same mesh (the per-node mask folded
                  into the connectivity): the price of the class table
  solve_ns        one solveFS + solve at rtol 1e-10 with nothing of the KLE
                  system assembled: iterations, and the true residuals
                  (K+Kfs) v - bFS and K u - b through the assembled matrices

  python tools/elem_ab.py [--meshes 20,16,16:5 8,8,6:7] [--rounds 3] [--check]
                          [--matfree | --operators [--config4] | --noslip | --sumfac | --sumfac-system |
                           --sumfac-noslip]
"""
import argparse
import ctypes as C
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Hip:
    """The few HIP runtime calls the timing needs."""

    def __init__(self, ctx):
        from pynama_amd._lib import call
        self.rt = C.CDLL("libamdhip64.so")
        s = C.c_void_p()
        call("kle_ctx_get_stream", ctx.h, C.byref(s))
        self.stream = s

    def _ok(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: hipError {rc}")

    def free_bytes(self):
        f, t = C.c_size_t(), C.c_size_t()
        self._ok(self.rt.hipMemGetInfo(C.byref(f), C.byref(t)), "hipMemGetInfo")
        return f.value

    def timed_ms(self, fn):
        e0, e1 = C.c_void_p(), C.c_void_p()
        self._ok(self.rt.hipEventCreate(C.byref(e0)), "hipEventCreate")
        self._ok(self.rt.hipEventCreate(C.byref(e1)), "hipEventCreate")
        try:
            self._ok(self.rt.hipEventRecord(e0, self.stream), "hipEventRecord")
            fn()
            self._ok(self.rt.hipEventRecord(e1, self.stream), "hipEventRecord")
            self._ok(self.rt.hipEventSynchronize(e1), "hipEventSynchronize")
            ms = C.c_float()
            self._ok(self.rt.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
            return float(ms.value)
        finally:
            self.rt.hipEventDestroy(e0)
            self.rt.hipEventDestroy(e1)


def spread(v):
    m = statistics.median(v)
    return {"median": m, "min": min(v), "max": max(v), "spread_pct": 100.0 * (max(v) - min(v)) / m}


def check_product(pa, np, dom, mat, Ke, nrows=4096, which="K"):
    """tests/test_gpu_elem.py's bound (which "Rw": tests/test_gpu_matfree.py's,
    Ke the element-wise Rw, reference rows from mat.Rw) on a sample of rows of
    the full-size mesh."""
    from pynama_amd._lib import call
    mesh, dim, ngl = dom.mesh, dom.mesh.dim, dom.mesh.ngl
    nn, nd, E = ngl ** dim, dim * ngl ** dim, mesh.E
    rw = which == "Rw"
    cw = (1 if dim == 2 else 3) if rw else dim  # components of the column space
    ctx = pa.get_ctx()
    eps = np.finfo(np.float64).eps
    isdir = np.zeros(mesh.N, bool)
    isdir[mesh.face_nodes(pa.mesh.FACES[dim])] = True
    conn = mesh.conn()
    ninc = np.bincount(conn.ravel(), minlength=mesh.N)
    # classes: (Dirichlet?, incident elements); the same share of the sample each
    rng = np.random.default_rng(7)
    cls = isdir.astype(np.int64) * 16 + ninc
    keys = np.unique(cls)
    per = max(1, (nrows // dim) // len(keys) + 1)
    nodes = np.concatenate([rng.permutation(np.flatnonzero(cls == k))[:per] for k in keys])
    rows = (nodes[:, None] * dim + np.arange(dim)[None, :]).ravel()[:nrows]
    # K_e0 (Rw_e0), Kmax, delta over the first / middle / last elements of every axis
    K0, Rwe = np.zeros((nd, nd)), np.zeros((nd, (1 if dim == 2 else 3) * nn))
    call("kle_element_kle", ctx.h, mesh._h, 0, K0, Rwe)
    if rw:
        K0 = Rwe.copy()
    Kmax = np.abs(K0).max()
    ne = list(mesh.nelem) + [1] * (3 - dim)
    pos = [sorted({0, n // 2, n - 1}) for n in ne]
    Kx, delta = np.zeros((nd, nd)), 0.0
    for ez in pos[2]:
        for ey in pos[1]:
            for ex in pos[0]:
                e = ex + ne[0] * (ey + ne[1] * ez)
                if e:
                    call("kle_element_kle", ctx.h, mesh._h, e, Kx, Rwe)
                    delta = max(delta, np.abs((Rwe if rw else Kx) - K0).max() / Kmax)
    x = np.random.default_rng(20240607).uniform(-1, 1, mesh.N * cw)
    xv = Ke.createVecRight()
    xv.setArray(x)
    y = (Ke * xv).getArray()
    # node -> incident (element, local node), from the connectivity
    order = np.argsort(conn.ravel(), kind="stable")
    start = np.concatenate([[0], np.cumsum(ninc)])
    dird = np.repeat(isdir, dim)
    aK0 = np.abs(K0)
    worst, bad, dir_nonzero = 0.0, 0, 0
    for r in rows:
        cols, vals = (mat.Rw if rw else mat.K).getRow(int(r))
        ref = np.sum(vals.astype(np.longdouble) * x[cols].astype(np.longdouble))
        node, a = divmod(int(r), dim)
        B = X = 0.0
        for t in order[start[node]:start[node + 1]]:
            e, l = divmod(int(t), nn)
            gd = (conn[e][:, None] * cw + np.arange(cw)[None, :]).ravel()
            # K drops the Dirichlet columns; Rw takes every column
            xe = np.abs(x[gd]) if rw else np.where(dird[gd], 0.0, np.abs(x[gd]))
            B += aK0[l * dim + a] @ xe
            X += xe.sum()
        if dird[r]:
            # unit diagonal (K); no entry at all (Rw: exactly 0)
            B = 0.0 if rw else max(B, abs(x[r]))
            dir_nonzero += rw and y[r] != 0.0
        bnd = (cw * nn + 8) * eps * B + delta * Kmax * X
        err = float(abs(np.longdouble(y[r]) - ref))
        worst = max(worst, err / bnd if bnd > 0 else (0.0 if err == 0 else np.inf))
        bad += err > bnd
    out = {"rows": int(len(rows)), "classes": int(len(keys)), "delta": float(delta), "delta_elements": 27,
           "max_err_over_bound": float(worst), "rows_over_bound": int(bad)}
    if rw:
        out["dirichlet_rows_sampled"] = int(dird[rows].sum())
        out["dirichlet_rows_not_zero"] = int(dir_nonzero)
    return out


def check_solve(pa, np, mat, Ke):
    K = mat.K
    xt = K.createVecRight()
    xt.setArray(np.random.default_rng(9).uniform(-1, 1, xt.getLocalSize()))
    b = K * xt
    out = {}
    for label, A in (("element", Ke), ("assembled", K)):
        ksp = pa.petsc.KSP().create()
        ksp.setType("cg")
        pc = pa.petsc.PC().create()
        pc.setType("jacobi")
        ksp.setPC(pc)
        ksp.setCGSingleReduction(False)
        ksp.setTolerances(rtol=1e-10, atol=0.0, max_it=100000)
        ksp.setOperators(A)
        ksp.setUp()
        u = A.createVecRight()
        ksp.solve(b, u)
        r = K * u  # the true residual through the assembled K
        r.aypx(-1.0, b)
        out[label] = {"iterations": ksp.getIterationNumber(), "reason": ksp.getConvergedReason(),
                      "correction_iterations": ksp.getCorrectionIterations(),
                      "true_rel_residual_assembled_K": r.norm() / b.norm()}
    return out


def check_solve_matfree(pa, np, dom, mat_e, mat_a):
    """KleSolver.solve on Taylor-Green from the matrix-free build; the true
    residual K u - (Rw w + Krhs u_bc) through the assembled matrices."""
    dim = dom.mesh.dim
    f = pa.fields.get("taylor_green3d" if dim == 3 else "taylor_green")
    sol = pa.KleSolver()
    sol.setMat(mat_e)
    sol.setUp()
    vort = mat_e.Rw.createVecRight()
    vort.setArray(np.asarray(f.vorticity(dom.getFullCoordArray(), 1.0), dtype=np.float64).ravel())
    vel = sol.getSolution()
    dom.applyBoundaryConditions(vel, "velocity", 0.0, 0.02)
    b = mat_a.Rw * vort
    b.axpy(1.0, mat_a.Krhs * vel)  # vel holds u_bc on the Dirichlet nodes; Krhs reads nothing else
    sol.solve(vort)
    ksp = sol.getKSP()
    r = mat_a.K * vel
    r.aypx(-1.0, b)
    return {"operator": ksp.getOperators()[0].spmvKernel(), "iterations": ksp.getIterationNumber(),
            "reason": ksp.getConvergedReason(), "rtol": 1e-10,
            "true_rel_residual_assembled": r.norm() / b.norm()}


def matfree(a, pa, np, hip, ctx, emit):
    for mi, spec in enumerate(a.meshes):
        ne_s, ngl = spec.split(":")
        nelem, ngl = [int(v) for v in ne_s.split(",")], int(ngl)
        dim = len(nelem)
        cfg = {"domain": {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": [0.0] * dim, "upper": [1.0] * dim}},
               "boundary-conditions": {"custom-func": {"name": "taylor_green3d" if dim == 3 else "taylor_green"}}}
        dom = pa.Domain()
        dom.configure(cfg)
        dom.setUp()
        base = {"nelem": nelem, "ngl": ngl, "dofs": dom.mesh.N * dim, "rounds": a.rounds}
        mats, t_build, mem = {}, {"assembled": [], "element": []}, {}
        for rnd in range(a.rounds + 1):  # round 0: untimed (module load, first allocations)
            for kt in ("assembled", "element"):
                mats.pop(kt, None)
                gc.collect()
                ctx.synchronize()
                m0 = hip.free_bytes()
                t0 = time.perf_counter()
                mat = pa.MatFS()
                mat.setDomain(dom)
                mat.build(buildOperators=False, kleType=kt)
                ctx.synchronize()
                t1 = time.perf_counter()
                mats[kt] = mat
                if rnd:
                    t_build[kt].append(1e3 * (t1 - t0))
                    mem[kt] = m0 - hip.free_bytes()
        for kt in ("assembled", "element"):
            emit(dict(base, leg="build", kleType=kt, formats=[m.getFormat() for m in mats[kt].kle],
                      ms=spread(t_build[kt]), device_memory={"bytes_K_Krhs_Rw_Rd": mem[kt]}))
        ops = {"assembled": mats["assembled"].Rw, "element": mats["element"].Rw}
        x = ops["element"].createVecRight()
        x.setArray(np.random.default_rng(1).uniform(-1, 1, x.getLocalSize()))
        y = ops["element"].createVecLeft()
        t_prod = {k: [] for k in ops}
        for _ in range(a.rounds):
            for label, A in ops.items():
                for _w in range(20):
                    A.mult(x, y)
                ms = hip.timed_ms(lambda: [A.mult(x, y) for _r in range(a.reps)])
                t_prod[label].append(1e3 * ms / a.reps)
        nn = ngl ** dim
        for label, A in ops.items():
            flops = (2.0 * dim * nn * (1 if dim == 2 else 3) * nn * dom.mesh.E if label == "element"
                     else 2.0 * A.getInfo()["nz_used"])
            emit(dict(base, leg="product_Rw", operator=label, kernel=A.spmvKernel(), bytes=A.spmvBytes(), flops=flops,
                      reps=a.reps, us=spread(t_prod[label])))
        emit(dict(base, leg="ratio_Rw", assembled_over_element={
            "product": statistics.median(t_prod["assembled"]) / statistics.median(t_prod["element"]),
            "build": statistics.median(t_build["assembled"]) / statistics.median(t_build["element"]),
            "device_memory": mem["assembled"] / max(mem["element"], 1)}))
        if a.check and mi == 0:
            emit(dict(base, leg="check_product_Rw",
                      **check_product(pa, np, dom, mats["assembled"], ops["element"], which="Rw")))
            emit(dict(base, leg="check_solve_matfree",
                      **check_solve_matfree(pa, np, dom, mats["element"], mats["assembled"])))
        del ops, mats, x, y, dom
        gc.collect()


def sumfac(a, pa, np, hip, ctx, emit):
    import tempfile

    from pynama_amd.meshgen import perturbed_box, write_gmsh
    from pynama_amd.petsc import Mat, Options
    ne_s, ngl = a.meshes[0].split(":")
    nelem, ngl = [int(v) for v in ne_s.split(",")], int(ngl)
    dim = len(nelem)
    bc = {"custom-func": {"name": "taylor_green3d" if dim == 3 else "taylor_green"}}
    path = os.path.join(tempfile.mkdtemp(prefix="kle_sumfac_"), "mesh.msh")
    write_gmsh(path, dim, *perturbed_box(dim, nelem, seed=5))
    domains = {"unstructured": {"ngl": ngl, "gmsh-file": path},
               "box": {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": [0.0] * dim, "upper": [1.0] * dim}}}

    def timed_build(fn):
        gc.collect()
        ctx.synchronize()
        m0, t0 = hip.free_bytes(), time.perf_counter()
        out = fn()
        ctx.synchronize()
        return out, 1e3 * (time.perf_counter() - t0), m0 - hip.free_bytes()

    for leg, domain in domains.items():
        dom = pa.Domain()
        dom.configure({"domain": domain, "boundary-conditions": bc})
        dom.setUp()
        base = {"mesh": leg, "nelem": nelem, "ngl": ngl, "dofs": dom.mesh.N * dim, "rounds": a.rounds}
        mat = pa.MatFS()
        mat.setDomain(dom)
        _, t_asm, m_asm = timed_build(lambda: mat.build(buildOperators=False))
        Ks, t_sf, m_sf = timed_build(lambda: Mat.createKLESumFactored(dom.mesh, "K"))
        build = {"assembled": {"ms": t_asm, "device_bytes_K_Krhs_Rw": m_asm},
                 "sumfac": {"ms": t_sf, "device_bytes_K": m_sf}}
        if leg == "box":
            Ke, t_el, m_el = timed_build(lambda: mat.getElementK())
            build["element"] = {"ms": t_el, "device_bytes_K": m_el}
            ops = {"element": Ke, "sumfac": Ks}
        else:
            ops = {"assembled": mat.K, "sumfac": Ks}
        x = mat.K.createVecRight()
        x.setArray(np.random.default_rng(1).uniform(-1, 1, x.getLocalSize()))
        y = mat.K.createVecLeft()
        b = mat.K.createVecLeft()
        b.setArray(np.random.default_rng(2).uniform(-1, 1, b.getLocalSize()))
        ksps = {}
        if leg == "unstructured":
            for label, A in ops.items():
                ksp = pa.petsc.KSP().create()
                ksp.setType("cg")
                pc = pa.petsc.PC().create()
                pc.setType("jacobi")
                ksp.setPC(pc)
                ksp.setCGSingleReduction(False)
                ksp.setOperators(A)
                ksp.setUp()
                ksp.setFixedIterations(a.its)
                ksps[label] = (ksp, A.createVecRight())
        t_prod, t_cg = {k: [] for k in ops}, {k: [] for k in ksps}
        for _ in range(a.rounds):
            for label, A in ops.items():
                for _w in range(20):
                    A.mult(x, y)
                ms = hip.timed_ms(lambda: [A.mult(x, y) for _r in range(a.reps)])
                t_prod[label].append(1e3 * ms / a.reps)
            for label, (ksp, u) in ksps.items():
                u.set(0.0)
                ksp.solve(b, u)  # warm-up: the same fixed iterations
                u.set(0.0)
                ms = hip.timed_ms(lambda: ksp.solve(b, u))
                if ksp.getConvergedReason() < 0:
                    raise SystemExit(f"elem_ab: the fixed CG iterations diverged ({label})")
                t_cg[label].append(1e3 * ms / a.its)
        for label, A in ops.items():
            emit(dict(base, leg="product", operator=label, kernel=A.spmvKernel(), bytes=A.spmvBytes(), reps=a.reps,
                      us=spread(t_prod[label]), build=build[label]))
        for label, (ksp, _u) in ksps.items():
            emit(dict(base, leg="cg", operator=label, ksp="cg (classic) + jacobi", kernel=ops[label].spmvKernel(),
                      iterations=a.its, us_per_iteration=spread(t_cg[label])))
        other = "element" if leg == "box" else "assembled"
        ratio = {"product": statistics.median(t_prod[other]) / statistics.median(t_prod["sumfac"])}
        if ksps:
            ratio["cg_iteration"] = statistics.median(t_cg[other]) / statistics.median(t_cg["sumfac"])
        emit(dict(base, leg="ratio", **{other + "_over_sumfac": ratio}))
        if a.check and leg == "unstructured":
            f = pa.fields.get(bc["custom-func"]["name"])
            for ktype in ("assembled", "sumfac"):
                opts = Options()
                opts.setValue("kle_k_type", ktype)
                try:
                    sol = pa.KleSolver()
                    sol.setMat(mat)
                    sol.setUp()
                finally:
                    opts.delValue("kle_k_type")
                vort = mat.Rw.createVecRight()
                vort.setArray(np.asarray(f.vorticity(dom.getFullCoordArray(), 1.0), dtype=np.float64).ravel())
                vel = sol.getSolution()
                dom.applyBoundaryConditions(vel, "velocity", 0.0, 0.02)
                rhs = mat.Rw * vort
                rhs.axpy(1.0, mat.Krhs * vel)  # vel holds u_bc on the Dirichlet nodes; Krhs reads nothing else
                sol.solve(vort)
                ksp = sol.getKSP()
                r = mat.K * vel
                r.aypx(-1.0, rhs)
                emit(dict(base, leg="check_solve", k_type=ktype, operator=ksp.getOperators()[0].spmvKernel(),
                          iterations=ksp.getIterationNumber(), reason=ksp.getConvergedReason(), rtol=1e-10,
                          true_rel_residual_assembled=r.norm() / rhs.norm()))
                del sol
        del ksps, ops, Ks, mat, dom, x, y, b
        gc.collect()


def sumfac_system(a, pa, np, hip, ctx, emit):
    import tempfile

    from pynama_amd._lib import call
    from pynama_amd.meshgen import perturbed_box, write_gmsh
    from pynama_amd.petsc import Options
    ne_s, ngl = a.meshes[0].split(":")
    nelem, ngl = [int(v) for v in ne_s.split(",")], int(ngl)
    dim = len(nelem)
    tg = "taylor_green3d" if dim == 3 else "taylor_green"
    bc = {"custom-func": {"name": tg}}
    path = os.path.join(tempfile.mkdtemp(prefix="kle_sumfac_system_"), "mesh.msh")
    write_gmsh(path, dim, *perturbed_box(dim, nelem, seed=5))
    domains = {"unstructured": {"ngl": ngl, "gmsh-file": path},
               "box": {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": [0.0] * dim, "upper": [1.0] * dim}}}
    names = ("Rw",) + OPS

    def get(mat, nm):
        return mat.Rw if nm == "Rw" else getattr(mat.getOperators(), nm)

    for leg, domain in domains.items():
        forms = ("assembled", "sumfac") + (("element",) if leg == "box" else ())
        dom = pa.Domain()
        dom.configure({"domain": domain, "boundary-conditions": bc})
        dom.setUp()
        base = {"mesh": leg, "nelem": nelem, "ngl": ngl, "nodes": dom.mesh.N, "rounds": a.rounds}
        mats = {}
        for form in forms:
            gc.collect()
            ctx.synchronize()
            m0, t0 = hip.free_bytes(), time.perf_counter()
            mat = pa.MatFS()
            mat.setDomain(dom)
            mat.build(kleType=form, opType=form)
            ctx.synchronize()
            t1 = time.perf_counter()
            mats[form] = mat
            emit(dict(base, leg="build_system", form=form, ms=1e3 * (t1 - t0),
                      device_bytes_K_Krhs_Rw_Curl_SrT_DivSrT=m0 - hip.free_bytes(),
                      formats=[mat.K.getFormat(), mat.Krhs.getFormat()] + [get(mat, n).getFormat() for n in names]))
        ratios = {}
        for nm in names:
            ops = {form: get(mats[form], nm) for form in forms}
            x = ops["sumfac"].createVecRight()
            x.setArray(np.random.default_rng(1).uniform(-1, 1, x.getLocalSize()))
            y = ops["sumfac"].createVecLeft()
            t_prod = {k: [] for k in forms}
            for _ in range(a.rounds):
                for label, A in ops.items():
                    for _w in range(20):
                        A.mult(x, y)
                    ms = hip.timed_ms(lambda: [A.mult(x, y) for _r in range(a.reps)])
                    t_prod[label].append(1e3 * ms / a.reps)
            for label, A in ops.items():
                emit(dict(base, leg="product_" + nm, form=label, kernel=A.spmvKernel(), bytes=A.spmvBytes(),
                          reps=a.reps, us=spread(t_prod[label]),
                          tb_per_s=A.spmvBytes() / statistics.median(t_prod[label]) * 1e-6))
            ratios[nm] = {f + "_over_sumfac": statistics.median(t_prod[f]) / statistics.median(t_prod["sumfac"])
                          for f in forms if f != "sumfac"}
            ratios[nm]["sumfac_faster_than_assembled_beyond_spread"] = bool(max(t_prod["sumfac"]) < min(t_prod["assembled"]))
        chains = {form: Chain(mats[form].getOperators(), dim) for form in forms}
        f = pa.fields.get(tg)
        vel = mats["sumfac"].K.createVecRight()
        vel.setArray(np.asarray(f.velocity(dom.getFullCoordArray(), 1.0), dtype=np.float64).ravel())
        rhs, fo = vel.duplicate(), mats["sumfac"].getOperators().Curl.createVecLeft()
        t_chain = {k: [] for k in forms}
        for _ in range(a.rounds):
            for label, ch in chains.items():
                for _w in range(10):
                    eval_rhs_chain(call, ch, vel, rhs, fo)
                ms = hip.timed_ms(lambda: [eval_rhs_chain(call, ch, vel, rhs, fo) for _r in range(a.reps)])
                t_chain[label].append(ms / a.reps)
        for label in forms:
            emit(dict(base, leg="chain", form=label, steps="computeVtensV, SrT, scale, axpy, DivSrT, scale, Curl",
                      reps=a.reps, ms=spread(t_chain[label])))
        ratios["chain"] = {f + "_over_sumfac": statistics.median(t_chain[f]) / statistics.median(t_chain["sumfac"])
                           for f in forms if f != "sumfac"}
        emit(dict(base, leg="ratio_system", **ratios))
        del chains, rhs, fo
        # one whole evalRHS per form: a BaseProblem of its own
        cfg = {"name": "sumfac_system", "material-properties": {"rho": 0.5, "mu": 0.01}, "domain": domain,
               "boundary-conditions": bc, "initial-conditions": bc}
        for form in forms:
            opts = Options()
            opts.setValue("kle_mat_type", form)
            opts.setValue("kle_op_type", form)
            try:
                prob = pa.BaseProblem(cfg)
                prob.setUp()
                prob.setUpSolver()
            finally:
                opts.delValue("kle_mat_type")
                opts.delValue("kle_op_type")
            fo = prob.operator.Curl.createVecLeft()
            prob.evalRHS(None, 0.0, prob.vort, fo)  # warm-up
            walls = []
            for _ in range(a.rounds):
                ctx.synchronize()
                t0 = time.perf_counter()
                prob.evalRHS(None, 0.0, prob.vort, fo)
                ctx.synchronize()
                walls.append(1e3 * (time.perf_counter() - t0))
            ksp = prob.solverKLE.getKSP()
            emit(dict(base, leg="eval_rhs", form=form, wall_ms=spread(walls), kle_iterations=ksp.getIterationNumber(),
                      kle_reason=ksp.getConvergedReason(), finite=bool(np.all(np.isfinite(fo.getArray())))))
            del prob, fo
            gc.collect()
        if a.check and leg == "unstructured":
            asm, mf = mats["assembled"], mats["sumfac"]
            sol = pa.KleSolver()
            sol.setMat(mf)
            sol.setUp()
            vort = mf.Rw.createVecRight()
            vort.setArray(np.asarray(f.vorticity(dom.getFullCoordArray(), 1.0), dtype=np.float64).ravel())
            vel = sol.getSolution()
            dom.applyBoundaryConditions(vel, "velocity", 0.0, 0.02)
            rhs = asm.Rw * vort
            rhs.axpy(1.0, asm.Krhs * vel)  # vel holds u_bc on the Dirichlet nodes; Krhs reads nothing else
            sol.solve(vort)
            ksp = sol.getKSP()
            r = asm.K * vel
            r.aypx(-1.0, rhs)
            emit(dict(base, leg="check_solve", form="sumfac", operator=ksp.getOperators()[0].spmvKernel(),
                      rw=mf.Rw.spmvKernel(), iterations=ksp.getIterationNumber(), reason=ksp.getConvergedReason(),
                      rtol=1e-10, true_rel_residual_assembled=r.norm() / rhs.norm()))
            del sol
        del mats, dom, vel
        gc.collect()


OPS = ("Curl", "SrT", "DivSrT")


def op_shape(dim, nm):
    dw, ds = (1, 3) if dim == 2 else (3, 6)
    return {"Curl": (dw, dim), "SrT": (ds, dim), "DivSrT": (dim, ds)}[nm]


def check_product_ops(pa, np, dom, asm, elem, nrows=4096):
    """tests/test_gpu_colloc.py's bound on a sample of rows of the full-size
    mesh, per operator."""
    from oracle import oracle as O
    mesh, dim, ngl = dom.mesh, dom.mesh.dim, dom.mesh.ngl
    nn, E, N = ngl ** dim, mesh.E, mesh.N
    eps = np.finfo(np.float64).eps
    conn = mesh.conn()
    ninc = np.bincount(conn.ravel(), minlength=N)
    ne = list(mesh.nelem) + [1] * (3 - dim)
    om = O.BoxMesh(dim, ne[:dim], [0.0] * dim, [1.0] * dim, ngl)  # the tool's meshes are unit boxes
    perm = np.array([np.where(conn[0] == c)[0][0] for c in om.conn()[0]])
    del om
    el = O.Element(ngl, dim)
    corners = mesh.corners()

    def ops(e):
        SrT, Div, Curl, W = el.ops(corners[e].ravel())
        out = {}
        for nm, M in (("Curl", Curl), ("SrT", SrT), ("DivSrT", Div)):
            R, Cc = op_shape(dim, nm)
            pr = (perm[:, None] * R + np.arange(R)[None, :]).ravel()
            pc = (perm[:, None] * Cc + np.arange(Cc)[None, :]).ravel()
            T = np.zeros_like(M)
            T[np.ix_(pr, pc)] = M
            out[nm] = T
        c = np.zeros(nn)
        c[perm] = W
        return out, c

    M0, c0 = ops(0)
    pos = [sorted({0, n // 2, n - 1}) for n in ne]
    delta, delta_w = {nm: 0.0 for nm in OPS}, 0.0
    for ez in pos[2]:
        for ey in pos[1]:
            for ex in pos[0]:
                e = ex + ne[0] * (ey + ne[1] * ez)
                if e:
                    Me, ce = ops(e)
                    for nm in OPS:
                        delta[nm] = max(delta[nm], np.abs(Me[nm] - M0[nm]).max() / np.abs(M0[nm]).max())
                    delta_w = max(delta_w, np.abs(ce - c0).max() / np.abs(c0).max())
    W = np.zeros(N)
    np.add.at(W, conn, np.broadcast_to(c0[None, :], conn.shape))
    winv = 1.0 / W
    rng = np.random.default_rng(7)
    keys = np.unique(ninc)
    order = np.argsort(conn.ravel(), kind="stable")
    start = np.concatenate([[0], np.cumsum(ninc)])
    out = {"classes": int(len(keys)), "delta_elements": 27, "delta_w": float(delta_w)}
    for nm in OPS:
        R, Cc = op_shape(dim, nm)
        per = max(1, (nrows // R) // len(keys) + 1)
        nodes = np.concatenate([rng.permutation(np.flatnonzero(ninc == k))[:per] for k in keys])
        rows = (nodes[:, None] * R + np.arange(R)[None, :]).ravel()[:nrows]
        A, Ae = getattr(asm, nm), getattr(elem, nm)
        x = np.random.default_rng(20240611).uniform(-1, 1, N * Cc)
        xv = Ae.createVecRight()
        xv.setArray(x)
        y = (Ae * xv).getArray()
        aM, Mmax = np.abs(M0[nm]), np.abs(M0[nm]).max()
        n = Cc * (dim * (ngl - 1) + 1) + 2 ** dim + 8
        worst, bad = 0.0, 0
        for r in rows:
            cols, vals = A.getRow(int(r))
            ref = np.sum(vals.astype(np.longdouble) * x[cols].astype(np.longdouble))
            node, a = divmod(int(r), R)
            B = X = 0.0
            for t in order[start[node]:start[node + 1]]:
                e, l = divmod(int(t), nn)
                xe = np.abs(x[(conn[e][:, None] * Cc + np.arange(Cc)[None, :]).ravel()])
                B += aM[l * R + a] @ xe
                X += xe.sum()
            B *= winv[node]
            bnd = n * eps * B + delta[nm] * Mmax * X * winv[node] + 2 * delta_w * B
            err = float(abs(np.longdouble(y[r]) - ref))
            worst = max(worst, err / bnd if bnd > 0 else (0.0 if err == 0 else np.inf))
            bad += err > bnd
        out[nm] = {"rows": int(len(rows)), "delta": float(delta[nm]), "max_err_over_bound": float(worst),
                   "rows_over_bound": int(bad)}
    return out


def eval_rhs_chain(call, prob, vel, rhs, f):
    """BaseProblem.evalRHS after the KLE solve."""
    op = prob.operator
    call("kle_vec_tensor_square", vel._h, prob.dim, prob._VtensV._h)
    op.SrT.mult(vel, prob._Aux1)
    prob._Aux1 *= (2.0 * prob.mu)
    prob._Aux1.axpy(-1.0 * prob.rho, prob._VtensV)
    op.DivSrT.mult(prob._Aux1, rhs)
    rhs.scale(1 / prob.rho)
    op.Curl.mult(rhs, f)


class Chain:
    """What evalRHS's chain reads of a BaseProblem, around one Operators."""

    def __init__(self, op, dim):
        self.operator, self.dim, self.mu, self.rho = op, dim, 0.01, 0.5
        self._VtensV = op.SrT.createVecLeft()
        self._Aux1 = self._VtensV.duplicate()


def operators(a, pa, np, hip, ctx, emit):
    from pynama_amd._lib import call
    from pynama_amd.matrices import Operators
    for mi, spec in enumerate(a.meshes):
        ne_s, ngl = spec.split(":")
        nelem, ngl = [int(v) for v in ne_s.split(",")], int(ngl)
        dim = len(nelem)
        cfg = {"domain": {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": [0.0] * dim, "upper": [1.0] * dim}},
               "boundary-conditions": {"custom-func": {"name": "taylor_green3d" if dim == 3 else "taylor_green"}}}
        dom = pa.Domain()
        dom.configure(cfg)
        dom.setUp()
        base = {"nelem": nelem, "ngl": ngl, "nodes": dom.mesh.N, "rounds": a.rounds}
        kinds = ("assembled", "element")
        built, t_build, mem = {}, {k: [] for k in kinds}, {}
        for rnd in range(a.rounds + 1):  # round 0: untimed (module load, first allocations)
            for ot in kinds:
                built.pop(ot, None)
                gc.collect()
                ctx.synchronize()
                m0 = hip.free_bytes()
                t0 = time.perf_counter()
                op = Operators()
                op.setDimensions(dom.getDimensions())
                op.build(dom.getMesh(), ot)
                ctx.synchronize()
                t1 = time.perf_counter()
                built[ot] = op
                if rnd:
                    t_build[ot].append(1e3 * (t1 - t0))
                    mem[ot] = m0 - hip.free_bytes()
        for ot in kinds:
            emit(dict(base, leg="build_operators", opType=ot, formats=[getattr(built[ot], n).getFormat() for n in OPS],
                      ms=spread(t_build[ot]), device_memory={"bytes_Curl_SrT_DivSrT": mem[ot]}))
        ratios = {}
        for nm in OPS:
            ops = {ot: getattr(built[ot], nm) for ot in kinds}
            x = ops["element"].createVecRight()
            x.setArray(np.random.default_rng(1).uniform(-1, 1, x.getLocalSize()))
            y = ops["element"].createVecLeft()
            t_prod = {k: [] for k in kinds}
            for _ in range(a.rounds):
                for label, A in ops.items():
                    for _w in range(20):
                        A.mult(x, y)
                    ms = hip.timed_ms(lambda: [A.mult(x, y) for _r in range(a.reps)])
                    t_prod[label].append(1e3 * ms / a.reps)
            for label, A in ops.items():
                emit(dict(base, leg="product_" + nm, operator=label, kernel=A.spmvKernel(), bytes=A.spmvBytes(),
                          reps=a.reps, us=spread(t_prod[label]),
                          tb_per_s=A.spmvBytes() / statistics.median(t_prod[label]) * 1e-6))
            ratios[nm] = {"assembled_over_element": statistics.median(t_prod["assembled"]) / statistics.median(t_prod["element"]),
                          "element_faster_beyond_spread": bool(max(t_prod["element"]) < min(t_prod["assembled"]))}
        chains = {ot: Chain(built[ot], dim) for ot in kinds}
        vel = built["element"].SrT.createVecRight()
        f = pa.fields.get("taylor_green3d" if dim == 3 else "taylor_green")
        vel.setArray(np.asarray(f.velocity(dom.getFullCoordArray(), 1.0), dtype=np.float64).ravel())
        rhs, fo = vel.duplicate(), built["element"].Curl.createVecLeft()
        t_chain, outs = {k: [] for k in kinds}, {}
        for _ in range(a.rounds):
            for label, ch in chains.items():
                for _w in range(10):
                    eval_rhs_chain(call, ch, vel, rhs, fo)
                ms = hip.timed_ms(lambda: [eval_rhs_chain(call, ch, vel, rhs, fo) for _r in range(a.reps)])
                t_chain[label].append(ms / a.reps)
                outs[label] = fo.getArray().copy()
        for label in kinds:
            emit(dict(base, leg="chain", operator=label, steps="computeVtensV, SrT, scale, axpy, DivSrT, scale, Curl",
                      reps=a.reps, ms=spread(t_chain[label])))
        ratios["chain"] = {"assembled_over_element": statistics.median(t_chain["assembled"]) / statistics.median(t_chain["element"]),
                           "element_faster_beyond_spread": bool(max(t_chain["element"]) < min(t_chain["assembled"])),
                           "max_abs_difference_of_f": float(np.abs(outs["element"] - outs["assembled"]).max()),
                           "max_abs_f": float(np.abs(outs["assembled"]).max())}
        ratios["build"] = {"assembled_over_element": statistics.median(t_build["assembled"]) / statistics.median(t_build["element"])}
        ratios["device_memory"] = {"assembled_over_element": mem["assembled"] / max(mem["element"], 1)}
        emit(dict(base, leg="ratio_operators", **ratios))
        if a.check and mi == 0:
            emit(dict(base, leg="check_product_operators",
                      **check_product_ops(pa, np, dom, built["assembled"], built["element"])))
        del chains, built, vel, rhs, fo, dom
        gc.collect()


def config4(a, pa, np, hip, ctx, emit):
    """One BaseProblem at config 4's stated size with nothing assembled."""
    from pynama_amd._lib import call
    from pynama_amd.petsc import Options
    nelem, ngl = [18, 18, 18], 7
    bc = {"custom-func": {"name": "taylor_green3d"}}
    cfg = {"name": "config4", "material-properties": {"rho": 0.5, "mu": 0.01},
           "domain": {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": [0.0] * 3, "upper": [1.0] * 3}},
           "boundary-conditions": bc, "initial-conditions": bc}
    ctx.synchronize()
    m0 = hip.free_bytes()
    opts = Options()
    opts.setValue("kle_mat_type", "element")
    opts.setValue("kle_op_type", "element")
    t0 = time.perf_counter()
    try:
        prob = pa.BaseProblem(cfg)
        prob.setUp()
        prob.setUpSolver()
    finally:
        opts.delValue("kle_mat_type")
        opts.delValue("kle_op_type")
    ctx.synchronize()
    t1 = time.perf_counter()
    m1 = hip.free_bytes()
    fo = prob.operator.Curl.createVecLeft()
    prob.evalRHS(None, 0.0, prob.vort, fo)
    ctx.synchronize()
    t2 = time.perf_counter()
    ksp = prob.solverKLE.getKSP()
    vel = prob.solverKLE.getSolution()
    rhs = vel.duplicate()
    for _w in range(3):
        eval_rhs_chain(call, prob, vel, rhs, fo)
    chain_ms = [hip.timed_ms(lambda: [eval_rhs_chain(call, prob, vel, rhs, fo) for _r in range(20)]) / 20
                for _ in range(a.rounds)]
    out = fo.getArray()
    emit({"leg": "config4_eval_rhs", "nelem": nelem, "ngl": ngl, "nodes": prob.dom.mesh.N,
          "options": "-kle_mat_type element -kle_op_type element",
          "formats": {n: getattr(prob.operator, n).getFormat() for n in OPS} | {"K": prob.mat.K.getFormat()},
          "whole_eval_rhs_ran_on_one_gpu": bool(np.all(np.isfinite(out))),
          "setup_wall_s": t1 - t0, "eval_rhs_wall_s": t2 - t1,
          "kle_iterations": ksp.getIterationNumber(), "kle_reason": ksp.getConvergedReason(),
          "chain_ms": spread(chain_ms),
          "device_memory": {"bytes_after_setup": m0 - m1, "bytes_after_eval_rhs": m0 - hip.free_bytes()},
          "assembled_counterpart": "not built: by SURVEY section 7's entry counts the assembled Curl, SrT and DivSrT "
                                   "hold about 320 GB at this size, more than one MI355X's 288 GB"})


NS_WALLS = {"up": [1.0, 0.0, 0.0], "down": [0.0, 0.0, 0.0], "left": [0.0, 0.0, 0.0], "right": [0.0, 0.0, 0.0],
            "front": [0.0, 0.0, 0.0], "back": [0.0, 0.0, 0.0]}


def noslip(a, pa, np, hip, ctx, emit):
    from pynama_amd.petsc import Mat

    def parse(spec):
        ne_s, ngl = spec.split(":")
        return [int(v) for v in ne_s.split(",")], int(ngl)

    def domain(nelem, ngl, bc):
        dom = pa.Domain()
        dom.configure({"domain": {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": [0.0] * 3, "upper": [1.0] * 3}},
                       "boundary-conditions": bc})
        dom.setUp()
        return dom

    def build(dom, kind):
        mat = pa.MatNS()
        mat.setDomain(dom)
        mat.build(buildOperators=False, nsType=kind)
        ctx.synchronize()
        return mat

    # the largest candidate mesh on which the assembled set can be built
    wanted, refused = a.meshes[0], []
    for spec in [wanted] + list(a.fallback_meshes):
        nelem, ngl = parse(spec)
        dom = domain(nelem, ngl, {"no-slip": NS_WALLS})
        try:
            build(dom, "assembled")
            break
        except pa.Error as e:
            refused.append({"mesh": spec, "error": str(e)})
            del dom
            gc.collect()
    else:
        raise SystemExit("elem_ab --noslip: the assembled no-slip set could not be built on any mesh")
    gc.collect()
    dim = 3
    base = {"nelem": nelem, "ngl": ngl, "dofs": dom.mesh.N * dim, "walls": sorted(NS_WALLS), "rounds": a.rounds,
            "mesh_wanted": wanted, "assembled_refused_on": refused}
    kinds = ("assembled", "element")
    mats, t_build, mem = {}, {k: [] for k in kinds}, {}
    for rnd in range(a.rounds + 1):  # round 0: untimed (module load, first allocations)
        for kt in kinds:
            mats.pop(kt, None)
            gc.collect()
            ctx.synchronize()
            m0 = hip.free_bytes()
            t0 = time.perf_counter()
            mats[kt] = build(dom, kt)
            t1 = time.perf_counter()
            if rnd:
                t_build[kt].append(1e3 * (t1 - t0))
                mem[kt] = m0 - hip.free_bytes()
    for kt in kinds:
        emit(dict(base, leg="build_ns", nsType=kt, formats=[m.getFormat() for m in mats[kt].kle],
                  ms=spread(t_build[kt]), device_memory={"bytes_kle_and_Ksum": mem[kt]}))
    emit(dict(base, leg="ratio_build_ns", assembled_over_element={
        "build": statistics.median(t_build["assembled"]) / statistics.median(t_build["element"]),
        "device_memory": mem["assembled"] / max(mem["element"], 1)}))

    def get(mat, nm):
        return mat.getKplusKfs() if nm == "K+Kfs" else getattr(mat, nm)

    def time_legs(ops, x, y):
        t = {k: [] for k in ops}
        for _ in range(a.rounds):
            for label, A in ops.items():
                for _w in range(20):
                    A.mult(x, y)
                ms = hip.timed_ms(lambda: [A.mult(x, y) for _r in range(a.reps)])
                t[label].append(1e3 * ms / a.reps)
        return t

    for nm in ("K", "K+Kfs", "Krhsfs", "Rwfs"):
        ops = {kt: get(mats[kt], nm) for kt in kinds}
        x = ops["element"].createVecRight()
        x.setArray(np.random.default_rng(1).uniform(-1, 1, x.getLocalSize()))
        y = ops["element"].createVecLeft()
        t = time_legs(ops, x, y)
        for label, A in ops.items():
            emit(dict(base, leg="product_" + nm, operator=label, kernel=A.spmvKernel(), bytes=A.spmvBytes(),
                      reps=a.reps, us=spread(t[label])))
        emit(dict(base, leg="ratio_" + nm, assembled_over_element=statistics.median(t["assembled"]) /
                  statistics.median(t["element"]),
                  element_faster_beyond_spread=bool(max(t["element"]) < min(t["assembled"]))))
    # the wider index table: per-DoF K against the per-node free-slip K on the same lattice
    fs = domain(nelem, ngl, {"custom-func": {"name": "taylor_green3d"}})
    ops = {"per_dof": mats["element"].K, "per_node": Mat.createKLEElement(fs.mesh, "K")}
    x = ops["per_dof"].createVecRight()
    x.setArray(np.random.default_rng(1).uniform(-1, 1, x.getLocalSize()))
    y = ops["per_dof"].createVecLeft()
    t = time_legs(ops, x, y)
    for label, A in ops.items():
        emit(dict(base, leg="product_K_dof_vs_node", operator=label, kernel=A.spmvKernel(), bytes=A.spmvBytes(),
                  reps=a.reps, us=spread(t[label])))
    emit(dict(base, leg="ratio_K_dof_vs_node", per_dof_over_per_node=statistics.median(t["per_dof"]) /
              statistics.median(t["per_node"]),
              differ_beyond_spread=bool(max(t["per_node"]) < min(t["per_dof"]) or max(t["per_dof"]) < min(t["per_node"]))))
    del ops, fs
    # one solveFS + solve with nothing of the KLE system assembled
    mat = mats["element"]
    sol = pa.KleSolver()
    sol.setMat(mat)
    sol.setUp()
    vort = mat.Rw.createVecRight()
    vort.setArray(np.random.default_rng(3).uniform(-1, 1, vort.getLocalSize()))
    vel = sol.getSolution()
    dom.applyBoundaryConditions(vel, "velocity", 0.0, 0.02)
    ctx.synchronize()
    t0 = time.perf_counter()
    sol.solveFS(vort)
    ctx.synchronize()
    t1 = time.perf_counter()
    sol.solve(vort)
    ctx.synchronize()
    t2 = time.perf_counter()
    emit(dict(base, leg="solve_ns", nsType="element", ksp="cg + jacobi", rtol=1e-10,
              solveFS={"wall_ms": 1e3 * (t1 - t0), "iterations": sol.solverFS.getIterationNumber(),
                       "reason": sol.solverFS.getConvergedReason(), "operator": mat.getKplusKfs().spmvKernel()},
              solve={"wall_ms": 1e3 * (t2 - t1), "iterations": sol.getKSP().getIterationNumber(),
                     "reason": sol.getKSP().getConvergedReason(), "operator": mat.K.spmvKernel()},
              finite=bool(np.all(np.isfinite(vel.getArray())))))


def sumfac_noslip(a, pa, np, hip, ctx, emit):
    import tempfile

    from pynama_amd.meshgen import perturbed_box, write_gmsh
    from pynama_amd.petsc import Mat
    ne_s, ngl = a.meshes[0].split(":")
    nelem, ngl = [int(v) for v in ne_s.split(",")], int(ngl)
    dim = len(nelem)
    path = os.path.join(tempfile.mkdtemp(prefix="kle_sumfac_noslip_"), "mesh.msh")
    write_gmsh(path, dim, *perturbed_box(dim, nelem, seed=5))

    def domain(bc):
        dom = pa.Domain()
        dom.configure({"domain": {"ngl": ngl, "gmsh-file": path}, "boundary-conditions": bc})
        dom.setUp()
        return dom

    def build(dom, kind):
        mat = pa.MatNS()
        mat.setDomain(dom)
        mat.build(buildOperators=False, nsType=kind)
        ctx.synchronize()
        return mat

    dom = domain({"no-slip": NS_WALLS})
    base = {"mesh": "perturbed_box seed 5", "nelem": nelem, "ngl": ngl, "dofs": dom.mesh.N * dim,
            "walls": sorted(NS_WALLS), "rounds": a.rounds}
    kinds = ["sumfac", "assembled"]
    mats, t_build, mem, refused = {}, {k: [] for k in kinds}, {}, None
    for rnd in range(a.rounds + 1):  # round 0: untimed (module load, first allocations)
        for kt in list(kinds):
            mats.pop(kt, None)
            gc.collect()
            ctx.synchronize()
            m0 = hip.free_bytes()
            t0 = time.perf_counter()
            try:
                mats[kt] = build(dom, kt)
            except pa.Error as e:
                if kt != "assembled":
                    raise
                refused = {"error": str(e), "free_bytes_before": m0}
                kinds.remove(kt)
                gc.collect()
                continue
            t1 = time.perf_counter()
            if rnd:
                t_build[kt].append(1e3 * (t1 - t0))
                mem[kt] = m0 - hip.free_bytes()
    for kt in kinds:
        emit(dict(base, leg="build_ns", nsType=kt, formats=[m.getFormat() for m in mats[kt].kle],
                  ms=spread(t_build[kt]), device_memory={"bytes_kle_and_Ksum": mem[kt]}))
    if refused:
        emit(dict(base, leg="build_ns", nsType="assembled", fits=False, **refused))
    else:
        emit(dict(base, leg="ratio_build_ns", assembled_over_sumfac={
            "build": statistics.median(t_build["assembled"]) / statistics.median(t_build["sumfac"]),
            "device_memory": mem["assembled"] / max(mem["sumfac"], 1)}))

    def get(mat, nm):
        return mat.getKplusKfs() if nm == "K+Kfs" else getattr(mat, nm)

    def time_legs(ops, x, y):
        t = {k: [] for k in ops}
        for _ in range(a.rounds):
            for label, A in ops.items():
                for _w in range(20):
                    A.mult(x, y)
                ms = hip.timed_ms(lambda: [A.mult(x, y) for _r in range(a.reps)])
                t[label].append(1e3 * ms / a.reps)
        return t

    for nm in ("K", "Krhs", "Rw", "Kfs", "Krhsfs", "Rwfs", "K+Kfs"):
        ops = {kt: get(mats[kt], nm) for kt in kinds}
        x = ops["sumfac"].createVecRight()
        x.setArray(np.random.default_rng(1).uniform(-1, 1, x.getLocalSize()))
        y = ops["sumfac"].createVecLeft()
        t = time_legs(ops, x, y)
        for label, A in ops.items():
            emit(dict(base, leg="product_" + nm, operator=label, kernel=A.spmvKernel(), bytes=A.spmvBytes(),
                      reps=a.reps, us=spread(t[label]),
                      tb_per_s=A.spmvBytes() / statistics.median(t[label]) * 1e-6))
        if "assembled" in t:
            emit(dict(base, leg="ratio_" + nm, assembled_over_sumfac=statistics.median(t["assembled"]) /
                      statistics.median(t["sumfac"]),
                      differ_beyond_spread=bool(max(t["sumfac"]) < min(t["assembled"]) or
                                                max(t["assembled"]) < min(t["sumfac"]))))
    # the class table: the masked K against the free-slip K of the same mesh (per-node mask in the connectivity)
    fs = domain({"custom-func": {"name": "taylor_green3d" if dim == 3 else "taylor_green"}})
    ops = {"per_dof_class": mats["sumfac"].K, "per_node": Mat.createKLESumFactored(fs.mesh, "K")}
    x = ops["per_dof_class"].createVecRight()
    x.setArray(np.random.default_rng(1).uniform(-1, 1, x.getLocalSize()))
    y = ops["per_dof_class"].createVecLeft()
    t = time_legs(ops, x, y)
    for label, A in ops.items():
        emit(dict(base, leg="product_K_cls_vs_node", operator=label, kernel=A.spmvKernel(), bytes=A.spmvBytes(),
                  reps=a.reps, us=spread(t[label])))
    bc, bn = ops["per_dof_class"].spmvBytes(), ops["per_node"].spmvBytes()
    emit(dict(base, leg="ratio_K_cls_vs_node", per_dof_class_over_per_node=statistics.median(t["per_dof_class"]) /
              statistics.median(t["per_node"]), bytes_ratio=bc / bn, class_table_share_of_bytes=(bc - bn) / bc,
              differ_beyond_spread=bool(max(t["per_node"]) < min(t["per_dof_class"]) or
                                        max(t["per_dof_class"]) < min(t["per_node"]))))
    del ops, fs
    gc.collect()
    # one solveFS + solve with nothing of the KLE system assembled; true residuals through the assembled matrices
    mat = mats["sumfac"]
    sol = pa.KleSolver()
    sol.setMat(mat)
    sol.setUp()
    vort = mat.Rw.createVecRight()
    vort.setArray(np.random.default_rng(3).uniform(-1, 1, vort.getLocalSize()))
    vel = sol.getSolution()
    dom.applyBoundaryConditions(vel, "velocity", 0.0, 0.02)
    asm = mats.get("assembled")
    true = {}
    if asm is not None:  # the right-hand sides before the solves overwrite vel's free entries
        bfs = asm.Rw * vort
        bfs.axpy(1.0, asm.Rwfs * vort)
        bfs.axpy(1.0, asm.Krhsfs * vel)
        b = asm.Rw * vort
        b.axpy(1.0, asm.Krhs * vel)
    ctx.synchronize()
    t0 = time.perf_counter()
    sol.solveFS(vort)
    ctx.synchronize()
    t1 = time.perf_counter()
    sol.solve(vort)
    ctx.synchronize()
    t2 = time.perf_counter()
    if asm is not None:
        r = asm.getKplusKfs() * sol.getFreeSlipSolution()
        r.aypx(-1.0, bfs)
        true["solveFS"] = r.norm() / bfs.norm()
        r = asm.K * vel
        r.aypx(-1.0, b)
        true["solve"] = r.norm() / b.norm()
    emit(dict(base, leg="solve_ns", nsType="sumfac", ksp="cg + jacobi", rtol=1e-10,
              solveFS={"wall_ms": 1e3 * (t1 - t0), "iterations": sol.solverFS.getIterationNumber(),
                       "reason": sol.solverFS.getConvergedReason(), "operator": mat.getKplusKfs().spmvKernel()},
              solve={"wall_ms": 1e3 * (t2 - t1), "iterations": sol.getKSP().getIterationNumber(),
                     "reason": sol.getKSP().getConvergedReason(), "operator": mat.K.spmvKernel()},
              true_rel_residual_assembled=true or None, finite=bool(np.all(np.isfinite(vel.getArray())))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", nargs="+", default=["20,16,16:5", "8,8,6:7"], help="nelem:ngl")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--its", type=int, default=50)
    ap.add_argument("--check", action="store_true", help="full-size correctness on the first mesh")
    ap.add_argument("--matfree", action="store_true",
                    help="the matrix-free legs: build time and memory per kleType, the Rw product")
    ap.add_argument("--operators", action="store_true",
                    help="the collocation-operator legs: build, products and the evalRHS chain per opType")
    ap.add_argument("--config4", action="store_true",
                    help="with --operators: one evalRHS at [18,18,18] ngl 7 with nothing assembled, instead of the legs")
    ap.add_argument("--noslip", action="store_true",
                    help="the matrix-free no-slip legs on a six-wall lid-driven box at the first mesh")
    ap.add_argument("--sumfac", action="store_true",
                    help="the sum-factorised K: the first mesh as bench.py's unstructured mesh (vs the assembled K) "
                         "and as a box (vs the dense-GEMM element K)")
    ap.add_argument("--sumfac-system", action="store_true",
                    help="the whole matrix-free set (K, Krhs, Rw, Curl, SrT, DivSrT) on the first mesh as an "
                         "unstructured mesh and as a box: builds, products, the evalRHS chain, one evalRHS")
    ap.add_argument("--sumfac-noslip", action="store_true",
                    help="the matrix-free no-slip set (K, Krhs, Rw, Kfs, Krhsfs, Rwfs, K+Kfs) on the first mesh as "
                         "an unstructured six-wall mesh: builds, products, the class table's price, solveFS + solve")
    ap.add_argument("--fallback-meshes", nargs="*", default=["16,12,12:5", "12,10,10:5", "8,8,6:5"],
                    help="with --noslip: tried in order where the assembled no-slip set cannot be built")
    ap.add_argument("--out", default=None, help="default profiles/elem/elem_ab.jsonl (matfree.jsonl with --matfree, "
                                                "operators.jsonl with --operators, noslip.jsonl with --noslip)")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "elem", "sumfac_noslip.jsonl" if a.sumfac_noslip else
                             "sumfac_system.jsonl" if a.sumfac_system else
                             "sumfac.jsonl" if a.sumfac else "noslip.jsonl" if a.noslip else
                             "operators.jsonl" if a.operators else
                             "matfree.jsonl" if a.matfree else "elem_ab.jsonl")
    import numpy as np

    import pynama_amd as pa
    ctx = pa.get_ctx()
    hip = Hip(ctx)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    fout = open(a.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        fout.write(line + "\n")
        fout.flush()

    if a.sumfac_noslip:
        sumfac_noslip(a, pa, np, hip, ctx, emit)
        fout.close()
        return
    if a.sumfac_system:
        sumfac_system(a, pa, np, hip, ctx, emit)
        fout.close()
        return
    if a.sumfac:
        sumfac(a, pa, np, hip, ctx, emit)
        fout.close()
        return
    if a.noslip:
        noslip(a, pa, np, hip, ctx, emit)
        fout.close()
        return
    if a.operators:
        (config4 if a.config4 else operators)(a, pa, np, hip, ctx, emit)
        fout.close()
        return
    if a.matfree:
        matfree(a, pa, np, hip, ctx, emit)
        fout.close()
        return
    for mi, spec in enumerate(a.meshes):
        ne_s, ngl = spec.split(":")
        nelem, ngl = [int(v) for v in ne_s.split(",")], int(ngl)
        dim = len(nelem)
        cfg = {"domain": {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": [0.0] * dim, "upper": [1.0] * dim}},
               "boundary-conditions": {"custom-func": {"name": "taylor_green3d" if dim == 3 else "taylor_green"}}}
        dom = pa.Domain()
        dom.configure(cfg)
        dom.setUp()
        ctx.synchronize()
        m0 = hip.free_bytes()
        mat = pa.MatFS()
        mat.setDomain(dom)
        mat.build(buildOperators=False)
        ctx.synchronize()
        m1 = hip.free_bytes()
        Ke = mat.getElementK()
        ctx.synchronize()
        m2 = hip.free_bytes()
        ops = {"assembled": mat.K, "element": Ke}
        nd, E = dim * ngl ** dim, dom.mesh.E
        base = {"nelem": nelem, "ngl": ngl, "dofs": mat.K.getSize()[0], "rounds": a.rounds}
        x = mat.K.createVecRight()
        x.setArray(np.random.default_rng(1).uniform(-1, 1, x.getLocalSize()))
        y = mat.K.createVecLeft()
        b = mat.K.createVecLeft()
        b.setArray(np.random.default_rng(2).uniform(-1, 1, b.getLocalSize()))
        ksps = {}
        for label, A in ops.items():
            ksp = pa.petsc.KSP().create()
            ksp.setType("cg")
            pc = pa.petsc.PC().create()
            pc.setType("jacobi")
            ksp.setPC(pc)
            ksp.setCGSingleReduction(False)
            ksp.setOperators(A)
            ksp.setUp()
            ksp.setFixedIterations(a.its)
            ksps[label] = (ksp, A.createVecRight())
        t_prod = {k: [] for k in ops}
        t_cg = {k: [] for k in ops}
        for _ in range(a.rounds):
            for label, A in ops.items():
                for _w in range(20):
                    A.mult(x, y)
                ms = hip.timed_ms(lambda: [A.mult(x, y) for _r in range(a.reps)])
                t_prod[label].append(1e3 * ms / a.reps)
            for label, (ksp, u) in ksps.items():
                u.set(0.0)
                ksp.solve(b, u)  # warm-up: the same fixed iterations
                u.set(0.0)
                ms = hip.timed_ms(lambda: ksp.solve(b, u))
                if ksp.getConvergedReason() < 0:
                    raise SystemExit(f"elem_ab: the fixed CG iterations diverged ({label})")
                t_cg[label].append(1e3 * ms / a.its)
        mem = {"assembled": {"bytes_K_Krhs_Rw": m0 - m1}, "element": {"bytes_K": m1 - m2}}
        for label, A in ops.items():
            flops = 2.0 * nd * nd * E if label == "element" else 2.0 * A.getInfo()["nz_used"]
            emit(dict(base, leg="product", operator=label, kernel=A.spmvKernel(), bytes=A.spmvBytes(), flops=flops,
                      reps=a.reps, us=spread(t_prod[label]), device_memory=mem[label]))
        for label, (ksp, _u) in ksps.items():
            emit(dict(base, leg="cg", operator=label, ksp="cg (classic) + jacobi", kernel=ops[label].spmvKernel(),
                      iterations=a.its, us_per_iteration=spread(t_cg[label])))
        ratio = {"product": statistics.median(t_prod["assembled"]) / statistics.median(t_prod["element"]),
                 "cg_iteration": statistics.median(t_cg["assembled"]) / statistics.median(t_cg["element"])}
        emit(dict(base, leg="ratio", assembled_over_element=ratio,
                  gate_element_cg_not_slower=bool(ratio["cg_iteration"] >= 1.0) if mi == 0 else None))
        if a.check and mi == 0:
            emit(dict(base, leg="check_product", **check_product(pa, np, dom, mat, Ke)))
            emit(dict(base, leg="check_solve", **check_solve(pa, np, mat, Ke)))
        del ksps, ops, Ke, mat, dom, x, y, b
    fout.close()


if __name__ == "__main__":
    main()
