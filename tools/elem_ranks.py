"""The element-wise K on a slab partition, every part timed alone on one GPU:
N ranks share the GPU over the IPC transport (KLE_TRANSPORT=ipc, as bench.py's
one-GPU rehearsals of the multi-GPU configs), each builds its part of the mesh
-- the assembled K as bench.py configures it (symmetric storage on bricks) and
the element-wise K (Mat.createKLEElement) -- and then, rank by rank behind
barriers so that parts never share the GPU, calls Mat.timeLocalSpmv
(kle_mat_time_local_spmv: the part's own launches, no halo) on

  element        the GEMM over its local elements and the owned-row gather,
                 the ghost layer over the row groups of its top plane alone
  element_full   the same with the ghost layer over every row group
                 (tuning elem_ghost_rows 0)
  brick          its assembled brick part

--rounds rounds; per rank one JSON line with the median and spread of each,
appended to --out.  Then one matrix-free solve (MatFS.build(kleType="element")
+ KleSolver on Taylor-Green, rtol 1e-10) on the N ranks: its iteration count
and true residual, one more line.  No cross-GPU run is made here: every rank is
on GPU 0.

With --sumfac the mesh is unstructured -- perturbed_box(dim, nelem, seed=5)
written as a Gmsh file, inertial partition -- and the legs are the
sum-factorised operators of a partitioned mesh (-kle_mat_type sumfac
-kle_op_type sumfac: K, Rw, Curl, SrT, DivSrT; kle_sumfac.hip, kle_colloc.hip)
against the assembled part of the same rank (K on graph bricks where the part
is large enough for them, the others node-block), every part alone behind
barriers with timeLocalSpmv (both element lists and the gather, or the
assembled part's rows, no halo).  Per rank one JSON line with the median and
spread of each; then one matrix-free solve (KleSolver on the sum-factorised K,
Taylor-Green, rtol 1e-10) on the N ranks.  --ranks 1 runs the same script on
one rank (host transport) and writes the solve's line alone: the one to compare
the N-rank iteration count and true residual with.  Records to profiles/elem/sumfac_ranks.jsonl.

  python tools/elem_ranks.py [--ranks 8] [--mesh 20,16,16:5] [--rounds 3] [--reps 50] [--sumfac]
"""
import argparse
import json
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    m = statistics.median(v)
    return {"median": m, "min": min(v), "max": max(v), "spread_pct": 100.0 * (max(v) - min(v)) / m}


def worker(rank, a, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), KLE_TRANSPORT="ipc", RANK=str(rank),
                      WORLD_SIZE=str(a.ranks))
    import numpy as np
    import torch  # noqa: F401
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=a.ranks)
    try:
        import pynama_amd as pa
        ne_s, ngl = a.mesh.split(":")
        nelem, ngl = [int(v) for v in ne_s.split(",")], int(ngl)
        dim = len(nelem)
        cfg = {"domain": {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": [0.0] * dim, "upper": [1.0] * dim}},
               "boundary-conditions": {"custom-func": {"name": "taylor_green3d" if dim == 3 else "taylor_green"}}}
        dom = pa.Domain()
        dom.configure(cfg)
        dom.setUp()
        mat = pa.MatFS()
        mat.setDomain(dom)
        mat.build(buildOperators=False)
        K, Ke = mat.K, mat.getElementK()
        lo, hi = K.getOwnershipRange()
        x, y = K.createVecRight(), K.createVecLeft()
        x.setArray(np.random.default_rng(1).uniform(-1, 1, dim * dom.mesh.N)[lo:hi])
        legs = {"element": [], "element_full": [], "brick": []}
        brick = K.spmvKernel().startswith("k_nb_spmv_sym_brick<")
        for _ in range(a.rounds):
            for t in range(a.ranks):
                dist.barrier()
                if t != rank:
                    continue
                for leg in legs:
                    if leg == "brick" and not brick:
                        continue
                    A = K if leg == "brick" else Ke
                    pa.runtime.set_tuning("elem_ghost_rows", 0 if leg == "element_full" else 1)
                    A.timeLocalSpmv(x, y, 10)  # warm-up
                    legs[leg].append(1e3 * A.timeLocalSpmv(x, y, a.reps))
                pa.runtime.set_tuning("elem_ghost_rows", 1)
            dist.barrier()
        el = dom.mesh.elem_range
        rec = {"leg": "local_product", "rank": rank, "ranks": a.ranks, "nelem": nelem, "ngl": ngl,
               "transport": pa.get_ctx().device_info()["transport"], "owned_dofs": hi - lo,
               "local_elements": el[1] - el[0], "rounds": a.rounds, "reps": a.reps,
               "kernel": {"element": Ke.spmvKernel(), "brick": K.spmvKernel()},
               "bytes": {"element": Ke.spmvBytes(), "brick": K.spmvBytes()},
               "us": {k: spread(v) for k, v in legs.items() if v}}
        del K, Ke, mat, x, y
        # the matrix-free solve on the same ranks
        mf = pa.MatFS()
        mf.setDomain(dom)
        mf.build(buildOperators=False, kleType="element")
        sol = pa.KleSolver()
        sol.setMat(mf)
        sol.setUp()
        f = pa.fields.get("taylor_green3d" if dim == 3 else "taylor_green")
        vort = mf.Rw.createVecRight()
        vort.setArray(np.asarray(f.vorticity(dom.getFullCoordArray(), 1.0), np.float64).ravel())
        vel = sol.getSolution()
        dom.applyBoundaryConditions(vel, "velocity", 0.0, 0.02)
        sol.solve(vort)
        ksp = sol.getKSP()
        rec["solve"] = {"leg": "matrix_free_solve", "ranks": a.ranks, "nelem": nelem, "ngl": ngl,
                        "ksp": ksp.getType() + " + jacobi", "rtol": 1e-10, "iterations": ksp.getIterationNumber(),
                        "correction_iterations": ksp.getCorrectionIterations(), "reason": ksp.getConvergedReason(),
                        "true_relative_residual": ksp.getTrueRelativeResidual(), "kernel": mf.K.spmvKernel(),
                        "cross_gpu_run": False}
        q.put(rec)
    except Exception:
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc()})
    finally:
        dist.destroy_process_group()


SUMFAC_LEGS = ("K", "Rw", "Curl", "SrT", "DivSrT")


def worker_sumfac(rank, a, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), KLE_TRANSPORT="ipc" if a.ranks > 1 else "host",
                      RANK=str(rank), WORLD_SIZE=str(a.ranks))
    import numpy as np
    import torch  # noqa: F401
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=a.ranks)
    try:
        import pynama_amd as pa
        ne_s, ngl = a.mesh.split(":")
        nelem, ngl = [int(v) for v in ne_s.split(",")], int(ngl)
        dim = len(nelem)
        domain = {"ngl": ngl, "gmsh-file": a.msh}
        if a.ranks > 1:
            domain["partitioner"] = "inertial"
        cfg = {"domain": domain,
               "boundary-conditions": {"custom-func": {"name": "taylor_green3d" if dim == 3 else "taylor_green"}}}
        dom = pa.Domain()
        dom.configure(cfg)
        dom.setUp()
        asm = pa.MatFS()
        asm.setDomain(dom)
        asm.build()
        mf = pa.MatFS()
        mf.setDomain(dom)
        mf.build(kleType="sumfac", opType="sumfac")
        pair = {"K": (mf.K, asm.K), "Rw": (mf.Rw, asm.Rw)}
        pair.update({nm: (getattr(mf.getOperators(), nm), getattr(asm.getOperators(), nm)) for nm in SUMFAC_LEGS[2:]})
        vecs = {}
        for nm, (S, _A) in pair.items():
            x, y = S.createVecRight(), S.createVecLeft()
            x.setArray(np.random.default_rng(1).uniform(-1, 1, x.getLocalSize()))
            vecs[nm] = (x, y)
        t = {nm: {"sumfac": [], "assembled": []} for nm in pair}
        # (one rank: the product is the local product -- tools/elem_ab.py --sumfac-system times it)
        for _ in range(a.rounds if a.ranks > 1 else 0):
            for turn in range(a.ranks):
                dist.barrier()
                if turn != rank:
                    continue
                for nm, (S, A) in pair.items():
                    x, y = vecs[nm]
                    for form, M in (("sumfac", S), ("assembled", A)):
                        M.timeLocalSpmv(x, y, 10)  # warm-up
                        t[nm][form].append(1e3 * M.timeLocalSpmv(x, y, a.reps))
            dist.barrier()
        lo, hi = mf.K.getOwnershipRange()
        el = dom.mesh.elem_range
        rec = {"leg": "local_product", "rank": rank, "ranks": a.ranks, "mesh": "perturbed_box seed 5", "nelem": nelem,
               "ngl": ngl, "partitioner": "inertial" if a.ranks > 1 else None,
               "transport": pa.get_ctx().device_info()["transport"], "owned_dofs": hi - lo,
               "local_elements": el[1] - el[0], "peers": len(dom.mesh.peers()), "rounds": a.rounds, "reps": a.reps,
               "kernel": {nm: {"sumfac": S.spmvKernel(), "assembled": A.spmvKernel()} for nm, (S, A) in pair.items()},
               "bytes": {nm: {"sumfac": S.spmvBytes(), "assembled": A.spmvBytes()} for nm, (S, A) in pair.items()},
               "us": {nm: {f: spread(v) for f, v in forms.items() if v} for nm, forms in t.items()},
               "assembled_over_sumfac": {nm: statistics.median(forms["assembled"]) / statistics.median(forms["sumfac"])
                                         for nm, forms in t.items() if forms["sumfac"]}}
        del pair, vecs, asm
        sol = pa.KleSolver()
        sol.setMat(mf)
        sol.setUp()
        f = pa.fields.get("taylor_green3d" if dim == 3 else "taylor_green")
        vort = mf.Rw.createVecRight()
        vort.setArray(np.asarray(f.vorticity(dom.getFullCoordArray(), 1.0), np.float64).ravel())
        vel = sol.getSolution()
        dom.applyBoundaryConditions(vel, "velocity", 0.0, 0.02)
        sol.solve(vort)
        ksp = sol.getKSP()
        rec["solve"] = {"leg": "matrix_free_solve", "ranks": a.ranks, "mesh": "perturbed_box seed 5", "nelem": nelem,
                        "ngl": ngl, "ksp": ksp.getType() + " + jacobi", "rtol": 1e-10,
                        "iterations": ksp.getIterationNumber(),
                        "correction_iterations": ksp.getCorrectionIterations(), "reason": ksp.getConvergedReason(),
                        "true_relative_residual": ksp.getTrueRelativeResidual(), "kernel": mf.K.spmvKernel(),
                        "cross_gpu_run": False}
        q.put(rec)
    except Exception:
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc()})
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--mesh", default="20,16,16:5", help="nelem:ngl")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sumfac", action="store_true",
                    help="the sum-factorised operators on an inertial partition of the perturbed mesh")
    ap.add_argument("--out", default=None, help="default profiles/elem/ranks.jsonl (sumfac_ranks.jsonl with --sumfac)")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "elem", "sumfac_ranks.jsonl" if a.sumfac else "ranks.jsonl")
    if not (1 if a.sumfac else 2) <= a.ranks <= 8:
        raise SystemExit("elem_ranks: 2 to 8 ranks on the one GPU (--sumfac: 1 to 8)")
    target = worker
    if a.sumfac:
        import tempfile

        from pynama_amd.meshgen import perturbed_box, write_gmsh
        nelem = [int(v) for v in a.mesh.split(":")[0].split(",")]
        a.msh = os.path.join(tempfile.mkdtemp(prefix="kle_sumfac_ranks_"), "mesh.msh")
        write_gmsh(a.msh, len(nelem), *perturbed_box(len(nelem), nelem, seed=5))
        target = worker_sumfac
    import queue

    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, a, port, q)) for r in range(a.ranks)]
    for p in procs:
        p.start()
    res = []
    try:
        while len(res) < a.ranks:
            try:
                r = q.get(timeout=5)
            except queue.Empty:
                dead = [(i, p.exitcode) for i, p in enumerate(procs) if p.exitcode not in (None, 0)]
                if dead:
                    raise SystemExit(f"elem_ranks: ranks died (rank, exit code): {dead}")
                continue
            if "error" in r:
                raise SystemExit(f"elem_ranks: rank {r['rank']}: {r['error']}")
            res.append(r)
    except BaseException:
        for p in procs:
            p.kill()
        raise
    for p in procs:
        p.join(timeout=60)
    if a.sumfac:  # the mesh file was the workers' alone
        import shutil
        shutil.rmtree(os.path.dirname(a.msh), ignore_errors=True)
    res.sort(key=lambda r: r["rank"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fout:
        solve = res[0].pop("solve")
        for r in res:
            r.pop("solve", None)
            if a.sumfac and a.ranks == 1:
                continue  # (no part was timed: the solve's line alone)
            line = json.dumps(r)
            print(line, flush=True)
            fout.write(line + "\n")
        line = json.dumps(solve)
        print(line, flush=True)
        fout.write(line + "\n")


if __name__ == "__main__":
    main()
