"""The element-wise no-slip operators (Mat.createNSElement, kle_elem.hip) on
several ranks: slab-partitioned box meshes with no-slip walls, at most 3 ranks
on one GPU, launched as tests/test_gpu_elem_ranks.py launches its ranks
(torch.multiprocessing spawn, gloo, KLE_TRANSPORT=host or ipc); one spawned run
per configuration is cached and shared by the assertions on it.

x of every product is sin(arange) over each rank's ownership range of the
column space.  For all seven operators the concatenated owned rows must be the
one-rank product of the same operator (made in the parent) bit for bit, with
halo overlap on and off.

solveFS + solve (MatNS.build(nsType="element"), CG + Jacobi at rtol 1e-12)
against the one-rank run of the same code: the operators are the same bits, so
the runs differ by the allreduce rounding of the dot products alone, amplified
by the solve.  The measured difference is printed; 1e-10 relative is asserted."""
import functools
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS_OPS = ("K", "Krhs", "Rw", "Kfs", "Krhsfs", "Rwfs", "K+Kfs")
CAVITY = {"up": [2, 0], "down": [0, 0], "left": [0, 0], "right": [0, 0]}
SIX = {"up": [1, 0, 0.5], "down": [0, 0, 0], "left": [0, 0, 0], "right": [0, 0, 0], "front": [0, 0, 0],
       "back": [0, 0, 0]}
SHAPES = {
    # 2-D, partition axis y: two layers per rank / uneven layers 2 / 1 / 1
    "r2_cavity_3x4_p4": dict(size=2, nelem=[3, 4], ngl=4, walls=CAVITY),
    "r3_cavity_3x4_p4": dict(size=3, nelem=[3, 4], ngl=4, walls=CAVITY),
    "r2_six_2x2x4_p3": dict(size=2, nelem=[2, 2, 4], ngl=3, walls=SIX),
    # one layer per rank: the middle rank has no interior element
    "r3_six_2x2x3_p3": dict(size=3, nelem=[2, 2, 3], ngl=3, walls=SIX),
}
SOLVE_RTOL = 1e-12


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _product(A, x):
    xv = A.createVecRight()
    xv.setArray(x)
    return (A * xv).getArray().copy()


def _run_case(pa, spec):
    """What every rank (and the parent, on one rank) computes."""
    dim = len(spec["nelem"])
    dom = pa.Domain()
    dom.configure({"domain": {"ngl": spec["ngl"], "box-mesh": {"nelem": list(spec["nelem"]), "lower": [0.0] * dim,
                                                               "upper": [1.0] * dim}},
                   "boundary-conditions": {"no-slip": spec["walls"]}})
    dom.setUp()
    mat = pa.MatNS()
    mat.setDomain(dom)
    mat.build(buildOperators=False, nsType="element")
    ops = dict(zip(NS_OPS, (mat.K, mat.Krhs, mat.Rw, mat.Kfs, mat.Krhsfs, mat.Rwfs, mat.getKplusKfs())))
    res = {"transport": pa.get_ctx().device_info()["transport"], "node_range": tuple(dom.getMesh().node_range),
           "ops": {}}
    for nm, A in ops.items():
        assert A.getFormat() == "elem", nm
        clo, chi = A.createVecRight().getOwnershipRange()
        x = np.sin(np.arange(clo, chi, dtype=np.float64))
        y = _product(A, x)
        A.setHaloOverlap(False)
        y_plain = _product(A, x)
        A.setHaloOverlap(True)
        reps = [_product(A, x) for _ in range(3)]
        r = {"y": y, "plain_equal": y_plain.tobytes() == y.tobytes(),
             "repeat_equal": all(v.tobytes() == y.tobytes() for v in reps), "nz": A.getInfo()["nz_used"],
             "kernel": A.spmvKernel()}
        if nm not in ("Rw", "Rwfs"):
            r["diag"] = A.getDiagonal().getArray().copy()
        res["ops"][nm] = r
    sol = pa.KleSolver()
    sol.setMat(mat)
    sol.setUp()
    sol.getKSP().setTolerances(rtol=SOLVE_RTOL)
    sol.solverFS.setTolerances(rtol=SOLVE_RTOL)
    vort = mat.Rw.createVecRight()
    vort.setArray(np.cos(0.37 * np.arange(*vort.getOwnershipRange(), dtype=np.float64)))
    vel = sol.getSolution()
    dom.applyBoundaryConditions(vel, "velocity", 0.0, 0.02)
    ubc = vel.getArray().copy()
    sol.solveFS(vort)
    vfs = sol.getFreeSlipSolution().getArray().copy()
    sol.solve(vort)
    res["solve"] = {"u": vel.getArray().copy(), "vfs": vfs, "ubc": ubc,
                    "reason": (sol.solverFS.getConvergedReason(), sol.getKSP().getConvergedReason()),
                    "its": (sol.solverFS.getIterationNumber(), sol.getKSP().getIterationNumber())}
    res["cls_tang"] = np.asarray(sorted(dom.getTangDofs(collect=True)), np.int64)
    res["cls_normal"] = np.asarray(sorted(dom.getNormalDofs(collect=True)), np.int64)
    return res


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
        res = _run_case(pa, spec)
        res["rank"] = rank
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


@functools.lru_cache(maxsize=None)
def _run(name, transport="host"):
    import torch.multiprocessing as mp
    spec = SHAPES[name]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, spec["size"], port, spec, q, transport))
             for r in range(spec["size"])]
    return _collect(procs, q, spec["size"])


@functools.lru_cache(maxsize=None)
def _one(name):
    import pynama_amd as pa
    pa.load()
    return _run_case(pa, SHAPES[name])


def _cat(res, nm, key="y"):
    return np.concatenate([r["ops"][nm][key] for r in res])


def _check_products(name, res, one, transport):
    spec = SHAPES[name]
    assert [r["transport"] for r in res] == [transport] * spec["size"]
    assert res[0]["node_range"][0] == 0 and res[-1]["node_range"][1] == one["node_range"][1]
    assert all(a["node_range"][1] == b["node_range"][0] for a, b in zip(res, res[1:]))
    for nm in NS_OPS:
        for r in res:
            o = r["ops"][nm]
            assert o["plain_equal"], (nm, r["rank"])
            assert o["repeat_equal"], (nm, r["rank"])
            assert o["nz"] == 0 and "k_elem_gather_cls" in o["kernel"], (nm, o["kernel"])
        y, y1 = _cat(res, nm), one["ops"][nm]["y"]
        assert y.shape == y1.shape
        diff = np.nonzero(y.view(np.int64) != y1.view(np.int64))[0]
        assert y.tobytes() == y1.tobytes(), (name, nm, len(diff), diff[:8].tolist())
        assert np.any(y != 0.0), nm
        if nm not in ("Rw", "Rwfs"):
            assert _cat(res, nm, "diag").tobytes() == one["ops"][nm]["diag"].tobytes(), (name, nm)


@pytest.mark.parametrize("name", list(SHAPES))
def test_products_on_ranks(name):
    _check_products(name, _run(name), _one(name), "host")


def test_ipc_transport_same_bits():
    name = "r3_six_2x2x3_p3"
    _check_products(name, _run(name, "ipc"), _one(name), "ipc")


@pytest.mark.parametrize("name", list(SHAPES))
def test_solves_on_ranks(name):
    res, one = _run(name), _one(name)
    sv = [r["solve"] for r in res]
    u, vfs, ubc = (np.concatenate([s[k] for s in sv]) for k in ("u", "vfs", "ubc"))
    o = one["solve"]
    for s in sv + [o]:
        assert s["reason"][0] > 0 and s["reason"][1] > 0, s["reason"]
    rel_fs = np.linalg.norm(vfs - o["vfs"]) / np.linalg.norm(o["vfs"])
    rel_u = np.linalg.norm(u - o["u"]) / np.linalg.norm(o["u"])
    print(f"{name}: |velFS - one rank| / |.| {rel_fs:.3e}  |u - one rank| / |.| {rel_u:.3e}  "
          f"iterations {sv[0]['its']} (one rank {o['its']})")
    assert rel_fs <= 1e-10 and rel_u <= 1e-10
    # the identity rows come back exactly: N entries of velFS, wall entries of u
    n = len(u)
    wall, normal = np.zeros(n, bool), np.zeros(n, bool)
    wall[one["cls_tang"]] = True
    wall[one["cls_normal"]] = normal[one["cls_normal"]] = True
    assert ubc.tobytes() == o["ubc"].tobytes() and np.any(ubc[wall] != 0.0)
    assert u[wall].tobytes() == ubc[wall].tobytes()
    assert vfs[normal].tobytes() == ubc[normal].tobytes()
