"""The sum-factorised no-slip operators (Mat.createNSSumFactored,
kle_sumfac.hip) on partitioned meshes: a Gmsh slab partition on 2 ranks, an
inertial partition on 3 (host and IPC transport) and the cavity box on 2 slabs,
all ranks on one GPU, at most 3 processes at once.

Ranks are spawned with the worker harness of tests/test_gpu_sumfac_ranks.py
(test_gpu_sym_ranks_ref.spawn / rank_setup: torch.multiprocessing spawn, gloo,
every worker under a time limit); one spawned run per configuration and one of
the same mesh on one rank, cached and shared by the assertions.  The parent
never opens the GPU: the host meshes, the partition and the inputs are formed
on the CPU (sumfac_ranks_ref.Partition), and rank rows are mapped into the
one-rank numbering by coordinates.

a. Products: mult of the seven operators on two different x in turn (a stale
   halo fails the second): the stitched owned rows are the one-rank product of
   the same operator bit for bit, with halo overlap on and off and on three
   repeats; multAdd = y0 + the product rounded once.  Kfs's two passes share
   one halo: its second product on another x is exact too.
b. Selection through the ghosts: NaN in every entry of a class a pass drops, on
   every rank (so it arrives in ghost slots), leaves that pass's rows bit-equal
   to the clean product.
c. getDiagonal of K, Krhs, Kfs, Krhsfs and K+Kfs: the one-rank diagonal's owned
   rows bit for bit; refused for Rw and Rwfs.
d. solveFS + solve (MatNS.build(nsType="sumfac"), rtol 1e-13) against the same
   code on one rank: 1e-9 relative; the identity rows hold the wall values bit
   for bit on every rank.
e. A mesh partitioned for another rank count is refused with Error 56."""
import numpy as np
import pytest

import sumfac_ns_ref as SN
import sumfac_ranks_ref as SR
import test_gpu_sym_ranks_ref as SRK

pytestmark = pytest.mark.gpu
OPS, SPECS, RW = SN.OPS, SN.SPECS, SN.RW
F, T, N = SN.F, SN.T, SN.N
SIX = {"up": [1, 0, 0.5], "down": [0, 0, 0], "left": [0, 0, 0], "right": [0, 0, 0], "front": [0, 0, 0],
       "back": [0, 0, 0]}
CAVITY = {"up": [2, 0], "down": [0, 0], "left": [0, 0], "right": [0, 0]}
CONFIGS = {
    "slab2": dict(pbox=(3, [3, 3, 4], 5), ngl=3, size=2, part="slab", walls=SIX, solve=True, refusals=True),
    "inertial3": dict(pbox=(3, [3, 3, 4], 5), ngl=3, size=3, part="inertial", walls=SIX, solve=True),
    "inertial3_ipc": dict(pbox=(3, [3, 3, 4], 5), ngl=3, size=3, part="inertial", walls=SIX, transport="ipc",
                          host="inertial3"),
    "cavity2": dict(box=[3, 4], ngl=4, size=2, part=None, walls=CAVITY, solve=True),
}
_RUNS, _PARTS = {}, {}


def _cw(dim, nm):
    return (1 if dim == 2 else 3) if nm in RW else dim


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


def _refused(pa, fn):
    try:
        fn()
    except pa.Error as e:
        return e.ierr
    return 0


def _worker(rank, size, port, cfg, msh, q):
    dist = SRK.rank_setup(rank, size, port, cfg)
    try:
        import pynama_amd as pa
        dim = SR.dim_of(cfg)
        if msh is not None:
            d = {"ngl": cfg["ngl"], "gmsh-file": msh}
            if size > 1:
                d["partitioner"] = cfg["part"]
        else:
            d = {"ngl": cfg["ngl"], "box-mesh": {"nelem": cfg["box"], "lower": [0] * dim, "upper": [1] * dim}}
        dom = pa.Domain()
        dom.configure({"domain": d, "boundary-conditions": {"no-slip": cfg["walls"]}})
        dom.setUp()
        mesh = dom.getMesh()
        mat = pa.MatNS()
        mat.setDomain(dom)
        mat.build(buildOperators=False, nsType="sumfac")
        ops = dict(zip(OPS, (mat.K, mat.Krhs, mat.Rw, mat.Kfs, mat.Krhsfs, mat.Rwfs, mat.getKplusKfs())))
        n = mesh.N * dim
        cls = np.zeros(n, np.int64)
        cls[np.asarray(sorted(dom.getTangDofs(collect=True)), np.int64)] = T
        cls[np.asarray(sorted(dom.getNormalDofs(collect=True)), np.int64)] = N
        lo, hi = mesh.node_range
        # (a rank's domain names its own nodes' DoFs: every rank's owned slices, in this run's numbering)
        parts = [None] * size
        dist.all_gather_object(parts, cls[lo * dim:hi * dim])
        cls = np.concatenate(parts)
        assert len(cls) == n
        out = {"rank": rank, "transport": pa.get_ctx().device_info()["transport"], "node_range": (lo, hi),
               "coords": mesh.coords(), "cls": cls, "ops": {}}
        for nm, A in ops.items():
            xs, y0 = cfg["x"][nm], cfg["y0"]
            r = {"y": [], "z": [], "nan": [], "plain_equal": True, "repeat_equal": True, "format": A.getFormat(),
                 "size": A.getSize(), "rows": A.getOwnershipRange(), "kernel": A.spmvKernel(), "info": A.getInfo()}
            for x in xs:  # in turn: the second product finds the first's ghosts in place
                A.setHaloOverlap(True)
                y = _product(A, x)
                r["y"].append(y)
                r["z"].append(_product(A, x, y0))
                A.setHaloOverlap(False)
                r["plain_equal"] &= _product(A, x).tobytes() == y.tobytes()
                A.setHaloOverlap(True)
                r["repeat_equal"] &= all(_product(A, x).tobytes() == y.tobytes() for _ in range(3))
            if nm not in RW:
                for cols, _rows in SPECS[nm]["passes"]:
                    xn = np.where(SN.isin(cls, cols), xs[1], np.nan)  # (every rank's: the halo carries them)
                    r["nan"].append(_product(A, xn))
                r["diag"] = A.getDiagonal().getArray().copy()
            else:
                r["diag_refused"] = _refused(pa, A.getDiagonal)
            out["ops"][nm] = r
        if cfg.get("solve"):
            sol = pa.KleSolver()
            sol.setMat(mat)
            sol.setUp()
            assert sol.isNS() and sol.solverFS.getOperators()[0] is mat.getKplusKfs()
            sol.getKSP().setTolerances(rtol=1e-13)
            sol.solverFS.setTolerances(rtol=1e-13)
            vort = mat.Rw.createVecRight()
            wlo, whi = vort.getOwnershipRange()
            vort.setArray(cfg["x"]["Rw"][0][wlo:whi])
            vel = sol.getSolution()
            vlo, vhi = vel.getOwnershipRange()
            vel.setArray(np.where(cls != F, cfg["x"]["K"][0], 0.0)[vlo:vhi])  # wall values on the T and N DoFs
            ubc = vel.getArray().copy()
            sol.solveFS(vort)
            vfs = sol.getFreeSlipSolution().getArray().copy()
            sol.solve(vort)
            out["solve"] = {"u": vel.getArray().copy(), "vfs": vfs, "ubc": ubc,
                            "reason": (sol.solverFS.getConvergedReason(), sol.getKSP().getConvergedReason()),
                            "its": (sol.solverFS.getIterationNumber(), sol.getKSP().getIterationNumber())}
        if cfg.get("refusals"):
            other = pa.BoxMesh(3, [2, 2, 6], [0, 0, 0], [1, 1, 1], 3, rank=rank, nranks=size + 1)
            other.set_noslip_faces(list(SIX))
            out["refused"] = {nm: _refused(pa, lambda nm=nm: pa.petsc.Mat.createNSSumFactored(other, nm))
                              for nm in ("K", "Rw", "Kfs")}
            out["refused"]["csr"] = _refused(pa, mat.K.getValuesCSR)
            out["after"] = _product(mat.K, cfg["x"]["K"][0]).tobytes() == out["ops"]["K"]["y"][0].tobytes()
        q.put(out)
    except Exception:  # report instead of hanging the peers
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc()})
    finally:
        dist.destroy_process_group()


def _msh(name, tmp_path_factory):
    if "dir" not in _PARTS:
        _PARTS["dir"] = tmp_path_factory.mktemp("sumfac_ns_ranks")
    return SR.mesh_file(CONFIGS[name], _PARTS["dir"])


def _partition(name, tmp_path_factory):
    """The host partition of a configuration and its inputs in owner numbering (CPU)."""
    cfg = CONFIGS[name]
    key = cfg.get("host", name)
    if key not in _PARTS:
        P = SR.Partition(cfg, _msh(name, tmp_path_factory))
        for p in P.parts:
            # (an inertial part's inner list may be empty: nothing runs beside its halo)
            assert len(p.outer) and len(p.ghosts), (name, p.rank)
        rng = np.random.default_rng(20241022)
        P.x = {nm: [rng.uniform(-1, 1, P.N * _cw(P.dim, nm)) for _ in range(2)] for nm in OPS}
        P.y0 = rng.uniform(-1, 1, P.N * P.dim)
        _PARTS[key] = P
    return _PARTS[key]


def _run(name, tmp_path_factory, one=False):
    """The spawned run of a configuration, or of its mesh on one rank (inputs
    in that run's numbering)."""
    cfg = CONFIGS[name]
    P = _partition(name, tmp_path_factory)
    key = ("one", cfg.get("host", name)) if one else name
    if key not in _RUNS:
        c = dict(cfg)
        if one:
            c.update(size=1, transport="host", refusals=False)
            c["x"] = {nm: [P.to_one(x, _cw(P.dim, nm)) for x in xs] for nm, xs in P.x.items()}
            c["y0"] = P.to_one(P.y0, P.dim)
        else:
            c.update(x=P.x, y0=P.y0)
        assert c["size"] <= 3
        res = SRK.spawn(_worker, c, _msh(name, tmp_path_factory))
        assert one or all(r["transport"] == c.get("transport", "host") for r in res)
        if not one:  # the workers' partition is the host's
            assert [r["node_range"] for r in res] == P.ranges
            assert np.array_equal(np.concatenate([r["coords"] for r in res]), P.coords)
        _RUNS[key] = res
    return _RUNS[key]


def _cat(res, nm, key, k=None):
    return np.concatenate([r["ops"][nm][key] if k is None else r["ops"][nm][key][k] for r in res])


# ---------------------------------------------------------------- a. products
@pytest.mark.parametrize("name", list(CONFIGS))
def test_products_on_ranks_equal_one_rank(name, tmp_path_factory):
    P = _partition(name, tmp_path_factory)
    print(f"SUMFAC-NS-RANKS {name}: inner {[len(p.inner) for p in P.parts]}  outer {[len(p.outer) for p in P.parts]}  "
          f"ghost nodes {[len(p.ghosts) for p in P.parts]}")
    res = _run(name, tmp_path_factory)
    one = _run(name, tmp_path_factory, one=True)[0]
    dim = P.dim
    # the classes of the ranks' numbering are the one-rank run's, and every rank's ghosts hold wall DoFs
    cls = res[0]["cls"]
    assert all(np.array_equal(r["cls"], cls) for r in res)
    assert np.array_equal(P.to_one(cls, dim), one["cls"])
    for p in P.parts:
        gc = cls.reshape(-1, dim)[p.ext[p.ghosts]]
        assert (gc != F).any() and (gc == F).any(), (name, p.rank)
    for nm in OPS:
        C_ = _cw(dim, nm)
        for r, (lo, hi) in zip(res, P.ranges):
            o = r["ops"][nm]
            assert o["format"] == "elem" and o["kernel"] == one["ops"][nm]["kernel"], (nm, o["kernel"])
            assert "k_sumfac_gather_cls" in o["kernel"]
            assert o["size"] == (P.N * dim, P.N * C_) and o["rows"] == (lo * dim, hi * dim), (nm, r["rank"])
            assert o["info"]["format"] == "elem" and o["info"]["nz_used"] == 0 and o["info"]["spmv_bytes"] > 0
            assert o["plain_equal"], (name, nm, r["rank"], "halo overlap on / off differ")
            assert o["repeat_equal"], (name, nm, r["rank"], "repeated products differ")
        for k in range(2):
            y = _cat(res, nm, "y", k)
            yo = P.to_one(y, dim)
            y1 = one["ops"][nm]["y"][k]
            diff = np.nonzero(yo != y1)[0]
            assert yo.tobytes() == y1.tobytes(), (name, nm, k, len(diff), diff[:8].tolist())
            assert np.any(yo != 0.0)
            z = _cat(res, nm, "z", k)
            assert z.tobytes() == (P.y0 + y).tobytes(), (name, nm, k, "multAdd")
            assert P.to_one(z, dim).tobytes() == one["ops"][nm]["z"][k].tobytes()


def test_ipc_transport_same_bits(tmp_path_factory):
    name = "inertial3_ipc"
    res, host = _run(name, tmp_path_factory), _run(CONFIGS[name]["host"], tmp_path_factory)
    assert [r["transport"] for r in res] == ["ipc"] * 3 and [r["transport"] for r in host] == ["host"] * 3
    for nm in OPS:
        for k in range(2):
            assert _cat(res, nm, "y", k).tobytes() == _cat(host, nm, "y", k).tobytes(), (nm, k)


# -------------------------------------------------- b. selection, c. diagonal
@pytest.mark.parametrize("name", list(CONFIGS))
def test_selection_and_diagonal_on_ranks(name, tmp_path_factory):
    P = _partition(name, tmp_path_factory)
    res = _run(name, tmp_path_factory)
    one = _run(name, tmp_path_factory, one=True)[0]
    dim = P.dim
    cls = res[0]["cls"]
    for nm in OPS:
        if nm in RW:
            assert all(r["ops"][nm]["diag_refused"] == 56 for r in res), nm
            continue
        S = SPECS[nm]
        y = _cat(res, nm, "y", 1)
        x = P.x[nm][1]
        ident, zero = SN.isin(cls, S["ident"]), SN.isin(cls, S["zero"])
        for p, (cols, rows) in enumerate(S["passes"]):
            yn = np.concatenate([r["ops"][nm]["nan"][p] for r in res])
            take = SN.isin(cls, rows)
            assert take.any() and not np.isnan(yn[take]).any(), (name, nm, p)
            assert yn[take].tobytes() == y[take].tobytes(), (name, nm, p)
            xn = np.where(SN.isin(cls, cols), x, np.nan)
            assert yn[ident].tobytes() == xn[ident].tobytes(), (name, nm, p)  # x_i as given, NaN included
            assert yn[zero].tobytes() == np.zeros(int(zero.sum())).tobytes()  # +0.0 in bytes
            assert P.to_one(yn, dim).tobytes() == one["ops"][nm]["nan"][p].tobytes(), (name, nm, p)
        dg = P.to_one(_cat(res, nm, "diag"), dim)
        assert dg.tobytes() == one["ops"][nm]["diag"].tobytes(), (name, nm, "diagonal")
        d = _cat(res, nm, "diag")
        assert np.all(d[ident] == 1.0) and np.all(d[zero] == 0.0)
        if nm in ("K", "K+Kfs"):
            assert np.all(d[~ident] > 0.0)


# ------------------------------------------------------------------ d. solves
@pytest.mark.parametrize("name", [n for n, c in CONFIGS.items() if c.get("solve")])
def test_solvefs_and_solve_on_ranks_match_one_rank(name, tmp_path_factory):
    P = _partition(name, tmp_path_factory)
    res = _run(name, tmp_path_factory)
    sv = [r["solve"] for r in res]
    o = _run(name, tmp_path_factory, one=True)[0]["solve"]
    dim = P.dim
    cls = res[0]["cls"]
    for s in sv + [o]:
        assert min(s["reason"]) > 0, s["reason"]
    u, vfs, ubc = (np.concatenate([s[k] for s in sv]) for k in ("u", "vfs", "ubc"))
    assert P.to_one(ubc, dim).tobytes() == o["ubc"].tobytes()
    rel_fs = np.linalg.norm(P.to_one(vfs, dim) - o["vfs"]) / np.linalg.norm(o["vfs"])
    rel_u = np.linalg.norm(P.to_one(u, dim) - o["u"]) / np.linalg.norm(o["u"])
    print(f"SUMFAC-NS-RANKS {name}: |velFS - one rank| / |.| {rel_fs:.3e}  |u - one rank| / |.| {rel_u:.3e}  "
          f"iterations (solveFS, solve) {[s['its'] for s in sv]} (one rank {o['its']})")
    assert np.linalg.norm(o["vfs"]) > 0 and np.linalg.norm(o["u"]) > 0
    assert rel_fs <= 1e-9 and rel_u <= 1e-9
    # the identity rows are copied back exactly on every rank
    assert vfs[cls == N].tobytes() == ubc[cls == N].tobytes()
    assert u[cls != F].tobytes() == ubc[cls != F].tobytes()


# --------------------------------------------------------------- e. refusals
def test_refusals_on_ranks(tmp_path_factory):
    for r in _run("slab2", tmp_path_factory):
        assert r["refused"] == {k: 56 for k in r["refused"]} and len(r["refused"]) == 4, (r["rank"], r["refused"])
        assert r["after"]
