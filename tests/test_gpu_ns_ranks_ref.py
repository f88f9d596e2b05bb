"""The assembled no-slip system on several ranks (all on one GPU), against the
longdouble restatement of tests/ns_ref.py on the global mesh --
tests/test_gpu_ns_ref.py on ranks, where kle_mesh_set_noslip_faces classes the
ghost DoFs, the gathers read dcls past the owned range and the CSR export
masks ghost columns.

One spawned run per configuration (CONFIGS) and one of the same mesh on one
rank, cached and shared by the assertions; the parent never opens the GPU:
the meshes, the partitions (pa.BoxMesh / UnstructuredMesh with rank=, on the
host), the reference and the conditions on the inputs (_conditions) are all
formed on the CPU before any comparison.  Gmsh partitions number their nodes
by owner: the reference is built in that numbering (oracle.node_map by
coordinates).

Configurations: 2 and 3 ranks on the cavity [3,4] ngl 4 (host and IPC; layers
2/1/1 on 3), 2 ranks [3,4] ngl 3 with left, up, down, 2 and 3 ranks on the
six-wall boxes [2,2,4] / [2,2,3] ngl 3, perturbed_box(3, [3,3,4], seed 5) ngl 3
on 2 slab and 3 inertial ranks, the cavity [4,4] ngl 3 of the fixture, and the
cavity [3,2] ngl 4 on 2 ranks, where rank 0 has one element layer and its wall
corners -- the nodes the corner rule acts on -- are ghosts of rank 1.

a. Classes: the ranks' getTangDofs / getNormalDofs(collect=True) are disjoint
   and their union is the reference's sets.
b. Exports: ranks_ref.global_csr of the ranks' getValuesCSR() parts of each of
   the nine matrices has the reference's pattern bit for bit and every entry
   inside its bound (ns_ref.check_exports; NSREF lines).  Whether the stitched
   export is the one-rank export bit for bit is printed for every
   configuration and asserted (BITS_EQUAL) where the summation order explains
   it: box slabs, where k_gather_ns walks a row's cells in ascending lattice
   order on any partition, and the Gmsh partitions, whose local cells ascend
   by global cell id (k_gather_u), so every entry is the same sum of the same
   element blocks in the same order.
c. Products: mult and multAdd of K, Krhs, Rw, Kfs, Krhsfs, Rwfs, K+Kfs row by
   row against the longdouble product of the global export within
   mat_ref.product's bound, inputs of ranks_ref.op_inputs; halo overlap on and
   off the same bits.
d. Solves: KleSolver.solveFS + solve (CG + Jacobi, rtol 1e-12 on both) on the
   box configurations against the same code on one rank: <= 1e-10 relative,
   the figure and the reason of tests/test_gpu_ns_elem_ranks.py (the runs
   differ by the allreduce rounding of the dot products -- and here by nothing
   else, the matrices being the same bits -- amplified by the solve).  On
   cavity [4,4] ngl 3, 2 ranks, solveFS + solve and one BaseProblem.evalRHS
   against case_cavity2d.npz at the tolerances of tests/test_gpu_ns.py: 1e-9
   on the solves (rtol 1e-13), 1e-6 of scale on f.
"""
import os

import numpy as np
import pytest

import mat_ref as M
import ns_ref as NS
import ranks_ref as RR
import test_gpu_sym_ranks_ref as SR
from oracle import oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = -7.25
PRODUCTS = ("K", "Krhs", "Rw", "Kfs", "Krhsfs", "Rwfs", "KplusKfs")
CAVITY = {"up": [2, 0], "down": [0, 0], "left": [0, 0], "right": [0, 0]}
THREE = {"left": [0, 1], "up": [2, 0], "down": [0, 0]}
SIX = {"up": [1, 0, 0.5], "down": [0, 0, 0], "left": [0, 0, 0], "right": [0, 0, 0], "front": [0, 0, 0],
       "back": [0, 0, 0]}
GMSH = [3, 3, 4]  # perturbed_box(3, GMSH, seed=5)
SOLVE_RTOL = 1e-12
CONFIGS = {
    "r2_cavity": dict(size=2, nelem=[3, 4], ngl=4, walls=CAVITY, solve=True),
    "r2_cavity_ipc": dict(size=2, nelem=[3, 4], ngl=4, walls=CAVITY, solve=True, transport="ipc", host="r2_cavity"),
    "r3_cavity": dict(size=3, nelem=[3, 4], ngl=4, walls=CAVITY, solve=True),
    "r2_three_walls": dict(size=2, nelem=[3, 4], ngl=3, walls=THREE),
    "r2_six": dict(size=2, nelem=[2, 2, 4], ngl=3, walls=SIX, solve=True),
    "r3_six": dict(size=3, nelem=[2, 2, 3], ngl=3, walls=SIX, solve=True),
    "gmsh2_slab": dict(size=2, gmsh="slab", ngl=3, walls=SIX),
    "gmsh3_inertial": dict(size=3, gmsh="inertial", ngl=3, walls=SIX),
    "r2_cavity44": dict(size=2, nelem=[4, 4], ngl=3, walls=CAVITY, fixture=True),
    # one element layer on rank 0: its wall corners, where the corner rule acts, are ghosts of rank 1
    "r2_ghost_corner": dict(size=2, nelem=[3, 2], ngl=4, walls=CAVITY, ghost_corner=True),
}
# configurations whose stitched export is asserted to be the one-rank export bit for bit (docstring, b)
BITS_EQUAL = ("r2_cavity", "r2_cavity_ipc", "r3_cavity", "r2_three_walls", "r2_six", "r3_six", "gmsh2_slab",
              "gmsh3_inertial", "r2_cavity44", "r2_ghost_corner")
_RUNS, _REFS = {}, {}


def _mats(mat):
    ms = dict(zip(NS.NAMES[:-1], mat.kle))
    ms["KplusKfs"] = mat.getKplusKfs()
    return ms


def _solves(pa, dom, mat, rtol, vort0=None, vel0=None):
    sol = pa.KleSolver()
    sol.setMat(mat)
    sol.setUp()
    assert sol.isNS()
    sol.getKSP().setTolerances(rtol=rtol)
    sol.solverFS.setTolerances(rtol=rtol)
    vort = mat.Rw.createVecRight()
    wlo, whi = vort.getOwnershipRange()
    vel = sol.getSolution()
    vlo, vhi = vel.getOwnershipRange()
    if vort0 is None:
        vort.setArray(np.cos(0.37 * np.arange(wlo, whi, dtype=np.float64)))
        dom.applyBoundaryConditions(vel, "velocity", 0.0, 0.02)
    else:
        vort.setArray(vort0[wlo:whi])
        vel.setArray(vel0[vlo:vhi])
    ubc = vel.getArray().copy()
    sol.solveFS(vort)
    vfs = sol.getFreeSlipSolution().getArray().copy()
    sol.solve(vort)
    return {"u": vel.getArray().copy(), "vfs": vfs, "ubc": ubc,
            "reason": (sol.solverFS.getConvergedReason(), sol.getKSP().getConvergedReason()),
            "its": (sol.solverFS.getIterationNumber(), sol.getKSP().getIterationNumber())}


def _eval_rhs(pa, cfg, g):
    """test_eval_rhs_noslip_matches_reference (tests/test_gpu_ns.py) on this rank's slices."""
    dim = len(cfg["nelem"])
    pcfg = {"name": "cavity", "material-properties": {"rho": float(g["rho"]), "mu": float(g["mu"])},
            "domain": {"ngl": cfg["ngl"], "box-mesh": {"nelem": cfg["nelem"], "lower": [0] * dim, "upper": [1] * dim}},
            "boundary-conditions": {"no-slip": cfg["walls"]}, "initial-conditions": {"velocity": [0, 0]}}
    prob = pa.BaseProblem(pcfg)
    prob.setUp()
    prob.setUpSolver()
    sol = prob.solverKLE
    assert sol.isNS() and prob.mat.K.getFormat() != "elem"
    sol.getKSP().setTolerances(rtol=1e-13)
    sol.solverFS.setTolerances(rtol=1e-13)
    vel = sol.getSolution()
    vlo, vhi = vel.getOwnershipRange()
    vel.setArray(g["vel0"][vlo:vhi])
    wlo, whi = prob.vort.getOwnershipRange()
    prob.vort.setArray(g["rhs_vort_in"][wlo:whi])
    f = prob.operator.Curl.createVecLeft()
    prob.evalRHS(None, float(g["rhs_t"]), prob.vort, f)
    return {"velFS": sol.getFreeSlipSolution().getArray().copy(), "vort_bc": prob.vort.getArray().copy(),
            "vel": sol.getSolution().getArray().copy(), "f": f.getArray().copy(), "vrange": (vlo, vhi),
            "wrange": (wlo, whi), "frange": tuple(f.getOwnershipRange())}


def _worker(rank, size, port, cfg, msh, q):
    dist = SR.rank_setup(rank, size, port, cfg)
    try:
        import pynama_amd as pa
        dom, mat = SR.build_system(pa, cfg, msh, False, walls=cfg["walls"])
        mesh = dom.getMesh()
        out = {"rank": rank, "transport": pa.get_ctx().device_info()["transport"],
               "node_range": tuple(mesh.node_range), "ext_range": tuple(mesh.ext_range),
               "tang": sorted(int(i) for i in dom.getTangDofs(collect=True)),
               "normal": sorted(int(i) for i in dom.getNormalDofs(collect=True)), "mats": {}}
        for name, A in _mats(mat).items():
            lo, hi = A.getOwnershipRange()
            m, n = A.getSize()
            r = {"part": (lo, hi) + tuple(A.getValuesCSR()), "size": (m, n), "format": A.getFormat()}
            if name in PRODUCTS:
                x, y, z, v = A.createVecRight(), A.createVecLeft(), A.createVecLeft(), A.createVecLeft()
                clo, chi = x.getOwnershipRange()
                cols = [None] * size
                dist.all_gather_object(cols, (clo, chi))
                xs = RR.op_inputs(n, cols, seed=len(name))
                ya = M.x_uniform(m, 77)[lo:hi]
                r.update(cols=(clo, chi), kernel=A.spmvKernel(), y={}, z={}, plain_differs=[])
                for nm, xa in xs.items():
                    x.setArray(xa[clo:chi])
                    for overlap in (True, False):
                        A.setHaloOverlap(overlap)
                        y.set(SENTINEL)  # (a row the kernel does not write stays visible)
                        A.mult(x, y)
                        v.setArray(ya)
                        z.set(SENTINEL)
                        A.multAdd(x, v, z)
                        if overlap:
                            r["y"][nm], r["z"][nm] = y.getArray().copy(), z.getArray().copy()
                        elif not (np.array_equal(y.getArray(), r["y"][nm]) and np.array_equal(z.getArray(), r["z"][nm])):
                            r["plain_differs"].append(nm)
                    A.setHaloOverlap(True)
            out["mats"][name] = r
        if cfg.get("solve"):
            out["solve"] = _solves(pa, dom, mat, SOLVE_RTOL)
        if cfg.get("fixture"):
            g = np.load(os.path.join(G, "case_cavity2d.npz"))
            out["solve_fixture"] = _solves(pa, dom, mat, 1e-13, g["vort0"], g["vel0"])
            out["eval"] = _eval_rhs(pa, cfg, g)
        q.put(out)
    except Exception:  # report instead of hanging the peers
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc()})
    finally:
        dist.destroy_process_group()


def _msh(cfg, tmp_path_factory):
    return SR.gmsh_file(tmp_path_factory, GMSH) if cfg.get("gmsh") else None


def _run(name, tmp_path_factory, one=False):
    """The spawned run of a configuration, or of its mesh on one rank (shared
    by the configurations of the same mesh and walls)."""
    cfg = CONFIGS[name]
    assert cfg["size"] <= 4
    if one:
        cfg = dict(cfg, size=1, transport="host")
        cfg.pop("host", None)
        key = ("one", str(cfg.get("nelem")), cfg["ngl"], str(list(cfg["walls"])), bool(cfg.get("gmsh")),
               bool(cfg.get("fixture")))
        cfg["gmsh"] = "slab" if cfg.get("gmsh") else None
    else:
        key = name
    if key not in _RUNS:
        res = SR.spawn(_worker, cfg, _msh(cfg, tmp_path_factory))
        assert one or all(r["transport"] == cfg.get("transport", "host") for r in res)
        _RUNS[key] = res
    return _RUNS[key]


def _host_meshes(cfg, msh):
    """The one-rank mesh and each rank's part, on the host."""
    import pynama_amd as pa
    from pynama_amd.mesh import UnstructuredMesh
    size = cfg["size"]
    if cfg.get("gmsh"):
        one = UnstructuredMesh.from_gmsh(msh, cfg["ngl"])
        parts = [UnstructuredMesh.from_gmsh(msh, cfg["ngl"], rank=r, nranks=size, partitioner=cfg["gmsh"])
                 for r in range(size)]
    else:
        dim = len(cfg["nelem"])
        one = pa.BoxMesh(dim, cfg["nelem"], [0] * dim, [1] * dim, cfg["ngl"])
        parts = [pa.BoxMesh(dim, cfg["nelem"], [0] * dim, [1] * dim, cfg["ngl"], rank=r, nranks=size)
                 for r in range(size)]
    return one, parts


def _reference(name, tmp_path_factory):
    """cls and the nine references in the ranks' global numbering, the node
    ranges and the ghost nodes of every rank, the map from one-rank nodes."""
    cfg = CONFIGS[name]
    key = (str(cfg.get("nelem")), cfg["ngl"], str(list(cfg["walls"])), cfg.get("gmsh"), cfg["size"])
    if key not in _REFS:
        one, parts = _host_meshes(cfg, _msh(cfg, tmp_path_factory))
        dim = one.dim
        coords = np.concatenate([p.coords() for p in parts])
        ranges = [tuple(p.node_range) for p in parts]
        assert ranges[0][0] == 0 and ranges[-1][1] == one.N == len(coords)
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        mp = O.node_map(one.coords(), coords)  # one-rank node -> the ranks' global node
        if not cfg.get("gmsh"):
            assert np.array_equal(mp, np.arange(one.N))
        cls, ref = NS.reference(dim, cfg["ngl"], mp[one.conn()], one.corners(), coords, list(cfg["walls"]))
        ghosts = []
        for p, (lo, hi) in zip(parts, ranges):
            g = np.asarray(p.ext_gids())
            ghosts.append(np.sort(g[(g < lo) | (g >= hi)]))
        _REFS[key] = dict(dim=dim, cls=cls, ref=ref, ranges=ranges, ghosts=ghosts, coords=coords, mp=mp)
        _conditions(name, _REFS[key])
    return _REFS[key]


def _conditions(name, c):
    """What the inputs must offer, from the mesh alone (CPU)."""
    cfg = CONFIGS[name]
    dim, cls, ref, ranges, coords = c["dim"], c["cls"], c["ref"], c["ranges"], c["coords"]
    size = cfg["size"]
    node_cls = cls.reshape(-1, dim)
    for k, (lo, hi) in enumerate(ranges):
        # every rank owns a row of each class
        for what in (NS.F, NS.T, NS.N):
            assert (node_cls[lo:hi] == what).any(), (name, k, what)
        # and stores, in some checked matrix, a non-zero in a ghost column whose DoF is T or N
        hit = []
        for nm in ("Krhs", "Kfs", "Krhsfs", "KplusKfs"):
            A = ref[nm]
            rn, cn = A.rows // dim, A.indices // dim
            sel = (rn >= lo) & (rn < hi) & ((cn < lo) | (cn >= hi)) & (cls[A.indices] != NS.F) & (A.value != 0)
            assert np.isin(cn[sel], c["ghosts"][k]).all(), (name, k, nm)  # (a stored foreign column is a ghost)
            if sel.any():
                hit.append(nm)
        assert hit, (name, k)
        print(f"NSREF-RANKS {name} rank {k}: nodes {hi - lo}, ghosts {len(c['ghosts'][k])}, "
              f"wall ghost columns stored in {hit}")
    on = {w: np.zeros(len(coords), bool) for w in NS.FACE}
    for w in NS.FACE:
        if NS.FACE[w][0] < dim:
            on[w][NS.wall_nodes(coords, w)] = True
    owner = RR.owner_of(ranges, np.arange(len(coords)))
    if dim == 2:  # a corner-rule node on a rank other than 0
        walls = list(cfg["walls"])
        corner = np.zeros(len(coords), bool)
        for s in ("left", "right"):
            for t in ("up", "down"):
                if s in walls and t in walls:
                    corner |= on[s] & on[t]
        assert (owner[corner] > 0).any(), name
        if cfg.get("ghost_corner"):  # some rank reads a corner-rule DoF's class past its owned range
            A = ref["Krhsfs"]
            seen = [bool((np.isin(A.indices // dim, np.intersect1d(c["ghosts"][k], np.nonzero(corner)[0]))
                          & (A.rows // dim >= lo) & (A.rows // dim < hi) & (A.value != 0)).any())
                    for k, (lo, hi) in enumerate(ranges)]
            assert any(seen), (name, seen)
    if size == 3 and not cfg.get("gmsh"):  # the middle rank has no wall of the partition axis
        lo, hi = ranges[1]
        axis_walls = ("down", "up") if dim == 2 else ("back", "front")
        assert not any(on[w][lo:hi].any() for w in axis_walls), name


def _stitched(res, nm, ncols):
    return RR.global_csr([r["mats"][nm]["part"] for r in res], ncols=ncols)


# ----------------------------------------------------------------- a. classes
@pytest.mark.parametrize("name", list(CONFIGS))
def test_rank_classes(name, tmp_path_factory):
    c = _reference(name, tmp_path_factory)
    res = _run(name, tmp_path_factory)
    assert [r["node_range"] for r in res] == c["ranges"]
    t, n = NS.class_sets(c["cls"])
    normals, tangs = [set(r["normal"]) for r in res], [set(r["tang"]) for r in res]
    for sets in (normals, tangs):
        assert sum(len(s) for s in sets) == len(set().union(*sets)), name  # disjoint
    dim = c["dim"]
    for r, tn, nn in zip(res, tangs, normals):  # each rank reports its own nodes
        lo, hi = r["node_range"]
        assert all(lo * dim <= i < hi * dim for i in tn | nn), r["rank"]
    normal = set().union(*normals)
    assert normal == n
    assert set().union(*tangs) - normal == t


# ----------------------------------------------------------------- b. exports
@pytest.mark.parametrize("name", list(CONFIGS))
def test_rank_exports_match_longdouble(name, tmp_path_factory):
    c = _reference(name, tmp_path_factory)
    res = _run(name, tmp_path_factory)
    one = _run(name, tmp_path_factory, one=True)[0]
    dim, ref, mp = c["dim"], c["ref"], c["mp"]
    exports, equal = {}, {}
    for nm in NS.NAMES:
        E, ranges = _stitched(res, nm, ref[nm].n)
        assert ranges == [(lo * dim, hi * dim) for lo, hi in c["ranges"]] and E.m == ref[nm].m  # no row left out
        exports[nm] = (E.indptr, E.indices, E.data)
        rb, cb = NS.block_shape(nm, dim)
        o = NS.relabel_csr(one["mats"][nm]["part"][2:], mp, rb, cb)
        equal[nm] = all(np.array_equal(a, b) for a, b in zip(o, exports[nm]))
    bad, worst = NS.check_exports(name, exports, ref)
    print(f"NSREF-RANKS {name} stitched export == one-rank export bit for bit: "
          + ", ".join(f"{k} {'yes' if v else 'NO'}" for k, v in equal.items()))
    assert not bad, (name, bad)
    if name in BITS_EQUAL:
        assert all(equal.values()), (name, equal)


# ---------------------------------------------------------------- c. products
@pytest.mark.parametrize("name", list(CONFIGS))
def test_rank_products_multiply_by_what_they_export(name, tmp_path_factory):
    res = _run(name, tmp_path_factory)
    for mname in PRODUCTS:
        rs = [r["mats"][mname] for r in res]
        m, n = rs[0]["size"]
        E, ranges = RR.global_csr([r["part"] for r in rs], ncols=n)
        cols = [r["cols"] for r in rs]
        assert cols[0][0] == 0 and cols[-1][1] == n and all(a[1] == b[0] for a, b in zip(cols, cols[1:])), cols
        xs = RR.op_inputs(n, cols, seed=len(mname))
        ya = M.x_uniform(m, 77)
        rows = M.rows_of(E)
        worst, worst_a = (0.0, None), (0.0, None)
        for nm, xa in xs.items():
            ref, b = M.product(E, xa)
            zr, zb = M.mult_add(ref, b, ya)
            for k, (r, (lo, hi), (clo, chi)) in enumerate(zip(rs, ranges, cols)):
                assert not r["plain_differs"], (name, mname, k, "overlapped != plain", r["plain_differs"])
                w, at = M.worst(r["y"][nm], ref[lo:hi], b[lo:hi])
                assert w <= 1, (name, mname, nm, "mult", k, w, at)
                if w >= worst[0]:
                    worst = (w, (k, at[0] if at else None, nm))
                w, at = M.worst(r["z"][nm], zr[lo:hi], zb[lo:hi])
                assert w <= 1, (name, mname, nm, "multAdd", k, w, at)
                if w >= worst_a[0]:
                    worst_a = (w, (k, at[0] if at else None, nm))
                mine = (rows >= lo) & (rows < hi)
                ghost = mine & ((E.indices < clo) | (E.indices >= chi)) & (E.data != 0)
                if nm.startswith("only_r") and int(nm[6:]) != k and ghost.any() and np.any(ref[lo:hi] != 0):
                    assert np.any(r["y"][nm] != 0), (name, mname, nm, k)  # seen through the halo alone
        print(f"NSREF-RANKS {name} {mname} format={rs[0]['format']} kernel={rs[0]['kernel']} "
              f"mult: worst err/bound {worst[0]:.3g} at {worst[1]}; multAdd: {worst_a[0]:.3g} at {worst_a[1]}")


@pytest.mark.parametrize("name", [n for n, cfg in CONFIGS.items() if cfg.get("host")])
def test_ipc_transport_equals_host_bitwise(name, tmp_path_factory):
    a, b = _run(name, tmp_path_factory), _run(CONFIGS[name]["host"], tmp_path_factory)
    for ra, rb in zip(a, b):
        assert ra["transport"] == "ipc" and rb["transport"] == "host"
        for nm in NS.NAMES:
            assert all(np.array_equal(u, v) for u, v in zip(ra["mats"][nm]["part"], rb["mats"][nm]["part"])), nm
        for nm in PRODUCTS:
            for which in ("y", "z"):
                for inp, y in ra["mats"][nm][which].items():
                    assert np.array_equal(y, rb["mats"][nm][which][inp]), (ra["rank"], nm, which, inp)


# ------------------------------------------------------------------ d. solves
@pytest.mark.parametrize("name", [n for n, cfg in CONFIGS.items() if cfg.get("solve")])
def test_rank_solves_match_one_rank(name, tmp_path_factory):
    c = _reference(name, tmp_path_factory)
    res = _run(name, tmp_path_factory)
    o = _run(name, tmp_path_factory, one=True)[0]["solve"]
    sv = [r["solve"] for r in res]
    u, vfs, ubc = (np.concatenate([s[k] for s in sv]) for k in ("u", "vfs", "ubc"))
    for s in sv + [o]:
        assert s["reason"][0] > 0 and s["reason"][1] > 0, s["reason"]
    rel_fs = np.linalg.norm(vfs - o["vfs"]) / np.linalg.norm(o["vfs"])
    rel_u = np.linalg.norm(u - o["u"]) / np.linalg.norm(o["u"])
    print(f"NSREF-RANKS {name} solves: |velFS - one rank| / |.| {rel_fs:.3e}  |u - one rank| / |.| {rel_u:.3e}  "
          f"iterations {sv[0]['its']} (one rank {o['its']})")
    assert rel_fs <= 1e-10 and rel_u <= 1e-10
    wall = c["cls"] != NS.F
    assert ubc.tobytes() == o["ubc"].tobytes() and np.any(ubc[wall] != 0.0)


def test_two_rank_cavity_matches_fixture(tmp_path_factory):
    name = "r2_cavity44"
    g = np.load(os.path.join(G, "case_cavity2d.npz"))
    res = _run(name, tmp_path_factory)
    sv = [r["solve_fixture"] for r in res]
    vfs, u = (np.concatenate([s[k] for s in sv]) for k in ("vfs", "u"))
    # (vort0 is 0 and vel0 has no normal part: the fixture's velFS is exactly 0, and so must ours be)
    dfs, nfs = np.linalg.norm(vfs - g["velFS"]), np.linalg.norm(g["velFS"])
    rel_u = np.linalg.norm(u - g["u"]) / np.linalg.norm(g["u"])
    print(f"NSREF-RANKS {name} vs case_cavity2d: |velFS - ref| {dfs:.3e} (|ref| {nfs:.3e})  u {rel_u:.3e} relative  "
          f"iterations {sv[0]['its']}")
    assert dfs <= 1e-9 * nfs and rel_u <= 1e-9


def test_two_rank_eval_rhs_matches_fixture(tmp_path_factory):
    name = "r2_cavity44"
    g = np.load(os.path.join(G, "case_cavity2d.npz"))
    ev = [r["eval"] for r in _run(name, tmp_path_factory)]
    for key, n in (("vrange", len(g["rhs_vel"])), ("wrange", len(g["rhs_vort_bc"])), ("frange", len(g["rhs_f"]))):
        assert ev[0][key][0] == 0 and ev[0][key][1] == ev[1][key][0] and ev[1][key][1] == n
    vfs, vbc, vel, f = (np.concatenate([e[k] for e in ev]) for k in ("velFS", "vort_bc", "vel", "f"))
    rel_fs = np.linalg.norm(vfs - g["rhs_velFS"]) / np.linalg.norm(g["rhs_velFS"])
    rel_u = np.linalg.norm(vel - g["rhs_vel"]) / np.linalg.norm(g["rhs_vel"])
    err_w = np.abs(vbc - g["rhs_vort_bc"]).max() / np.abs(g["rhs_vort_bc"]).max()
    scale = max(1.0, np.abs(g["rhs_f"]).max())
    err_f = np.abs(f - g["rhs_f"]).max() / scale
    print(f"NSREF-RANKS {name} evalRHS vs case_cavity2d: velFS {rel_fs:.3e}  vort_bc {err_w:.3e}  vel {rel_u:.3e}  "
          f"f {err_f:.3e} of scale")
    assert rel_fs <= 1e-9 and err_w <= 1e-9 and rel_u <= 1e-9
    assert err_f <= 1e-6
