"""K x and the CG on it over several ranks (all on one GPU, as
tests/test_gpu_multirank.py runs them), row by row against longdouble
references on the global matrix -- tests/test_gpu_sym_ref.py on ranks.

One spawned run per configuration (CONFIGS), shared by its tests.  The
workers exchange their getValuesCSR() parts over gloo, so every rank forms the
same global inputs (ranks_ref.rank_inputs) and sets its owned slice; symmetric
storage is collective, so every rank sets the same tunings and calls
setOption(SPD, ...) in the same order, and asserts its spmvKernel() prefix.
The parent never opens the GPU: it joins the parts (ranks_ref.global_csr),
asserts the matrix symmetric bit for bit, computes the references once and
checks every rank's rows.

a. Products.  For each owned row i, the one-rank inequality

       |y_i - ref_i| <= 16 max(restatement, u) den_i + allowance_i

   with den = |K||x| and the restatement on the global CSR; allowance_i = 0 in
   full storage, nT_i q/2 otherwise with sym_ref.apriori_quantum of the global
   matrix: the global ||K||inf and ||x||inf bound every rank's local ones (a
   rank's bricks, tiles and groups take their scales from its own rows and its
   own part of x, ghosts included), and nT_i counts the blocks transposed into
   node i on whichever rank stores them.

   A row that receives a reverse-halo sum.  On a slab (kle_brick.hip
   brick_spmv / brick_gather_rest, kle_sym.hip sym_spmv) the sender's gather
   forms the ghost row's sum s_i like any row's -- the int64 sum of the
   rint(t / q) of the blocks it transposes into the row, times q, one rounding
   to fp64 -- into d_sgsend; halo_reverse copies the doubles; the owner forms
   its own y_i (direct sum and own transposed sum) and then adds, in
   k_brick_add_recv / k_axpy_first / the gather's last term, y_i += s_i: one
   fp64 add.  On a graph partition (gsym_spmv) k_gsym_unpack does the same add
   once per lower peer, in ascending sender order.  Against the one-rank
   product the row therefore has (1) the same fixed-point terms, each off by
   at most q/2 with q <= the a-priori quantum whichever rank formed them:
   nT_i q/2 in all, the allowance; (2) one more conversion rounding per
   sender, <= u |s_i| <= u (sum of the sender's |t|) <= u den_i^(sender),
   where the den_i^(sender) of the senders and the owner's own den_i^(own)
   add up to den_i; (3) one more fp64 add per sender, <= u |partial sum|
   <= u den_i (+ u x the allowance, second order).  With p <= 3 senders in
   these partitions that is at most 2 p u den_i <= 6 u den_i more than the
   one-rank product, whose own direct sum and single conversion stay as they
   were; the first term, 16 max(restatement, u) den_i >= 16 u den_i, holds
   both (the one-rank runs use well under half of it: DESIGN.md).  The factor
   16 is not enlarged and no storage needs a further term.

   Inputs: every input of the one-rank test over the global lattice, and the
   rank families of ranks_ref: only_r{k}, iface_spike_{k}_first / _last.
   Also: Dirichlet rows return x_i bit for bit; rows without a nonzero
   product are exactly 0; near overflow never a finite wrong value; the
   overlapped schedule equals the plain one bitwise for every input; the IPC
   transport equals the host transport bitwise.  That the check bites is
   asserted too: each rank's y of the uniform input with one row moved by
   1e-12 den_i does not pass.

   Each rank, storage and input family prints a SYMREF-RANKS line with the
   restatement's error, the device's, and the shares of the tolerance and of
   the allowance used.

b. CG through the rank products: x_k (each rank's owned slice) and ||r_k||
   for k = 1 .. 12, corrections off, against krylov_ref.pcg_reference on the
   global CSR with the tolerances of part b of tests/test_gpu_sym_ref.py;
   the last solve twice, bitwise; the pipelined CG with the gather folded
   into its update (k_pipe_iter_g) and separate, each held to the reference
   and to each other.

The shapes are the smallest at which these paths differ, and each test asserts
the property it was chosen for (_require_shape): the neighbour layout, owned
node rows a multiple of 64 or below 64, a rank with two peers, the kernels.
"""
import json
import os

import numpy as np
import pytest

import krylov_ref as R
import ranks_ref as RR
import sym_ref as S
import test_gpu_sym_ref as T
from test_gpu_multirank import _collect, _free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
BRICK = "k_nb_spmv_sym_brick<"

# storage -> (tunings, symmetric, kernel prefix, kernel substring)
STORAGES = {
    "full": ({}, False, "k_nb_spmv<3,3,", None),
    "bricks": ({}, True, BRICK, None),
    "rounds4": ({"spmv_brick_rounds": 4}, True, BRICK, None),
    "singles0": ({"spmv_brick_singles": 0}, True, BRICK, None),
    "pair0": ({"spmv_brick_pair": 0}, True, BRICK, None),
    "wps1": ({"spmv_gather_wps": 1}, True, BRICK, "k_nb_gsym_gather<1>"),
    "wps2": ({"spmv_gather_wps": 2}, True, BRICK, "k_nb_gsym_gather<2>"),
    "wps4": ({"spmv_gather_wps": 4}, True, BRICK, "k_nb_gsym_gather<4>"),
    "tiles": ({"spmv_sym_brick": 0}, True, "k_nb_spmv_sym_xl<", None),
    "tiles128": ({"spmv_sym_brick": 0, "spmv_sym_tile64": 2}, True, "k_nb_spmv_sym_xl<", ",4,4>+k_nb_sym_gather<8,4,4>"),
    "sym_small": ({}, True, "k_nb_spmv_sym", None),  # (whatever the planner gives a part below 64 node rows)
    "full_xl": ({}, False, None, "k_nb_spmv_xl<8>"),
    "full_dict": ({}, False, None, "k_nb_spmv_dict"),
    "groups": ({"spmv_gsym_brick": 0}, True, "k_nb_spmv_gsym<", None),
    "gbricks": ({}, True, "k_nb_spmv_gsym_brick<", None),
}
WAVES8 = {"KLE_SPMV_WAVES": "8", "KLE_SPMV_DICT_MIN_ROWS": "0"}
BOX_CG = [(v, pc) for v in ("cg", "pipecg") for pc in ("none", "jacobi")]
GMSH = [4, 4, 4]  # perturbed_box(3, GMSH, seed=5), ngl 3
CONFIGS = {
    "box2": dict(size=2, nelem=[3, 2, 4], ngl=4, cg=BOX_CG,
                 storages=["full", "bricks", "rounds4", "singles0", "pair0", "wps1", "wps2", "wps4", "tiles",
                           "tiles128"]),
    "box2_ipc": dict(size=2, nelem=[3, 2, 4], ngl=4, transport="ipc", storages=["bricks", "full"], host="box2"),
    "box3": dict(size=3, nelem=[2, 3, 3], ngl=3, cg=BOX_CG, storages=["full", "bricks", "tiles"]),
    "box8": dict(size=8, nelem=[2, 2, 8], ngl=4, storages=["bricks", "full"]),
    "box8_ipc_sentinel": dict(size=8, nelem=[2, 2, 8], ngl=4, transport="ipc", tuning={"ipc_sentinel": 1},
                              storages=["bricks", "full"], host="box8"),
    "slice64": dict(size=2, nelem=[7, 7, 4], ngl=2, storages=["bricks", "full"]),
    "below64": dict(size=2, nelem=[3, 3, 4], ngl=2, storages=["sym_small", "full"]),
    "box2_waves8": dict(size=2, nelem=[3, 2, 4], ngl=5, env=WAVES8, storages=["full_xl"]),
    "box3_waves8": dict(size=3, nelem=[4, 3, 6], ngl=4, env=WAVES8, storages=["full_xl"]),
    "gmsh2_slab": dict(size=2, gmsh="slab", ngl=3, storages=["full", "groups", "gbricks"]),
    "gmsh4": dict(size=4, gmsh="inertial", ngl=3, storages=["full", "groups", "gbricks"],
                  cg=[("pipecg", "jacobi")], cg_tunings={"spmv_gsym_brick": 0}, cg_prefix="k_nb_spmv_gsym<"),
    "gmsh4_ipc": dict(size=4, gmsh="inertial", ngl=3, transport="ipc", storages=["groups"], host="gmsh4"),
    "gmsh2_waves8": dict(size=2, gmsh="slab", ngl=3, env=WAVES8, storages=["full_dict"]),
    "gmsh3_waves8": dict(size=3, gmsh="inertial", ngl=3, env=WAVES8, storages=["full_dict"]),
}
_RUNS, _CASES, _CG, WORST = {}, {}, {}, {}


def lattice(cfg):
    """(dims, P) of a box configuration's global lattice, (None, None) for Gmsh."""
    if cfg.get("gmsh"):
        return None, None
    return [n * (cfg["ngl"] - 1) + 1 for n in cfg["nelem"]], cfg["ngl"] - 1


def rank_setup(rank, size, port, cfg):
    """A worker's first steps: the environment of its rank, gloo, the package."""
    import sys
    for p in (os.path.join(ROOT, "tests"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), KLE_TRANSPORT=cfg.get("transport", "host"),
                      RANK=str(rank), WORLD_SIZE=str(size), KLE_COMM_TIMEOUT_S="60")
    os.environ.update(cfg.get("env", {}))
    if cfg.get("tuning"):
        os.environ["KLE_TUNING"] = json.dumps(cfg["tuning"])
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=size)
    return dist


def build_system(pa, cfg, msh, operators, walls=None):
    """Domain and MatFS of a configuration; with walls ({name: wall velocity},
    in configuration order) the no-slip Domain and MatNS."""
    dim = 3 if cfg.get("gmsh") else len(cfg["nelem"])
    bc = {"custom-func": {"name": "taylor_green3d" if dim == 3 else "taylor_green"}}
    if walls:
        bc = {"no-slip": walls}
    if cfg.get("gmsh"):
        dcfg = {"ngl": cfg["ngl"], "gmsh-file": msh, "partitioner": cfg["gmsh"]}
    else:
        dcfg = {"ngl": cfg["ngl"], "box-mesh": {"nelem": cfg["nelem"], "lower": [0] * dim, "upper": [1] * dim}}
    dom = pa.Domain()
    dom.configure({"domain": dcfg, "boundary-conditions": bc})
    dom.setUp()
    mat = pa.MatNS() if walls else pa.MatFS()
    mat.setDomain(dom)
    mat.build(buildOperators=operators)
    return dom, mat


def gather_csr(dist, size, A_):
    """This rank's export and every peer's: ranks_ref.global_csr's parts."""
    lo, hi = A_.getOwnershipRange()
    parts = [None] * size
    dist.all_gather_object(parts, (lo, hi) + tuple(A_.getValuesCSR()))
    return parts


def _worker(rank, size, port, cfg, msh, q):
    dist = rank_setup(rank, size, port, cfg)
    try:
        import pynama_amd as pa
        from pynama_amd.runtime import get_tuning, set_tuning
        dom, mat = build_system(pa, cfg, msh, False)
        mesh = dom.getMesh()
        K = mat.K
        lo, hi = K.getOwnershipRange()
        parts = gather_csr(dist, size, K)
        A, ranges = RR.global_csr(parts)
        dims, P = lattice(cfg)
        xs = RR.rank_inputs(A, ranges, dims, P)
        xs["big"] = xs["uniform"] * 1e305
        out = {"rank": rank, "part": parts[rank], "halo": mesh.halo(), "npeers": len(mesh.peers()),
               "transport": pa.get_ctx().device_info()["transport"], "storages": {}, "cg": {}}
        x = K.createVecRight()

        def products():
            ys = {}
            for nm, xa in xs.items():
                x.setArray(xa[lo:hi])
                ys[nm] = (K * x).getArray().copy()
            return ys

        for sname in cfg["storages"]:
            tun, sym, prefix, has = STORAGES[sname]
            keep = {k: get_tuning(k) for k in tun}
            try:
                for k, v in tun.items():
                    set_tuning(k, v)
                K.setOption(K.Option.SPD, sym)
                kern = K.spmvKernel()
                assert K.isSymmetricStorage() == sym, (sname, kern)
                assert prefix is None or kern.startswith(prefix), (sname, kern)
                assert has is None or has in kern, (sname, kern)
                bricks = K.getSymmetricBricks() if sym else None
                K.setHaloOverlap(True)
                ys = products()
                K.setHaloOverlap(False)
                plain = products()
                K.setHaloOverlap(True)
            finally:
                for k, v in keep.items():
                    set_tuning(k, v)
            out["storages"][sname] = {
                "kernel": kern, "bricks": None if bricks is None else bricks["bricks"], "y": ys,
                "plain_differs": [nm for nm in xs if not np.array_equal(ys[nm], plain[nm], equal_nan=True)]}
        if cfg.get("cg"):
            tun = cfg.get("cg_tunings", {})
            keep = {k: get_tuning(k) for k in tun}
            try:
                for k, v in tun.items():
                    set_tuning(k, v)
                K.setOption(K.Option.SPD, True)
                kern = K.spmvKernel()
                assert kern.startswith(cfg.get("cg_prefix", BRICK)), kern
                g = {"b": np.random.default_rng(77).uniform(-1.0, 1.0, A.m)[lo:hi]}  # (T.cg_case's b)
                out["cg_b"], out["cg_kernel"] = g["b"], kern
                for variant, pc in cfg["cg"]:
                    for fold in T.FOLDS[variant]:
                        # (on ranks the folded product reports the matrix's kernels: split_kernel_name)
                        hx, hr = T.cg_history(pa, K, g, variant, pc, fold, None)
                        out["cg"][(variant, pc, bool(fold and fold[1]))] = (hx[1:], hr[1:])
            finally:
                for k, v in keep.items():
                    set_tuning(k, v)
        q.put(out)
    except Exception:  # report instead of hanging the peers
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc()})
    finally:
        dist.destroy_process_group()


def gmsh_file(tmp_path_factory, nelem=None):
    key = "msh" if nelem is None else ("msh",) + tuple(nelem)
    if key not in _RUNS:
        from pynama_amd.meshgen import perturbed_box, write_gmsh
        path = str(tmp_path_factory.mktemp("ranksref") / "part.msh")
        write_gmsh(path, 3, *perturbed_box(3, GMSH if nelem is None else list(nelem), seed=5))
        _RUNS[key] = path
    return _RUNS[key]


def spawn(worker, cfg, msh):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, cfg["size"], port, cfg, msh, q)) for r in range(cfg["size"])]
    return _collect(procs, q, cfg["size"], timeout=240)


def _case(name, tmp_path_factory):
    """The run of a configuration and, from its parts, the global matrix, the
    inputs and their longdouble references -- once, left unchanged."""
    if name in _CASES:
        return _CASES[name]
    cfg = CONFIGS[name]
    assert cfg["size"] <= 8
    res = spawn(_worker, cfg, gmsh_file(tmp_path_factory) if cfg.get("gmsh") else None)
    assert all(r["transport"] == cfg.get("transport", "host") for r in res)
    host = cfg.get("host")
    if host and host in _CASES and _same_matrix(_CASES[host], res):
        h = _CASES[host]  # (the same matrix: the references are the host run's)
        c = dict(h, res=res)
    else:
        A, ranges = RR.global_csr([r["part"] for r in res])
        dims, P = lattice(cfg)
        xs = RR.rank_inputs(A, ranges, dims, P)
        refs = {}
        for nm, x in xs.items():
            ref, den = S.reference(A, x)
            refs[nm] = (ref, den, S.restatement(A, x, ref, den))
        big = xs["uniform"] * 1e305
        c = dict(res=res, A=A, ranges=ranges, xs=xs, refs=refs, ident=S.identity_rows(A), big=big,
                 big_ref=S.reference(A, big), symmetric=S.is_symmetric(A), asym=S.asymmetry(A), apriori={},
                 dims=dims, P=P)
    _CASES[name] = c
    return c


def _same_matrix(h, res):
    return all(len(a["part"]) == len(b["part"]) and all(np.array_equal(u, v) for u, v in zip(a["part"], b["part"]))
               for a, b in zip(h["res"], res))


def _require_shape(name, c):
    """The property each configuration was chosen for, from what the ranks report."""
    res, ranges, A = c["res"], c["ranges"], c["A"]
    size = CONFIGS[name]["size"]
    assert len(res) == size and [r["part"][:2] for r in res] == ranges
    nodes = [(hi - lo) // 3 for lo, hi in ranges]
    assert all(n > 0 for n in nodes)
    T.require_symmetric(c)
    rows = S._rows(A)
    for k, (lo, hi) in enumerate(ranges):  # every rank's rows read a peer's columns
        mine = (rows >= lo) & (rows < hi)
        assert np.any(mine & ((A.indices < lo) | (A.indices >= hi)) & (A.data != 0)), k
    if not CONFIGS[name].get("gmsh"):
        for k, r in enumerate(res):  # z slabs: the lower and the upper neighbour, none at the ends
            assert r["halo"]["lo_rank"] == (k - 1 if k > 0 else -1), (k, r["halo"])
            assert r["halo"]["hi_rank"] == (k + 1 if k < size - 1 else -1), (k, r["halo"])
    if name.startswith("box8"):  # one element layer per rank: the lower ghost range is a whole slab
        plane = c["dims"][0] * c["dims"][1]
        for k in range(2, size):  # (rank 0's lowest plane is all Dirichlet: K holds no column of it)
            lo, hi = ranges[k]
            cols = A.indices[A.indptr[lo]:A.indptr[hi]]
            below = cols[cols < lo] // 3 // plane  # the lattice planes of the columns below the owned rows
            assert (below.min(), below.max()) == (ranges[k - 1][0] // 3 // plane, lo // 3 // plane - 1), k
    if name == "slice64":
        assert all(n % 64 == 0 for n in nodes), nodes
    if name == "below64":
        assert all(n < 64 for n in nodes), nodes
    if name.startswith("gmsh4"):
        assert max(r["npeers"] for r in res) >= 2, [r["npeers"] for r in res]
    if CONFIGS[name].get("gmsh"):
        for k in range(size):  # the interface spikes sit on nodes with a neighbour owned by a peer
            assert len(RR.interface_nodes(A, ranges, None, k)) == 2, k
    combs = [nm for nm in c["xs"] if nm.startswith("comb")]
    if c["P"] is not None and c["P"] <= 2:
        hit = np.zeros(A.n, bool)
        for nm in combs:
            assert S.terms_per_row(A, c["xs"][nm]).max() <= 1, nm
            hit |= c["xs"][nm] != 0
        assert len(combs) == (2 * c["P"] + 1) ** 3 and hit.reshape(-1, 3).any(axis=1).all()
    else:
        for nm in combs:
            assert S.terms_per_row(A, c["xs"][nm]).max() == 1 and np.count_nonzero(c["xs"][nm]) >= 1, nm


def _allowance(c, sym, nm, x):
    A = c["A"]
    if not sym:
        return np.zeros(A.m, LD)
    if nm not in c["apriori"]:
        c["apriori"][nm] = S.apriori_quantum(A, x)
    q, nT = c["apriori"][nm]
    return nT * q / 2


def _check_big(name, c, r, sname, sym, y, bad):
    """x near overflow (the `big` case of test_gpu_sym_ref.run_products): never
    a finite wrong value.  A row whose den_i = sum |K_ij||x_j| is below DBL_MAX
    cannot overflow in any summation order: finite and within the tolerance.
    A row whose reference is past DBL_MAX: non-finite.  Between the two
    (|ref_i| < DBL_MAX <= den_i; the flat elements of the 8-slab box have such
    rows) a partial sum may pass DBL_MAX in one order and not in another, so
    fp64 allows either answer: non-finite, or finite and within the tolerance."""
    lo, hi = r["part"][:2]
    xa = c["big"]
    ref, den = (a[lo:hi] for a in c["big_ref"])
    with np.errstate(all="ignore"):
        fin = np.abs(ref) < LD(S.DBL_MAX)
        safe = den < LD(S.DBL_MAX)
        allow = _allowance(c, sym, "big", xa)[lo:hi]
        rest = c["refs"]["uniform"][2]  # (the same x but for the scale)
        tol = 16 * LD(max(rest, S.U)) * den + allow
        isf = np.isfinite(y)
        err = np.where(isf, np.abs(np.where(isf, y, 0.0).astype(LD) - ref), LD(0))
        within = isf & (err <= tol)
        on = isf & fin & (tol > 0)
        used = float((err[on] / tol[on]).max()) if on.any() else 0.0
    print(f"SYMREF-RANKS {name} rank={r['rank']} storage={sname} input=near_overflow rows_past_dbl_max={int((~fin).sum())} "
          f"rows_either_way={int((fin & ~safe).sum())} of them finite={int((fin & ~safe & isf).sum())} "
          f"tol_used={used:.3f}")
    if not within[safe].all():
        bad.append((r["rank"], "near_overflow: rows that cannot overflow", int((~within[safe]).sum())))
    mid = fin & ~safe
    if not np.all(within[mid] | ~isf[mid]):
        bad.append((r["rank"], "near_overflow: finite wrong values", int((~(within[mid] | ~isf[mid])).sum())))
    if not np.all(~isf[~fin]):
        bad.append((r["rank"], "near_overflow: finite values past DBL_MAX", int(isf[~fin].sum())))
    ident = c["ident"][(c["ident"] >= lo) & (c["ident"] < hi)]
    assert np.array_equal(y[ident - lo], xa[ident])


PRODUCT_PARAMS = [pytest.param(n, s, id=f"{n}-{s}") for n, cfg in CONFIGS.items() for s in cfg["storages"]]


@pytest.mark.parametrize("name,sname", PRODUCT_PARAMS)
def test_rank_products_match_longdouble(name, sname, tmp_path_factory):
    c = _case(name, tmp_path_factory)
    _require_shape(name, c)
    sym = STORAGES[sname][1]
    bad, worst_t, worst_a = [], 0.0, 0.0
    for r in c["res"]:
        lo, hi = r["part"][:2]
        st = r["storages"][sname]
        print(f"SYMREF-RANKS {name} rank={r['rank']} storage={sname} kernel={st['kernel']} bricks={st['bricks']} "
              f"node_rows={(hi - lo) // 3}")
        assert not st["plain_differs"], (r["rank"], "overlapped != plain", st["plain_differs"])
        if sname == "rounds4":
            assert st["bricks"] > 1
        if STORAGES[sname][2] == BRICK:
            assert st["bricks"] is not None and st["bricks"] >= 1
        ident = c["ident"][(c["ident"] >= lo) & (c["ident"] < hi)]
        fam = {}
        for nm, xa in c["xs"].items():
            ref, den, rest = c["refs"][nm]
            y = st["y"][nm]
            allow = _allowance(c, sym, nm, xa)
            dev, used, aused, ok = RR.owned_slice_check(y, lo, hi, ref, den, rest, allow)
            f = RR.family(nm)
            fam[f] = [max(a, b) for a, b in zip(fam.get(f, [0.0] * 4), (rest, dev, used, aused))]
            assert np.array_equal(y[ident - lo], xa[ident]), (r["rank"], nm, "identity rows")
            if nm.startswith("only_r") and int(nm[6:]) != r["rank"]:
                # nothing of this rank's own x: what is not 0 came through a halo
                assert not np.any(y[np.asarray(den[lo:hi] == 0)] != 0)
            if not ok:
                bad.append((r["rank"], nm, used))
            if nm == "uniform":
                # the check bites: the device's y with one owned row moved by 1e-12 den_i
                # (what a received sum counted 1 + 1e-12 times would do) does not pass
                i = int(np.argmax(den[lo:hi]))
                moved = y.copy()
                moved[i] += 1e-12 * float(den[lo + i])
                assert moved[i] != y[i] and not RR.owned_slice_check(moved, lo, hi, ref, den, rest, allow)[3], r["rank"]
        for f, (rest, dev, used, aused) in fam.items():
            print(f"SYMREF-RANKS {name} rank={r['rank']} storage={sname} input={f} restatement={rest / S.U:.3g}u "
                  f"device={dev / S.U:.3g}u tol_used={used:.3f} allowance_used={aused:.3f}")
            worst_t, worst_a = max(worst_t, used), max(worst_a, aused)
        _check_big(name, c, r, sname, sym, st["y"]["big"], bad)
    WORST[(name, sname)] = (worst_t, worst_a)
    assert not bad, (name, sname, bad)


@pytest.mark.parametrize("name", [n for n, cfg in CONFIGS.items() if cfg.get("host")])
def test_ipc_transport_equals_host_bitwise(name, tmp_path_factory):
    """The product does not depend on how its halos travel."""
    h = _case(CONFIGS[name]["host"], tmp_path_factory)
    c = _case(name, tmp_path_factory)
    assert _same_matrix(h, c["res"])
    for a, b in zip(c["res"], h["res"]):
        assert a["transport"] == "ipc" and b["transport"] == "host"
        for sname in CONFIGS[name]["storages"]:
            assert a["storages"][sname]["kernel"] == b["storages"][sname]["kernel"]
            for nm, y in a["storages"][sname]["y"].items():
                assert np.array_equal(y, b["storages"][sname]["y"][nm], equal_nan=True), (a["rank"], sname, nm)


# ------------------------------------------------ b. CG through the rank products
CG_PARAMS = [pytest.param(n, v, pc, id=f"{n}-{pc}-{v}") for n, cfg in CONFIGS.items() for v, pc in cfg.get("cg", [])]


@pytest.mark.parametrize("name,variant,pc", CG_PARAMS)
def test_rank_cg_iterates_match_reference(name, variant, pc, tmp_path_factory):
    """A ghost slice's sums folded in twice, a stale receive buffer or a wrong
    split of the gather is an O(1) error in an iterate; with corrections off
    nothing repairs it."""
    c = _case(name, tmp_path_factory)
    _require_shape(name, c)
    res = c["res"]
    g = T.cg_case(c, ("ranks", name), pc)
    for r in res:
        lo, hi = r["part"][:2]
        assert np.array_equal(r["cg_b"], g["b"][lo:hi])
        assert r["cg_kernel"].startswith(CONFIGS[name].get("cg_prefix", BRICK)), r["cg_kernel"]
    ex, er = g["err"][variant]
    tolx, tolr = 16 * max(ex, R.FLOOR), 16 * max(er, R.FLOOR)
    hist = {}
    for fold in T.FOLDS[variant]:
        folded = bool(fold and fold[1])
        key = (variant, pc, folded)
        rns = res[0]["cg"][key][1]
        for r in res:  # the norms are allreduced: the same bits on every rank
            assert r["cg"][key][1] == rns, r["rank"]
        xs = [None] + [np.concatenate([r["cg"][key][0][k] for r in res]) for k in range(T.CG_ITERS)]
        dx, dr = T.history_errors(xs, [None] + list(rns), g)
        print(f"SYMREF-CG ranks={name} variant={variant} pc={pc} gather={'folded' if folded else 'separate'} "
              f"restatement_x={ex:.2e} device_x={dx:.2e} tol_used_x={dx / tolx:.3f} "
              f"restatement_r={er:.2e} device_r={dr:.2e} tol_used_r={dr / tolr:.3f}")
        WORST[(name, "cg", variant, pc, folded)] = (max(dx / tolx, dr / tolr), 0.0)
        assert dx <= tolx, (fold, dx, tolx)
        assert dr <= tolr, (fold, dr, tolr)
        hist[folded] = xs
    if len(hist) == 2:
        for k in range(1, T.CG_ITERS + 1):
            d = float(np.abs(hist[True][k] - hist[False][k]).max() / np.abs(g["xs"][k]).max())
            assert d <= tolx, (k, d, tolx)


def test_worst_shares_on_ranks():
    """The figures of DESIGN.md: the worst shares of the tolerance and of the
    allowance over the cases run so far (last in this file)."""
    prod = [v for k, v in WORST.items() if len(k) == 2]
    cg = [v for k, v in WORST.items() if len(k) > 2]
    for k, (t, a) in sorted(WORST.items(), key=lambda kv: str(kv[0])):
        print(f"SYMREF-RANKS worst {' '.join(map(str, k))}: tol_used={t:.3f} allowance_used={a:.3f}")
    if prod:
        print(f"SYMREF-RANKS worst of all products: tol_used={max(t for t, _ in prod):.3f} "
              f"allowance_used={max(a for _, a in prod):.3f}")
    if cg:
        print(f"SYMREF-CG worst of all rank histories: tol_used={max(t for t, _ in cg):.3f}")
    assert all(t <= 1.0 and a <= 1.0 for t, a in WORST.values())
