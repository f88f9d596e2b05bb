"""A matrix multiplies by what it exports (tests/test_gpu_mat_ref.py), on
ranks: mult and multAdd of the assembled Krhs, Rw, Curl, SrT and DivSrT, row
by row against the longdouble product of the global exported CSR
(ranks_ref.global_csr of the ranks' getValuesCSR() parts) within
mat_ref.product's bound, 1.01 n_i u sum_k |a_ik||x_k| (mult_add: one more
rounding of the result).  Full storage on ranks launches the interior rows
beside the halo and the ghost-dependent rows behind an event (kle_mat.hip);
each row is still one sum of its stored entries, so the one-rank bound holds
unchanged.

2 ranks: the 3-D box [3,2,4] ngl 4, the 2-D box [4,6] ngl 4 and the slab
partition of perturbed_box(3, [4,4,4], seed 5) ngl 3.  The right-hand vectors
carry their ghosts by the matrix's column block size -- 1 (2-D vorticity),
2 or 3 (velocity), 3 (3-D vorticity, 2-D strain), 6 (3-D strain) -- and for
each of them some checked row of every rank reads a ghost column (asserted).
Inputs: uniform, the 6-decade ramp, and only_r{k} per rank (uniform on rank
k's columns, 0 elsewhere: every nonzero of the other rank's rows came through
the halo).  One spawned run per configuration; the parent never opens the
GPU.  Each matrix prints a MATREF-RANKS line with its worst err / bound."""
import numpy as np
import pytest

import mat_ref as M
import ranks_ref as RR
import test_gpu_sym_ranks_ref as SR

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
MATS = ("Krhs", "Rw", "Curl", "SrT", "DivSrT")
CONFIGS = {
    "box3d": dict(size=2, nelem=[3, 2, 4], ngl=4, col_blocks={3, 6}),
    "box2d": dict(size=2, nelem=[4, 6], ngl=4, col_blocks={1, 2, 3}),
    "gmsh3d": dict(size=2, gmsh="slab", ngl=3, col_blocks={3, 6}),
}
_RUNS = {}


def _worker(rank, size, port, cfg, msh, q):
    dist = SR.rank_setup(rank, size, port, cfg)
    try:
        import pynama_amd as pa
        dom, mat = SR.build_system(pa, cfg, msh, True)
        op = mat.getOperators()
        mats = {"Krhs": mat.Krhs, "Rw": mat.Rw, "Curl": op.Curl, "SrT": op.SrT, "DivSrT": op.DivSrT}
        out = {"rank": rank, "mats": {}}
        for name in MATS:
            A = mats[name]
            lo, hi = A.getOwnershipRange()
            m, n = A.getSize()
            x, y, z, v = A.createVecRight(), A.createVecLeft(), A.createVecLeft(), A.createVecLeft()
            clo, chi = x.getOwnershipRange()
            parts = SR.gather_csr(dist, size, A)
            cols = [None] * size
            dist.all_gather_object(cols, (clo, chi))
            xs = RR.op_inputs(n, cols, seed=len(name))
            ya = M.x_uniform(m, 77)[lo:hi]
            r = {"part": parts[rank], "cols": (clo, chi), "size": (m, n), "blocks": (A._rbs, A._cbs),
                 "kernel": A.spmvKernel(), "format": A.getFormat(), "y": {}, "z": {}, "zy": {}}
            for nm, xa in xs.items():
                x.setArray(xa[clo:chi])
                y.set(SENTINEL)  # (a row the kernel does not write stays visible)
                A.mult(x, y)
                r["y"][nm] = y.getArray().copy()
                v.setArray(ya)
                z.set(SENTINEL)
                A.multAdd(x, v, z)
                assert np.array_equal(v.getArray(), ya), (name, nm, "multAdd changed y")
                r["z"][nm] = z.getArray().copy()
                A.multAdd(x, v, v)
                r["zy"][nm] = v.getArray().copy()
            out["mats"][name] = r
        q.put(out)
    except Exception:  # report instead of hanging the peer
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc()})
    finally:
        dist.destroy_process_group()


def _run(name, tmp_path_factory):
    if name not in _RUNS:
        cfg = CONFIGS[name]
        _RUNS[name] = SR.spawn(_worker, cfg, SR.gmsh_file(tmp_path_factory) if cfg.get("gmsh") else None)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_rank_operators_multiply_by_what_they_export(name, tmp_path_factory):
    res = _run(name, tmp_path_factory)
    cfg = CONFIGS[name]
    ghost_read = {}  # column block size -> per rank: some checked row reads a ghost column
    for mname in MATS:
        rs = [r["mats"][mname] for r in res]
        m, n = rs[0]["size"]
        rbs, cbs = rs[0]["blocks"]
        E, ranges = RR.global_csr([r["part"] for r in rs], ncols=n)
        assert E.m == m
        cols = [r["cols"] for r in rs]
        assert cols[0][0] == 0 and cols[-1][1] == n and all(a[1] == b[0] for a, b in zip(cols, cols[1:])), cols
        assert all((hi - lo) % rbs == 0 for lo, hi in ranges) and all((hi - lo) % cbs == 0 for lo, hi in cols)
        xs = RR.op_inputs(n, cols, seed=len(mname))
        ya = M.x_uniform(m, 77)
        rows = M.rows_of(E)
        worst, worst_a = (0.0, None), (0.0, None)
        for nm, xa in xs.items():
            ref, b = M.product(E, xa)
            zr, zb = M.mult_add(ref, b, ya)
            for k, (r, (lo, hi), (clo, chi)) in enumerate(zip(rs, ranges, cols)):
                w, at = M.worst(r["y"][nm], ref[lo:hi], b[lo:hi])
                assert w <= 1, (name, mname, nm, "mult", k, w, at)
                if w >= worst[0]:
                    worst = (w, (k, at[0] if at else None, nm))
                for which in ("z", "zy"):
                    w, at = M.worst(r[which][nm], zr[lo:hi], zb[lo:hi])
                    assert w <= 1, (name, mname, nm, "multAdd", which, k, w, at)
                    if w >= worst_a[0]:
                        worst_a = (w, (k, at[0] if at else None, nm, which))
                mine = (rows >= lo) & (rows < hi)
                ghost = mine & ((E.indices < clo) | (E.indices >= chi)) & (E.data != 0)
                if nm == "uniform":
                    ghost_read.setdefault(cbs, [False] * len(rs))
                    ghost_read[cbs][k] = ghost_read[cbs][k] or bool(ghost.any())
                if nm.startswith("only_r") and int(nm[6:]) != k and ghost.any():
                    # rank k's rows see the other rank's x through the halo alone, and they do see it
                    assert np.any(ref[lo:hi] != 0) and np.any(r["y"][nm] != 0), (name, mname, nm, k)
        print(f"MATREF-RANKS {name} {mname} blocks={rbs}x{cbs} format={rs[0]['format']} kernel={rs[0]['kernel']} "
              f"mult: worst err/bound {worst[0]:.3g} at {worst[1]}; multAdd: {worst_a[0]:.3g} at {worst_a[1]}")
    assert set(ghost_read) == cfg["col_blocks"], (set(ghost_read), cfg["col_blocks"])
    for cbs, seen in ghost_read.items():
        assert all(seen), (name, cbs, seen)
