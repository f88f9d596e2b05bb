"""Row dedup of the brick value stream (kle_brick.hip brick_dedup; tuning
spmv_brick_dedup).

A box-mesh K repeats a few distinct rows over its lattice.  With
spmv_brick_dedup 1 the bricked rows whose packed streams are bitwise equal
share one copy: a hash proposes, a comparison decides, and the kernel reads
the same values in the same order.  So:

  * the product is the product of spmv_brick_dedup 0 bit for bit -- for a
    random x, an x with one huge entry and a NaN x, repeated products too --
    on the compact and the full stream, on the planned bricks and on a forced
    split, with the one-block rows in the gather and as items of the bricks;
  * the rows stored lie between the count D of distinct upper-triangle rows
    of the exported CSR (relative block positions and value bits: ground
    truth computed here, not by the library) and 2 D (in the compact stream a
    unit's second row stores its last partial pass first: other bytes than
    the same row as a first one; the full layout stores exactly D rows);
  * a row that differs from every other keeps its own storage, and a matrix
    without duplicates reports dedup false and keeps the old layout;
  * 30 single-reduction CG iterations give the same iterates bit for bit,
    and the classic recurrence on the shared rows meets the longdouble
    reference within the brick CG tests' tolerance.

Meshes (the smallest that go wrong in their own way): [4,3,3] ngl 3 (interior
elements on every axis, spacing 1/3 inexact in y and z), [4,4,2] ngl 3 (exact
spacing), [3,3,2] ngl 5 (rows of more than 64 blocks: several passes and the
shared tail item), [2,2,2] ngl 5 (no interior element, few duplicates).
Measured: these four repeat too few rows for the sharing to save half of the
bytes (D 111 of 174, 93 of 146, 810 of 846, 342 of 342 bricked rows), so the
library keeps their old layout; [8,8,4] ngl 3 and [8,8,2] ngl 5 (rows of more
than 64 blocks) are where the shared storage itself is multiplied with.
Every case with asm_box_uniform 1 (default: translated rows are the same
bits) and 0 (each cell's own matrix: no two rows equal on these meshes).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MESHES = {
    "4x3x3-p2": ([4, 3, 3], 3),
    "4x4x2-p2": ([4, 4, 2], 3),
    "3x3x2-p4": ([3, 3, 2], 5),
    "2x2x2-p4": ([2, 2, 2], 5),
    # enough elements along x and y that most rows are translates of another:
    # the sharing is taken here (the four above repeat too little to save half)
    "8x8x4-p2": ([8, 8, 4], 3),
    "8x8x2-p4": ([8, 8, 2], 5),
}
# tunings of the brick storage beside spmv_brick_dedup / spmv_brick_compact
PLANS = {
    "planned": {},
    "split": {"spmv_brick_split": 2 + 100 * 2 + 10000 * 1},  # ([8,8,2] ngl 5: 4 x 4 x 1, whose regions fit the LDS)
    "singles0": {"spmv_brick_singles": 0},
}


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


_mats = {}


def get_mat(pa, name, uniform=1):
    """The assembled K of a mesh (asm_box_uniform = uniform, read at assembly)
    and its exported CSR: built once."""
    from pynama_amd.runtime import get_tuning, set_tuning
    if (name, uniform) not in _mats:
        nelem, ngl = ([3, 2, 2], 5) if name == "3x2x2-p4" else MESHES[name]
        cfg = {"domain": {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": [0, 0, 0], "upper": [1, 1, 1]}},
               "boundary-conditions": {"custom-func": {"name": "taylor_green3d"}}}
        keep = get_tuning("asm_box_uniform")
        set_tuning("asm_box_uniform", uniform)
        try:
            dom = pa.Domain()
            dom.configure(cfg)
            dom.setUp()
            mat = pa.MatFS()
            mat.setDomain(dom)
            mat.build(buildOperators=False)
        finally:
            set_tuning("asm_box_uniform", keep)
        _mats[(name, uniform)] = dict(dom=dom, mat=mat, L=[(ngl - 1) * e + 1 for e in nelem],
                                      csr={m: tuple(getattr(mat, m).getValuesCSR()) for m in ("K", "Krhs", "Rw")})
    return _mats[(name, uniform)]


class storage:
    """K in brick storage under the given tunings; on exit the tunings as
    they were and K in full storage."""

    def __init__(self, K, **tunings):
        self.K, self.tunings = K, tunings

    def __enter__(self):
        from pynama_amd.runtime import get_tuning, set_tuning
        self.keep = {k: get_tuning(k) for k in self.tunings}
        for k, v in self.tunings.items():
            set_tuning(k, v)
        self.K.setOption(self.K.Option.SPD, False)
        self.K.setOption(self.K.Option.SPD, True)
        assert self.K.spmvKernel().startswith("k_nb_spmv_sym_brick"), self.K.spmvKernel()
        return self.K

    def __exit__(self, *exc):
        from pynama_amd.runtime import set_tuning
        for k, v in self.keep.items():
            set_tuning(k, v)
        self.K.setOption(self.K.Option.SPD, False)
        return False


def inputs(n):
    rng = np.random.default_rng(5)
    x = rng.uniform(-1.0, 1.0, n)
    huge = x.copy()
    huge[n // 3] = 1e200
    nan = x.copy()
    nan[n // 2] = np.nan
    return {"random": x, "huge": huge, "nan": nan}


def products(K):
    x = K.createVecRight()
    out = {}
    for nm, xa in inputs(x.getLocalSize()).items():
        x.setArray(xa)
        y = (K * x).getArray().copy()
        np.testing.assert_array_equal(_bits((K * x).getArray()), _bits(y))  # (repeatable)
        out[nm] = y
    return out


def distinct_rows(csr, L, singles):
    """(D, bricked rows, bytes of the distinct rows, bytes of all): the
    distinct upper-triangle rows of the node-block CSR among the rows the
    bricks hold (spmv_brick_singles 1: those with more than one stored block),
    each as its blocks' lattice offsets from the row and the bits of their 9
    values; bytes in the full layout (9 doubles per block, rows padded to 16
    doubles)."""
    ip, ix, d = csr
    n = (len(ip) - 1) // 3
    seen = {}
    rows = total = 0
    for i in range(n):
        key = []
        nblk = 0
        for a in range(3):
            s, e = ip[3 * i + a], ip[3 * i + a + 1]
            cols, vals = np.asarray(ix[s:e], np.int64), d[s:e]
            up = cols // 3 >= i
            nblk = int(up.sum()) // 3
            key.append((cols[up] - 3 * i).tobytes())
            key.append(_bits(vals[up]).tobytes())
        if singles and nblk <= 1:
            continue
        rows += 1
        seen[tuple(key)] = 8 * ((9 * nblk + 15) // 16 * 16)
        total += 8 * ((9 * nblk + 15) // 16 * 16)
    return len(seen), rows, sum(seen.values()), total


@pytest.mark.parametrize("uniform", [1, 0])
@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("compact", [1, 0])
@pytest.mark.parametrize("name", list(MESHES))
def test_product_is_bitwise_the_full_streams_and_rows_are_stored_once(pa, name, compact, plan, uniform):
    c = get_mat(pa, name, uniform)
    K = c["mat"].K
    tun = dict(PLANS[plan], spmv_brick_dedup_full=0)  # (the layout asked for, shared or not)
    if plan == "split" and name == "8x8x2-p4":
        tun["spmv_brick_split"] = 4 + 100 * 4 + 10000 * 1
    with storage(K, spmv_brick_dedup=0, spmv_brick_compact=compact, **tun):
        info0 = K.getSymmetricBricks()
        bytes0, kern0 = K.spmvBytes(), K.spmvKernel()
        y0 = products(K)
    with storage(K, spmv_brick_dedup=1, spmv_brick_compact=compact, **tun):
        info1 = K.getSymmetricBricks()
        bytes1, kern1 = K.spmvBytes(), K.spmvKernel()
        y1 = products(K)
    assert info0["dedup"] is False and info0["unique_rows"] == 0 and info0["unique_bytes"] == 0
    assert info0["compact"] is bool(compact) and info1["compact"] is bool(compact)
    assert (bytes0, kern0) == (bytes1, kern1)  # (reported as before: what the loads request)
    assert {k: v for k, v in info1.items() if not k.startswith(("dedup", "unique"))} == \
           {k: v for k, v in info0.items() if not k.startswith(("dedup", "unique"))}
    for nm in y0:
        np.testing.assert_array_equal(_bits(y1[nm]), _bits(y0[nm]), err_msg=nm)
    assert np.isnan(y0["nan"]).any() and np.isfinite(y0["random"]).all()
    singles = PLANS[plan].get("spmv_brick_singles", 1)
    D, rows, dbytes, total = distinct_rows(c["csr"]["K"], c["L"], singles)
    print(f"DEDUP {name} uniform={uniform} compact={compact} plan={plan}: bricked rows {rows} ({total} B full layout), "
          f"distinct D {D} ({dbytes} B), stored {info1['unique_rows']} ({info1['unique_bytes']} B), "
          f"dedup {info1['dedup']}")
    if info1["dedup"]:
        assert D <= info1["unique_rows"] <= 2 * D, (D, info1)
        if not compact:
            assert dbytes <= info1["unique_bytes"] <= 2 * dbytes, (dbytes, info1)
        assert 0 < 2 * info1["unique_bytes"] <= total
    elif not compact:
        # refused only where sharing saves less than half of the bytes: the
        # stored rows are at most the distinct ones in both roles of a unit
        assert 2 * (2 * dbytes) > total, (dbytes, total)
    if name.startswith("8x8") and uniform:
        assert 4 * dbytes <= total  # (these meshes repeat enough, whatever the roles)
        assert info1["dedup"] is True


def test_shared_rows_keep_the_full_blocks_by_default(pa):
    """spmv_brick_dedup_full 1 (default): a K whose rows are shared is stored
    in the full 9-entry blocks (its kernel is bound by instructions, not
    bytes); one whose rows are not keeps the compact stream as before.  The
    product is the compact stream's to rounding (another fixed-point scale
    only where a brick's bound differs: here the same bits)."""
    shared, own = get_mat(pa, "8x8x2-p4")["mat"].K, get_mat(pa, "3x3x2-p4")["mat"].K
    with storage(shared):
        info = shared.getSymmetricBricks()
        y1 = products(shared)
    assert info["dedup"] is True and info["compact"] is False and info["dropped_entries"] == 0
    with storage(shared, spmv_brick_dedup_full=0):
        info = shared.getSymmetricBricks()
        y0 = products(shared)
    assert info["dedup"] is True and info["compact"] is True and info["dropped_entries"] > 0
    assert np.abs(y1["random"] - y0["random"]).max() <= 1e-13 * np.abs(y0["random"]).max()
    with storage(own):
        info = own.getSymmetricBricks()
    assert info["dedup"] is False and info["compact"] is True


def _node_rows(csr, i):
    ip, ix, d = csr
    out = []
    for a in range(3):
        s, e = ip[3 * i + a], ip[3 * i + a + 1]
        out.append(((np.asarray(ix[s:e], np.int64) - 3 * i).tobytes(), _bits(d[s:e]).tobytes()))
    return out


def test_uniform_assembly_makes_translated_rows_the_same_bits(pa):
    """[4,3,3] ngl 3 (spacing 1/3: each cell's own matrix differs from the
    next one's in the last places).  With asm_box_uniform 1 the free rows at
    x = 3 and x = 5 -- the mid nodes of the two interior elements along x,
    whose columns are all free -- are translates of each other: whole rows of
    K, Krhs and Rw equal bit for bit, so D is below the bricked row count by
    at least those pairs.  Key 1 against key 0: max |dK| <= 1e-12 max |K|, the
    bound of the assembled-against-oracle tests."""
    name = "4x3x3-p2"
    c1, c0 = get_mat(pa, name, 1), get_mat(pa, name, 0)
    L = c1["L"]
    pairs = 0
    for z in range(1, L[2] - 1):
        for y in range(1, L[1] - 1):
            i, j = 3 + L[0] * (y + L[1] * z), 5 + L[0] * (y + L[1] * z)
            for m in ("K", "Krhs", "Rw"):
                assert _node_rows(c1["csr"][m], i) == _node_rows(c1["csr"][m], j), (m, y, z)
            pairs += 1
    D, rows, _, _ = distinct_rows(c1["csr"]["K"], L, 1)
    D0, rows0, _, _ = distinct_rows(c0["csr"]["K"], L, 1)
    print(f"DEDUP {name}: uniform 1: D {D} of {rows} bricked rows ({pairs} translated pairs); uniform 0: D {D0}")
    assert rows == rows0 and D <= rows - pairs and D <= D0
    for m in ("K", "Krhs", "Rw"):
        (ip, ix, d), (ip0, ix0, d0) = c1["csr"][m], c0["csr"][m]
        np.testing.assert_array_equal(ip, ip0)
        np.testing.assert_array_equal(ix, ix0)
        assert np.abs(d - d0).max() <= 1e-12 * np.abs(d0).max(), m


def _scaled(pa, name, d):
    """A fresh K of the mesh scaled to diag(d) K diag(d) (symmetric still)."""
    c = get_mat(pa, name)
    mat = pa.MatFS()
    mat.setDomain(c["dom"])
    mat.build(buildOperators=False)
    K = mat.K
    v = K.createVecRight()
    v.setArray(d)
    K.diagonalScale(v, v)
    K.assemble()
    return mat, K


def _host_product(K, xa):
    import scipy.sparse as sp
    ip, ix, d = K.getValuesCSR()
    return sp.csr_matrix((d, ix, ip), shape=(len(ip) - 1, len(xa))) @ xa


def test_a_changed_row_keeps_its_own_storage_and_the_dedup_reruns(pa):
    """Values changed after the first symmetric copy (one node's rows and
    columns doubled: exact, symmetric): the copy is rebuilt, the dedup reruns
    on the new values -- the changed rows no longer equal their former
    representatives -- and the product is the full stream's, bit for bit, and
    the exported CSR's to rounding.  (A single entry cannot be set: setValues
    refuses a node-block matrix, asserted here, so no setValues path leads
    into the rebuild; diagonalScale is the narrowest value change a bricked K
    takes.)"""
    name = "8x8x4-p2"
    c = get_mat(pa, name)
    n = 3 * int(np.prod(c["L"]))
    L = c["L"]
    node = 3 + L[0] * (3 + L[1] * 1)  # (a free node inside the lattice)
    d = np.ones(n)
    d[3 * node:3 * node + 3] = 2.0
    mat, K = _scaled(pa, name, np.ones(n))
    with pytest.raises(pa.petsc.Error):
        K.setValue(3 * node, 3 * node, 1.0)
    with storage(K, spmv_brick_dedup=1):
        before = K.getSymmetricBricks()
        assert before["dedup"] is True
        v = K.createVecRight()
        v.setArray(d)
        K.diagonalScale(v, v)
        K.assemble()
        K.setOption(K.Option.SPD, True)
        after = K.getSymmetricBricks()
        y1 = products(K)
    with storage(K, spmv_brick_dedup=0):
        y0 = products(K)
    assert after["dedup"] is True
    assert after["unique_rows"] > before["unique_rows"], (before, after)
    for nm in y0:
        np.testing.assert_array_equal(_bits(y1[nm]), _bits(y0[nm]), err_msg=nm)
    xa = inputs(n)["random"]
    yh = _host_product(K, xa)
    assert np.abs(y1["random"] - yh).max() <= 1e-13 * np.abs(yh).max()
    ch = np.abs(_host_product(get_mat(pa, name)["mat"].K, xa) - yh).max()
    assert ch > 1e-3 * np.abs(yh).max()  # (the change is in the product)


def test_a_matrix_without_duplicates_keeps_the_old_layout(pa):
    """diag(d) K diag(d) with every d distinct: no two rows equal, so nothing
    is shared, dedup is reported false and the product is unchanged."""
    name = "8x8x4-p2"
    n = 3 * int(np.prod(get_mat(pa, name)["L"]))
    d = 1.0 + np.arange(n) / (4.0 * n)
    mat, K = _scaled(pa, name, d)
    D, rows, _, _ = distinct_rows(tuple(K.getValuesCSR()), get_mat(pa, name)["L"], 1)
    assert D == rows
    with storage(K, spmv_brick_dedup=1):
        info = K.getSymmetricBricks()
        y1 = products(K)
    with storage(K, spmv_brick_dedup=0):
        info0 = K.getSymmetricBricks()
        y0 = products(K)
    assert info["dedup"] is False and info["unique_rows"] == 0 and info == info0
    for nm in y0:
        np.testing.assert_array_equal(_bits(y1[nm]), _bits(y0[nm]), err_msg=nm)


@pytest.mark.parametrize("full", [0, 1])
@pytest.mark.parametrize("fold", [0, 2])
def test_cg_iterates_are_bitwise_equal(pa, fold, full):
    """30 single-reduction CG iterations with Jacobi (the benchmark's KSP; its
    gather separate, ksp_sr_gather 0, and folded into the update, 2): every
    product is the same bits, so the iterate and the residual norm are.
    full 0: spmv_brick_dedup_full 0, both legs in the compact stream -- the
    sharing alone differs.  full 1 (default): the shared K keeps the full
    blocks, the other leg the compact stream; still the same bits on this K
    (the entries the compact stream leaves out are exact zeros, the sums are
    fixed-point and the bricks' bounds are equal)."""
    import test_gpu_sym_ref as T
    from pynama_amd.runtime import get_tuning, set_tuning
    K = get_mat(pa, "8x8x2-p4")["mat"].K
    b = np.random.default_rng(3).uniform(-1.0, 1.0, K.createVecRight().getLocalSize())
    out = {}
    keep = get_tuning("ksp_sr_gather")
    set_tuning("ksp_sr_gather", fold)
    try:
        for dd in (0, 1):
            with storage(K, spmv_brick_dedup=dd, spmv_brick_dedup_full=full):
                info = K.getSymmetricBricks()
                assert info["dedup"] is bool(dd) and info["compact"] is not bool(dd and full), info
                ksp = T.make_ksp(pa, K, "sr", "jacobi")
                bv, x = K.createVecLeft(), K.createVecRight()
                bv.setArray(b)
                ksp.setFixedIterations(30)
                ksp.solve(bv, x)
                assert ksp.getIterationNumber() == 30
                out[dd] = (x.getArray().copy(), ksp.getResidualNorm())
    finally:
        set_tuning("ksp_sr_gather", keep)
    np.testing.assert_array_equal(_bits(out[1][0]), _bits(out[0][0]))
    assert out[1][1] == out[0][1]
    assert np.isfinite(out[0][0]).all()


@pytest.mark.parametrize("full", [1, 0])
def test_classic_cg_on_shared_rows_matches_the_reference(pa, full):
    """The classic CG recurrence (PC Jacobi) on the deduplicated K of [8,8,2]
    ngl 5, in the full blocks (default) and the compact stream: x_k and
    ||r_k||, k = 1 .. 12, against the longdouble recurrence on the exported
    CSR (krylov_ref.pcg_reference), with the tolerances of the brick CG tests
    (tests/test_gpu_sym_ref.py: 16 x the fp64 restatement's error of the same
    recurrence, floor 16 x 2.2e-16, residuals above 1e-6 ||b||)."""
    import krylov_ref as R
    import sym_ref as S
    import test_gpu_sym_ref as T
    c = get_mat(pa, "8x8x2-p4")
    K = c["mat"].K
    if "A" not in c:
        c["A"] = S.as_csr(*c["csr"]["K"])
        assert S.is_symmetric(c["A"])
    g = T.cg_case(c, ("dedup", "8x8x2-p4"), "jacobi")
    ex, er = g["err"]["cg"]
    with storage(K, spmv_brick_dedup=1, spmv_brick_dedup_full=full):
        info = K.getSymmetricBricks()
        assert info["dedup"] is True and info["compact"] is not bool(full), info
        xs, rns = T.cg_history(pa, K, g, "cg", "jacobi", None, None)
    dx, dr = T.history_errors(xs, rns, g)
    print(f"DEDUP-CG 8x8x2 ngl=5 variant=cg pc=jacobi full={full} restatement_x={ex:.2e} device_x={dx:.2e} "
          f"restatement_r={er:.2e} device_r={dr:.2e}")
    assert dx <= 16 * max(ex, R.FLOOR), (dx, ex)
    assert dr <= 16 * max(er, R.FLOOR), (dr, er)


# --------------------------------------------------------------- two ranks
ROOT = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))


def _slab_worker(rank, size, port, nelem, ngl, q):
    import os
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), KLE_TRANSPORT="host", RANK=str(rank),
                      WORLD_SIZE=str(size))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=size)
    try:
        import pynama_amd as pa
        cfg = {"domain": {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": [0, 0, 0], "upper": [1, 1, 1]}},
               "boundary-conditions": {"custom-func": {"name": "taylor_green3d"}}}
        dom = pa.Domain()
        dom.configure(cfg)
        dom.setUp()
        mat = pa.MatFS()
        mat.setDomain(dom)
        mat.build(buildOperators=False)
        K = mat.K
        out = {"rank": rank, "lo": K.getOwnershipRange()[0],
               "csr": {m: tuple(getattr(mat, m).getValuesCSR()) for m in ("K", "Krhs", "Rw")}}
        xv = K.createVecRight()
        xv.setArray(np.sin(np.arange(*K.getOwnershipRange(), dtype=np.float64)))
        from pynama_amd.runtime import set_tuning
        set_tuning("spmv_brick_dedup_full", 0)  # (both legs in the compact stream: the sharing alone differs)
        for dd in (0, 1):  # (symmetric storage is collective: both ranks take it)
            set_tuning("spmv_brick_dedup", dd)
            K.setOption(K.Option.SPD, False)
            K.setOption(K.Option.SPD, True)
            out[("y", dd)] = (K.spmvKernel(), K.getSymmetricBricks(), (K * xv).getArray().copy())
        q.put(out)
    except Exception:  # report instead of hanging the peer
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc()})
    finally:
        dist.destroy_process_group()


def test_two_z_slabs_assemble_the_one_rank_rows_and_share_their_own(pa):
    """[8,8,4] ngl 3 on 2 ranks (host transport): with asm_box_uniform 1 every
    rank adds global element 0's blocks, so its owned rows of K, Krhs and Rw
    are the one-rank matrices' rows bit for bit; each rank shares the rows of
    its own slab, and its product is its unshared stream's bit for bit (both
    in the compact layout, spmv_brick_dedup_full 0) and the one-rank product
    to rounding."""
    import torch.multiprocessing as mp
    from test_gpu_multirank import _collect, _free_port
    name = "8x8x4-p2"
    nelem, ngl = MESHES[name]
    size = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    res = _collect([ctx.Process(target=_slab_worker, args=(r, size, port, nelem, ngl, q)) for r in range(size)], q,
                   size)
    one = get_mat(pa, name)
    K1 = one["mat"].K
    x = K1.createVecRight()
    n = x.getLocalSize()
    x.setArray(np.sin(np.arange(n, dtype=np.float64)))
    K1.setOption(K1.Option.SPD, False)
    y_one = (K1 * x).getArray().copy()
    for r in sorted(res, key=lambda r: r["rank"]):
        for m in ("K", "Krhs", "Rw"):
            ip1, ix1, d1 = one["csr"][m]
            ip, ix, d = r["csr"][m]
            lo, rows = r["lo"], len(ip) - 1
            s, e = ip1[lo], ip1[lo + rows]
            np.testing.assert_array_equal(ip1[lo:lo + rows + 1] - s, ip, err_msg=m)
            np.testing.assert_array_equal(ix1[s:e], ix, err_msg=m)
            np.testing.assert_array_equal(_bits(d1[s:e]), _bits(d), err_msg=m)
        (k0, i0, y0), (k1, i1, y1) = r[("y", 0)], r[("y", 1)]
        assert k0.startswith("k_nb_spmv_sym_brick") and k1 == k0, (k0, k1)
        assert i0["dedup"] is False and i1["dedup"] is True and 0 < i1["unique_rows"], (i0, i1)
        assert i0["compact"] is True and i1["compact"] is True, (i0, i1)
        np.testing.assert_array_equal(_bits(y1), _bits(y0))
        sl = slice(r["lo"], r["lo"] + len(y1))
        for y in (y0, y1):
            assert np.abs(y - y_one[sl]).max() <= 1e-13 * np.abs(y_one).max()


# ------------------------------------------------------------ key 0 pinned
# sha256 of the values getValuesCSR returns with asm_box_uniform 0, recorded
# from the parent commit's library and reproduced by a key-0 run of this one
KEY0_SHA256 = {
    ("4x3x3-p2", "K"): "637e944e12d22392c1f469e78358aa912d6fe2cedb8e7812e16361b61fd7bf06",
    ("4x3x3-p2", "Krhs"): "368a68b9aa1af2decfad637cffb05581676062818d5bb37f339896c04e3217a4",
    ("4x3x3-p2", "Rw"): "19e76ee330728fbd197cea58dfc30d11c96aadd14ad6563e306e9bd569c00c85",
    ("3x2x2-p4", "K"): "bec74892232fbe8a926ae879485dcb6a6e025e8cd3d9375033006a829f081fce",
    ("3x2x2-p4", "Krhs"): "272256e1d229e61d86d4f9c263fbb6d0e55562a3244252f690fbcfef9b017a8a",
    ("3x2x2-p4", "Rw"): "ada464ef4283bbc096c1db3bc64a8151c1e60e4044fda643595b8ccd73fc8cab",
}


@pytest.mark.parametrize("name", ["4x3x3-p2", "3x2x2-p4"])
def test_key_0_assembles_the_former_values(pa, name):
    import hashlib
    c = get_mat(pa, name, 0)
    for m in ("K", "Krhs", "Rw"):
        h = hashlib.sha256(np.ascontiguousarray(c["csr"][m][2], np.float64).tobytes()).hexdigest()
        assert h == KEY0_SHA256[(name, m)], (m, h)
