"""The analytic zeros of a 3-D box mesh's free-slip K on the device
(kle_assemble.hip box_zero_entry, tuning asm_box_zeros; the rule is stated
again, and checked on the CPU oracle's K, in tests/test_box_zero_rule.py).

a. Assembly, on the smallest meshes that reach each branch ([2,2,2] ngl 3: an
   interior element face, the zeros exist only by cancellation between two
   elements; [2,3,2] ngl 3 with the faces left and down alone: free nodes on
   boundary planes; [3,2,2] ngl 5: rows of more than 64 stored blocks;
   [3,2,2] ngl 3 on an offset box of non-cubic cells; [1,1,1] ngl 3: one free
   node (every row of one stored block, formed by the gather: no brick; with
   spmv_brick_singles 0 the plan's host check refuses that lattice, asserted);
   [2,1,1] ngl 7; [3,2,2] ngl 5 and the left/down mesh again with
   spmv_brick_singles 0 (one-block rows as items of compact bricks); two z slabs of [2,2,4] ngl 4: the slab's end planes
   are not boundary planes): the exported K holds +0.0 at every free-free
   entry under the rule; every other entry, and the pattern, equals bit for
   bit the export of an assembly with asm_box_zeros 0 (whose entries under the
   rule are rounding noise: <= 1e-13 max|K|, as the CPU test bounds them);
   K = K^T bit for bit; Krhs and Rw are the same bits for both values.  A 2-D
   mesh's K is the same bits for both values.

b. The brick product of the K that carries the zeros multiplies by what K
   exports: every input of sym_ref.inputs (uniform, ramp, spike,
   sign-adversarial, subnormal, every comb) obeys the inequality of
   tests/test_gpu_sym_ref.py against the longdouble product of the exported
   CSR, with the allowance of the planned bricks; Dirichlet rows return x bit
   for bit; two runs are bit-identical.

c. The compact brick stream (spmv_brick_compact, kle_brick.hpp): it is chosen
   exactly where K carries the zeros (getSymmetricBricks()["compact"]; a K
   assembled with asm_box_zeros 0 keeps the full stream), leaves out exactly
   the rule's entries of the rows the bricks hold, and spmvBytes falls by 8 B
   for each; the products of (b) run on it; with spmv_brick_compact 0 and 1
   y is the same bits for NaN, +-inf and near-overflow x, and the export, the
   diagonal and the aij copy's product are the same bits; diagonalScale and
   a product stay inside the inequality; after K += (a K with noise there)
   the check refuses the compact stream and the product multiplies by what K
   exports; the bench's KSP (single-reduction CG, Jacobi, gather separate and
   folded) meets the longdouble PCG over 12 iterates; two z slabs take the
   compact stream and multiply by what they export.
"""
import os

import numpy as np
import pytest

import sym_ref as S
from test_box_zero_rule import lattice, rule_mask

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

UNIT = ([0, 0, 0], [1, 1, 1])
OFFSET = ([0.3, -1.0, 2.0], [1.7, 0.5, 2.9])
# name -> (nelem, ngl, Dirichlet faces (None: all), box, tunings of the brick storage)
MESHES = {
    "element-face": ([2, 2, 2], 3, None, UNIT, {}),
    "left-down": ([2, 3, 2], 3, ("left", "down"), UNIT, {}),
    "passes": ([3, 2, 2], 5, None, UNIT, {}),
    "offset-box": ([3, 2, 2], 3, None, OFFSET, {}),
    "one-free-node": ([1, 1, 1], 3, None, UNIT, {}),  # (every row of one stored block: formed by the gather)
    "rounds4": ([2, 1, 1], 7, None, UNIT, {"spmv_brick_rounds": 4}),
    # the one-block rows (every Dirichlet row, the far-corner free row) as items of compact bricks: 3, 5 or 9 doubles
    "passes-singles0": ([3, 2, 2], 5, None, UNIT, {"spmv_brick_singles": 0}),
    "left-down-singles0": ([2, 3, 2], 3, ("left", "down"), UNIT, {"spmv_brick_singles": 0}),
}
NOISE = 1e-13  # (tests/test_box_zero_rule.py)


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _assemble(pa, nelem, ngl, faces, box, zeros):
    """(dom, mat) assembled with asm_box_zeros = zeros (read at assembly)."""
    from pynama_amd.runtime import get_tuning, set_tuning
    dim = len(nelem)
    if faces is None:
        bc = {"custom-func": {"name": "taylor_green3d" if dim == 3 else "taylor_green"}}
    else:
        bc = {"free-slip": {f: {"velocity": [1, 0, 0], "vorticity": [0, 0, 0]} for f in faces}}
    cfg = {"domain": {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": box[0][:dim], "upper": box[1][:dim]}},
           "boundary-conditions": bc}
    keep = get_tuning("asm_box_zeros")
    set_tuning("asm_box_zeros", zeros)
    try:
        dom = pa.Domain()
        dom.configure(cfg)
        dom.setUp()
        mat = pa.MatFS()
        mat.setDomain(dom)
        mat.build(buildOperators=False)
    finally:
        set_tuning("asm_box_zeros", keep)
    return dom, mat


_cases = {}


def get_case(pa, name):
    """Both assemblies of a mesh and their exports: built once, left unchanged."""
    if name not in _cases:
        nelem, ngl, faces, box, _ = MESHES[name]
        dom, mat = _assemble(pa, nelem, ngl, faces, box, 1)
        _, mat0 = _assemble(pa, nelem, ngl, faces, box, 0)
        flag = np.zeros(dom.getNumOfNodes(), bool)
        flag[sorted(dom.getNodesDirichlet())] = True
        _cases[name] = dict(mat=mat, L=lattice(nelem, ngl), flag=flag,
                            csr={m: tuple(getattr(mat, m).getValuesCSR()) for m in ("K", "Krhs", "Rw")},
                            csr0={m: tuple(getattr(mat0, m).getValuesCSR()) for m in ("K", "Krhs", "Rw")})
    return _cases[name]


def check_zeros(L, flag, row0, csr, csr0):
    """The assertions of (a) on the rows [row0, row0 + m) of K: csr with the
    zeros, csr0 without.  Returns the count of entries under the rule."""
    (ip, ix, d), (ip0, ix0, d0) = csr, csr0
    np.testing.assert_array_equal(ip, ip0)
    np.testing.assert_array_equal(ix, ix0)
    rows = row0 + np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    cols = np.asarray(ix, np.int64)
    z = rule_mask(rows, cols, L) & ~flag[rows // 3] & ~flag[cols // 3]
    assert z.any()
    assert not _bits(d[z]).any()  # (+0.0: no bit set)
    np.testing.assert_array_equal(_bits(d[~z]), _bits(d0[~z]))
    kmax = np.abs(d0).max()
    assert np.abs(d0[z]).max() <= NOISE * kmax  # (what was dropped was rounding noise)
    return int(z.sum())


@pytest.mark.parametrize("name", list(MESHES))
def test_assembly_stores_the_rule_entries_as_zero(pa, name):
    c = get_case(pa, name)
    n = check_zeros(c["L"], c["flag"], 0, c["csr"]["K"], c["csr0"]["K"])
    A = S.as_csr(*c["csr"]["K"])
    assert S.is_symmetric(A), S.asymmetry(A)
    for m in ("Krhs", "Rw"):
        for a, b in zip(c["csr"][m], c["csr0"][m]):
            np.testing.assert_array_equal(_bits(a) if a.dtype == np.float64 else a,
                                          _bits(b) if b.dtype == np.float64 else b)
    print(f"BOXZEROS {name}: {n} of {len(c['csr']['K'][2])} stored entries under the rule")


def test_2d_mesh_is_untouched(pa):
    """The rule has been checked for the 3-D K alone: a 2-D K is the same bits."""
    out = []
    for zeros in (1, 0):
        _, mat = _assemble(pa, [3, 2], 4, None, UNIT, zeros)
        out.append(mat.K.getValuesCSR())
    for a, b in zip(*out):
        np.testing.assert_array_equal(_bits(a) if a.dtype == np.float64 else a,
                                      _bits(b) if b.dtype == np.float64 else b)


@pytest.mark.parametrize("name", list(MESHES))
def test_brick_product_multiplies_by_the_exported_matrix(pa, name):
    import test_gpu_sym_ref as T
    c = get_case(pa, name)
    nelem, ngl, _, _, tunings = MESHES[name]
    K = c["mat"].K
    A = S.as_csr(*c["csr"]["K"])
    assert S.is_symmetric(A)
    xs = S.inputs(A, c["L"], ngl - 1)
    ident = S.identity_rows(A)
    cc = dict(A=A, apriori={}, brick={})
    with bricks(name, K, 1):
        assert K.isSymmetricStorage()
        assert K.spmvKernel().startswith("k_nb_spmv_sym_brick"), K.spmvKernel()
        info = K.getSymmetricBricks()
        assert (info is None) == (name == "one-free-node")
        assert info is None or info["compact"] is True
        x = K.createVecRight()
        bad = []
        for nm, xa in xs.items():
            ref, den = S.reference(A, xa)
            rest = S.restatement(A, xa, ref, den)
            x.setArray(xa)
            y = (K * x).getArray().copy()
            np.testing.assert_array_equal((K * x).getArray(), y)
            assert np.array_equal(y[ident], xa[ident]), (nm, "identity rows")
            dev, used, aused, ok = T.check_product(y, ref, den, rest, T.allowance(cc, "bricks", nm, xa))
            if not nm.startswith("comb"):
                print(f"BOXZEROS {name} input={nm} restatement={rest / S.U:.3g}u device={dev / S.U:.3g}u "
                      f"tol_used={used:.3f} allowance_used={aused:.3f}")
            if not ok:
                bad.append((nm, used))
        assert not bad, bad


# ------------------------------------------------ the compact brick stream
class bricks:
    """K of a case on bricks with the mesh's tunings and spmv_brick_compact =
    compact; on exit every tuning as it was and K in full storage."""

    def __init__(self, name, K, compact=1):
        self.K = K
        self.tunings = dict(MESHES[name][4], spmv_brick_compact=compact)

    def __enter__(self):
        from pynama_amd.runtime import get_tuning, set_tuning
        self.keep = {k: get_tuning(k) for k in self.tunings}
        for k, v in self.tunings.items():
            set_tuning(k, v)
        self.K.setOption(self.K.Option.SPD, True)
        return self.K

    def __exit__(self, *exc):
        from pynama_amd.runtime import set_tuning
        for k, v in self.keep.items():
            set_tuning(k, v)
        self.K.setOption(self.K.Option.SPD, False)
        return False


def stream_rule_entries(c, singles):
    """The rule's entries in what the bricks stream: the stored triangle
    (blocks j >= i, whole) of the rows the bricks hold.  spmv_brick_singles 1:
    every row with more than one stored block (a row of one stored block is
    formed by the gather from its 9 doubles), so only free-free blocks.  0:
    every row, the Dirichlet rows' identity blocks too -- their off-diagonal
    zeros fall under the lattice rule like any block's."""
    ip, ix, d = c["csr"]["K"]
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    cols = np.asarray(ix, np.int64)
    up = cols // 3 >= rows // 3
    first = up & (rows % 3 == 0) & (cols % 3 == 0)  # one entry per stored block
    blocks = np.bincount(rows[first] // 3, minlength=len(c["flag"]))
    z = rule_mask(rows, cols, c["L"])
    if not singles:
        # (a Dirichlet row exports its diagonal alone; its stored identity
        # block loses the off-diagonal pairs with a coordinate off the
        # boundary planes: 2 entries per pair)
        L = np.array(c["L"])
        dn = np.flatnonzero(c["flag"])
        nb = np.stack([dn % L[0], (dn // L[0]) % L[1], dn // (L[0] * L[1])], axis=-1)
        nb = (nb > 0) & (nb < L - 1)
        ident = 2 * int(((nb[:, 0] | nb[:, 1]).sum() + (nb[:, 0] | nb[:, 2]).sum() + (nb[:, 1] | nb[:, 2]).sum()))
        free = ~c["flag"][rows // 3] & ~c["flag"][cols // 3]
        return int((z & up & free).sum()) + ident
    z &= ~c["flag"][rows // 3] & ~c["flag"][cols // 3]
    return int((z & up & (blocks[rows // 3] > 1)).sum())


@pytest.mark.parametrize("name", list(MESHES))
def test_compact_stream_is_chosen_and_counted(pa, name):
    """With the zeros in K the bricks take the compact stream; it leaves out
    exactly the rule's entries of the rows it holds, and spmvBytes falls by
    8 B for each (spmvBytes counts entries, not the rows' padding to 16
    doubles, so the difference is exact: padding bound 0).  The K assembled
    with asm_box_zeros 0 fails the device check and keeps the full stream."""
    c = get_case(pa, name)
    K = c["mat"].K
    singles = MESHES[name][4].get("spmv_brick_singles", 1)
    want = stream_rule_entries(c, singles)
    with bricks(name, K, 0):
        assert K.spmvKernel().startswith("k_nb_spmv_sym_brick"), K.spmvKernel()
        info0, bytes0 = K.getSymmetricBricks(), K.spmvBytes()
    with bricks(name, K, 1):
        assert K.spmvKernel().startswith("k_nb_spmv_sym_brick"), K.spmvKernel()
        info1, bytes1 = K.getSymmetricBricks(), K.spmvBytes()
    if info0 is None:  # (no brick at all: every row of one stored block, formed by the gather)
        assert name == "one-free-node" and info1 is None and want == 0 and bytes0 == bytes1
        return
    if not singles:
        assert want > stream_rule_entries(c, 1)  # (one-block rows do lose entries)
    assert info0["compact"] is False and info0["dropped_entries"] == 0
    assert info1["compact"] is True
    assert info1["dropped_entries"] == want
    assert bytes0 - bytes1 == 8.0 * want
    print(f"BOXZEROS {name}: compact stream leaves out {want} entries, spmvBytes {bytes0:.0f} -> {bytes1:.0f}")


@pytest.mark.parametrize("compact", [0, 1])
def test_one_block_lattice_without_singles_is_refused(pa, compact):
    """[1,1,1] ngl 3 with spmv_brick_singles 0 -- 27 rows of one stored block
    on as many CUs as the device has: the planner leaves bricks without rows
    and the plan's host check refuses it ("brick plan: ..."), with and
    without the compact stream, so no kernel is launched on it and K keeps
    the full storage, whose product is the exported matrix's."""
    from pynama_amd._lib import call
    from pynama_amd.runtime import get_tuning, set_tuning
    c = get_case(pa, "one-free-node")
    K = c["mat"].K
    keep = {k: get_tuning(k) for k in ("spmv_brick_singles", "spmv_brick_compact")}
    try:
        set_tuning("spmv_brick_singles", 0)
        set_tuning("spmv_brick_compact", compact)
        with pytest.raises(pa.Error, match="brick plan"):
            call("kle_mat_set_symmetric", K._h, 1)
        assert not K.isSymmetricStorage() and K.getSymmetricBricks() is None
        A = S.as_csr(*c["csr"]["K"])
        xa = S.inputs(A, c["L"], 2)["uniform"]
        x = K.createVecRight()
        x.setArray(xa)
        ref, den = S.reference(A, xa)
        assert S.scaled_err((K * x).getArray(), ref, den) <= 16 * max(S.restatement(A, xa, ref, den), S.U)
    finally:
        for k, v in keep.items():
            set_tuning(k, v)
        K.setOption(K.Option.SPD, False)


@pytest.mark.parametrize("name", list(MESHES))
def test_noise_matrix_keeps_the_full_stream(pa, name):
    nelem, ngl, faces, box, _ = MESHES[name]
    _, mat0 = _assemble(pa, nelem, ngl, faces, box, 0)
    K0 = mat0.K
    with bricks(name, K0, 1):
        info = K0.getSymmetricBricks()
        assert (info is None) == (name == "one-free-node")
        assert info is None or info["compact"] is False


@pytest.mark.parametrize("name", list(MESHES))
def test_compact_and_full_stream_agree(pa, name):
    """Non-finite x gives what the full stream gives; the export, the
    diagonal and the aij copy's product are the same bits; diagonalScale
    followed by a product stays inside the inequality."""
    import test_gpu_sym_ref as T
    c = get_case(pa, name)
    K = c["mat"].K
    A = S.as_csr(*c["csr"]["K"])
    n = A.n
    base = np.random.default_rng(9).uniform(-1, 1, n)
    bad = {}
    for nm, v in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf)):
        bad[nm] = base.copy()
        bad[nm][n // 2] = v
    bad["huge"] = base * 1e305
    out = {}
    for compact in (0, 1):
        with bricks(name, K, compact):
            x = K.createVecRight()
            ys = {}
            with np.errstate(all="ignore"):
                for nm, xa in bad.items():
                    x.setArray(xa)
                    ys[nm] = (K * x).getArray().copy()
            x.setArray(base)
            B = K.convert("aij")
            xb = B.createVecRight()
            xb.setArray(base)
            yb = B.createVecLeft()
            B.mult(xb, yb)
            out[compact] = (ys, K.getValuesCSR(), K.getDiagonal().getArray().copy(), yb.getArray().copy())
    for nm in bad:
        # (the same arithmetic on the same values -- the entries left out enter
        # as 0.0 -- so the same bits, NaN for NaN)
        np.testing.assert_array_equal(out[0][0][nm], out[1][0][nm], err_msg=nm)
    for a, b in zip(out[0][1], out[1][1]):
        np.testing.assert_array_equal(_bits(a) if a.dtype == np.float64 else a,
                                      _bits(b) if b.dtype == np.float64 else b)
    np.testing.assert_array_equal(_bits(out[0][2]), _bits(out[1][2]))
    np.testing.assert_array_equal(_bits(out[0][3]), _bits(out[1][3]))
    # diagonalScale (powers of two: the zeros stay zeros, K stays symmetric), then the compact product
    D = K.duplicate(copy=True)
    sv = 2.0 ** np.random.default_rng(10).integers(-3, 4, n // 3).repeat(3)
    lv, rv = D.createVecLeft(), D.createVecRight()
    lv.setArray(sv)
    rv.setArray(sv)
    D.diagonalScale(L=lv, R=rv)
    E = S.as_csr(*D.getValuesCSR())
    assert S.is_symmetric(E)
    with bricks(name, D, 1):
        info = D.getSymmetricBricks()
        assert (info is None) == (name == "one-free-node")
        assert info is None or info["compact"] is True
        x = D.createVecRight()
        x.setArray(base)
        y = (D * x).getArray().copy()
    ref, den = S.reference(E, base)
    rest = S.restatement(E, base, ref, den)
    _, used, _, ok = T.check_product(y, ref, den, rest, T.allowance(dict(A=E, apriori={}, brick={}), "bricks", "u", base))
    assert ok, used


def test_fallback_when_rule_entries_become_nonzero(pa):
    """Through the Mat surface only axpy can make an entry under the rule
    nonzero on this matrix (setValues is refused on a node-block matrix, a
    shift touches the diagonal alone): K += the K assembled with
    asm_box_zeros 0 puts rounding noise there.  The device check then refuses
    the compact stream and the product multiplies by what K now exports."""
    import test_gpu_sym_ref as T
    name = "passes"
    nelem, ngl, faces, box, _ = MESHES[name]
    _, mat = _assemble(pa, nelem, ngl, faces, box, 1)
    _, mat0 = _assemble(pa, nelem, ngl, faces, box, 0)
    c = get_case(pa, name)
    K = mat.K
    with pytest.raises(pa.Error):
        K.setValues([4], [3], [[1.0]])
    with bricks(name, K, 1):
        assert K.getSymmetricBricks()["compact"] is True
        K.axpy(1.0, mat0.K)  # (drops the symmetric storage)
        K.assemble()
        assert not K.isSymmetricStorage()
    E = S.as_csr(*K.getValuesCSR())
    assert S.is_symmetric(E)
    ip, ix, d = c["csr"]["K"]
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    cols = np.asarray(ix, np.int64)
    z = rule_mask(rows, cols, c["L"]) & ~c["flag"][rows // 3] & ~c["flag"][cols // 3]
    assert np.count_nonzero(E.data[z]) > 0
    with bricks(name, K, 1):
        assert K.spmvKernel().startswith("k_nb_spmv_sym_brick"), K.spmvKernel()
        assert K.getSymmetricBricks()["compact"] is False
        x = K.createVecRight()
        for nm, xa in S.inputs(E, c["L"], ngl - 1).items():
            ref, den = S.reference(E, xa)
            rest = S.restatement(E, xa, ref, den)
            x.setArray(xa)
            y = (K * x).getArray().copy()
            _, used, _, ok = T.check_product(y, ref, den, rest,
                                             T.allowance(dict(A=E, apriori={}, brick={}), "bricks", nm, xa))
            assert ok, (nm, used)


@pytest.mark.parametrize("fold", [0, 2])
def test_cg_on_the_compact_stream_matches_reference(pa, fold):
    """The single-reduction CG with Jacobi (the bench's KSP), its gather
    separate (ksp_sr_gather 0) and folded into the update (2), on [3,2,2] ngl
    5: iterates k = 1 .. 12 against the longdouble PCG of tests/krylov_ref.py
    within 16 x the fp64 restatement's error, as
    test_gpu_sym_ref.test_brick_cg_iterates_match_reference asserts."""
    import krylov_ref as R
    import test_gpu_sym_ref as T
    name = "passes"
    c = get_case(pa, name)
    K = c["mat"].K
    cs = dict(A=S.as_csr(*c["csr"]["K"]))
    g = T.cg_case(cs, ("boxzeros", name), "jacobi")
    ex, er = g["err"]["sr"]
    with bricks(name, K, 1):
        assert K.getSymmetricBricks()["compact"] is True
        xs, rns = T.cg_history(pa, K, g, "sr", "jacobi", ("ksp_sr_gather", fold),
                               "k_nb_spmv_sym_brick<16,true,true>" if fold else None)
    dx, dr = T.history_errors(xs, rns, g)
    print(f"BOXZEROS-CG ksp_sr_gather={fold} restatement_x={ex:.2e} device_x={dx:.2e} restatement_r={er:.2e} "
          f"device_r={dr:.2e}")
    assert dx <= 16 * max(ex, R.FLOOR), (dx, ex)
    assert dr <= 16 * max(er, R.FLOOR), (dr, er)


# ------------------------------------------------------------- two z slabs
def _slab_worker(rank, size, port, nelem, ngl, q):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), KLE_TRANSPORT="host", RANK=str(rank),
                      WORLD_SIZE=str(size))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=size)
    try:
        import pynama_amd as pa
        out = {"rank": rank}
        for zeros in (1, 0):
            _, mat = _assemble(pa, nelem, ngl, None, UNIT, zeros)
            out[zeros] = {m: tuple(getattr(mat, m).getValuesCSR()) for m in ("K", "Krhs", "Rw")}
            out["lo"] = mat.K.getOwnershipRange()[0]
            # the slab's bricks (symmetric storage is collective: both ranks take it)
            K = mat.K
            K.setOption(K.Option.SPD, True)
            xv = K.createVecRight()
            xv.setArray(np.sin(np.arange(*K.getOwnershipRange(), dtype=np.float64)))
            out[("bricks", zeros)] = (K.spmvKernel(), K.getSymmetricBricks(), (K * xv).getArray().copy())
        q.put(out)
    except Exception:  # report instead of hanging the peer
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc()})
    finally:
        dist.destroy_process_group()


def test_two_z_slabs_use_the_global_lattice():
    """[2,2,4] ngl 4 on 2 ranks: the slab interface (global z plane 6 of 13) is
    not a boundary plane, so pairs of nodes in it lose their entries as every
    interior plane's do; each rank's rows against the rule on the global
    lattice."""
    import torch.multiprocessing as mp
    from test_gpu_multirank import _collect, _free_port
    nelem, ngl, size = [2, 2, 4], 4, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    res = _collect([ctx.Process(target=_slab_worker, args=(r, size, port, nelem, ngl, q)) for r in range(size)], q,
                   size)
    L = lattice(nelem, ngl)
    c = np.arange(L[0] * L[1] * L[2])
    coords = np.stack([c % L[0], (c // L[0]) % L[1], c // (L[0] * L[1])], axis=-1)
    flag = ((coords == 0) | (coords == np.array(L) - 1)).any(axis=1)
    zplane = (L[2] - 1) // 2
    seen = 0
    for r in sorted(res, key=lambda r: r["rank"]):
        check_zeros(L, flag, r["lo"], r[1]["K"], r[0]["K"])
        for m in ("Krhs", "Rw"):
            for a, b in zip(r[1][m], r[0][m]):
                np.testing.assert_array_equal(_bits(a) if a.dtype == np.float64 else a,
                                              _bits(b) if b.dtype == np.float64 else b)
        # the (x, z) entries between two free nodes of the interface plane
        ip, ix, d = r[1]["K"]
        rows = r["lo"] + np.repeat(np.arange(len(ip) - 1), np.diff(ip))
        cols = np.asarray(ix, np.int64)
        on = (coords[rows // 3, 2] == zplane) & (coords[cols // 3, 2] == zplane) & ~flag[rows // 3] & ~flag[cols // 3]
        xz = on & (rows % 3 == 0) & (cols % 3 == 2)
        seen += int(xz.sum())
        assert not _bits(d[xz]).any()
    assert seen > 0
    # the slabs' bricks take the compact stream where K carries the zeros, and
    # multiply by what K exports (the longdouble product of the two ranks' rows)
    res = sorted(res, key=lambda r: r["rank"])
    ip = np.concatenate([[0]] + [r[1]["K"][0][1:] + sum(len(q[1]["K"][2]) for q in res[:k]) for k, r in enumerate(res)])
    A = S.as_csr(ip, np.concatenate([r[1]["K"][1] for r in res]), np.concatenate([r[1]["K"][2] for r in res]))
    xa = np.sin(np.arange(A.m, dtype=np.float64))
    ref, den = S.reference(A, xa)
    rest = S.restatement(A, xa, ref, den)
    import test_gpu_sym_ref as T
    allow = T.allowance(dict(A=A, apriori={}, brick={}), "bricks", "sin", xa)
    for r in res:
        kern, info, y = r[("bricks", 1)]
        assert kern.startswith("k_nb_spmv_sym_brick<"), kern
        assert info["compact"] is True and info["dropped_entries"] > 0
        assert r[("bricks", 0)][1]["compact"] is False
        sl = slice(r["lo"], r["lo"] + len(y))
        _, used, _, ok = T.check_product(y, ref[sl], den[sl], rest, allow[sl])
        assert ok, (r["rank"], used)
