"""The symmetric-storage SpMV kernels and the CG that runs on them, row by row
against longdouble references (tests/sym_ref.py, tests/krylov_ref.py).  One
rank, 3-D; tests/test_gpu_sym_ranks_ref.py holds the same on several ranks.

a. K x in every storage -- full, box bricks (planned, one brick, a forced
   split, one-block rows as brick items, unpaired rows, the gather with 1, 2
   and 4 waves per slice), 128-row tiles, graph bricks, 64-row groups --
   against ref = K x in longdouble on the exported CSR (asserted symmetric
   bit for bit), component-wise:

       |y_i - ref_i| <= 16 max(restatement, u) den_i + allowance_i

   den = |K||x|, restatement = the same scaled error of the fp64 CSR product,
   u = 2^-53.  allowance_i is 0 in full storage; nT_i q for one brick, q
   restated from k_brick_bound (sym_ref.brick_quantum: nT_i q/2 is the worst
   case, the factor 2 covers the device's bound landing on the other side of
   a power of two); nT_i q/2 with the a-priori q <= 2^-57 ||K||inf ||x||inf
   (sym_ref.apriori_quantum, derived from the kernels' bounds) everywhere
   else.  Inputs: uniform, a 6-decade ramp, a 1e8 spike, the sign pattern
   that maximises one region sum, subnormal x, combs (6 with random offsets
   and components, every offset on the lattices of order <= 2; every row a
   single product K_ij x_j: a block missing or doubled at a brick, region,
   tile or group edge is an O(1) error), x near overflow (never a finite
   wrong value), and the Dirichlet rows bit for bit.  Each case prints the
   restatement's error, the device's, and the share of the tolerance and of
   the allowance it used.

b. CG through the bricks: x_k and ||r_k|| for k = 1 .. 12 of the classic,
   single-reduction and pipelined variants, PC none and Jacobi, with the
   product's gather folded into the update (k_sr_iter_g, k_pipe_iter_g) and
   separate, against krylov_ref.pcg_reference on the exported CSR with the
   tolerances of tests/test_gpu_krylov.py (16 x the fp64 restatement's error
   of the same recurrence, floor 16 x 2.2e-16, residuals above 1e-6 ||b||).
"""
import numpy as np
import pytest

import krylov_ref as R
import sym_ref as S

pytestmark = pytest.mark.gpu

LD = np.longdouble
BOX_MESHES = (([3, 2, 2], 5), ([4, 3, 3], 5), ([7, 5, 4], 3), ([6, 5, 3], 2), ([3, 3, 2], 7), ([6, 5, 4], 5))
ONE_BRICK_NODES = 2873  # [4,3,3] ngl 5: the largest of these lattices whose region fits one brick's LDS

# storage -> (tunings, kernel prefix); every tuning is restored afterwards
BOX_STORAGES = {
    "full": ({}, None),
    "bricks": ({}, "k_nb_spmv_sym_brick"),
    "one_brick": ({"spmv_brick_max": 1}, "k_nb_spmv_sym_brick"),
    "rounds4": ({"spmv_brick_rounds": 4}, "k_nb_spmv_sym_brick"),
    "singles0": ({"spmv_brick_singles": 0}, "k_nb_spmv_sym_brick"),
    "pair0": ({"spmv_brick_pair": 0}, "k_nb_spmv_sym_brick"),
    "wps1": ({"spmv_gather_wps": 1}, "k_nb_spmv_sym_brick"),
    "wps2": ({"spmv_gather_wps": 2}, "k_nb_spmv_sym_brick"),
    "wps4": ({"spmv_gather_wps": 4}, "k_nb_spmv_sym_brick"),
    "tiles": ({"spmv_sym_brick": 0}, "k_nb_spmv_sym_xl"),
}
GRAPH_STORAGES = {
    "full": ({}, None),
    "gbricks": ({}, "k_nb_spmv_gsym_brick"),
    "groups": ({"spmv_gsym_brick": 0}, "k_nb_spmv_gsym<"),
}


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


@pytest.fixture(scope="module")
def mesh_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("symref")


_cases = {}


def _build(pa, cfg):
    dom = pa.Domain()
    dom.configure(cfg)
    dom.setUp()
    mat = pa.MatFS()
    mat.setDomain(dom)
    mat.build(buildOperators=False)
    return dom, mat


def get_case(pa, kind, nelem, ngl, mesh_dir=None):
    """The matrix of a mesh on the device, its exported CSR, the inputs and
    their longdouble references -- built once per mesh, left unchanged."""
    key = (kind, tuple(nelem), ngl)
    if key in _cases:
        return _cases[key]
    bc = {"custom-func": {"name": "taylor_green3d"}}
    if kind == "box":
        dom, mat = _build(pa, {"domain": {"ngl": ngl, "box-mesh": {"nelem": nelem, "lower": [0, 0, 0],
                                                                   "upper": [1, 1, 1]}},
                               "boundary-conditions": bc})
        dims, P = [n * (ngl - 1) + 1 for n in nelem], ngl - 1
    else:
        from pynama_amd.meshgen import perturbed_box, write_gmsh
        V, Cc, F, T = perturbed_box(3, nelem, seed=5)
        path = mesh_dir / ("g" + "_".join(map(str, nelem)) + f"_{ngl}.msh")
        write_gmsh(path, 3, V, Cc, F, T)
        dom, mat = _build(pa, {"domain": {"ngl": ngl, "gmsh-file": str(path)}, "boundary-conditions": bc})
        dims = P = None
    K = mat.K
    assert K.isStructured() == (kind == "box")
    A = S.as_csr(*K.getValuesCSR())
    xs = S.inputs(A, dims, P)
    refs = {}
    for nm, x in xs.items():
        ref, den = S.reference(A, x)
        refs[nm] = (ref, den, S.restatement(A, x, ref, den))
        if nm.startswith("comb"):
            assert S.terms_per_row(A, x).max() == 1 and np.count_nonzero(x) >= 1, nm
    big = xs["uniform"] * 1e305
    c = dict(dom=dom, mat=mat, K=K, A=A, xs=xs, refs=refs, ident=S.identity_rows(A), big=big,
             big_ref=S.reference(A, big), symmetric=S.is_symmetric(A), asym=S.asymmetry(A), apriori={}, brick={})
    _cases[key] = c
    return c


def require_symmetric(c):
    """The precondition of every test here: the exported CSR equals its
    transpose bit for bit (the symmetric storages keep one triangle)."""
    assert c["symmetric"], f"the exported CSR is not exactly symmetric: {c['asym']}"


class storage:
    """K in one of the storages: the tunings set, the storage planned anew;
    on exit every tuning as it was and K in its default symmetric storage."""

    def __init__(self, K, table, name):
        self.K, self.name = K, name
        self.tunings, self.prefix = table[name]

    def __enter__(self):
        from pynama_amd.runtime import get_tuning, set_tuning
        K = self.K
        self.keep = {k: get_tuning(k) for k in self.tunings}
        try:
            for k, v in self.tunings.items():
                set_tuning(k, v)
            K.setOption(K.Option.SPD, self.name != "full")
            if self.name == "full":
                assert not K.isSymmetricStorage()
            else:
                assert K.isSymmetricStorage()
                assert K.spmvKernel().startswith(self.prefix), (self.name, K.spmvKernel())
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        from pynama_amd.runtime import set_tuning
        for k, v in self.keep.items():
            set_tuning(k, v)
        self.K.setOption(self.K.Option.SPD, True)
        return False


def allowance(c, storage_name, nm, x):
    """allowance_i of the module docstring (derived from the code, not measured)."""
    A = c["A"]
    if storage_name == "full":
        return np.zeros(A.m, LD)
    if storage_name == "one_brick":
        if nm not in c["brick"]:
            c["brick"][nm] = S.brick_quantum(A, x)
        q, nT = c["brick"][nm]
        return nT * q
    if nm not in c["apriori"]:
        c["apriori"][nm] = S.apriori_quantum(A, x)
    q, nT = c["apriori"][nm]
    return nT * q / 2


def check_product(y, ref, den, rest, allow):
    """The inequality of the module docstring.  Returns (device error,
    share of the tolerance used, share of the allowance used, holds); rows
    without a nonzero product must be exactly 0."""
    dev = S.scaled_err(y, ref, den)
    err = np.abs(y.astype(LD) - ref)
    fp = 16 * LD(max(rest, S.U)) * den
    tol = fp + allow
    on = tol > 0
    used = float((err[on] / tol[on]).max()) if on.any() else 0.0
    over = err - fp
    oa = allow > 0
    aused = float(max((over[oa] / allow[oa]).max(), 0)) if oa.any() else 0.0
    return dev, used, aused, bool(np.all(err <= tol))


def run_products(c, tag, storage_name):
    K, A = c["K"], c["A"]
    x = K.createVecRight()
    bad = []
    comb = [0.0, 0.0, 0.0, 0.0]
    for nm, xa in c["xs"].items():
        ref, den, rest = c["refs"][nm]
        x.setArray(xa)
        y = (K * x).getArray().copy()
        allow = allowance(c, storage_name, nm, xa)
        dev, used, aused, ok = check_product(y, ref, den, rest, allow)
        if nm.startswith("comb"):
            comb = [max(a, b) for a, b in zip(comb, (rest, dev, used, aused))]
        else:
            extra = ""
            if nm in ("ramp", "spike"):
                on = den > 0
                extra = f" rows_allowance_larger={float(np.mean(allow[on] > (LD(S.U) * den)[on])):.2f}"
            print(f"SYMREF {tag} storage={storage_name} input={nm} restatement={rest / S.U:.3g}u "
                  f"device={dev / S.U:.3g}u tol_used={used:.3f} allowance_used={aused:.3f}{extra}")
            # Dirichlet rows: x_i bit for bit
            assert np.array_equal(y[c["ident"]], xa[c["ident"]]), (nm, "identity rows")
        if not ok:
            bad.append((nm, used))
    ncomb = sum(nm.startswith("comb") for nm in c["xs"])
    print(f"SYMREF {tag} storage={storage_name} input=comb(x{ncomb}) restatement={comb[0] / S.U:.3g}u "
          f"device={comb[1] / S.U:.3g}u tol_used={comb[2]:.3f} allowance_used={comb[3]:.3f}")
    # x near overflow: within the tolerance where the reference is finite in
    # fp64, non-finite where it is not -- never a finite wrong value
    xa = c["big"]
    ref, den = c["big_ref"]
    x.setArray(xa)
    with np.errstate(all="ignore"):
        y = (K * x).getArray().copy()
        fin = np.abs(ref) < LD(S.DBL_MAX)
        allow = allowance(c, storage_name, "big", xa)
        rest = c["refs"]["uniform"][2]  # (the same x but for the scale)
        tol = 16 * LD(max(rest, S.U)) * den + allow
        err = np.abs(y[fin].astype(LD) - ref[fin])
        okf = np.isfinite(y[fin]) & (err <= tol[fin])
    print(f"SYMREF {tag} storage={storage_name} input=near_overflow rows_past_dbl_max={int((~fin).sum())} "
          f"tol_used={float(np.nanmax(err / tol[fin])):.3f} max|ref|={float(np.abs(ref).max()):.3g}")
    if not okf.all():
        bad.append(("near_overflow finite rows", int((~okf).sum())))
    if not np.all(~np.isfinite(y[~fin])):
        bad.append(("near_overflow: finite values past DBL_MAX", int(np.isfinite(y[~fin]).sum())))
    assert np.array_equal(y[c["ident"]], xa[c["ident"]])
    assert not bad, (tag, storage_name, bad)


def box_params():
    out = []
    for nelem, ngl in BOX_MESHES:
        nodes = int(np.prod([n * (ngl - 1) + 1 for n in nelem]))
        for s in BOX_STORAGES:
            if s == "one_brick" and nodes > ONE_BRICK_NODES:
                continue
            out.append(pytest.param(nelem, ngl, s, id=f"{'x'.join(map(str, nelem))}-ngl{ngl}-{s}"))
    return out


@pytest.mark.parametrize("nelem,ngl,sname", box_params())
def test_box_spmv_rows_match_longdouble(pa, nelem, ngl, sname):
    c = get_case(pa, "box", nelem, ngl)
    require_symmetric(c)
    K = c["K"]
    with storage(K, BOX_STORAGES, sname):
        tag = f"box={'x'.join(map(str, nelem))} ngl={ngl}"
        if sname not in ("full", "tiles"):
            bricks = K.getSymmetricBricks()
            assert bricks is not None and bricks["bricks"] >= 1
            print(f"SYMREF {tag} storage={sname} bricks={bricks['bricks']} dims={bricks['dims']}")
            if sname == "one_brick":
                assert bricks["bricks"] == 1
            if sname == "rounds4":
                assert bricks["bricks"] > 1
        else:
            assert K.getSymmetricBricks() is None
        run_products(c, tag, sname)


@pytest.mark.parametrize("nelem,ngl,sname", [pytest.param(n, g, s, id=f"{'x'.join(map(str, n))}-ngl{g}-{s}")
                                            for n, g in BOX_MESHES for s in GRAPH_STORAGES])
def test_graph_spmv_rows_match_longdouble(pa, mesh_dir, nelem, ngl, sname):
    c = get_case(pa, "graph", nelem, ngl, mesh_dir)
    require_symmetric(c)
    with storage(c["K"], GRAPH_STORAGES, sname):
        run_products(c, f"gmsh={'x'.join(map(str, nelem))} ngl={ngl}", sname)


# ------------------------------------------------ b. CG through the bricks
CG_MESHES = (([4, 3, 3], 5), ([6, 5, 4], 5))
CG_ITERS = 12
# variant -> ((tuning, folded value), ...); the classic recurrence has no fold
FOLDS = {"cg": (None,), "sr": (("ksp_sr_gather", 2), ("ksp_sr_gather", 0)),
         "pipecg": (("ksp_pipe_gather", 1), ("ksp_pipe_gather", 0))}
_cg = {}


def cg_case(c, key, pc):
    """b = U(-1, 1), the reference history of 12 iterations on the exported
    CSR and, per recurrence, the fp64 restatement's error against it."""
    if (key, pc) not in _cg:
        A = c["A"]
        b = np.random.default_rng(77).uniform(-1.0, 1.0, A.m)
        xs, rns = R.pcg_reference(A, b, pc, CG_ITERS)
        assert len(xs) == CG_ITERS + 1
        bn = float(rns[0])
        err = {v: R.history_error(*f(A, b, pc, CG_ITERS), xs, rns, 1e-6 * bn) for v, f in R.RECURRENCES.items()}
        _cg[(key, pc)] = dict(b=b, xs=xs, rns=rns, bn=bn, err=err)
    return _cg[(key, pc)]


def make_ksp(pa, K, variant, pc):
    k = pa.petsc.KSP().create()
    k.setType("pipecg" if variant == "pipecg" else "cg")
    k.setCGSingleReduction(variant == "sr")
    p = pa.petsc.PC()
    p.setType(pc)
    k.setPC(p)
    k.setOperators(K)
    k.setCorrections(0)
    return k


def cg_history(pa, K, g, variant, pc, fold, expect_split):
    """x_k, ||r_k|| for k = 1 .. 12 by fixed-iteration solves; the last one
    twice (bitwise repeatable)."""
    from pynama_amd.runtime import get_tuning, set_tuning
    keep = get_tuning(fold[0]) if fold else None
    try:
        if fold:
            set_tuning(*fold)
        ksp = make_ksp(pa, K, variant, pc)
        b, x = K.createVecLeft(), K.createVecRight()
        b.setArray(g["b"])
        xs, rns = [None], [None]
        for k in range(1, CG_ITERS + 1):
            x.setArray(np.ones(len(g["b"])))  # (the solve starts from zero whatever x holds)
            ksp.setFixedIterations(k)
            ksp.solve(b, x)
            assert ksp.getIterationNumber() == k and ksp.getConvergedReason() == R.ITS_OK
            xs.append(x.getArray().copy())
            rns.append(ksp.getResidualNorm())
            if variant == "cg":
                pass  # (the classic recurrence reports no product kernel: it has no fold)
            elif expect_split is None:
                assert ksp.getProductKernel() == K.spmvKernel()
            else:
                assert ksp.getProductKernel() == expect_split, ksp.getProductKernel()
        ksp.solve(b, x)
        assert np.array_equal(x.getArray(), xs[-1]) and ksp.getResidualNorm() == rns[-1]
    finally:
        if fold:
            set_tuning(fold[0], keep)
    return xs, rns


def history_errors(xs, rns, g):
    dx = dr = 0.0
    for k in range(1, CG_ITERS + 1):
        dx = max(dx, float(np.abs(xs[k].astype(LD) - g["xs"][k]).max() / np.abs(g["xs"][k]).max()))
        if g["rns"][k] >= 1e-6 * g["bn"]:
            dr = max(dr, float(abs(LD(rns[k]) - g["rns"][k]) / g["rns"][k]))
    return dx, dr


@pytest.mark.parametrize("nelem,ngl,pc,variant", [pytest.param(n, g, pc, v, id=f"{'x'.join(map(str, n))}-{pc}-{v}")
                                                 for n, g in CG_MESHES for pc in ("none", "jacobi")
                                                 for v in ("cg", "sr", "pipecg")])
def test_brick_cg_iterates_match_reference(pa, nelem, ngl, pc, variant):
    """A wrong brick share of (A u, u) or a stale gather is an O(1) error in
    an iterate.  The folded and the separate gather each meet the reference
    and so each other (asserted directly too), each bitwise repeatable."""
    c = get_case(pa, "box", nelem, ngl)
    require_symmetric(c)
    K = c["K"]
    K.setOption(K.Option.SPD, True)
    assert K.spmvKernel().startswith("k_nb_spmv_sym_brick<"), K.spmvKernel()
    g = cg_case(c, (tuple(nelem), ngl), pc)
    ex, er = g["err"][variant]
    tolx, tolr = 16 * max(ex, R.FLOOR), 16 * max(er, R.FLOOR)
    split = {"sr": "k_nb_spmv_sym_brick<16,true,true>", "pipecg": "k_nb_spmv_sym_brick<16,true,false>"}
    hist = {}
    for fold in FOLDS[variant]:
        folded = bool(fold and fold[1])
        xs, rns = cg_history(pa, K, g, variant, pc, fold, split[variant] if folded else None)
        dx, dr = history_errors(xs, rns, g)
        print(f"SYMREF-CG box={'x'.join(map(str, nelem))} ngl={ngl} variant={variant} pc={pc} "
              f"gather={'folded' if folded else 'separate'} restatement_x={ex:.2e} device_x={dx:.2e} "
              f"restatement_r={er:.2e} device_r={dr:.2e}")
        assert dx <= tolx, (fold, dx, tolx)
        assert dr <= tolr, (fold, dr, tolr)
        hist[folded] = xs
    if len(hist) == 2:
        for k in range(1, CG_ITERS + 1):
            d = float(np.abs(hist[True][k] - hist[False][k]).max() / np.abs(g["xs"][k]).max())
            assert d <= tolx, (k, d, tolx)


def test_graph_brick_cg_iterates_match_reference(pa, mesh_dir):
    """The single-reduction CG on graph bricks.  No fold exists there: the
    split product is the box bricks' alone (spmv_can_split refuses graph
    storage), so with ksp_sr_gather 2 the solve still runs K's own product
    and its separate gather -- asserted -- and the iterates meet the
    reference with the same tolerances."""
    nelem, ngl = [4, 3, 3], 5
    c = get_case(pa, "graph", nelem, ngl, mesh_dir)
    require_symmetric(c)
    K = c["K"]
    K.setOption(K.Option.SPD, True)
    assert K.spmvKernel().startswith("k_nb_spmv_gsym_brick"), K.spmvKernel()
    for pc in ("none", "jacobi"):
        g = cg_case(c, ("graph", tuple(nelem), ngl), pc)
        ex, er = g["err"]["sr"]
        xs, rns = cg_history(pa, K, g, "sr", pc, ("ksp_sr_gather", 2), None)
        dx, dr = history_errors(xs, rns, g)
        print(f"SYMREF-CG gmsh={'x'.join(map(str, nelem))} ngl={ngl} variant=sr pc={pc} gather=separate "
              f"restatement_x={ex:.2e} device_x={dx:.2e} restatement_r={er:.2e} device_r={dr:.2e}")
        assert dx <= 16 * max(ex, R.FLOOR), (dx, ex)
        assert dr <= 16 * max(er, R.FLOOR), (dr, er)
