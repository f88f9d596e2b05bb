"""The Krylov layer (kle_ksp.hip) on generic matrices against the extended-
precision references of tests/krylov_ref.py: every iterate of the three CG
variants with PC none and Jacobi at lengths around the 256-thread block and
past the grid caps, the update kernels' knobs bit for bit, every converged
reason with the iterate it reports, GMRES(m) on a non-symmetric matrix, and
the scalar-CSR product and vector kernels all of that rests on.  One rank.

Tolerances for iterates are not fixed numbers: 16 x the error of the fp64
numpy restatement of the same recurrence against the longdouble reference
(floor 16 x 2.2e-16), in the same norm over the same iterations.  The factor
covers the device's different summation tree and FMA contraction; a dropped,
doubled or stale entry is an O(1) error in that norm.  Each case prints the
restatement's error and the device's.
"""
import math

import numpy as np
import pytest

import krylov_ref as R

pytestmark = pytest.mark.gpu

LD = np.longdouble
PCS = ("none", "jacobi")
VARIANTS = ("cg", "sr", "pipecg")
BIG = (262144 + 77, 524288 + 300)  # past the 1024- and 2048-workgroup grid caps


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


_mats = {}


def device_mat(pa, key, A):
    """createAIJ(csr=...) of a host Csr, kept per key (the long ones are 1.5 M nonzeros)."""
    if key not in _mats:
        _mats[key] = pa.petsc.Mat().createAIJ(((A.m, A.m), (A.n, A.n)), csr=A.csr)
    return _mats[key]


def vec_of(M, a, left=True):
    v = M.createVecLeft() if left else M.createVecRight()
    v.setArray(np.asarray(a, dtype=np.float64))
    return v


def make_ksp(pa, M, variant, pc, restart=None):
    k = pa.petsc.KSP().create()
    k.setType({"cg": "cg", "sr": "cg", "pipecg": "pipecg", "gmres": "gmres"}[variant])
    k.setCGSingleReduction(variant == "sr")
    p = pa.petsc.PC()
    p.setType(pc)
    k.setPC(p)
    if restart is not None:
        k.setGMRESRestart(restart)
    k.setOperators(M)
    k.setCorrections(0)
    return k


def xerr(x, ref):
    """max|x - ref| / max|ref|: one wrong entry anywhere shows."""
    return float(np.abs(x.astype(LD) - ref).max() / np.abs(ref).max())


def cg_params(lengths, variants=VARIANTS):
    # (n, pc) outermost: the reference of a length is built once and reused
    return [pytest.param(n, pc, v, id=f"{n}-{pc}-{v}") for n in lengths for pc in PCS for v in variants]


# ------------------------------------------------- a. iterates, step by step
@pytest.mark.parametrize("n,pc,variant", cg_params(R.CG_LENGTHS))
def test_cg_iterates_match_reference(pa, n, pc, variant):
    c = R.cg_case(n, pc)
    tolx, tolr = R.cg_tols(c, variant)
    M = device_mat(pa, ("sym", n), c["A"])
    b, x = vec_of(M, c["b"]), vec_of(M, np.ones(n), left=False)
    ksp = make_ksp(pa, M, variant, pc)
    dx = dr = 0.0
    for k in range(1, c["K"] + 1):
        ksp.setFixedIterations(k)
        ksp.solve(b, x)
        assert ksp.getIterationNumber() == k
        assert ksp.getConvergedReason() == R.ITS_OK
        dx = max(dx, xerr(x.getArray(), c["xs"][k]))
        if c["rns"][k] >= 1e-6 * c["bn"]:
            dr = max(dr, float(abs(LD(ksp.getResidualNorm()) - c["rns"][k]) / c["rns"][k]))
    ex, er = c["err"][variant]
    print(f"KRYLOV-A variant={variant} pc={pc} n={n} restatement_x={ex:.2e} device_x={dx:.2e} "
          f"restatement_r={er:.2e} device_r={dr:.2e}")
    assert dx <= tolx, (dx, tolx)
    assert dr <= tolr, (dr, tolr)


@pytest.mark.parametrize("n,pc,variant", cg_params((257,) + BIG, ("sr", "pipecg")))
def test_continue_in_pieces_is_bitwise(pa, n, pc, variant):
    """5 + 7 iterations by solveContinue equal 12 at once, bit for bit."""
    c = R.cg_case(n, pc)
    M = device_mat(pa, ("sym", n), c["A"])
    b, x = vec_of(M, c["b"]), vec_of(M, np.zeros(n), left=False)
    ksp = make_ksp(pa, M, variant, pc)
    ksp.setFixedIterations(12)
    ksp.solve(b, x)
    whole, rn = x.getArray(), ksp.getResidualNorm()
    ksp.setFixedIterations(5)
    ksp.solve(b, x)
    ksp.solveContinue(b, x, 7)
    assert np.array_equal(x.getArray(), whole)
    assert ksp.getResidualNorm() == rn


# ------------------------------------------- b. update-kernel knobs, bitwise
@pytest.mark.parametrize("n,pc,variant", cg_params((257,) + BIG, ("sr", "pipecg")))
def test_update_knobs_are_bitwise(pa, n, pc, variant):
    from pynama_amd.runtime import get_tuning, set_tuning
    A, bh = R.sym_tridiag(n)
    M = device_mat(pa, ("sym", n), A)
    b, x = vec_of(M, bh), vec_of(M, np.zeros(n), left=False)
    ksp = make_ksp(pa, M, variant, pc)
    ksp.setFixedIterations(12)
    names = ("upd_preload", "upd_nt", "upd_unroll")
    keep = {k: get_tuning(k) for k in names}
    try:
        ksp.solve(b, x)
        default = x.getArray()
        assert np.isfinite(default).all() and np.abs(default).max() > 0
        combos = ([(p, t, u) for p in (0, 1) for t in (0, 1) for u in (1, 2)] if variant == "sr"
                  else [(p, keep["upd_nt"], keep["upd_unroll"]) for p in (0, 1)])
        for combo in combos:
            for k, v in zip(names, combo):
                set_tuning(k, v)
            ksp.solve(b, x)
            assert np.array_equal(x.getArray(), default), dict(zip(names, combo))
    finally:
        for k, v in keep.items():
            set_tuning(k, v)


# ----------------- c. stopping: reason, count, and x is that iteration's iterate
STOP_LENGTHS = (1025, 262144 + 77)


def check_stop(ksp, x, c, variant, reason, k):
    tolx, tolr = R.cg_tols(c, variant)
    assert ksp.getConvergedReason() == reason
    assert ksp.getIterationNumber() == k
    # x_k itself: not advanced by the launches queued before the host polled
    dx = xerr(x.getArray(), c["xs"][k])
    assert dx <= tolx, (dx, tolx, xerr(x.getArray(), c["xs"][k + 1]))
    assert abs(LD(ksp.getResidualNorm()) - c["rns"][k]) <= tolr * c["rns"][k]


@pytest.mark.parametrize("n,pc,variant", cg_params(STOP_LENGTHS))
@pytest.mark.parametrize("kind", ["rtol", "atol"])
def test_stop_on_tolerance(pa, kind, n, pc, variant):
    c = R.cg_case(n, pc)
    M = device_mat(pa, ("sym", n), c["A"])
    b, x = vec_of(M, c["b"]), vec_of(M, np.ones(n), left=False)
    for k in (7, 8, 9):  # around the host's poll every 8 iterations
        thr = R.gap_threshold(c["rns"], k)
        ksp = make_ksp(pa, M, variant, pc)
        if kind == "rtol":
            ksp.setTolerances(rtol=thr / c["bn"])
        else:
            ksp.setTolerances(rtol=0.0, atol=thr)
        ksp.solve(b, x)
        check_stop(ksp, x, c, variant, R.RTOL if kind == "rtol" else R.ATOL, k)


@pytest.mark.parametrize("n,pc,variant", cg_params(STOP_LENGTHS))
def test_stop_on_max_it(pa, n, pc, variant):
    c = R.cg_case(n, pc)
    M = device_mat(pa, ("sym", n), c["A"])
    b, x = vec_of(M, c["b"]), vec_of(M, np.ones(n), left=False)
    for max_it in (5, 8, 9):
        ksp = make_ksp(pa, M, variant, pc)
        ksp.setTolerances(rtol=1e-30, max_it=max_it)
        ksp.solve(b, x)
        check_stop(ksp, x, c, variant, R.DIV_ITS, max_it)


@pytest.mark.parametrize("n,pc,variant", cg_params(STOP_LENGTHS, VARIANTS + ("gmres",)))
def test_zero_right_hand_side(pa, n, pc, variant):
    A, _ = R.sym_tridiag(n)
    M = device_mat(pa, ("sym", n), A)
    b, x = vec_of(M, np.zeros(n)), vec_of(M, np.ones(n), left=False)
    ksp = make_ksp(pa, M, variant, pc)
    ksp.solve(b, x)
    assert ksp.getConvergedReason() == R.ATOL
    assert ksp.getIterationNumber() == 0
    assert not x.getArray().any()


@pytest.mark.parametrize("variant", VARIANTS)
def test_indefinite_matrix(pa, variant):
    A, bh = R.indefinite_case()
    M = device_mat(pa, "indefinite", A)
    b, x = vec_of(M, bh), vec_of(M, np.ones(A.m), left=False)
    ksp = make_ksp(pa, M, variant, "none")
    ksp.solve(b, x)
    assert ksp.getConvergedReason() == R.DIV_INDEFINITE
    assert ksp.getIterationNumber() == 0
    assert np.isfinite(x.getArray()).all()


@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("variant", VARIANTS + ("gmres",))
def test_nan_in_right_hand_side(pa, variant, pc):
    n = 1025
    A, bh = R.sym_tridiag(n)
    bh = bh.copy()
    bh[700] = np.nan
    M = device_mat(pa, ("sym", n), A)
    b, x = vec_of(M, bh), vec_of(M, np.zeros(n), left=False)
    ksp = make_ksp(pa, M, variant, pc)
    ksp.setTolerances(max_it=40)
    ksp.solve(b, x)
    assert ksp.getConvergedReason() == R.DIV_NAN
    assert ksp.getIterationNumber() == 0


@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("variant", VARIANTS + ("gmres",))
def test_dtol_at_iteration_zero(pa, variant, pc):
    """KSPConvergedDefault tests ||r_0|| >= divtol ||b|| too: divtol <= 1 stops at once."""
    n = 1025
    A, bh = R.sym_tridiag(n)
    M = device_mat(pa, ("sym", n), A)
    b, x = vec_of(M, bh), vec_of(M, np.ones(n), left=False)
    ksp = make_ksp(pa, M, variant, pc)
    ksp.setTolerances(divtol=0.5)
    ksp.solve(b, x)
    assert ksp.getConvergedReason() == R.DIV_DTOL
    assert ksp.getIterationNumber() == 0
    assert not x.getArray().any()


@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_dtol_on_a_rising_residual(pa, variant, pc):
    A, bh, divtol, kx = R.dtol_case(pc)
    xs, rns = R.pcg_reference(A, bh, pc, kx)
    ex, _ = R.history_error(*R.RECURRENCES[variant](A, bh, pc, kx), xs, rns, 0.0)
    M = device_mat(pa, ("dtol", pc), A)
    b, x = vec_of(M, bh), vec_of(M, np.ones(A.m), left=False)
    ksp = make_ksp(pa, M, variant, pc)
    ksp.setTolerances(divtol=divtol)
    ksp.solve(b, x)
    assert ksp.getConvergedReason() == R.DIV_DTOL
    assert ksp.getIterationNumber() == kx
    dx = xerr(x.getArray(), xs[kx])
    assert dx <= 16 * max(ex, R.FLOOR), (dx, ex)
    # and the default divtol (1e5) lets the same solve run on
    ksp.setTolerances(divtol=1e5)
    ksp.solve(b, x)
    assert ksp.getConvergedReason() > 0


# ------------------------------------------------------------------ d. GMRES
@pytest.mark.parametrize("restart", R.GMRES_RESTARTS)
@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("n", R.GMRES_LENGTHS)
def test_gmres_matches_reference(pa, n, pc, restart):
    c = R.gmres_case(n, pc, restart)
    M = device_mat(pa, ("convdiff", n), c["A"])
    b, x = vec_of(M, c["b"]), vec_of(M, np.ones(n), left=False)
    ksp = make_ksp(pa, M, "gmres", pc, restart)
    ksp.setTolerances(rtol=c["rtol"])
    ksp.solve(b, x)
    dx = xerr(x.getArray(), c["ref"]["x"])
    print(f"KRYLOV-D gmres pc={pc} n={n} restart={restart} its={c['ref']['its']} rtol={c['rtol']:.2e} "
          f"restatement_x={c['ex']:.2e} device_x={dx:.2e}")
    assert ksp.getIterationNumber() == c["ref"]["its"]
    if c["ref"]["rn"] >= 1e-13 * c["bn"]:
        assert ksp.getConvergedReason() == c["ref"]["reason"] == R.RTOL
    else:
        # (n = 1: the exact residual is 0, and whether its computed value
        # lands under atol = 1e-50 is rounding's choice: RTOL or ATOL)
        assert ksp.getConvergedReason() in (R.RTOL, R.ATOL)
    assert ksp.getTrueRelativeResidual() <= 2 * c["rtol"]
    assert dx <= 16 * max(c["ex"], R.FLOOR), (dx, c["ex"])


@pytest.mark.parametrize("pc", PCS)
def test_gmres_max_it_inside_a_cycle(pa, pc):
    """max_it = 7 with restart 3: the third cycle ends after one iteration."""
    n = 257
    c = R.gmres_maxit_case(n, pc)
    M = device_mat(pa, ("convdiff", n), c["A"])
    b, x = vec_of(M, c["b"]), vec_of(M, np.ones(n), left=False)
    ksp = make_ksp(pa, M, "gmres", pc, 3)
    ksp.setTolerances(rtol=1e-30, max_it=7)
    ksp.solve(b, x)
    assert ksp.getConvergedReason() == R.DIV_ITS
    assert ksp.getIterationNumber() == 7
    dx = xerr(x.getArray(), c["ref"]["x"])
    assert dx <= 16 * max(c["ex"], R.FLOOR), (dx, c["ex"])


def test_gmres_lucky_breakdown(pa):
    A, bh = R.lucky_case()
    n = A.m
    for key, mat, most in (("lucky3", A, 3), ("lucky1", R.Csr(np.arange(n + 1), np.arange(n), np.full(n, 2.0)), 1)):
        M = device_mat(pa, key, mat)
        b, x = vec_of(M, bh), vec_of(M, np.ones(n), left=False)
        ksp = make_ksp(pa, M, "gmres", "none")
        ksp.setTolerances(rtol=1e-10)
        ksp.solve(b, x)
        assert ksp.getConvergedReason() > 0
        assert 1 <= ksp.getIterationNumber() <= most
        if most == 1:
            assert ksp.getIterationNumber() == 1
        xa = x.getArray()
        assert np.isfinite(xa).all()
        assert ksp.getTrueRelativeResidual() <= 2e-10
        assert np.abs(xa - bh / mat.data).max() <= 2e-10 * np.abs(bh).max()  # (||A^-1|| <= 1/2)


# ------------------------------------------- e. the scalar-CSR product
U = 1.1e-16  # fp64 unit roundoff


@pytest.mark.parametrize("m,ncols", [(1, 1100), (3, 1100), (4, 1100), (5, 1100), (129, 1100), (1000, 1100),
                                     (129, 129), (1000, 1000), (1000, 40)])
def test_aij_product(pa, m, ncols):
    A, xh = R.spmv_case(m, ncols)
    M = pa.petsc.Mat().createAIJ(((m, m), (ncols, ncols)), csr=A.csr)
    assert M.spmvKernel().startswith("k_aij_spmv<8,4>")
    x = vec_of(M, xh, left=False)
    y = (M * x).getArray()
    ref, scale = A.mult(xh.astype(LD)), A.abs_mult(xh)
    # D, the additions one product can pass through in k_aij_spmv<8,4>: a wave
    # per row; a pass covers 512 entries from the row start rounded down to 32
    # and adds a lane's 8 entries of it to the lane's sum one after the other
    # (8 per pass), then 6 xor-shuffle steps sum the 64 lanes.  With the
    # product's own rounding: (D + 1) u sum_j |a_ij x_j|.
    s, e = A.indptr[:-1], A.indptr[1:]
    passes = -(-(e - (s & ~31)) // 512)
    D = 8 * passes + 6
    assert D.max() <= 8 * 3 + 6
    bound = (D + 1) * U * scale
    worst = float(np.max(np.abs(y.astype(LD) - ref) / np.where(scale > 0, scale, 1)))
    print(f"KRYLOV-E m={m} ncols={ncols} D<={int(D.max())} worst |y-ref|/sum|ax| = {worst:.2e}")
    assert np.all(np.abs(y.astype(LD) - ref) <= bound)
    empty = A.row_lengths() == 0
    assert not y[empty].any()


# ------------------------------------------------------- f. vector kernels
VEC_LENGTHS = (1, 63, 65, 257, 10001, 524288 + 300)  # the last: a second grid-stride pass


def dot_depth(n):
    """Additions one product can pass through in kle_vec_dot: k_dot_partial
    (grid min(ceil(n / 256), 2048) of 256 threads) adds ceil(n / (grid 256))
    products per thread, 6 shuffle steps per wave, 4 wave sums per workgroup;
    k_reduce (one workgroup of 1024) adds ceil(grid / 1024) partials per
    thread, 6 shuffle steps, 16 wave sums."""
    g = min(-(-n // 256), 2048)
    return -(-n // (g * 256)) + 6 + 4 + -(-g // 1024) + 6 + 16


def host_vecs(n):
    rng = np.random.default_rng(60000 + n)
    return rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)


def dvec(pa, a):
    v = pa.petsc.Vec().createSeq(len(a))
    v.setArray(a)
    return v


@pytest.mark.parametrize("n", VEC_LENGTHS)
def test_vec_axpy_aypx_waxpy(pa, n):
    xh, yh = host_vecs(n)
    a = -0.7310585786300049
    xl, yl, al = xh.astype(LD), yh.astype(LD), LD(a)
    # one rounding of a x, one of the sum -- or one for both, fused: either is
    # within 2 u (|a x_i| + |y_i|)
    x, y = dvec(pa, xh), dvec(pa, yh)
    y.axpy(a, x)
    assert np.all(np.abs(y.getArray().astype(LD) - (yl + al * xl)) <= 2.2e-16 * (np.abs(al * xl) + np.abs(yl)))
    y = dvec(pa, yh)
    y.aypx(a, x)  # y = x + a y
    assert np.all(np.abs(y.getArray().astype(LD) - (xl + al * yl)) <= 2.2e-16 * (np.abs(al * yl) + np.abs(xl)))
    y, w = dvec(pa, yh), dvec(pa, np.full(n, 7.0))
    w.waxpy(a, x, y)  # w = a x + y
    assert np.all(np.abs(w.getArray().astype(LD) - (al * xl + yl)) <= 2.2e-16 * (np.abs(al * xl) + np.abs(yl)))
    assert np.array_equal(x.getArray(), xh) and np.array_equal(y.getArray(), yh)


@pytest.mark.parametrize("n", VEC_LENGTHS)
def test_vec_exact_kernels(pa, n):
    xh, yh = host_vecs(n)
    x, y = dvec(pa, xh), dvec(pa, yh)
    w = dvec(pa, np.zeros(n))
    w.pointwiseMult(x, y)
    assert np.array_equal(w.getArray(), xh * yh)
    x.scale(1.0 / 3.0)
    assert np.array_equal(x.getArray(), xh * (1.0 / 3.0))
    x.set(-2.5)
    assert np.array_equal(x.getArray(), np.full(n, -2.5))
    y.copy(x)
    assert np.array_equal(x.getArray(), yh)
    zh = yh.copy()
    zh[::3] = 0.0
    z = dvec(pa, zh)
    z.reciprocal()  # zeros stay zero (VecReciprocal)
    za = z.getArray()
    assert not za[::3].any()
    nz = zh != 0
    # (a correctly rounded quotient: half an ulp, 2^-53 relative)
    assert np.all(np.abs(za[nz].astype(LD) - 1 / zh[nz].astype(LD)) <= 1.12e-16 * np.abs(1 / zh[nz].astype(LD)))


@pytest.mark.parametrize("n", VEC_LENGTHS)
def test_vec_dot_and_norm(pa, n):
    xh, yh = host_vecs(n)
    x, y = dvec(pa, xh), dvec(pa, yh)
    D = dot_depth(n)
    ref = R.two_prod_fsum(xh, yh)  # math.fsum of error-free products: the exact sum, rounded once
    scale = math.fsum(np.abs(xh * yh).tolist())
    got = x.dot(y)
    print(f"KRYLOV-F n={n} D={D} |dot-ref|/sum|xy| = {abs(got - ref) / scale:.2e}")
    assert abs(got - ref) <= (D + 1) * U * scale
    # the norm: half the sum's relative error and the root's rounding, <= (D + 1) u
    ref2 = math.sqrt(R.two_prod_fsum(xh, xh))
    assert abs(x.norm() - ref2) <= (D + 1) * U * ref2


def test_dot_depth_values():
    assert [dot_depth(n) for n in (1, 257, 10001, 524288 + 300)] == [34, 34, 34, 36]


def test_vec_set_values_add_with_repeated_index(pa):
    n = 257
    start = np.arange(n, dtype=np.float64) * 0.5
    idx = np.array([5, 5, 256, 5, 100, 0, 5, 256])
    vals = np.array([0.25, 0.5, -3.0, 1.0, 8.0, -0.125, 2.0, 3.0])  # dyadic: every sum exact
    v = dvec(pa, start)
    v.setValues(idx, vals, addv=True)
    v.assemble()
    ref = start.copy()
    np.add.at(ref, idx, vals)
    assert np.array_equal(v.getArray(), ref)
    v.setValues([5, 256], [1.5, -1.5])  # insert: the last value stands
    ref[[5, 256]] = [1.5, -1.5]
    assert np.array_equal(v.getArray(), ref)
