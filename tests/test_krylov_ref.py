"""The numpy Krylov references check themselves (no GPU): the three CG
recurrences are one iteration, GMRES solves the system, and every input of
tests/test_gpu_krylov.py has the gaps its assertions rely on, so that no GPU
test can pass or fail by a coin flip."""
import numpy as np
import pytest

import krylov_ref as R

LD = np.longdouble
PCS = ("none", "jacobi")


def test_longdouble_is_extended_precision():
    assert np.finfo(LD).eps < 2e-19


@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("n", [65, 1025, 524288 + 300])
def test_recurrences_agree_in_longdouble(n, pc):
    """In longdouble the single-reduction and pipelined recurrences reproduce
    the reference's iterates and residual norms to 1e-16 over 12 iterations."""
    A, b = R.sym_tridiag(n)
    xs, rns = R.pcg_reference(A, b, pc, R.CG_ITERS)
    assert len(xs) == R.CG_ITERS + 1
    for name in ("sr", "pipecg"):
        ex, er = R.history_error(*R.RECURRENCES[name](A, b, pc, R.CG_ITERS, dtype=LD), xs, rns, 1e-6 * float(rns[0]))
        print(f"n={n} pc={pc} {name}: x {ex:.1e} rnorm {er:.1e}")
        assert ex <= 1e-16, (name, ex)
    # the reference's recursive residual is the true one
    r = b.astype(LD) - A.mult(xs[-1])
    assert abs(np.sqrt((r * r).sum()) - rns[-1]) <= 1e-16 * rns[0]


@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("n", [1, 2, 63, 257, 1025])
def test_fp64_restatements_are_at_rounding_level(n, pc):
    """The yardstick itself: fp64 restatements sit within 1e-14 of the
    reference (a wrong recurrence would sit at O(1))."""
    c = R.cg_case(n, pc)
    assert c["K"] == min(R.CG_ITERS, n)
    for v, (ex, er) in c["err"].items():
        assert ex <= 1e-14, (v, ex)


@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("n", [1025, 262144 + 77])
def test_cg_residual_history_has_the_gaps_the_stopping_tests_use(n, pc):
    c = R.cg_case(n, pc)
    rns = c["rns"]
    for k in (7, 8, 9):
        thr = R.gap_threshold(rns, k)
        assert R.gap_ok(rns, k, thr), (k, [float(v) for v in rns])
    for maxit in (5, 8, 9):  # DIVERGED_ITS at rtol 1e-30: nothing converges before
        assert rns[maxit] > 1e-20 * c["bn"]


@pytest.mark.parametrize("pc", PCS)
def test_dtol_case_crosses_cleanly(pc):
    A, b, divtol, kx = R.dtol_case(pc)
    xs, rns = R.pcg_reference(A, b, pc, kx)
    bn = rns[0]
    assert all(rns[k] < 0.5 * divtol * bn for k in range(kx))
    assert rns[kx] > 2.0 * divtol * bn
    assert rns[0] > 1e-5 * bn  # (and it does not converge first at the default rtol)
    if pc == "none":
        assert abs(float(rns[1] / bn) - 49.995) < 1e-9
    else:
        assert np.count_nonzero(A.data) == 4  # not diagonal


def test_indefinite_case():
    A, b = R.indefinite_case()
    assert float((b.astype(LD) * A.mult(b.astype(LD))).sum()) < -1.0


@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("n", [65, 257, 1025])
def test_gmres_reference_solves_the_system(n, pc):
    """||A^-1|| <= 1 for this family, so ||x - x_thomas|| <= ||r|| <= rtol ||b||."""
    A, b, lo, d, up = R.convdiff(n)
    rtol = 1e-15
    out = R.gmres(A, b, pc, 30, rtol, dtype=LD)
    assert out["reason"] == R.RTOL
    xt = R.thomas(lo, d, up, b)
    err = np.sqrt(((out["x"] - xt) ** 2).sum())
    assert err <= 2 * rtol * out["bn"], float(err)
    rt = b.astype(LD) - A.mult(xt)
    assert np.abs(rt).max() <= 1e-18 * n


@pytest.mark.parametrize("restart", R.GMRES_RESTARTS)
@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("n", R.GMRES_LENGTHS)
def test_gmres_cases_stop_in_a_gap(n, pc, restart):
    c = R.gmres_case(n, pc, restart)
    floor = 1e-13 * c["bn"]
    rns = [max(v, LD(floor)) for v in c["rns"]]
    assert R.gap_ok(rns, c["k"], c["thr"]), (c["k"], [float(v) for v in rns])
    assert c["ref"]["its"] == c["k"] == c["f64"]["its"]
    assert c["ref"]["reason"] == c["f64"]["reason"] > 0
    if n > 1 and restart < 8:
        assert c["k"] > restart  # the stop lies past a restart (m = 3: past two)
    # a restart's true residual equals the estimate it replaces: same side of the gap
    for its, est, x in c["ref"]["hist"]:
        r = c["b"].astype(LD) - c["A"].mult(x)
        assert abs(np.sqrt((r * r).sum()) - est) <= 1e-15 * c["bn"]
    assert c["ex"] <= 1e-14


@pytest.mark.parametrize("pc", PCS)
def test_gmres_maxit_case(pc):
    c = R.gmres_maxit_case(257, pc)
    assert c["ref"]["its"] == 7 and c["ref"]["reason"] == R.DIV_ITS
    assert c["ref"]["hist"][-1][0] == 7
    assert np.abs(c["ref"]["x"] - c["ref"]["hist"][-1][2]).max() == 0


def test_gmres_lucky_breakdown_and_nan():
    A, b = R.lucky_case()
    out = R.gmres(A, b, "none", 30, 1e-10, dtype=LD)
    assert out["its"] <= 3 and out["reason"] > 0
    A2 = R.Csr(np.arange(258), np.arange(257), np.full(257, 2.0))
    assert R.gmres(A2, b, "none", 30, 1e-10, dtype=LD)["its"] == 1
    bad = b.copy()
    bad[100] = np.nan
    assert R.gmres(A, bad, "none", 30, 1e-10)["reason"] == R.DIV_NAN
    assert R.gmres(A, b, "none", 30, 1e-10, dtol=0.5)["reason"] == R.DIV_DTOL


def test_thomas():
    n = 40
    A, b, lo, d, up = R.convdiff(n)
    x = R.thomas(lo, d, up, b)
    dense = np.zeros((n, n))
    for i in range(n):
        dense[i, A.indices[A.indptr[i]:A.indptr[i + 1]]] = A.data[A.indptr[i]:A.indptr[i + 1]]
    assert np.abs(np.linalg.solve(dense, b) - x.astype(np.float64)).max() <= 1e-14


def test_csr_product_and_exact_dot():
    A, x = R.spmv_case(129, 1100)
    assert set(A.row_lengths()) == set(R.SPMV_ROW_LENGTHS)
    assert len({int(s) % 32 for s in A.indptr[:-1]}) > 8  # row starts at many offsets modulo 32
    dense = np.zeros((A.m, A.n))
    for i in range(A.m):
        dense[i, A.indices[A.indptr[i]:A.indptr[i + 1]]] = A.data[A.indptr[i]:A.indptr[i + 1]]
    y = A.mult(x.astype(LD))
    assert y.dtype == LD
    # (two longdouble summation orders of <= 1100 terms: n eps sum|a x| apart at most)
    assert np.all(np.abs(y - dense.astype(LD) @ x.astype(LD)) <= 1100 * np.finfo(LD).eps * A.abs_mult(x))
    assert y[A.row_lengths() == 0].tolist() == [0.0] * int((A.row_lengths() == 0).sum())
    # math.fsum over error-free products is the exact dot product
    a = np.array([1e16, 1.0, -1e16, 3.0])
    assert R.two_prod_fsum(a, np.ones(4)) == 4.0
    xr = np.random.default_rng(3).uniform(-1, 1, 1001)
    yr = np.random.default_rng(4).uniform(-1, 1, 1001)
    assert abs(R.two_prod_fsum(xr, yr) - float((xr.astype(LD) * yr.astype(LD)).sum())) <= 1e-16 * np.abs(xr * yr).sum()
