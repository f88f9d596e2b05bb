"""The host helpers of tests/sym_ref.py on the CPU oracle's K (box [4,3,3],
ngl 5: 2,873 nodes, 2.15 M nonzeros; Dirichlet on every face), no GPU.

  * the comb inputs have the single-term property they are made for;
  * a host emulation of the one-brick arithmetic (fp64 direct sums, every
    transposed term rounded to the brick's quantum q, integer sums) stays,
    row by row and for every input maker, within
        16 u (|K||x|)_i + nT_i q / 2 + (nnz_i + 2) eta,
    the bound the GPU tests hold the device to (tests/test_gpu_sym_ref.py;
    there the fp64 restatement's own error stands for the first and the last
    term).  eta = 2^-1075 is fp64's absolute rounding error where a product
    underflows gradually, fl(a b) = a b (1 + d) + e with |d| <= u and
    |e| <= eta: one per product of the row and two for the sum's way back
    to fp64.  It is 5e-324 x nnz_i, nothing unless x is subnormal -- without
    it the subnormal input misses 16 u (|K||x|)_i by 2e7, and so does the
    plain fp64 product;
  * the a-priori quantum bounds the brick's;
  * the bound restated from k_brick_bound keeps every region sum below 2^61
    (asserted inside the emulation) and the adversarial input uses more of it
    than a uniform one.
"""
import numpy as np
import pytest

import sym_ref as S
from krylov_ref import LD
from oracle import oracle as O

NELEM, NGL = [4, 3, 3], 5
ETA = np.ldexp(LD(1), -1075)  # half the smallest subnormal


@pytest.fixture(scope="module")
def case():
    m = O.BoxMesh(3, NELEM, [0, 0, 0], [1, 1, 1], NGL)
    c = m.coords()
    flag = np.any((c == 0.0) | (c == 1.0), axis=1).astype(np.uint8)
    K, _, _ = m.assemble_fs(flag)
    A = S.as_csr(K.indptr, K.indices, K.data)
    dims = [n * (NGL - 1) + 1 for n in NELEM]
    assert A.m == 3 * int(np.prod(dims))
    return A, dims, S.inputs(A, dims, NGL - 1)


def test_oracle_k_is_symmetric_with_identity_rows(case):
    A, dims, _ = case
    assert S.is_symmetric(A)
    ident = S.identity_rows(A)
    inner = int(np.prod([d - 2 for d in dims]))
    assert len(ident) == A.m - 3 * inner


def test_comb_has_one_term_per_row(case):
    A, dims, xs = case
    for nm, x in xs.items():
        if not nm.startswith("comb"):
            continue
        assert np.count_nonzero(x) >= 1 and np.abs(x[x != 0]).min() >= 0.5 and np.abs(x).max() <= 2.0
        assert len({int(i) % 3 for i in np.flatnonzero(x)}) == 1
        tpr = S.terms_per_row(A, x)
        assert tpr.max() == 1 and tpr.sum() > 0, nm
        # so the product is that one entry times its x, exactly
        ref, den = S.reference(A, x)
        assert np.array_equal(np.abs(ref), den)
        assert S.restatement(A, x, ref, den) <= S.U
    g = S.comb_greedy(A, 1, seed=3)
    assert S.terms_per_row(A, g).max() == 1 and np.count_nonzero(g) >= 2


def test_scaled_err_sees_one_small_entry(case):
    """A dropped entry that a norm-wise 1e-14 does not see is O(1) here."""
    A, _, xs = case
    x = xs["uniform"]
    ref, den = S.reference(A, x)
    y = A.mult(x)
    r = int(np.argmin(np.where(den > 0, np.abs(ref), np.inf)))
    p = A.indptr[r] + int(np.argmax(np.abs(A.data[A.indptr[r]:A.indptr[r + 1]] * x[A.indices[A.indptr[r]:A.indptr[r + 1]]])))
    y2 = y.copy()
    y2[r] -= A.data[p] * x[A.indices[p]]
    assert np.linalg.norm(y2 - y) <= 1e-3 * np.linalg.norm(y)
    assert S.scaled_err(y2, ref, den) > 1e10 * S.scaled_err(y, ref, den)
    with pytest.raises(AssertionError):  # (a row of zero products must be exactly 0)
        S.scaled_err(np.ones(A.m), ref, np.zeros(A.m, LD))


@pytest.mark.parametrize("name", ["uniform", "ramp", "spike", "sign_adversarial", "subnormal"] +
                         [f"comb{k}" for k in range(S.COMB_CASES)])
def test_emulated_brick_is_within_the_bound(case, name):
    A, _, xs = case
    x = xs[name]
    ref, den = S.reference(A, x)
    q, nT = S.brick_quantum(A, x)
    qa, nTa = S.apriori_quantum(A, x)
    assert q <= qa and np.array_equal(nT, nTa)
    y = S.emulate_one_brick(A, x, q)
    on = den > 0
    assert not y[~on].any()
    err = np.abs(y.astype(LD) - ref)
    bound = 16 * LD(S.U) * den + nT * q / 2 + (A.row_lengths() + 2) * ETA
    used = float((err[on] / bound[on]).max())
    quant = float(np.mean((nT * q / 2)[on] > (LD(S.U) * den)[on]))
    nw = float(np.sqrt(((y.astype(LD) - ref) ** 2).sum() / (ref ** 2).sum()))
    print(f"SYM-EMU input={name} restatement={S.restatement(A, x, ref, den) / S.U:.2f}u "
          f"emulated={S.scaled_err(y, ref, den) / S.U:.3g}u bound_used={used:.2f} rows_quantum_larger={quant:.2f} "
          f"normwise={nw:.1e}")
    assert used <= 1.0, (name, used)


def test_identity_rows_are_exact_in_the_emulation(case):
    A, _, xs = case
    x = xs["uniform"]
    q, _ = S.brick_quantum(A, x)
    ident = S.identity_rows(A)
    assert np.array_equal(S.emulate_one_brick(A, x, q)[ident], x[ident])


def test_adversarial_input_fills_more_of_the_bound(case):
    """The share of 2^61 the largest region sum reaches: the adversarial x is
    made to reach the most a row's transposed sum can, a uniform x stays below."""
    A, _, xs = case
    fill = {}
    for nm in ("uniform", "sign_adversarial"):
        x = xs[nm]
        q, _ = S.brick_quantum(A, x)
        rows = np.repeat(np.arange(A.m), np.diff(A.indptr))
        low = A.indices // 3 < rows // 3
        tr = np.zeros(A.m, LD)
        np.add.at(tr, rows[low], (A.data[low] * x[A.indices[low]]).astype(LD))
        fill[nm] = float(np.abs(tr).max() / q / LD(2.0) ** 61)
    print(f"SYM-EMU fill of 2^61: {fill}")
    assert fill["uniform"] < fill["sign_adversarial"] < 1.0
