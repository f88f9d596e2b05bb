"""tests/ranks_ref.py on the host: the ranks' exports join into the matrix they
were cut from, the restated partitioned product of a synthetic
block-tridiagonal 3 x 3 SPD matrix on 2 and 3 row ranges passes the row-by-row
check of the GPU tests, and each interface error planted in it
(ranks_ref.FAULTS) fails that check on a comb or an only_r input."""
import numpy as np
import pytest

import ranks_ref as RR
import sym_ref as S

NODES = 240  # 80 or 120 node rows per range: more than one 64-row slice each
CUTS = {2: [0, 120, 240], 3: [0, 80, 160, 240]}
DIMS, ORDER = [1, 1, NODES], 1  # the chain as a z lattice of order 1, one node per plane: combs of stride 3


@pytest.fixture(scope="module")
def K():
    A = RR.block_tridiagonal(NODES)
    assert S.is_symmetric(A)
    return A


def _ranges(size):
    c = CUTS[size]
    return [(3 * a, 3 * b) for a, b in zip(c, c[1:])]


def _parts(A, ranges):
    out = []
    for lo, hi in ranges:
        s, e = A.indptr[lo], A.indptr[hi]
        out.append((lo, hi, A.indptr[lo:hi + 1] - s, A.indices[s:e], A.data[s:e]))
    return out


@pytest.fixture(scope="module")
def cases(K):
    """Per number of ranges: the inputs and their longdouble references."""
    out = {}
    for size in CUTS:
        ranges = _ranges(size)
        xs = RR.rank_inputs(K, ranges, DIMS, ORDER)
        refs = {}
        for nm, x in xs.items():
            ref, den = S.reference(K, x)
            refs[nm] = (ref, den, S.restatement(K, x, ref, den))
        out[size] = (ranges, xs, refs)
    return out


def _failing(A, ranges, xs, refs, fault):
    """The inputs on which some rank's rows miss the check, products taken in
    the inputs' order (a stale buffer holds the previous product's sums)."""
    bad, prev = [], np.zeros(A.m)
    zero = np.zeros(A.m, np.longdouble)
    for nm, x in xs.items():
        y, recv = RR.partitioned_product(A, ranges, x, fault, prev)
        prev = recv
        ref, den, rest = refs[nm]
        for lo, hi in ranges:
            try:
                ok = RR.owned_slice_check(y[lo:hi], lo, hi, ref, den, rest, zero)[3]
            except AssertionError:  # (a row without a product is not exactly 0)
                ok = False
            if not ok:
                bad.append(nm)
                break
    return bad


def test_global_csr_joins_the_parts(K):
    for size in CUTS:
        ranges = _ranges(size)
        A, got = RR.global_csr(_parts(K, ranges)[::-1])  # (any order)
        assert got == ranges
        for a, b in zip(A.csr, K.csr):
            np.testing.assert_array_equal(a, b)
    parts = _parts(K, _ranges(3))
    with pytest.raises(AssertionError):
        RR.global_csr([parts[0], parts[2]])  # a gap
    with pytest.raises(AssertionError):
        RR.global_csr(parts[1:])  # does not start at 0


@pytest.mark.parametrize("size", list(CUTS))
def test_inputs_tell_the_ranks_apart(K, cases, size):
    ranges, xs, refs = cases[size]
    combs = [nm for nm in xs if nm.startswith("comb")]
    assert len(combs) == 27
    hit = np.zeros(K.n, bool)
    for nm in combs:
        assert S.terms_per_row(K, xs[nm]).max() <= 1
        hit |= xs[nm] != 0
    assert hit.reshape(-1, 3).any(axis=1).all()  # every node is in some comb
    for k, (lo, hi) in enumerate(ranges):
        x = xs[f"only_r{k}"]
        assert np.all(x[lo:hi] != 0) and not x[:lo].any() and not x[hi:].any()
        ref = refs[f"only_r{k}"][0]
        for j, (a, b) in enumerate(ranges):  # a neighbour's rows see rank k through the interface alone
            assert bool(ref[a:b].any()) == (abs(j - k) <= 1)
        for where in ("first", "last"):
            x = xs[f"iface_spike_{k}_{where}"]
            at = np.flatnonzero(x == 1e8)
            assert len(at) == 1 and lo <= at[0] < hi
            assert at[0] // 3 == (lo // 3 if where == "first" else hi // 3 - 1)
    assert RR.family("comb12") == "comb" and RR.family("only_r2") == "only_r"
    assert RR.family("iface_spike_0_last") == "iface_spike" and RR.family("ramp") == "ramp"


@pytest.mark.parametrize("size", list(CUTS))
def test_restated_partitioned_product_passes(K, cases, size):
    ranges, xs, refs = cases[size]
    assert _failing(K, ranges, xs, refs, None) == []
    worst = 0.0
    zero = np.zeros(K.m, np.longdouble)
    for nm, x in xs.items():
        y, recv = RR.partitioned_product(K, ranges, x)
        ref, den, rest = refs[nm]
        for lo, hi in ranges:
            dev, used, _, ok = RR.owned_slice_check(y[lo:hi], lo, hi, ref, den, rest, zero)
            assert ok, (nm, lo, used)
            worst = max(worst, used)
        if nm.startswith("only_r"):
            k = int(nm[len("only_r"):])
            assert recv[:ranges[k][0]].any() == 0 and (k + 1 == size or recv[ranges[k + 1][0]:ranges[k + 1][1]].any())
    print(f"SYMREF-RANKS restated ranges={size} tol_used={worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("size", list(CUTS))
@pytest.mark.parametrize("fault", RR.FAULTS)
def test_planted_interface_error_fails_the_check(K, cases, size, fault):
    ranges, xs, refs = cases[size]
    bad = _failing(K, ranges, xs, refs, fault)
    sharp = [nm for nm in bad if nm.startswith(("comb", "only_r"))]
    print(f"SYMREF-RANKS planted={fault} ranges={size} failing={len(bad)} of {len(xs)} "
          f"(combs and only_r: {len(sharp)})")
    assert sharp, (fault, bad)
