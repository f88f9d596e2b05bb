"""The references of tests/vec_ref.py against exact arithmetic, and what their
bounds can see: errors planted in a host restatement of the device's dot (its
summation order, in fp64) must exceed the bound on every input class while
the unplanted restatement stays inside.  The assertions the suite had before
(tests/test_gpu.py::test_vec_ops: abs(dot - a @ b) < 1e-12, rtol 1e-14 on
axpy) are applied to the same planted errors and reported (VECREF old ...):
the record of what the new tests add.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import vec_ref as V

LD = V.LD
CPU_SIZES = [1, 2, 65, 257, 1025, 10001, V.TRIP + 1, 2 * V.TRIP + 1 + 256]
PLANTS = ["drop_last", "twice", "f32_term", "drop_trip2", "drop_rank"]


def test_rounding_count():
    assert V.grid(0) == 1 and V.grid(257) == 2 and V.grid(V.TRIP + 1) == 2048
    assert [V.dot_roundings(n) for n in (1, 1025, 10001, 262144)] == [31, 31, 31, 31]
    assert V.dot_roundings(262145) == 32 == V.dot_roundings(V.TRIP)  # two partials per k_reduce thread
    assert V.dot_roundings(V.TRIP + 1) == 33  # a second trip of the grid-stride loop
    assert V.dot_roundings(2 * V.TRIP + 257) == 34
    assert V.dot_roundings(10001, 3) == 33
    assert V.SIZES[-1] == 1048577 + 256


@pytest.mark.parametrize("n", [1, 2, 65, 1025, 4096])
def test_fraction_and_longdouble_agree(n):
    """Where both references run they agree to 2^-60 of sum |x_i y_i|."""
    for name, (x, y) in V.dot_inputs(n).items():
        sf, af = V.dot_fraction(x, y)
        sl, al = V.dot_longdouble(x, y)
        assert abs(V._two(sf) - sl) <= LD(2.0) ** -60 * al, (n, name)
        assert abs(V._two(af) - al) <= LD(2.0) ** -60 * al, (n, name)


def test_fraction_reference_is_exact():
    """Against integers: 2^70 + 1 - 2^70 is lost by fp64 and by longdouble, not by the reference."""
    x = np.array([2.0 ** 35, 1.0, -2.0 ** 35, 3.0])
    y = np.array([2.0 ** 35, 1.0, 2.0 ** 35, 0.5])
    s, a = V.dot_fraction(x, y)
    assert s == Fraction(5, 2) and a == 2 ** 71 + Fraction(5, 2)
    assert float(V.dot_exact(x, y)[0]) == 2.5
    c = V.dot_case(x, y)
    assert c["kind"] == "bound" and float(c["ref"]) == 2.5
    assert float(c["bound"]) == pytest.approx(1.01 * 31 * 2.0 ** -53 * 2.0 ** 71, rel=1e-12)


@pytest.mark.parametrize("n", [n for n in V.SIZES if n >= 2])
def test_cancellation_class_cancels(n):
    x, y = V.xy_cancel(n, 15)  # dot_inputs' seed for this class
    assert V.cancels(x, y), n
    assert np.all(x * y != 0.0)


@pytest.mark.parametrize("n", CPU_SIZES)
def test_device_order_stays_inside(n):
    """The fp64 restatement in the kernel's order, on 1 and 3 ranks: inside
    the bound on every class, so the count C covers the code as it stands."""
    for name, (x, y) in V.dot_inputs(n).items():
        for R in (1, 3):
            nmax = max(hi - lo for lo, hi in V.split(n, R))
            c = V.dot_case(x, y, R, nmax)
            assert c["kind"] == "bound"
            r = V.ratio(V.kernel_dot(x, y, R), c)
            print(f"VECREF host dot n={n} R={R} {name}: C={c['C']} err/bound={r:.3f}")
            assert r <= 1.0, (n, name, R, r)
        cn = V.norm_case(x)
        rn = V.ratio(V.kernel_norm(x), cn)
        assert cn["kind"] == "bound" and rn <= 1.0, (n, name, rn)


def _old_dot_accepts(dev, x, y):
    return abs(dev - x @ y) < 1e-12  # tests/test_gpu.py::test_vec_ops, as it was


@pytest.mark.parametrize("n", CPU_SIZES)
def test_planted_errors_exceed_the_bound(n):
    lines = []
    for name, (x, y) in V.dot_inputs(n).items():
        clean_old = _old_dot_accepts(V.kernel_dot(x, y), x, y)
        for plant in PLANTS:
            if plant == "drop_trip2" and n <= V.TRIP:
                continue
            R = 3 if plant == "drop_rank" else 1
            if R > n:
                continue
            nmax = max(hi - lo for lo, hi in V.split(n, R))
            c = V.dot_case(x, y, R, nmax)
            dev = V.kernel_dot(x, y, R, plant)
            r = V.ratio(dev, c)
            old = _old_dot_accepts(dev, x, y)
            lines.append(f"VECREF old n={n} {name} {plant}: err/bound={r:.3g} old-accepts={old} "
                         f"(old accepts the correct sum: {clean_old})")
            assert r > 1.0, (n, name, plant, r)
    print("\n".join(lines))


def test_old_assertion_never_reaches_the_second_trip():
    """The old test's one size (10001) has no 524289th entry: that planted
    error is outside what it could see at all."""
    assert 10001 <= V.TRIP


@pytest.mark.parametrize("a", [1.0 / 3.0, 0.1, -2.0 / 7.0])
def test_axpy_bound_sees_a_rounded_to_float32(a):
    x, y = V.x_uniform(10001, 3), V.x_uniform(10001, 4)
    ref, b = V.axpy(a, x, y)
    r0, _ = V.worst(a * x + y, ref, b)
    fused = np.asarray(LD(a) * x.astype(LD) + y.astype(LD), np.float64)  # one rounding (double rounding aside)
    r1, _ = V.worst(fused, ref, b)
    assert r0 <= 1.0 and r1 <= 1.0
    bad = float(np.float32(a)) * x + y
    rb, k = V.worst(bad, ref, b)
    frac = float(np.mean(np.abs(bad.astype(LD) - ref) > b))
    old = bool(np.allclose(bad, a * x + y, rtol=1e-14, atol=0))
    print(f"VECREF old axpy a={a:.4g} as float32: err/bound={rb:.3g} at {k}, {100 * frac:.1f}% of entries "
          f"outside, old-accepts={old}")
    assert rb > 1.0 and frac > 0.9


def test_axpy_bound_is_entrywise_under_cancellation():
    """y = -a x to rounding: the result is tiny, the bound stays u |a x|."""
    x = V.x_uniform(1000, 5)
    a = 1.0 / 3.0
    y = -(a * x)
    ref, b = V.axpy(a, x, y)
    assert V.worst(a * x + y, ref, b)[0] <= 1.0
    assert V.worst(np.asarray(LD(a) * x.astype(LD) + y.astype(LD), np.float64), ref, b)[0] <= 1.0
    assert np.all(b <= 2.03 * V.U * np.abs(a * x) + 1e-300)


def test_tensor_square_order_and_swap():
    v = V.x_uniform(3 * 50, 6)
    t = V.tensor_square(v, 3).reshape(-1, 6)
    x, y, z = v.reshape(-1, 3).T
    assert np.array_equal(t[:, 1], x * y) and np.array_equal(t[:, 3], y * z) and np.array_equal(t[:, 5], z * x)
    swapped = t[:, [0, 3, 2, 1, 4, 5]].ravel()  # the planted error: xy and yz exchanged
    assert not V.same_bits(swapped, t.ravel())
    t2 = V.tensor_square(v[:100], 2).reshape(-1, 3)
    x, y = v[:100].reshape(-1, 2).T
    assert np.array_equal(t2, np.stack([x * x, x * y, y * y], 1))


def test_same_bits_sees_signed_zero_and_nan_positions():
    assert V.same_bits([0.0, np.nan, 1.0], [0.0, np.nan, 1.0])
    assert not V.same_bits([0.0], [-0.0])
    assert not V.same_bits([np.nan, 1.0], [1.0, np.nan])
    assert V.first_diff([1.0, -0.0], [1.0, 0.0])[0] == 1
    r = V.reciprocal(np.array([2.0, 0.0, -0.0, -4.0, np.inf]))
    assert V.same_bits(r, [0.5, 0.0, -0.0, -0.25, 0.0])


def test_norm_cases_are_named():
    x = V.x_uniform(1025, 7)
    big, small, huge, over = x * 2.0 ** 600, x * 2.0 ** -600, x * 2.0 ** 1000, x * 2.0 ** 1020
    # 2^1000 U(-1, 1) at n = 1025: the squares overflow, the norm (about 2^1004) does not
    for v in (big, small, huge):
        c = V.norm_case(v)
        assert c["kind"] == "bound"
        assert float(c["ref"]) == pytest.approx(np.linalg.norm(x) * (v[0] / x[0]), rel=1e-14)
    # sqrt(dot(x, x)) as the code stood: inf and 0.0 for representable norms (finding 2)
    assert V.kernel_norm(big) == np.inf and V.kernel_norm(small) == 0.0
    assert V.ratio(V.kernel_norm(big), V.norm_case(big)) == np.inf
    assert V.ratio(V.kernel_norm(small), V.norm_case(small)) > 1.0
    assert V.norm_case(over)["kind"] == "overflow"
    x[3] = np.nan
    assert V.norm_case(x)["kind"] == "exact-special" and np.isnan(V.norm_case(x)["ref"])
    x[3] = -np.inf
    assert V.norm_case(x)["ref"] == np.inf
    tiny = np.full(10, 2.0 ** -1060)
    assert V.dot_case(tiny, tiny)["kind"] == "subnormal"


def test_dot_special_values():
    x, y = V.x_uniform(100, 8), V.x_uniform(100, 9)
    x[63] = np.nan
    assert np.isnan(V.dot_case(x, y)["ref"])
    x[63] = np.inf
    c = V.dot_case(x, y)
    assert c["kind"] == "exact-special" and c["ref"] == math.copysign(np.inf, y[63])
    x[5] = -np.inf * np.sign(y[5]) * np.sign(y[63])
    assert np.isnan(V.dot_case(x, y)["ref"])  # +inf and -inf among the terms
    assert V.special_ok(float("nan"), V.dot_case(x, y)) and not V.special_ok(1.0, V.dot_case(x, y))
