"""References and rounding bounds of the Vec surface (kle_core.hip: k_set,
k_axpy, k_aypx, k_waxpy, k_scale, k_pmult, k_recip, k_vtensv, k_dot_partial,
k_reduce, the allreduce), no GPU and no project import.  u = 2^-53 and the 1.01
slack of mat_ref / elem_ref (second-order terms, the reference's own 2^-64).

Single-rounding operations (set, copy, scale, pointwiseMult, reciprocal, the
tensor square): numpy's fp64 result IS the reference, the device must give its
bits (same_bits: sign of zero and NaN positions included).

axpy / aypx / waxpy: a x_i + y_i (x_i + b y_i) in longdouble; fused or not the
device is within 1.01 u (|a x_i| + |ref_i|) of it: the product's rounding is at
most u |a x_i|, the sum's u |result|.

dot / norm: the reference is exact -- Fraction arithmetic up to EXACT_MAX
entries, longdouble pairwise sums of longdouble products (each a 2^-64
rounding) beyond.  The bound is 1.01 C u sum |x_i y_i| with C the roundings on
the longest path of one term through the code as it stands
(dot_roundings(n, R), n the largest local size):

  k_dot_partial  grid g = min(max(ceil(n / 256), 1), 2048) blocks of 256; a
                 thread adds its m = ceil(n / (256 g)) terms to s = 0.  A term
                 is rounded once as a product (or once in the fma that adds
                 it) and once in each later addition; the first addition, to
                 0, is exact.  m roundings at most (not 2 m: a path holds one
                 product, not m of them).
  wave_sum       6 xor-shuffle levels: 6.
  block_sum      4 wave sums added to s = 0 in turn, the first exactly: 3.
  k_reduce       1024 threads, thread t adds partials t, t + 1024, ... to 0:
                 ceil(g / 1024) - 1; then 6 shuffle levels and 16 wave sums, the
                 first added exactly: 6 + 15.
  allreduce      R - 1 additions in whatever order the transport takes.

  C(n, R) = m + 6 + 3 + (ceil(g / 1024) - 1) + 6 + 15 + (R - 1)
          = 31 for n <= 262144 on one rank (g <= 1024), 32 up to 524288,
            33 for n = 524289 (m = 2), 34 for 1048833 (m = 3).

(Additions of the exact zeros of idle threads round nothing, so small n sit
far inside.)  norm: the sum of squares has no cancellation, so its relative
error C u halves under the square root, whose own rounding adds one:
1.01 (C / 2 + 1) u ||x||.  The scaled path scales by a power of two, exactly,
and sums in the same order: the same count.

The ulp model needs normal numbers: dot_case / norm_case name the cases it does
not cover instead of bounding them -- "exact-special" (a NaN or an infinity:
IEEE fixes the result), "subnormal" (sum |x_i y_i| below 2^-969: the terms may
round by absolute 2^-1075 steps) and "overflow" (the true result is beyond
fp64: inf is the answer).

kernel_dot restates the device summation order in plain fp64 (the "device" of
the CPU tests) and takes the planted errors of test_vec_ref.py.
"""
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SLACK = 1.01
VB, VMAX, RB = 256, 2048, 1024
EXACT_MAX = 4096
TRIP = VB * VMAX  # entries of one trip of the grid-stride loop: 524288
TINY = 2.0 ** -969

# the sizes of the GPU tests: each the smallest that reaches an edge
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 10001, TRIP - 1, TRIP, TRIP + 1, 2 * TRIP + 1 + 256]


def grid(n):
    return int(min(max(-(-n // VB), 1), VMAX))


def dot_roundings(n, R=1):
    """C of the module docstring; n the largest local size, R the ranks."""
    g = grid(n)
    m = -(-n // (VB * g))
    return m + 6 + 3 + (-(-g // RB) - 1) + 6 + 15 + (R - 1)


def same_bits(a, b):
    """Bit equality of two fp64 arrays, every NaN counted as one value."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return bool(np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def first_diff(a, b):
    """(index, a, b) of the first entry whose bits differ, for messages."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    if a.shape != b.shape:
        return ("shape", a.shape, b.shape)
    bad = np.nonzero(~((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))[0]
    return None if len(bad) == 0 else (int(bad[0]), float(a[bad[0]]).hex(), float(b[bad[0]]).hex())


# ---------------------------------------------------------------- element-wise
def axpy(a, x, y):
    """(a x + y in longdouble, entry-wise bound); aypx(b, x, y) = axpy(b, y, x)."""
    ax = LD(a) * np.asarray(x, LD)
    ref = ax + np.asarray(y, LD)
    return ref, SLACK * LD(U) * (np.abs(ax) + np.abs(ref))


def worst(dev, ref, bound):
    """Largest err / bound and its index (bound 0: the entry must be equal)."""
    dev = np.asarray(dev, np.float64)
    if len(dev) == 0:
        return 0.0, -1
    err = np.abs(dev.astype(LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, LD(0), LD(np.inf)))
    r = np.where(np.isnan(r), LD(np.inf), r)
    k = int(np.argmax(r))
    return float(r[k]), k


def tensor_square(v, dim):
    """computeVtensV's order: xx, xy, yy (2-D); xx, xy, yy, yz, zz, zx (3-D)."""
    v = np.asarray(v, np.float64).reshape(-1, dim)
    x, y = v[:, 0], v[:, 1]
    if dim == 2:
        return np.stack([x * x, x * y, y * y], axis=1).ravel()
    z = v[:, 2]
    return np.stack([x * x, x * y, y * y, y * z, z * z, z * x], axis=1).ravel()


def reciprocal(x):
    """VecReciprocal: an entry that compares equal to 0 stays as it is."""
    x = np.asarray(x, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(x != 0.0, 1.0 / np.where(x != 0.0, x, 1.0), x)


# ------------------------------------------------------------------ dot, norm
def _two(fr):
    """A Fraction in longdouble (to its 64 bits, over its whole exponent
    range: squares of entries near 2^1000 are beyond fp64)."""
    if fr == 0:
        return LD(0)
    num, den = abs(fr.numerator), fr.denominator
    s = 128 - (num.bit_length() - den.bit_length())
    q = (num << s) // den if s >= 0 else num // (den << -s)  # 128 or 129 bits of the quotient
    v = LD(0)
    for k in range((q.bit_length() + 31) // 32 - 1, -1, -1):
        v = v * LD(2.0 ** 32) + LD(float((q >> (32 * k)) & 0xFFFFFFFF))
    return np.ldexp(v if fr > 0 else -v, -s)


def dot_fraction(x, y):
    """(sum x_i y_i, sum |x_i y_i|) exactly, as Fractions (finite entries)."""
    s, a = Fraction(0), Fraction(0)
    for p, q in zip(np.asarray(x, np.float64).tolist(), np.asarray(y, np.float64).tolist()):
        t = Fraction(p) * Fraction(q)
        s += t
        a += abs(t)
    return s, a


def _pairwise(t):
    """Pairwise longdouble sum (numpy's own is pairwise only per 128-block)."""
    t = np.asarray(t, LD)
    while len(t) > 1:
        if len(t) & 1:
            t = np.concatenate([t, np.zeros(1, LD)])
        t = t[0::2] + t[1::2]
    return t[0] if len(t) else LD(0)


def dot_longdouble(x, y):
    t = np.asarray(x, LD) * np.asarray(y, LD)
    return _pairwise(t), _pairwise(np.abs(t))


def dot_exact(x, y):
    """(sum, sum of |terms|) in longdouble: the exact sums rounded once (2^-64)
    up to EXACT_MAX entries; beyond, each product and each of the log2(n)
    levels of the pairwise sum round by 2^-64 of sum |terms| at most."""
    if len(x) <= EXACT_MAX:
        s, a = dot_fraction(x, y)
        return _two(s), _two(a)
    return dot_longdouble(x, y)


def dot_case(x, y, R=1, nmax=None):
    """{"kind", "ref", "bound", "C"} of dot(x, y) on R ranks, nmax the largest
    local size (default: all of it on one rank).  kind: "bound" (|dev - ref| <=
    bound), "exact-special" (dev must be ref: NaN, +inf or -inf by IEEE rules)
    or "subnormal" (sum |x_i y_i| below 2^-969: no ulp bound, named)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    C = dot_roundings(len(x) if nmax is None else nmax, R)
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        with np.errstate(invalid="ignore", over="ignore"):
            t = x * y  # every IEEE sum of terms holding a NaN, or infinities, gives the same
            ref = np.nan if np.isnan(t).any() or (np.isposinf(t).any() and np.isneginf(t).any()) else \
                (np.inf if np.isposinf(t).any() else -np.inf)
        return {"kind": "exact-special", "ref": ref, "bound": 0.0, "C": C}
    s, a = dot_exact(x, y)
    kind = "bound" if (a == 0 or a >= TINY) else "subnormal"
    return {"kind": kind, "ref": s, "abs": a, "bound": SLACK * C * LD(U) * a, "C": C}


def norm_case(x, R=1, nmax=None):
    """The same for norm(x): bound 1.01 (C / 2 + 1) u ||x||; "overflow" when
    the true norm is beyond fp64 (dev must be inf).  Entries near 2^+-600 are
    "bound" cases: the norm is representable, the longdouble squares too."""
    x = np.asarray(x, np.float64)
    C = dot_roundings(len(x) if nmax is None else nmax, R)
    if np.isnan(x).any():
        return {"kind": "exact-special", "ref": np.nan, "bound": 0.0, "C": C}
    if np.isinf(x).any():
        return {"kind": "exact-special", "ref": np.inf, "bound": 0.0, "C": C}
    if len(x) <= EXACT_MAX:
        ref = np.sqrt(_two(dot_fraction(x, x)[0]))
    else:
        ref = np.sqrt(dot_longdouble(x, x)[0])
    if ref > LD(np.finfo(np.float64).max):
        return {"kind": "overflow", "ref": np.inf, "bound": 0.0, "C": C}
    kind = "bound" if (ref == 0 or ref >= LD(2.0) ** -1021) else "subnormal"
    return {"kind": kind, "ref": ref, "bound": SLACK * (C / 2 + 1) * LD(U) * ref, "C": C}


def ratio(dev, case):
    """err / bound of a device scalar against a "bound" case (0 / 0 = 0)."""
    err = abs(LD(dev) - case["ref"])
    if not np.isfinite(dev):
        return float("inf")
    if case["bound"] == 0:
        return 0.0 if err == 0 else float("inf")
    return float(err / case["bound"])


def special_ok(dev, case):
    ref = case["ref"]
    return bool(np.isnan(dev)) if np.isnan(ref) else dev == ref


# ------------------------------------------------ the device order, in fp64
def _butterfly(v):
    """wave_sum on rows of 64 lanes: v += v[lane ^ o], o = 32 .. 1."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    return v[:, 0]


def _block_sums(v, nw):
    """block_sum: the wave sums added to 0 in wave order."""
    w = _butterfly(v.reshape(-1, 64)).reshape(-1, nw)
    s = np.zeros(len(w))
    for i in range(nw):
        s = s + w[:, i]
    return s


def kernel_sum(p):
    """The terms p summed as k_dot_partial + k_reduce sum them on one rank
    (unfused: the products are already rounded)."""
    p = np.asarray(p, np.float64)
    n = len(p)
    g = grid(n)
    T = VB * g
    m = max(-(-n // T), 1)
    q = np.zeros(m * T)
    q[:n] = p
    s = np.zeros(T)
    for row in q.reshape(m, T):
        s = s + row
    part = _block_sums(s, VB // 64)  # g partials
    k = -(-g // RB)
    q = np.zeros(k * RB)
    q[:g] = part
    s = np.zeros(RB)
    for row in q.reshape(k, RB):
        s = s + row
    return float(_block_sums(s, RB // 64)[0])


def split(n, R):
    """createMPI((None, n))'s ownership ranges."""
    cnt = [n // R + (1 if r < n % R else 0) for r in range(R)]
    off = np.concatenate([[0], np.cumsum(cnt)])
    return [(int(off[r]), int(off[r + 1])) for r in range(R)]


def kernel_dot(x, y, R=1, plant=None):
    """dot(x, y) in the device's order on R ranks (partials added in rank
    order), with one planted error: "drop_last", "twice" (entry n // 3 counted
    twice), "f32_term" (the term that float32 rounding moves most, rounded),
    "drop_trip2" (entry 524288, the first of the second grid-stride trip),
    "drop_rank" (rank R // 2's partial, R >= 2)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        p = x * y
    n = len(p)
    if plant == "drop_last":
        p[n - 1] = 0.0
    elif plant == "twice":
        p[n // 3] *= 2.0
    elif plant == "f32_term":
        r = p.astype(np.float32).astype(np.float64)
        k = int(np.argmax(np.abs(r - p)))
        p[k] = r[k]
    elif plant == "drop_trip2":
        p[TRIP] = 0.0
    parts = [kernel_sum(p[lo:hi]) for lo, hi in split(n, R)]
    if plant == "drop_rank":
        parts[R // 2] = 0.0
    s = 0.0
    for t in parts:
        s = s + t
    return s


def kernel_norm(x, R=1, plant=None):
    with np.errstate(over="ignore", invalid="ignore"):
        return math.sqrt(kernel_dot(x, x, R, plant))


# ------------------------------------------------------------- input classes
def probes(n):
    """Entries whose loss the tests plant or that sit on an edge of the code:
    pinned to the largest magnitude by x_spread so that none can hide."""
    return sorted({k for k in (0, 63, 255, n // 3, n - 1, TRIP) if 0 <= k < n})


def x_uniform(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n)


def x_spread(n, seed):
    """+-m 2^e, m in [1, 2), e uniform in [-40, 40]; the probes at e = 40."""
    rng = np.random.default_rng(seed)
    e = rng.integers(-40, 41, n)
    if n:
        e[probes(n)] = 40
    return np.ldexp(rng.uniform(1, 2, n) * rng.choice([-1.0, 1.0], n), e)


def x_constant(n, c=0.7):
    return np.full(n, c)


def xy_cancel(n, seed):
    """(x, y) with sum x_i y_i below 1e-12 sum |x_i y_i| (n >= 2): entry
    i + n // 2 of y undoes term i, so the two meet only late in the reduction
    (other threads, other blocks, other ranks).  cancels() checks the claim."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
    y = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
    h = n // 2
    y[h:2 * h] = -(x[:h] * y[:h]) / x[h:2 * h]
    if n & 1:  # the last two entries undo term h - 1 by halves (no zero term: a lost entry must show)
        y[2 * h - 1] = -(x[h - 1] * y[h - 1]) / x[2 * h - 1] / 2
        y[n - 1] = -(x[h - 1] * y[h - 1]) / x[n - 1] / 2
    return x, y


def cancels(x, y):
    s, a = dot_exact(x, y)
    return abs(s) <= LD(1e-12) * a and a > 0


def dot_inputs(n, seed=11):
    """{class: (x, y)} for dot at size n ("small": U(-1, 1) 2^-20, terms below
    1e-12 -- the class on which an absolute tolerance sees nothing)."""
    out = {"uniform": (x_uniform(n, seed), x_uniform(n, seed + 1)),
           "small": (x_uniform(n, seed + 5) * 2.0 ** -20, x_uniform(n, seed + 6) * 2.0 ** -20),
           "spread": (x_spread(n, seed + 2), x_spread(n, seed + 3)),
           "constant": (x_constant(n, 0.7), x_constant(n, 1.3))}
    if n >= 2:
        out["cancel"] = xy_cancel(n, seed + 4)
    return out
