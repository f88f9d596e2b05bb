"""The Vec surface (pynama_amd/petsc.py Vec over kle_core.hip's vector kernels,
halo_exchange and k_halo_pack) against the references of tests/vec_ref.py:
bit equality with numpy where an operation rounds once, the counted bounds of
vec_ref's docstring for axpy / aypx / waxpy / dot / norm, IEEE rules for NaN
and infinities, PETSc's rules for aliasing, repeated indices and ghost reads.
Every case prints a VECREF line with its err / bound.

Sizes (vec_ref.SIZES): 0, 1; 63, 64, 65 (one wave); 255, 256, 257 (one block);
1023, 1024, 1025 (four blocks; k_reduce's second wave); 10001; 524287, 524288,
524289 (the grid cap of 2048 blocks, the first entry of a second grid-stride
trip); 1048833 (two full trips and a partial block).  8 MB per vector at most.

Several ranks (all on one GPU, as tests/test_gpu_multirank.py runs them): one
spawned run per configuration, shared by its tests -- slab boxes on 2 and 3
ranks, the perturbed Gmsh mesh under the inertial partitioner on 3 and 4
ranks, and the 2-rank box over the IPC transport."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

import vec_ref as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = V.LD
A_VALUES = [0.0, 1.0, -1.0, 1.0 / 3.0, 2.0 ** -30, 1e300]
_RATIOS = {}


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


def _vec(pa, a):
    return pa.petsc.Vec().createWithArray(np.asarray(a, np.float64))


def _report(op, n, what, r):
    key = (op, n)
    _RATIOS[key] = max(_RATIOS.get(key, 0.0), r)
    print(f"VECREF {op} n={n} {what}: err/bound={r:.3f}")


def _bits(dev, ref, what):
    assert V.same_bits(dev, ref), (what, V.first_diff(dev, ref))


def _check_scalar(op, n, what, dev, case):
    if case["kind"] == "bound":
        r = V.ratio(dev, case)
        _report(op, n, f"{what} C={case['C']}", r)
        assert r <= 1.0, (op, n, what, dev, float(case["ref"]), r)
    elif case["kind"] in ("exact-special", "overflow"):
        print(f"VECREF {op} n={n} {what}: {case['kind']}, device {dev}, expected {case['ref']}")
        assert V.special_ok(dev, case), (op, n, what, dev, case["ref"])
    else:  # named, not bounded: the ulp model does not apply
        print(f"VECREF {op} n={n} {what}: {case['kind']} (no ulp bound), device {dev}")
        assert np.isfinite(dev)


# ------------------------------------------------------------------ dot, norm
@pytest.mark.parametrize("n", V.SIZES)
def test_dot_and_norm(pa, n):
    for name, (x, y) in V.dot_inputs(n).items():
        if name == "cancel":
            assert V.cancels(x, y), n
        vx, vy = _vec(pa, x), _vec(pa, y)
        _check_scalar("dot", n, name, vx.dot(vy), V.dot_case(x, y))
        _check_scalar("dot", n, name + " (y, x)", vy.dot(vx), V.dot_case(x, y))
        _check_scalar("norm", n, name, vx.norm(), V.norm_case(x))
        assert vx.norm("2") == vx.norm(None) == vx.norm()


@pytest.mark.parametrize("n", [1, 65, 1025, 10001, V.TRIP + 1])
@pytest.mark.parametrize("e", [600, -600])
def test_norm_of_scaled_vectors(pa, n, e):
    """Entries near 2^+-600: the squares overflow (vanish), the norm does not."""
    x = V.x_uniform(n, 21) * 2.0 ** e
    c = V.norm_case(x)
    assert c["kind"] == "bound"
    _check_scalar("norm", n, f"uniform 2^{e}", _vec(pa, x).norm(), c)


def test_norm_at_the_overflow_edge(pa):
    x = V.x_uniform(1025, 21)
    c = V.norm_case(x * 2.0 ** 1000)  # about 2^1004: representable, the reference says which
    _check_scalar("norm", 1025, "uniform 2^1000", _vec(pa, x * 2.0 ** 1000).norm(), c)
    c = V.norm_case(x * 2.0 ** 1020)
    assert c["kind"] == "overflow"
    _check_scalar("norm", 1025, "uniform 2^1020", _vec(pa, x * 2.0 ** 1020).norm(), c)
    # the scaled path's own edges: all zeros, a NaN, an infinity among huge entries
    z = _vec(pa, np.zeros(1025))
    assert z.norm() == 0.0 and np.signbit(z.norm()) == False  # noqa: E712
    y = x * 2.0 ** 600
    y[1024] = np.nan
    assert np.isnan(_vec(pa, y).norm())
    y[1024] = -np.inf
    assert _vec(pa, y).norm() == np.inf
    tiny = np.full(300, 2.0 ** -1060)  # subnormal entries: the norm, 2^-1060 sqrt(300), is one too
    c = V.norm_case(tiny)
    assert c["kind"] == "subnormal"
    d = _vec(pa, tiny).norm()
    print(f"VECREF norm n=300 subnormal entries (named, no ulp bound): device {d}, reference {float(c['ref'])}")
    assert abs(d - float(c["ref"])) <= 2.0 ** -1074 * 2


@pytest.mark.parametrize("n", [1, 64, 256, 257, 10001, V.TRIP + 1])
def test_special_values_in_reductions(pa, n):
    x0, y0 = V.x_uniform(n, 31), V.x_uniform(n, 32)
    for pos in [p for p in (0, 63, 255, n - 1, V.TRIP) if p < n]:
        x = x0.copy()
        x[pos] = np.nan
        vx, vy = _vec(pa, x), _vec(pa, y0)
        assert np.isnan(vx.dot(vy)) and np.isnan(vy.dot(vx)) and np.isnan(vx.norm()), (n, pos)
        x[pos] = np.inf
        y = y0.copy()
        y[pos] = abs(y[pos])
        vx, vy = _vec(pa, x), _vec(pa, y)
        c = V.dot_case(x, y)
        assert c["ref"] == np.inf
        assert vx.dot(vy) == np.inf and vx.norm() == np.inf, (n, pos)
        y[pos] = -y[pos]
        assert _vec(pa, x).dot(_vec(pa, y)) == -np.inf, (n, pos)
        if n > 1:
            q = (pos + n // 2 + 1) % n if (pos + n // 2 + 1) % n != pos else (pos + 1) % n
            x[q], y[q], y[pos] = np.inf, 1.0, -1.0  # +inf and -inf among the terms
            assert np.isnan(V.dot_case(x, y)["ref"])
            assert np.isnan(_vec(pa, x).dot(_vec(pa, y))), (n, pos, q)
    print(f"VECREF special n={n}: NaN, +inf, -inf, inf - inf as IEEE has them")


# ---------------------------------------------------------------- element-wise
@pytest.mark.parametrize("n", V.SIZES)
def test_elementwise(pa, n):
    x, y = V.x_uniform(n, 41), V.x_uniform(n, 42)
    if n > 3:
        x[1], y[2], x[n - 1] = 0.0, -0.0, -0.0
    vx, vy = _vec(pa, x), _vec(pa, y)
    w = vx.duplicate()
    assert w.getSizes() == (n, n)
    _bits(w.getArray(), np.zeros(n), "duplicate is zero")
    for a in A_VALUES + [-0.0, np.inf]:
        w.set(a)
        _bits(w.getArray(), np.full(n, a), f"set {a}")
    with np.errstate(over="ignore", invalid="ignore"):
        for a in A_VALUES:
            w = vx.copy()
            w.scale(a)
            _bits(w.getArray(), x * a, f"scale {a}")
            # y += a x; y = x + a y; w = a x + y
            ref, b = V.axpy(a, x, y)
            w = vy.copy()
            w.axpy(a, vx)
            _report("axpy", n, f"a={a:.3g}", V.worst(w.getArray(), ref, b)[0])
            assert V.worst(w.getArray(), ref, b)[0] <= 1.0, (n, a)
            ref, b = V.axpy(a, y, x)
            w = vy.copy()
            w.aypx(a, vx)
            _report("aypx", n, f"b={a:.3g}", V.worst(w.getArray(), ref, b)[0])
            assert V.worst(w.getArray(), ref, b)[0] <= 1.0, (n, a)
            ref, b = V.axpy(a, x, y)
            w.set(7.0)
            w.waxpy(a, vx, vy)
            _report("waxpy", n, f"a={a:.3g}", V.worst(w.getArray(), ref, b)[0])
            assert V.worst(w.getArray(), ref, b)[0] <= 1.0, (n, a)
    big = _vec(pa, x * 1e10)
    big.scale(1e300)  # the product overflows: inf with x's sign, 0 stays a signed 0
    with np.errstate(over="ignore"):
        _bits(big.getArray(), x * 1e10 * 1e300, "scale overflow")
    w = vx.duplicate()
    w.pointwiseMult(vx, vy)
    _bits(w.getArray(), x * y, "pointwiseMult")
    r = vx.copy()
    r.reciprocal()
    _bits(r.getArray(), V.reciprocal(x), "reciprocal")
    c = vx.duplicate()
    assert vx.copy(c) is c
    _bits(c.getArray(), x, "copy(result)")
    _bits(vx.getArray(), x, "x untouched")
    _bits(vy.getArray(), y, "y untouched")
    print(f"VECREF bits n={n}: set, scale, pointwiseMult, reciprocal, copy equal numpy's bits")


@pytest.mark.parametrize("n", V.SIZES)
@pytest.mark.parametrize("dim", [2, 3])
def test_tensor_square(pa, n, dim):
    """Nodes = n up to 10001; above, n // 6 nodes (the output stays within 8 MB)."""
    from pynama_amd._lib import call
    nodes = n if n <= 10001 else n // 6
    ds = 3 if dim == 2 else 6
    v = V.x_uniform(nodes * dim, 51)
    vv, out = _vec(pa, v), _vec(pa, np.full(nodes * ds, 9.0))
    call("kle_vec_tensor_square", vv._h, dim, out._h)
    _bits(out.getArray(), V.tensor_square(v, dim), f"tensor square dim {dim}")
    _bits(vv.getArray(), v, "input untouched")
    print(f"VECREF bits nodes={nodes} dim={dim}: tensor square equals numpy's bits in computeVtensV's order")


def test_subnormals_and_signed_zeros(pa):
    rng = np.random.default_rng(61)
    s = rng.integers(1, 2 ** 52, 1025).astype(np.float64) * 2.0 ** -1074 * rng.choice([-1.0, 1.0], 1025)
    t = rng.integers(1, 2 ** 51, 1025).astype(np.float64) * 2.0 ** -1074
    assert np.all(np.abs(s) < 2.0 ** -1022) and np.all(s != 0)
    vs, vt = _vec(pa, s), _vec(pa, t)
    _bits(vs.getArray(), s, "upload")
    for a in (1.0, 0.5, -0.25, 2.0 ** 30):
        w = vs.copy()
        w.scale(a)
        _bits(w.getArray(), s * a, f"subnormal scale {a}")
    w = vs.duplicate()
    w.pointwiseMult(vs, _vec(pa, np.full(1025, 0.5)))
    _bits(w.getArray(), s * 0.5, "subnormal pointwiseMult")
    w = vt.copy()
    w.axpy(1.0, vs)  # both steps exact: the sum of two subnormals
    _bits(w.getArray(), s + t, "subnormal axpy")
    w.waxpy(-1.0, vs, vt)
    _bits(w.getArray(), t - s, "subnormal waxpy")
    r = vs.copy()
    r.reciprocal()
    with np.errstate(over="ignore"):
        _bits(r.getArray(), 1.0 / s, "subnormal reciprocal")
    z = _vec(pa, np.array([np.inf, -np.inf, 1.0, -0.0, 0.0]))
    z.scale(0.0)
    got = z.getArray()
    assert np.isnan(got[0]) and np.isnan(got[1])
    _bits(got[2:], [0.0, -0.0, 0.0], "scale(0.0)")
    z.set(-0.0)
    assert np.all(np.signbit(z.getArray()))
    z.zeroEntries()
    assert not np.any(np.signbit(z.getArray()))
    r = _vec(pa, np.array([2.0, 0.0, -0.0, -4.0, np.inf, -np.inf, np.nan]))
    r.reciprocal()
    _bits(r.getArray(), [0.5, 0.0, -0.0, -0.25, 0.0, -0.0, np.nan], "reciprocal keeps the zeros as they are")


def test_python_spellings(pa):
    P = pa.petsc
    n = 1025
    x, y = V.x_uniform(n, 71), V.x_uniform(n, 72)
    vx, vy = _vec(pa, x), _vec(pa, y)
    _bits((vx + vy).getArray(), x + y, "+")  # 1.0 y is exact, the sum rounds once
    _bits((vx - vy).getArray(), x - y, "-")
    _bits((vx * vy).getArray(), x * y, "Vec * Vec")
    _bits((vx * (1.0 / 3.0)).getArray(), x * (1.0 / 3.0), "Vec * scalar")
    _bits(((1.0 / 3.0) * vx).getArray(), x * (1.0 / 3.0), "scalar * Vec")
    w = vx.copy()
    keep = w
    w *= -0.7
    assert w is keep
    _bits(w.getArray(), x * -0.7, "*=")
    d = vx.duplicate()
    assert d.getSizes() == vx.getSizes() and d.getOwnershipRange() == (0, n)
    _bits(d.getArray(), np.zeros(n), "duplicate")
    vx.copy(d)
    d.zeroEntries()
    _bits(d.getArray(), np.zeros(n), "zeroEntries")
    a2 = V.x_uniform(35, 73).reshape(5, 7)
    v2 = P.Vec().createWithArray(a2)
    assert v2.getSizes() == (35, 35)
    _bits(v2.getArray(), a2.ravel(), "createWithArray 2-D")
    _bits(np.asarray(v2), a2.ravel(), "__array__")
    _bits(vx.getArray(), x, "operands untouched")
    e = P.Vec().createWithArray(np.zeros(0))
    assert e.getSizes() == (0, 0) and e.dot(e) == 0.0 and e.norm() == 0.0 and len(e.getArray()) == 0
    e.scale(2.0)
    e.axpy(1.0, e.duplicate())
    print("VECREF bits n=1025: + - * (Vec, scalar, reflected) *= copy(result) duplicate zeroEntries "
          "createWithArray(2-D) equal numpy's bits")


# -------------------------------------------------------------------- aliasing
@pytest.mark.parametrize("n", [1, 257, 10001, V.TRIP + 1])
def test_pointwise_mult_takes_aliased_operands(pa, n):
    x, y = V.x_uniform(n, 81), V.x_uniform(n, 82)
    w, vy = _vec(pa, x), _vec(pa, y)
    w.pointwiseMult(w, vy)
    _bits(w.getArray(), x * y, "w = w * y")
    w, vx = _vec(pa, y), _vec(pa, x)
    w.pointwiseMult(vx, w)
    _bits(w.getArray(), x * y, "w = x * w")
    w = _vec(pa, x)
    w.pointwiseMult(w, w)
    _bits(w.getArray(), x * x, "w = w * w")
    _bits((vx * vx).getArray(), x * x, "x * x")
    _bits(vx.getArray(), x, "x untouched")
    print(f"VECREF alias n={n}: pointwiseMult with w = x, w = y, w = x = y equals numpy's bits")


def test_axpy_family_refuses_aliased_output(pa):
    Error = pa.petsc.Error
    n = 1025
    x, y = V.x_uniform(n, 83), V.x_uniform(n, 84)
    vx, vy = _vec(pa, x), _vec(pa, y)
    w = _vec(pa, x + 1.0)
    for what, f, v, ref in (("y.axpy(a, y)", lambda: vy.axpy(0.5, vy), vy, y),
                            ("y.aypx(b, y)", lambda: vy.aypx(0.5, vy), vy, y),
                            ("w.waxpy(a, w, y)", lambda: w.waxpy(0.5, w, vy), w, x + 1.0),
                            ("w.waxpy(a, x, w)", lambda: w.waxpy(0.5, vx, w), w, x + 1.0)):
        with pytest.raises(Error) as ei:
            f()
        assert ei.value.ierr == 61, (what, ei.value)
        _bits(v.getArray(), ref, what + " left the vector unchanged")
    w.waxpy(0.5, vx, vx)  # the inputs may be one vector
    ref, b = V.axpy(0.5, x, x)
    assert V.worst(w.getArray(), ref, b)[0] <= 1.0
    print("VECREF alias n=1025: axpy, aypx, waxpy with the output among the inputs raise 61, vectors unchanged")


# ---------------------------------------------------------- setValues, getValues
def test_set_values_and_get_values(pa):
    Error = pa.petsc.Error
    n = 3000
    base = V.x_uniform(n, 91)
    v = _vec(pa, base)
    rng = np.random.default_rng(92)
    idx = rng.permutation(n)[:700]
    vals = V.x_uniform(700, 93)
    v.setValues(idx, vals)
    ref = base.copy()
    ref[idx] = vals
    _bits(v.getArray(), ref, "insert, unique indices")
    v.setValues(set(), [])
    v.setValues([], [], addv=True)
    v.setValues(np.zeros(0, np.int64), np.zeros(0))
    assert len(v.getValues([])) == 0
    _bits(v.getArray(), ref, "empty lists")
    v.setValues([5, 6, 2999], -0.0)  # a scalar is broadcast
    ref[[5, 6, 2999]] = -0.0
    v.setValue(0, 4.5)
    v.setValue(0, 0.25, addv=True)
    ref[0] = 4.75
    _bits(v.getArray(), ref, "scalar broadcast, setValue")
    # add with repeats: np.add.at applies them in list order
    ia = rng.integers(0, 50, 400)
    va = V.x_uniform(400, 94) * 10.0 ** rng.integers(-8, 8, 400)
    v.setValues(ia, va, addv=True)
    np.add.at(ref, ia, va)
    _bits(v.getArray(), ref, "add with repeats, list order")
    # getValues in any order, with repeats
    ig = rng.integers(0, n, 5000)
    _bits(v.getValues(ig), ref[ig], "getValues")
    _bits(v.getValues([2999, 0, 2999]), ref[[2999, 0, 2999]], "getValues, ends")
    # refused before anything is written: -1, n, and both after valid entries
    for bad in ([-1], [n], [3, 4, -1], [3, n, 4], [2 ** 40]):
        for addv in (False, True):
            with pytest.raises(Error) as ei:
                v.setValues(bad, np.full(len(bad), 99.0), addv=addv)
            assert ei.value.ierr == 63, (bad, ei.value)
        with pytest.raises(Error) as ei:
            v.getValues(bad)
        assert ei.value.ierr == 63, (bad, ei.value)
    _bits(v.getArray(), ref, "refused calls changed nothing")
    print("VECREF values n=3000: insert, add in list order, broadcast, empty lists, getValues exact; "
          "-1, n, 2^40 raise 63 and write nothing")


def test_insert_with_repeated_indices_keeps_the_last_value(pa):
    """VecSetValues(INSERT_VALUES): the last value given for an index stays
    (boundary lists repeat shared nodes)."""
    n = 4000
    base = V.x_uniform(n, 95)
    v = _vec(pa, base)
    ref = base.copy()
    wrong = []
    for k in range(20):
        v.setValues([7 + k, 7 + k, 7 + k], [1.0 + k, 2.0 + k, 3.0 + k])
        ref[7 + k] = 3.0 + k
        got = v.getValues([7 + k])[0]
        if got != 3.0 + k:
            wrong.append((k, got))
    print(f"VECREF insert-repeat: {len(wrong)} of 20 triple inserts kept another value than the last: {wrong[:5]}")
    assert not wrong
    rng = np.random.default_rng(96)
    idx = np.concatenate([np.arange(1000, 2500), np.arange(1000, 2500)])[rng.permutation(3000)]
    vals = V.x_uniform(3000, 97)
    v.setValues(idx, vals)
    for i, a in zip(idx, vals):  # list order: the later one stays
        ref[i] = a
    bad = int(np.sum(v.getArray() != ref))
    print(f"VECREF insert-repeat: {bad} of 1500 doubled indices hold the earlier value")
    _bits(v.getArray(), ref, "3000-entry list, every index twice")
    v.setValues([3999, 0, 3999, 0, 1], [1.0, 2.0, 3.0, 4.0, 5.0])
    ref[[3999, 0, 1]] = [3.0, 4.0, 5.0]
    _bits(v.getArray(), ref, "unsorted repeats")


def test_refusals(pa):
    from pynama_amd._lib import call
    Error = pa.petsc.Error
    a, b = _vec(pa, np.ones(12)), _vec(pa, np.ones(13))
    c = a.duplicate()
    for what, f in (("axpy", lambda: a.axpy(1.0, b)), ("aypx", lambda: a.aypx(1.0, b)),
                    ("waxpy x", lambda: c.waxpy(1.0, b, a)), ("waxpy y", lambda: c.waxpy(1.0, a, b)),
                    ("waxpy w", lambda: b.waxpy(1.0, a, c)), ("pointwiseMult", lambda: c.pointwiseMult(a, b)),
                    ("pointwiseMult w", lambda: b.pointwiseMult(a, c)), ("dot", lambda: a.dot(b)),
                    ("copy", lambda: a.copy(b)), ("setArray", lambda: a.setArray(np.ones(13)))):
        with pytest.raises(Error) as ei:
            f()
        assert ei.value.ierr == 60, (what, ei.value)
    _bits(a.getArray(), np.ones(12), "a unchanged")
    _bits(b.getArray(), np.ones(13), "b unchanged")
    _bits(c.getArray(), np.zeros(12), "c unchanged")
    out3, out6, out5 = _vec(pa, np.zeros(18)), _vec(pa, np.zeros(24)), _vec(pa, np.zeros(5))
    for what, args in (("dim 1", (a._h, 1, out3._h)), ("dim 4", (a._h, 4, out3._h)), ("dim 0", (a._h, 0, out3._h)),
                       ("2-D output of the wrong size", (a._h, 2, out6._h)),
                       ("3-D output of the wrong size", (a._h, 3, out3._h)),
                       ("input no multiple of dim", (b._h, 2, out5._h))):
        with pytest.raises(Error) as ei:
            call("kle_vec_tensor_square", *args)
        assert ei.value.ierr == 62, (what, ei.value)
    call("kle_vec_tensor_square", a._h, 2, out3._h)
    call("kle_vec_tensor_square", a._h, 3, out6._h)
    for t in (1, "1", "inf", 0, 3):
        with pytest.raises(Error) as ei:
            a.norm(t)
        assert ei.value.ierr == 56, t
    print("VECREF refusals: sizes 60, tensor square dim / output size 62, other norms 56")


def test_worst_ratio_table(pa):
    """The table of DESIGN.md: the worst err / bound per operation and size of
    the cases run so far (run last in this file's single-rank part)."""
    for (op, n), r in sorted(_RATIOS.items()):
        print(f"VECREF worst {op} n={n}: {r:.3f}")
        assert r <= 1.0


# ------------------------------------------------------------- several ranks
CONFIGS = {
    "box2_host": dict(size=2, nelem=[3, 2, 4], ngl=4, gmsh=False, transport="host"),
    "box3_host": dict(size=3, nelem=[2, 3, 3], ngl=3, gmsh=False, transport="host"),
    "gmsh3_inertial": dict(size=3, nelem=[3, 4, 4], ngl=3, gmsh=True, transport="host"),
    "gmsh4_inertial": dict(size=4, nelem=[4, 4, 4], ngl=3, gmsh=True, transport="host"),
    "box2_ipc": dict(size=2, nelem=[3, 2, 4], ngl=4, gmsh=False, transport="ipc"),
}
POISON = -777.0
_RUNS = {}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _global_inputs(n):
    """{name: (x, y)} of global length n, the same on every rank."""
    out = V.dot_inputs(n, seed=111)
    x = V.x_uniform(n, 117)
    out["norm 2^600"] = (x * 2.0 ** 600, x * 2.0 ** 600)
    out["norm 2^-600"] = (x * 2.0 ** -600, x * 2.0 ** -600)
    out["zero"] = (np.zeros(n), x)
    xn = x.copy()
    xn[n - 1] = np.nan  # on the last rank that owns anything
    out["nan"] = (xn, x)
    return out


def _dots(P, make, n):
    """{name: (dot, norm of x)} with `make(global array) -> Vec` of this rank."""
    res = {}
    for name, (x, y) in _global_inputs(n).items():
        vx, vy = make(x), make(y)
        with np.errstate(over="ignore", invalid="ignore"):
            res[name] = (vx.dot(vy), vx.norm())
    return res


def _rank_worker(rank, size, port, cfg, msh, q):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), KLE_TRANSPORT=cfg["transport"],
                      RANK=str(rank), WORLD_SIZE=str(size), KLE_COMM_TIMEOUT_S="30")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=size)
    try:
        import pynama_amd as pa
        from pynama_amd._lib import call, load
        P = pa.petsc
        ctx = pa.get_ctx()
        lib = load()
        lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        lib.hipMemcpy.restype = C.c_int
        if cfg["gmsh"]:
            mesh = pa.mesh.UnstructuredMesh.from_gmsh(msh, cfg["ngl"], rank, size, partitioner="inertial")
        else:
            mesh = pa.BoxMesh(3, cfg["nelem"], [0, 0, 0], [1, 1, 1], cfg["ngl"], rank, size)
        nb, ne = mesh.node_range
        eb, ee = mesh.ext_range
        ext = mesh.ext_gids()
        ghost = (ext < nb) | (ext >= ne)
        out = {"rank": rank, "N": mesh.N, "node_range": (nb, ne), "ext_range": (eb, ee), "ext": ext,
               "transport": ctx.device_info()["transport"], "kind": mesh.kind, "npeers": len(mesh.peers()),
               "halo": mesh.halo(), "ghost": {}, "getvalues": {}}

        def raw(v, bs, write=None):
            """The whole ext buffer through the raw device pointer (plain hipMemcpy)."""
            p = C.c_void_p()
            call("kle_vec_device_ptr", v._h, C.byref(p))
            base = (p.value or 0) - (nb - eb) * bs * 8
            n = (ee - eb) * bs
            ctx.synchronize()
            if write is not None:
                lo, hi, val = write
                buf = np.full(hi - lo, val)
                if hi > lo:
                    assert lib.hipMemcpy(C.c_void_p(base + lo * 8), buf.ctypes.data_as(C.c_void_p), 8 * (hi - lo), 1) == 0
                return None
            host = np.zeros(n)
            if n:
                assert lib.hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(base), 8 * n, 2) == 0
            return host

        for bs in (1, 3, 6):
            v = P.Vec.fromMesh(mesh, bs)
            lo, hi = v.getOwnershipRange()
            assert (lo, hi) == (nb * bs, ne * bs) and v.getSize() == mesh.N * bs
            glo, ntot = (nb - eb) * bs, (ee - eb) * bs
            raw(v, bs, write=(0, glo, POISON))
            raw(v, bs, write=(glo + hi - lo, ntot, POISON))
            v.setArray(np.arange(lo, hi, dtype=np.float64) + 0.25)
            before = raw(v, bs)
            v.ghostUpdate()
            after1 = raw(v, bs)
            d = v.duplicate()  # a duplicate carries the halo and the ghost map
            d.setArray(-(np.arange(lo, hi, dtype=np.float64) + 1000.5))
            d.ghostUpdate()
            v.setArray(np.arange(lo, hi, dtype=np.float64) * 2.0 + 1000.5)
            stale = raw(v, bs)
            v.ghostUpdate()
            v.ghostUpdate()  # twice in a row: the same
            after2 = raw(v, bs)
            out["ghost"][bs] = {"before": before, "after1": after1, "stale": stale, "after2": after2,
                                "dup": raw(d, bs)}
            # getValues: every ghost entry by its global index, then a shuffled mix with repeats
            gidx = (ext[ghost][:, None] * bs + np.arange(bs)).ravel()
            g = {"gidx": gidx}
            try:
                g["ghosts"] = v.getValues(gidx)
            except P.Error as e:
                g["ghosts"] = ("error", e.ierr, str(e))
            rng = np.random.default_rng(5 + rank)
            allidx = (ext[:, None] * bs + np.arange(bs)).ravel()
            mix = allidx[rng.integers(0, len(allidx), 300)]
            g["mix"] = mix
            try:
                g["mixed"] = v.getValues(mix)
            except P.Error as e:
                g["mixed"] = ("error", e.ierr, str(e))
            # indices that are neither owned nor ghosts: inside the ext window of
            # positions (what the code accepted before) and outside it
            mine = set(ext.tolist())
            foreign = [k for k in range(mesh.N) if k not in mine]
            inside = [k for k in foreign if eb <= k < ee]
            g["foreign"] = []
            for k in ([inside[0], inside[-1]] if inside else []) + ([foreign[0], foreign[-1]] if foreign else []):
                try:
                    val = v.getValues([k * bs + bs - 1])
                    g["foreign"].append((k, eb <= k < ee, "value", float(val[0])))
                except P.Error as e:
                    g["foreign"].append((k, eb <= k < ee, "error", e.ierr))
            for k in (-1, mesh.N * bs):
                try:
                    v.getValues([k])
                    g["foreign"].append((k, False, "value", None))
                except P.Error as e:
                    g["foreign"].append((k, False, "error", e.ierr))
            try:  # setValues stays owned-only: a ghost index is refused, nothing written
                if len(gidx):
                    v.setValues([int(gidx[0])], [1.0])
                g["set_ghost"] = "accepted" if len(gidx) else 63
            except P.Error as e:
                g["set_ghost"] = e.ierr
            g["after_refusals"] = raw(v, bs)
            out["getvalues"][bs] = g

        # dot and norm: a mesh vector (bs 3), createMPI((None, n)) and createMPI((7, None))
        def mesh_vec(bs):
            def make(a):
                v = P.Vec.fromMesh(mesh, bs)
                lo, hi = v.getOwnershipRange()
                v.setArray(a[lo:hi])
                return v
            return make

        def mpi_vec(size_arg):
            def make(a):
                v = P.Vec().createMPI(size_arg)
                lo, hi = v.getOwnershipRange()
                v.setArray(a[lo:hi])
                return v
            return make

        out["dots"] = {"mesh3": _dots(P, mesh_vec(3), mesh.N * 3),
                       "mpi_none_2": _dots(P, mpi_vec((None, 2)), 2),
                       "mpi_7_none": _dots(P, mpi_vec((7, None)), 7 * size),
                       "mpi_none_10001": _dots(P, mpi_vec((None, 10001)), 10001)}
        t = P.Vec().createMPI((None, 2))
        out["range_none_2"] = t.getOwnershipRange() + t.getSizes()
        t = P.Vec().createMPI((7, None))
        out["range_7_none"] = t.getOwnershipRange() + t.getSizes()
        q.put(out)
    except Exception:  # report instead of hanging the peers
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc()})
    finally:
        dist.destroy_process_group()


def _ranks(name, tmp_path_factory):
    """One spawned run per configuration, shared by every test of it."""
    if name in _RUNS:
        return _RUNS[name]
    import torch.multiprocessing as mp
    from test_gpu_multirank import _collect
    cfg = CONFIGS[name]
    msh = None
    if cfg["gmsh"]:
        from pynama_amd.meshgen import perturbed_box, write_gmsh
        msh = str(tmp_path_factory.mktemp("vecref") / "part.msh")
        write_gmsh(msh, 3, *perturbed_box(3, cfg["nelem"], seed=31))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, cfg["size"], port, cfg, msh, q)) for r in range(cfg["size"])]
    _RUNS[name] = _collect(procs, q, cfg["size"])
    return _RUNS[name]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_ranks_dot_and_norm(name, tmp_path_factory):
    res = _ranks(name, tmp_path_factory)
    R = CONFIGS[name]["size"]
    assert all(r["transport"] == CONFIGS[name]["transport"] for r in res)
    N = res[0]["N"]
    lay = {"mesh3": (N * 3, max(r["node_range"][1] - r["node_range"][0] for r in res) * 3),
           "mpi_none_2": (2, 1), "mpi_7_none": (7 * R, 7), "mpi_none_10001": (10001, -(-10001 // R))}
    assert [r["range_none_2"] for r in res] == [(lo, hi, hi - lo, 2) for lo, hi in V.split(2, R)]  # ranks that own nothing
    assert [r["range_7_none"] for r in res] == [(7 * k, 7 * k + 7, 7, 7 * R) for k in range(R)]
    for vec, (n, nmax) in lay.items():
        for cls, (x, y) in _global_inputs(n).items():
            d0, n0 = res[0]["dots"][vec][cls]
            for r in res:  # the same bits on every rank
                d, nm = r["dots"][vec][cls]
                assert V.same_bits([d, nm], [d0, n0]), (vec, cls, r["rank"], d, d0, nm, n0)
            if cls == "nan":
                assert np.isnan(d0) and np.isnan(n0), (vec, cls)
                continue
            if cls == "zero":
                assert d0 == 0.0 and n0 == 0.0, (vec, cls, d0, n0)
                continue
            if not cls.startswith("norm"):
                _check_scalar(f"dot R={R} {name} {vec}", n, cls, d0, V.dot_case(x, y, R, nmax))
            _check_scalar(f"norm R={R} {name} {vec}", n, cls, n0, V.norm_case(x, R, nmax))


def _expected_ext(r, bs, f):
    """f(global entry index) at every position of rank r's ext buffer."""
    return f((r["ext"][:, None] * bs + np.arange(bs)).ravel().astype(np.float64))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_ranks_ghost_update(name, tmp_path_factory):
    """Owned entries hold (global entry index + 0.25), the ghost region is
    poisoned through the raw pointer; after ghostUpdate every ghost position
    holds its owner's value (position -> node from mesh.ext_gids()), exactly,
    and the owned part is as it was; new owned values travel with the next
    update.  Read through the raw device pointer, not through getValues."""
    res = _ranks(name, tmp_path_factory)
    cfg = CONFIGS[name]
    assert sum(r["node_range"][1] - r["node_range"][0] for r in res) == res[0]["N"]
    if cfg["gmsh"]:
        assert all(r["kind"] == "unstructured" and r["npeers"] >= 1 for r in res)
        # graph partition: some rank's ghosts are not its neighbouring index ranges
        assert any(not np.array_equal(r["ext"], np.arange(*r["ext_range"])) for r in res)
    elif cfg["size"] == 3:
        assert res[1]["halo"]["lo_rank"] == 0 and res[1]["halo"]["hi_rank"] == 2  # two neighbours
    for r in res:
        nb, ne = r["node_range"]
        ghost = (r["ext"] < nb) | (r["ext"] >= ne)
        assert ghost.sum() > 0 and len(np.unique(r["ext"])) == len(r["ext"])
        for bs in (1, 3, 6):
            g = r["ghost"][bs]
            gm = np.repeat(ghost, bs)
            first = _expected_ext(r, bs, lambda i: i + 0.25)
            second = _expected_ext(r, bs, lambda i: i * 2.0 + 1000.5)
            _bits(g["before"][gm], np.full(gm.sum(), POISON), "poisoned ghosts")
            _bits(g["before"][~gm], first[~gm], "owned before")
            _bits(g["after1"], first, (name, r["rank"], bs, "first update"))
            _bits(g["stale"][gm], first[gm], "ghosts wait for the next update")
            _bits(g["stale"][~gm], second[~gm], "owned rewritten")
            _bits(g["after2"], second, (name, r["rank"], bs, "second update"))
            _bits(g["dup"], -_expected_ext(r, bs, lambda i: i + 1000.5), (name, r["rank"], bs, "duplicate"))
        print(f"VECREF ghostUpdate {name} rank {r['rank']}: {int(ghost.sum())} ghost nodes x bs 1, 3, 6 exact")


@pytest.mark.parametrize("name", list(CONFIGS))
def test_ranks_get_values_on_ghosts(name, tmp_path_factory):
    """getValues by global index: owned and ghost entries return the owner's
    value (graph partitions: through the mesh's ext_gids, not by offset); an
    index that is neither raises 63, inside the old window of positions too."""
    res = _ranks(name, tmp_path_factory)
    for r in res:
        for bs in (1, 3, 6):
            g = r["getvalues"][bs]
            f = lambda i: np.asarray(i, np.float64) * 2.0 + 1000.5  # noqa: E731
            assert not isinstance(g["ghosts"], tuple), (name, r["rank"], bs, g["ghosts"])
            _bits(g["ghosts"], f(g["gidx"]), (name, r["rank"], bs, "ghost entries"))
            assert not isinstance(g["mixed"], tuple), (name, r["rank"], bs, g["mixed"])
            _bits(g["mixed"], f(g["mix"]), (name, r["rank"], bs, "owned and ghost entries, shuffled"))
            assert len(g["foreign"]) >= 3, g["foreign"]
            for k, inside, what, val in g["foreign"]:
                assert (what, val) == ("error", 63), (name, r["rank"], bs, k, inside, what, val)
            assert g["set_ghost"] == 63
            _bits(g["after_refusals"], _expected_ext(r, bs, f), "refusals wrote nothing")
        inside = sum(1 for k, ins, _, _ in r["getvalues"][1]["foreign"] if ins)
        print(f"VECREF getValues {name} rank {r['rank']}: {len(r['getvalues'][1]['gidx'])} ghost nodes read by global "
              f"index, {inside} foreign indices inside the window of positions refused")
