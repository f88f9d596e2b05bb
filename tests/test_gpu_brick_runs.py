"""Runs of same-class units in the brick SpMV (kle_brick.hip, template
parameter G; kle_brick.hpp brick_runs_build).

On a shared (deduplicated) full-layout K the units of a brick whose two rows
have the same packed boxes and value offsets stream identical items.  They are
ordered class by class and handed to the waves in runs of at most
dedup_run_cap units; a wave loads an item's nine values and forms its lanes'
block positions once per run and applies them to each unit in turn.  Which
rows form a unit is untouched, so every row's direct sum keeps its bits, and
the fixed-point region sums do not depend on any order.  So:

  * the product is bitwise that of spmv_brick_dedup 0 (no sharing, no runs)
    under the same tunings -- random x, one huge entry, a NaN -- repeatable,
    and within the longdouble bound of tests/test_gpu_sym_ref.py of the
    exported CSR's product;
  * 30 iterations of the benchmark's KSP give bitwise equal iterates.

The default plan on small meshes gives one brick per CU and only runs of one,
so the split is forced (host count, tests/test_brick_runs_plan.py):
[8,8,4] ngl 3 as one brick -- 812 units in 254 classes of every size 1..8 and
250 units in classes of 9 or more (runs shorter than the cap, equal to it and
classes cut across it; every unit a single item); [8,8,2] ngl 5 as 4 x 4 x 1
bricks -- 3,515 units in 2,184 classes of 1, 2, 4 and 8 (rows of several
passes, shared items, null partners).  Each also with the one-block rows as
items of the bricks and with unpaired rows.  Every case asserts that runs
longer than one were in use: it must not pass by not running the new code.
"""
import numpy as np
import pytest

import sym_ref as S
import test_gpu_brick_dedup as D
import test_gpu_sym_ref as T

pytestmark = pytest.mark.gpu

CASES = {
    "8x8x4-p2": 1 + 100 * 1 + 10000 * 1,
    "8x8x2-p4": 4 + 100 * 4 + 10000 * 1,
}
VARIANTS = {"default": {}, "singles0": {"spmv_brick_singles": 0}, "pair0": {"spmv_brick_pair": 0}}


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


def _runs_in_use(info):
    assert info["dedup"] is True and info["compact"] is False, info
    assert info["dedup_run_cap"] >= 2, info
    assert 0 < info["dedup_runs"] < info["dedup_units"], info
    assert 0 < info["dedup_item_loads"] < info["dedup_items"], info


_ref = {}


def _reference(c, name):
    """The longdouble product of the exported CSR for the random x: once per mesh."""
    if name not in _ref:
        A = S.as_csr(*c["csr"]["K"])
        x = D.inputs(A.n)["random"]
        ref, den = S.reference(A, x)
        q, nT = S.apriori_quantum(A, x)
        _ref[name] = (ref, den, S.restatement(A, x, ref, den), nT * q / 2)
    return _ref[name]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(CASES))
def test_product_with_runs_is_bitwise_the_unshared_streams(pa, name, variant):
    c = D.get_mat(pa, name)
    K = c["mat"].K
    tun = dict(VARIANTS[variant], spmv_brick_split=CASES[name], spmv_brick_compact=0)
    with D.storage(K, spmv_brick_dedup=0, **tun):
        info0 = K.getSymmetricBricks()
        y0 = D.products(K)
    with D.storage(K, spmv_brick_dedup=1, **tun):
        info1 = K.getSymmetricBricks()
        y1 = D.products(K)
    assert info0["dedup"] is False and info0["compact"] is False
    assert all(info0[k] == 0 for k in info0 if k.startswith("dedup_")), info0
    print(f"RUNS {name} {variant}: bricks {info1['bricks']} units {info1['dedup_units']} runs {info1['dedup_runs']} "
          f"cap {info1['dedup_run_cap']} items {info1['dedup_items']} loaded {info1['dedup_item_loads']}")
    _runs_in_use(info1)
    for nm in y0:
        np.testing.assert_array_equal(D._bits(y1[nm]), D._bits(y0[nm]), err_msg=nm)
    assert np.isnan(y0["nan"]).any() and np.isfinite(y0["random"]).all()
    ref, den, rest, allow = _reference(c, name)
    dev, used, aused, ok = T.check_product(y1["random"], ref, den, rest, allow)
    print(f"RUNS {name} {variant}: restatement {rest:.2e} device {dev:.2e} tolerance used {used:.3f} "
          f"allowance used {aused:.3f}")
    assert ok, (dev, rest, used, aused)


def test_units_and_items_are_the_host_count(pa):
    """The device path groups what the host planner entry counts (equal boxes
    mean equal rows on these K: asserted by the stored rows in
    tests/test_gpu_brick_dedup.py)."""
    K = D.get_mat(pa, "8x8x4-p2")["mat"].K
    with D.storage(K, spmv_brick_dedup=1, spmv_brick_compact=0, spmv_brick_split=CASES["8x8x4-p2"]):
        info = K.getSymmetricBricks()
    _runs_in_use(info)
    assert info["bricks"] == 1
    assert (info["dedup_units"], info["dedup_items"]) == (812, 812), info
    # 254 classes: at least one run each, at most one more per cap units
    cap = info["dedup_run_cap"]
    assert 254 <= info["dedup_runs"] <= 254 + 812 // cap, info
    assert info["dedup_item_loads"] == info["dedup_runs"]  # (every unit a single item)


def test_cg_iterates_with_runs_are_bitwise_equal(pa):
    """30 iterations of the benchmark's KSP (single-reduction CG, Jacobi,
    ksp_sr_gather 0) on [8,8,4] ngl 3 as one brick: the iterate and the
    residual norm with runs are those of the unshared stream, bit for bit."""
    from pynama_amd.runtime import get_tuning, set_tuning
    name = "8x8x4-p2"
    K = D.get_mat(pa, name)["mat"].K
    b = np.random.default_rng(3).uniform(-1.0, 1.0, K.createVecRight().getLocalSize())
    out = {}
    keep = get_tuning("ksp_sr_gather")
    set_tuning("ksp_sr_gather", 0)
    try:
        for dd in (0, 1):
            with D.storage(K, spmv_brick_dedup=dd, spmv_brick_compact=0, spmv_brick_split=CASES[name]):
                info = K.getSymmetricBricks()
                if dd:
                    _runs_in_use(info)
                ksp = T.make_ksp(pa, K, "sr", "jacobi")
                bv, x = K.createVecLeft(), K.createVecRight()
                bv.setArray(b)
                ksp.setFixedIterations(30)
                ksp.solve(bv, x)
                assert ksp.getIterationNumber() == 30
                out[dd] = (x.getArray().copy(), ksp.getResidualNorm())
    finally:
        set_tuning("ksp_sr_gather", keep)
    np.testing.assert_array_equal(D._bits(out[1][0]), D._bits(out[0][0]))
    assert out[1][1] == out[0][1]
    assert np.isfinite(out[0][0]).all()
