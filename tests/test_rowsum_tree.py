"""The wave sum of the symmetric SpMV kernels restated in numpy, lane by lane
(kle_sym_dev.hpp wsum3_dpp): quad swaps, half-row and row mirrors, the two
row broadcasts, lane 63 read back -- the balanced 64-lane tree of lane pairs,
quads, 8-groups, 16-lane rows, row pairs and both halves.

What the helper's change rests on, shown here on uniform random parts, parts
over 16 decades, one huge part, a NaN, all -0.0 and a comb of one nonzero per
7 (signed zeros in the partial sums):
  * the four full-row stages write every lane, so what their DPP moves would
    have left in an unwritten lane (the "old" operand) never reaches a sum:
    any old value gives the same bits;
  * the two row broadcasts do leave lanes unwritten that are added to
    afterwards: lane 63's sum is the same whatever those lanes hold, but the
    lanes themselves are not -- which is why they keep a defined (zero) old;
  * the tree is the grouping said above, and a schedule with one wrong pairing
    (quads paired across the 8-groups) gives other last bits.
This is a restatement of what the instructions are meant to do -- it proves
the argument, not the hardware: that the device code does this is held by the
digests of tests/test_gpu_rowsum_bits.py.
"""
import numpy as np
import pytest

L = np.arange(64)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---- the lanes a DPP move reads from
QUAD_1032 = L ^ 1
QUAD_2301 = L ^ 2
HALF_MIRROR = (L & ~7) | (7 - (L & 7))
MIRROR = (L & ~15) | (15 - (L & 15))
FULL = (QUAD_1032, QUAD_2301, HALF_MIRROR, MIRROR)


def dpp(a, src, written, old):
    """A DPP move: written lanes take a[src], the others keep old."""
    return np.where(written, a[src], old)


def wsum(a, full_old=None, bcast_old=0.0, stages=FULL):
    """wsum3_dpp for one value (every add is own + moved): all 64 lanes after
    the last stage.  full_old / bcast_old: what the moves' old operand holds
    (None: the source itself, as the helper passed it before)."""
    a = a.copy()
    every = np.ones(64, bool)
    for src in stages:
        a = a + dpp(a, src, every, a if full_old is None else full_old)
    rows = L >> 4
    a = a + dpp(a, (L & ~15) - 1, (rows == 1) | (rows == 3), bcast_old)  # row_bcast15
    a = a + dpp(a, np.full(64, 31), rows >= 2, bcast_old)  # row_bcast31
    return a


def parts(kind, k, rng):
    x = rng.uniform(-1.0, 1.0, (k, 64))
    if kind == "decades":
        x = x * 10.0 ** rng.uniform(-8.0, 8.0, (k, 64))
    elif kind == "huge":
        x[:, 21] = 1e200
    elif kind == "nan":
        x[:, 32] = np.nan
    elif kind == "negzero":
        x = np.full((k, 64), -0.0)
    elif kind == "comb":
        x = np.where(np.arange(k * 64).reshape(k, 64) % 7 == 0, x, rng.choice([0.0, -0.0], (k, 64)))
    return x


KINDS = ["uniform", "decades", "huge", "nan", "negzero", "comb"]


@pytest.mark.parametrize("kind", KINDS)
def test_full_row_stages_need_no_old_operand(kind):
    rng = np.random.default_rng(KINDS.index(kind))
    for v in parts(kind, 40, rng):
        want = wsum(v)
        for old in (0.0, -0.0, 1e300, np.nan, rng.uniform(-1, 1, 64)):
            assert np.array_equal(bits(wsum(v, full_old=old)), bits(want)), kind


@pytest.mark.parametrize("kind", KINDS)
def test_row_broadcasts_keep_lane_63_but_not_the_unwritten_lanes(kind):
    rng = np.random.default_rng(10 + KINDS.index(kind))
    for v in parts(kind, 40, rng):
        want = wsum(v)
        other = wsum(v, bcast_old=rng.uniform(1.0, 2.0, 64))
        assert bits(other[63:]) == bits(want[63:]), kind
        if kind == "uniform":  # (rows 0 and 2 took the old value into their sums)
            assert (bits(other[:16]) != bits(want[:16])).any()


def test_the_tree_is_the_sum_by_groups():
    """Pairs, quads, 8, 16, 32, 64: lane 63's sum is the pairwise tree's."""
    rng = np.random.default_rng(1)
    for kind in KINDS:
        for v in parts(kind, 20, rng):
            a = v.copy()
            while len(a) > 1:
                a = a[1::2] + a[0::2]
            assert bits(wsum(v)[63:]) == bits(a), kind


def test_a_wrong_pairing_changes_bits():
    """The mirrors swapped (quads paired across the 8-groups first): still
    every value's sum, other last bits on parts spread over 16 decades."""
    rng = np.random.default_rng(7)
    x = parts("decades", 240, rng)
    wrong = (QUAD_1032, QUAD_2301, (L & ~15) | ((L & 15) ^ 11), HALF_MIRROR)  # lane l with l ^ 8 (mirrored), then l ^ 4
    got = np.array([wsum(v, stages=wrong)[63] for v in x])
    want = np.array([wsum(v)[63] for v in x])
    assert (np.abs(got - want) <= 1e-12 * np.abs(x).max(axis=1)).all()
    assert (bits(got) != bits(want)).any()
    z = parts("negzero", 3, rng)
    assert np.array_equal(bits(np.array([wsum(v, stages=wrong)[63] for v in z])), bits(np.array([wsum(v)[63] for v in z])))
