"""The brick plan's validator on deduplicated value offsets (host only).

kle_brick_plan_box_shared plans an Lx x Ly x Lz box lattice, rewrites the row
descriptors' value offsets the way the row dedup of the brick SpMV does (rows
with equal packed boxes share one copy; every brick's base 0; a unit's second
row anywhere in the array) and runs the validator every brick product passes
before its first launch.  A consistent rewrite is accepted; an offset moved
out of the unique array is refused, and so is a brick whose value base is
not the array's.
"""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    import pynama_amd
    from pynama_amd._lib import load
    return load()


@pytest.mark.parametrize("L,p,dirichlet", [((9, 7, 7), 2, 1), ((17, 17, 9), 4, 1), ((13, 9, 9), 4, 0),
                                           ((15, 15, 8), 7, 1)])
def test_rewritten_offsets_must_stay_inside_the_unique_array(lib, L, p, dirichlet):
    out = (C.c_longlong * 3)()
    assert lib.kle_brick_plan_box_shared(*L, p, dirichlet, 256, 0, out) == 0, lib.kle_last_error()
    rows, kept, total = out[0], out[1], out[2]
    assert 0 < kept <= rows and total > 0 and total % 16 == 0
    if min(L) > 3 * p:
        assert kept < rows  # (interior rows share their boxes)
    # the last row's values moved on by the whole array, and as far as the
    # descriptor's 23 bits go: out of the array, refused; naming what is wrong
    for shift in (int(total // 16), (1 << 22)):
        rc = lib.kle_brick_plan_box_shared(*L, p, dirichlet, 256, shift, out)
        assert rc != 0, shift
        assert b"a row's values" in lib.kle_last_error(), lib.kle_last_error()
    # a brick with a value base of its own (every range still inside a longer
    # array): refused, shared values have the one base 0
    assert lib.kle_brick_plan_box_shared(*L, p, dirichlet, 256, -1, out) != 0
    assert b"a deduplicated row's values" in lib.kle_last_error(), lib.kle_last_error()
    # and the refusals left nothing behind: the consistent rewrite still passes
    assert lib.kle_brick_plan_box_shared(*L, p, dirichlet, 256, 0, out) == 0, lib.kle_last_error()
    assert (out[0], out[1], out[2]) == (rows, kept, total)
