"""Runs of same-class units of the brick plan (host only; kle_brick.hpp
brick_runs_build, the validator in kle_brick_plan.cpp).

kle_brick_plan_box_runs plans a box lattice under a forced split, rewrites
the value offsets by packed box as the row dedup does, orders each brick's
units class by class and cuts the classes into runs of at most G units, as
the device path does for a shared full-layout K, and runs the validator every
brick product passes before its first launch.  A class: the units whose two
rows have the same packed boxes and value offsets (or both no second row).
The kernel takes a run's items from its first unit and only the region
indices from the others, so the validator's checks are the product's
correctness: every run inside its brick's units, 1 <= count <= G, every unit
in exactly one run, all units of a run of one class.

Lattices: (17,17,9) p 2 as one brick and (33,33,9) p 4 as 4 x 4 x 1 bricks (the
meshes of tests/test_gpu_brick_runs.py), and the benchmark's (81,65,65) p 4 on
256 CUs, planned.
"""
import ctypes as C

import pytest

LATTICES = {
    "17x17x9-p2": ((17, 17, 9), 2, 1 + 100 * 1 + 10000 * 1),
    "33x33x9-p4": ((33, 33, 9), 4, 4 + 100 * 4 + 10000 * 1),
    "81x65x65-p4": ((81, 65, 65), 4, 0),
}
# (units, classes, items) counted from the pairing alone: the same for every G
COUNTS = {"17x17x9-p2": (812, 254, 812), "33x33x9-p4": (3515, 2184, 7685), "81x65x65-p4": (175930, 40443, 502002)}


@pytest.fixture(scope="module")
def lib():
    import pynama_amd
    from pynama_amd._lib import load
    return load()


def plan(lib, name, G, corrupt=0):
    L, p, split = LATTICES[name]
    out = (C.c_longlong * 6)()
    rc = lib.kle_brick_plan_box_runs(*L, p, 1, 256, split, G, corrupt, out)
    return rc, dict(units=out[0], classes=out[1], runs=out[2], items=out[3], item_loads=out[4], largest=out[5])


@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("name", list(LATTICES))
def test_runs_cover_the_units_class_by_class(lib, name, G):
    rc, r = plan(lib, name, G)
    assert rc == 0, lib.kle_last_error()  # (the validator's four checks passed)
    assert (r["units"], r["classes"], r["items"]) == COUNTS[name]
    # at least one run per class, at most one more per G units; none longer than G
    assert r["classes"] <= r["runs"] <= r["classes"] + r["units"] // G
    assert r["runs"] >= -(-r["units"] // G)
    assert 1 <= r["largest"] <= G
    assert r["item_loads"] <= r["items"]
    if G == 1:
        assert r["runs"] == r["units"] and r["item_loads"] == r["items"]
    else:
        assert r["runs"] < r["units"] and r["item_loads"] < r["items"]
        assert r["largest"] == G  # (classes of G units or more exist on each lattice)


def test_single_item_units_load_once_per_run(lib):
    rc, r = plan(lib, "17x17x9-p2", 4)
    assert rc == 0, lib.kle_last_error()
    assert r["item_loads"] == r["runs"] == 349


@pytest.mark.parametrize("name", list(LATTICES))
def test_a_unit_in_a_run_of_another_class_is_refused(lib, name):
    rc, _ = plan(lib, name, 4, corrupt=1)
    assert rc != 0
    assert b"a run's units of different classes" in lib.kle_last_error(), lib.kle_last_error()
    # a run one unit longer than its class: past the cap, into the next class or out of the brick
    rc, _ = plan(lib, name, 4, corrupt=2)
    assert rc != 0
    assert b"a run" in lib.kle_last_error(), lib.kle_last_error()
    # the refusals left nothing behind
    rc, r = plan(lib, name, 4)
    assert rc == 0 and (r["units"], r["classes"], r["items"]) == COUNTS[name]


def test_benchmark_lattice_keeps_the_reuse(lib):
    """(81,65,65) p 4, G = 4: the items whose values are loaded are at most
    0.40 of the items (0.370 with the runs cut in lattice order inside each
    class); a regrouping must not quietly lose the reuse."""
    rc, r = plan(lib, "81x65x65-p4", 4)
    assert rc == 0, lib.kle_last_error()
    assert r["item_loads"] <= 0.40 * r["items"], r
