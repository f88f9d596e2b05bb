"""The planner diagnostics' outputs, pinned (host only).

tests/golden/brick_plan_surface.json holds what kle_brick_plan_box,
kle_brick_plan_box_shared and kle_brick_plan_box_runs returned -- return
codes, kle_last_error() texts, every output word, doubles by their bits --
on the lattices of the CPU plan tests (tests/test_host.py, the brick planner;
tests/test_brick_dedup_plan.py; tests/test_brick_runs_plan.py) before the
row-descriptor codec (kle_brick.hpp BrickRowBox) replaced the hand-written
decodes.  They read every field of the descriptors, so a changed bit of the
tables, a changed refusal or a changed message shows here as an inequality.
"""
import ctypes as C
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "brick_plan_surface.json")
with open(GOLDEN) as f:
    CASES = {c["name"]: c for c in json.load(f)}


@pytest.fixture(scope="module")
def lib():
    import pynama_amd
    from pynama_amd._lib import load
    return load()


def args(c):
    return (*c["L"], c["p"], c["dirichlet"], c["ncu"])


def err(lib, rc):
    return lib.kle_last_error().decode() if rc else ""


@pytest.mark.parametrize("name", list(CASES))
def test_plan_box_outputs_are_pinned(lib, name):
    c, want = CASES[name], CASES[name]["box"]
    info, st = (C.c_int * 8)(), (C.c_double * 8)()
    rc = lib.kle_brick_plan_box(*args(c), c["rounds"], c["split"], info, st)
    assert (rc, err(lib, rc)) == (want["rc"], want["error"])
    if rc == 0:
        assert list(info[:5]) == want["info"]
        assert [float(v).hex() for v in st[:6]] == want["stats"]


@pytest.mark.parametrize("name", list(CASES))
def test_plan_box_shared_outputs_are_pinned(lib, name):
    c, want = CASES[name], CASES[name]["shared"]
    out = (C.c_longlong * 3)()
    rc = lib.kle_brick_plan_box_shared(*args(c), 0, out)
    assert (rc, err(lib, rc)) == (want["rc"], want["error"])
    if rc:
        return
    assert list(out[:3]) == want["out"]
    for shift, key in ((1, "shift1"), (-1, "shift_neg")):
        rc = lib.kle_brick_plan_box_shared(*args(c), shift, out)
        assert (rc, err(lib, rc)) == (want["rc_" + key], want["error_" + key]), shift


@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_plan_box_runs_outputs_are_pinned(lib, name, G):
    c, want = CASES[name], CASES[name]["runs"]["G%d" % G]
    out = (C.c_longlong * 6)()
    rc = lib.kle_brick_plan_box_runs(*args(c), c["split"], G, 0, out)
    assert (rc, err(lib, rc)) == (want["rc"], want["error"])
    if rc:
        return
    assert list(out[:6]) == want["out"]
    for corrupt in (1, 2):
        rc = lib.kle_brick_plan_box_runs(*args(c), c["split"], G, corrupt, out)
        assert (rc, err(lib, rc)) == (want["rc_corrupt%d" % corrupt], want["error_corrupt%d" % corrupt]), corrupt
