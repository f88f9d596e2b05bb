"""tests/sumfac_ranks_ref.py on the host: the restated partitioned product of
the sum-factorised K and Krhs equals the global one-rank restatement bit for
bit on every configuration of the GPU test, each planted fault
(sumfac_ranks_ref.FAULTS) changes some row, and every configuration has the
host-side property it is there for (conditions)."""
import functools

import numpy as np
import pytest

import sumfac_ranks_ref as SR

NAMES = [n for n, c in SR.CONFIGS.items() if "host" not in c]  # (the IPC configuration is its host twin's mesh)
FAULT_CONFIGS = ("slab2_p2", "inertial3_p2", "msh2d_r3_p2")


@pytest.fixture(scope="module")
def msh_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("sumfac_ranks")


@functools.lru_cache(maxsize=None)
def _partition_cached(name, d):
    cfg = SR.CONFIGS[name]
    return SR.Partition(cfg, SR.mesh_file(cfg, d))


def _partition(name, msh_dir):
    return _partition_cached(name, str(msh_dir))


@functools.lru_cache(maxsize=None)
def _global(name, d, which, k):
    P = _partition_cached(name, d)
    x = SR.inputs(P)[k]
    y = SR.global_product(P.dim, P.ngl, P.one_conn, P.one_corners, P.one_dir, which, P.to_one(x, P.dim))
    return P.to_owner(y, P.dim)


@pytest.mark.parametrize("name", list(SR.CONFIGS))
def test_configurations_have_their_property(name, msh_dir):
    P = _partition(name, msh_dir)
    c = SR.conditions(name, P)
    print(f"SUMFAC-RANKS {name}: neb {c['neb']}  inner {c['inner']}  outer {c['outer']}  peers {c['peers']}")
    assert len(P.parts) == SR.CONFIGS[name]["size"]


@pytest.mark.parametrize("which", ["K", "Krhs"])
@pytest.mark.parametrize("name", NAMES)
def test_partitioned_equals_global(name, which, msh_dir):
    P = _partition(name, msh_dir)
    ghosts = None
    for k, x in enumerate(SR.inputs(P)):  # two x in turn: the second finds the first's ghosts in place
        y, ghosts = SR.partitioned_product(P, which, x, ghosts=ghosts)
        ref = _global(name, str(msh_dir), which, k)
        assert not np.isnan(y).any()
        diff = np.nonzero(y != ref)[0]
        assert y.tobytes() == ref.tobytes(), (name, which, k, len(diff), diff[:8].tolist())
        free = ~np.repeat(P.dirflag, P.dim)
        assert np.any(y[free] != 0.0)


@pytest.mark.parametrize("fault", SR.FAULTS)
@pytest.mark.parametrize("name", FAULT_CONFIGS)
def test_planted_fault_is_caught(name, fault, msh_dir):
    P = _partition(name, msh_dir)
    which = "Krhs" if fault == "inc_order" and P.dim == 2 else "K"
    x0, x1 = SR.inputs(P)
    caught = []
    for at in range(len(P.parts)):
        if fault == "inner_ghost" and len(P.parts[at].outer) == 0:
            continue
        _, ghosts = SR.partitioned_product(P, which, x0)
        y, _ = SR.partitioned_product(P, which, x1, fault=fault, at=at, ghosts=ghosts)
        ref = _global(name, str(msh_dir), which, 1)
        lo, hi = P.ranges[at]
        rows = slice(lo * P.dim, hi * P.dim)
        if y[rows].tobytes() != ref[rows].tobytes():
            caught.append(at)
        # the other ranks' rows are untouched: the fault is local to the rank
        other = np.ones(len(y), bool)
        other[rows] = False
        assert y[other].tobytes() == ref[other].tobytes(), (name, fault, at)
    print(f"SUMFAC-RANKS {name} {fault}: caught on ranks {caught}")
    if fault == "inc_order":
        # (reversing a sum of two terms changes nothing: a node of three or more elements is needed)
        assert any(np.diff(p.incp).max() >= 3 for p in P.parts)
        assert caught, (name, fault)
    else:
        assert caught == [at for at in range(len(P.parts))], (name, fault, caught)
