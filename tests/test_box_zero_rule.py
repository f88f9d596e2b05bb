"""The analytic zeros of the free-slip K of an axis-aligned box mesh, on the
CPU oracle's assembly (oracle.BoxMesh.assemble_fs).

The rule (kle_assemble.hip box_zero_entry writes these entries as +0.0):
entry (a, b), a != b, of the 3 x 3 block between lattice nodes i and j is
analytically zero when, for c = a or c = b, the two nodes share lattice
coordinate c and that shared plane is not a plane of the domain boundary
(0 < coordinate < L_c - 1).  On a boundary plane the one-sided endpoint terms
do not cancel, so the exclusion is part of the rule.

Bounds: the assembly's rounding noise on these entries is a few 1e-16 of
max|K| (worst of the five meshes 5.6e-16); the entries that are not noise
start at 5e-7 of max|K|.  1e-13 lies more than two decades above the one
and six below the other.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as O

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
ALL = ("x-", "x+", "y-", "y+", "z-", "z+")
# (nelem, ngl, Dirichlet faces, box)
MESHES = {
    "cube-all": ([4, 4, 4], 5, ALL, UNIT),
    "noncubic-all": ([5, 4, 3], 4, ALL, UNIT),
    "xlow-ylow": ([3, 4, 2], 5, ("x-", "y-"), UNIT),
    "offset-zhigh": ([3, 2, 2], 3, ("z+",), ([0.3, -1.0, 2.0], [1.7, 0.5, 2.9])),
    "no-faces": ([2, 2, 3], 6, (), UNIT),
}
MIXED = ("xlow-ylow", "offset-zhigh")
NOISE = 1e-13


def lattice(nelem, ngl):
    return [n * (ngl - 1) + 1 for n in nelem]


def node_coords(nodes, L):
    return np.stack([nodes % L[0], (nodes // L[0]) % L[1], nodes // (L[0] * L[1])], axis=-1)


def face_flags(nelem, ngl, faces):
    L = lattice(nelem, ngl)
    c = node_coords(np.arange(L[0] * L[1] * L[2]), L)
    flag = np.zeros(len(c), np.uint8)
    for f in faces:
        d = "xyz".index(f[0])
        flag[c[:, d] == (0 if f[1] == "-" else L[d] - 1)] = 1
    return flag


def rule_mask(rows, cols, L, boundary_exclusion=True):
    """Per scalar entry (row, col) of K: does the rule make it zero?"""
    a, b = rows % 3, cols % 3
    ci, cj = node_coords(rows // 3, L), node_coords(cols // 3, L)
    shared = ci == cj
    if boundary_exclusion:
        shared &= (ci > 0) & (ci < np.array(L) - 1)
    k = np.arange(len(rows))
    return (a != b) & (shared[k, a] | shared[k, b])


@functools.lru_cache(maxsize=None)
def load(name):
    """The free-free entries of the oracle's K on mesh `name` (assembled once)."""
    nelem, ngl, faces, (lo, hi) = MESHES[name]
    m = O.BoxMesh(3, nelem, lo, hi, ngl)
    flag = face_flags(nelem, ngl, faces)
    assert len(flag) == m.N
    K = m.assemble_fs(flag)[0]
    rows = np.repeat(np.arange(K.m), np.diff(K.indptr))
    cols = K.indices
    free = (flag[rows // 3] == 0) & (flag[cols // 3] == 0)
    return {"name": name, "L": lattice(nelem, ngl), "faces": faces, "rows": rows[free], "cols": cols[free],
            "val": np.abs(K.data[free]), "kmax": np.abs(K.data).max()}


@pytest.mark.parametrize("name", list(MESHES))
def test_rule_entries_are_noise(name):
    case = load(name)
    z = rule_mask(case["rows"], case["cols"], case["L"])
    assert z.any()
    worst = case["val"][z].max() / case["kmax"]
    print(f"{case['name']}: {int(z.sum())} entries under the rule ({z.mean():.1%} of free-free nnz), "
          f"largest {worst:.1e} max|K|, smallest other {case['val'][~z].min() / case['kmax']:.1e}")
    assert worst <= NOISE


@pytest.mark.parametrize("name", [n for n in MESHES if MESHES[n][2] == ALL])
def test_rule_covers_all_noise_with_all_faces(name):
    case = load(name)
    z = rule_mask(case["rows"], case["cols"], case["L"])
    assert (case["val"][~z] >= NOISE * case["kmax"]).all()


@pytest.mark.parametrize("name", MIXED)
def test_boundary_exclusion_is_needed(name):
    case = load(name)
    wide = rule_mask(case["rows"], case["cols"], case["L"], boundary_exclusion=False)
    assert case["val"][wide].max() > 1e-2 * case["kmax"]
