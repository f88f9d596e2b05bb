"""The symmetric SpMV kernels' products pinned to recorded bits
(kle_sym_dev.hpp wsum3_dpp; DESIGN 3, "Row sums").

Every symmetric kernel -- box bricks (runs, unit by unit, compact stream,
DOT), 128-row tiles, graph bricks, 64-row groups -- sums a row's direct part
over the wave with the one helper wsum3_dpp.  A change of that helper changes
every kernel alike, which the same-build comparisons of
tests/test_gpu_brick_runs.py and tests/test_gpu_brick_dedup.py cannot see.  So
the products are held to sha256 digests recorded from the library as it was
before the helper lost its register copies (tools/record_product_bits.py with
KLE_LIBRARY naming that build; tests/golden/rowsum_bits.json).

The DOT kernel (ksp_sr_gather 2) shows its w only through CG steps, and those
pass through (A u, u), which it forms itself: each wave adds its rows' shares
in the order it is handed them, and beyond a brick's first 48 units (3 static
per wave) the waves take units from a counter as they finish -- which wave
sums which rows, and with it the last bits of (A u, u), follows their timing
(measured: the recorded library gave other digests of three CG steps on the
two splits above in a second process).  y itself does not depend on it.  So
the DOT case runs [8,8,4] ngl 3 split into 8 x 8 x 4 bricks of at most 27 rows
(DOT_SPLITS: at most 48 units whatever the pairing), where every unit is a
static one and every sum has a fixed order, and three CG steps are digested
like the products.  [8,8,2] ngl 5 has no such split: the planner cuts no
brick below one element, whose 64 interior rows make up to 64 units.

Meshes: the two forced splits of tests/test_gpu_brick_runs.py -- [8,8,4]
ngl 3 as one brick (classes of every size 1..8: runs of 1, 2, 3, 4, classes
cut across the cap) and [8,8,2] ngl 5 as 4 x 4 x 1 bricks (rows of several
passes, shared tail items, null partners) -- each also with
spmv_brick_singles 0 and spmv_brick_pair 0; the graph bricks and the groups on
the smallest Gmsh case of tests/test_gpu_gbrick.py ([3,2,2] ngl 5).
Inputs: uniform random; random x 10^uniform(-8, 8) (another tree shape changes
last bits); one huge entry; one NaN; all -0.0; a comb of one nonzero per 7
entries (signed-zero partial sums).
The run cases assert dedup_runs < dedup_units: they must not pass by not
running the run kernel.
"""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rowsum_bits.json")

SPLITS = {
    "8x8x4-p2": 1 + 100 * 1 + 10000 * 1,
    "8x8x2-p4": 4 + 100 * 4 + 10000 * 1,
}
VARIANTS = {"default": {}, "singles0": {"spmv_brick_singles": 0}, "pair0": {"spmv_brick_pair": 0}}
# tunings of the brick kernels beside the split and the variant
BRICK_KERNELS = {
    "runs": {"spmv_brick_dedup": 1, "spmv_brick_compact": 0},
    "unit": {"spmv_brick_dedup": 0, "spmv_brick_compact": 0},
    "compact": {"spmv_brick_dedup": 1, "spmv_brick_compact": 1, "spmv_brick_dedup_full": 0},
}
GMSH = ([3, 2, 2], 5)
# DOT: cuts by equal node counts (+ 1000000) into 8 x 8 x 4 bricks of the 17 x 17 x 9 lattice: parts of at most
# 3 x 3 x 3 nodes
DOT_SPLITS = {"8x8x4-p2": (1000000 + 8 + 100 * 8 + 10000 * 4, [8, 8, 4], 27)}
DOT_INPUTS = ("uniform", "decades", "comb")


def inputs(n):
    rng = np.random.default_rng(11)
    x = rng.uniform(-1.0, 1.0, n)
    decades = rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.uniform(-8.0, 8.0, n)
    huge = x.copy()
    huge[n // 3] = 1e200
    nan = x.copy()
    nan[n // 2] = np.nan
    comb = np.zeros(n)
    comb[::7] = rng.uniform(-1.0, 1.0, len(comb[::7]))
    return {"uniform": x, "decades": decades, "huge": huge, "nan": nan, "negzero": np.full(n, -0.0), "comb": comb}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()


def product_digests(K):
    x = K.createVecRight()
    out = {}
    for nm, xa in inputs(x.getLocalSize()).items():
        x.setArray(xa)
        out[nm] = _sha((K * x).getArray())
    return out


class tunings:
    """Tunings set for a block; put back on exit, K back in full storage."""

    def __init__(self, K, **kv):
        self.K, self.kv = K, kv

    def __enter__(self):
        from pynama_amd.runtime import get_tuning, set_tuning
        self.keep = {k: get_tuning(k) for k in self.kv}
        for k, v in self.kv.items():
            set_tuning(k, v)
        self.K.setOption(self.K.Option.SPD, False)
        self.K.setOption(self.K.Option.SPD, True)
        return self.K

    def __exit__(self, *exc):
        from pynama_amd.runtime import set_tuning
        for k, v in self.keep.items():
            set_tuning(k, v)
        self.K.setOption(self.K.Option.SPD, False)
        return False


def brick_case(pa, name, variant, kernel):
    """(digests per input, getSymmetricBricks()) of one box brick kernel."""
    import test_gpu_brick_dedup as D
    K = D.get_mat(pa, name)["mat"].K
    with tunings(K, spmv_brick_split=SPLITS[name], **VARIANTS[variant], **BRICK_KERNELS[kernel]):
        assert K.spmvKernel().startswith("k_nb_spmv_sym_brick"), K.spmvKernel()
        return product_digests(K), K.getSymmetricBricks()


def tile_case(pa, name):
    import test_gpu_brick_dedup as D
    K = D.get_mat(pa, name)["mat"].K
    with tunings(K, spmv_sym_brick=0):
        assert K.isSymmetricStorage() and not K.spmvKernel().startswith("k_nb_spmv_sym_brick"), K.spmvKernel()
        return product_digests(K), K.spmvKernel()


def dot_case(pa, name):
    """Three single-reduction CG steps with the gather folded into the update
    (ksp_sr_gather 2: the bricks' DOT kernel forms (A u, u)) on the fine
    split: digests of (x, ||r||, iterations), the product kernel, the bricks."""
    import test_gpu_brick_dedup as D
    import test_gpu_sym_ref as T
    K = D.get_mat(pa, name)["mat"].K
    out = {}
    with tunings(K, spmv_brick_split=DOT_SPLITS[name][0], ksp_sr_gather=2):
        info = K.getSymmetricBricks()
        ksp = T.make_ksp(pa, K, "sr", "jacobi")
        b, x = K.createVecLeft(), K.createVecRight()
        ins = inputs(b.getLocalSize())
        for nm in DOT_INPUTS:
            b.setArray(ins[nm])
            ksp.setFixedIterations(3)
            ksp.solve(b, x)
            out[nm] = _sha(np.append(x.getArray(), [ksp.getResidualNorm(), ksp.getIterationNumber()]))
        return out, ksp.getProductKernel(), info


def gmsh_case(pa, tmp_path, bricks):
    from pynama_amd.meshgen import perturbed_box, write_gmsh
    from pynama_amd.runtime import get_tuning, set_tuning
    nelem, ngl = GMSH
    V, Cc, F, T = perturbed_box(3, nelem, seed=5)
    path = os.path.join(str(tmp_path), "g5.msh")
    write_gmsh(path, 3, V, Cc, F, T)
    cfg = {"domain": {"ngl": ngl, "gmsh-file": path}, "boundary-conditions": {"custom-func": {"name": "taylor_green3d"}}}
    dom = pa.Domain()
    dom.configure(cfg)
    dom.setUp()
    mat = pa.MatFS()
    mat.setDomain(dom)
    mat.build(buildOperators=False)
    K = mat.K
    keep = get_tuning("spmv_gsym_brick")
    set_tuning("spmv_gsym_brick", bricks)
    try:
        K.setOption(K.Option.SPD, True)
        return product_digests(K), K.spmvKernel(), int(K.createVecRight().getLocalSize())
    finally:
        set_tuning("spmv_gsym_brick", keep)


def record(pa, tmp_path):
    """Every case's digests, as tests/golden/rowsum_bits.json holds them."""
    import test_gpu_brick_dedup as D
    out = {"shapes": {}, "digests": {}}
    for name in SPLITS:
        out["shapes"][name] = int(D.get_mat(pa, name)["mat"].K.createVecRight().getLocalSize())
        for variant in VARIANTS:
            for kernel in BRICK_KERNELS:
                out["digests"][f"{name}/{variant}/{kernel}"] = brick_case(pa, name, variant, kernel)[0]
        out["digests"][f"{name}/tiles"] = tile_case(pa, name)[0]
        if name in DOT_SPLITS:
            out["digests"][f"{name}/dot"] = dot_case(pa, name)[0]
    for bricks, nm in ((1, "gbrick"), (0, "groups")):
        out["digests"][f"gmsh/{nm}"], _, out["shapes"]["gmsh"] = gmsh_case(pa, tmp_path, bricks)
    return out


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _same(got, want, what):
    assert set(got) == set(want), what
    bad = [nm for nm in got if got[nm] != want[nm]]
    assert not bad, (what, bad)


@pytest.mark.parametrize("kernel", list(BRICK_KERNELS))
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(SPLITS))
def test_box_brick_products_are_the_recorded_bits(pa, golden, name, variant, kernel):
    got, info = brick_case(pa, name, variant, kernel)
    if kernel == "runs":  # (the run kernel is what ran)
        assert info["dedup"] is True and info["compact"] is False, info
        assert 0 < info["dedup_runs"] < info["dedup_units"], info
    elif kernel == "unit":
        assert info["dedup"] is False and info["dedup_runs"] == 0, info
    else:
        assert info["compact"] is True and info["dedup_runs"] == 0, info
    _same(got, golden["digests"][f"{name}/{variant}/{kernel}"], (name, variant, kernel))


@pytest.mark.parametrize("name", list(SPLITS))
def test_tile_products_are_the_recorded_bits(pa, golden, name):
    got, kern = tile_case(pa, name)
    _same(got, golden["digests"][f"{name}/tiles"], (name, kern))


@pytest.mark.parametrize("name", list(DOT_SPLITS))
def test_cg_steps_through_the_dot_kernel_are_the_recorded_bits(pa, golden, name):
    got, kern, info = dot_case(pa, name)
    assert kern.startswith("k_nb_spmv_sym_brick") and kern.endswith("true>") and "+" not in kern, kern
    _, dims, rows = DOT_SPLITS[name]
    # (every brick at most 48 units: no unit is handed out by the counter)
    assert list(info["dims"]) == dims and info["bricks"] == dims[0] * dims[1] * dims[2] and rows <= 48, info
    _same(got, golden["digests"][f"{name}/dot"], (name, kern))


@pytest.mark.parametrize("bricks,nm,prefix", [(1, "gbrick", "k_nb_spmv_gsym_brick"), (0, "groups", "k_nb_spmv_gsym<")])
def test_gmsh_products_are_the_recorded_bits(pa, golden, tmp_path, bricks, nm, prefix):
    got, kern, n = gmsh_case(pa, tmp_path, bricks)
    assert kern.startswith(prefix), kern
    assert n == golden["shapes"]["gmsh"], (n, golden["shapes"])  # (the generated mesh is the recorded one)
    _same(got, golden["digests"][f"gmsh/{nm}"], kern)


def test_shapes_are_the_recorded_ones(pa, golden):
    import test_gpu_brick_dedup as D
    for name in SPLITS:
        assert golden["shapes"][name] == D.get_mat(pa, name)["mat"].K.createVecRight().getLocalSize()
