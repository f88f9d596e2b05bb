"""The partitioned product of the sum-factorised K and Krhs (kle_sumfac.hip on
several ranks) restated in numpy, on host-built partitions only; nothing here
opens the GPU.  tests/test_sumfac_ranks_ref.py checks it against the global
one-rank restatement, tests/test_gpu_sumfac_ranks.py takes its configurations
and host-side conditions.

A rank's part (Part, from a host mesh made with rank= / nranks=):

  * the local elements, every cell touching an owned node, ascending global
    cell id, with conn in ext-local ids (the position of the global id in
    mesh.ext_gids(), which ascends) and the Dirichlet flags of the ext range;
  * the incidence list of the owned nodes, (e, l) ascending local element;
  * the inner list (every entry an owned node) and the outer list (at least
    one ghost).

The product (partitioned_product), per rank: the ext vector holds the owned x
and, in its ghost slots, whatever the last product left there (NaN at first);
the inner elements are applied to it as it stands -- they run beside the halo;
the halo is an index copy of the owners' entries into the ghost slots; the
outer elements follow; the owned rows gather their incidence entries in list
order; the ranks' rows are stitched in owner numbering.  The element apply is
sumfac_ref.sumfac_apply in float64, a deterministic function of the element's
corners and entries, so a partition that is right reproduces
global_product's bits: the same element sums in the same order.

Planted faults (FAULTS), each of which must change some row:

  stale_ghost     a rank skips the halo copy (its ghosts keep the last x)
  drop_element    a rank leaves out a local element that holds a ghost
  inner_ghost     an outer element is run with the inner list, before the halo
  inc_order       the incidence lists are walked in descending element order
  ghost_dir       the Dirichlet flags of a rank's ghost slots are ignored
"""
import os

import numpy as np

import elem_ref as R
import sumfac_ref as SF

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAULTS = ("stale_ghost", "drop_element", "inner_ghost", "inc_order", "ghost_dir")

# The smallest meshes that reach each edge of the partitioned product; `need`
# names the host-side properties conditions() asserts for the configuration.
CONFIGS = {
    # neb = 9: the last batches of both lists partial (the inertial one is a mesh of test_gpu_ns_ranks_ref;
    # its slabs hold whole batches, 9 elements a layer, so the slab mesh has layers of 6)
    "slab2_p2": dict(pbox=(3, [3, 2, 4], 5), ngl=3, size=2, part="slab", need=("partial",), solve=True,
                     variants=True),
    "inertial3_p2": dict(pbox=(3, [3, 3, 4], 5), ngl=3, size=3, part="inertial", need=("partial",), solve=True),
    # config 5's element, 2 per batch: a list of odd length
    "inertial2_p4": dict(pbox=(3, [3, 1, 4], 13), ngl=5, size=2, part="inertial", need=("odd",)),
    # 343 nodes: the per-thread site loop, neb 1; on every rank but the last nothing runs beside the halo
    # (a node belongs to the highest rank whose cells touch it, so the last rank's cells read owned nodes
    # alone on any mesh: its inner list cannot be empty)
    "inertial2_p6": dict(pbox=(3, [1, 1, 2], 3), ngl=7, size=2, part="inertial", need=("no_inner",)),
    # a rank with three or more peers
    "inertial4_peers": dict(pbox=(3, [4, 4, 1], 5), ngl=3, size=4, part="inertial", need=("peers3",)),
    # 2-D, valence other than 4: Gauss full rule, and GLL (the nodal geometry is the full rule's)
    "msh2d_r3_p2": dict(msh="test.msh", ngl=3, size=3, part="inertial", need=()),
    "msh2d_r2_p4": dict(msh="test.msh", ngl=5, size=2, part="inertial", need=(), eval_rhs=True),
    # box slabs, and one configuration over the IPC transport
    "box2_p3": dict(box=[2, 2, 4], ngl=4, size=2, part=None, need=()),
    "inertial3_p2_ipc": dict(pbox=(3, [3, 3, 4], 5), ngl=3, size=3, part="inertial", need=("partial",),
                             transport="ipc", host="inertial3_p2"),
}


def dim_of(cfg):
    if "msh" in cfg:
        return 2
    return cfg["pbox"][0] if "pbox" in cfg else len(cfg["box"])


def mesh_file(cfg, tmpdir):
    """The Gmsh file of a configuration (None for a box), written under tmpdir."""
    from pynama_amd.meshgen import perturbed_box, write_gmsh
    if "msh" in cfg:
        return os.path.join(G, cfg["msh"])
    if "box" in cfg:
        return None
    dim, nelem, seed = cfg["pbox"]
    p = os.path.join(str(tmpdir), "pbox_%s_%d.msh" % ("x".join(map(str, nelem)), seed))
    if not os.path.exists(p):
        write_gmsh(p, dim, *perturbed_box(dim, nelem, seed=seed))
    return p


def host_meshes(cfg, msh):
    """The one-rank mesh and each rank's part, on the host."""
    import pynama_amd as pa
    from pynama_amd.mesh import UnstructuredMesh
    size, ngl = cfg["size"], cfg["ngl"]
    if msh is not None:
        one = UnstructuredMesh.from_gmsh(msh, ngl)
        parts = [UnstructuredMesh.from_gmsh(msh, ngl, rank=r, nranks=size, partitioner=cfg["part"])
                 for r in range(size)]
    else:
        dim = len(cfg["box"])
        one = pa.BoxMesh(dim, cfg["box"], [0] * dim, [1] * dim, ngl)
        parts = [pa.BoxMesh(dim, cfg["box"], [0] * dim, [1] * dim, ngl, rank=r, nranks=size) for r in range(size)]
    return one, parts


class Part:
    """One rank's tables (module docstring), from its host mesh and the global
    Dirichlet flags in owner numbering."""

    def __init__(self, mesh, dirflag):
        self.rank = mesh.rank
        self.lo, self.hi = mesh.node_range
        self.ext = np.asarray(mesh.ext_gids())
        assert np.all(np.diff(self.ext) > 0)
        self.own0 = int(np.searchsorted(self.ext, self.lo))
        self.N, self.next = self.hi - self.lo, len(self.ext)
        assert np.array_equal(self.ext[self.own0:self.own0 + self.N], np.arange(self.lo, self.hi))
        cg = np.asarray(mesh.conn())
        self.conn = np.searchsorted(self.ext, cg)
        assert np.array_equal(self.ext[self.conn], cg)  # every node of a local element is in the ext range
        self.corners = np.asarray(mesh.corners())
        self.cells = (np.asarray(mesh.elements()) if hasattr(mesh, "elements")
                      else np.arange(*mesh.elem_range))
        assert np.all(np.diff(self.cells) > 0)
        self.dir = np.asarray(dirflag, bool)[self.ext]
        owned = (self.conn >= self.own0) & (self.conn < self.own0 + self.N)
        assert owned.any(axis=1).all()  # a local element touches an owned node
        self.inner = np.nonzero(owned.all(axis=1))[0]
        self.outer = np.nonzero(~owned.all(axis=1))[0]
        # incidence of the owned nodes: (e, l) ascending e
        E, nn = self.conn.shape
        e, l = np.nonzero(owned)
        node = self.conn[e, l] - self.own0
        order = np.lexsort((e, node))
        self.inc = np.stack([e[order], l[order]], 1)
        self.incp = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=self.N))])
        self.ghosts = np.concatenate([np.arange(self.own0), np.arange(self.own0 + self.N, self.next)])


class Partition:
    """The parts of one configuration with the global data in owner numbering:
    N, dim, ngl, the Dirichlet flags, the coordinates, the one-rank mesh's
    arrays and mp, one-rank node -> owner-numbered node."""

    def __init__(self, cfg, msh):
        import pynama_amd as pa
        from oracle import oracle as O
        one, meshes = host_meshes(cfg, msh)
        self.cfg, self.dim, self.ngl, self.N = cfg, one.dim, cfg["ngl"], one.N
        faces = pa.mesh.FACES[one.dim]
        ranges = [tuple(m.node_range) for m in meshes]
        assert ranges[0][0] == 0 and ranges[-1][1] == one.N and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        self.ranges = ranges
        self.coords = np.concatenate([m.coords() for m in meshes])
        self.dirflag = np.zeros(one.N, bool)
        for m in meshes:
            self.dirflag[m.face_nodes(faces)] = True
        self.mp = O.node_map(one.coords(), self.coords)
        one_dir = np.zeros(one.N, bool)
        one_dir[one.face_nodes(faces)] = True
        assert np.array_equal(self.dirflag[self.mp], one_dir)
        self.one_conn, self.one_corners, self.one_dir = np.asarray(one.conn()), np.asarray(one.corners()), one_dir
        self.parts = [Part(m, self.dirflag) for m in meshes]
        self.peers = [sorted(m.peers()) for m in meshes]
        self.neb = max(1, 256 // one.nn)

    def to_owner(self, v_one, bs):
        """A one-rank vector (bs entries per node) in owner numbering."""
        out = np.empty_like(v_one)
        out.reshape(-1, bs)[self.mp] = np.asarray(v_one).reshape(-1, bs)
        return out

    def to_one(self, v_owner, bs):
        return np.ascontiguousarray(np.asarray(v_owner).reshape(-1, bs)[self.mp]).ravel()


def conditions(name, P):
    """The host-side properties a configuration is there for (CONFIGS' need)."""
    need = P.cfg["need"]
    ni, no = [len(p.inner) for p in P.parts], [len(p.outer) for p in P.parts]
    for p in P.parts:
        assert len(p.inner) + len(p.outer) == len(p.conn) and len(np.intersect1d(p.inner, p.outer)) == 0
        assert p.dir[p.ghosts].any(), (name, p.rank, "no ghost Dirichlet node")
    assert all(n > 0 for n in no), (name, "a rank without outer elements")
    if "partial" in need:  # the last batches of both lists are partial on some rank
        assert any(a % P.neb and b % P.neb for a, b in zip(ni, no)), (name, P.neb, ni, no)
    if "odd" in need:
        assert P.neb == 2 and any(n % 2 for n in ni + no), (name, ni, no)
    if "no_inner" in need:
        assert P.neb == 1 and all(n == 0 for n in ni[:-1]) and len(ni) > 1, (name, ni)
        assert ni[-1] > 0
    if "peers3" in need:
        assert max(len(q) for q in P.peers) >= 3, (name, P.peers)
    return {"inner": ni, "outer": no, "peers": [len(q) for q in P.peers], "neb": P.neb}


def _apply(dim, ngl, X, xt):
    return SF.sumfac_apply(dim, ngl, np.asarray(X, np.float64), xt, dtype=np.float64)


def global_product(dim, ngl, conn, corners, dirflag, which, x):
    """The one-rank product: element sums in float64, gathered in ascending
    element order; Dirichlet rows y_i = x_i."""
    dirn = np.asarray(dirflag, bool)
    keep = ~dirn if which == "K" else dirn
    sgn = 1.0 if which == "K" else -1.0
    y = np.zeros(len(dirn) * dim)
    for e in range(len(conn)):
        nd = conn[e]
        cols = R.dof(nd, dim)
        xt = np.where(np.repeat(keep[nd], dim), x[cols], 0.0)
        y[cols] += sgn * _apply(dim, ngl, corners[e], xt)  # (an element names a node once)
    dird = np.repeat(dirn, dim)
    return np.where(dird, x, y)


def partitioned_product(P, which, x, fault=None, at=0, ghosts=None):
    """y in owner numbering and the ranks' ext vectors after the product
    (hand them back as `ghosts` for the next one: a stale slot keeps them).
    fault: one of FAULTS, planted on rank `at`."""
    dim, ngl = P.dim, P.ngl
    sgn = 1.0 if which == "K" else -1.0
    exts, ys = [], []
    for p in P.parts:  # every rank's ext vector before the halo
        v = np.full(p.next * dim, np.nan) if ghosts is None else ghosts[p.rank].copy()
        v[p.own0 * dim:(p.own0 + p.N) * dim] = x[p.lo * dim:p.hi * dim]
        exts.append(v)
    for p in P.parts:
        planted = fault if p.rank == at else None
        xe = exts[p.rank]
        dirn = p.dir.copy()
        if planted == "ghost_dir":
            dirn[p.ghosts] = False
        keep = ~dirn if which == "K" else dirn
        inner, outer = p.inner, p.outer
        if planted == "drop_element":
            outer = outer[1:]
        if planted == "inner_ghost":
            inner, outer = np.concatenate([inner, outer[:1]]), outer[1:]
        E, nn = p.conn.shape
        ws = np.zeros((E, nn * dim))

        def run(lst):
            for e in lst:
                cols = R.dof(p.conn[e], dim)
                xt = np.where(np.repeat(keep[p.conn[e]], dim), xe[cols], 0.0)  # (a dropped entry is never read)
                ws[e] = sgn * _apply(dim, ngl, p.corners[e], xt)

        run(inner)
        if planted != "stale_ghost":  # the halo: the owners' entries, an index copy
            g = R.dof(p.ext[p.ghosts], dim)
            xe[R.dof(p.ghosts, dim)] = x[g]
        run(outer)
        y = np.zeros(p.N * dim)
        for i in range(p.N):
            ent = p.inc[p.incp[i]:p.incp[i + 1]]
            if planted == "inc_order":
                ent = ent[::-1]
            s = np.zeros(dim)
            for e, l in ent:
                s = s + ws[e, l * dim:(l + 1) * dim]
            y[i * dim:(i + 1) * dim] = s
        own = slice(p.own0 * dim, (p.own0 + p.N) * dim)
        dird = np.repeat(p.dir[p.own0:p.own0 + p.N], dim)
        ys.append(np.where(dird, xe[own], y))
    return np.concatenate(ys), exts


def inputs(P, seed=20241021):
    """Two different x in owner numbering."""
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, P.N * P.dim) for _ in range(2)]
