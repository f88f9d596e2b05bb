"""Host helpers for the products on several ranks, no GPU: the ranks' exports
joined into one CSR, the inputs that tell the ranks' parts apart, one rank's
rows held to the global longdouble reference, and a restatement of the
partitioned symmetric product in which interface errors can be planted.
Built on tests/sym_ref.py and tests/krylov_ref.py.

  global_csr          the ranks' getValuesCSR() exports (local rows, global
                      columns) with their ownership ranges -> one Csr; the
                      ranges must tile [0, m)
  rank_inputs         sym_ref.inputs over the global lattice, plus
                        only_r{k}       uniform values on rank k's DoFs, 0
                                        elsewhere: every nonzero of another
                                        rank's y came through a halo
                        iface_spike_{k}_first / _last
                                        the 1e8 spike on a node of rank k's
                                        first / last owned plane (graph
                                        partitions: the first / last node of
                                        rank k with a neighbour owned by a peer)
  op_inputs           uniform, ramp and only_r{k} for a rectangular operator,
                      by the ownership ranges of its right-hand vector
  owned_slice_check   test_gpu_sym_ref.check_product on one rank's rows
  partitioned_product the product as slabs form it in symmetric storage: per
                      rank the upper triangle of its rows, the transposed parts
                      of blocks into a higher rank's rows as a separately
                      rounded double, then one fp64 add at the owner -- and the
                      same with one planted error (FAULTS)
"""
import numpy as np

import sym_ref as S
from krylov_ref import Csr

FAULTS = ("drop_block", "double_block", "recv_twice", "stale_recv", "slice_off")
SLICE = 64  # node rows per gather slice (kle_brick.hip: nlo = n / 64 * 64)


def global_csr(parts, ncols=None):
    """parts: one (lo, hi, indptr, indices, data) per rank, in any order.
    Returns (Csr of all rows, [(lo, hi)] in rank order)."""
    parts = sorted(parts, key=lambda p: int(p[0]))
    ranges = [(int(p[0]), int(p[1])) for p in parts]
    assert ranges[0][0] == 0 and all(lo <= hi for lo, hi in ranges), ranges
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), f"the ranges do not tile [0, m): {ranges}"
    ip, ix, d, off = [np.zeros(1, np.int64)], [], [], 0
    for lo, hi, pi, px, pd in parts:
        pi = np.asarray(pi, np.int64)
        assert len(pi) == hi - lo + 1 and pi[0] == 0 and pi[-1] == len(px) == len(pd), (lo, hi, len(pi), len(px))
        ip.append(pi[1:] + off)
        off += int(pi[-1])
        ix.append(np.asarray(px, np.int64))
        d.append(np.asarray(pd, np.float64))
    m = ranges[-1][1]
    A = Csr(np.concatenate(ip), np.concatenate(ix), np.concatenate(d), m if ncols is None else ncols)
    assert A.m == m and (len(A.indices) == 0 or (A.indices.min() >= 0 and A.indices.max() < A.n))
    return A, ranges


def owner_of(ranges, idx):
    """The rank that owns each global index."""
    his = np.array([hi for _, hi in ranges])
    return np.searchsorted(his, np.asarray(idx), side="right")


def interface_nodes(A, ranges, dims, k):
    """[(where, node)] for rank k: on a box lattice (dims = nodes per axis, z
    slabs) the middle node of its first and of its last owned plane; without
    a lattice the first and the last of its nodes with a neighbour (a stored
    column) owned by a peer."""
    lo, hi = ranges[k]
    if dims is not None:
        plane = dims[0] * dims[1]
        assert lo % (3 * plane) == 0 and hi % (3 * plane) == 0 and hi > lo, (ranges, dims)
        mid = (dims[1] // 2) * dims[0] + dims[0] // 2
        return [("first", lo // 3 + mid), ("last", hi // 3 - plane + mid)]
    rows = S._rows(A)
    sel = (rows >= lo) & (rows < hi) & ((A.indices < lo) | (A.indices >= hi)) & (A.data != 0)
    nodes = np.unique(rows[sel] // 3)
    return [("first", int(nodes[0])), ("last", int(nodes[-1]))] if len(nodes) else []


def rank_inputs(A, ranges, dims=None, P=None, seed=0):
    """Every input of sym_ref.inputs(A, dims, P) over the global lattice (the
    greedy combs where dims is None), only_r{k} and iface_spike_{k}_*."""
    out = S.inputs(A, dims, P, seed)
    base = S.uniform(A.n, seed + 17)
    for k, (lo, hi) in enumerate(ranges):
        x = np.zeros(A.n)
        x[lo:hi] = base[lo:hi]
        out[f"only_r{k}"] = x
    for k in range(len(ranges)):
        for where, node in interface_nodes(A, ranges, dims, k):
            out[f"iface_spike_{k}_{where}"] = S.spike(A.n, 3 * node + k % 3, 1e8, seed + 31 + k)
    return out


def op_inputs(n, col_ranges, seed=0):
    """Inputs of a rectangular operator with n columns, owned as col_ranges."""
    out = {"uniform": S.uniform(n, seed), "ramp": S.ramp(n, 6, seed)}
    base = S.uniform(n, seed + 17)
    for k, (lo, hi) in enumerate(col_ranges):
        x = np.zeros(n)
        x[lo:hi] = base[lo:hi]
        out[f"only_r{k}"] = x
    return out


def family(name):
    """The input family of a name: comb3 -> comb, only_r1 -> only_r, ..."""
    for f in ("comb", "only_r", "iface_spike"):
        if name.startswith(f):
            return f
    return name


def owned_slice_check(y, lo, hi, ref, den, rest, allow):
    """check_product (tests/test_gpu_sym_ref.py) on the rows [lo, hi) of the
    global reference: (device error, share of the tolerance, share of the
    allowance, holds).  rest is the global restatement's error, allow the
    global allowance_i."""
    from test_gpu_sym_ref import check_product
    assert len(y) == hi - lo, (len(y), lo, hi)
    return check_product(np.asarray(y), ref[lo:hi], den[lo:hi], rest, allow[lo:hi])


# ------------------------------------------------ the partitioned product
def block_tridiagonal(nodes, seed=0):
    """A synthetic SPD matrix of 3 x 3 node blocks, block-tridiagonal: random
    off-diagonal blocks, symmetric diagonal blocks made dominant; K == K^T bit
    for bit."""
    rng = np.random.default_rng(9000 + seed)
    off = rng.uniform(-1.0, 1.0, (nodes - 1, 3, 3))
    dg = rng.uniform(-1.0, 1.0, (nodes, 3, 3))
    dg = dg + dg.transpose(0, 2, 1) + 8.0 * np.eye(3)
    ip, ix, d = [0], [], []
    for i in range(nodes):
        for a in range(3):
            if i > 0:
                ix += [3 * i - 3, 3 * i - 2, 3 * i - 1]
                d += list(off[i - 1][:, a])  # (the transposed block)
            ix += [3 * i, 3 * i + 1, 3 * i + 2]
            d += list(dg[i][a])
            if i < nodes - 1:
                ix += [3 * i + 3, 3 * i + 4, 3 * i + 5]
                d += list(off[i][a])
            ip.append(len(ix))
    return Csr(ip, ix, d)


def partitioned_product(A, ranges, x, fault=None, prev_recv=None):
    """(y, recv): K x as the ranks of a slab partition form it in symmetric
    storage, all sums in fp64.  Per rank: row i's direct sum over its stored
    blocks (columns from node i on); the transposed parts B_ij^T x_i into the
    rows j the rank owns; the transposed parts into rows of a higher rank
    summed apart (recv: what the reverse halo delivers, one rounded double
    per row) and added by the owner last, y_j += recv_j.

    fault plants one error at an interface:
      drop_block    the first block stored across an interface is left out
      double_block  ... is added twice
      recv_twice    the received sums are added twice
      stale_recv    the received sums are those of the previous product
                    (prev_recv)
      slice_off     the sender takes its ghost rows' sums one 64-row slice
                    early: row j's sum from its local row j - 64 nodes
    """
    assert fault is None or fault in FAULTS, fault
    x = np.asarray(x, np.float64)
    rows, cols = S._rows(A), A.indices
    rn, cn = rows // 3, cols // 3
    with np.errstate(all="ignore"):
        up = cn >= rn
        y = np.zeros(A.m)
        np.add.at(y, rows[up], (A.data * x[cols])[up])
        st = np.flatnonzero(cn > rn)  # stored blocks off the diagonal: their transposes
        src, dst = owner_of(ranges, rows[st]), owner_of(ranges, cols[st])
        assert np.all(dst >= src) and np.all(dst - src <= 1), "more than one sender per row: not a slab partition"
        tval = A.data[st] * x[rows[st]]
        loc, far = st[src == dst], st[src != dst]
        tloc = np.zeros(A.m)
        np.add.at(tloc, cols[loc], tval[src == dst])
        fval = tval[src != dst]
        if fault in ("drop_block", "double_block") and len(far):
            blk = (rn[far] == rn[far[0]]) & (cn[far] == cn[far[0]])
            if fault == "drop_block":
                far, fval = far[~blk], fval[~blk]
            else:
                far, fval = np.concatenate([far, far[blk]]), np.concatenate([fval, fval[blk]])
        recv = np.zeros(A.m)
        np.add.at(recv, cols[far], fval)
        if fault == "slice_off":
            recv = np.zeros(A.m)
            for k, (lo, hi) in enumerate(ranges[:-1]):
                ghost = np.unique(cols[st][(src == k) & (dst == k + 1)])
                from_row = ghost - 3 * SLICE
                ok = from_row >= lo
                recv[ghost[ok]] = tloc[from_row[ok]]
        y = y + tloc
        if fault == "stale_recv":
            assert prev_recv is not None
            y = y + prev_recv
        else:
            y = y + recv
            if fault == "recv_twice":
                y = y + recv
    return y, recv
