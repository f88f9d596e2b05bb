"""MatFS: device assembly of the KLE matrices.

Mirror of the reference's MatFS (matrices/mat_fs.py:5-209): same public
surface -- setDomain, build, K, Krhs, Rw, Rd, getOperators, bcType -- but the
per-cell Python loop of buildFS (mat_fs.py:150-192), which calls
Spectral.getElemKLEMatrices and MatSetValues once per element, is replaced by
one batch device assembly (libkle kle_assemble_kle): element matrices on the
GPU, deterministic gather into node-block CSR, PETSc pattern and ADD order.
"""
import ctypes as C

import numpy as np

from ._lib import Error, call
from .petsc import Mat, Options
from .runtime import get_ctx


def kle_mat_type(kleType=None):
    """The form of the KLE matrices: the keyword, else -kle_mat_type, else
    "assembled"; anything but assembled | element | sumfac raises Error 62."""
    if kleType is None:
        kleType = Options().getString("kle_mat_type", "assembled")
    if kleType not in ("assembled", "element", "sumfac"):
        raise Error(62, f"-kle_mat_type {kleType}: assembled | element | sumfac")
    return kleType


def kle_op_type(opType=None):
    """The form of Curl, SrT and DivSrT: the keyword, else -kle_op_type, else
    "assembled"; anything but assembled | element | sumfac raises Error 62."""
    if opType is None:
        opType = Options().getString("kle_op_type", "assembled")
    if opType not in ("assembled", "element", "sumfac"):
        raise Error(62, f"-kle_op_type {opType}: assembled | element | sumfac")
    return opType


def kle_ns_type(nsType=None):
    """The form of the no-slip KLE matrices (MatNS): the keyword, else
    -kle_ns_type, else "assembled"; anything but assembled | element | sumfac
    raises Error 62."""
    if nsType is None:
        nsType = Options().getString("kle_ns_type", "assembled")
    if nsType not in ("assembled", "element", "sumfac"):
        raise Error(62, f"-kle_ns_type {nsType}: assembled | element | sumfac")
    return nsType


class MatFS:
    bcType = "FS"

    def __init__(self):
        self.kle = []
        self.K = self.Krhs = self.Rw = self.Rd = None
        self.operator = None

    def setDomain(self, dom):
        self.dom = dom

    def build(self, buildKLE=True, buildOperators=True, kleType=None, opType=None):
        """kleType (default: -kle_mat_type, default "assembled"): "element"
        builds K, Krhs and Rw as element-wise operators and assembles nothing
        (uniform box meshes, one rank or slabs on several; anything else
        raises Error 56).  "sumfac" builds them as sum-factorised operators
        (Mat.createKLESumFactored, Mat.createRwSumFactored: any
        mesh, unstructured included) and assembles nothing either; Rd is the
        empty matrix and mat.kle keeps its order.
        opType (default: -kle_op_type, default "assembled"): "element" does the
        same for Curl, SrT and DivSrT, "sumfac" with every element's own
        geometry on any mesh, one rank or the parts of a partition (Mat.createOperatorSumFactored); with
        both, nothing at all is assembled."""
        if self.dom.getBoundaryType() != "FS":
            raise Error(56, "MatFS needs free-slip (Dirichlet) boundaries")
        kleType = kle_mat_type(kleType) if buildKLE else kleType
        opType = kle_op_type(opType) if buildOperators else opType
        if buildKLE:
            self.buildFS(kleType)
        if buildOperators:
            self.buildOperators(opType)

    def buildFS(self, kleType="assembled"):
        ctx = get_ctx()
        mesh = self.dom.getMesh()
        dim = self.dom.getDimensions()[0]
        if kleType == "element":
            # matrix-free: no kle_assemble_kle, no assembled values; the three
            # operators are the ones getElementK/Krhs/Rw return
            self.K, self.Krhs, self.Rw = (Mat.createKLEElement(mesh, n) for n in ("K", "Krhs", "Rw"))
            for m, n in ((self.K, "K"), (self.Krhs, "Krhs"), (self.Rw, "Rw")):
                m.setName(n)
            self._elemK, self._elemKrhs, self._elemRw = self.K, self.Krhs, self.Rw
            self.Rd = self._empty(dim)
            self.kle = [self.K, self.Krhs, self.Rw, self.Rd]
            return
        if kleType == "sumfac":
            # matrix-free on any mesh, one rank or the parts of a partition: the operators getSumFactoredK /
            # Krhs / Rw return, sharing one geometry set
            self.K, self.Krhs, self.Rw = self.getSumFactoredK(), self.getSumFactoredKrhs(), self.getSumFactoredRw()
            for m, n in ((self.K, "K"), (self.Krhs, "Krhs"), (self.Rw, "Rw")):
                m.setName(n)
            self.Rd = self._empty(dim)
            self.kle = [self.K, self.Krhs, self.Rw, self.Rd]
            return
        hK, hKr, hRw = C.c_void_p(), C.c_void_p(), C.c_void_p()
        call("kle_assemble_kle", ctx.h, mesh._h, C.byref(hK), C.byref(hKr), C.byref(hRw))
        dim, dim_w, _ = self.dom.getDimensions()
        self.K = Mat._wrap(hK, ctx, mesh, dim, dim)
        self.Krhs = Mat._wrap(hKr, ctx, mesh, dim, dim)
        self.Rw = Mat._wrap(hRw, ctx, mesh, dim, dim_w)
        for m, n in ((self.K, "K"), (self.Krhs, "Krhs"), (self.Rw, "Rw")):
            m.setName(n)
        # Rd is preallocated but never filled in free slip (preAlloc_Rd_Rw,
        # mat_fs.py:54-94; buildFS adds no Rd entries): after assembleAll it is
        # an assembled [dim N x N] matrix without stored entries
        self.Rd = self._empty(dim)
        self.kle = [self.K, self.Krhs, self.Rw, self.Rd]

    def _empty(self, dim, name="Rd"):
        lo, hi = self.dom.getNodesRange()
        N = self.dom.getMesh().N
        A = Mat().createAIJ((((hi - lo) * dim, N * dim), (hi - lo, N)),
                            nnz=(np.zeros((hi - lo) * dim, dtype=np.int32), None))
        A.assemble()
        A.setName(name)
        return A

    def getElementK(self):
        """K as an element-wise operator (Mat.createKLEElement): no assembled
        values, uniform box meshes (one rank or slabs on several).  Created on
        first use."""
        if getattr(self, "_elemK", None) is None:
            self._elemK = Mat.createKLEElement(self.dom.getMesh(), "K")
        return self._elemK

    def getElementKrhs(self):
        """Krhs as an element-wise operator; created on first use."""
        if getattr(self, "_elemKrhs", None) is None:
            self._elemKrhs = Mat.createKLEElement(self.dom.getMesh(), "Krhs")
        return self._elemKrhs

    def getElementRw(self):
        """Rw as an element-wise operator; created on first use."""
        if getattr(self, "_elemRw", None) is None:
            self._elemRw = Mat.createKLEElement(self.dom.getMesh(), "Rw")
        return self._elemRw

    def getSumFactoredK(self):
        """K as a sum-factorised element-wise operator
        (Mat.createKLESumFactored): no assembled values and no element matrix,
        any mesh, one rank or the parts of a partition (box or unstructured).  Created on first use."""
        if getattr(self, "_sumfacK", None) is None:
            self._sumfacK = Mat.createKLESumFactored(self.dom.getMesh(), "K")
        return self._sumfacK

    def getSumFactoredKrhs(self):
        """Krhs as a sum-factorised element-wise operator; created on first use."""
        if getattr(self, "_sumfacKrhs", None) is None:
            self._sumfacKrhs = Mat.createKLESumFactored(self.dom.getMesh(), "Krhs")
        return self._sumfacKrhs

    def getSumFactoredRw(self):
        """Rw as a sum-factorised element-wise operator
        (Mat.createRwSumFactored); created on first use."""
        if getattr(self, "_sumfacRw", None) is None:
            self._sumfacRw = Mat.createRwSumFactored(self.dom.getMesh())
        return self._sumfacRw

    def buildOperators(self, opType=None):
        """Curl / SrT / DivSrT on the device (mat_fs.py:194-201): assembled
        whatever the kleType, unless opType (default: -kle_op_type) is
        "element" or "sumfac"."""
        self.operator = Operators()
        self.operator.setDimensions(self.dom.getDimensions())
        self.operator.build(self.dom.getMesh(), opType)

    def getOperators(self):
        return self.operator

    def assembleAll(self):
        pass


class MatNS(MatFS):
    """Mirror of the reference's MatNS (matrices/mat_ns.py:5-161): no-slip walls.
    K, Krhs, Rw fix the no-slip nodes; Kfs, Krhsfs, Rwfs free their tangential
    DoFs for the free-slip pre-solve (solveFS).  One device pass
    (kle_assemble_ns) with PETSc's DoF-level patterns; K + Kfs, the operator of
    KleSolver.solverFS, is assembled directly (getKplusKfs)."""
    bcType = "NS"

    def __init__(self):
        super().__init__()
        self.Kfs = self.Krhsfs = self.Rwfs = self.Rdfs = None
        self._Ksum = None

    def build(self, buildKLE=True, buildOperators=True, kleType=None, opType=None, nsType=None):
        """opType "element" or "sumfac" (default: -kle_op_type): Curl, SrT and
        DivSrT as element-wise operators, which carry no boundary rule
        ("sumfac": any mesh, one rank or the parts of a partition; the NS matrices stay assembled).
        nsType (default: -kle_ns_type, default "assembled"): "element" builds
        K, Krhs, Rw, Kfs, Krhsfs, Rwfs and K + Kfs as element-wise operators
        (Mat.createNSElement) and never calls kle_assemble_ns; Rd and Rdfs are
        empty assembled matrices and mat.kle keeps its order of eight.  Uniform
        box meshes, one rank or slabs on several; anything else raises Error
        56.  "sumfac" builds the same seven as sum-factorised operators
        (Mat.createNSSumFactored) on any mesh, Gmsh meshes and their partitions
        included, sharing one geometry set; with opType="sumfac" as well nothing
        at all is assembled.  This switch is the way to the matrix-free no-slip system:
        kleType="element" / -kle_mat_type element (and "sumfac") name the
        free-slip forms, which a no-slip mesh does not have, and keep raising
        Error 56 here."""
        if kle_mat_type(kleType) in ("element", "sumfac"):
            raise Error(56, f"-kle_mat_type {kle_mat_type(kleType)}: no-slip matrices have no such form")
        if self.dom.getBoundaryType() != "NS":
            raise Error(56, "MatNS needs no-slip boundaries")
        nsType = kle_ns_type(nsType) if buildKLE else nsType
        opType = kle_op_type(opType) if buildOperators else opType
        if buildKLE:
            self.buildNS(nsType)
        if buildOperators:
            self.buildOperators(opType)

    def buildNS(self, nsType="assembled"):
        ctx = get_ctx()
        mesh = self.dom.getMesh()
        if nsType in ("element", "sumfac"):
            # matrix-free: no kle_assemble_ns, no assembled values
            dim = self.dom.getDimensions()[0]
            names = ("K", "Krhs", "Rw", "Kfs", "Krhsfs", "Rwfs", "K+Kfs")
            create = Mat.createNSElement if nsType == "element" else Mat.createNSSumFactored
            ops = {n: create(mesh, n) for n in names}
            for n, m in ops.items():
                m.setName(n)
            self.K, self.Krhs, self.Rw = ops["K"], ops["Krhs"], ops["Rw"]
            self.Kfs, self.Krhsfs, self.Rwfs = ops["Kfs"], ops["Krhsfs"], ops["Rwfs"]
            self._Ksum = ops["K+Kfs"]
            self.Rd, self.Rdfs = self._empty(dim), self._empty(dim, "Rdfs")
            self.kle = [self.K, self.Krhs, self.Rw, self.Rd, self.Kfs, self.Krhsfs, self.Rwfs, self.Rdfs]
            return
        h = [C.c_void_p() for _ in range(9)]
        call("kle_assemble_ns", ctx.h, mesh._h, *[C.byref(x) for x in h])
        dim, dim_w, _ = self.dom.getDimensions()
        shapes = [(dim, dim), (dim, dim), (dim, dim_w), (dim, 1), (dim, dim), (dim, dim), (dim, dim_w), (dim, 1),
                  (dim, dim)]
        mats = [Mat._wrap(x, ctx, mesh, r, c) for x, (r, c) in zip(h, shapes)]
        (self.K, self.Krhs, self.Rw, self.Rd, self.Kfs, self.Krhsfs, self.Rwfs, self.Rdfs, self._Ksum) = mats
        for m, n in zip(mats, ("K", "Krhs", "Rw", "Rd", "Kfs", "Krhsfs", "Rwfs", "Rdfs", "K+Kfs")):
            m.setName(n)
        self.kle = mats[:8]

    def getKplusKfs(self):
        return self._Ksum


class Operators:
    """Mirror of the reference's Operators (mat_fs.py:211-271): the collocation
    operators Curl [dim_w N x dim N], SrT [dim_s N x dim N] and DivSrT
    [dim N x dim_s N], each left-scaled by the inverse lumped nodal weight.
    Assembled in one device pass (libkle kle_assemble_operators) instead of
    the per-cell setValues loop; same pattern (explicit zeros kept) and the
    same ascending-cell ADD order.  With opType "element" (-kle_op_type
    element) nothing is assembled: the three are element-wise operators
    (Mat.createOperatorElement; uniform box meshes, one rank or slabs on
    several).  With opType "sumfac" they read every element's own geometry
    (Mat.createOperatorSumFactored; any mesh, one rank or the parts of a partition)."""

    def __init__(self):
        self.Curl = self.SrT = self.DivSrT = None

    def setDimensions(self, dims):
        self.dim, self.dim_w, self.dim_s = dims

    def build(self, mesh, opType=None):
        opType = kle_op_type(opType)
        if opType in ("element", "sumfac"):
            create = Mat.createOperatorElement if opType == "element" else Mat.createOperatorSumFactored
            self.Curl, self.SrT, self.DivSrT = (create(mesh, n) for n in ("Curl", "SrT", "DivSrT"))
            for m, n in ((self.Curl, "Curl"), (self.SrT, "SrT"), (self.DivSrT, "DivSrT")):
                m.setName(n)
            return
        ctx = get_ctx()
        hc, hs, hd = C.c_void_p(), C.c_void_p(), C.c_void_p()
        call("kle_assemble_operators", ctx.h, mesh._h, C.byref(hc), C.byref(hs), C.byref(hd))
        self.Curl = Mat._wrap(hc, ctx, mesh, self.dim_w, self.dim)
        self.SrT = Mat._wrap(hs, ctx, mesh, self.dim_s, self.dim)
        self.DivSrT = Mat._wrap(hd, ctx, mesh, self.dim, self.dim_s)
        for m, n in ((self.Curl, "Curl"), (self.SrT, "SrT"), (self.DivSrT, "DivSrT")):
            m.setName(n)

    def assembleAll(self):
        pass  # assembled (and weight-scaled) on the device by build()
