"""KleSolver / KspSolver: the KLE velocity solve on the device.

Mirror of the reference's solver/kle_solver.py:5-64 (same methods and
behaviour): ``solve(vort)`` forms b = Rw*vort + Krhs*vel (vel carries the
Dirichlet values, written beforehand by applyBoundaryConditions) and solves
K vel = b in place.  The reference's KSP is gmres + PC lu, overridden to
preonly + lu by the makefile (makefile:7); K is SPD, so the device default is
CG + Jacobi at rtol 1e-10 (the north-star tolerance), overridable with the
usual -ksp_type / -pc_type / -ksp_rtol / -ksp_max_it options.  The makefile's
-ksp_type preonly -pc_type lu is a dense device LU (rocSOLVER getrf/getrs) for
sequential systems up to 40k unknowns (config 1, the unit cases); beyond that,
or on several ranks, it raises like PETSc without a parallel direct solver --
there is no CPU fallback.
"""
from ._lib import Error
from .petsc import KSP, PC, Options

DEFAULT_RTOL = 1e-10


class KspSolver(KSP):
    def createSolver(self, mat):
        self.create()
        self.setType("cg")
        pc = PC().create()
        pc.setType("jacobi")
        self.setPC(pc)
        self.setTolerances(rtol=DEFAULT_RTOL, atol=0.0, max_it=100000)
        self.setFromOptions()
        self.setOperators(mat)
        self.setUp()


class KleSolver:
    """solve(): after a matrix-free build with the element-wise operators of a
    box mesh (-kle_mat_type element) the Dirichlet values are copied back
    exactly (Mat.copyDirichletRows).  After a sum-factorised build
    (-kle_mat_type sumfac), whose operators hold no such call, they are held to
    the solve's rtol, as in the assembled solve and as with -kle_k_type
    sumfac.  The matrix-free no-slip builds (-kle_ns_type element | sumfac)
    copy the identity rows of K and of K + Kfs back exactly."""

    def __init__(self):
        self.mat = None
        self._b = None
        self._Krhs = self._Rw = None  # the element-wise Krhs and Rw with -kle_k_type element (sumfac: Krhs)
        self._exactBC = False

    def setMat(self, mat):
        self.mat = mat

    def setUp(self):
        K = self.mat.K
        # -kle_k_type element: the KSP's operator and rhs()'s Krhs and Rw are the
        # element-wise operators (MatFS.getElementK / getElementKrhs /
        # getElementRw); whatever they refuse (unstructured, no-slip) raises --
        # no fallback.  After a matrix-free build
        # (-kle_mat_type element) mat.K, mat.Krhs and mat.Rw are those already.
        # -kle_k_type sumfac: the KSP's operator and rhs()'s Krhs are the
        # sum-factorised operators (MatFS.getSumFactoredK / getSumFactoredKrhs:
        # any mesh, one rank or the parts of a partition, unstructured included); Rw stays mat.Rw.
        ktype = Options().getString("kle_k_type", "assembled")
        if ktype not in ("assembled", "element", "sumfac"):
            raise Error(62, f"-kle_k_type {ktype}: assembled | element | sumfac")
        self._Krhs = self.mat.getElementKrhs() if ktype == "element" else None
        self._Rw = self.mat.getElementRw() if ktype == "element" else None
        if ktype == "sumfac":
            self._Krhs = self.mat.getSumFactoredKrhs()
        # matrix-free build (-kle_mat_type element): solve() hands back the
        # Dirichlet values exactly.  The sum-factorised operators refuse
        # copyDirichletRows, so after a sumfac build the Dirichlet values are
        # held to the solve's rtol, as in the assembled solve and with
        # -kle_k_type sumfac.  The sum-factorised no-slip operators
        # (-kle_ns_type sumfac) copy their identity rows like the element-wise ones.
        kern = K.spmvKernel() if K.getFormat() == "elem" else ""
        self._exactBC = K.getFormat() == "elem" and ("k_sumfac" not in kern or "k_sumfac_gather_cls" in kern)
        self.solver = KspSolver()
        self.solver.createSolver(self.mat.getElementK() if ktype == "element"
                                 else self.mat.getSumFactoredK() if ktype == "sumfac" else K)
        self.__vel = K.createVecRight()
        self.__vel.setName("velocity")
        self._b = K.createVecLeft()
        self._wtmp = K.createVecLeft()
        self.__isNS = False
        if self.mat.bcType == "NS":
            # solverFS on K + Kfs (kle_solver.py:22-28); MatNS assembles the sum
            # on the device with PETSc's union pattern and rounding
            self.solverFS = KspSolver()
            self.solverFS.createSolver(self.mat.getKplusKfs())
            self.__velFS = K.createVecRight()
            self.__velFS.setName("free-slip")
            self._bfs = K.createVecLeft()
            self.__isNS = True

    def isNS(self):
        return self.__isNS

    def rhs(self, vort, vec=None):
        """b = Rw * vort + Krhs * vel (kle_solver.py:35) without temporaries."""
        vel = self.__vel if vec is None else vec
        (self._Rw or self.mat.Rw).mult(vort, self._b)
        (self._Krhs or self.mat.Krhs).mult(vel, self._wtmp)
        self._b.axpy(1.0, self._wtmp)
        return self._b

    def solve(self, vort, vec=None):
        vel = self.__vel if vec is None else vec
        b = self.rhs(vort, vel)
        self.solver(b, vel)
        if self._exactBC:
            # the Dirichlet rows of K are unit rows, so there u = b = u_bc; the
            # Krylov iterate (started from 0) holds them to rtol only.  _wtmp is
            # Krhs * vel from rhs(): the Dirichlet values as they came in.
            self.mat.K.copyDirichletRows(self._wtmp, vel)

    def getSolution(self):
        return self.__vel

    def getKSP(self):
        return self.solver

    def rhsFS(self, vort):
        """b = Rw * vort + Rwfs * vort + Krhsfs * vel (kle_solver.py:39-41)."""
        self.mat.Rw.mult(vort, self._bfs)
        self.mat.Rwfs.mult(vort, self._wtmp)
        self._bfs.axpy(1.0, self._wtmp)
        self.mat.Krhsfs.mult(self.__vel, self._wtmp)
        self._bfs.axpy(1.0, self._wtmp)
        return self._bfs

    def solveFS(self, vort):
        self.solverFS(self.rhsFS(vort), self.__velFS)
        if self._exactBC:
            # K + Kfs holds unit rows on the normal DoFs alone; _wtmp is
            # Krhsfs * vel from rhsFS(), whose normal rows are vel exactly
            self.mat.getKplusKfs().copyDirichletRows(self._wtmp, self.__velFS)

    def getFreeSlipSolution(self):
        return self.__velFS
