// kle_elem.hip -- element-wise K, Krhs and Rw of a uniform box mesh (kle_mat kind 2).
//
// kle_mesh_create_box makes every element the same brick, so every element
// matrix equals that of the first element up to coordinate rounding and
//
//     K u = sum over elements e of  S_e^T  K_e0  S_e u
//
// with the Dirichlet masking of MatFS.buildFS (mat_fs.py:150-190): no matrix
// values are stored or streamed.  K_e0 (nd x nd, nd = dim * ngl^dim) stays in
// cache; the product is one FP64 GEMM K_e0 [nd x nd] * X [nd x E] followed by
// a gather per node.  Rw (mat_fs.py:185-186) is the same construction with the
// rectangular Rw_e0 [nd x nc], nc = dim_w * ngl^dim (dim_w = 1 in 2-D, 3 in
// 3-D): free rows take every vorticity column of their elements (no column
// mask, no negation), Dirichlet rows hold no entry.
//
//   k_elem_gemm    one 256-thread workgroup per (batch of 16 * NCT elements,
//                  NCT = 2 or 1; group of 128 rows).  The batch's x entries
//                  are gathered through the connectivity into LDS, 64 k rows
//                  at a time, masked by selection (K: Dirichlet entries
//                  dropped; Krhs: free entries dropped; the rule is folded
//                  into the connectivity as -1), so an Inf or NaN in a masked
//                  entry is never read.  Every wave owns two 16-row tiles and
//                  keeps 2 * NCT accumulators; per k step of 4 it feeds each
//                  of its two K_e0 operands (stored in operand order: one
//                  coalesced 512-B load each) to NCT v_mfma_f64_16x16x4_f64
//                  (lane: A[l = lane&15][k = lane>>4], B[k = lane>>4][n =
//                  lane&15]; result reg r at l = (lane>>4) + 4r, n = lane&15).
//                  Loads run a chunk (operands, x) or two (node ids) ahead of
//                  the MFMAs in registers.  Rows and columns beyond nd and
//                  elements beyond E are zero operands and are never stored.
//                  The contraction runs over the nc columns of the element
//                  matrix, padded to the k step of 4 (ncp); x is gathered as
//                  x[node * CW + b], CW the component count of the column
//                  space (dim for K and Krhs, dim_w for Rw), so a padding
//                  column is a zero operand and is never read from x.
//                  Krhs negates the result (the assembly adds -K_e).
//   k_elem_gather  one thread per owned DoF: the sum of its node's incidence
//                  entries from the element results in table (ascending
//                  element) order -- fixed order, no atomics, bitwise
//                  repeatable.  Dirichlet rows: y_i = x_i (K, Krhs); 0 for Rw,
//                  which reads neither x nor the element results there.
//
// Several ranks (slabs of whole element layers, kle_mesh_create_box): owner
// computes.  A rank's local elements are every element touching an owned node
// -- one ghost layer below (rank > 0), its own layers, the top one of which
// reads the single upper ghost plane -- so the tables hold ext-local node ids
// (global id - ext_begin), x is read through the vector's ghosted allocation
// after one forward halo, and the gather runs over the owned nodes alone.  The
// GEMM is launched over element ranges (elem_ranges): the interior elements
// beside the halo, the ghost layer and the top layer after it.  Of a ghost-
// layer element only the top-plane rows [nd - nd / ngl, nd) are ever gathered:
// its launch covers the row groups holding them and no other.  K_e0 is that of
// global element 0 on every rank and neither the per-element accumulation nor
// the ascending-element gather depends on the partition, so a rank's owned
// rows are the one-rank product's bit for bit.
//
// No-slip meshes (kle_mat_create_ns_element): the seven matrices of
// MatNS.buildNS (mat_ns.py:47-145) are the same sums with masks per velocity
// DoF -- classes F / T / N from the mesh's dof_cls -- instead of per node, and
// Kfs's kept columns depend on the row's class.  Each is at most two passes of
// (column classes kept -> row classes taking the sum) and a fixed rule on every
// other row (NS_SPECS, kle_internal.hpp):
//
//   k_elem_gemm<CW, NCT, DOF = true>  the same kernel with its column index
//                  from a per-element, per-column table [E][nc] of ext-local x
//                  indices (-1 dropped) instead of the node table [E][nn]; a
//                  second pass is the same launch over a second table into a
//                  second result array (Kfs only).  Rw and Rwfs keep every
//                  column and run the per-node kernel unchanged.
//   k_elem_gather_cls  one thread per owned DoF; the rule byte of its class
//                  says zero (+0.0, nothing read), identity (x_i bit for bit),
//                  the sum from pass 0 or from pass 1 (incidence-table order,
//                  no atomics) and whether -x_i is added (Kfs's T rows).
//
// Ghost DoFs are masked through the ext-indexed classes; layout, element
// ranges, halo and the ghost layer's row groups are those above.
#include <algorithm>
#include <cstring>

#include "kle_internal.hpp"

namespace kle {

struct ElemOp {
    int which = 0, dim = 3, cw = 3, nn = 0, nd = 0, ndp = 0, nc = 0, ncp = 0, maxinc = 8, nct = 1;
    int64_t E = 0, N = 0;       // local elements, owned nodes
    int rg_top = 0;             // first 128-row group holding a top-plane row (the ghost layer's launch starts there)
    double *d_kt = nullptr;     // K_e0 (Rw_e0) padded to ndp x ncp in MFMA operand order [row tile][k step][lane]
    double *d_kdiag = nullptr;  // [nd] its diagonal (K, Krhs)
    double *d_ws = nullptr;     // [E][nd] element results
    int32_t *d_conn = nullptr;  // [E][nn] element -> ext-local node, tensor order; -1 where the operator drops the entry
    int32_t *d_inc = nullptr;   // [N][maxinc] owned node -> e * nn + l, ascending e, -1 padded
    uint8_t *d_dir = nullptr;   // [N] Dirichlet flag of the owned nodes
    int negate = 0;             // the GEMM stores -K_e0 x_e (Krhs, Krhsfs)
    // no-slip operators (kle_mat_create_ns_element): masks per velocity DoF
    int ns = 0;                 // 1: rows by DoF class (k_elem_gather_cls), which = 0 .. 6
    int npass = 1;              // GEMM passes (Kfs: 2), pass p over d_cidx[p] into d_wsp[p]
    bool dofcols = false;       // columns through the per-DoF tables d_cidx (Rw, Rwfs: the node table d_conn)
    int32_t *d_cidx[2] = {nullptr, nullptr};  // [E][nc] element column -> ext-local x index, -1 dropped
    double *d_wsp[2] = {nullptr, nullptr};    // [E][nd] per pass (d_wsp[0] == d_ws)
    uint8_t *d_cls = nullptr;   // [N * dim] class of the owned DoFs
    unsigned rules = 0;         // row rule of class c in byte c (NS_*)
    unsigned drules = 0;        // diagonal of class c in byte c: 0 zero, 1 one, 2 the element sums, 3 the sums - 1
};

constexpr int EG_KC = 64;            // k rows of X per LDS chunk
constexpr int EG_TR = 2;             // 16-row tiles per wave
constexpr int EG_ROWS = 4 * EG_TR * 16;  // rows per workgroup

typedef double edbl4 __attribute__((ext_vector_type(4)));

// DOF: the column index comes from a per-element, per-column table [E][nc] of
// ext-local x indices (-1 dropped) in mconn -- the no-slip masks act per
// velocity DoF, not per node; everything else is the same kernel.
template <int CW, int NCT, bool DOF = false>
__global__ __launch_bounds__(256, 2) void k_elem_gemm(int negate, int nn, int nd, int ndp, int nc, int ncp, int64_t eb,
                                                      int64_t E, int rg0, const double *__restrict__ kt,
                                                      const int32_t *__restrict__ mconn,
                                                      const double *__restrict__ x, double *__restrict__ ws,
                                                      const int *__restrict__ istate)
{
    if (istate && istate[I_REASON] != 0) return;
    constexpr int NE = 16 * NCT, SX = NE + 1;  // (odd row stride: the fill's lanes run along k)
    constexpr int NPT = EG_KC * NE / 256;      // x entries per thread and chunk: k row `lane`, elements wv + 4 i
    constexpr int KS = EG_KC / 4;              // k steps per chunk
    __shared__ double sX[EG_KC * SX];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int64_t e0 = eb + (int64_t)blockIdx.x * NE;              // elements [eb, E) of the launch's range
    const int rt0 = ((rg0 + (int)blockIdx.y) * 4 + wv) * EG_TR;  // this wave's first row tile (row groups from rg0)
    const int ntile = ndp >> 4, nks = ncp >> 2;

    const edbl4 z4 = {0.0, 0.0, 0.0, 0.0};
    edbl4 acc[EG_TR][NCT];
#pragma unroll
    for (int j = 0; j < EG_TR; ++j)
#pragma unroll
        for (int c = 0; c < NCT; ++c) acc[j][c] = z4;

    // Three loads deep: while chunk c runs its MFMAs, the x entries and the
    // K_e0 operands of chunk c + 1 and the node ids of chunk c + 2 are in
    // flight.  Node ids come through the masked connectivity (-1: dropped --
    // selection, the entry is never read; also beyond nc, E and the last chunk).
    int nr[NPT];
    double xr[NPT], ar[EG_TR][KS], an[EG_TR][KS];
    auto fetch_idx = [&](int k0) {
        const int g = k0 + lane;
        const int l = g / CW;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int64_t e = e0 + wv + 4 * i;
            if constexpr (DOF) nr[i] = g < nc && e < E ? mconn[e * nc + g] : -1;
            else nr[i] = g < nc && e < E ? mconn[e * nn + l] : -1;
        }
    };
    auto fetch_x = [&](int k0) {
        const int g = k0 + lane;
        const int a = g - (g / CW) * CW;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            if constexpr (DOF) xr[i] = nr[i] >= 0 ? x[nr[i]] : 0.0;
            else xr[i] = nr[i] >= 0 ? x[(int64_t)nr[i] * CW + a] : 0.0;
        }
    };
    // (a tile beyond the last re-reads the wave's first: its sums are never stored)
    auto fetch_a = [&](int k0, double (&t)[EG_TR][KS]) {
        const int nksc = max(min(EG_KC, ncp - k0), 0) >> 2;
        if (rt0 >= ntile) return;
#pragma unroll
        for (int j = 0; j < EG_TR; ++j) {
            const double *ka = kt + ((int64_t)(rt0 + j < ntile ? rt0 + j : rt0) * nks + (k0 >> 2)) * 64 + lane;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) t[j][ks] = ks < nksc ? ka[ks * 64] : 0.0;
        }
    };
    fetch_idx(0);
    fetch_a(0, ar);
    fetch_x(0);
    fetch_idx(EG_KC);
    for (int k0 = 0; k0 < ncp; k0 += EG_KC) {
        const int nksc = min(EG_KC, ncp - k0) >> 2;
#pragma unroll
        for (int i = 0; i < NPT; ++i) sX[lane * SX + wv + 4 * i] = xr[i];
        __syncthreads();
        fetch_x(k0 + EG_KC);
        fetch_idx(k0 + 2 * EG_KC);
        fetch_a(k0 + EG_KC, an);
        if (rt0 < ntile) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (ks < nksc) {
#pragma unroll
                    for (int c = 0; c < NCT; ++c) {
                        const double b = sX[(ks * 4 + kq) * SX + c * 16 + li];
#pragma unroll
                        for (int j = 0; j < EG_TR; ++j)
                            acc[j][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[j][ks], b, acc[j][c], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < EG_TR; ++j)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) ar[j][ks] = an[j][ks];
    }
#pragma unroll
    for (int j = 0; j < EG_TR; ++j)
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
            const int64_t e = e0 + c * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int l = (rt0 + j) * 16 + kq + 4 * r;
                if (rt0 + j < ntile && l < nd && e < E) ws[e * nd + l] = negate ? -acc[j][c][r] : acc[j][c][r];
            }
        }
}

template <int DIM>
__global__ __launch_bounds__(256) void k_elem_gather(int64_t N, int nn, int nd, int maxinc,
                                                     const int32_t *__restrict__ inc,
                                                     const uint8_t *__restrict__ dir,
                                                     const double *__restrict__ ws, const double *__restrict__ x,
                                                     double *__restrict__ y, const int *__restrict__ istate)
{
    if (istate && istate[I_REASON] != 0) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * DIM) return;
    const int64_t node = i / DIM;
    const int a = (int)(i - node * DIM);
    if (dir[node]) {
        // setIndices2One: unit Dirichlet diagonal of K and of Krhs; Rw (x null:
        // another column space) holds no entry in the row
        y[i] = x ? x[i] : 0.0;
        return;
    }
    double s = 0.0;
    for (int j = 0; j < maxinc; ++j) {
        const int t = inc[node * maxinc + j];
        if (t < 0) break;
        const int e = t / nn, l = t - e * nn;
        s += ws[(int64_t)e * nd + l * DIM + a];
    }
    y[i] = s;
}

// diagonal: the incident elements' K_e0 diagonal entries in the same order
// (K), 0 (Krhs: a free row holds Dirichlet columns only); 1 on Dirichlet rows
template <int DIM>
__global__ __launch_bounds__(256) void k_elem_diag(int64_t N, int nn, int maxinc, int which,
                                                   const int32_t *__restrict__ inc,
                                                   const uint8_t *__restrict__ dir,
                                                   const double *__restrict__ kdiag, double *__restrict__ d)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * DIM) return;
    const int64_t node = i / DIM;
    const int a = (int)(i - node * DIM);
    if (dir[node]) {
        d[i] = 1.0;
        return;
    }
    double s = 0.0;
    if (which == 0)
        for (int j = 0; j < maxinc; ++j) {
            const int t = inc[node * maxinc + j];
            if (t < 0) break;
            s += kdiag[(t % nn) * DIM + a];
        }
    d[i] = s;
}

// dst_i = src_i on the Dirichlet rows, nothing else touched
__global__ __launch_bounds__(256) void k_elem_copy_dirichlet(int64_t n, int dim, const uint8_t *__restrict__ dir,
                                                             const double *__restrict__ src, double *__restrict__ dst)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (dir[i / dim]) dst[i] = src[i];
}

// No-slip operators: one thread per owned DoF, its row by the rule byte of its
// class (MatNS.buildNS, mat_ns.py:47-145) -- zero (+0.0, nothing read), the
// identity (x_i bit for bit) or the sum of its node's incidence entries from
// the element results of pass 0 or pass 1, in table (ascending element) order
// like k_elem_gather; NS_MINUS_X adds -x_i (the -1 on Kfs's tangential
// diagonal).  x is null where the column space is the vorticity's (Rw, Rwfs:
// no rule of theirs reads it).
template <int DIM>
__global__ __launch_bounds__(256) void k_elem_gather_cls(int64_t N, int nn, int nd, int maxinc, unsigned rules,
                                                         const int32_t *__restrict__ inc,
                                                         const uint8_t *__restrict__ cls,
                                                         const double *__restrict__ ws0,
                                                         const double *__restrict__ ws1,
                                                         const double *__restrict__ x, double *__restrict__ y,
                                                         const int *__restrict__ istate)
{
    if (istate && istate[I_REASON] != 0) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * DIM) return;
    const unsigned r = (rules >> (8 * cls[i])) & 0xffu, kind = r & NS_KIND;
    if (kind == NS_ZERO) {
        y[i] = 0.0;
        return;
    }
    if (kind == NS_IDENT) {
        y[i] = x[i];
        return;
    }
    const int64_t node = i / DIM;
    const int a = (int)(i - node * DIM);
    const double *__restrict__ ws = kind == NS_SUM0 ? ws0 : ws1;
    double s = 0.0;
    for (int j = 0; j < maxinc; ++j) {
        const int t = inc[node * maxinc + j];
        if (t < 0) break;
        const int e = t / nn, l = t - e * nn;
        s += ws[(int64_t)e * nd + l * DIM + a];
    }
    if (r & NS_MINUS_X) s += -x[i];
    y[i] = s;
}

// diagonal by class: 0, 1 (identity rows), the incident elements' K_e0
// diagonal entries in gather order (a summed row whose own class is a kept
// column), those sums + (-1) (Kfs's tangential rows)
template <int DIM>
__global__ __launch_bounds__(256) void k_elem_diag_cls(int64_t N, int nn, int maxinc, unsigned drules,
                                                       const int32_t *__restrict__ inc,
                                                       const uint8_t *__restrict__ cls,
                                                       const double *__restrict__ kdiag, double *__restrict__ d)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * DIM) return;
    const unsigned r = (drules >> (8 * cls[i])) & 0xffu;
    if (r < 2) {
        d[i] = r ? 1.0 : 0.0;
        return;
    }
    const int64_t node = i / DIM;
    const int a = (int)(i - node * DIM);
    double s = 0.0;
    for (int j = 0; j < maxinc; ++j) {
        const int t = inc[node * maxinc + j];
        if (t < 0) break;
        s += kdiag[(t % nn) * DIM + a];
    }
    d[i] = r == 3 ? s + (-1.0) : s;
}

// dst_i = src_i on the identity rows of a no-slip operator, nothing else touched
__global__ __launch_bounds__(256) void k_elem_copy_ident_cls(int64_t n, unsigned rules, const uint8_t *__restrict__ cls,
                                                             const double *__restrict__ src, double *__restrict__ dst)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (((rules >> (8 * cls[i])) & NS_KIND) == NS_IDENT) dst[i] = src[i];
}

// Every index the device tables hold, checked on the host before upload: a
// bad table is an error code, never an out-of-range access.
// conn holds ext-local node ids in [0, next); inc covers the owned nodes, ext
// nodes [own0, own0 + N).  Elements [eghost, eint1) (run beside the halo) may
// name owned nodes only, and an element below eghost (the ghost layer) may be
// gathered only at its top-plane nodes l >= ltop.
int elem_validate(const std::vector<int32_t> &conn, const std::vector<int32_t> &inc, const ElemLayout &L, int nn,
                  int maxinc)
{
    const int64_t N = L.N, E = L.E;
    if (E < 1 || N < 1 || L.own0 < 0 || L.own0 + N > L.next || L.eghost < 0 || L.eghost > L.eint1 || L.eint1 > E ||
        L.ltop < 0 || L.ltop > nn)
        return fail(KLE_ERR_OUTOFRANGE, "element operator: inconsistent element ranges");
    if ((int64_t)conn.size() != E * nn || (int64_t)inc.size() != N * maxinc)
        return fail(KLE_ERR_SIZ, "element operator: table sizes do not match the mesh");
    for (int64_t k = 0; k < E * nn; ++k) {
        if (conn[k] < 0 || conn[k] >= L.next)
            return fail(KLE_ERR_OUTOFRANGE, "element operator: connectivity entry %lld = %d outside [0, %lld)",
                        (long long)k, conn[k], (long long)L.next);
        const int64_t e = k / nn;
        if (e >= L.eghost && e < L.eint1 && (conn[k] < L.own0 || conn[k] >= L.own0 + N))
            return fail(KLE_ERR_OUTOFRANGE, "element operator: interior element %lld names the ghost node %d",
                        (long long)e, conn[k]);
    }
    for (int64_t i = 0; i < N; ++i) {
        bool ended = false;
        int32_t prev = -1;
        for (int j = 0; j < maxinc; ++j) {
            const int32_t t = inc[i * maxinc + j];
            if (t < 0) {
                if (t != -1 || j == 0)
                    return fail(KLE_ERR_OUTOFRANGE, "element operator: node %lld has a bad incidence entry", (long long)i);
                ended = true;
                continue;
            }
            if (ended || (int64_t)t >= E * nn || conn[t] != i + L.own0 || (prev >= 0 && t / nn <= prev / nn) ||
                (t / nn < L.eghost && t % nn < L.ltop))
                return fail(KLE_ERR_OUTOFRANGE, "element operator: incidence entry %d of node %lld is inconsistent", j,
                            (long long)i);
            prev = t;
        }
    }
    return 0;
}

// elements [e0, e1), row groups from rg0 on
template <int CW>
static void launch_gemm(const ElemOp *P, int64_t e0, int64_t e1, int rg0, hipStream_t st, const double *x,
                        const int *istate)
{
    const int ne = 16 * P->nct;
    dim3 grid((unsigned)((e1 - e0 + ne - 1) / ne), (unsigned)((P->ndp + EG_ROWS - 1) / EG_ROWS - rg0));
#define KLE_ELEM_GEMM(NCT)                                                                                      \
    hipLaunchKernelGGL((k_elem_gemm<CW, NCT>), grid, dim3(256), 0, st, P->negate, P->nn, P->nd, P->ndp, P->nc, \
                       P->ncp, e0, e1, rg0, P->d_kt, P->d_conn, x, P->d_ws, istate)
    if (P->nct == 2) KLE_ELEM_GEMM(2);
    else KLE_ELEM_GEMM(1);
#undef KLE_ELEM_GEMM
}

// pass p of a no-slip operator with per-DoF columns: the same launch over the
// pass's index table and result array
template <int CW>
static void launch_gemm_dof(const ElemOp *P, int p, int64_t e0, int64_t e1, int rg0, hipStream_t st, const double *x,
                            const int *istate)
{
    const int ne = 16 * P->nct;
    dim3 grid((unsigned)((e1 - e0 + ne - 1) / ne), (unsigned)((P->ndp + EG_ROWS - 1) / EG_ROWS - rg0));
#define KLE_ELEM_GEMM(NCT)                                                                                       \
    hipLaunchKernelGGL((k_elem_gemm<CW, NCT, true>), grid, dim3(256), 0, st, P->negate, P->nn, P->nd, P->ndp, P->nc, \
                       P->ncp, e0, e1, rg0, P->d_kt, P->d_cidx[p], x, P->d_wsp[p], istate)
    if (P->nct == 2) KLE_ELEM_GEMM(2);
    else KLE_ELEM_GEMM(1);
#undef KLE_ELEM_GEMM
}

// The element launches of one product of an element-wise operator (kind 2),
// launch(e0, e1, ghost layer?) per element range.  One rank or local (timing:
// no halo): every element at once.  Several ranks: one forward halo of x; with
// overlap the interior elements run on the compute stream beside the halo on
// the comm stream, the ghost layer and the top layer after it -- as the
// node-block product's interior and ghost-dependent rows (kle_mat.hip spmv).
int elem_ranges(kle_mat *A, const kle_vec *x, bool local, const std::function<int(int64_t, int64_t, bool)> &launch)
{
    kle_ctx *c = A->ctx;
    // [0, g1) the ghost layer, [g1, i1) the interior, [i1, E) the top layer
    const int64_t E = A->el_n, g1 = A->el_ghost, i1 = A->el_int1;
    if (E < 1 || g1 < 0 || g1 > i1 || i1 > E) return fail(KLE_ERR_STATE, "element operator: bad element ranges");
    const bool overlap = c->nranks > 1 && !local && spmv_uses_comm_stream(A, x);
    if (!overlap) {
        if (c->nranks > 1 && !local)
            KLE_TRY(halo_exchange(c, x->base, x->ghost_lo, x->n_local, x->ghost_hi, x->lo_rank, x->hi_rank,
                                  x->send_lo, x->send_hi, nullptr, x->plan.get()));
        if (g1 > 0) KLE_TRY(launch(0, g1, true));
        return g1 < E ? launch(g1, E, false) : 0;
    }
    SideBusy busy(c);
    KLE_HIP(hipEventRecord(c->ev_x_ready, c->stream));
    KLE_HIP(hipStreamWaitEvent(c->comm_stream, c->ev_x_ready, 0));
    KLE_TRY(launch(g1, i1, false));  // (overlap only where g1 < i1: spmv_uses_comm_stream)
    KLE_TRY(halo_exchange(c, x->base, x->ghost_lo, x->n_local, x->ghost_hi, x->lo_rank, x->hi_rank, x->send_lo,
                          x->send_hi, c->comm_stream, x->plan.get()));
    KLE_HIP(hipEventRecord(c->ev_halo_done, c->comm_stream));
    KLE_HIP(hipStreamWaitEvent(c->stream, c->ev_halo_done, 0));
    if (g1 > 0) KLE_TRY(launch(0, g1, true));
    return i1 < E ? launch(i1, E, false) : 0;
}

// x and y of a product against the operator's layout: x a ghosted vector of
// the column space (read through its allocation in ext indices), y the owned rows
int elem_check_vecs(const kle_mat *A, const kle_vec *x, const kle_vec *y, const char *what)
{
    if (x->n_local != A->n_local || y->n_local != A->m_local || x->ghost_lo != A->ghost_lo ||
        x->ghost_hi != A->ghost_hi || !x->base || x->d != x->base + x->ghost_lo)
        return fail(KLE_ERR_SIZ, "%s: vector layout does not match", what);
    if (x->d == y->d) return fail(KLE_ERR_ARG, "%s: y must not alias x", what);
    return 0;
}

int elem_spmv(kle_mat *A, const kle_vec *x, kle_vec *y, const int *istate, bool local)
{
    const ElemOp *P = A->elem;
    if (!P) return fail(KLE_ERR_STATE, "element operator without tables");
    KLE_TRY(elem_check_vecs(A, x, y, "element operator"));
    hipStream_t st = A->ctx->stream;
    KLE_TRY(elem_ranges(A, x, local, [&](int64_t e0, int64_t e1, bool ghost) -> int {
        const int rg0 = ghost && g_tune.elem_ghost_rows ? P->rg_top : 0;
        if (P->dofcols) {
            // (per-DoF columns: the column space is the velocity's, cw = dim)
            for (int p = 0; p < P->npass; ++p) {
                if (P->cw == 2) launch_gemm_dof<2>(P, p, e0, e1, rg0, st, x->base, istate);
                else launch_gemm_dof<3>(P, p, e0, e1, rg0, st, x->base, istate);
            }
            KLE_HIP(hipGetLastError());
            return 0;
        }
        if (P->cw == 1) launch_gemm<1>(P, e0, e1, rg0, st, x->base, istate);
        else if (P->cw == 2) launch_gemm<2>(P, e0, e1, rg0, st, x->base, istate);
        else launch_gemm<3>(P, e0, e1, rg0, st, x->base, istate);
        KLE_HIP(hipGetLastError());
        return 0;
    }));
    const int64_t n = P->N * P->dim;
    dim3 gg((unsigned)((n + 255) / 256));
    if (P->ns) {
        // (Rw, Rwfs: x is the vorticity -- their rules, zero and sum, never read it)
        const double *xv = P->dofcols ? x->d : nullptr;
        if (P->dim == 2)
            hipLaunchKernelGGL(k_elem_gather_cls<2>, gg, dim3(256), 0, st, P->N, P->nn, P->nd, P->maxinc, P->rules,
                               P->d_inc, P->d_cls, P->d_wsp[0], P->d_wsp[1], xv, y->d, istate);
        else
            hipLaunchKernelGGL(k_elem_gather_cls<3>, gg, dim3(256), 0, st, P->N, P->nn, P->nd, P->maxinc, P->rules,
                               P->d_inc, P->d_cls, P->d_wsp[0], P->d_wsp[1], xv, y->d, istate);
        KLE_HIP(hipGetLastError());
        return 0;
    }
    const double *xd = P->which == 2 ? nullptr : x->d;  // Rw: no Dirichlet diagonal, x is never read by the gather
    if (P->dim == 2)
        hipLaunchKernelGGL(k_elem_gather<2>, gg, dim3(256), 0, st, P->N, P->nn, P->nd, P->maxinc, P->d_inc, P->d_dir,
                           P->d_ws, xd, y->d, istate);
    else
        hipLaunchKernelGGL(k_elem_gather<3>, gg, dim3(256), 0, st, P->N, P->nn, P->nd, P->maxinc, P->d_inc, P->d_dir,
                           P->d_ws, xd, y->d, istate);
    KLE_HIP(hipGetLastError());
    return 0;
}

int elem_diagonal(const kle_mat *A, kle_vec *d)
{
    const ElemOp *P = A->elem;
    if (!P) return fail(KLE_ERR_STATE, "element operator without tables");
    if (P->ns ? !P->dofcols : P->which == 2)
        return fail(KLE_ERR_SUP, "getDiagonal: the element-wise Rw is rectangular");
    hipStream_t st = A->ctx->stream;
    const int64_t n = P->N * P->dim;
    dim3 gg((unsigned)((n + 255) / 256));
    if (P->ns) {
        if (P->dim == 2)
            hipLaunchKernelGGL(k_elem_diag_cls<2>, gg, dim3(256), 0, st, P->N, P->nn, P->maxinc, P->drules, P->d_inc,
                               P->d_cls, P->d_kdiag, d->d);
        else
            hipLaunchKernelGGL(k_elem_diag_cls<3>, gg, dim3(256), 0, st, P->N, P->nn, P->maxinc, P->drules, P->d_inc,
                               P->d_cls, P->d_kdiag, d->d);
    } else if (P->dim == 2)
        hipLaunchKernelGGL(k_elem_diag<2>, gg, dim3(256), 0, st, P->N, P->nn, P->maxinc, P->which, P->d_inc, P->d_dir,
                           P->d_kdiag, d->d);
    else
        hipLaunchKernelGGL(k_elem_diag<3>, gg, dim3(256), 0, st, P->N, P->nn, P->maxinc, P->which, P->d_inc, P->d_dir,
                           P->d_kdiag, d->d);
    KLE_HIP(hipGetLastError());
    KLE_HIP(hipStreamSynchronize(st));
    return 0;
}

void elem_drop(kle_mat *A)
{
    ElemOp *P = A->elem;
    if (!P) return;
    (void)hipFree(P->d_kt);
    (void)hipFree(P->d_kdiag);
    (void)hipFree(P->d_ws);
    (void)hipFree(P->d_conn);
    (void)hipFree(P->d_inc);
    (void)hipFree(P->d_dir);
    (void)hipFree(P->d_cidx[0]);
    (void)hipFree(P->d_cidx[1]);
    (void)hipFree(P->d_wsp[1]);  // (d_wsp[0] is d_ws)
    (void)hipFree(P->d_cls);
    delete P;
    A->elem = nullptr;
}

// Algorithmic bytes of one product: element matrix, connectivity, incidence
// and Dirichlet tables, x read, y written, the element results written and read.
double elem_spmv_bytes(const kle_mat *A)
{
    const ElemOp *P = A->elem;
    if (!P) return 0.0;
    if (P->ns)  // the index tables (per DoF: nc entries per element and pass) and the class bytes instead
        return 8.0 * P->nd * P->nc + 4.0 * P->E * (P->dofcols ? P->nc * P->npass : P->nn) + 4.0 * P->N * P->maxinc +
               1.0 * P->N * P->dim + 8.0 * (A->n_local + A->ghost_lo + A->ghost_hi) + 8.0 * A->m_local +
               2.0 * 8.0 * P->E * P->nd * P->npass;
    return 8.0 * P->nd * P->nc + 4.0 * P->E * P->nn + 4.0 * P->N * P->maxinc + 1.0 * P->N +
           8.0 * (A->n_local + A->ghost_lo + A->ghost_hi) + 8.0 * A->m_local + 2.0 * 8.0 * P->E * P->nd;
}

std::string elem_kernel_name(const kle_mat *A)
{
    const ElemOp *P = A->elem;
    if (!P) return "?";
    if (P->ns)
        return "k_elem_gemm<" + std::to_string(P->cw) + "," + std::to_string(P->nct) + (P->dofcols ? ",1>" : ">") +
               (P->npass == 2 ? "x2" : "") + "+k_elem_gather_cls<" + std::to_string(P->dim) + ">";
    return "k_elem_gemm<" + std::to_string(P->cw) + "," + std::to_string(P->nct) + ">+k_elem_gather<" +
           std::to_string(P->dim) + ">";
}

// The part of a box mesh an element-wise operator on ctx works on.  The mesh's
// partition must be the context's (a one-rank context takes no part of a
// several-rank mesh); the 32-bit tables bound the local sizes, bw the widest
// block of the operator.
int elem_layout(const kle_ctx *ctx, const kle_mesh *m, int bw, ElemLayout *out)
{
    if (m->kind != 0)
        return fail(KLE_ERR_SUP, "element-wise operator: needs a uniform box mesh (unstructured mesh given)");
    if (m->nranks != ctx->nranks)
        return fail(KLE_ERR_SUP, "element-wise operator: the mesh is partitioned for %d ranks, the context has %d",
                    m->nranks, ctx->nranks);
    KLE_ARG(m->rank == ctx->rank, "mesh partition does not match ctx");
    ElemLayout L;
    L.N = m->node_end - m->node_begin;
    L.next = m->ext_end - m->ext_begin;
    L.own0 = m->node_begin - m->ext_begin;
    L.E = m->elem_end - m->elem_begin;
    L.eghost = m->rank > 0 ? m->elem_layer : 0;
    L.eint1 = m->rank < m->nranks - 1 ? L.E - m->elem_layer : L.E;
    L.ltop = m->nn() - m->nn() / m->ngl;
    KLE_ARG(L.E >= 1 && L.N >= 1 && L.own0 >= 0 && L.own0 + L.N <= L.next && L.eghost <= L.eint1 &&
                (m->nranks > 1 || (L.own0 == 0 && L.next == L.N && m->node_begin == 0)),
            "unexpected slab layout");
    if (L.E * m->nn() >= INT32_MAX || L.next * bw >= INT32_MAX)
        return fail(KLE_ERR_SUP, "element-wise operator: the mesh exceeds the 32-bit tables");
    *out = L;
    return 0;
}

// conn [E][nn] in ext-local node ids and the owned nodes' incidence lists
// inc [N][maxinc] (e * nn + l, ascending e, -1 padded), validated
int elem_tables(const kle_mesh *m, const ElemLayout &L, std::vector<int32_t> &conn, std::vector<int32_t> &inc)
{
    const int nn = m->nn(), maxinc = 1 << m->dim;
    std::vector<int64_t> conn64((size_t)L.E * nn);
    KLE_TRY(kle_mesh_get_conn(m, conn64.data()));
    conn.assign((size_t)L.E * nn, 0);
    inc.assign((size_t)L.N * maxinc, -1);
    std::vector<uint8_t> cnt((size_t)L.N, 0);
    for (int64_t k = 0; k < L.E * nn; ++k) {
        const int64_t g = conn64[k] - m->ext_begin;
        if (g < 0 || g >= L.next)
            return fail(KLE_ERR_OUTOFRANGE, "element operator: connectivity entry %lld outside the mesh", (long long)k);
        conn[k] = (int32_t)g;
        const int64_t o = g - L.own0;
        if (o < 0 || o >= L.N) continue;  // a ghost node: read, never written
        if (cnt[o] >= maxinc)
            return fail(KLE_ERR_OUTOFRANGE, "element operator: node %lld lies in more than %d elements",
                        (long long)conn64[k], maxinc);
        inc[o * maxinc + cnt[o]++] = (int32_t)k;  // k = e * nn + l, ascending e
    }
    return elem_validate(conn, inc, L, nn, maxinc);
}

// sizes, ownership and the column space's halo plan, as kle_assemble_kle sets
// them for a node-block matrix of R x C blocks on the same mesh
void elem_mat_fields(kle_mat *A, const kle_mesh *m, const ElemLayout &L, int R, int C)
{
    A->kind = 2;
    A->R = R;
    A->C = C;
    A->nrows = L.N;
    A->m_local = L.N * R;
    A->n_local = L.N * C;
    A->m_global = m->N * R;
    A->n_global = m->N * C;
    A->row_lo = m->node_begin * R;
    A->col_lo = m->node_begin * C;
    A->node_begin = m->node_begin;
    A->ext_begin = m->ext_begin;
    A->ext_nodes = L.next;
    A->lo_rank = m->halo_lo_rank;
    A->hi_rank = m->halo_hi_rank;
    A->ghost_lo = L.own0 * C;
    A->ghost_hi = (L.next - L.own0 - L.N) * C;
    A->send_lo = m->send_lo_nodes * C;
    A->send_hi = m->send_hi_nodes * C;
    A->el_n = L.E;
    A->el_ghost = L.eghost;
    A->el_int1 = L.eint1;
    if (const char *e = getenv("KLE_HALO_OVERLAP")) A->halo_overlap = atoi(e) != 0;
}

// A one-element, one-rank mesh holding global element 0 of m: every rank
// forms K_e0 and the operator geometry from the same corners, so the tables
// are the same bits whatever the partition.
void first_element_mesh(const kle_mesh *m, kle_mesh *o)
{
    o->dim = m->dim;
    o->ngl = m->ngl;
    o->p = m->p;
    for (int d = 0; d < 3; ++d) {
        o->nel[d] = m->nel[d];
        o->L[d] = m->L[d];
        o->lower[d] = m->lower[d];
        o->upper[d] = m->upper[d];
        o->h[d] = m->h[d];
    }
    o->N = m->N;
    o->E = m->E;
    o->xi = m->xi;
    o->axis = m->axis;
    o->plane = m->plane;
    o->elem_layer = m->elem_layer;
    o->elem_begin = 0;
    o->elem_end = 1;
}

// K_e0 (rw: Rw_e0) of global element 0 through the assembly's own geometry
// and element kernels: kt zero-padded to ndp x ncp in MFMA operand order,
// kdiag its diagonal (K_e0 only)
static int elem_first_operand(kle_ctx *ctx, const kle_mesh *m, bool rw, int cw, std::vector<double> &kt,
                              std::vector<double> &kdiag)
{
    const int dim = m->dim, nn = m->nn(), nd = dim * nn, ndp = (nd + 15) & ~15, nc = cw * nn, ncp = (nc + 3) & ~3;
    kle_mesh m0;
    first_element_mesh(m, &m0);
    double *dKe = nullptr, *dRwe = nullptr;
    KLE_TRY(element_first_k(ctx, &m0, &dKe, rw ? &dRwe : nullptr));
    std::vector<double> kb((size_t)nd * nc);
    hipError_t he = hipMemcpy(kb.data(), rw ? dRwe : dKe, sizeof(double) * kb.size(), hipMemcpyDeviceToHost);
    (void)hipFree(dKe);
    (void)hipFree(dRwe);
    if (he != hipSuccess) return fail(KLE_ERR_DEVICE, "element matrix download failed: %s", hipGetErrorString(he));
    // blocks [l][m][a][b], b < cw -> K[l dim + a][m cw + b], zero-padded to ndp x ncp, in operand order
    auto kat = [&](int r, int c) {
        return kb[(((size_t)(r / dim) * nn + c / cw) * dim + r % dim) * cw + c % cw];
    };
    kt.assign((size_t)ndp * ncp, 0.0);
    kdiag.assign((size_t)(rw ? 0 : nd), 0.0);
    const int nks = ncp / 4;
    for (int rt = 0; rt < ndp / 16; ++rt)
        for (int ks = 0; ks < nks; ++ks)
            for (int lane = 0; lane < 64; ++lane) {
                const int r = rt * 16 + (lane & 15), c = ks * 4 + (lane >> 4);
                if (r < nd && c < nc) kt[((size_t)rt * nks + ks) * 64 + lane] = kat(r, c);
            }
    for (size_t r = 0; r < kdiag.size(); ++r) kdiag[r] = kat((int)r, (int)r);
    return 0;
}

// a device array of an element-wise operator, filled from src where given
template <class T>
static int elem_upload(T **dp, const void *src, size_t bytes)
{
    if (hipMalloc(dp, bytes) != hipSuccess) {
        (void)hipGetLastError();
        *dp = nullptr;
        return fail(KLE_ERR_MEM, "out of device memory for the element-wise operator");
    }
    return src ? h2d(*dp, src, bytes) : 0;
}

}  // namespace kle

using namespace kle;

extern "C" int kle_mat_copy_dirichlet_rows(const kle_mat *A, const kle_vec *src, kle_vec *dst)
{
    KLE_ARG(A && src && dst, "null arg");
    if (A->kind == 2 && A->sumfac) return sumfac_copy_ident_rows(A, src, dst);
    if (A->kind != 2 || !A->elem)
        return fail(KLE_ERR_SUP, "copyDirichletRows: an element-wise operator only (it holds the Dirichlet flags)");
    const ElemOp *P = A->elem;
    const int64_t n = P->N * P->dim;
    if (src->n_local != n || dst->n_local != n)
        return fail(KLE_ERR_SIZ, "copyDirichletRows: vectors do not match the operator's rows");
    if (src->d == dst->d) return 0;
    if (P->ns)  // a no-slip operator: its identity rows, by DoF class
        hipLaunchKernelGGL(k_elem_copy_ident_cls, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, A->ctx->stream, n,
                           P->rules, P->d_cls, src->d, dst->d);
    else
        hipLaunchKernelGGL(k_elem_copy_dirichlet, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, A->ctx->stream, n,
                           P->dim, P->d_dir, src->d, dst->d);
    KLE_HIP(hipGetLastError());
    return 0;
}

extern "C" int kle_mat_create_kle_element(kle_ctx *ctx, kle_mesh *m, int which, kle_mat **out)
{
    KLE_ARG(ctx && m && out, "null arg");
    KLE_ARG(which >= 0 && which <= 2, "which must be 0 (K), 1 (Krhs) or 2 (Rw)");
    if (m->kind != 0) return fail(KLE_ERR_SUP, "element-wise operator: needs a uniform box mesh (unstructured mesh given)");
    if (!m->dof_cls.empty()) return fail(KLE_ERR_SUP, "element-wise operator: no-slip meshes are not supported");
    // rows nd = dim nn (padded to the row tile); columns nc = cw nn (padded to the k step)
    const int dim = m->dim, nn = m->nn(), nd = dim * nn, ndp = (nd + 15) & ~15, maxinc = 1 << dim;
    const int cw = which == 2 ? (dim == 2 ? 1 : 3) : dim, nc = cw * nn, ncp = (nc + 3) & ~3;
    ElemLayout L;
    KLE_TRY(elem_layout(ctx, m, std::max(dim, cw), &L));
    KLE_ARG(m->dir_set, "Dirichlet nodes not set (kle_mesh_set_dirichlet_*)");
    const int64_t E = L.E, N = L.N;
    if ((int64_t)m->dir.size() != L.next)
        return fail(KLE_ERR_SIZ, "element operator: Dirichlet flags do not match the mesh");

    // tables (host) in ext-local node ids, validated before upload
    std::vector<int32_t> conn, inc;
    KLE_TRY(elem_tables(m, L, conn, inc));
    // the mask rule folded into the connectivity the GEMM reads: K drops the
    // Dirichlet entries of x (ghosts included: m->dir covers the ext range),
    // Krhs the free ones, Rw none
    if (which != 2)
        for (int64_t k = 0; k < E * nn; ++k)
            if ((m->dir[conn[k]] != 0) != (which == 1)) conn[k] = -1;

    KLE_HIP(hipSetDevice(ctx->device));
    std::vector<double> kt, kdiag;
    KLE_TRY(elem_first_operand(ctx, m, which == 2, cw, kt, kdiag));

    kle_mat *A = new kle_mat;
    ElemOp *P = new ElemOp;
    A->ctx = ctx;
    A->elem = P;
    elem_mat_fields(A, m, L, dim, cw);
    P->which = which;
    P->negate = which == 1;
    P->dim = dim;
    P->cw = cw;
    P->nn = nn;
    P->nd = nd;
    P->ndp = ndp;
    P->nc = nc;
    P->ncp = ncp;
    P->maxinc = maxinc;
    P->E = E;
    P->N = N;
    // element columns per held K_e0 operand: two tiles of 16 where that still
    // gives every CU a workgroup, else one (four would spill the operand
    // double buffer out of 256 VGPRs); E the local elements
    const int64_t nrg = (ndp + EG_ROWS - 1) / EG_ROWS;
    P->rg_top = (nd - nd / m->ngl) / EG_ROWS;
    P->nct = (E + 31) / 32 * nrg >= ctx->num_cus ? 2 : 1;
    int rc = elem_upload(&P->d_kt, kt.data(), sizeof(double) * kt.size());
    if (!rc && !kdiag.empty()) rc = elem_upload(&P->d_kdiag, kdiag.data(), sizeof(double) * kdiag.size());
    if (!rc) rc = elem_upload(&P->d_conn, conn.data(), sizeof(int32_t) * conn.size());
    if (!rc) rc = elem_upload(&P->d_inc, inc.data(), sizeof(int32_t) * inc.size());
    if (!rc) rc = elem_upload(&P->d_dir, m->dir.data() + L.own0, (size_t)N);
    if (!rc) rc = elem_upload(&P->d_ws, nullptr, sizeof(double) * (size_t)E * nd);
    if (rc) {
        kle_mat_destroy(A);
        return rc;
    }
    *out = A;
    return 0;
}

// The no-slip operators of MatNS.buildNS (mat_ns.py:47-145) in element-wise
// form: NS_SPECS (kle_internal.hpp) with the element GEMM as the pass.
extern "C" int kle_mat_create_ns_element(kle_ctx *ctx, kle_mesh *m, int which, kle_mat **out)
{
    KLE_ARG(ctx && m && out, "null arg");
    KLE_ARG(which >= 0 && which <= 6, "which must be 0 (K), 1 (Krhs), 2 (Rw), 3 (Kfs), 4 (Krhsfs), 5 (Rwfs) or 6 (K + Kfs)");
    if (m->kind != 0) return fail(KLE_ERR_SUP, "element-wise operator: needs a uniform box mesh (unstructured mesh given)");
    if (m->dof_cls.empty())
        return fail(KLE_ERR_SUP, "element-wise no-slip operator: the mesh has no no-slip DoFs (kle_mesh_set_noslip_*)");
    const NsSpec &S = NS_SPECS[which];
    const int dim = m->dim, nn = m->nn(), nd = dim * nn, ndp = (nd + 15) & ~15, maxinc = 1 << dim;
    const int cw = S.rw ? (dim == 2 ? 1 : 3) : dim, nc = cw * nn, ncp = (nc + 3) & ~3;
    ElemLayout L;
    KLE_TRY(elem_layout(ctx, m, std::max(dim, cw), &L));
    const int64_t E = L.E, N = L.N;
    if ((int64_t)m->dof_cls.size() != L.next * dim)
        return fail(KLE_ERR_SIZ, "element operator: DoF classes do not cover the mesh's ext range");
    for (size_t k = 0; k < m->dof_cls.size(); ++k)
        if (m->dof_cls[k] > DOF_NORMAL)
            return fail(KLE_ERR_OUTOFRANGE, "element operator: DoF %lld has the unknown class %d", (long long)k,
                        (int)m->dof_cls[k]);
    if (E * nc >= INT32_MAX) return fail(KLE_ERR_SUP, "element-wise operator: the mesh exceeds the 32-bit tables");

    // tables (host) in ext-local ids, validated before upload
    std::vector<int32_t> conn, inc, cidx[2];
    KLE_TRY(elem_tables(m, L, conn, inc));
    if (!S.rw) {
        // per element and column (l, b): the ext-local x index conn * dim + b where
        // the pass keeps the DoF's class, else -1 (ghost DoFs: dof_cls covers the ext range)
        const int64_t xmax = L.next * cw;
        for (int p = 0; p < S.npass; ++p) {
            cidx[p].assign((size_t)E * nc, -1);
            for (int64_t e = 0; e < E; ++e)
                for (int g = 0; g < nc; ++g) {
                    const int64_t xi = (int64_t)conn[e * nn + g / dim] * dim + g % dim;
                    if (xi < 0 || xi >= xmax)
                        return fail(KLE_ERR_OUTOFRANGE, "element operator: column %d of element %lld outside the x range",
                                    g, (long long)e);
                    if ((S.cols[p] >> m->dof_cls[xi]) & 1u) cidx[p][e * nc + g] = (int32_t)xi;
                }
            for (int64_t k = 0; k < E * nc; ++k)
                if (cidx[p][k] < -1 || cidx[p][k] >= xmax)
                    return fail(KLE_ERR_OUTOFRANGE, "element operator: index table entry %lld = %d outside [-1, %lld)",
                                (long long)k, cidx[p][k], (long long)xmax);
        }
    }

    KLE_HIP(hipSetDevice(ctx->device));
    std::vector<double> kt, kdiag;
    KLE_TRY(elem_first_operand(ctx, m, S.rw, cw, kt, kdiag));

    kle_mat *A = new kle_mat;
    ElemOp *P = new ElemOp;
    A->ctx = ctx;
    A->elem = P;
    elem_mat_fields(A, m, L, dim, cw);
    P->which = which;
    P->ns = 1;
    P->negate = S.negate;
    P->npass = S.npass;
    P->dofcols = !S.rw;
    P->dim = dim;
    P->cw = cw;
    P->nn = nn;
    P->nd = nd;
    P->ndp = ndp;
    P->nc = nc;
    P->ncp = ncp;
    P->maxinc = maxinc;
    P->E = E;
    P->N = N;
    ns_rule_words(S, &P->rules, &P->drules);
    // (element columns per held operand and the ghost layer's row groups: as kle_mat_create_kle_element)
    const int64_t nrg = (ndp + EG_ROWS - 1) / EG_ROWS;
    P->rg_top = (nd - nd / m->ngl) / EG_ROWS;
    P->nct = (E + 31) / 32 * nrg >= ctx->num_cus ? 2 : 1;
    int rc = elem_upload(&P->d_kt, kt.data(), sizeof(double) * kt.size());
    if (!rc && !kdiag.empty()) rc = elem_upload(&P->d_kdiag, kdiag.data(), sizeof(double) * kdiag.size());
    if (!rc && S.rw) rc = elem_upload(&P->d_conn, conn.data(), sizeof(int32_t) * conn.size());
    for (int p = 0; p < S.npass && !rc && !S.rw; ++p)
        rc = elem_upload(&P->d_cidx[p], cidx[p].data(), sizeof(int32_t) * cidx[p].size());
    if (!rc) rc = elem_upload(&P->d_inc, inc.data(), sizeof(int32_t) * inc.size());
    if (!rc) rc = elem_upload(&P->d_cls, m->dof_cls.data() + L.own0 * dim, (size_t)N * dim);
    if (!rc) rc = elem_upload(&P->d_ws, nullptr, sizeof(double) * (size_t)E * nd);
    P->d_wsp[0] = P->d_ws;
    if (!rc && S.npass == 2) rc = elem_upload(&P->d_wsp[1], nullptr, sizeof(double) * (size_t)E * nd);
    if (rc) {
        kle_mat_destroy(A);
        return rc;
    }
    *out = A;
    return 0;
}
