// kle_colloc.hip -- element-wise Curl, SrT and DivSrT (kle_mat kind 2 with
// colloc set): no assembled values.  Of a uniform box mesh with one element's
// geometry (kle_mat_create_operator_element), of any mesh with every
// element's own (kle_mat_create_operator_sumfac, at the end of this header).
//
// The operators (kle_assemble.hip "operators") are collocation operators on
// the GLL nodes: row (l, a) of an element matrix M_e holds entries only at the
// nodes on the dim grid lines through l, each c_l (+-1 | 1/2) inv J D[l_k][m_k].
// kle_mesh_create_box makes every element the same brick, so with M_e0 the
// first element's matrix
//
//     y = Winv  sum over elements e of  S_e^T  M_e0  S_e^c x,
//
// Winv the inverse of the lumped nodal weight W_n = sum_e c_0[l(n)], and
// M_e0 x_e is sum-factorised: dim 1-D derivative passes along the grid lines.
//
//   k_colloc_elem<DIM, OP>  a 256-thread workgroup takes a batch of whole
//       elements (as many as fit 256 threads, at least one) and gathers their
//       x entries through the connectivity into LDS, component-major
//       [CW][element][k][j][i] with odd line, plane and element strides (in
//       doubles).  One thread per (element, node), looping where an element
//       has more than 256 nodes: for every column component the dim line sums
//       sum_m D[l_k][m] x_b(m), m ascending, then inv J (the assembly's H),
//       the operator's coefficient placement (colloc_coef: that of
//       k_ops_gather), times c_l; the RW row components go to ws[e][l][a].
//   k_colloc_gather<RW>     one thread per node: its incidence entries of ws
//       in table (ascending element) order, times winv[node].
//
// No atomics, fixed order: the product is repeatable bit for bit.  Both
// kernels do nothing once the Krylov reason word is set.  The operators carry
// no boundary rule, so no Dirichlet or no-slip table is read.
//
// Several ranks (slabs of whole element layers): as the element-wise K
// (kle_elem.hip) -- the connectivity in ext-local node ids over every element
// touching an owned node, x read through the vector's ghosted allocation after
// one forward halo, winv and the incidence lists for the owned nodes, whose
// incident elements are all local, the element kernel launched over element
// ranges (elem_ranges: the interior beside the halo, the ghost layer and the
// top layer after it).  A workgroup takes whole elements, so the ghost layer
// is computed whole although only its top plane is gathered.  geo is that of
// global element 0 on every rank: the owned rows are the one-rank product's
// bit for bit.
//
// Per-element geometry (any mesh, box or unstructured; several ranks: the
// element lists of kle_sumfac.hip):
//
//     y = Winv  sum over elements e of  S_e^T  M_e  S_e^c x,
//
//   k_colloc_elem<DIM, OP, true>  the same kernel reading c_l and inv J of its
//       own element from the nodal table [E][nn][1 + dim^2] that k_geometry
//       fills at the operator points (the one kle_assemble_operators builds
//       for k_ops_gather_u; the mesh's shared set, mesh_geometry).
//   k_colloc_gather_csr<RW>  one thread per node: its incidence entries of ws
//       through a CSR list (inc_ptr, inc_idx = e nn + l, ascending e: any
//       valence), times winv[node].
//   k_colloc_weights         once at creation: winv = 1 / sum of the incident
//       c_{e,l}, in incidence order (k_ops_weights_u's sum, so the weights
//       are the assembled operators' bit for bit).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "kle_basis.hpp"
#include "kle_internal.hpp"

namespace kle {

constexpr int CL_SD = 9;     // row stride of the derivative table in LDS (odd, >= 8)
constexpr int CL_SC3 = 584;  // doubles per component, 3-D: one ngl 8 element, strides 9 / 73 / 584
constexpr int CL_SC2 = 448;  // 2-D: 64 ngl 2 elements, strides 3 / 7

struct CollocOp {
    int which = 0, dim = 3, cw = 3, rw = 3, ngl = 0, nn = 0, maxinc = 8;
    int neb = 1, sy = 0, sz = 0, se = 0;  // elements per workgroup; LDS line, plane and element strides
    int64_t E = 0, N = 0;       // local elements, owned nodes
    double *d_dh = nullptr;     // [ngl][ngl] 1-D derivative table
    double *d_geo = nullptr;    // [nn][1 + dim^2] c_l, inv J of the first element
    double *d_winv = nullptr;   // [N] 1 / lumped nodal weight of the owned nodes
    double *d_ws = nullptr;     // [E][nn][rw] element results
    int32_t *d_conn = nullptr;  // [E][nn] element -> ext-local node, tensor order
    int32_t *d_inc = nullptr;   // [N][maxinc] owned node -> e * nn + l, ascending e, -1 padded
    // per-element geometry (kle_mat_create_operator_sumfac): d_geo is the nodal
    // table [E][nn][1 + dim^2] of the mesh's set, d_inc a CSR list [ninc] behind d_incp
    bool per_elem = false;
    std::shared_ptr<GeoSet> geo;
    int32_t *d_incp = nullptr;  // [N + 1]
    int64_t ninc = 0;
    int32_t *d_elist = nullptr;  // several ranks: [E] the inner, then the outer elements (kle_sumfac.hip)
};

// OP 0 Curl [dim_w x dim], 1 SrT [dim_s x dim], 2 DivSrT [dim x dim_s]
__host__ __device__ constexpr int colloc_rw(int dim, int op)
{
    return op == 0 ? (dim == 2 ? 1 : 3) : op == 1 ? (dim == 2 ? 3 : 6) : dim;
}
__host__ __device__ constexpr int colloc_cw(int dim, int op) { return op == 2 ? (dim == 2 ? 3 : 6) : dim; }

// Coefficient of d x_b / d x_d in row component a: the placement of
// k_ops_gather (spectral.py indCurl with signs (-1)^i; strain order xx, xy,
// yy, yz, zz, zx with the 0.5 on the shear terms; indBdiv).  The kernel and
// the creation check both read it from here.
template <int DIM, int OP>
__host__ __device__ constexpr double colloc_coef(int a, int b, int d)
{
    if (DIM == 3 && OP == 0) {
        return (a == 0 && b == 2 && d == 1) || (a == 1 && b == 0 && d == 2) || (a == 2 && b == 1 && d == 0)   ? 1.0
               : (a == 0 && b == 1 && d == 2) || (a == 1 && b == 2 && d == 0) || (a == 2 && b == 0 && d == 1) ? -1.0
                                                                                                               : 0.0;
    } else if (DIM == 2 && OP == 0) {
        return (b == 1 && d == 0) ? 1.0 : (b == 0 && d == 1) ? -1.0 : 0.0;
    } else {
        // strain component s <-> (velocity component v, derivative d): s = pair(v, d)
        const int s = OP == 1 ? a : b, v = OP == 1 ? b : a;
        int p = -1;
        if (DIM == 3) {
            const int pair3[3][3] = {{0, 1, 5}, {1, 2, 3}, {5, 3, 4}};
            p = pair3[v][d];
        } else {
            const int pair2[2][2] = {{0, 1}, {1, 2}};
            p = pair2[v][d];
        }
        if (p != s) return 0.0;
        return OP == 1 && v != d ? 0.5 : 1.0;
    }
}

// PE: geo holds every element's table, [E][nn][G1], instead of the first element's
// LIST: [eb, E) are positions of elist, which names the elements (several ranks
// with PE: the inner or the outer list); conn, geo and ws stay indexed by the
// element's own id, the LDS tile by its place in the batch
template <int DIM, int OP, bool PE = false, bool LIST = false>
__global__ __launch_bounds__(256) void k_colloc_elem(int ngl, int nn, int neb, int sy, int sz, int se, int64_t eb,
                                                     int64_t E,
                                                     const double *__restrict__ dh, const double *__restrict__ geo,
                                                     const int32_t *__restrict__ conn, const double *__restrict__ x,
                                                     double *__restrict__ ws, const int *__restrict__ istate,
                                                     const int32_t *__restrict__ elist)
{
    if (istate && istate[I_REASON] != 0) return;
    constexpr int CW = colloc_cw(DIM, OP), RW = colloc_rw(DIM, OP), G1 = 1 + DIM * DIM;
    constexpr int SC = DIM == 3 ? CL_SC3 : CL_SC2;
    __shared__ double sx[CW * SC];
    __shared__ double sd[8 * CL_SD];
    const int tid = threadIdx.x;
    const int64_t e0 = eb + (int64_t)blockIdx.x * neb;  // elements [eb, E) of the launch's range
    const int nt = (int)min((int64_t)neb, E - e0) * nn;  // (element, node) pairs of this batch
    const int64_t t0 = e0 * nn;
    if (tid < ngl * ngl) sd[(tid / ngl) * CL_SD + tid % ngl] = dh[tid];
    for (int t = tid; t < nt; t += 256) {
        const int el = t / nn, l = t - el * nn;
        const int i = l % ngl, r = l / ngl, j = DIM == 3 ? r % ngl : r, k = DIM == 3 ? r / ngl : 0;
        const int p = el * se + k * sz + j * sy + i;
        const int64_t node = conn[LIST ? (int64_t)elist[e0 + el] * nn + l : t0 + t];
#pragma unroll
        for (int b = 0; b < CW; ++b) sx[b * SC + p] = x[node * CW + b];
    }
    __syncthreads();
    for (int t = tid; t < nt; t += 256) {
        const int el = t / nn, l = t - el * nn;
        const int i = l % ngl, r = l / ngl, j = DIM == 3 ? r % ngl : r, k = DIM == 3 ? r / ngl : 0;
        const int base = el * se + k * sz + j * sy + i;
        // line sums along x, y (, z) of every component, m ascending
        double h[CW][DIM];
#pragma unroll
        for (int b = 0; b < CW; ++b)
#pragma unroll
            for (int d = 0; d < DIM; ++d) h[b][d] = 0.0;
        for (int m = 0; m < ngl; ++m) {
            int o[DIM];
            double dm[DIM];
            o[0] = base + (m - i);
            o[1] = base + (m - j) * sy;
            dm[0] = sd[i * CL_SD + m];
            dm[1] = sd[j * CL_SD + m];
            if constexpr (DIM == 3) {
                o[2] = base + (m - k) * sz;
                dm[2] = sd[k * CL_SD + m];
            }
#pragma unroll
            for (int b = 0; b < CW; ++b)
#pragma unroll
                for (int d = 0; d < DIM; ++d) h[b][d] += dm[d] * sx[b * SC + o[d]];
        }
        const int64_t tg = LIST ? (int64_t)elist[e0 + el] * nn + l : t0 + t;  // the (element, node) pair's own index
        const double *g = PE ? geo + tg * G1 : geo + l * G1;
        const double c = g[0];
        double Ji[DIM][DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d)
#pragma unroll
            for (int kk = 0; kk < DIM; ++kk) Ji[d][kk] = g[1 + d * DIM + kk];
        double H[CW][DIM];
#pragma unroll
        for (int b = 0; b < CW; ++b)
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                double acc = 0.0;
#pragma unroll
                for (int kk = 0; kk < DIM; ++kk) acc += Ji[d][kk] * h[b][kk];
                H[b][d] = acc;
            }
        double *out = ws + tg * RW;
#pragma unroll
        for (int a = 0; a < RW; ++a) {
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < CW; ++b)
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    constexpr double one = 1.0;
                    const double cf = colloc_coef<DIM, OP>(a, b, d);
                    if (cf == one) s += H[b][d];
                    else if (cf == -one) s -= H[b][d];
                    else if (cf != 0.0) s += cf * H[b][d];
                }
            out[a] = c * s;
        }
    }
}

template <int RW>
__global__ __launch_bounds__(256) void k_colloc_gather(int64_t N, int maxinc, const int32_t *__restrict__ inc,
                                                       const double *__restrict__ winv, const double *__restrict__ ws,
                                                       double *__restrict__ y, const int *__restrict__ istate)
{
    if (istate && istate[I_REASON] != 0) return;
    const int64_t node = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= N) return;
    double s[RW];
#pragma unroll
    for (int a = 0; a < RW; ++a) s[a] = 0.0;
    for (int j = 0; j < maxinc; ++j) {
        const int t = inc[node * maxinc + j];
        if (t < 0) break;
        const double *w = ws + (int64_t)t * RW;
#pragma unroll
        for (int a = 0; a < RW; ++a) s[a] += w[a];
    }
    const double wi = winv[node];
#pragma unroll
    for (int a = 0; a < RW; ++a) y[node * RW + a] = s[a] * wi;
}

template <int RW>
__global__ __launch_bounds__(256) void k_colloc_gather_csr(int64_t N, const int32_t *__restrict__ incp,
                                                           const int32_t *__restrict__ inc,
                                                           const double *__restrict__ winv,
                                                           const double *__restrict__ ws, double *__restrict__ y,
                                                           const int *__restrict__ istate)
{
    if (istate && istate[I_REASON] != 0) return;
    const int64_t node = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= N) return;
    double s[RW];
#pragma unroll
    for (int a = 0; a < RW; ++a) s[a] = 0.0;
    const int j1 = incp[node + 1];
    for (int j = incp[node]; j < j1; ++j) {
        const double *w = ws + (int64_t)inc[j] * RW;
#pragma unroll
        for (int a = 0; a < RW; ++a) s[a] += w[a];
    }
    const double wi = winv[node];
#pragma unroll
    for (int a = 0; a < RW; ++a) y[node * RW + a] = s[a] * wi;
}

// winv of the per-element geometry: k_ops_weights_u's sum over the CSR list
__global__ __launch_bounds__(256) void k_colloc_weights(int64_t N, int G1, const int32_t *__restrict__ incp,
                                                        const int32_t *__restrict__ inc,
                                                        const double *__restrict__ geo, double *__restrict__ winv)
{
    const int64_t node = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= N) return;
    double W = 0.0;
    const int j1 = incp[node + 1];
    for (int j = incp[node]; j < j1; ++j) W += geo[(int64_t)inc[j] * G1];
    winv[node] = 1.0 / W;
}

// the element kernel over elements [e0, e1) (x: the ghosted allocation), or with e0 < 0 the gather
template <int DIM, int OP>
static void launch_colloc(const CollocOp *P, hipStream_t st, int64_t e0, int64_t e1, const double *x, double *y,
                          const int *istate)
{
    if (P->per_elem) {  // every element (several ranks: positions [e0, e1) of the element lists), then the CSR gather
        if (e0 >= 0) {
            const unsigned ge = (unsigned)((e1 - e0 + P->neb - 1) / P->neb);
            if (P->d_elist)
                hipLaunchKernelGGL((k_colloc_elem<DIM, OP, true, true>), dim3(ge), dim3(256), 0, st, P->ngl, P->nn,
                                   P->neb, P->sy, P->sz, P->se, e0, e1, P->d_dh, P->d_geo, P->d_conn, x, P->d_ws, istate,
                                   P->d_elist);
            else
                hipLaunchKernelGGL((k_colloc_elem<DIM, OP, true>), dim3(ge), dim3(256), 0, st, P->ngl, P->nn, P->neb,
                                   P->sy, P->sz, P->se, e0, e1, P->d_dh, P->d_geo, P->d_conn, x, P->d_ws, istate,
                                   nullptr);
            return;
        }
        const unsigned gn = (unsigned)((P->N + 255) / 256);
        hipLaunchKernelGGL((k_colloc_gather_csr<colloc_rw(DIM, OP)>), dim3(gn), dim3(256), 0, st, P->N, P->d_incp,
                           P->d_inc, P->d_winv, P->d_ws, y, istate);
        return;
    }
    if (e0 >= 0) {
        const unsigned ge = (unsigned)((e1 - e0 + P->neb - 1) / P->neb);
        hipLaunchKernelGGL((k_colloc_elem<DIM, OP>), dim3(ge), dim3(256), 0, st, P->ngl, P->nn, P->neb, P->sy, P->sz,
                           P->se, e0, e1, P->d_dh, P->d_geo, P->d_conn, x, P->d_ws, istate, nullptr);
        return;
    }
    const unsigned gn = (unsigned)((P->N + 255) / 256);
    hipLaunchKernelGGL((k_colloc_gather<colloc_rw(DIM, OP)>), dim3(gn), dim3(256), 0, st, P->N, P->maxinc, P->d_inc,
                       P->d_winv, P->d_ws, y, istate);
}

int colloc_spmv(kle_mat *A, const kle_vec *x, kle_vec *y, const int *istate, bool local)
{
    const CollocOp *P = A->colloc;
    if (!P) return fail(KLE_ERR_STATE, "collocation operator without tables");
    KLE_TRY(elem_check_vecs(A, x, y, "collocation operator"));
    hipStream_t st = A->ctx->stream;
    auto launch = [&](int64_t e0, int64_t e1) -> int {
        switch (P->dim * 3 + P->which) {
        case 6: launch_colloc<2, 0>(P, st, e0, e1, x->base, y->d, istate); break;
        case 7: launch_colloc<2, 1>(P, st, e0, e1, x->base, y->d, istate); break;
        case 8: launch_colloc<2, 2>(P, st, e0, e1, x->base, y->d, istate); break;
        case 9: launch_colloc<3, 0>(P, st, e0, e1, x->base, y->d, istate); break;
        case 10: launch_colloc<3, 1>(P, st, e0, e1, x->base, y->d, istate); break;
        case 11: launch_colloc<3, 2>(P, st, e0, e1, x->base, y->d, istate); break;
        default: return fail(KLE_ERR_STATE, "collocation operator: bad tables");
        }
        KLE_HIP(hipGetLastError());
        return 0;
    };
    if (P->per_elem) {
        if (!P->d_elist) KLE_TRY(launch(0, P->E));
        else KLE_TRY(elem_ranges(A, x, local, [&](int64_t l0, int64_t l1, bool) -> int { return launch(l0, l1); }));
        return launch(-1, -1);
    }
    // (the ghost layer whole: a workgroup takes whole elements)
    KLE_TRY(elem_ranges(A, x, local, [&](int64_t e0, int64_t e1, bool) -> int { return launch(e0, e1); }));
    return launch(-1, -1);
}

void colloc_drop(kle_mat *A)
{
    CollocOp *P = A->colloc;
    if (!P) return;
    (void)hipFree(P->d_dh);
    if (!P->per_elem) (void)hipFree(P->d_geo);  // (else the mesh's set: it goes with its last holder)
    (void)hipFree(P->d_incp);
    (void)hipFree(P->d_elist);
    (void)hipFree(P->d_winv);
    (void)hipFree(P->d_ws);
    (void)hipFree(P->d_conn);
    (void)hipFree(P->d_inc);
    delete P;
    A->colloc = nullptr;
}

// Algorithmic bytes of one product.  k_colloc_elem: the connectivity (4 E nn),
// x read once (8 n), the derivative table and the first element's geometry,
// the element results written (8 E nn RW).  k_colloc_gather: the incidence
// table (4 N maxinc), the element results read, winv (8 N), y written (8 m).
double colloc_spmv_bytes(const kle_mat *A)
{
    const CollocOp *P = A->colloc;
    if (!P) return 0.0;
    if (P->per_elem)  // every element's geometry, the CSR list instead of the padded table
        // (several ranks: the local E, the ext range of x, the owned N and the element lists)
        return 4.0 * P->E * P->nn + 8.0 * (A->n_local + A->ghost_lo + A->ghost_hi) + 8.0 * P->ngl * P->ngl +
               8.0 * P->E * P->nn * (1 + P->dim * P->dim) + 2.0 * 8.0 * P->E * P->nn * P->rw + 4.0 * (P->N + 1) +
               4.0 * P->ninc + 8.0 * P->N + 8.0 * A->m_local + (P->d_elist ? 4.0 * P->E : 0.0);
    return 4.0 * P->E * P->nn + 8.0 * (A->n_local + A->ghost_lo + A->ghost_hi) + 8.0 * P->ngl * P->ngl + 8.0 * P->nn * (1 + P->dim * P->dim) +
           2.0 * 8.0 * P->E * P->nn * P->rw + 4.0 * P->N * P->maxinc + 8.0 * P->N + 8.0 * A->m_local;
}

std::string colloc_kernel_name(const kle_mat *A)
{
    const CollocOp *P = A->colloc;
    if (!P) return "?";
    const char *ops[3] = {"Curl", "SrT", "DivSrT"};
    if (P->per_elem)
        return "k_colloc_elem<" + std::to_string(P->dim) + "," + ops[P->which] + ",geo>+k_colloc_gather_csr<" +
               std::to_string(P->rw) + ">";
    return "k_colloc_elem<" + std::to_string(P->dim) + "," + ops[P->which] + ">+k_colloc_gather<" +
           std::to_string(P->rw) + ">";
}

// The dense M_e0 the factored tables stand for, against the element matrix the
// assembly path forms for element 0 (k_ops_element): exactly 0 off the grid
// lines, equal to a few ulps on them.
template <int DIM, int OP>
static int colloc_check(int ngl, int nn, const std::vector<double> &geo, const std::vector<double> &dh,
                        const std::vector<double> &dense)
{
    constexpr int CW = colloc_cw(DIM, OP), RW = colloc_rw(DIM, OP), G1 = 1 + DIM * DIM;
    const double eps = 2.220446049250313e-16;
    if (dense.size() != (size_t)RW * nn * CW * nn) return fail(KLE_ERR_STATE, "collocation operator: element matrix size");
    for (int l = 0; l < nn; ++l) {
        const int oi[3] = {l % ngl, (l / ngl) % ngl, DIM == 3 ? l / (ngl * ngl) : 0};
        const double *g = &geo[(size_t)l * G1];
        for (int m = 0; m < nn; ++m) {
            const int oj[3] = {m % ngl, (m / ngl) % ngl, DIM == 3 ? m / (ngl * ngl) : 0};
            int differ = 0;
            for (int d = 0; d < DIM; ++d) differ += oj[d] != oi[d];
            // the factored form: the 1-D derivative along each line through l that holds m
            double hl[DIM];
            for (int kk = 0; kk < DIM; ++kk) {
                bool on = true;
                for (int j = 0; j < DIM; ++j)
                    if (j != kk) on = on && oj[j] == oi[j];
                hl[kk] = on ? dh[(size_t)oi[kk] * ngl + oj[kk]] : 0.0;
            }
            double H[DIM], Habs[DIM];
            for (int d = 0; d < DIM; ++d) {
                double acc = 0.0, aab = 0.0;
                for (int kk = 0; kk < DIM; ++kk) {
                    acc += g[1 + d * DIM + kk] * hl[kk];
                    aab += std::fabs(g[1 + d * DIM + kk] * hl[kk]);
                }
                H[d] = acc;
                Habs[d] = aab;
            }
            for (int a = 0; a < RW; ++a)
                for (int b = 0; b < CW; ++b) {
                    const double have = dense[((size_t)l * RW + a) * nn * CW + (size_t)m * CW + b];
                    if (differ > 1) {
                        if (have != 0.0)
                            return fail(KLE_ERR_STATE,
                                        "collocation operator: element entry (%d,%d)x(%d,%d) off the grid lines is %g, "
                                        "not 0", l, a, m, b, have);
                        continue;
                    }
                    double want = 0.0, scale = 0.0;
                    for (int d = 0; d < DIM; ++d) {
                        want += colloc_coef<DIM, OP>(a, b, d) * H[d];
                        scale += std::fabs(colloc_coef<DIM, OP>(a, b, d)) * Habs[d];
                    }
                    want *= g[0];
                    scale *= std::fabs(g[0]);
                    if (!(std::fabs(have - want) <= 8.0 * eps * scale))
                        return fail(KLE_ERR_STATE,
                                    "collocation operator: element entry (%d,%d)x(%d,%d) is %.17g, the factored tables "
                                    "give %.17g", l, a, m, b, have, want);
                }
        }
    }
    return 0;
}

}  // namespace kle

using namespace kle;

extern "C" int kle_mat_create_operator_element(kle_ctx *ctx, kle_mesh *m, int which, kle_mat **out)
{
    KLE_ARG(ctx && m && out, "null arg");
    KLE_ARG(which >= 0 && which <= 2, "which must be 0 (Curl), 1 (SrT) or 2 (DivSrT)");
    if (m->kind != 0)
        return fail(KLE_ERR_SUP, "element-wise operator: needs a uniform box mesh (unstructured mesh given)");
    const int dim = m->dim, ngl = m->ngl, nn = m->nn(), maxinc = 1 << dim, G1 = 1 + dim * dim;
    KLE_ARG((dim == 2 || dim == 3) && ngl >= 2 && ngl <= 8, "element-wise operator: dim 2 or 3, ngl 2..8");
    const int rw = colloc_rw(dim, which), cw = colloc_cw(dim, which);
    ElemLayout L;
    KLE_TRY(elem_layout(ctx, m, std::max(rw, cw), &L));
    const int64_t E = L.E, N = L.N;

    // tables (host) in ext-local node ids, validated before upload
    std::vector<int32_t> conn, inc;
    KLE_TRY(elem_tables(m, L, conn, inc));

    // LDS layout: odd strides (in doubles) of the y lines, z planes and elements
    // (a workgroup's only element needs no element stride)
    const int neb = std::max(1, 256 / nn);
    const int sy = ngl | 1, sz = dim == 3 ? (ngl * sy) | 1 : 0, se = ngl * (dim == 3 ? sz : sy) | (neb > 1 ? 1 : 0);
    if ((int64_t)neb * se > (dim == 3 ? CL_SC3 : CL_SC2))
        return fail(KLE_ERR_STATE, "collocation operator: %d elements of stride %d exceed the LDS tile", neb, se);

    KLE_HIP(hipSetDevice(ctx->device));
    // c_l, inv J and D through the assembly's own geometry path on the corners
    // of global element 0, and the element matrix it forms there
    kle_mesh m0;
    first_element_mesh(m, &m0);
    std::vector<double> geo, dh, dense;
    KLE_TRY(element_ops(ctx, &m0, 0, geo, dh, which == 0 ? &dense : nullptr, which == 1 ? &dense : nullptr,
                        which == 2 ? &dense : nullptr));
    if ((int)geo.size() != nn * G1 || (int)dh.size() != ngl * ngl)
        return fail(KLE_ERR_STATE, "collocation operator: geometry tables do not match the element");
    for (double v : geo)
        if (!std::isfinite(v)) return fail(KLE_ERR_STATE, "collocation operator: the element geometry is not finite");
    int rc = 0;
    switch (dim * 3 + which) {
    case 6: rc = colloc_check<2, 0>(ngl, nn, geo, dh, dense); break;
    case 7: rc = colloc_check<2, 1>(ngl, nn, geo, dh, dense); break;
    case 8: rc = colloc_check<2, 2>(ngl, nn, geo, dh, dense); break;
    case 9: rc = colloc_check<3, 0>(ngl, nn, geo, dh, dense); break;
    case 10: rc = colloc_check<3, 1>(ngl, nn, geo, dh, dense); break;
    default: rc = colloc_check<3, 2>(ngl, nn, geo, dh, dense); break;
    }
    if (rc) return rc;
    // winv = 1 / sum of the incident c_0[l], in incidence order
    std::vector<double> winv((size_t)N);
    for (int64_t g = 0; g < N; ++g) {
        double W = 0.0;
        for (int j = 0; j < maxinc; ++j) {
            const int32_t t = inc[g * maxinc + j];
            if (t < 0) break;
            W += geo[(size_t)(t % nn) * G1];
        }
        winv[g] = 1.0 / W;
        if (!std::isfinite(winv[g]))
            return fail(KLE_ERR_STATE, "collocation operator: node %lld has no finite nodal weight", (long long)g);
    }

    kle_mat *A = new kle_mat;
    CollocOp *P = new CollocOp;
    A->ctx = ctx;
    A->colloc = P;
    elem_mat_fields(A, m, L, rw, cw);
    P->which = which;
    P->dim = dim;
    P->cw = cw;
    P->rw = rw;
    P->ngl = ngl;
    P->nn = nn;
    P->maxinc = maxinc;
    P->neb = neb;
    P->sy = sy;
    P->sz = sz;
    P->se = se;
    P->E = E;
    P->N = N;
    auto up = [&](auto **dp, const void *src, size_t bytes) {
        if (hipMalloc(dp, bytes) != hipSuccess) {
            (void)hipGetLastError();
            *dp = nullptr;
            return fail(KLE_ERR_MEM, "out of device memory for the element-wise operator");
        }
        return src ? h2d(*dp, src, bytes) : 0;
    };
    rc = up(&P->d_dh, dh.data(), sizeof(double) * dh.size());
    if (!rc) rc = up(&P->d_geo, geo.data(), sizeof(double) * geo.size());
    if (!rc) rc = up(&P->d_winv, winv.data(), sizeof(double) * winv.size());
    if (!rc) rc = up(&P->d_conn, conn.data(), sizeof(int32_t) * conn.size());
    if (!rc) rc = up(&P->d_inc, inc.data(), sizeof(int32_t) * inc.size());
    if (!rc) rc = up(&P->d_ws, nullptr, sizeof(double) * (size_t)E * nn * rw);
    if (rc) {
        kle_mat_destroy(A);
        return rc;
    }
    *out = A;
    return 0;
}

// The same operators with every element's own geometry: any mesh, on one rank
// or on the parts of a partition (tables, element lists and halo as kle_sumfac.hip;
// winv over the owned nodes, whose incident elements are all local).
extern "C" int kle_mat_create_operator_sumfac(kle_ctx *ctx, kle_mesh *m, int which, kle_mat **out)
{
    KLE_ARG(ctx && m && out, "null arg");
    KLE_ARG(which >= 0 && which <= 2, "which must be 0 (Curl), 1 (SrT) or 2 (DivSrT)");
    const int dim = m->dim, ngl = m->ngl, nn = m->nn(), G1 = 1 + dim * dim;
    KLE_ARG((dim == 2 || dim == 3) && ngl >= 2 && ngl <= 8, "sum-factorised operator: dim 2 or 3, ngl 2..8");
    const int rw = colloc_rw(dim, which), cw = colloc_cw(dim, which);

    // connectivity in ext-local ids, the owned nodes' CSR incidence list and (several
    // ranks) the element lists (host), validated before upload
    ElemLayout L;
    std::vector<int32_t> conn, incp, inc, elist;
    KLE_TRY(sumfac_tables(ctx, m, std::max(rw, cw), &L, conn, incp, inc, elist));
    const int64_t E = L.E, N = L.N;
    for (int64_t i = 0; i < N; ++i)
        if (incp[i + 1] == incp[i])
            return fail(KLE_ERR_STATE, "sum-factorised operator: node %lld lies in no element", (long long)i);

    const int neb = std::max(1, 256 / nn);
    const int sy = ngl | 1, sz = dim == 3 ? (ngl * sy) | 1 : 0, se = ngl * (dim == 3 ? sz : sy) | (neb > 1 ? 1 : 0);
    if ((int64_t)neb * se > (dim == 3 ? CL_SC3 : CL_SC2))
        return fail(KLE_ERR_STATE, "collocation operator: %d elements of stride %d exceed the LDS tile", neb, se);

    // the derivative table at the operator points: the assembly's (T.O.dh)
    PointSet1D full, red, op;
    element_sets(ngl, full, red, op);
    if ((int)op.x.size() != ngl || (int)op.dh.size() != ngl * ngl)
        return fail(KLE_ERR_STATE, "operator points are not the element's nodes");

    KLE_HIP(hipSetDevice(ctx->device));
    kle_mat *A = new kle_mat;
    CollocOp *P = new CollocOp;
    A->ctx = ctx;
    A->colloc = P;
    elem_mat_fields(A, m, L, rw, cw);
    P->which = which;
    P->dim = dim;
    P->cw = cw;
    P->rw = rw;
    P->ngl = ngl;
    P->nn = nn;
    P->maxinc = 0;
    P->neb = neb;
    P->sy = sy;
    P->sz = sz;
    P->se = se;
    P->E = E;
    P->N = N;
    P->per_elem = true;
    P->ninc = (int64_t)inc.size();
    // (a graph partition: the column space's halo goes through the mesh's plan)
    A->plan = m->plan;
    A->ext_gid = m->ext_gid;
    auto up = [&](auto **dp, const void *src, size_t bytes) {
        if (hipMalloc(dp, bytes) != hipSuccess) {
            (void)hipGetLastError();
            *dp = nullptr;
            return fail(KLE_ERR_MEM, "out of device memory for the sum-factorised operator");
        }
        return src ? h2d(*dp, src, bytes) : 0;
    };
    int rc = mesh_geometry(ctx, m, false, true, &P->geo);
    if (!rc && P->geo->npO != ngl) rc = fail(KLE_ERR_STATE, "sum-factorised operator: the nodal geometry does not match the element");
    if (!rc) P->d_geo = P->geo->O;
    if (!rc) rc = up(&P->d_dh, op.dh.data(), sizeof(double) * op.dh.size());
    if (!rc) rc = up(&P->d_conn, conn.data(), sizeof(int32_t) * conn.size());
    if (!rc) rc = up(&P->d_incp, incp.data(), sizeof(int32_t) * incp.size());
    if (!rc) rc = up(&P->d_inc, inc.data(), sizeof(int32_t) * inc.size());
    if (!rc && !elist.empty()) rc = up(&P->d_elist, elist.data(), sizeof(int32_t) * elist.size());
    if (!rc) rc = up(&P->d_winv, nullptr, sizeof(double) * (size_t)N);
    if (!rc) rc = up(&P->d_ws, nullptr, sizeof(double) * (size_t)E * nn * rw);
    if (!rc) {
        hipStream_t st = ctx->stream;
        hipLaunchKernelGGL(k_colloc_weights, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, N, G1, P->d_incp,
                           P->d_inc, P->d_geo, P->d_winv);
        hipError_t he = hipGetLastError();
        std::vector<double> winv((size_t)N);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he == hipSuccess) he = hipMemcpy(winv.data(), P->d_winv, sizeof(double) * winv.size(), hipMemcpyDeviceToHost);
        if (he != hipSuccess) rc = fail(KLE_ERR_DEVICE, "sum-factorised operator: weights: %s", hipGetErrorString(he));
        for (int64_t g = 0; g < N && !rc; ++g)
            if (!std::isfinite(winv[g]))
                rc = fail(KLE_ERR_STATE, "sum-factorised operator: node %lld has no finite nodal weight", (long long)g);
    }
    if (rc) {
        kle_mat_destroy(A);
        return rc;
    }
    *out = A;
    return 0;
}
