// kle_sumfac.hip -- sum-factorised element-wise K, Krhs and Rw on any mesh, box
// or unstructured, on one rank or on the parts of a partition (kle_mat kind 2
// with sumfac set): no assembled values and no element matrix.
//
// On distorted hexes the element matrices differ, so the one K_e0 of
// kle_elem.hip is gone; the factored form of the assembly (kle_assemble.hip
// store_elem_blocks) applied to a vector is a quadrature-point evaluation with
// per-point geometry.  With (grad u)_ab = d_b u^a at the point:
//
//     (K_e u)_l^a =  sum_{q in full} c_q sum_b d_b N_l(q) (grad u)_ab(q)
//                  + sum_{q in red}  c_q sum_b d_b N_l(q) T_ab(q)
//     T = a_d (div u) I + a_w (grad u - grad u^T)
//
// and the tensor structure of N turns both sums into 1-D passes with the h / dh
// tables of kle_basis (full: GLL(ngl) for ngl > 3, else Gauss(ngl); reduced:
// Gauss(ngl - 1)).
//
//   k_sumfac_elem<DIM>    a 256-thread workgroup takes a batch of whole
//       elements (as many as fit 256 threads, at least one) and gathers their
//       x entries through the connectivity into LDS, component-major tiles
//       [element][k][j][i] with the odd line, plane and element strides of
//       kle_colloc.hip.  The mask is folded into the connectivity as -1 (K: the
//       Dirichlet columns, Krhs: the free ones): such an entry is 0 and x is
//       never read there.  The four 1-D tables sit in LDS (row stride 9).  One
//       thread per (element, lattice site), looping where an element has more
//       than 256 sites (ngl 7, 8 in 3-D); a site is a node or, along the
//       directions already contracted, a point (sites beyond the rule's points
//       idle).  Per rule, full first:
//         forward, per component: x pass (h u, dh u), y pass, z pass -> the
//           reference gradient of the component at the thread's point, m
//           ascending in every line sum;
//         point: grad u = sum_k invJ[b][k] g_ref[a][k] (as fill_chunk), the
//           flux c grad u (full) or c T (reduced), back with invJ^T;
//         transposed, per component: z, y, x passes with the tables read
//           transposed, q ascending; the x pass leaves the node's sum.
//       The reduced rule's sum is added to the full rule's; ws[e][l][a] takes
//       it, negated for Krhs.
//   k_sumfac_gather<DIM>  one thread per owned DoF: the sum of its node's
//       incidence entries of ws, a CSR list (inc_ptr, inc_idx = e nn + l,
//       ascending e -- a Gmsh node lies in any number of elements).  Dirichlet
//       rows: y_i = x_i.
//   k_sumfac_diag<DIM>    once at creation: the element diagonal
//         sum_full c |grad N_l|^2 + sum_red c [a_d (d_a N_l)^2 + a_w (|grad N_l|^2 - (d_a N_l)^2)]
//       per (element, node), gathered like the product; 1 on Dirichlet rows, 0
//       on the free rows of Krhs.
//
//   k_sumfac_rw<DIM>      Rw applied to a vorticity vector w (dim_w = 3
//       components in 3-D, 1 in 2-D), the same batching, tiles, tables and
//       geometry as k_sumfac_elem:
//         (Rw_e w)_l^a =  sum_{q in full} c_q N_l(q) (curl w)_a(q)
//                       + a_w sum_{q in red} c_q sum_b d_b N_l(q) eps_{acb} w_c(q)
//       (2-D: y_0 = sum c N_l d_y w - a_w sum c d_y N_l w, y_1 the same in x
//       with the signs turned).  Full rule: the forward passes of
//       k_sumfac_elem per component of w, inv J, c curl w, then value passes
//       back (h transposed, no derivative table).  Reduced rule: forward value
//       passes only, the flux c (a_w w_c) placed by eps, back with inv J^T and
//       the transposed derivative passes of k_sumfac_elem.  No entry of w is
//       dropped; ws[e][l][a] takes the sum.
//   k_sumfac_gather_rw<DIM>  as k_sumfac_gather, but a Dirichlet row is +0.0
//       and reads nothing (the assembled Rw has no entry there).
//
// c_q and inv J come from two tables [e][q][1 + dim^2], one per rule, that the
// assembly's k_geometry fills from the mesh's own corners: the numbers the
// assembled matrix was formed from; K, Krhs and Rw of one mesh share them
// (mesh_geometry).  No atomics, fixed order: the same input
// gives the same bits.  Both product kernels do nothing once the Krylov reason
// word is set.
//
// Several ranks (box slabs; Gmsh slab and inertial partitions): a rank's local
// elements are every cell touching an owned node, ascending global cell id;
// conn holds ext-local node ids over all of them, masked by the Dirichlet flags
// of the ext range (a ghost Dirichlet column is dropped like an owned one); x
// is read through the vector's ghosted allocation after one forward halo (the
// vector's plan on a graph partition); the incidence list, the gather and the
// diagonal cover the owned nodes, whose incident elements are all local.  The
// elements reading owned nodes alone are not contiguous in that order, so the
// element kernels take an element list (LIST): inner, run on the compute
// stream beside the halo on the comm stream, and outer, run after it
// (elem_ranges over list positions: el_ghost 0, el_int1 the inner list's length).  ws, the geometry tables and conn stay indexed by the element's
// own id, so the gather sums a node's entries in the one-rank order: the owned
// rows are the one-rank product's bit for bit.
//
// No-slip meshes (kle_mat_create_ns_sumfac): the seven matrices of
// MatNS.buildNS are the same sums with masks per velocity DoF -- classes F / T
// / N from the mesh's dof_cls -- each at most two passes of (column classes
// kept -> row classes taking the sum) and a fixed rule on every other row
// (NS_SPECS, kle_internal.hpp; the table of kle_elem.hip):
//
//   k_sumfac_elem<DIM, LIST, CLS = true>  the same kernel with conn unmasked
//       and a class table [E][nn], one byte per element node holding the dim
//       classes of its DoFs at 2 bits each (ext-indexed, ghosts included);
//       the pass's 3-bit set of kept classes is a launch argument and
//       component b of a site loads x iff it holds the DoF's class.  Kfs runs
//       two passes into two result arrays; Rw and Rwfs keep every column and
//       run k_sumfac_rw unchanged.  The CLS = false instantiations are the
//       free-slip kernels, instruction for instruction.
//   k_sumfac_gather_cls  one thread per owned DoF; the rule byte of its class
//       says zero (+0.0, nothing read), identity (x_i bit for bit), the sum
//       from pass 0 or from pass 1 over the CSR incidence list (ascending
//       element, no atomics) and whether -x_i is added (Kfs's T rows).
//   k_sumfac_diag_gather_cls  the diagonal by class, once at creation, from
//       k_sumfac_diag's element entries.
//
// On several ranks both passes of Kfs run per element list, so they share the
// product's one halo.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "kle_basis.hpp"
#include "kle_internal.hpp"

namespace kle {

constexpr int SF_SD = 9;      // row stride of a 1-D table in LDS (odd, >= 8)
constexpr int SF_ST = 8 * SF_SD;  // doubles per table in LDS
constexpr int SF_SC3 = 584;   // doubles per tile, 3-D: one ngl 8 element, strides 9 / 73 / 584
constexpr int SF_SC2 = 448;   // 2-D: 64 ngl 2 elements, strides 3 / 7
constexpr double SF_ALPHA_W = 1e2, SF_ALPHA_D = 1e3;  // kle_assemble.hip ALPHA_W, ALPHA_D (spectral.py:96-97)

struct SumfacOp {
    int which = 0, dim = 3, ngl = 0, nn = 0, negate = 0;
    int neb = 1, sy = 0, sz = 0, se = 0;  // elements per workgroup; LDS line, plane and element strides
    int npF = 0, npR = 0;       // 1-D points of the full and the reduced rule
    int64_t E = 0, N = 0, ninc = 0;
    double *d_tab = nullptr;    // [4][8][8] h, dh of the full rule, h, dh of the reduced rule: [q][a], row length ngl
    std::shared_ptr<GeoSet> geo;  // the mesh's geometry set: owns the two tables below
    double *d_geoF = nullptr;   // [E][npF^dim][1 + dim^2] c_q, inv J
    double *d_geoR = nullptr;   // [E][npR^dim][1 + dim^2]
    double *d_ws = nullptr;     // [E][nn][dim] element results
    double *d_diag = nullptr;   // [N dim] the diagonal, formed at creation (Rw: none)
    int32_t *d_conn = nullptr;  // [E][nn] element -> node, tensor order; -1 where the operator drops the entry
    int32_t *d_incp = nullptr;  // [N + 1] node -> its entries of d_inc
    int32_t *d_inc = nullptr;   // [E nn] e * nn + l, ascending e per node
    uint8_t *d_dir = nullptr;   // [N] Dirichlet flag
    // several ranks: the local elements as two lists, [0, n_inner) those reading
    // owned nodes alone, [n_inner, E) those reading a ghost; each ascending
    int32_t *d_elist = nullptr;  // [E] (one rank: none, the kernels take every element in order)
    // no-slip operators (kle_mat_create_ns_sumfac): masks per velocity DoF.  which
    // stays the kernel family (0: k_sumfac_elem, 2: k_sumfac_rw), ns_which the operator
    int ns = 0, ns_which = 0;   // ns 1: rows by DoF class (k_sumfac_gather_cls); ns_which 0 .. 6 (NS_SPECS)
    int npass = 1;              // element passes (Kfs: 2), pass p keeps the classes keep[p], into d_wsp[p]
    unsigned keep[2] = {0, 0};
    unsigned rules = 0, drules = 0;  // row rule and diagonal of class c in byte c (ns_rule_words)
    uint8_t *d_ncls = nullptr;  // [E][nn] the dim classes of an element node, 2 bits each (K-family operators)
    uint8_t *d_cls = nullptr;   // [N dim] class of the owned DoFs
    double *d_wsp[2] = {nullptr, nullptr};  // [E][nn][dim] per pass (d_wsp[0] == d_ws)
};

// LIST: the batch's elements are elist[e0 .. e0 + neb) of the E listed (several
// ranks: the inner or the outer list); conn, geo and ws stay indexed by the
// element's own id, the LDS tile by its place in the batch
//
// CLS (the no-slip operators): the mask acts per velocity
// DoF, so conn stays unmasked and ncls [E][nn] holds the dim classes of every
// element node at 2 bits each; component b of a site loads x iff keep, the
// pass's 3-bit set of kept classes, holds its class.
template <int DIM, bool LIST = false, bool CLS = false>
__global__ __launch_bounds__(256) void k_sumfac_elem(int ngl, int nn, int neb, int sy, int sz, int se, int64_t E,
                                                     int negate, const double *__restrict__ tab,
                                                     const double *__restrict__ geoF, const double *__restrict__ geoR,
                                                     const int32_t *__restrict__ conn, const double *__restrict__ x,
                                                     double *__restrict__ ws, const int *__restrict__ istate,
                                                     const int32_t *__restrict__ elist,
                                                     const uint8_t *__restrict__ ncls, unsigned keep)
{
    if (istate && istate[I_REASON] != 0) return;
    constexpr int NIT = DIM == 3 ? 2 : 1;  // sites per thread: 512 at ngl 8 in 3-D
    constexpr int G1 = 1 + DIM * DIM, SC = DIM == 3 ? SF_SC3 : SF_SC2;
    __shared__ double sx[DIM * SC];                 // x, per component
    __shared__ double sA[2 * SC];                   // after the x pass: (h u, dh u); before the transposed x pass
    __shared__ double sB[DIM * SC];                 // after the y pass (3-D); the point fluxes
    __shared__ double sC[DIM == 3 ? 3 * SC : 1];    // after the transposed z pass (3-D)
    __shared__ double sd[4 * SF_ST];
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * neb;
    const int nt = (int)min((int64_t)neb, E - e0) * nn;  // (element, site) pairs of this batch
    const int64_t t0 = e0 * nn;
    {
        const int n2 = ngl * ngl;
        for (int t = tid; t < 4 * n2; t += 256) {
            const int tb = t / n2, r = t - tb * n2;
            sd[tb * SF_ST + (r / ngl) * SF_SD + r % ngl] = tab[tb * 64 + r];
        }
    }
    bool ok[NIT];
    int base[NIT], si[NIT], sj[NIT], sk[NIT], sel[NIT];
    int64_t eid[NIT];  // the element's own id
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int t = tid + it * 256;
        ok[it] = t < nt;
        const int el = t / nn, l = t - el * nn;
        eid[it] = LIST && ok[it] ? elist[e0 + el] : 0;
        const int r = l / ngl;
        si[it] = l % ngl;
        sj[it] = DIM == 3 ? r % ngl : r;
        sk[it] = DIM == 3 ? r / ngl : 0;
        sel[it] = el;
        base[it] = el * se + sk[it] * sz + sj[it] * sy + si[it];
        if (ok[it]) {
            const int node = conn[LIST ? eid[it] * nn + l : t0 + t];
            unsigned cb = 0;
            if constexpr (CLS) cb = ncls[LIST ? eid[it] * nn + l : t0 + t];
#pragma unroll
            for (int b = 0; b < DIM; ++b) {
                double v = 0.0;
                if constexpr (CLS) {
                    if ((keep >> ((cb >> (2 * b)) & 3u)) & 1u) v = x[(int64_t)node * DIM + b];
                } else {
                    if (node >= 0) v = x[(int64_t)node * DIM + b];  // (a dropped entry is never read)
                }
                sx[b * SC + base[it]] = v;
            }
        }
    }
    double res[NIT][DIM];
    double g[NIT][DIM][DIM];  // [component][reference direction]: the gradient, then the flux
    for (int rule = 0; rule < 2; ++rule) {
        const int P = rule ? ngl - 1 : ngl;
        const double *th = sd + rule * 2 * SF_ST, *tdh = th + SF_ST;
        const double *geo = rule ? geoR : geoF;
        const int nq = DIM == 3 ? P * P * P : P * P;
        __syncthreads();  // x and the tables; the last rule's reads of sA
        // ---- forward: reference gradient of every component at the points
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (!(ok[it] && si[it] < P)) continue;
                const int i = si[it], o = a * SC + base[it] - i;
                double ah = 0.0, ad = 0.0;
                for (int m = 0; m < ngl; ++m) {
                    const double v = sx[o + m];
                    ah += th[i * SF_SD + m] * v;
                    ad += tdh[i * SF_SD + m] * v;
                }
                sA[base[it]] = ah;
                sA[SC + base[it]] = ad;
            }
            __syncthreads();
            if constexpr (DIM == 2) {
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    if (!(ok[it] && si[it] < P && sj[it] < P)) continue;
                    const int j = sj[it], o = base[it] - j * sy;
                    double g0 = 0.0, g1 = 0.0;
                    for (int m = 0; m < ngl; ++m) {
                        g0 += th[j * SF_SD + m] * sA[SC + o + m * sy];
                        g1 += tdh[j * SF_SD + m] * sA[o + m * sy];
                    }
                    g[it][a][0] = g0;
                    g[it][a][1] = g1;
                }
                __syncthreads();  // the next component's x pass rewrites sA
            } else {
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    if (!(ok[it] && si[it] < P && sj[it] < P)) continue;
                    const int j = sj[it], o = base[it] - j * sy;
                    double b0 = 0.0, b1 = 0.0, b2 = 0.0;
                    for (int m = 0; m < ngl; ++m) {
                        const double ah = sA[o + m * sy], ad = sA[SC + o + m * sy];
                        const double hj = th[j * SF_SD + m], dj = tdh[j * SF_SD + m];
                        b0 += hj * ad;
                        b1 += dj * ah;
                        b2 += hj * ah;
                    }
                    sB[base[it]] = b0;
                    sB[SC + base[it]] = b1;
                    sB[2 * SC + base[it]] = b2;
                }
                __syncthreads();
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    if (!(ok[it] && si[it] < P && sj[it] < P && sk[it] < P)) continue;
                    const int k = sk[it], o = base[it] - k * sz;
                    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
                    for (int m = 0; m < ngl; ++m) {
                        const double hk = th[k * SF_SD + m], dk = tdh[k * SF_SD + m];
                        g0 += hk * sB[o + m * sz];
                        g1 += hk * sB[SC + o + m * sz];
                        g2 += dk * sB[2 * SC + o + m * sz];
                    }
                    g[it][a][0] = g0;
                    g[it][a][1] = g1;
                    g[it][a][2] = g2;
                }
            }
        }
        // ---- the point: physical gradient, flux, back to reference directions
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (!(ok[it] && si[it] < P && sj[it] < P && sk[it] < P)) continue;
            const int q = (sk[it] * P + sj[it]) * P + si[it];
            const double *gp = geo + ((LIST ? eid[it] : e0 + sel[it]) * nq + q) * G1;
            const double c = gp[0];
            double Ji[DIM][DIM];
#pragma unroll
            for (int b = 0; b < DIM; ++b)
#pragma unroll
                for (int k = 0; k < DIM; ++k) Ji[b][k] = gp[1 + b * DIM + k];
            double G[DIM][DIM], F[DIM][DIM];
#pragma unroll
            for (int a = 0; a < DIM; ++a)
#pragma unroll
                for (int b = 0; b < DIM; ++b) {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < DIM; ++k) s += Ji[b][k] * g[it][a][k];
                    G[a][b] = s;
                }
            if (rule == 0) {
#pragma unroll
                for (int a = 0; a < DIM; ++a)
#pragma unroll
                    for (int b = 0; b < DIM; ++b) F[a][b] = c * G[a][b];
            } else {
                double div = G[0][0];
#pragma unroll
                for (int a = 1; a < DIM; ++a) div += G[a][a];
                const double cd = c * (SF_ALPHA_D * div);
#pragma unroll
                for (int a = 0; a < DIM; ++a)
#pragma unroll
                    for (int b = 0; b < DIM; ++b) F[a][b] = a == b ? cd : c * (SF_ALPHA_W * (G[a][b] - G[b][a]));
            }
#pragma unroll
            for (int a = 0; a < DIM; ++a)
#pragma unroll
                for (int k = 0; k < DIM; ++k) {
                    double s = 0.0;
#pragma unroll
                    for (int b = 0; b < DIM; ++b) s += Ji[b][k] * F[a][b];
                    g[it][a][k] = s;
                }
        }
        __syncthreads();  // the last component's reads of sB (3-D)
        // ---- transposed passes, per component
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (!(ok[it] && si[it] < P && sj[it] < P && sk[it] < P)) continue;
#pragma unroll
                for (int k = 0; k < DIM; ++k) sB[k * SC + base[it]] = g[it][a][k];
            }
            __syncthreads();
            if constexpr (DIM == 3) {
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    if (!(ok[it] && si[it] < P && sj[it] < P)) continue;
                    const int k = sk[it], o = base[it] - k * sz;
                    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
                    for (int m = 0; m < P; ++m) {
                        const double hk = th[m * SF_SD + k], dk = tdh[m * SF_SD + k];
                        c0 += hk * sB[o + m * sz];
                        c1 += hk * sB[SC + o + m * sz];
                        c2 += dk * sB[2 * SC + o + m * sz];
                    }
                    sC[base[it]] = c0;
                    sC[SC + base[it]] = c1;
                    sC[2 * SC + base[it]] = c2;
                }
                __syncthreads();
            }
            const double *sY = DIM == 3 ? sC : sB;  // the y pass's input: (d/dx, d/dy[, h h d/dz]) parts
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (!(ok[it] && si[it] < P)) continue;
                const int j = sj[it], o = base[it] - j * sy;
                double d0 = 0.0, d1 = 0.0;
                for (int m = 0; m < P; ++m) {
                    const double hj = th[m * SF_SD + j], dj = tdh[m * SF_SD + j];
                    d0 += hj * sY[o + m * sy];
                    d1 += dj * sY[SC + o + m * sy];
                    if constexpr (DIM == 3) d1 += hj * sY[2 * SC + o + m * sy];
                }
                sA[base[it]] = d0;
                sA[SC + base[it]] = d1;
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (!ok[it]) continue;
                const int i = si[it], o = base[it] - i;
                double s = 0.0;
                for (int m = 0; m < P; ++m) {
                    s += tdh[m * SF_SD + i] * sA[o + m];
                    s += th[m * SF_SD + i] * sA[SC + o + m];
                }
                res[it][a] = rule ? res[it][a] + s : s;
            }
        }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        if (!ok[it]) continue;
        double *out = ws + (LIST ? eid[it] * nn + (tid + it * 256 - sel[it] * nn) : t0 + tid + it * 256) * DIM;
#pragma unroll
        for (int a = 0; a < DIM; ++a) out[a] = negate ? -res[it][a] : res[it][a];
    }
}

template <int DIM>
__global__ __launch_bounds__(256) void k_sumfac_gather(int64_t N, const int32_t *__restrict__ incp,
                                                       const int32_t *__restrict__ inc,
                                                       const uint8_t *__restrict__ dir, const double *__restrict__ ws,
                                                       const double *__restrict__ x, double *__restrict__ y,
                                                       const int *__restrict__ istate)
{
    if (istate && istate[I_REASON] != 0) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * DIM) return;
    const int64_t node = i / DIM;
    const int a = (int)(i - node * DIM);
    if (dir[node]) {
        y[i] = x[i];  // setIndices2One: the unit Dirichlet diagonal of K and of Krhs
        return;
    }
    double s = 0.0;
    const int j1 = incp[node + 1];
    for (int j = incp[node]; j < j1; ++j) s += ws[(int64_t)inc[j] * DIM + a];
    y[i] = s;
}

// Rw_e w of a batch of whole elements: see the header.  The tiles, strides,
// tables and site decoding are k_sumfac_elem's.
template <int DIM, bool LIST = false>
__global__ __launch_bounds__(256) void k_sumfac_rw(int ngl, int nn, int neb, int sy, int sz, int se, int64_t E,
                                                   const double *__restrict__ tab, const double *__restrict__ geoF,
                                                   const double *__restrict__ geoR, const int32_t *__restrict__ conn,
                                                   const double *__restrict__ x, double *__restrict__ ws,
                                                   const int *__restrict__ istate, const int32_t *__restrict__ elist)
{
    if (istate && istate[I_REASON] != 0) return;
    constexpr int NIT = DIM == 3 ? 2 : 1;  // sites per thread: 512 at ngl 8 in 3-D
    constexpr int DW = DIM == 3 ? 3 : 1;   // components of w
    constexpr int G1 = 1 + DIM * DIM, SC = DIM == 3 ? SF_SC3 : SF_SC2;
    __shared__ double sx[DW * SC];                  // w, per component
    __shared__ double sA[2 * SC];                   // after the x pass: (h w, dh w); before the transposed x pass
    __shared__ double sB[DIM * SC];                 // after the y pass (3-D); the point fluxes
    __shared__ double sC[DIM == 3 ? 3 * SC : 1];    // after the transposed z pass (3-D); the reduced x pass (3-D)
    __shared__ double sd[4 * SF_ST];
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * neb;
    const int nt = (int)min((int64_t)neb, E - e0) * nn;  // (element, site) pairs of this batch
    const int64_t t0 = e0 * nn;
    {
        const int n2 = ngl * ngl;
        for (int t = tid; t < 4 * n2; t += 256) {
            const int tb = t / n2, r = t - tb * n2;
            sd[tb * SF_ST + (r / ngl) * SF_SD + r % ngl] = tab[tb * 64 + r];
        }
    }
    bool ok[NIT];
    int base[NIT], si[NIT], sj[NIT], sk[NIT], sel[NIT];
    int64_t eid[NIT];  // the element's own id
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int t = tid + it * 256;
        ok[it] = t < nt;
        const int el = t / nn, l = t - el * nn;
        eid[it] = LIST && ok[it] ? elist[e0 + el] : 0;
        const int r = l / ngl;
        si[it] = l % ngl;
        sj[it] = DIM == 3 ? r % ngl : r;
        sk[it] = DIM == 3 ? r / ngl : 0;
        sel[it] = el;
        base[it] = el * se + sk[it] * sz + sj[it] * sy + si[it];
        if (ok[it]) {
            const int64_t node = conn[LIST ? eid[it] * nn + l : t0 + t];  // (Rw drops no column)
#pragma unroll
            for (int b = 0; b < DW; ++b) sx[b * SC + base[it]] = x[node * DW + b];
        }
    }
    double res[NIT][DIM];
    // ================= full rule: c N_l curl w
    {
        const int P = ngl;
        const double *th = sd, *tdh = th + SF_ST;
        const int nq = DIM == 3 ? P * P * P : P * P;
        double g[NIT][DW][DIM];  // [component][reference direction]
        __syncthreads();         // w and the tables
        // ---- forward: reference gradient of every component at the points
#pragma unroll
        for (int a = 0; a < DW; ++a) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (!(ok[it] && si[it] < P)) continue;
                const int i = si[it], o = a * SC + base[it] - i;
                double ah = 0.0, ad = 0.0;
                for (int m = 0; m < ngl; ++m) {
                    const double v = sx[o + m];
                    ah += th[i * SF_SD + m] * v;
                    ad += tdh[i * SF_SD + m] * v;
                }
                sA[base[it]] = ah;
                sA[SC + base[it]] = ad;
            }
            __syncthreads();
            if constexpr (DIM == 2) {
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    if (!(ok[it] && si[it] < P && sj[it] < P)) continue;
                    const int j = sj[it], o = base[it] - j * sy;
                    double g0 = 0.0, g1 = 0.0;
                    for (int m = 0; m < ngl; ++m) {
                        g0 += th[j * SF_SD + m] * sA[SC + o + m * sy];
                        g1 += tdh[j * SF_SD + m] * sA[o + m * sy];
                    }
                    g[it][a][0] = g0;
                    g[it][a][1] = g1;
                }
            } else {
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    if (!(ok[it] && si[it] < P && sj[it] < P)) continue;
                    const int j = sj[it], o = base[it] - j * sy;
                    double b0 = 0.0, b1 = 0.0, b2 = 0.0;
                    for (int m = 0; m < ngl; ++m) {
                        const double ah = sA[o + m * sy], ad = sA[SC + o + m * sy];
                        const double hj = th[j * SF_SD + m], dj = tdh[j * SF_SD + m];
                        b0 += hj * ad;
                        b1 += dj * ah;
                        b2 += hj * ah;
                    }
                    sB[base[it]] = b0;
                    sB[SC + base[it]] = b1;
                    sB[2 * SC + base[it]] = b2;
                }
                __syncthreads();
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    if (!(ok[it] && si[it] < P && sj[it] < P && sk[it] < P)) continue;
                    const int k = sk[it], o = base[it] - k * sz;
                    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
                    for (int m = 0; m < ngl; ++m) {
                        const double hk = th[k * SF_SD + m], dk = tdh[k * SF_SD + m];
                        g0 += hk * sB[o + m * sz];
                        g1 += hk * sB[SC + o + m * sz];
                        g2 += dk * sB[2 * SC + o + m * sz];
                    }
                    g[it][a][0] = g0;
                    g[it][a][1] = g1;
                    g[it][a][2] = g2;
                }
            }
        }
        __syncthreads();  // the last component's reads of sA (2-D) and sB (3-D)
        // ---- the point: physical gradient, c curl w into sB
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (!(ok[it] && si[it] < P && sj[it] < P && sk[it] < P)) continue;
            const int q = (sk[it] * P + sj[it]) * P + si[it];
            const double *gp = geoF + ((LIST ? eid[it] : e0 + sel[it]) * nq + q) * G1;
            const double c = gp[0];
            double Ji[DIM][DIM];
#pragma unroll
            for (int b = 0; b < DIM; ++b)
#pragma unroll
                for (int k = 0; k < DIM; ++k) Ji[b][k] = gp[1 + b * DIM + k];
            double G[DW][DIM];  // G[a][b] = d_b w_a
#pragma unroll
            for (int a = 0; a < DW; ++a)
#pragma unroll
                for (int b = 0; b < DIM; ++b) {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < DIM; ++k) s += Ji[b][k] * g[it][a][k];
                    G[a][b] = s;
                }
            if constexpr (DIM == 3) {
                sB[base[it]] = c * (G[2][1] - G[1][2]);
                sB[SC + base[it]] = c * (G[0][2] - G[2][0]);
                sB[2 * SC + base[it]] = c * (G[1][0] - G[0][1]);
            } else {
                sB[base[it]] = c * G[0][1];
                sB[SC + base[it]] = -(c * G[0][0]);
            }
        }
        __syncthreads();
        // ---- value passes back, every component: z, y, x with h read transposed, q ascending
        if constexpr (DIM == 3) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (!(ok[it] && si[it] < P && sj[it] < P)) continue;
                const int k = sk[it], o = base[it] - k * sz;
                double c0 = 0.0, c1 = 0.0, c2 = 0.0;
                for (int m = 0; m < P; ++m) {
                    const double hk = th[m * SF_SD + k];
                    c0 += hk * sB[o + m * sz];
                    c1 += hk * sB[SC + o + m * sz];
                    c2 += hk * sB[2 * SC + o + m * sz];
                }
                sC[base[it]] = c0;
                sC[SC + base[it]] = c1;
                sC[2 * SC + base[it]] = c2;
            }
            __syncthreads();
        }
        {
            const double *sY = DIM == 3 ? sC : sB;  // the y pass's input
            double *sX = DIM == 3 ? sB : sA;        // ... and its output, the x pass's input
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (!(ok[it] && si[it] < P)) continue;
                const int j = sj[it], o = base[it] - j * sy;
                double d[DIM];
#pragma unroll
                for (int a = 0; a < DIM; ++a) d[a] = 0.0;
                for (int m = 0; m < P; ++m) {
                    const double hj = th[m * SF_SD + j];
#pragma unroll
                    for (int a = 0; a < DIM; ++a) d[a] += hj * sY[a * SC + o + m * sy];
                }
#pragma unroll
                for (int a = 0; a < DIM; ++a) sX[a * SC + base[it]] = d[a];
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (!ok[it]) continue;
                const int i = si[it], o = base[it] - i;
                double s[DIM];
#pragma unroll
                for (int a = 0; a < DIM; ++a) s[a] = 0.0;
                for (int m = 0; m < P; ++m) {
                    const double hi = th[m * SF_SD + i];
#pragma unroll
                    for (int a = 0; a < DIM; ++a) s[a] += hi * sX[a * SC + o + m];
                }
#pragma unroll
                for (int a = 0; a < DIM; ++a) res[it][a] = s[a];
            }
        }
    }
    // ================= reduced rule: a_w c (w x grad N_l)
    {
        const int P = ngl - 1;
        const double *th = sd + 2 * SF_ST, *tdh = th + SF_ST;
        const int nq = DIM == 3 ? P * P * P : P * P;
        double w[NIT][DW];
        __syncthreads();  // the full rule's reads of sA / sB
        // ---- forward value passes, every component: x, y (, z), m ascending
        {
            double *sX = DIM == 3 ? sC : sA;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (!(ok[it] && si[it] < P)) continue;
                const int i = si[it], o = base[it] - i;
                double a[DW];
#pragma unroll
                for (int c = 0; c < DW; ++c) a[c] = 0.0;
                for (int m = 0; m < ngl; ++m) {
                    const double hi = th[i * SF_SD + m];
#pragma unroll
                    for (int c = 0; c < DW; ++c) a[c] += hi * sx[c * SC + o + m];
                }
#pragma unroll
                for (int c = 0; c < DW; ++c) sX[c * SC + base[it]] = a[c];
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (!(ok[it] && si[it] < P && sj[it] < P)) continue;
                const int j = sj[it], o = base[it] - j * sy;
                double a[DW];
#pragma unroll
                for (int c = 0; c < DW; ++c) a[c] = 0.0;
                for (int m = 0; m < ngl; ++m) {
                    const double hj = th[j * SF_SD + m];
#pragma unroll
                    for (int c = 0; c < DW; ++c) a[c] += hj * sX[c * SC + o + m * sy];
                }
#pragma unroll
                for (int c = 0; c < DW; ++c) {
                    if constexpr (DIM == 3) sB[c * SC + base[it]] = a[c];
                    else w[it][c] = a[c];
                }
            }
            if constexpr (DIM == 3) {
                __syncthreads();
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    if (!(ok[it] && si[it] < P && sj[it] < P && sk[it] < P)) continue;
                    const int k = sk[it], o = base[it] - k * sz;
                    double a[DW];
#pragma unroll
                    for (int c = 0; c < DW; ++c) a[c] = 0.0;
                    for (int m = 0; m < ngl; ++m) {
                        const double hk = th[k * SF_SD + m];
#pragma unroll
                        for (int c = 0; c < DW; ++c) a[c] += hk * sB[c * SC + o + m * sz];
                    }
#pragma unroll
                    for (int c = 0; c < DW; ++c) w[it][c] = a[c];
                }
            }
        }
        // ---- the point: the flux a_w c eps_{acb} w_c, back to reference directions with inv J^T
        double g[NIT][DIM][DIM];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (!(ok[it] && si[it] < P && sj[it] < P && sk[it] < P)) continue;
            const int q = (sk[it] * P + sj[it]) * P + si[it];
            const double *gp = geoR + ((LIST ? eid[it] : e0 + sel[it]) * nq + q) * G1;
            const double c = gp[0];
            double Ji[DIM][DIM];
#pragma unroll
            for (int b = 0; b < DIM; ++b)
#pragma unroll
                for (int k = 0; k < DIM; ++k) Ji[b][k] = gp[1 + b * DIM + k];
            double t[DW];
#pragma unroll
            for (int cc = 0; cc < DW; ++cc) t[cc] = c * (SF_ALPHA_W * w[it][cc]);
            if constexpr (DIM == 3) {
#pragma unroll
                for (int k = 0; k < DIM; ++k) {
                    g[it][0][k] = Ji[2][k] * t[1] - Ji[1][k] * t[2];
                    g[it][1][k] = Ji[0][k] * t[2] - Ji[2][k] * t[0];
                    g[it][2][k] = Ji[1][k] * t[0] - Ji[0][k] * t[1];
                }
            } else {
#pragma unroll
                for (int k = 0; k < DIM; ++k) {
                    g[it][0][k] = -(Ji[1][k] * t[0]);
                    g[it][1][k] = Ji[0][k] * t[0];
                }
            }
        }
        __syncthreads();  // the z pass's reads of sB (3-D)
        // ---- transposed passes, per component, as k_sumfac_elem
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (!(ok[it] && si[it] < P && sj[it] < P && sk[it] < P)) continue;
#pragma unroll
                for (int k = 0; k < DIM; ++k) sB[k * SC + base[it]] = g[it][a][k];
            }
            __syncthreads();
            if constexpr (DIM == 3) {
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    if (!(ok[it] && si[it] < P && sj[it] < P)) continue;
                    const int k = sk[it], o = base[it] - k * sz;
                    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
                    for (int m = 0; m < P; ++m) {
                        const double hk = th[m * SF_SD + k], dk = tdh[m * SF_SD + k];
                        c0 += hk * sB[o + m * sz];
                        c1 += hk * sB[SC + o + m * sz];
                        c2 += dk * sB[2 * SC + o + m * sz];
                    }
                    sC[base[it]] = c0;
                    sC[SC + base[it]] = c1;
                    sC[2 * SC + base[it]] = c2;
                }
                __syncthreads();
            }
            const double *sY = DIM == 3 ? sC : sB;  // the y pass's input: (d/dx, d/dy[, h h d/dz]) parts
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (!(ok[it] && si[it] < P)) continue;
                const int j = sj[it], o = base[it] - j * sy;
                double d0 = 0.0, d1 = 0.0;
                for (int m = 0; m < P; ++m) {
                    const double hj = th[m * SF_SD + j], dj = tdh[m * SF_SD + j];
                    d0 += hj * sY[o + m * sy];
                    d1 += dj * sY[SC + o + m * sy];
                    if constexpr (DIM == 3) d1 += hj * sY[2 * SC + o + m * sy];
                }
                sA[base[it]] = d0;
                sA[SC + base[it]] = d1;
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (!ok[it]) continue;
                const int i = si[it], o = base[it] - i;
                double s = 0.0;
                for (int m = 0; m < P; ++m) {
                    s += tdh[m * SF_SD + i] * sA[o + m];
                    s += th[m * SF_SD + i] * sA[SC + o + m];
                }
                res[it][a] += s;
            }
        }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        if (!ok[it]) continue;
        double *out = ws + (LIST ? eid[it] * nn + (tid + it * 256 - sel[it] * nn) : t0 + tid + it * 256) * DIM;
#pragma unroll
        for (int a = 0; a < DIM; ++a) out[a] = res[it][a];
    }
}

template <int DIM>
__global__ __launch_bounds__(256) void k_sumfac_gather_rw(int64_t N, const int32_t *__restrict__ incp,
                                                          const int32_t *__restrict__ inc,
                                                          const uint8_t *__restrict__ dir,
                                                          const double *__restrict__ ws, double *__restrict__ y,
                                                          const int *__restrict__ istate)
{
    if (istate && istate[I_REASON] != 0) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * DIM) return;
    const int64_t node = i / DIM;
    const int a = (int)(i - node * DIM);
    double s = 0.0;
    if (!dir[node]) {  // (a Dirichlet row of Rw is empty: +0.0, nothing read)
        const int j1 = incp[node + 1];
        for (int j = incp[node]; j < j1; ++j) s += ws[(int64_t)inc[j] * DIM + a];
    }
    y[i] = s;
}

// the diagonal of K_e per (element, node), into ws[e][l][a]
template <int DIM>
__global__ __launch_bounds__(256) void k_sumfac_diag(int ngl, int nn, int64_t E, const double *__restrict__ tab,
                                                     const double *__restrict__ geoF, const double *__restrict__ geoR,
                                                     double *__restrict__ ws)
{
    constexpr int G1 = 1 + DIM * DIM;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= E * nn) return;
    const int64_t e = t / nn;
    const int l = (int)(t - e * nn);
    const int li[3] = {l % ngl, (l / ngl) % ngl, DIM == 3 ? l / (ngl * ngl) : 0};
    double sF = 0.0, sR[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) sR[a] = 0.0;
    for (int rule = 0; rule < 2; ++rule) {
        const int P = rule ? ngl - 1 : ngl;
        const double *th = tab + rule * 128, *tdh = th + 64;
        const int nq = DIM == 3 ? P * P * P : P * P;
        const double *geo = (rule ? geoR : geoF) + e * nq * G1;
        for (int q = 0; q < nq; ++q) {
            const int qi[3] = {q % P, (q / P) % P, DIM == 3 ? q / (P * P) : 0};
            double hh[DIM], dd[DIM], dref[DIM], gr[DIM];
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                hh[d] = th[qi[d] * ngl + li[d]];
                dd[d] = tdh[qi[d] * ngl + li[d]];
            }
            if constexpr (DIM == 2) {
                dref[0] = dd[0] * hh[1];
                dref[1] = hh[0] * dd[1];
            } else {
                dref[0] = dd[0] * hh[1] * hh[2];
                dref[1] = hh[0] * dd[1] * hh[2];
                dref[2] = hh[0] * hh[1] * dd[2];
            }
            const double *gp = geo + q * G1;
            double n2 = 0.0;
#pragma unroll
            for (int i = 0; i < DIM; ++i) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < DIM; ++k) s += gp[1 + i * DIM + k] * dref[k];
                gr[i] = s;
                n2 += s * s;
            }
            if (rule == 0) {
                sF += gp[0] * n2;
            } else {
#pragma unroll
                for (int a = 0; a < DIM; ++a) {
                    const double ga = gr[a] * gr[a];
                    sR[a] += gp[0] * (SF_ALPHA_D * ga + SF_ALPHA_W * (n2 - ga));
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < DIM; ++a) ws[t * DIM + a] = sF + sR[a];
}

// diagonal: the incident elements' entries in gather order (K), 0 (Krhs: a
// free row holds Dirichlet columns only); 1 on Dirichlet rows
template <int DIM>
__global__ __launch_bounds__(256) void k_sumfac_diag_gather(int64_t N, int which, const int32_t *__restrict__ incp,
                                                            const int32_t *__restrict__ inc,
                                                            const uint8_t *__restrict__ dir,
                                                            const double *__restrict__ ws, double *__restrict__ d)
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
    if (which == 0) {
        const int j1 = incp[node + 1];
        for (int j = incp[node]; j < j1; ++j) s += ws[(int64_t)inc[j] * DIM + a];
    }
    d[i] = s;
}

// No-slip operators: one thread per owned DoF, its row by the rule byte of its
// class (as k_elem_gather_cls) -- zero (+0.0, nothing read), the identity (x_i
// bit for bit) or the sum of its node's incidence entries from the element
// results of pass 0 or pass 1, ascending element; NS_MINUS_X adds -x_i (the -1
// on Kfs's tangential diagonal).  x is null where the column space is the
// vorticity's (Rw, Rwfs: no rule of theirs reads it).
template <int DIM>
__global__ __launch_bounds__(256) void k_sumfac_gather_cls(int64_t N, unsigned rules,
                                                           const int32_t *__restrict__ incp,
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
    const int j1 = incp[node + 1];
    for (int j = incp[node]; j < j1; ++j) s += ws[(int64_t)inc[j] * DIM + a];
    if (r & NS_MINUS_X) s += -x[i];
    y[i] = s;
}

// diagonal by class: 0, 1 (identity rows), the incident elements' diagonal
// entries in gather order, those sums + (-1) (Kfs's tangential rows)
template <int DIM>
__global__ __launch_bounds__(256) void k_sumfac_diag_gather_cls(int64_t N, unsigned drules,
                                                                const int32_t *__restrict__ incp,
                                                                const int32_t *__restrict__ inc,
                                                                const uint8_t *__restrict__ cls,
                                                                const double *__restrict__ ws, double *__restrict__ d)
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
    const int j1 = incp[node + 1];
    for (int j = incp[node]; j < j1; ++j) s += ws[(int64_t)inc[j] * DIM + a];
    d[i] = r == 3 ? s + (-1.0) : s;
}

// dst_i = src_i on the identity rows of a no-slip operator, nothing else touched
__global__ __launch_bounds__(256) void k_sumfac_copy_ident_cls(int64_t n, unsigned rules,
                                                               const uint8_t *__restrict__ cls,
                                                               const double *__restrict__ src, double *__restrict__ dst)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (((rules >> (8 * cls[i])) & NS_KIND) == NS_IDENT) dst[i] = src[i];
}

// the element kernel over every element in order (list null: one rank), or
// over the n elements list names
template <int DIM>
static void launch_sumfac_elems(const SumfacOp *P, hipStream_t st, const int32_t *list, int64_t n, const double *x,
                                const int *istate)
{
    const unsigned ge = (unsigned)((n + P->neb - 1) / P->neb);
#define KLE_SUMFAC_ELEMS(LIST)                                                                                        \
    do {                                                                                                              \
        if (P->which == 2)                                                                                            \
            hipLaunchKernelGGL((k_sumfac_rw<DIM, LIST>), dim3(ge), dim3(256), 0, st, P->ngl, P->nn, P->neb, P->sy,    \
                               P->sz, P->se, n, P->d_tab, P->d_geoF, P->d_geoR, P->d_conn, x, P->d_ws, istate, list); \
        else if (P->ns) /* a pass per kept class set, each into its own result array (Kfs: two) */                    \
            for (int p = 0; p < P->npass; ++p)                                                                        \
                hipLaunchKernelGGL((k_sumfac_elem<DIM, LIST, true>), dim3(ge), dim3(256), 0, st, P->ngl, P->nn,       \
                                   P->neb, P->sy, P->sz, P->se, n, P->negate, P->d_tab, P->d_geoF, P->d_geoR,         \
                                   P->d_conn, x, P->d_wsp[p], istate, list, P->d_ncls, P->keep[p]);                   \
        else                                                                                                          \
            hipLaunchKernelGGL((k_sumfac_elem<DIM, LIST>), dim3(ge), dim3(256), 0, st, P->ngl, P->nn, P->neb, P->sy,  \
                               P->sz, P->se, n, P->negate, P->d_tab, P->d_geoF, P->d_geoR, P->d_conn, x, P->d_ws,     \
                               istate, list, nullptr, 0u);                                                            \
    } while (0)
    if (list) KLE_SUMFAC_ELEMS(true);
    else KLE_SUMFAC_ELEMS(false);
#undef KLE_SUMFAC_ELEMS
}

// the owned rows' gather (x: the owned part; Rw never reads it)
template <int DIM>
static void launch_sumfac_gather(const SumfacOp *P, hipStream_t st, const double *x, double *y, const int *istate)
{
    const unsigned gn = (unsigned)((P->N * DIM + 255) / 256);
    if (P->ns)  // (Rw, Rwfs: x is the vorticity -- their rules, zero and sum, never read it)
        hipLaunchKernelGGL(k_sumfac_gather_cls<DIM>, dim3(gn), dim3(256), 0, st, P->N, P->rules, P->d_incp, P->d_inc,
                           P->d_cls, P->d_wsp[0], P->d_wsp[1], P->which == 2 ? nullptr : x, y, istate);
    else if (P->which == 2)
        hipLaunchKernelGGL(k_sumfac_gather_rw<DIM>, dim3(gn), dim3(256), 0, st, P->N, P->d_incp, P->d_inc, P->d_dir,
                           P->d_ws, y, istate);
    else
        hipLaunchKernelGGL(k_sumfac_gather<DIM>, dim3(gn), dim3(256), 0, st, P->N, P->d_incp, P->d_inc, P->d_dir,
                           P->d_ws, x, y, istate);
}

int sumfac_spmv(kle_mat *A, const kle_vec *x, kle_vec *y, const int *istate, bool local)
{
    const SumfacOp *P = A->sumfac;
    if (!P) return fail(KLE_ERR_STATE, "sum-factorised operator without tables");
    KLE_TRY(elem_check_vecs(A, x, y, "sum-factorised operator"));
    hipStream_t st = A->ctx->stream;
    // (x: the ghosted allocation, read in ext-local ids)
    auto elems = [&](const int32_t *list, int64_t n) -> int {
        if (P->dim == 2) launch_sumfac_elems<2>(P, st, list, n, x->base, istate);
        else launch_sumfac_elems<3>(P, st, list, n, x->base, istate);
        KLE_HIP(hipGetLastError());
        return 0;
    };
    if (!P->d_elist) KLE_TRY(elems(nullptr, P->E));
    else  // list positions [0, el_int1) inner, the rest outer: elem_ranges' interior and top layer, no ghost layer
        KLE_TRY(elem_ranges(A, x, local,
                            [&](int64_t l0, int64_t l1, bool) -> int { return elems(P->d_elist + l0, l1 - l0); }));
    if (P->dim == 2) launch_sumfac_gather<2>(P, st, x->d, y->d, istate);
    else launch_sumfac_gather<3>(P, st, x->d, y->d, istate);
    KLE_HIP(hipGetLastError());
    return 0;
}

int sumfac_diagonal(const kle_mat *A, kle_vec *d)
{
    const SumfacOp *P = A->sumfac;
    if (P && P->which == 2) return fail(KLE_ERR_SUP, "getDiagonal: the sum-factorised Rw is rectangular");  // (Rwfs too)
    if (!P || !P->d_diag) return fail(KLE_ERR_STATE, "sum-factorised operator without tables");
    hipStream_t st = A->ctx->stream;
    KLE_HIP(hipMemcpyAsync(d->d, P->d_diag, sizeof(double) * (size_t)P->N * P->dim, hipMemcpyDeviceToDevice, st));
    KLE_HIP(hipStreamSynchronize(st));
    return 0;
}

// dst_i = src_i on the identity rows of a no-slip operator (the free-slip
// operators refuse: kle_mat_copy_dirichlet_rows)
int sumfac_copy_ident_rows(const kle_mat *A, const kle_vec *src, kle_vec *dst)
{
    const SumfacOp *P = A->sumfac;
    if (!P || !P->ns)
        return fail(KLE_ERR_SUP, "copyDirichletRows: an element-wise operator only (it holds the Dirichlet flags)");
    const int64_t n = P->N * P->dim;
    if (src->n_local != n || dst->n_local != n)
        return fail(KLE_ERR_SIZ, "copyDirichletRows: vectors do not match the operator's rows");
    if (src->d == dst->d) return 0;
    hipLaunchKernelGGL(k_sumfac_copy_ident_cls, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, A->ctx->stream, n,
                       P->rules, P->d_cls, src->d, dst->d);
    KLE_HIP(hipGetLastError());
    return 0;
}

void sumfac_drop(kle_mat *A)
{
    SumfacOp *P = A->sumfac;
    if (!P) return;
    (void)hipFree(P->d_tab);  // (the geometry tables go with the last holder of P->geo)
    (void)hipFree(P->d_ws);
    (void)hipFree(P->d_diag);
    (void)hipFree(P->d_conn);
    (void)hipFree(P->d_incp);
    (void)hipFree(P->d_inc);
    (void)hipFree(P->d_dir);
    (void)hipFree(P->d_elist);
    (void)hipFree(P->d_ncls);
    (void)hipFree(P->d_cls);
    (void)hipFree(P->d_wsp[1]);  // (d_wsp[0] is d_ws)
    delete P;
    A->sumfac = nullptr;
}

static int64_t sf_ipow(int b, int d) { return d == 2 ? (int64_t)b * b : (int64_t)b * b * b; }

// Algorithmic bytes of one product.  k_sumfac_elem: the connectivity (4 E nn),
// both geometry tables (8 E (nqF + nqR) (1 + dim^2)), the 1-D tables, x read
// once (8 n), the element results written (8 E nn dim).  k_sumfac_gather: the
// incidence list (4 (N + 1) + 4 E nn), the Dirichlet flags (N), the element
// results read, y written (8 m).  Rw: the same streams with its own n.
// Several ranks: E the local elements, n the ext range of x, N the owned
// nodes, and the two element lists (4 E).  A no-slip operator: every
// element-kernel stream once per pass, the class table with it (E nn bytes per
// pass, K-family operators), one result array per pass written and read, and
// the owned DoFs' class bytes (N dim) instead of the Dirichlet flags.
double sumfac_spmv_bytes(const kle_mat *A)
{
    const SumfacOp *P = A->sumfac;
    if (!P) return 0.0;
    const double nq = (double)(sf_ipow(P->npF, P->dim) + sf_ipow(P->npR, P->dim));
    if (P->ns) {
        const double elem = 4.0 * P->E * P->nn + (P->d_ncls ? 1.0 * P->E * P->nn : 0.0) +
                            8.0 * P->E * nq * (1 + P->dim * P->dim) + 8.0 * 4 * P->ngl * P->ngl +
                            8.0 * (A->n_local + A->ghost_lo + A->ghost_hi) + 2.0 * 8.0 * P->E * P->nn * P->dim +
                            (P->d_elist ? 4.0 * P->E : 0.0);
        return P->npass * elem + 4.0 * (P->N + 1) + 4.0 * P->ninc + 1.0 * P->N * P->dim + 8.0 * A->m_local;
    }
    return 4.0 * P->E * P->nn + 8.0 * P->E * nq * (1 + P->dim * P->dim) + 8.0 * 4 * P->ngl * P->ngl +
           8.0 * (A->n_local + A->ghost_lo + A->ghost_hi) + 2.0 * 8.0 * P->E * P->nn * P->dim + 4.0 * (P->N + 1) +
           4.0 * P->ninc + 1.0 * P->N + 8.0 * A->m_local + (P->d_elist ? 4.0 * P->E : 0.0);
}

std::string sumfac_kernel_name(const kle_mat *A)
{
    const SumfacOp *P = A->sumfac;
    if (!P) return "?";
    const std::string d = std::to_string(P->dim);
    if (P->ns)
        return (P->which == 2 ? "k_sumfac_rw<" + d + ">" : "k_sumfac_elem<" + d + ",cls>" + (P->npass == 2 ? "x2" : "")) +
               "+k_sumfac_gather_cls<" + d + ">";
    if (P->which == 2) return "k_sumfac_rw<" + d + ">+k_sumfac_gather_rw<" + d + ">";
    return "k_sumfac_elem<" + d + ">+k_sumfac_gather<" + d + ">";
}

// Every index the device tables hold, checked on the host before upload: a
// bad table is an error code, never an out-of-range access.  conn [E][nn]
// (unmasked) names ext-local nodes in [0, next), the owned ones [own0, own0 + N)
// (one rank: next = N, own0 = 0).  Owned node i's incidence entries
// inc[incp[i] .. incp[i + 1]) are positions of conn that name it, their
// elements strictly ascending, and together they cover every position of conn
// that names an owned node.  elist (several ranks, else null): [0, n_inner)
// and [n_inner, E) each ascend, are disjoint and cover the elements; an inner
// element names owned nodes only, an outer one at least one ghost.
int sumfac_validate(const std::vector<int32_t> &conn, const std::vector<int32_t> &incp,
                    const std::vector<int32_t> &inc, int64_t E, int64_t N, int nn, int dim, int64_t next, int64_t own0,
                    const std::vector<int32_t> *elist, int64_t n_inner)
{
    if (next < 0) next = N;
    if (E < 1 || N < 1 || nn < 1) return fail(KLE_ERR_OUTOFRANGE, "sum-factorised operator: empty mesh");
    if (own0 < 0 || own0 + N > next)
        return fail(KLE_ERR_OUTOFRANGE, "sum-factorised operator: the owned nodes lie outside the ext range");
    if (E * nn >= INT32_MAX || next * dim >= INT32_MAX)
        return fail(KLE_ERR_SUP, "sum-factorised operator: the mesh exceeds the 32-bit tables");
    if ((int64_t)conn.size() != E * nn || (int64_t)incp.size() != N + 1)
        return fail(KLE_ERR_SIZ, "sum-factorised operator: table sizes do not match the mesh");
    int64_t nowned = 0;
    for (int64_t k = 0; k < E * nn; ++k) {
        if (conn[k] < 0 || conn[k] >= next)
            return fail(KLE_ERR_OUTOFRANGE, "sum-factorised operator: connectivity entry %lld = %d outside [0, %lld)",
                        (long long)k, conn[k], (long long)next);
        nowned += conn[k] >= own0 && conn[k] < own0 + N;
    }
    if ((int64_t)inc.size() != nowned)
        return fail(KLE_ERR_SIZ, "sum-factorised operator: table sizes do not match the mesh");
    if (incp[0] != 0 || incp[N] != nowned)
        return fail(KLE_ERR_OUTOFRANGE, "sum-factorised operator: the incidence list does not cover the connectivity");
    for (int64_t i = 0; i < N; ++i) {
        if (incp[i + 1] < incp[i] || incp[i + 1] > nowned)
            return fail(KLE_ERR_OUTOFRANGE, "sum-factorised operator: incidence offsets of node %lld descend", (long long)i);
        int64_t prev = -1;
        for (int32_t j = incp[i]; j < incp[i + 1]; ++j) {
            const int32_t t = inc[j];
            if (t < 0 || (int64_t)t >= E * nn || conn[t] != i + own0 || t / nn <= prev)
                return fail(KLE_ERR_OUTOFRANGE, "sum-factorised operator: incidence entry %d of node %lld is inconsistent",
                            j - incp[i], (long long)i);
            prev = t / nn;
        }
    }
    if (!elist) return 0;
    if ((int64_t)elist->size() != E || n_inner < 0 || n_inner > E)
        return fail(KLE_ERR_SIZ, "sum-factorised operator: the element lists do not match the mesh");
    std::vector<uint8_t> seen((size_t)E, 0);
    for (int64_t k = 0; k < E; ++k) {
        const int32_t e = (*elist)[k];
        if (e < 0 || e >= E || seen[e] || (k > 0 && k != n_inner && e <= (*elist)[k - 1]))
            return fail(KLE_ERR_OUTOFRANGE, "sum-factorised operator: element list entry %lld = %d is out of range, "
                                            "repeated or out of order", (long long)k, e);
        seen[e] = 1;
        bool ghost = false;
        for (int l = 0; l < nn; ++l) ghost |= conn[(int64_t)e * nn + l] < own0 || conn[(int64_t)e * nn + l] >= own0 + N;
        if (ghost != (k >= n_inner))
            return fail(KLE_ERR_OUTOFRANGE, "sum-factorised operator: %s element %d %s", k < n_inner ? "inner" : "outer",
                        e, k < n_inner ? "names a ghost node" : "names no ghost node");
    }
    return 0;  // (E distinct entries in [0, E): the lists cover the elements)
}

// The host tables of a sum-factorised operator on ctx's part of m, validated:
// the layout (L.eint1 the inner elements), conn [E][nn] in ext-local ids
// (unmasked), the CSR incidence list of the owned nodes, ascending local
// element (= ascending global cell id), and on several ranks the element
// lists, inner then outer.  bw: the operator's widest block.
int sumfac_tables(const kle_ctx *ctx, const kle_mesh *m, int bw, ElemLayout *Lout, std::vector<int32_t> &conn,
                  std::vector<int32_t> &incp, std::vector<int32_t> &inc, std::vector<int32_t> &elist)
{
    if (m->nranks != ctx->nranks)
        return fail(KLE_ERR_SUP, "sum-factorised operator: the mesh is partitioned for %d ranks, the context has %d",
                    m->nranks, ctx->nranks);
    KLE_ARG(m->rank == ctx->rank, "mesh partition does not match ctx");
    const int nn = m->nn();
    ElemLayout L;
    L.N = m->node_end - m->node_begin;
    L.next = m->ext_end - m->ext_begin;
    L.own0 = m->node_begin - m->ext_begin;
    L.E = L.eint1 = m->n_local_elems();
    const int64_t E = L.E, N = L.N;
    KLE_ARG(E >= 1 && N >= 1 && L.own0 >= 0 && L.own0 + N <= L.next &&
                (m->nranks > 1 || (m->node_begin == 0 && L.own0 == 0 && L.next == N && N == m->N)),
            "unexpected mesh layout");
    if (E * nn >= INT32_MAX || L.next * bw >= INT32_MAX)
        return fail(KLE_ERR_SUP, "sum-factorised operator: the mesh exceeds the 32-bit tables");
    // (a graph partition's u_conn holds the pseudo ids ext_begin + ext position)
    std::vector<int64_t> conn64((size_t)E * nn);
    if (m->kind == 1) {
        if ((int64_t)m->u_conn.size() != E * nn)
            return fail(KLE_ERR_SIZ, "sum-factorised operator: the connectivity does not match the mesh");
        conn64 = m->u_conn;
    } else {
        KLE_TRY(kle_mesh_get_conn(m, conn64.data()));
    }
    conn.assign((size_t)E * nn, 0);
    incp.assign((size_t)N + 1, 0);
    for (int64_t k = 0; k < E * nn; ++k) {
        const int64_t g = conn64[k] - m->ext_begin;
        if (g < 0 || g >= L.next)
            return fail(KLE_ERR_OUTOFRANGE, "sum-factorised operator: connectivity entry %lld outside the mesh", (long long)k);
        conn[k] = (int32_t)g;
        if (g >= L.own0 && g < L.own0 + N) ++incp[g - L.own0 + 1];  // (a ghost node: read, never written)
    }
    for (int64_t i = 0; i < N; ++i) incp[i + 1] += incp[i];
    inc.assign((size_t)incp[N], -1);
    {
        std::vector<int32_t> fill(incp.begin(), incp.end() - 1);
        for (int64_t k = 0; k < E * nn; ++k) {
            const int64_t o = conn[k] - L.own0;
            if (o >= 0 && o < N) inc[fill[o]++] = (int32_t)k;  // k = e * nn + l, ascending e
        }
    }
    elist.clear();
    if (m->nranks > 1) {
        std::vector<int32_t> outer;
        for (int64_t e = 0; e < E; ++e) {
            bool ghost = false;
            for (int l = 0; l < nn; ++l) ghost |= conn[e * nn + l] < L.own0 || conn[e * nn + l] >= L.own0 + N;
            (ghost ? outer : elist).push_back((int32_t)e);
        }
        L.eint1 = (int64_t)elist.size();
        elist.insert(elist.end(), outer.begin(), outer.end());
    }
    KLE_TRY(sumfac_validate(conn, incp, inc, E, N, nn, bw, L.next, L.own0, m->nranks > 1 ? &elist : nullptr, L.eint1));
    *Lout = L;
    return 0;
}

}  // namespace kle

using namespace kle;

// which: 0 K, 1 Krhs, 2 Rw of a free-slip mesh (ns < 0); ns 0 .. 6: the no-slip
// operator NS_SPECS[ns] of a mesh with its DoF classes, which its kernel
// family (0: k_sumfac_elem with the class table, 2: k_sumfac_rw)
static int sumfac_create(kle_ctx *ctx, kle_mesh *m, int which, kle_mat **out, int ns = -1)
{
    const NsSpec *S = ns >= 0 ? &NS_SPECS[ns] : nullptr;
    if (!S && !m->dof_cls.empty())
        return fail(KLE_ERR_SUP, "sum-factorised operator: a no-slip mesh (its operators: kle_mat_create_ns_sumfac)");
    if (S && m->dof_cls.empty())
        return fail(KLE_ERR_SUP, "sum-factorised no-slip operator: the mesh has no no-slip DoFs (kle_mesh_set_noslip_*)");
    const int dim = m->dim, ngl = m->ngl, nn = m->nn();
    KLE_ARG((dim == 2 || dim == 3) && ngl >= 2 && ngl <= 8, "sum-factorised operator: dim 2 or 3, ngl 2..8");
    // tables (host) in ext-local ids, validated before upload
    ElemLayout L;
    std::vector<int32_t> conn, incp, inc, elist;
    KLE_TRY(sumfac_tables(ctx, m, dim, &L, conn, incp, inc, elist));
    const int64_t E = L.E, N = L.N;
    std::vector<uint8_t> ncls;
    if (S) {
        if ((int64_t)m->dof_cls.size() != L.next * dim)
            return fail(KLE_ERR_SIZ, "sum-factorised operator: DoF classes do not cover the mesh's ext range");
        for (size_t k = 0; k < m->dof_cls.size(); ++k)
            if (m->dof_cls[k] > DOF_NORMAL)
                return fail(KLE_ERR_OUTOFRANGE, "sum-factorised operator: DoF %lld has the unknown class %d",
                            (long long)k, (int)m->dof_cls[k]);
        // the mask acts per DoF: conn stays unmasked (sumfac_tables checked it
        // against the ext range the classes cover) and every element node
        // carries the classes of its dim DoFs, ghosts included, 2 bits each
        if (!S->rw) {
            ncls.assign((size_t)E * nn, 0);
            for (int64_t k = 0; k < E * nn; ++k)
                for (int b = 0; b < dim; ++b) ncls[k] |= (uint8_t)(m->dof_cls[(int64_t)conn[k] * dim + b] << (2 * b));
        }
    } else {
        KLE_ARG(m->dir_set, "Dirichlet nodes not set (kle_mesh_set_dirichlet_*)");
        if ((int64_t)m->dir.size() != L.next)
            return fail(KLE_ERR_SIZ, "sum-factorised operator: Dirichlet flags do not match the mesh");
        // the mask rule folded into the connectivity the element kernel reads: K
        // drops the Dirichlet entries of x (ghosts included: m->dir covers the ext
        // range), Krhs the free ones
        // (Rw drops nothing)
        for (int64_t k = 0; k < E * nn && which != 2; ++k)
            if ((m->dir[conn[k]] != 0) != (which == 1)) conn[k] = -1;
    }

    // LDS layout: odd strides (in doubles) of the y lines, z planes and elements
    // (a workgroup's only element needs no element stride), as kle_colloc.hip
    const int neb = std::max(1, 256 / nn);
    const int sy = ngl | 1, sz = dim == 3 ? (ngl * sy) | 1 : 0, se = ngl * (dim == 3 ? sz : sy) | (neb > 1 ? 1 : 0);
    if ((int64_t)neb * se > (dim == 3 ? SF_SC3 : SF_SC2) || (int64_t)neb * nn > (dim == 3 ? 512 : 256))
        return fail(KLE_ERR_STATE, "sum-factorised operator: %d elements of stride %d exceed the LDS tile", neb, se);

    // the 1-D tables of kle_basis, [q][a]
    PointSet1D full, red, op;
    element_sets(ngl, full, red, op);
    const int npF = (int)full.x.size(), npR = (int)red.x.size();
    if (npF != ngl || npR != ngl - 1 || (int)full.h.size() != npF * ngl || (int)red.dh.size() != npR * ngl)
        return fail(KLE_ERR_STATE, "sum-factorised operator: unexpected quadrature rules");
    std::vector<double> tab(256, 0.0);
    std::copy(full.h.begin(), full.h.end(), tab.begin());
    std::copy(full.dh.begin(), full.dh.end(), tab.begin() + 64);
    std::copy(red.h.begin(), red.h.end(), tab.begin() + 128);
    std::copy(red.dh.begin(), red.dh.end(), tab.begin() + 192);

    KLE_HIP(hipSetDevice(ctx->device));
    kle_mat *A = new kle_mat;
    SumfacOp *P = new SumfacOp;
    A->ctx = ctx;
    A->sumfac = P;
    elem_mat_fields(A, m, L, dim, which == 2 ? (dim == 2 ? 1 : 3) : dim);
    P->which = which;
    P->negate = S ? S->negate : which == 1;
    if (S) {
        P->ns = 1;
        P->ns_which = ns;
        P->npass = S->npass;
        P->keep[0] = S->cols[0];
        P->keep[1] = S->cols[1];
        ns_rule_words(*S, &P->rules, &P->drules);
    }
    P->dim = dim;
    P->ngl = ngl;
    P->nn = nn;
    P->neb = neb;
    P->sy = sy;
    P->sz = sz;
    P->se = se;
    P->npF = npF;
    P->npR = npR;
    P->E = E;
    P->N = N;
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
    // c_q and inv J of every element at both rules' points: the assembly's own
    // geometry kernel on the mesh's own corners
    int rc = mesh_geometry(ctx, m, true, false, &P->geo);
    if (!rc && (P->geo->npF != npF || P->geo->npR != npR))
        rc = fail(KLE_ERR_STATE, "sum-factorised operator: geometry tables do not match the rules");
    if (!rc) {
        P->d_geoF = P->geo->F;
        P->d_geoR = P->geo->R;
    }
    if (!rc) rc = up(&P->d_tab, tab.data(), sizeof(double) * tab.size());
    if (!rc) rc = up(&P->d_conn, conn.data(), sizeof(int32_t) * conn.size());
    if (!rc) rc = up(&P->d_incp, incp.data(), sizeof(int32_t) * incp.size());
    if (!rc) rc = up(&P->d_inc, inc.data(), sizeof(int32_t) * inc.size());
    if (!rc && !S) rc = up(&P->d_dir, m->dir.data() + L.own0, (size_t)N);
    if (!rc && S) rc = up(&P->d_cls, m->dof_cls.data() + L.own0 * dim, (size_t)N * dim);
    if (!rc && !ncls.empty()) rc = up(&P->d_ncls, ncls.data(), ncls.size());
    if (!rc && !elist.empty()) rc = up(&P->d_elist, elist.data(), sizeof(int32_t) * elist.size());
    if (!rc) rc = up(&P->d_ws, nullptr, sizeof(double) * (size_t)E * nn * dim);
    P->d_wsp[0] = P->d_ws;
    if (!rc && P->npass == 2) rc = up(&P->d_wsp[1], nullptr, sizeof(double) * (size_t)E * nn * dim);
    if (!rc && which != 2) rc = up(&P->d_diag, nullptr, sizeof(double) * (size_t)N * dim);
    if (!rc && S && which != 2) {
        // the diagonal by class, once: the element entries into ws where a class
        // sums them (K, Kfs, K + Kfs), gathered like a product
        const unsigned ge = (unsigned)((E * nn + 255) / 256), gn = (unsigned)((N * dim + 255) / 256);
        const bool sums = ((P->drules | (P->drules >> 8) | (P->drules >> 16)) & 2u) != 0;
        hipStream_t st = ctx->stream;
        if (dim == 2) {
            if (sums)
                hipLaunchKernelGGL(k_sumfac_diag<2>, dim3(ge), dim3(256), 0, st, ngl, nn, E, P->d_tab, P->d_geoF,
                                   P->d_geoR, P->d_ws);
            hipLaunchKernelGGL(k_sumfac_diag_gather_cls<2>, dim3(gn), dim3(256), 0, st, N, P->drules, P->d_incp,
                               P->d_inc, P->d_cls, P->d_ws, P->d_diag);
        } else {
            if (sums)
                hipLaunchKernelGGL(k_sumfac_diag<3>, dim3(ge), dim3(256), 0, st, ngl, nn, E, P->d_tab, P->d_geoF,
                                   P->d_geoR, P->d_ws);
            hipLaunchKernelGGL(k_sumfac_diag_gather_cls<3>, dim3(gn), dim3(256), 0, st, N, P->drules, P->d_incp,
                               P->d_inc, P->d_cls, P->d_ws, P->d_diag);
        }
        hipError_t he = hipGetLastError();
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) rc = fail(KLE_ERR_DEVICE, "sum-factorised operator: diagonal kernels: %s", hipGetErrorString(he));
    }
    if (!rc && !S && which != 2) {
        // the diagonal, once: element entries into ws, gathered like a product
        const unsigned ge = (unsigned)((E * nn + 255) / 256), gn = (unsigned)((N * dim + 255) / 256);
        hipStream_t st = ctx->stream;
        if (dim == 2) {
            if (which == 0)
                hipLaunchKernelGGL(k_sumfac_diag<2>, dim3(ge), dim3(256), 0, st, ngl, nn, E, P->d_tab, P->d_geoF,
                                   P->d_geoR, P->d_ws);
            hipLaunchKernelGGL(k_sumfac_diag_gather<2>, dim3(gn), dim3(256), 0, st, N, which, P->d_incp, P->d_inc,
                               P->d_dir, P->d_ws, P->d_diag);
        } else {
            if (which == 0)
                hipLaunchKernelGGL(k_sumfac_diag<3>, dim3(ge), dim3(256), 0, st, ngl, nn, E, P->d_tab, P->d_geoF,
                                   P->d_geoR, P->d_ws);
            hipLaunchKernelGGL(k_sumfac_diag_gather<3>, dim3(gn), dim3(256), 0, st, N, which, P->d_incp, P->d_inc,
                               P->d_dir, P->d_ws, P->d_diag);
        }
        hipError_t he = hipGetLastError();
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) rc = fail(KLE_ERR_DEVICE, "sum-factorised operator: diagonal kernels: %s", hipGetErrorString(he));
    }
    if (rc) {
        kle_mat_destroy(A);
        return rc;
    }
    *out = A;
    return 0;
}

extern "C" int kle_mat_create_kle_sumfac(kle_ctx *ctx, kle_mesh *m, int which, kle_mat **out)
{
    KLE_ARG(ctx && m && out, "null arg");
    KLE_ARG(which >= 0 && which <= 2, "which must be 0 (K) or 1 (Krhs)");
    if (which == 2)
        return fail(KLE_ERR_SUP, "sum-factorised operator: Rw has its own call (kle_mat_create_rw_sumfac)");
    return sumfac_create(ctx, m, which, out);
}

extern "C" int kle_mat_create_rw_sumfac(kle_ctx *ctx, kle_mesh *m, kle_mat **out)
{
    KLE_ARG(ctx && m && out, "null arg");
    return sumfac_create(ctx, m, 2, out);
}

// The no-slip operators of any mesh, sum-factorised: NS_SPECS with
// k_sumfac_elem<D, LIST, CLS> (Rw, Rwfs: k_sumfac_rw) as the pass
extern "C" int kle_mat_create_ns_sumfac(kle_ctx *ctx, kle_mesh *m, int which, kle_mat **out)
{
    KLE_ARG(ctx && m && out, "null arg");
    KLE_ARG(which >= 0 && which <= 6, "which must be 0 (K), 1 (Krhs), 2 (Rw), 3 (Kfs), 4 (Krhsfs), 5 (Rwfs) or 6 (K + Kfs)");
    return sumfac_create(ctx, m, NS_SPECS[which].rw ? 2 : 0, out, which);
}
