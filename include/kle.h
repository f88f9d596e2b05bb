/*
 * kle.h -- C ABI of libkle.so, the MI355X-native KLE assembly + Krylov library.
 *
 * This is the drop-in boundary.  It replaces, for Pynama's hot path, the
 * petsc4py objects the reference creates and the Python element loops that
 * fill them (paths are under the reference's src/):
 *
 *   PETSc Mat (AIJ)  createAIJ/setValues/assemble/mult/diagonalScale
 *                      matrices/mat_fs.py:102-106,115-120,175-186,245-267
 *   PETSc Vec          createMPI/setValues/axpy/scale/dot/norm/...
 *                      matrices/mat_fs.py:228-236, cases/base_problem.py:129-154
 *   PETSc KSP/PC       KspSolver.createSolver / KleSolver.solve
 *                      solver/kle_solver.py:33-41,54-64
 *   MatFS.build element loops (buildFS, buildOperators)
 *                      matrices/mat_fs.py:131-201  -> kle_assemble_kle()
 *   DMPlex box mesh + FEM section numbering
 *                      domain/dmplex.py:31-49,193-196,382-388 -> kle_mesh_*
 *
 * Conventions (PETSc-like):
 *   - every function returns int: 0 = success, a KLE_ERR_* code otherwise;
 *     kle_last_error() returns a thread-local message for the last failure.
 *   - handles are opaque; plain pointers/sizes only, no torch types.
 *   - all device work is ordered on the context's HIP stream.
 *   - one process per GPU; ranks partition the mesh into slabs along the
 *     slowest lattice axis (z in 3-D, y in 2-D).  Collectives (halo exchange,
 *     Krylov dot products) go over RCCL inside the library.
 *   - handles are not thread-safe (same as PETSc objects).
 */
#ifndef KLE_H
#define KLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    KLE_OK = 0,
    KLE_ERR_ARG = 62,        /* PETSC_ERR_ARG_WRONG          */
    KLE_ERR_SIZ = 60,        /* PETSC_ERR_ARG_SIZ            */
    KLE_ERR_IDN = 61,        /* PETSC_ERR_ARG_IDN: an output vector that is also an input */
    KLE_ERR_OUTOFRANGE = 63, /* PETSC_ERR_ARG_OUTOFRANGE     */
    KLE_ERR_MEM = 55,        /* PETSC_ERR_MEM                */
    KLE_ERR_SUP = 56,        /* PETSC_ERR_SUP (not supported) */
    KLE_ERR_STATE = 73,      /* PETSC_ERR_ARG_WRONGSTATE     */
    KLE_ERR_DEVICE = 76,     /* HIP runtime failure          */
    KLE_ERR_COMM = 98,       /* RCCL failure                 */
    KLE_ERR_NEWNZ = 77       /* insertion outside the preallocated pattern */
};

/* KSP converged reasons (same numeric values as PETSc's KSPConvergedReason). */
enum {
    KLE_CONVERGED_RTOL = 2,
    KLE_CONVERGED_ATOL = 3,
    KLE_CONVERGED_ITS = 4,
    KLE_DIVERGED_ITS = -3,
    KLE_DIVERGED_DTOL = -4,
    KLE_DIVERGED_BREAKDOWN = -5,
    KLE_DIVERGED_INDEFINITE_MAT = -8,
    KLE_DIVERGED_NANORINF = -9,
    KLE_CONVERGED_ITERATING = 0
};

typedef struct kle_ctx kle_ctx;
typedef struct kle_mesh kle_mesh;
typedef struct kle_vec kle_vec;
typedef struct kle_mat kle_mat;
typedef struct kle_ksp kle_ksp;

const char *kle_last_error(void);
/* Tuning keys (kle_set_tuning, kle_get_tuning), for in-process A/B
 * measurements (tools/cg_ab.py).  One entry per key: its values with the
 * default marked *, then when the library reads it -- [call] at every product
 * or solve, [build] when a matrix's SpMV storage is built, [assembly] by
 * kle_assemble_kle and its kin, [create] when a matrix or KSP is created.
 * Except where an entry says otherwise every value gives bitwise the same
 * results; the symmetric-storage keys give the same product to rounding.
 *
 * 3x3 SpMV (full storage)
 *   "spmv_waves"          0* auto (8 from 64000 node rows, else 4), 4, 8 [call]: rows per SpMV workgroup of
 *                         3x3 chunked matrices
 *   "spmv_x_lds"          0, 1* [call]: structured 3x3 rows at 8 waves stage x in LDS
 *   "spmv_xcd_chunk"      0 .. 4096, 16* [call]: consecutive row blocks per XCD run; 0 round-robin
 *   "spmv_dyn_lds"        -1* auto, 0 .. 65536 [call]: unused LDS bytes per SpMV workgroup while side-stream
 *                         work runs (caps the workgroups per CU)
 *   "spmv_dict"           0, 1* [call]: unstructured 3x3 rows at 8 waves read x through per-group column
 *                         dictionaries
 *   "spmv_dict_min_rows"  >= 0, 64000* [create]: node rows from which matrices get dictionaries
 *
 * Symmetric storage and its 128-row tiles
 *   "spmv_sym"            0, 1* [call, assembly]: matrices holding symmetric storage run the symmetric
 *                         SpMV, and kle_assemble_kle builds that storage; 0 the full storage
 *   "spmv_sym_min_rows"   >= 0, 40000* [assembly]: node rows per rank from which kle_assemble_kle gives K
 *                         symmetric storage
 *   "spmv_sym_det"        0, 1* [call, build]: the transposed adds as exact fixed-point sums, y bitwise
 *                         reproducible; 0 fp64 LDS atomics, reproducible to rounding (and no bricks)
 *   "spmv_sym_waves"      0* auto, 8, 16 [call]: waves per workgroup of the box tile kernel
 *   "spmv_sym_tz"         0* auto (8 x 4 x 4-row tiles where two 8-wave workgroups fit a CU), 2 (8 x 8 x 2),
 *                         4 (8 x 4 x 4) [build]
 *   "spmv_sym_tile64"     0* auto, 1, 2 [build]: 8 x 2 x 4-row tiles (64 rows) -- 0 below
 *                         "spmv_sym_tile64_max" 128-row tiles, 1 wherever two workgroups fit a CU, 2 never
 *   "spmv_sym_tile64_max" >= 0, 640* [build]: the 128-row tile count below which "spmv_sym_tile64" 0
 *                         takes the 64-row tiles
 *   "spmv_sym_xcd"        0* .. 4096 [call]: the box tile kernel's runs of this many consecutive tiles per
 *                         XCD; 0 round-robin
 *   "spmv_sym_ovl_b"      0 .. 100, 50* [call]: N > 1, box symmetric SpMV with halo overlap: the percentage
 *                         of the interior tiles run beside the reverse halo, the rest beside the forward halo
 *   "spmv_sym_early"      0*, 1 [call]: the box tile kernel loads its first items before x is in LDS
 *   "spmv_sym_align"      0*, 1 [build]: partial slots aligned to 128-B lines
 *   "spmv_sym_stpol"      0* plain, 1 nontemporal, 2 sc1, 3 sc0 sc1 [call]: the box kernel's partial stores
 *
 * Box bricks (the box K of one rank)
 *   "spmv_sym_brick"      0, 1* [build]: the box K on bricks -- one 16-wave workgroup per CU, the brick
 *                         region's x and exact sums in LDS for the whole value stream; 0 the 128-row tiles
 *   "spmv_brick_max"      >= 0, 0* planned [build]: at most this many bricks
 *   "spmv_brick_rounds"   1* .. 4 [build]: at most this many bricks per CU
 *   "spmv_brick_split"    >= 0, 0* planned [build]: force nbx + 100 nby + 10000 nbz bricks
 *   "spmv_brick_pair"     0, 1* [build]: rows in units of two whose last partial 64-block passes share one
 *                         item
 *   "spmv_brick_singles"  0, 1* [build]: rows of one stored block -- the Dirichlet rows and the free rows at
 *                         the far corner of their box -- formed by the gather instead of as items of the
 *                         bricks
 *   "spmv_brick_compact"  0, 1* [build]: the brick value stream of a K that stores every analytically zero
 *                         entry as +0.0 -- checked on the device when the storage is built -- holds the
 *                         other entries alone, 3, 5 or 9 per block; 0 the full blocks.  The product is the
 *                         same matrix's either way: the entries left out are exact zeros
 *   "spmv_brick_dedup"    0, 1* [build]: bricked rows whose value streams are bitwise equal -- a box-mesh K
 *                         repeats a few distinct rows over the lattice -- are stored once; proposed by a
 *                         hash, decided by comparison, kept only where it saves at least half of the
 *                         bricked bytes and fits the descriptors' 1 GiB; the product is bitwise the same;
 *                         0 every row's own stream.  On the full layout the units (pairs of rows) whose rows
 *                         share boxes and values are then ordered class by class and handed to the waves in
 *                         runs of up to 4: an item's nine values and block positions are formed once per run
 *                         (kle_mat_get_brick_runs; taken where at most 3/4 of the items then load their values)
 *   "spmv_brick_dedup_full" 0, 1* [build]: a K whose rows are shared keeps the full 9-entry blocks -- read
 *                         from the caches, the kernel is bound by its instructions and the compact stream's
 *                         offsets cost more than its bytes save; the full layout is built first and the
 *                         compact one only where the sharing is not taken; 0 the compact stream first
 *   "spmv_brick_dedup_nt" 0* plain cached, 1 nontemporal as the full stream's [call]: value loads of a
 *                         deduplicated K
 *   "spmv_gather_wps"     0* by the runs per slice, 1, 2, 4 [call]: the run-mask gather's waves per 64-row
 *                         slice
 *
 * Graph bricks and groups (the symmetric storage of an unstructured K)
 *   "spmv_gsym_brick"     0, 1* [build]: graph K on graph bricks, whole rounds per CU; 0 the row groups
 *   "spmv_gsym_rows"      8, 16, 32, 64*, 128 [build]: rows per group
 *   "spmv_gsym_waves"     0* auto (16 for 64-row groups, else 8), 8, 16 [build]
 *   "spmv_gsym_split"     >= 0, 0* auto [build]: the largest dictionary of the first of its two launches
 *   "spmv_gsym_stpol"     0 plain, 1 nontemporal, 2* sc1, 3 sc0 sc1 [call]: the graph kernel's partial stores
 *
 * Assembly (these change stored values: not performance knobs)
 *   "asm_box_uniform"     0, 1* [assembly]: on a box mesh every cell adds the blocks of global element 0's
 *                         K_e and Rw_e into the free-slip K, Krhs and Rw, so rows that are translates of
 *                         each other are the same bits and the brick SpMV stores them once; the values
 *                         move by coordinate rounding, <= 1e-12 of the largest entry; 0 each cell's own
 *                         matrix
 *   "asm_box_zeros"       0, 1* [assembly]: an A/B and diagnosis switch: the free-slip K of a 3-D
 *                         kle_mesh_create_box mesh stores its analytically zero block entries as +0.0 --
 *                         entry (a, b), a != b, of the block between two nodes that share lattice
 *                         coordinate a or b on a plane that is not a domain boundary plane; 0 the
 *                         assembly's rounding noise there, a few 1e-16 of max|K|.  Every other entry, the
 *                         pattern, Krhs, Rw, the operators, the no-slip matrices, 2-D and unstructured
 *                         meshes are the same bits for both values
 *
 * CG
 *   "ksp_refine"          0 .. 8, 2* [create]: correction solves of new KSPs (kle_ksp_set_corrections);
 *                         0 PETSc's plain stop -- KLE_KSP_REFINE.  It changes what a solve returns
 *   "upd_preload"         0, 1* [call]: CG update kernels load their first element and the stage inputs
 *                         before the prologue
 *   "upd_nt"              0 off, 1 on, 2* auto = from 2M local entries [call]: single-reduction CG update:
 *                         every vector but u loaded and stored nontemporal, so u stays in the Infinity
 *                         Cache for the SpMV
 *   "upd_unroll"          1*, 2 [call]: elements per pass of the CG update kernel (2 only with "upd_preload" 1)
 *   "ksp_pipe_gather"     0, 1* [call]: box bricks: the pipelined CG's update gathers the split product
 *                         itself; 0 a separate gather launch
 *   "ksp_sr_gather"       0 never, 1* from 2^17 node rows, 2 always [call]: the same for the
 *                         single-reduction CG at one rank, the bricks forming (A u, u)
 *
 * Element-wise operators
 *   "elem_ghost_rows"     0, 1* [call]: element-wise K, Krhs, Rw on several ranks: the ghost layer's GEMM
 *                         over the row groups holding its top-plane rows alone; 0 every row group
 *
 * Debug and test hooks (not performance knobs)
 *   "ipc_sentinel"        0*, 1 [call]: IPC transport debug mode: consumed mailbox slots overwritten with
 *                         NaN before the ack
 *   "ksp_corr_fault"      0*, 1 [call]: test hook: correction solves that end in NaN
 *
 * Not pure performance knobs: "ksp_corr_fault" and "ipc_sentinel" (hooks), "asm_box_zeros" and
 * "asm_box_uniform" (stored values), "ksp_refine" (what a solve returns).  Every other value gives correct
 * results.  The timing probes of the symmetric SpMV (keys spmv_sym_probe, spmv_sym_probe_ts: wrong results
 * on purpose) exist only in the tools/ probe build, `make -C pynama_amd/csrc probe`. */
int kle_set_tuning(const char *key, int value);
int kle_get_tuning(const char *key, int *value);
int kle_version(void);

/* ---------------------------------------------------------------- context */
/* 128-byte RCCL unique id, produced on rank 0 and broadcast by the caller. */
int kle_get_unique_id(unsigned char out[128]);
/* device: HIP ordinal; nranks==1 needs no unique id (pass NULL). */
int kle_ctx_create(int device, int rank, int nranks, const unsigned char *unique_id,
                   kle_ctx **out);
/* Host-staged transport (testing / debugging): the same distributed code
 * paths with the collectives delegated to caller callbacks on host buffers
 * (e.g. gloo), so several ranks can share one GPU.  Production runs use RCCL.
 *   allreduce: in-place sum of n doubles over all ranks.
 *   halo: send n_send_lo doubles to lo_rank and n_send_hi to hi_rank, receive
 *         n_recv_lo from lo_rank and n_recv_hi from hi_rank (ranks < 0: none).
 *   exchange: general halo of graph-partitioned meshes: for peer k send
 *         send_cnt[k] doubles (packed back to back in `send`, peer order) and
 *         receive recv_cnt[k] (packed in `recv`); may be NULL when no mesh
 *         with a graph partition is used. */
typedef struct {
    int (*allreduce)(double *buf, int n, void *user);
    int (*halo)(const double *send_lo, int64_t n_send_lo, int lo_rank, const double *send_hi,
                int64_t n_send_hi, int hi_rank, double *recv_lo, int64_t n_recv_lo,
                double *recv_hi, int64_t n_recv_hi, void *user);
    void *user;
    int (*exchange)(int npeers, const int *peers, const double *send, const int64_t *send_cnt,
                    double *recv, const int64_t *recv_cnt, void *user);
} kle_host_comm;
int kle_ctx_create_host_comm(int device, int rank, int nranks, const kle_host_comm *comm,
                             kle_ctx **out);
/* Device-to-device transport for a host-comm context (KLE_TRANSPORT=ipc;
 * collective): every rank exports one mailbox (hipIpcGetMemHandle, handles
 * exchanged over the host callbacks) and maps the others'; the slab halos,
 * the symmetric SpMV's reverse halo and the allreduces then run as
 * hipMemcpyAsync copies into the peers' mailboxes with stream wait/write-value
 * signals (no host staging, no RCCL kernels on the SpMV's CUs; the allreduce
 * sums the ranks' slots in rank order, the same bits on every rank).  Graph-
 * partition halos keep the host path.  KLE_ERR_COMM when any rank cannot
 * export or map (then no rank switches). */
int kle_ctx_enable_ipc(kle_ctx *ctx);
int kle_ctx_destroy(kle_ctx *ctx);
int kle_ctx_synchronize(kle_ctx *ctx);
int kle_ctx_barrier(kle_ctx *ctx); /* device-side RCCL barrier + stream sync */
/* Diagnostics (no reference counterpart): the HIP ordinal, its PCI bus id
 * (may be NULL) and the transport: 0 single rank, 1 RCCL, 2 host-staged,
 * 3 IPC mailboxes (kle_ctx_enable_ipc). */
int kle_ctx_get_device(kle_ctx *ctx, int *device, char *pci_bus_id, int len, int *transport);
/* The context's HIP stream (a hipStream_t), on which all device work is
 * ordered: for events recorded around library calls (tools/elem_ab.py) and
 * for interop.  No reference counterpart. */
int kle_ctx_get_stream(kle_ctx *ctx, void **stream);
/* What the RCCL communicator itself reports (ncclCommCount /
 * ncclCommUserRank; the MPI communicator of DMPlex.distribute, dmplex.py:21,
 * and of KSPSolve's reductions, kle_solver.py:35): *count = 0, *rank = -1
 * when the context has no RCCL communicator (one rank, host or IPC transport). */
int kle_ctx_get_comm_info(kle_ctx *ctx, int *count, int *rank);
/* Diagnostic, host only (no device, no reference counterpart): the brick
 * plan of the symmetric SpMV for an Lx x Ly x Lz box lattice of p-node
 * elements (dirichlet: boundary rows the diagonal alone) on ncu CUs, at
 * most `rounds` bricks per CU (split: forced counts nbx + 100 nby + 10000 nbz, 0
 * planned).  info[5]: bricks, bricks along x / y / z, LDS bytes; stats[6]:
 * largest brick's bytes over the mean, region entries per row, stored blocks,
 * modelled microseconds, 64-lane items streamed, share of their lanes that
 * carry a block. */
int kle_brick_plan_box(int Lx, int Ly, int Lz, int p, int dirichlet, int ncu, int rounds, int split, int *info,
                       double *stats);
/* Diagnostic, host only: that plan with its value offsets rewritten as the
 * row dedup of the brick SpMV ("spmv_brick_dedup") rewrites them -- rows with
 * equal packed boxes share the first one's values, every brick's base is 0 --
 * and checked against the unique array by the validator every brick product
 * passes before its first launch.  shift > 0 moves the last row's offset
 * that many 16-double units on, out of the array: refused (KLE_ERR_SUP).
 * shift -1 gives the last brick a value base of its own inside a longer
 * array: refused too (shared values have one common base, 0).
 * out[3]: rows in bricks, rows stored, doubles of the unique array. */
int kle_brick_plan_box_shared(int Lx, int Ly, int Lz, int p, int dirichlet, int ncu, int shift, long long *out);
/* Diagnostic, host only: the plan under the forced split `split` (as
 * "spmv_brick_split"; 0 planned) with that rewrite, then its units grouped
 * into runs of at most G units of one class as the brick SpMV groups them on a
 * shared full-layout K (a class: the units whose two rows have the same packed
 * boxes and value offsets -- they stream identical items, so a wave loads an
 * item's values once for the whole run), checked by the same validator: every
 * run inside its brick's units, 1 <= count <= G, every unit in exactly one
 * run, all units of a run of one class.  corrupt 1 moves a unit into a run of
 * another class, 2 lengthens the first run by one: both refused (KLE_ERR_SUP).
 * out[6]: units, classes summed over the bricks, runs, 64-lane items, items
 * whose values are loaded, units of the largest run. */
int kle_brick_plan_box_runs(int Lx, int Ly, int Lz, int p, int dirichlet, int ncu, int split, int G, int corrupt,
                            long long *out);
/* Per-kernel HIP-event timing of the hot kernels (SpMV, CG updates). */
int kle_ctx_set_profiling(kle_ctx *ctx, int on);
/* Time only the launches tagged `name` ("spmv", "dot", "cg_update", "reduce",
 * "halo", "allreduce"); NULL or "" times all of them. */
int kle_ctx_set_profiling_filter(kle_ctx *ctx, const char *name);
/* Time only one launch in `every` of the profiled tags (1 = all): keeps the
 * event overhead out of a timed loop while still sampling it live. */
int kle_ctx_set_profiling_sample(kle_ctx *c, int every);
/* name: "spmv" | "cg_update" | "p_update" | "reduce" | "halo" | "allreduce" */
int kle_ctx_get_kernel_stats(kle_ctx *ctx, const char *name, int64_t *count, double *total_ms);
int kle_ctx_reset_kernel_stats(kle_ctx *ctx);

/* ------------------------------------------------------------------- mesh */
/* Structured box mesh (replaces BoxDom.create + DMPlexDom.setFemIndexing,
 * dmplex.py:31-49,382-388).  Host-only: usable without a GPU.  Node ids are
 * lattice-lexicographic (x fastest); cells x-fastest; element-local nodes in
 * tensor order. */
int kle_mesh_create_box(int dim, const int64_t nelem[3], const double lower[3],
                        const double upper[3], int ngl, int rank, int nranks, kle_mesh **out);
int kle_mesh_destroy(kle_mesh *m);
/* Unstructured quad (2-D) / hex (3-D) mesh (replaces GmshDom.create +
 * DMPlexDistribute + setFemIndexing, dmplex.py:18-49,390-395; entity
 * orientation rules indices.py:70-96).  vxyz: [nverts][3]; cells:
 * [ncells][2^dim] vertex indices in Gmsh order (quad counter-clockwise, hex
 * bottom 0-3 then 4-7 above them), cell ids = row order (the ADD order);
 * facets: [nfacets][2^(dim-1)] boundary faces with their Face Sets value
 * (tag t >= 1 -> face bit t-1, the reference's name order: dmplex.py:27-30,
 * 175-178).  Cells are partitioned by kle_set_partitioner's method; node ids
 * are global, owned ranges contiguous per rank (see kle_umesh.cpp).  Fails
 * with KLE_ERR_ARG for inverted cells, ranks without nodes, or slabs too thin
 * for the two-neighbour halo. */
int kle_mesh_create_unstructured(int dim, int ngl, int64_t nverts, const double *vxyz, int64_t ncells,
                                 const int64_t *cells, int64_t nfacets, const int64_t *facets,
                                 const int *facet_tags, int rank, int nranks, kle_mesh **out);
/* Gmsh MSH 4.1 ASCII file (GmshDom.create -> DMPlexCreateFromFile). */
int kle_mesh_create_gmsh(const char *path, int ngl, int rank, int nranks, kle_mesh **out);
/* Partitioner of the unstructured meshes created afterwards (the role of
 * DMPlexDistribute's Chaco partitioner, dmplex.py:21): 0 (default) inertial
 * recursive bisection of the cells -- general partitions, any number of
 * neighbours per rank, index-list halos; 1 slabs along the longest axis
 * (two-neighbour halo in contiguous ranges). */
int kle_set_partitioner(int method);
int kle_get_partitioner(void);
/* Halo of a rank: npeers neighbours, per peer its rank, the ghost nodes
 * received and the owned nodes sent; send_list (optional, sum of send_nodes
 * entries) holds the owned-local node indices sent, peer by peer. */
int kle_mesh_get_peers(const kle_mesh *m, int *npeers, int *ranks, int64_t *recv_nodes, int64_t *send_nodes,
                       int64_t *send_list);
/* Global node id of every ext (owned + ghost) node, in ext order. */
int kle_mesh_get_ext_gids(const kle_mesh *m, int64_t *gids);
/* Global cell ids of the local (owned + ghost) elements, ascending. */
int kle_mesh_get_elements(const kle_mesh *m, int64_t *ids);

typedef struct {
    int dim, ngl, rank, nranks;
    int64_t nelem[3];
    int64_t lattice[3];     /* nodes per axis                                */
    int64_t n_nodes;        /* global                                        */
    int64_t n_elems;        /* global                                        */
    int64_t node_begin;     /* owned node range [node_begin, node_end)       */
    int64_t node_end;
    int64_t ext_begin;      /* owned + ghost node range [ext_begin, ext_end) */
    int64_t ext_end;
    int64_t elem_begin;     /* local (owned + ghost) element range           */
    int64_t elem_end;
    int kind;               /* 0 structured box, 1 unstructured              */
    int axis;               /* partition axis                                */
} kle_mesh_info;

int kle_mesh_get_info(const kle_mesh *m, kle_mesh_info *info);
/* element->global node ids for local elements, tensor order [elem][ngl^dim]. */
int kle_mesh_get_conn(const kle_mesh *m, int64_t *conn);
/* cell corners in DMPlex closure order [elem][2^dim][dim] (dmplex.py:93-100). */
int kle_mesh_get_corners(const kle_mesh *m, double *xyz);
/* coordinates of the owned nodes [node][dim] (computeFullCoordinates). */
int kle_mesh_get_coords(const kle_mesh *m, double *xyz);
/* Boundary nodes of named faces: face bit f follows the reference's naming
 * (dmplex.py:27-30): 3-D 0 back(z-) 1 front(z+) 2 down(y-) 3 up(y+) 4 right(x+)
 * 5 left(x-); 2-D 0 down 1 right 2 up 3 left.  Fills the owned boundary
 * nodes (sorted) and returns their count in *n (pass nodes=NULL to count). */
int kle_mesh_face_nodes(const kle_mesh *m, unsigned face_mask, int64_t *nodes, int64_t *n);
/* Dirichlet (free-slip) node set: faces by mask, or explicit global ids. */
int kle_mesh_set_dirichlet_faces(kle_mesh *m, unsigned face_mask);
int kle_mesh_set_dirichlet_nodes(kle_mesh *m, const int64_t *nodes, int64_t n);
/* No-slip walls (BoundaryConditions.getNoSlipTangDofs / getNoSlipNormalDofs,
 * boundary_conditions.py:214-241): global velocity DoF ids; a DoF in both
 * lists is normal (mat_ns.py:60-62).  Their nodes become the fixed nodes. */
int kle_mesh_set_noslip_dofs(kle_mesh *m, const int64_t *tang, int64_t nt, const int64_t *normal, int64_t nn);
/* Same, from the no-slip faces (face bits as kle_mesh_set_dirichlet_faces) in
 * the order the configuration lists them (that order decides corner DoFs). */
int kle_mesh_set_noslip_faces(kle_mesh *m, const int *faces, int nfaces);
/* Symbolic node-block pattern (host).  which: 0 K, 1 Krhs, 2 Rw, 3 operators
 * (Curl/SrT/DivSrT: every node x every node sharing a cell).
 * row_ptr[n_owned+1] (block offsets, unpadded) and col[] (global node ids). */
int kle_mesh_pattern_size(const kle_mesh *m, int which, int64_t *nblocks);
int kle_mesh_pattern(const kle_mesh *m, int which, int64_t *row_ptr, int64_t *cols);
/* Halo plan of this rank (node counts): ghosts received from below/above,
 * owned nodes sent to the lower/upper neighbour, neighbour ranks (-1: none). */
int kle_mesh_halo(const kle_mesh *m, int64_t *lo_count, int64_t *hi_count, int64_t *send_lo,
                  int64_t *send_hi, int *lo_rank, int *hi_rank);

/* -------------------------------------------------------------------- vec */
/* Mesh vector with bs components per node, ghosted over the ext range. */
int kle_vec_create_mesh(kle_ctx *ctx, const kle_mesh *m, int bs, kle_vec **out);
/* Plain distributed vector (no ghosts). */
int kle_vec_create(kle_ctx *ctx, int64_t n_local, int64_t n_global, kle_vec **out);
int kle_vec_duplicate(const kle_vec *v, kle_vec **out);
int kle_vec_destroy(kle_vec *v);
int kle_vec_get_sizes(const kle_vec *v, int64_t *n_local, int64_t *n_global);
int kle_vec_get_ownership_range(const kle_vec *v, int64_t *lo, int64_t *hi);
int kle_vec_set(kle_vec *v, double alpha);
/* Aliasing: axpy, aypx and waxpy return KLE_ERR_IDN, with the vectors
 * unchanged, when the output is also an input (VecAXPY, VecAYPX, VecWAXPY);
 * pointwise_mult takes w == x, w == y and w == x == y (VecPointwiseMult). */
int kle_vec_copy(const kle_vec *x, kle_vec *y);                 /* y = x          */
int kle_vec_axpy(kle_vec *y, double alpha, const kle_vec *x);   /* y += a x       */
int kle_vec_aypx(kle_vec *y, double beta, const kle_vec *x);    /* y = x + b y    */
int kle_vec_waxpy(kle_vec *w, double alpha, const kle_vec *x, const kle_vec *y); /* w = a x + y */
int kle_vec_scale(kle_vec *v, double alpha);
int kle_vec_pointwise_mult(kle_vec *w, const kle_vec *x, const kle_vec *y);
/* out[node] = v v^T of the dim-vector at each node, components xx,xy,yy
 * (2-D) or xx,xy,yy,yz,zz,zx (3-D): BaseProblem.computeVtensV
 * (base_problem.py:138-154). */
int kle_vec_tensor_square(const kle_vec *v, int dim, kle_vec *out);
/* 1 / v_i; an entry that compares equal to 0 stays as it is (VecReciprocal). */
int kle_vec_reciprocal(kle_vec *v);
int kle_vec_dot(const kle_vec *x, const kle_vec *y, double *out);
/* The 2-norm to a few roundings whenever it is representable: sqrt of the sum
 * of squares while that sum is finite and at least 2^-969 (no extra launch or
 * synchronisation on that path), else a max-abs pass and the sum of squares of
 * the entries scaled by a power of two (entries near 2^+-600 do not give inf
 * or 0).  NaN for a NaN entry, inf for an infinite one, 0.0 for all zeros. */
int kle_vec_norm2(const kle_vec *x, double *out);
/* Host <-> device.  Indices are GLOBAL; only owned entries may be set
 * (KLE_ERR_OUTOFRANGE otherwise, before anything is written).
 * addv: 0 INSERT_VALUES (an index given more than once takes the last value
 * given), 1 ADD_VALUES (applied in list order).
 * get_values also reads the ghost entries of a mesh vector, as they stand
 * since the last ghost update: on slab partitions the neighbouring index
 * ranges, on graph partitions the entries of the ghost nodes
 * (kle_mesh_get_ext_gids); any other index is KLE_ERR_OUTOFRANGE. */
int kle_vec_set_values(kle_vec *v, int64_t n, const int64_t *idx, const double *vals, int addv);
int kle_vec_get_values(const kle_vec *v, int64_t n, const int64_t *idx, double *vals);
int kle_vec_get_array(const kle_vec *v, double *host_local);     /* owned part */
int kle_vec_set_array(kle_vec *v, const double *host_local);
/* petsc4py getArray()/restoreArray pair: kle_vec_get_array copies the owned
 * part out, kle_vec_restore_array writes a (modified) host copy back. */
int kle_vec_restore_array(kle_vec *v, const double *host_local);
/* VecAssemblyBegin/End: set_values writes owned entries immediately, so
 * assembly only completes the pending device work of the vector's stream. */
int kle_vec_assemble(kle_vec *v);
int kle_vec_ghost_update(kle_vec *v);                             /* halo fill  */
/* raw device pointer to the owned part (for zero-copy interop). */
int kle_vec_device_ptr(const kle_vec *v, double **dptr);

/* -------------------------------------------------------------------- mat */
/* Batch device assembly of the KLE system: replaces MatFS.build / buildFS
 * (mat_fs.py:131-192).  Produces node-block matrices K (dim x dim blocks),
 * Krhs (dim x dim) and Rw (dim x dim_w) with PETSc's pattern and ADD order. */
int kle_assemble_kle(kle_ctx *ctx, kle_mesh *m, kle_mat **K, kle_mat **Krhs, kle_mat **Rw);
/* Element matrices of local element e in tensor order (parity tests):
 * K_e [dim n][dim n], Rw_e [dim n][dim_w n] (row-major, n = ngl^dim). */
int kle_element_kle(kle_ctx *ctx, kle_mesh *m, int64_t e, double *Ke, double *Rwe);
/* No-slip assembly (replaces MatNS.build / buildNS, mat_ns.py:47-161):
 * K, Krhs, Rw as kle_assemble_kle on the no-slip nodes, Rd (free rows x
 * cell nodes), plus Kfs, Krhsfs, Rwfs, Rdfs with PETSc's DoF-level patterns,
 * and Ksum = K + Kfs (the operator of KleSolver.solverFS, kle_solver.py:22-28)
 * assembled directly. */
int kle_assemble_ns(kle_ctx *ctx, kle_mesh *m, kle_mat **K, kle_mat **Krhs, kle_mat **Rw, kle_mat **Rd,
                    kle_mat **Kfs, kle_mat **Krhsfs, kle_mat **Rwfs, kle_mat **Rdfs, kle_mat **Ksum);
/* Operators (replaces MatFS.buildOperators + Operators.setValues/assembleAll,
 * mat_fs.py:194-271, with Spectral.getElemKLEOperators spectral.py:162-228):
 * Curl [dim_w N x dim N], SrT [dim_s N x dim N], DivSrT [dim N x dim_s N],
 * each already scaled by the inverse lumped nodal weight.  Node-block CSR on
 * the full node adjacency (pattern 3), explicit zeros kept as PETSc does. */
int kle_assemble_operators(kle_ctx *ctx, kle_mesh *m, kle_mat **Curl, kle_mat **SrT, kle_mat **DivSrT);

/* Element-wise operator of a uniform box mesh: y = A x formed from the one
 * element matrix of the mesh, no assembled values.  which: 0 K (free rows x
 * free columns + unit Dirichlet diagonal), 1 Krhs (free rows x Dirichlet
 * columns, negated, + unit Dirichlet diagonal), 2 Rw (free rows x every
 * vorticity column of their elements, no mask and no negation; Dirichlet rows
 * hold no entry, y_i = 0 exactly; rows dim N by columns dim_w N, dim_w = 1 in
 * 2-D and 3 in 3-D, blocks dim x dim_w, from the rectangular Rw_e0 of the same
 * element kernel launch): the same operators
 * kle_assemble_kle assembles (MatFS.buildFS, mat_fs.py:150-190).  With all
 * three, b = Rw w + Krhs u_bc and K u = b need no assembly at all
 * (MatFS.build(kleType="element"), -kle_mat_type element).
 * kle_mesh_create_box makes every element the same brick, so K u = sum_e
 * S_e^T K_e0 S_e u with K_e0 the matrix of global element 0 (from the
 * assembly's own element kernel): one FP64 MFMA GEMM K_e0 x [gathered element
 * vectors] and a gather per node in ascending element order -- bitwise
 * repeatable, and equal to the assembled product to rounding plus the spread
 * of the element matrices over the mesh (coordinate rounding, ~1e-15).
 * Memory: K_e0, the connectivity and incidence tables, one Dirichlet flag per
 * node and E * dim * ngl^dim doubles of element results; nothing of nnz(K).
 * Each operator owns its tables and workspace; nothing is shared between them.
 * The result is a kle_mat of format 2 ("elem").  It supports kle_mat_mult,
 * kle_mat_mult_add, kle_mat_get_diagonal, the size / local-size / ownership
 * getters, kle_mat_get_info (nz_used = 0: no entry is stored),
 * kle_mat_spmv_bytes, kle_mat_spmv_kernel, kle_mat_destroy and
 * kle_ksp_set_operators with cg (classic and single reduction: the generic
 * paths), pipecg or gmres and PC none or jacobi, and
 * kle_mat_time_local_spmv (this rank's element launches and its gather, no
 * halo).  Calls that need stored values return KLE_ERR_SUP: set_values,
 * assemble, axpy, diagonal_scale, get_row, get_csr, get_csr_size,
 * convert_aij, duplicate, set_symmetric, move_values, PC lu.  Rw also refuses
 * kle_mat_get_diagonal
 * (KLE_ERR_SUP), and kle_ksp_set_operators refuses a non-square operator
 * (the 2-D Rw) before anything is launched.
 * Several ranks (the mesh's slab partition must be the context's): owner
 * computes.  The tables hold ext-local node ids over every element touching
 * an owned node (one ghost layer below, the own layers, of which the top one
 * reads the upper ghost plane); x is a ghosted mesh vector (kle_vec_create_mesh)
 * read through its allocation after one forward halo, which with halo overlap
 * on (kle_mat_set_halo_overlap, the default) runs on the comm stream beside
 * the interior elements; the gather, the Dirichlet flags, kle_mat_get_diagonal
 * and kle_mat_copy_dirichlet_rows cover the owned rows, which are the one-rank
 * product's bit for bit.  The 32-bit table limits apply to the local sizes.
 * Needs a box mesh with its Dirichlet set, 2-D or 3-D; KLE_ERR_SUP for
 * unstructured meshes, no-slip meshes and a mesh whose nranks is not the
 * context's. */
int kle_mat_create_kle_element(kle_ctx *ctx, kle_mesh *m, int which, kle_mat **out);
/* Sum-factorised element-wise K (which 0) or Krhs (which 1) of any mesh, kind
 * 0 (box) or kind 1 (unstructured), 2-D or 3-D, ngl 2..8, with its Dirichlet
 * set, on one rank or on the parts of a partition (below): no stored values
 * and no element matrix.  The factored form of
 * the element matrix,
 *     K_e(la, mb) = d_ab G_lm + a_d D_ab(l,m) + a_w (d_ab tr D(l,m) - D_ba(l,m)),
 *     G_lm = sum_full c_q grad N_l . grad N_m,  D_ab(l,m) = sum_red c_q d_a N_l d_b N_m,
 * applied to a vector is a quadrature-point evaluation with per-point
 * geometry: with (grad u)_ab = d_b u^a at the point,
 *     (K_e u)_l^a =  sum_{q in full} c_q sum_b d_b N_l(q) (grad u)_ab(q)
 *                  + sum_{q in red}  c_q sum_b d_b N_l(q) T_ab(q),
 *     T = a_d (div u) I + a_w (grad u - grad u^T),
 * and both sums factorise into 1-D passes with the h / dh tables of the rules
 * (full: GLL(ngl) for ngl > 3, else Gauss(ngl); reduced: Gauss(ngl - 1)).
 * k_sumfac_elem gathers a batch of whole elements' x through the connectivity
 * into LDS (mask folded in as -1: K drops the Dirichlet columns, Krhs keeps
 * only them; a dropped entry of x is never read, so an Inf or NaN there
 * reaches no result), runs the passes, the point stage (inv J, flux, inv J^T)
 * and the transposed passes for the full and then the reduced rule and stores
 * the element results (negated for Krhs); k_sumfac_gather sums a node's
 * incidence entries -- a CSR list, a node may lie in any number of elements --
 * in ascending element order; Dirichlet rows give y_i = x_i.  No atomics: the
 * same input gives the same bits.  c_q and inv J are read from two tables
 * [e][q][1 + dim^2] filled at creation by the assembly's geometry kernel from
 * the mesh's own corners.
 * Memory: the two geometry tables (8 E (ngl^dim + (ngl-1)^dim) (1 + dim^2)
 * bytes), E dim ngl^dim doubles of element results, the connectivity and the
 * incidence list (4 bytes per element node each), the diagonal (dim N
 * doubles, formed once at creation; 1 on Dirichlet rows, 0 on the free rows of
 * Krhs) and one flag per node.
 * The result is a kle_mat of format 2 ("elem") with the call surface of
 * kle_mat_create_kle_element's K and Krhs: kle_mat_mult, kle_mat_mult_add,
 * kle_mat_get_diagonal, the size and ownership getters, kle_mat_get_info
 * (nz_used 0), kle_mat_spmv_bytes, kle_mat_spmv_kernel
 * ("k_sumfac_elem<D>+k_sumfac_gather<D>"), kle_mat_time_local_spmv and
 * kle_ksp_set_operators with cg (classic and single reduction: the generic
 * paths), pipecg or gmres and PC none or jacobi.  Calls that need stored
 * values, and kle_mat_copy_dirichlet_rows, return KLE_ERR_SUP.
 * KLE_ERR_SUP also for which 2 (Rw: kle_mat_create_rw_sumfac), no-slip meshes
 * (their operators: kle_mat_create_ns_sumfac) and a mesh whose nranks is not
 * the context's; KLE_ERR_ARG for any other
 * which.  Every table index is checked on the host before upload
 * (connectivity inside the ext range, incidence consistent with it and
 * ascending, the element lists disjoint, covering and true to their kind,
 * E ngl^dim and dim times the ext nodes below 2^31): a bad table is an error
 * code, never a launch.
 * Several ranks (m->nranks == ctx->nranks > 1; box slabs, Gmsh slab and
 * inertial partitions): a rank's local elements are every cell touching an
 * owned node, ascending global cell id.  The connectivity holds ext-local node
 * ids over all of them, masked by the Dirichlet flags of the ext range (a
 * ghost Dirichlet column is dropped like an owned one).  x is a ghosted mesh
 * vector (kle_vec_create_mesh; a graph partition's carries the mesh's halo
 * plan), y covers the owned rows; sizes, ownership ranges and kle_mat_get_info
 * are as for kle_mat_create_kle_element on ranks.  The incidence list, the
 * gather and the diagonal cover the owned nodes, whose incident elements are
 * all local: no communication.  The elements that read owned nodes alone are
 * not contiguous in ascending-cell order, so the element kernels take an
 * element list: the inner list (every entry, masked or not, an owned node)
 * and the outer list (at least one ghost).  A product is one forward halo of
 * x; with halo overlap on (kle_mat_set_halo_overlap, the default) the inner
 * list runs on the compute stream beside the halo on the comm stream, the
 * outer list after it, then the gather; with overlap off the halo first, then
 * both lists; kle_mat_time_local_spmv runs both lists without the halo.  An
 * empty list launches nothing.  The element results, the geometry tables and
 * the connectivity stay indexed by the element's own id, so the owned rows
 * are the one-rank product's bit for bit.  kle_mat_spmv_bytes counts the
 * local elements, the ext range of x, the owned rows and the lists. */
int kle_mat_create_kle_sumfac(kle_ctx *ctx, kle_mesh *m, int which, kle_mat **out);
/* Sum-factorised element-wise Rw [dim N x dim_w N] (dim_w = 1 in 2-D, 3 in
 * 3-D) of any mesh, box or unstructured, one rank or several (as
 * kle_mat_create_kle_sumfac: element lists, one forward halo of the ghosted w,
 * owned rows bit-identical to the one-rank product): the Rw of kle_assemble_kle
 * with no assembled values and no element matrix,
 *     (Rw_e w)_l^a =  sum_{q in full} c_q N_l(q) (curl w)_a(q)
 *                   + a_w sum_{q in red} c_q sum_b d_b N_l(q) eps_{acb} w_c(q)
 * (2-D: y_0 = sum c N_l d_y w - a_w sum c d_y N_l w, y_1 = -sum c N_l d_x w +
 * a_w sum c d_x N_l w).  k_sumfac_rw has the batching, LDS tiles, tables and
 * geometry of k_sumfac_elem.  Full rule: forward passes with h / dh, inv J,
 * c curl w, value passes back (h transposed).  Reduced rule: forward value
 * passes, the flux c (a_w w_c) placed by eps, inv J^T, the transposed
 * derivative passes; its sum is added to the full rule's.  No entry of w is
 * dropped.  k_sumfac_gather_rw sums a free row's incidence entries in
 * ascending element order; a Dirichlet row is +0.0 and reads nothing, as the
 * assembled Rw has no entry there.  No atomics: the same input gives the same
 * bits.
 * K, Krhs and Rw of one mesh share the two geometry tables: the mesh hands out
 * one reference-counted set, freed with its last holder (operators may be
 * destroyed in any order, the mesh before them).
 * The result is a kle_mat of format 2 ("elem") with the call surface of
 * kle_mat_create_kle_element's Rw: kle_mat_mult, kle_mat_mult_add, the size
 * and ownership getters, kle_mat_get_info (nz_used 0), kle_mat_spmv_bytes,
 * kle_mat_spmv_kernel ("k_sumfac_rw<D>+k_sumfac_gather_rw<D>") and
 * kle_mat_time_local_spmv.  KLE_ERR_SUP: kle_mat_get_diagonal,
 * kle_mat_copy_dirichlet_rows, every call that needs stored values, no-slip
 * meshes (their Rw and Rwfs: kle_mat_create_ns_sumfac) and a mesh whose nranks
 * is not the context's.
 * kle_ksp_set_operators refuses the non-square 2-D Rw before any
 * launch.  Every table index is checked on the host before upload. */
int kle_mat_create_rw_sumfac(kle_ctx *ctx, kle_mesh *m, kle_mat **out);
/* Element-wise no-slip operator of a uniform box mesh: the matrices of
 * kle_assemble_ns (MatNS.buildNS, mat_ns.py:47-145) with no stored values.
 * which: 0 K, 1 Krhs, 2 Rw, 3 Kfs, 4 Krhsfs, 5 Rwfs, 6 K + Kfs (the operator
 * of KleSolver.solverFS).  The masks act per velocity DoF through the mesh's
 * classes F (free) / T (tangential) / N (normal).  Every operator is
 * S_e^T K_e0 S_e (Rw, Rwfs: S_e^T Rw_e0 S_e^w) restricted to at most two
 * passes of (column classes kept -> row classes that take the sum), with a
 * fixed rule on every other row:
 *     K       {F} -> {F};                       T, N: y_i = x_i
 *     Krhs    {T,N} -> {F}, negated;            T, N: y_i = x_i
 *     Rw      every w column -> {F};            T, N: 0
 *     Kfs     {F,T} -> {T} and {T} -> {F};      T rows also add -x_i; N: 0
 *     Krhsfs  {N} -> {F,T}, negated;            N: y_i = x_i
 *     Rwfs    every w column -> {T};            F, N: 0
 *     K + Kfs {F,T} -> {F,T};                   N: y_i = x_i
 * Dropping a column is selection: the entry of x is never read, so an Inf or
 * NaN in it reaches no result.  An identity row returns x_i bit for bit, a
 * zero row +0.0 and reads nothing.  A pass is one launch of the element GEMM
 * of kle_mat_create_kle_element whose column index comes from a per-element,
 * per-column table [E][nc] of ext-local x indices (-1 dropped) instead of the
 * node connectivity (Rw and Rwfs keep every column and use the node table);
 * Kfs runs two passes into two result arrays.  A gather per owned DoF applies
 * its class's rule, the sums in ascending element order: no atomics, bitwise
 * repeatable.  K + Kfs forms the element sums, where the assembled matrix
 * carries PETSc's 1 + (S - 1) on tangential diagonals: they differ by at most
 * eps S |x_i| per row.
 * kle_mat_get_diagonal: the element diagonal sums in gather order on the
 * summed rows of K and K + Kfs, those sums - 1 on Kfs's T rows, 0 on every
 * other summed or zero row, 1 on identity rows; refused for Rw and Rwfs.
 * kle_mat_copy_dirichlet_rows copies the identity rows (K + Kfs: the N DoFs).
 * Everything else -- the supported and refused calls, the Krylov solvers, the
 * several-rank layout with one forward halo beside the interior elements and
 * owned rows bit-identical to the one-rank product -- is as for
 * kle_mat_create_kle_element; ghost DoFs are masked through the ext-indexed
 * classes.  Each operator owns its tables and workspace.
 * Needs a box mesh with its no-slip DoFs set (kle_mesh_set_noslip_*).
 * KLE_ERR_SUP for an unstructured mesh (any mesh: kle_mat_create_ns_sumfac), a
 * free-slip mesh and a mesh whose nranks is not the context's; KLE_ERR_ARG for
 * a bad which.  Every index
 * table entry and class is checked on the host before upload. */
int kle_mat_create_ns_element(kle_ctx *ctx, kle_mesh *m, int which, kle_mat **out);
/* The same seven no-slip operators (which 0 K, 1 Krhs, 2 Rw, 3 Kfs, 4 Krhsfs,
 * 5 Rwfs, 6 K + Kfs) sum-factorised, on any mesh, kind 0 (box) or kind 1
 * (unstructured), 2-D or 3-D, ngl 2..8, one rank or the parts of a partition:
 * the table of passes and row rules above, unchanged, with the
 * quadrature-point kernels of kle_mat_create_kle_sumfac /
 * kle_mat_create_rw_sumfac as the pass instead of the element GEMM.  No
 * stored values and no element matrix.
 * The mask is per DoF, so the connectivity stays unmasked and each K-family
 * operator carries a class table [E][nn] of one byte per element node: the dim
 * classes of that node at 2 bits each, taken from the ext-indexed classes of
 * the mesh (ghost DoFs included).  A pass is one launch of
 * k_sumfac_elem<D, LIST, CLS = true> whose argument is the 3-bit set of kept
 * classes: component b of a site loads x iff (keep >> cls_b) & 1, else it is 0
 * and x is never read there.  The CLS = false instantiations are the free-slip
 * kernels, instruction for instruction.  Rw and Rwfs keep every vorticity
 * column and run k_sumfac_rw unchanged.  Kfs runs two passes, {F,T} -> {T}
 * and {T} -> {F}, into two result arrays.  k_sumfac_gather_cls, one thread per
 * owned DoF, applies the rule of the row's class: a summed row adds its node's
 * entries of its pass's result array over the CSR incidence list in ascending
 * element order (Kfs's T rows then add -x_i), an identity row returns x_i bit
 * for bit, a zero row is +0.0 and reads nothing.  No atomics: the same input
 * gives the same bits.  K + Kfs forms the element sums (at most eps S |x_i|
 * per row from the assembled 1 + (S - 1)).
 * kle_mat_get_diagonal: formed once at creation by k_sumfac_diag and a gather
 * by class -- the element diagonal sums on the summed rows of K and K + Kfs,
 * those sums - 1 on Kfs's T rows, 1 on identity rows, 0 elsewhere; refused for
 * Rw and Rwfs.  kle_mat_copy_dirichlet_rows copies the identity rows.
 * The geometry tables are the mesh's shared, reference-counted set: the seven
 * operators of one mesh (and its free-slip-form collocation operators at
 * ngl > 3) hold one set.  Each operator owns its connectivity, incidence
 * list, class table, class bytes of the owned DoFs and result arrays.
 * Several ranks: the ext-local connectivity and the inner / outer element
 * lists of kle_mat_create_kle_sumfac; one forward halo of x per product
 * (Kfs's two passes share it, both run per list); owned rows bit-identical to
 * the one-rank product.
 * Call surface as kle_mat_create_ns_element: kle_mat_mult, kle_mat_mult_add,
 * kle_mat_get_diagonal, the size and ownership getters, kle_mat_get_info
 * (nz_used 0), kle_mat_time_local_spmv, kle_mat_spmv_kernel
 * ("k_sumfac_elem<D,cls>[x2]+k_sumfac_gather_cls<D>", Rw and Rwfs
 * "k_sumfac_rw<D>+k_sumfac_gather_cls<D>"), kle_mat_spmv_bytes (the class
 * table and one result array per pass counted) and kle_ksp_set_operators on
 * K and K + Kfs with cg (classic and single reduction), pipecg or gmres and PC
 * none or jacobi.  Calls that need stored values return KLE_ERR_SUP.
 * Needs a mesh with its no-slip DoFs set (kle_mesh_set_noslip_*).  KLE_ERR_SUP
 * for a free-slip mesh and a mesh whose nranks is not the context's;
 * KLE_ERR_ARG for a bad which.  Connectivity, incidence, element lists and
 * every class are checked on the host before upload. */
int kle_mat_create_ns_sumfac(kle_ctx *ctx, kle_mesh *m, int which, kle_mat **out);
/* Element-wise collocation operator of a uniform box mesh: which 0 Curl
 * [dim_w N x dim N], 1 SrT [dim_s N x dim N], 2 DivSrT [dim N x dim_s N], the
 * operators kle_assemble_operators assembles, with no stored values:
 *     y = Winv sum_e S_e^T M_e0 S_e^c x.
 * Row (l, a) of the element matrix M_e0 has entries only at the nodes on the
 * dim grid lines through l, so M_e0 x_e is sum-factorised: per element dim
 * 1-D derivative passes over the gathered x (k_colloc_elem), then inv J, the
 * coefficient placement of the assembly and c_l = w_l det J; a gather per node
 * in ascending element order times the inverse lumped weight follows
 * (k_colloc_gather).  No atomics: bitwise repeatable, and equal to the
 * assembled product to rounding plus the spread of the element geometry over
 * the mesh.  c_l, inv J and the derivative table come from the assembly's own
 * geometry path on the corners of global element 0.  At creation the dense M_e0 of
 * the factored tables is compared on the host with the element matrix of the
 * assembly path (kle_element_ops): exactly 0 off the grid lines, a few ulps on
 * them, KLE_ERR_STATE otherwise.
 * Memory: connectivity and incidence tables, N weights and E * RW * ngl^dim
 * doubles of element results (RW the row components).
 * The result is a kle_mat of format 2 ("elem").  It supports kle_mat_mult
 * (KLE_ERR_ARG where y aliases x, KLE_ERR_SIZ for a wrong vector layout),
 * kle_mat_mult_add, the size / local-size / ownership getters,
 * kle_mat_get_info (nz_used = 0), kle_mat_spmv_bytes, kle_mat_spmv_kernel and
 * kle_mat_destroy.  KLE_ERR_SUP: everything the element-wise Rw refuses, and
 * kle_mat_get_diagonal, kle_ksp_set_operators, kle_mat_copy_dirichlet_rows.
 * kle_mat_time_local_spmv works as for the element-wise K.
 * Several ranks: as kle_mat_create_kle_element -- ext-local tables over every
 * element touching an owned node, one forward halo of the ghosted x beside
 * the interior elements, owned rows bit-identical to the one-rank product; a
 * workgroup takes whole elements, so the ghost layer is computed whole.
 * Needs a box mesh, ngl 2..8; no Dirichlet set is needed and no-slip box
 * meshes are accepted (the operators carry no boundary rule).  KLE_ERR_SUP
 * for unstructured meshes and a mesh whose nranks is not the context's,
 * KLE_ERR_ARG for a bad which. */
int kle_mat_create_operator_element(kle_ctx *ctx, kle_mesh *m, int which, kle_mat **out);
/* The same collocation operators (which 0 Curl, 1 SrT, 2 DivSrT) with every
 * element's own geometry, on any mesh, box or unstructured, 2-D or 3-D, ngl
 * 2..8, free-slip or no-slip, one rank or several:
 *     y = Winv sum_e S_e^T M_e S_e^c x.
 * k_colloc_elem reads c_l and inv J of its own element from the nodal table
 * [E][nn][1 + dim^2] that the assembly's geometry kernel fills at the operator
 * points over all local elements (the table kle_assemble_operators builds).
 * The gather runs over a CSR incidence list (any valence, ascending element),
 * then times winv[node]; winv = 1 / sum_e c_{e,l(n)} in ascending incidence
 * order, the assembled operators' weights bit for bit.  The three operators
 * of a mesh share the nodal table, and at ngl > 3, where the full rule's
 * points and weights are the operator points' bit for bit (checked on the
 * host), it is the full-rule table of kle_mat_create_kle_sumfac and
 * kle_mat_create_rw_sumfac.
 * Call surface and refusals as kle_mat_create_operator_element
 * (kle_mat_spmv_kernel: "k_colloc_elem<D,Op,geo>+k_colloc_gather_csr<RW>").
 * Several ranks: the tables, the two element lists and the halo pattern of
 * kle_mat_create_kle_sumfac; winv is formed over the owned nodes, whose
 * incident elements are all local; owned rows bit-identical to the one-rank
 * product.
 * KLE_ERR_SUP for a mesh whose nranks is not the context's, KLE_ERR_ARG for a
 * bad which; connectivity, incidence and element lists are checked on the
 * host before upload. */
int kle_mat_create_operator_sumfac(kle_ctx *ctx, kle_mesh *m, int which, kle_mat **out);
/* Dense collocation element matrices of local element e as the assembly forms
 * them, before the nodal weight (parity tests, the creation check above):
 * Curl_e [dim_w n][dim n], SrT_e [dim_s n][dim n], DivSrT_e [dim n][dim_s n]
 * (row-major, n = ngl^dim, node-major components) and c_e [n] = w_l det J. */
int kle_element_ops(kle_ctx *ctx, kle_mesh *m, int64_t e, double *Curl_e, double *SrT_e, double *DivSrT_e,
                    double *c_e);
/* dst_i = src_i on the Dirichlet rows of an element-wise operator (its own
 * Dirichlet flags; rows dim N; a no-slip operator of kle_mat_create_ns_element:
 * its identity rows by DoF class), every other entry of dst untouched; on the
 * context's stream, no synchronisation.  KleSolver uses it after a
 * matrix-free solve: the unit Dirichlet rows make u_i = b_i = u_bc exactly,
 * which a Krylov iteration started from 0 reaches only to its tolerance.
 * KLE_ERR_SUP for any other matrix kind. */
int kle_mat_copy_dirichlet_rows(const kle_mat *A, const kle_vec *src, kle_vec *dst);

/* Generic AIJ (petsc4py Mat().createAIJ + setValues + assemble). */
int kle_mat_create_aij(kle_ctx *ctx, int64_t m_local, int64_t n_local, int64_t m_global,
                       int64_t n_global, const int32_t *d_nnz, const int32_t *o_nnz,
                       kle_mat **out);
/* createAIJ(csr=(indptr, indices, data)): assembled scalar CSR (single rank),
 * strictly ascending columns per row. */
int kle_mat_create_aij_csr(kle_ctx *ctx, int64_t m, int64_t n, const int64_t *indptr, const int64_t *indices,
                           const double *data, kle_mat **out);
int kle_mat_set_values(kle_mat *A, int32_t nr, const int64_t *rows, int32_t nc,
                       const int64_t *cols, const double *v_rowmajor, int addv);
int kle_mat_assemble(kle_mat *A);
/* State of a generic AIJ matrix, as PETSc's: between creation and the first
 * kle_mat_assemble, and again between a kle_mat_set_values on the assembled
 * matrix and the next kle_mat_assemble, the matrix is not assembled.  In both
 * states kle_mat_mult, kle_mat_mult_add, kle_mat_get_diagonal, kle_mat_get_row,
 * kle_mat_get_csr_size, kle_mat_get_csr, kle_mat_duplicate, kle_mat_convert_aij,
 * kle_mat_diagonal_scale, kle_mat_axpy (either operand), kle_ksp_set_operators,
 * kle_ksp_set_up and kle_ksp_solve return KLE_ERR_STATE before any device work
 * and change nothing; kle_mat_assemble then makes the pending values visible
 * to all of them.  An insertion outside the assembled pattern stays
 * KLE_ERR_NEWNZ. */
int kle_mat_destroy(kle_mat *A);
int kle_mat_get_size(const kle_mat *A, int64_t *m_global, int64_t *n_global);
int kle_mat_get_ownership_range(const kle_mat *A, int64_t *lo, int64_t *hi);
/* MatGetLocalSize (petsc4py Mat.getLocalSize; the local sizes behind
 * createVecLeft / createVecRight, base_problem.py:175,184, kle_solver.py:18) */
int kle_mat_get_local_size(const kle_mat *A, int64_t *m_local, int64_t *n_local);
int kle_mat_get_local_nnz(const kle_mat *A, int64_t *nnz);
/* MatGetInfo (+ sizes): PETSc nonzeros of the owned rows, the storage format
 * (0 node-block, 1 scalar AIJ, 2 element-wise: nz_used 0), block shape and
 * the SpMV's algorithmic bytes. */
typedef struct {
    int64_t m_global, n_global, m_local, n_local;
    int64_t nz_used;       /* PETSc nonzeros of the owned rows (explicit zeros included) */
    int format;            /* 0 node-block CSR, 1 scalar AIJ, 2 element-wise */
    int block_rows, block_cols;
    double spmv_bytes;     /* algorithmic bytes of one y = A x on this rank */
} kle_mat_info;
int kle_mat_get_info(const kle_mat *A, kle_mat_info *info);
int kle_mat_mult(kle_mat *A, kle_vec *x, kle_vec *y);            /* y = A x */
int kle_mat_mult_add(kle_mat *A, kle_vec *x, kle_vec *y, kle_vec *z); /* z = y + A x */
/* A = diag(L) A diag(R), either may be NULL; every node-block shape the
 * product has a kernel for (3x2 and 2x3 of the 2-D SrT / DivSrT included).
 * R of a node-block matrix is a mesh vector of its column space. */
int kle_mat_diagonal_scale(kle_mat *A, const kle_vec *L, const kle_vec *R);
int kle_mat_get_diagonal(const kle_mat *A, kle_vec *d);
/* Y += a X where X's pattern is a subset of, or equal to, Y's.  Node-block
 * matrices: the same blocks AND the same export rule (DoF mask rule and
 * classes, diagonal-only Dirichlet rows) -- anything else is KLE_ERR_SUP, so
 * that the sum never multiplies by an entry its export does not show
 * (Mat.__add__ then forms the union-pattern AIJ sum). */
int kle_mat_axpy(kle_mat *Y, double a, const kle_mat *X);
int kle_mat_duplicate(const kle_mat *A, int copy_values, kle_mat **out);
/* Scalar CSR of the owned rows with GLOBAL column ids, PETSc pattern. */
int kle_mat_get_csr_size(const kle_mat *A, int64_t *m_local, int64_t *nnz);
/* Mat.getRow(row) (dmplex.py:332,363): owned global row -> global columns and
 * values in PETSc's pattern; call with cols = vals = NULL for the length. */
int kle_mat_get_row(const kle_mat *A, int64_t row, int64_t *ncols, int64_t *cols, double *vals);
int kle_mat_get_csr(const kle_mat *A, int64_t *indptr, int64_t *indices, double *data);
/* Convert (single rank) to the scalar-CSR device format (the AIJ kernel). */
int kle_mat_convert_aij(const kle_mat *A, kle_mat **out);
/* Structured columns: when every row's columns form a lattice box (K, Rw and
 * the operators on box meshes) the SpMV computes them from 8 B per row instead
 * of streaming 4 B per block (default on; 0 forces the column stream). */
int kle_mat_set_spmv_structured(kle_mat *A, int on);
int kle_mat_is_structured(const kle_mat *A, int *on);
/* Symmetric storage (MatSetOption(A, MAT_SPD, PETSC_TRUE) with PETSc's
 * MATSBAIJ layout; kle_solver.py:33-37 solves with the SPD K): keep only each
 * row's blocks from its diagonal block on and run the SpMV over them, every
 * stored off-diagonal block serving row i and, transposed, row j.  Needs a
 * 3x3 node-block matrix on a box lattice (one rank, or z slabs: the
 * transposed sums of upper ghost rows go back to their owner, MPISBAIJ's
 * reverse scatter) whose blocks are symmetric (to 1e-12 of the largest
 * entry; across ranks checked by one product through both storages);
 * otherwise KLE_ERR_SUP.  Collective at N > 1.  The full
 * storage stays (getRow, CSR export); any value change (diagonalScale, axpy,
 * setValues/assemble) drops the symmetric copy.  kle_assemble_kle turns it on
 * for K (tuning "spmv_sym", "spmv_sym_min_rows").  With the default
 * "spmv_sym_det" results are bitwise reproducible run to run.
 * Accuracy (tests/test_gpu_sym_ref.py): the assembled K equals its transpose
 * bit for bit (k_gather reads one triangle of every element matrix), so the
 * stored triangle is the exported matrix.  Norm-wise y agrees with the
 * full-storage product at fp64 level.  Component-wise, with u = 2^-53,
 *     |y_i - (K x)_i| <= O(u) (|K||x|)_i + nT_i 2^(E-62):
 * row i's direct sum is fp64; each of the nT_i node blocks transposed into it
 * enters an int64 sum rounded to q = 2^(E-61), 2^E > (the part's bound <=
 * 4 ||K||inf) x (max|x| over the part's region), E <= log2(16 ||K||inf
 * ||x||inf).  The sums are exact integer sums (order-free), not exact
 * products: where x spans many decades the quantum follows the region's
 * largest entry, and a row whose own terms are small sees it (one entry 1e8
 * among O(1): 1e-8 relative on the worst row, 4e-15 norm-wise).  The scale
 * is two normal factors: subnormal x is not flushed, sums near DBL_MAX do not
 * wrap (a transposed term that itself overflows is not detected). */
int kle_mat_set_symmetric(kle_mat *A, int on);
int kle_mat_get_symmetric(const kle_mat *A, int *on);
/* The brick decomposition of A's symmetric storage (kle_brick.hip; 0 bricks:
 * none -- full storage, tiles or the graph kernel): bricks, bricks along
 * x / y / z, region entries per row, the planner's modelled product time
 * (us). */
/* Diagnostic: move the symmetric storage's value array.  fresh = 1: to a new
 * allocation, `shift` bytes (a multiple of 8, <= 1 GiB) into it (the old one
 * freed).  fresh = 0: `shift` bytes into the allocation of the previous
 * fresh = 0 move -- the same physical pages, another offset (the first such
 * call makes that allocation, with 8 MB of room, at offset 0).  The product
 * is unchanged bit for bit; its speed should not depend on the offset
 * (tests/test_gpu_fullsize.py). */
int kle_mat_move_values(kle_mat *A, long long shift, int fresh);
int kle_mat_get_sym_bricks(const kle_mat *A, int *nbricks, int *dims, double *entries_per_row, double *model_us);
/* Whether the bricks' value stream is the compact one (tuning
 * "spmv_brick_compact": a K whose analytically zero entries, "asm_box_zeros",
 * are all stored as +0.0 streams the other entries alone) and how many entries
 * it leaves out; 0, 0 otherwise. */
int kle_mat_get_brick_compact(const kle_mat *A, int *compact, long long *dropped_entries);
/* Whether the bricks' rows with bitwise equal value streams share one copy
 * (tuning "spmv_brick_dedup"), and then the rows stored and their bytes
 * (each row padded to 16 doubles); 0, 0, 0 otherwise.  kle_mat_spmv_bytes
 * still counts what the kernel's loads request, not what reaches HBM. */
int kle_mat_get_brick_dedup(const kle_mat *A, int *dedup, long long *unique_rows, long long *unique_bytes);
/* The runs of a shared full-layout K (units of one class next to each other,
 * an item's values loaded once per run of at most run_cap units): the cap, the
 * runs, the units, the 64-lane items and the items whose values are loaded;
 * all 0 where the product takes no runs. */
int kle_mat_get_brick_runs(const kle_mat *A, int *run_cap, long long *runs, long long *units, long long *items,
                           long long *item_loads);
/* N > 1: run the rows that read no ghost entry while the halo exchange is in
 * flight on a second stream (default on). */
int kle_mat_set_halo_overlap(kle_mat *A, int on);
/* Row padding quantum (in blocks) of node-block matrices created afterwards:
 * every value stream of a row starts on a multiple of `quantum` doubles
 * (16 = one 128-B line) so adjacent streams never share a cache line. */
int kle_set_nb_pad(int quantum);  /* default 16 */
int kle_get_nb_pad(void);
/* Value layout of node-block matrices created afterwards: 0 = each row's
 * R*C value streams padded to the pad quantum; 1 = 16-block chunks (each
 * stream's 128-B line per chunk) + packed tail, rows 128-B aligned (no
 * per-stream padding). */
int kle_set_nb_layout(int layout);
int kle_get_nb_layout(void);
/* "nb" (node-block), "aij" or "elem" (kle_mat_create_kle_element). */
int kle_mat_get_format(const kle_mat *A, char *buf, int buflen);
/* Bytes one SpMV with this matrix moves (algorithmic: matrix + x + y). */
int kle_mat_spmv_bytes(const kle_mat *A, double *bytes);
/* Name of the kernel(s) y = A x launches with the current tuning, as rocprof
 * lists them (profile summaries, bench.py's roofline record). */
int kle_mat_spmv_kernel(const kle_mat *A, char *buf, int buflen);
/* Average device time (ms) of `reps` rank-local products y = A x: the bricks
 * and the gather of every row they touch, with no halo exchange either way
 * (the ghost x as they are).  A part's own kernel time, free of its
 * neighbours -- ranks that share a GPU take turns.  Box-brick symmetric
 * storage (y's ghost-row sums are not sent), an element-wise operator (its
 * element launches over this rank's local elements and the owned-row gather,
 * at any rank count; a sum-factorised operator on ranks: both element lists),
 * or, on several ranks, a rank's part of any other node-block matrix (every
 * owned row; graph symmetric storage: its groups or bricks and the gather,
 * the ghost rows' sums not sent; the box symmetric tiles are refused);
 * KLE_ERR_ARG otherwise, as for a one-rank matrix without bricks, whose
 * product is its local product. */
int kle_mat_time_local_spmv(kle_mat *A, const kle_vec *x, kle_vec *y, int reps, double *ms);

/* -------------------------------------------------------------------- ksp */
int kle_ksp_create(kle_ctx *ctx, kle_ksp **out);
int kle_ksp_destroy(kle_ksp *k);
int kle_ksp_set_type(kle_ksp *k, const char *type);      /* "cg" | "gmres" | "preonly" */
int kle_ksp_set_pc_type(kle_ksp *k, const char *type);   /* "none" | "jacobi" | "lu"   */
int kle_ksp_set_pc(kle_ksp *k, const char *type);        /* KSPSetPC(PCSetType): same as set_pc_type */
/* KSPSetTolerances (a negative value / maxit <= 0 keeps the current one;
 * defaults 1e-5, 1e-50, 1e5, 10000).  The residual norm r_k of every
 * iteration is tested as KSPConvergedDefault does: NaN/Inf ->
 * KLE_DIVERGED_NANORINF; r_k <= max(rtol ||b||, atol) -> converged; then
 * r_k >= dtol ||b|| -> KLE_DIVERGED_DTOL, at iteration 0 too (dtol <= 1
 * stops every solve there, x = 0); then max_it.  CG, single-reduction and
 * pipelined CG and GMRES all honour dtol; x is the iterate of the reported
 * iteration.  Fixed-iteration mode tests none of them. */
int kle_ksp_set_tolerances(kle_ksp *k, double rtol, double atol, double dtol, int maxit);
int kle_ksp_set_gmres_restart(kle_ksp *k, int restart);
/* CG with one reduction per iteration (Chronopoulos-Gear), as PETSc's
 * -ksp_cg_single_reduction. */
int kle_ksp_set_cg_single_reduction(kle_ksp *k, int flag);
/* Run exactly n iterations, no convergence test (benchmarks); 0 = off. */
int kle_ksp_set_fixed_iterations(kle_ksp *k, int n);
/* Benchmarks: n more iterations of the preceding fixed-iteration solve's
 * recurrence on the same (b, x) -- no restart (single-reduction / pipelined
 * CG), so a timed region holds exactly n iterations. */
int kle_ksp_continue(kle_ksp *k, kle_vec *b, kle_vec *x, int n);
int kle_ksp_set_operators(kle_ksp *k, kle_mat *A);
int kle_ksp_set_up(kle_ksp *k);
int kle_ksp_solve(kle_ksp *k, kle_vec *b, kle_vec *x);
int kle_ksp_get_iteration_number(const kle_ksp *k, int *its);
/* Kernel name(s) of the products inside the last solve call, as rocprof lists
 * them: kle_mat_spmv_kernel's, or -- where the CG update gathers a split
 * box-brick product itself -- the brick kernel alone (one rank). */
int kle_ksp_get_product_kernel(const kle_ksp *k, char *buf, int buflen);
/* Algorithmic bytes one of those products moves (kle_mat_spmv_bytes, or the
 * bricks' own share of a split product: the region sums written, not read). */
int kle_ksp_get_product_bytes(const kle_ksp *k, double *bytes);
int kle_ksp_get_residual_norm(const kle_ksp *k, double *rnorm);
int kle_ksp_get_converged_reason(const kle_ksp *k, int *reason);
/* ||b - A x|| / ||b|| recomputed after the last solve. */
int kle_ksp_get_true_relative_residual(const kle_ksp *k, double *rel);
/* CG / pipelined CG stop on their recursive residual (KSPSolve,
 * kle_solver.py:35), which drifts from the true one (pipelined: 1.1-1.3e-10
 * at rtol 1e-10).  When the true residual misses rtol, up to n correction
 * solves A e = b - A x (same method) follow, so the solve meets rtol on the
 * true residual (the north star's "same residual as PETSc KSP within
 * 1e-10"); n = 0 stops on the recursive residual exactly as PETSc's KSPCG /
 * KSPPIPECG do.  Default 2 (kle_set_tuning "ksp_refine" for new KSPs). */
int kle_ksp_set_corrections(kle_ksp *k, int n);
/* Iterations of the last solve's correction solves (0: none ran).  They are
 * NOT in kle_ksp_get_iteration_number, and the converged reason and residual
 * norm stay the main solve's (PETSc's KSPGetIterationNumber /
 * KSPGetConvergedReason of the recursive stop); each correction has max_it of
 * its own. */
int kle_ksp_get_correction_iterations(const kle_ksp *k, int *its);
/* Converged reason of the last correction solve (0: none ran; < 0: it hit
 * max_it or broke down and the true residual may still miss rtol). */
int kle_ksp_get_correction_reason(const kle_ksp *k, int *reason);

/* ------------------------------------------------------------ diagnostics */
/* Streaming read/copy microbenchmark (HBM ceiling for the roofline). */
int kle_stream_copy_bench(kle_ctx *ctx, int64_t bytes, int reps, double *gbps);
/* mode 0: copy (read+write bytes counted), 1: read-only 32 B/lane non-temporal,
 * 2: read-only 8 B/lane non-temporal, 3: read-only 8 B/lane plain. */
int kle_stream_bench(kle_ctx *ctx, int64_t bytes, int reps, int mode, double *gbps);

#ifdef __cplusplus
}
#endif
#endif
