// kle_brick.hip -- the box symmetric SpMV on bricks: one kernel in four
// variants and their device set-up.  Full: every stored block's nine doubles,
// each row its own stream.  Compact: the analytic zeros of a box K left out
// (kle_brick.hpp brick_drop_bits; chosen in kle_sym.hip sym_build_impl where
// they are all stored as exact zeros).  Dedup: rows with bitwise equal streams
// share one copy (brick_dedup, kept where it saves half the bytes), over
// either layout.  Runs: on a deduplicated full layout a wave takes up to
// BRICK_RUN_G units of one class at once (brick_runs_build, kept where
// brick_runs_pay).  brick_kernel_of picks the kernel of a matrix; the row
// descriptors' layout is kle_brick.hpp's, the plan kle_brick_plan.cpp's.
//
// Symmetric (SBAIJ-style, upper-triangle) storage of the structured KLE K
// (kle_mat_set_symmetric = MatSetOption(MAT_SPD); MatFS.buildFS,
// mat_fs.py:150-192; the product is the MatMult inside KSPSolve,
// kle_solver.py:35).  Block (i, j), j >= i, serves row i (B x_j) and row j
// (B^T x_i), so the rows a workgroup touches extend past the rows it owns and
// their sums meet those of other workgroups.  Rounds 2-4 cut the lattice into
// 128-row tiles and wrote each tile's region sums to HBM in the middle of the
// value stream (4.6 partial entries per row, 90 MB per SpMV at config 2);
// those stores made the stream's speed depend on where the value array lay
// (424-491 us at config 2).
//
// Here the owned lattice is cut into at most one element-aligned brick per
// CU (planner: kle_brick_plan.cpp; config 2: 254 bricks), and one 16-wave
// workgroup streams a whole brick with x AND the exact int64 fixed-point
// sums of the brick's region (config 2: about 25 x 21 x 5 nodes, 126 KB)
// resident in LDS from the first value load to the last.  The rows' direct
// sums go to y as each row ends (8 MB); nothing else is stored while the
// value array streams.  At the end each brick writes its region once
// ([entry][3]; 2.02 entries per row, 16 MB), and the graph kernels' run-mask
// gather (kle_sym.hip gsym_gather) adds, per row, the sums of the bricks
// whose regions hold it in ascending brick order (bitwise reproducible, as
// the fixed-point sums are order-free): per 64-row slice of the lattice, each
// brick region's stretch of one lattice line is one run of consecutive sums.
// Inside a brick the waves take rows from an LDS counter, so the brick's end
// is one row long, not one wave's share.
// The value array is laid out brick by brick (rows in brick order, each row's
// upper tail in the 16-block chunk layout), so every CU streams one
// contiguous range.
#include <algorithm>
#include <climits>
#include <cmath>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "kle_brick.hpp"
#include "kle_internal.hpp"
#include "kle_sym_dev.hpp"

namespace kle {

using cint = __attribute__((address_space(4))) const int;

// a row of the brick (every field wave-uniform: SGPRs)
struct BRow {
    const double *v;
    int bnx, bnxy, k0, mu, rb0, ir;
    int dbb;  // (compact stream: the row's position in its box and its boundary bits, kle_brick.hpp)
};

// an issued item, packed in five words (SGPRs are the kernel's scarce
// registers): row P on lanes [0, s), row Q on lanes [s, 64) (s = 64: P
// alone), each from its first block kbP / kbQ; eP / eQ: the item ends row P /
// Q (its direct sum is complete); ok 0: a re-read past the brick's last unit
struct BItem {
    int ok;
    int ir;  // irP | irQ << 16
    int mu;  // muP | muQ << 16
    int kb;  // kbP | kbQ << 16
    int sf;  // s | eP << 8 | eQ << 9
};
__device__ __forceinline__ BItem bitem(int s, int muP, int muQ, int irP, int irQ, int kbP, int kbQ, int eP, int eQ)
{
    return {1, irP | irQ << 16, muP | muQ << 16, kbP | kbQ << 16, s | eP << 8 | eQ << 9};
}
constexpr int BI_NEWP = 1024;  // (sf: the item starts row P -- its x into the row registers)
constexpr int BI_PB = 2048;    // (sf, runs: row P is the unit's second row -- its full passes)
// (runs: the record also carries the run's units, n of them, and their region
// indices irA | irB << 16, as the cursor may be at the next run when the item is summed)
template <int G>
struct BItemG : BItem {
    int n;
    int iu[G];
    __device__ __forceinline__ BItemG &operator=(const BItem &b)
    {
        BItem::operator=(b);
        return *this;
    }
};

// FF: the first item's registers are in flight when the item loop starts,
// which holds only while the compiler does not copy them on the way there
// (checked in the ISA; a variant with two items in flight ahead of the summed
// one -- no faster, round 5 -- had them moved, wrong products, and is gone)
// DOT (one rank, a split product whose gather the CG update does): the
// brick's share of (A x, x) in dpart[brick] -- its rows' direct sums and its
// region's transposed sums, each times the x it is added at (the gather adds
// every one of them to exactly one entry of A x), so the update's prologue
// has (A x, x) before any row is gathered (kle_ksp.hip k_sr_iter_g)
// CP: the compact value stream (kle_brick.hpp brick_drop_bits; the pack:
// kle_sym.hip k_brick_pack).  Items, units, the shared tail item, one item in
// flight and the fixed vmcnt(9) are as without it; only where a lane's nine
// loads point differs.  Per item and per row part (P's lanes, Q's lanes) the
// values lie slot-major and compacted: slot t holds the kept lanes' values
// in lane order, one slot after another.  A lane's place in slot t is the
// count of kept lanes of its part below it (ballot, mbcnt), the slot's base
// the running sum of the part's counts, the part's base a wave-uniform
// running offset along the row's passes (a unit's second row: its last
// partial pass first, as the shared item reads it before the full passes).
// A lane whose slot is left out loads its part's first value (a line an
// active lane of the same load reads) and takes 0.0 after the wait.
// DD: a deduplicated value array (brick_dedup, below): rows with bitwise
// equal streams share one copy, so the two rows of an item may lie anywhere
// in the array, the second before the first.  The loads' scalar base is then
// the array itself and each lane's 32-bit offset starts at its own row's
// place in it (below 2^30 bytes: 23 bits x 16 doubles), instead of row P's
// address and the distance from P to Q.  NTL: nontemporal value loads (the
// full stream is read once per product; a deduplicated one is re-read by
// every brick and may stay cached).
// G > 0 (DD, full layout, no DOT): runs of same-class units (kle_brick.hpp
// brick_runs_build).  A wave takes a run -- up to G units that stream the
// identical items and differ only in their rows' region indices -- instead of
// a unit; the issue cursor walks the class's items once, so an item's nine
// values are loaded and its lanes' block positions in the box are computed
// once, and the summed item is applied to each unit of the run in turn:
// rr = (block position - the row's own) + the unit's region index, the
// unit's x and sums, exactly the arithmetic of a unit on its own.  rowd then
// holds the runs' records (brick_run_words(G) ints each, rstride per brick)
// and bd[b].nrun the brick's runs.
template <int WV, bool FF = true, bool DOT = false, bool CP = false, bool DD = false, bool NTL = true, int G = 0>
__global__ __launch_bounds__(64 * WV, 1) void k_nb_spmv_sym_brick(int Lx, int Ly, int Lz, int zo, int hp, int rstride,
                                                                 const BrickDesc *__restrict__ bd,
                                                                 const int2 *__restrict__ rowd,
                                                                 const double *__restrict__ sval,
                                                                 const double *__restrict__ x,
                                                                 double *__restrict__ ws, double *__restrict__ y,
                                                                 double *__restrict__ dpart,
                                                                 const int *__restrict__ istate KLE_PROBE_PARAM)
{
    static_assert(G == 0 || (DD && !CP && !DOT), "runs: the full layout of a deduplicated array, no DOT");
    KLE_PROBE_CONST
    constexpr int NT = 64 * WV;
    constexpr int GG = G > 0 ? G : 1, RW = brick_run_words(GG);
    using Item = std::conditional_t<(G > 0), BItemG<GG>, BItem>;
    constexpr int D = 1;  // items in flight ahead of the summed one
    extern __shared__ double lds[];
    KLE_PROBE_TS(ts0)
#ifdef KLE_PROBE_BUILD
    __shared__ unsigned pmx[4];
    if (threadIdx.x == 0) pmx[0] = pmx[1] = pmx[2] = pmx[3] = 0;  // (racy by design: the other waves' maxima come microseconds later)
#endif
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int NU = G > 0 ? bd[b].nrun : bd[b].nr / 2;  // units of two rows (kle_brick_plan.cpp); G: runs of them
    const int ox = bd[b].ox, oy = bd[b].oy, oz = bd[b].oz, RX = bd[b].RX, RY = bd[b].RY, RZ = bd[b].RZ;
    const int eb = bd[b].eb;
    const long long vbase = bd[b].vbase, wsoff = bd[b].wsoff;
    const int RN = RX * RY * RZ, RS = RN + 64, RXY = RX * RY;
    double *xl = lds;
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(lds + 3 * RN);
    double *wred = lds + 3 * RN + 3 * RS;
    int *ctr = reinterpret_cast<int *>(wred + 2 * WV);
    const int64_t Lxy = (int64_t)Lx * Ly;
    // 2a. x of the region into LDS (nodes off the lattice read 0), its max
    // |x|; the sums zeroed.  Line (ry, rz) of the region is 3 RX contiguous
    // doubles of x; a thread takes one position in a line and every fstep-th
    // line, FB loads in flight (unconditional: clamped addresses, masked
    // values).  FF: the first FB loads go out here, before anything waits on
    // the row descriptors and before the first items' value loads (asm,
    // waited for with vmcnt(9 D) in 2b), so they queue neither behind the
    // descriptor round trip nor behind the whole chip's first value loads.
    double xm = 0.0;
    int bad = 0;
    constexpr int FB = 12;
    const int L3 = 3 * RX, NL = RY * RZ;
    const int c3 = threadIdx.x % L3, l0 = threadIdx.x / L3, fstep = NT / L3;
    const int rx = c3 / 3, c = c3 - 3 * rx, gx = ox + rx;
    const bool xok = l0 < fstep && gx >= 0 && gx < Lx;
    // (line l = (ry, rz) and its offset in x stepped by fstep lines without
    // a division per load; offsets in 32 bits: brick_setup refuses lattices
    // of 2^29 / 3 or more ext nodes)
    const int dz = fstep / RY, dy = fstep - dz * RY, sy = 3 * Lx, sz = 3 * Lx * Ly;
    int fz = l0 / RY, fy = l0 - fz * RY, fo = 3 * gx + c + sy * (oy + fy) + sz * (oz + zo + fz);
    // (the unused loads -- lines past the region, threads past fstep lines:
    // most of a small brick's 12 per thread -- read the brick's first node,
    // not x[0]: one line of every brick's fill, not one line of the chip,
    // which every workgroup's dummies made a hot spot at kernel start)
    const int fdummy = 3 * (min(max(ox, 0), Lx - 1) + Lx * (min(max(oy, 0), Ly - 1) +
                                                           Ly * min(max(oz + zo, 0), zo + Lz + hp - 1))) + c;
    auto fnode = [&](int l, bool &ok) -> int {
        const int gy = oy + fy, gz = oz + fz;
        ok = xok & (l < NL) & (gy >= 0) & (gy < Ly) & (gz + zo >= 0) & (gz < Lz + hp);  // (no branches)
        const int off = ok ? fo : fdummy;
        fy += dy;
        fz += dz;
        fo += sy * dy + sz * dz;
        if (fy >= RY) {
            fy -= RY;
            ++fz;
            fo += sz - sy * RY;
        }
        return off;
    };
    auto fstore = [&](int lb, double *fv) {
#pragma unroll
        for (int f = 0; f < FB; ++f) {
            const int l = lb + f * fstep;
            const bool st = l0 < fstep && l < NL;
            xl[st ? c * RN + rx + RX * l : 4 * RN + lane] = fv[f];  // (else a dummy slot of the sums)
            const double a = fabs(fv[f]);
            bad |= !(a <= 1.7976931348623157e308);
            xm = fmax(xm, a);
        }
    };
    double fv0[FB];
    unsigned okm = 0;
    if constexpr (FF) {
#pragma unroll
        for (int f = 0; f < FB; ++f) {
            bool ok;
            const int off = fnode(l0 + f * fstep, ok);
            okm |= (unsigned)ok << f;
            ld_x1(fv0[f], x, 8u * (unsigned)off);
        }
    }
    KLE_PROBE_TS(tsi)
    // (read after the fill's loads are out: the compiler waits for it at once)
    const int stop = istate ? istate[I_REASON] : 0;  // (tested before the first store)
    // (the brick's rows at a fixed stride: their descriptors' address needs
    // no load, so their scalar loads go out beside bd's; address-space
    // cast: scalar loads)
    // (G: the brick's run records, UW ints each -- the class's four words,
    // the count, the units' region indices)
    constexpr int UW = G > 0 ? RW : 4;
    cint *rdesc = G > 0 ? (cint *)(reinterpret_cast<const int *>(rowd) + (int64_t)b * rstride * RW)
                        : (cint *)(rowd + (int64_t)b * rstride);
    const double *vb = sval + vbase;
    // a row from its descriptor: the layout kle_brick.hpp brick_row_box,
    // brick_row_ir and brick_row_off define, decoded here in the kernel's own registers
    auto row_setup = [&](int r, int dw, int vw, BRow &R) {
        constexpr int DM = CP ? 7 : 15;
        const int dbx = dw & DM, dby = (dw >> 4) & DM, dbz = (dw >> 8) & DM;
        R.dbb = dw & 0xFFF;
        R.bnx = (dw >> 12) & 15;
        const int bny = (dw >> 16) & 15, bnz = (dw >> 20) & 15;
        R.bnxy = R.bnx * bny;
        R.k0 = dbx + R.bnx * (dby + bny * dbz);
        R.mu = R.bnxy * bnz - R.k0;
        R.ir = ((dw >> 24) & 255) | (((vw >> 24) & 255) << 8);
        R.rb0 = R.ir - (dbx + RX * (dby + RY * dbz));
        R.v = vb + (int64_t)(vw & (BRICK_ROW_NULL - 1)) * 16;
    };
    // the values of one item -- lanes below s from row P's blocks kbP + lane,
    // the others from row Q's blocks kbQ + lane - s (Q's values follow P's);
    // lanes past a row's end re-read its last block (their results go
    // nowhere) -- and each block's region index
    // (CP: oP / oQ the parts' first doubles in their rows' streams; zP / zQ
    // the doubles the parts hold; rr then carries the lane's left-out pairs
    // in bits 16..18)
    auto load_v = [&](const BRow &P, const BRow &Q, int kbP, int kbQ, int s, double *vv, int &rr, int oP, int oQ,
                      int &zP, int &zQ) {
        const bool q = lane >= s;
        const int mu = q ? Q.mu : P.mu;
        const int kraw = q ? kbQ + lane - s : kbP + lane;
        const int kk = min(kraw, mu - 1);
        const unsigned bo = DD ? (unsigned)((q ? Q.v : P.v) - vb) * 8u : q ? (unsigned)(Q.v - P.v) * 8u : 0u;
        const int k = (q ? Q.k0 : P.k0) + kk;
        const int bnxy = q ? Q.bnxy : P.bnxy, bnx = q ? Q.bnx : P.bnx;
        const int kz = sym_div(k, bnxy, __builtin_amdgcn_rcpf((float)bnxy)), rem = k - kz * bnxy;
        const int ky = sym_div(rem, bnx, __builtin_amdgcn_rcpf((float)bnx)), kx = rem - ky * bnx;
        rr = (q ? Q.rb0 : P.rb0) + kx + RX * (ky + RY * kz);
        unsigned o[9];
        if constexpr (!CP) {
            const int q16 = mu & ~15;
            const bool ch = kk < q16;
            const int o0 = ch ? (kk >> 4) * 144 + (kk & 15) : q16 * 9 + (kk - q16);
            const int st = ch ? 16 : mu - q16;
#pragma unroll
            for (int t = 0; t < 9; ++t) o[t] = bo + (unsigned)(o0 + t * st) * 8u;
            zP = zQ = 0;
        } else {
            const bool act = kraw < mu;
            const int db = brick_drop_bits(q ? Q.dbb : P.dbb, kx, ky, kz);
            const bool kp[3] = {act && !(db & 1), act && !(db & 2), act && !(db & 4)};
            // the kept lanes of the diagonal slots and of the three pairs
            const unsigned long long mP = s >= 64 ? ~0ull : (1ull << s) - 1ull;
            const unsigned long long bl[4] = {__ballot(act), __ballot(kp[0]), __ballot(kp[1]), __ballot(kp[2])};
            int nP[4], nQ[4], n[4], c[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                nP[g] = __popcll(bl[g] & mP);
                nQ[g] = __popcll(bl[g] & ~mP);
                n[g] = q ? nQ[g] : nP[g];
                // (kept lanes of the lane's part below it)
                c[g] = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bl[g] >> 32),
                                                      __builtin_amdgcn_mbcnt_lo((unsigned)bl[g], 0u)) -
                       (q ? nP[g] : 0);
            }
            zP = 3 * nP[0] + 2 * (nP[1] + nP[2] + nP[3]);
            zQ = 3 * nQ[0] + 2 * (nQ[1] + nQ[2] + nQ[3]);
            const unsigned pb0 = bo + (unsigned)(q ? oQ : oP) * 8u;
            int sb = 0;  // (the slot's base in the part)
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int g = brick_slot_pair(t) + 1;
                const bool keep = g == 0 ? act : kp[g - 1];
                o[t] = keep ? pb0 + (unsigned)(sb + c[g]) * 8u : pb0;
                sb += n[g];
            }
            rr |= db << 16;
        }
        // (the base is wave-uniform; said so, as the loads take it in SGPRs)
        const unsigned long long pb = (unsigned long long)(DD ? vb : P.v);
        const unsigned phi = (unsigned)__builtin_amdgcn_readfirstlane((int)(pb >> 32));
        const unsigned plo = (unsigned)__builtin_amdgcn_readfirstlane((int)(pb & 0xffffffffull));
        sym_ld9<NTL>(vv, reinterpret_cast<const double *>(((unsigned long long)phi << 32) | plo), o);
    };
    // 1. units from an LDS counter; each wave's first D + 2 static (w, w + WV,
    // ...: the counter starts past them -- as many as the D items issued
    // before the fill can reach), so those go out before the fill
    auto grab = [&]() -> int {
        int r = 0;
        if (lane == 0) r = atomicAdd(ctr, 1);
        return __builtin_amdgcn_readfirstlane(r);
    };
    constexpr int NSTAT = D + 2;
    int snext = w + WV;
    auto take = [&]() -> int {  // (the next unit of this wave)
        if (snext < NSTAT * WV) {
            const int r = snext;
            snext += WV;
            return r;
        }
        return grab();
    };
    // The issue cursor over the wave's units: a unit (A, B) streams A's
    // passes (B absent: all of them; else its full ones), the item shared by
    // A's and B's last partial passes, then B's full passes.
    BRow A, B;
    bool hasB = false, idone = w >= NU;
    int ph = 0, ki = 0, aend = 0, bend = 0;
    int oa = 0, ob = 0;  // (CP: the cursor's place in A's and in B's stream, doubles)
    auto unit_setup = [&](int u, int d0, int d1, int d2, int d3) {
        row_setup(2 * u, d0, d1, A);
        hasB = (d3 & BRICK_ROW_NULL) == 0;
        if (hasB) row_setup(2 * u + 1, d2, d3, B);
        else B = A;
        aend = hasB ? (A.mu & ~63) : A.mu;
        bend = hasB ? (B.mu & ~63) : 0;
        ph = aend > 0 ? 0 : 1;
        ki = 0;
        oa = ob = 0;
    };
    // G: the run at the cursor (its units, their irA | irB << 16) and the
    // next one's, fetched ahead with its class's descriptors
    int rcnt = 1, rir[GG], pcnt = 1, pir[GG];
#pragma unroll
    for (int g = 0; g < GG; ++g) rir[g] = pir[g] = 0;
    auto run_units = [&](int u, int &cnt, int *ir) {
        if constexpr (G > 0) {
            cnt = rdesc[UW * u + 4];
#pragma unroll
            for (int g = 0; g < GG; ++g) ir[g] = rdesc[UW * u + 5 + g];
        }
    };
    if (!idone) {
        unit_setup(w, rdesc[UW * w], rdesc[UW * w + 1], rdesc[UW * w + 2], rdesc[UW * w + 3]);
        run_units(w, rcnt, rir);
    } else {
        A.v = vb;
        A.mu = 1;
        A.k0 = 0;
        A.bnx = A.bnxy = 1;
        A.rb0 = 0;
        A.ir = 0;
        A.dbb = 0;
        B = A;
    }
#ifdef KLE_PROBE_BUILD
    if (probe_ts) {  // (probe: this wave's first row descriptors are in)
        asm volatile("" ::"s"(A.mu), "s"(A.k0));
        if (lane == 0) atomicMax(&pmx[0], (unsigned)(__builtin_amdgcn_s_memrealtime() - ts0));
    }
#endif
    // the next unit and its descriptors, fetched one unit ahead
    int pend = idone ? NU : take();
    // (a brick without rows, NU = 0, reads its slot's first unit: the table
    // holds at least one unit per brick)
    const int u0 = max(0, min(pend, NU - 1));
    int pd0 = rdesc[UW * u0], pd1 = rdesc[UW * u0 + 1];
    int pd2 = rdesc[UW * u0 + 2], pd3 = rdesc[UW * u0 + 3];
    run_units(u0, pcnt, pir);
    // the item at the cursor: its loads into vn, its record; the cursor then
    // moves on (past the last unit it stays, re-reading the last item)
    auto issue = [&](double *vn, int &rn, Item &itn) {
        int zp, zq;
        if (idone) {  // (a re-read of A's first pass: cache hits, the results go nowhere)
            load_v(A, A, 0, 0, 64, vn, rn, 0, 0, zp, zq);
            itn.ok = 0;
            return;
        }
        if constexpr (G > 0) {
            itn.n = rcnt;
#pragma unroll
            for (int g = 0; g < GG; ++g) itn.iu[g] = rir[g];
        }
        if (ph == 0) {  // A's passes
            load_v(A, A, ki, 0, 64, vn, rn, oa, 0, zp, zq);
            oa += zp;
            itn = bitem(64, A.mu, A.mu, A.ir, A.ir, ki, 0, !hasB && ki + 64 >= A.mu, 0);
            if (ki == 0) itn.sf |= BI_NEWP;
            ki += 64;
            if (ki >= aend) ph = hasB ? 1 : 3;
        } else if (ph == 1) {  // A's and B's last partial passes
            const int s = A.mu - aend;
            load_v(A, B, aend, bend, s, vn, rn, oa, 0, zp, zq);  // (B's last partial pass opens its stream)
            ob = zq;
            itn = bitem(s, A.mu, B.mu, A.ir, B.ir, aend, bend, 1, bend == 0);
            if (aend == 0) itn.sf |= BI_NEWP;
            ki = 0;
            ph = bend > 0 ? 2 : 3;
        } else {  // B's full passes
            load_v(B, B, ki, 0, 64, vn, rn, ob, 0, zp, zq);
            ob += zp;
            itn = bitem(64, B.mu, B.mu, B.ir, B.ir, ki, 0, ki + 64 >= bend, 0);
            if constexpr (G > 0) itn.sf |= BI_PB;
            ki += 64;
            if (ki >= bend) ph = 3;
        }
        if (ph == 3) {  // the unit is done: the next one
            if (pend >= NU) {
                idone = true;
            } else {
                unit_setup(pend, pd0, pd1, pd2, pd3);
                if constexpr (G > 0) {
                    rcnt = pcnt;
#pragma unroll
                    for (int g = 0; g < GG; ++g) rir[g] = pir[g];
                }
                pend = take();
                const int u = max(0, min(pend, NU - 1));
                pd0 = rdesc[UW * u];
                pd1 = rdesc[UW * u + 1];
                pd2 = rdesc[UW * u + 2];
                pd3 = rdesc[UW * u + 3];
                run_units(u, pcnt, pir);
            }
        }
    };
    double v0[9], v1[9];
    int r0 = 0, r1 = 0;
    Item i0, i1;
#ifdef KLE_PROBE_BUILD
    unsigned long long tsf = 0;
#endif
    // 2b. the first item's value loads, then the fill's first loads landed
    // (vmcnt(9): the value loads stay in flight), into LDS; further lines
    // (regions of more than FB x fstep lines) after them
    {
        int lb = l0;
        if constexpr (FF) {
            issue(v0, r0, i0);
#ifdef KLE_PROBE_BUILD
            if (probe_ts && lane == 0) {
                atomicMax(&pmx[2], (unsigned)(__builtin_amdgcn_s_memrealtime() - ts0));
                atomicMax(&pmx[3], (unsigned)ts0);  // (the latest wave's start)
            }
#endif
            wait_x12<9 * D>(fv0);
#ifdef KLE_PROBE_BUILD
            tsf = probe_ts ? __builtin_amdgcn_s_memrealtime() : 0ull;
#endif
#pragma unroll
            for (int f = 0; f < FB; ++f) fv0[f] = (okm >> f) & 1u ? fv0[f] : 0.0;
            fstore(lb, fv0);
            lb += FB * fstep;
        } else {
            issue(v0, r0, i0);
        }
        for (; lb < NL; lb += FB * fstep) {
            double fv[FB];
#pragma unroll
            for (int f = 0; f < FB; ++f) {
                bool ok;
                const int off = fnode(lb + f * fstep, ok);
                const double v = x[off];
                fv[f] = ok ? v : 0.0;
            }
            fstore(lb, fv);
        }
    }
    for (int k = threadIdx.x; k < 3 * RS; k += NT) acc[k] = 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) xm = fmax(xm, __shfl_xor(xm, o, 64));
    const unsigned long long anybad = __ballot(bad);
    if (lane == 0) {
        wred[w] = xm;
        wred[WV + w] = anybad ? 1.0 : 0.0;
    }
    if (threadIdx.x == 0) *ctr = NSTAT * WV;
#ifdef KLE_PROBE_BUILD
    // (probe: the latest wave's fill landed and its arrival at the barrier)
    if (probe_ts && lane == 0) {
        atomicMax(&pmx[1], (unsigned)(__builtin_amdgcn_s_memrealtime() - ts0));
    }
#endif
    __builtin_amdgcn_s_waitcnt(0xC07F);  // LDS stores done (lgkmcnt 0); the value loads stay in flight
    __builtin_amdgcn_s_barrier();
    if (__builtin_amdgcn_readfirstlane(stop) != 0) return;  // (nothing written yet)
    // the brick's scale: 2^(61 - E), 2^E > (its sums' bound, k_brick_bound) x
    // max |x|, as two factors S1 S2 (and 1 / S as T1 T2), each a normal
    // double, so that x near the bottom of the exponent range (2^(61 - E) >
    // 2^1023) keeps its 61 bits too, and sums near the top of it (bound x
    // max |x| >= 2^1024 while every sum itself is finite) stay below 2^61
    double S1 = 1.0, S2 = 1.0, T1 = 1.0, T2 = 1.0;
    {
        double m = 0.0, nb = 0.0;
#pragma unroll
        for (int q = 0; q < WV; ++q) {
            m = fmax(m, wred[q]);
            nb += wred[WV + q];
        }
        if (nb != 0.0) {
            S1 = 0.0;  // non-finite x: NaN sums, as a floating-point product would give
            T1 = __builtin_nan("");
        } else if (m > 0.0) {
            int em;
            (void)frexp(m, &em);
            const int E = max(eb + em, -1070);  // (<= 2048: no clamp above, or sums near DBL_MAX would pass 2^61)
            const int e1 = max(min(61 - E, 1000), -1000), e2 = 61 - E - e1;
            S1 = ldexp(1.0, e1);
            S2 = ldexp(1.0, e2);
            T1 = ldexp(1.0, -e1);
            T2 = ldexp(1.0, -e2);
        }
    }
    KLE_PROBE_TS(ts1)
    // 3. The issue cursor runs D items in front of the compute cursor; each
    // issued item leaves a record (rows, lengths, region indices, first
    // blocks, which rows it ends), so the compute cursor needs no state of
    // the issue cursor.  Past the brick's last unit the issue cursor re-reads
    // its last item under a record r = -1, so every step issues 9 loads and
    // the wait for the summed item is a fixed vmcnt(9 D).
    double dr = 0.0;  // DOT: this lane's share of its rows' (direct sum, x)
    if (i0.ok) {
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
        double cx0 = 0.0, cx1 = 0.0, cx2 = 0.0;  // x of the current row, kept across its items
        // the row's direct sum (fixed-order DPP, fp64), one writer, into y --
        // the gather adds the bricks' transposed sums to it (8 MB of stores
        // at config 2: the only ones before the end)
        // DOT: each lane's part of the row's sum times the row's x (the same
        // in every lane that holds a part of it), before the lanes' sum
        auto row_out = [&](int ir, double a0, double a1, double a2, double xr0, double xr1, double xr2) {
            if constexpr (DOT) dr += (a0 * xr0 + a1 * xr1) + a2 * xr2;
            wsum3_dpp(a0, a1, a2);
            // (the row's lattice node from its region index: bricks may be
            // ragged, kle_brick_plan.cpp)
            const int irz = ir / RXY, irem = ir - irz * RXY, iry = irem / RX, irx = irem - iry * RX;
            const int64_t j = (ox + irx) + (int64_t)Lx * (oy + iry) + Lxy * (oz + irz);
            if (lane < 3) y[3 * j + lane] = lane == 0 ? a0 : lane == 1 ? a1 : a2;
        };
        // one step: issue the next item into vn, wait for vv (the D newer
        // items stay in flight), sum it
        // (G: the direct sums of the run's units, each unit's as on its own)
        double ag[GG][3];
#pragma unroll
        for (int g = 0; g < GG; ++g) ag[g][0] = ag[g][1] = ag[g][2] = 0.0;
        auto step = [&](double *vv, const int rrk, const Item &it, double *vn, int &rn, Item &itn) {
            const int rr = CP ? rrk & 0xFFFF : rrk;
            issue(vn, rn, itn);
            if (!it.ok) return false;
            if constexpr (G > 0) {
                // the item once for every unit of its run: the lanes' rows
                // and blocks are the class's, rr the block's place relative
                // to the row's own (row_setup with a region index of 0)
                const int is = it.sf & 255;
                const bool q = lane >= is;
                const int kk = q ? (int)((unsigned)it.kb >> 16) + lane - is : (it.kb & 0xFFFF) + lane;
                const bool live = kk < (q ? (int)((unsigned)it.mu >> 16) : (it.mu & 0xFFFF));
                const bool tl = live && kk > 0, mine = live && !q, qs = live && q;
#pragma unroll
                for (int g = 0; g < GG; ++g) {
                    if (g < it.n) {
                        // (row P: the unit's first row, or its second in that row's full passes)
                        const int irQ = (int)((unsigned)it.iu[g] >> 16), irP = it.sf & BI_PB ? irQ : it.iu[g] & 0xFFFF;
                        // x of the lane's row (one address per part: a broadcast read) and of its block's column
                        const int irl = q ? irQ : irP, rg = rr + irl;
                        const double c0 = xl[irl], c1 = xl[RN + irl], c2 = xl[2 * RN + irl];
                        const double xj0 = xl[rg], xj1 = xl[RN + rg], xj2 = xl[2 * RN + rg];
                        if (g == 0) sym_wait9<9 * D>(vv);
                        const int rt = tl ? rg : RN + lane;
                        const double s0 = vv[0] * xj0 + vv[1] * xj1 + vv[2] * xj2;
                        const double s1 = vv[3] * xj0 + vv[4] * xj1 + vv[5] * xj2;
                        const double s2 = vv[6] * xj0 + vv[7] * xj1 + vv[8] * xj2;
                        const double t0 = vv[0] * c0 + vv[3] * c1 + vv[6] * c2;
                        const double t1 = vv[1] * c0 + vv[4] * c1 + vv[7] * c2;
                        const double t2 = vv[2] * c0 + vv[5] * c1 + vv[8] * c2;
                        if (!(probe & 1)) {  // (timing probe 1: no transposed adds)
                            atomicAdd(&acc[rt], fx_of(t0 * S1, S2));
                            atomicAdd(&acc[RS + rt], fx_of(t1 * S1, S2));
                            atomicAdd(&acc[2 * RS + rt], fx_of(t2 * S1, S2));
                        } else if (!live) {
                            acc[RN + lane] += (unsigned long long)(t0 + t1 + t2);
                        }
                        ag[g][0] += mine ? s0 : 0.0;
                        ag[g][1] += mine ? s1 : 0.0;
                        ag[g][2] += mine ? s2 : 0.0;
                        if (it.sf & 256) {
                            row_out(irP, ag[g][0], ag[g][1], ag[g][2], c0, c1, c2);
                            ag[g][0] = qs ? s0 : 0.0;  // (Q's lanes start Q's sum)
                            ag[g][1] = qs ? s1 : 0.0;
                            ag[g][2] = qs ? s2 : 0.0;
                            if (it.sf & 512) {
                                row_out(irQ, ag[g][0], ag[g][1], ag[g][2], c0, c1, c2);
                                ag[g][0] = ag[g][1] = ag[g][2] = 0.0;
                            }
                        }
                    }
                }
                return true;
            }
            const int is = it.sf & 255, irP = it.ir & 0xFFFF, irQ = (int)((unsigned)it.ir >> 16);
            const bool q = lane >= is;
            // x of the lane's row (P's below s, Q's from s on); the row
            // registers hold P's from its first item on, Q's after a shared
            // one (0.35 % ahead of reading it per item, profiles/r05/pair/)
            double p0, p1, p2;
            if (it.sf & BI_NEWP) {
                p0 = uni_d(xl[irP]);
                p1 = uni_d(xl[RN + irP]);
                p2 = uni_d(xl[2 * RN + irP]);
                cx0 = p0, cx1 = p1, cx2 = p2;
            } else {
                p0 = cx0, p1 = cx1, p2 = cx2;
            }
            double c0 = p0, c1 = p1, c2 = p2;
            if (is < 64) {
                const double q0 = uni_d(xl[irQ]), q1 = uni_d(xl[RN + irQ]), q2 = uni_d(xl[2 * RN + irQ]);
                c0 = q ? q0 : p0;
                c1 = q ? q1 : p1;
                c2 = q ? q2 : p2;
                cx0 = q0, cx1 = q1, cx2 = q2;
            }
            const double xj0 = xl[rr], xj1 = xl[RN + rr], xj2 = xl[2 * RN + rr];
            sym_wait9<9 * D>(vv);
            if constexpr (CP) {  // (the entries the stream leaves out are exact zeros)
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int g = brick_slot_pair(t);
                    if (g >= 0) vv[t] = (rrk >> (16 + g)) & 1 ? 0.0 : vv[t];
                }
                // (the sums below are compiled from opaque registers, as
                // after the wait alone, so the compiler contracts them as in
                // the full stream's kernel; tests/test_gpu_box_zeros.py
                // holds y to the full stream's bits)
                sym_opaque9(vv);
            }
            // B x_j into the row, B^T x_i into row j (lanes past the row's end
            // and the diagonal block add into their dummy slot)
            const int kk = q ? (int)((unsigned)it.kb >> 16) + lane - is : (it.kb & 0xFFFF) + lane;
            const bool live = kk < (q ? (int)((unsigned)it.mu >> 16) : (it.mu & 0xFFFF));
            const int rt = live && kk > 0 ? rr : RN + lane;
            const double s0 = vv[0] * xj0 + vv[1] * xj1 + vv[2] * xj2;
            const double s1 = vv[3] * xj0 + vv[4] * xj1 + vv[5] * xj2;
            const double s2 = vv[6] * xj0 + vv[7] * xj1 + vv[8] * xj2;
            const double t0 = vv[0] * c0 + vv[3] * c1 + vv[6] * c2;
            const double t1 = vv[1] * c0 + vv[4] * c1 + vv[7] * c2;
            const double t2 = vv[2] * c0 + vv[5] * c1 + vv[8] * c2;
            if (!(probe & 1)) {  // (timing probe 1: no transposed adds)
                atomicAdd(&acc[rt], fx_of(t0 * S1, S2));
                atomicAdd(&acc[RS + rt], fx_of(t1 * S1, S2));
                atomicAdd(&acc[2 * RS + rt], fx_of(t2 * S1, S2));
            } else if (!live) {
                acc[RN + lane] += (unsigned long long)(t0 + t1 + t2);
            }
            const bool mine = live && !q;  // (P's lanes)
            acc0 += mine ? s0 : 0.0;
            acc1 += mine ? s1 : 0.0;
            acc2 += mine ? s2 : 0.0;
            if (it.sf & 256) {
                // (DOT: P's x in every lane -- in the item P shares with Q the
                // lanes from s on still hold their parts of P's full passes,
                // and their c is Q's x)
                row_out(irP, acc0, acc1, acc2, p0, p1, p2);
                // (Q's lanes start Q's sum)
                const bool qs = live && q;
                acc0 = qs ? s0 : 0.0;
                acc1 = qs ? s1 : 0.0;
                acc2 = qs ? s2 : 0.0;
                if (it.sf & 512) {
                    row_out(irQ, acc0, acc1, acc2, c0, c1, c2);
                    acc0 = acc1 = acc2 = 0.0;
                }
            }
            return true;
        };
        while (step(v0, r0, i0, v1, r1, i1) && step(v1, r1, i1, v0, r0, i0)) {
        }
    }
    // the last (re-read) loads land before their registers are reused
    sym_wait9<0>(v0);
    sym_wait9<0>(v1);
    __syncthreads();
    KLE_PROBE_TS(ts2)
    // 4. the region's transposed sums, once, [entry][3] (coalesced; nodes
    // off the lattice are never read)
    double *dst = ws + wsoff;
    double ds = 0.0;  // DOT: this thread's (region sum, x)
    for (int t = threadIdx.x; t < 3 * RN; t += NT) {
        const int k = t / 3, c = t - 3 * k;
        const int rz = k / (RX * RY), rem = k - rz * RX * RY, ry = rem / RX, rx = rem - ry * RX;
        const int gx = ox + rx, gy = oy + ry, gz = oz + rz;
        if (gx < 0 || gx >= Lx || gy < 0 || gy >= Ly || gz + zo < 0 || gz >= Lz + hp) continue;
        const double v = fx_to_d(acc[c * RS + k]) * T1 * T2;
        dst[t] = v;
        if constexpr (DOT) ds += v * xl[c * RN + k];
    }
    if constexpr (DOT) {
        // fixed order: lanes (xor tree), then waves in order
        double s = ds + dr;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) wred[w] = s;  // (wred's scale inputs were read before the item loop)
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
#pragma unroll
            for (int q = 0; q < WV; ++q) t += wred[q];
            dpart[b] = t;
        }
    }
    KLE_PROBE_TS_END5(b, ts0, ts1, ts2, ts0 + pmx[0], ts0 + pmx[1], ts0 + pmx[2])
#ifdef KLE_PROBE_BUILD
    if (probe_ts && threadIdx.x == 0 && (int64_t)b < probe_cap)  // (the waves' start spread, 10 ns units)
        probe_ts[8 * (int64_t)b] |= (unsigned long long)(pmx[3] - (unsigned)ts0) << 32;
#endif
}

// y[0 .. n) += r: the lower neighbour's sums for this slab's lowest nodes
// (the reverse halo), added last -- after the bricks', in a fixed order
__global__ void k_brick_add_recv(int64_t n, const double *__restrict__ r, double *__restrict__ y,
                                 const int *__restrict__ istate)
{
    if (istate && istate[I_REASON] != 0) return;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) y[t] += r[t];
}

// Per brick: eb with 2^eb > the largest, over its region nodes j, of
//   sum over the brick's rows i != j with j in i's stored blocks of
//   max_b sum_a |B_ij[a][b]|   (the transposed adds, each <= that x max|x|)
// + (j owned by the brick) max_a sum over row j's stored blocks of sum_b |B[a][b]|
// (its direct sum), so no region sum can exceed 2^61 at the scale 2^(61-E),
// E = eb + (exponent of max |x| over the region).  Fixed summation order.
__global__ __launch_bounds__(256) void k_brick_bound(int Lx, int Ly, int Lz, int zo, int hp,
                                                     const BrickDesc *__restrict__ bd, const int *__restrict__ rowbox,
                                                     const int *__restrict__ smu, const int64_t *__restrict__ svptr,
                                                     const double *__restrict__ sval, int P,
                                                     const int *__restrict__ owner, int *__restrict__ ebo,
                                                     const int64_t *__restrict__ vptr, const int *__restrict__ rowptr,
                                                     const int *__restrict__ rowcnt, const double *__restrict__ val)
{
    // (val: the compact stream holds no entry at a fixed place -- the same
    // values from the full storage, block k0 + kk of the row; what the
    // stream leaves out adds |0.0|)
    auto entry = [&](int64_t i, const double *v, int t, int kk, int mu) -> double {
        if (!val) return v[vofs(1, 9, t, kk, mu, mu)];
        const int mp = rowptr[i + 1] - rowptr[i], m = rowcnt ? rowcnt[i] : mp;
        return val[vptr[i] + vofs(1, 9, t, m - mu + kk, m, mp)];
    };
    __shared__ double wred[256];
    const int b = blockIdx.x;
    const BrickDesc D = bd[b];
    const int RN = D.RX * D.RY * D.RZ;
    const int64_t Lxy = (int64_t)Lx * Ly;
    double wm = 0.0;
    for (int k = threadIdx.x; k < RN; k += 256) {
        const int rz = k / (D.RX * D.RY), rem = k - rz * D.RX * D.RY, ry = rem / D.RX, rx = rem - ry * D.RX;
        const int gx = D.ox + rx, gy = D.oy + ry, gz = D.oz + rz;  // (owned z)
        if (gx < 0 || gx >= Lx || gy < 0 || gy >= Ly || gz + zo < 0 || gz >= Lz + hp) continue;
        double s = 0.0;
        // rows i of the brick whose boxes may hold j: within P of it, not above it
        for (int iz = max(D.z0, gz - P); iz <= min(D.z0 + D.nz - 1, gz); ++iz)
            for (int iy = max(D.y0, gy - P); iy <= min(D.y0 + D.ny - 1, gy + P); ++iy)
                for (int ix = max(D.x0, gx - P); ix <= min(D.x0 + D.nx - 1, gx + P); ++ix) {
                    const int64_t i = ix + (int64_t)Lx * iy + Lxy * iz;
                    if (owner[i] != b) continue;  // (a ragged brick's bounding box holds others' rows)
                    const int64_t base = rowbox[2 * i];
                    const int d = rowbox[2 * i + 1];
                    const int bze = (int)(base / Lxy), by = (int)((base - bze * Lxy) / Lx);
                    const int bx = (int)(base - bze * Lxy - (int64_t)by * Lx), bz = bze - zo;
                    const int bnx = d & 255, bny = (d >> 8) & 255, bnz = (d >> 16) & 255;
                    if (gx < bx || gx >= bx + bnx || gy < by || gy >= by + bny || gz < bz || gz >= bz + bnz) continue;
                    const int k0 = (ix - bx) + bnx * ((iy - by) + bny * (iz - bz));
                    const int kj = (gx - bx) + bnx * ((gy - by) + bny * (gz - bz));
                    if (kj <= k0) continue;  // (lower triangle or the diagonal block)
                    const int mu = bnx * bny * bnz - k0, kk = kj - k0;
                    const double *v = sval + svptr[i];
                    double bmax = 0.0;
#pragma unroll
                    for (int bb = 0; bb < 3; ++bb) {
                        double cs = 0.0;
#pragma unroll
                        for (int a = 0; a < 3; ++a) cs += fabs(entry(i, v, a * 3 + bb, kk, mu));
                        bmax = fmax(bmax, cs);
                    }
                    s += bmax;
                }
        if (gz < Lz && owner[gx + (int64_t)Lx * gy + Lxy * gz] == b) {
            // the row's own direct sum
            const int64_t j = gx + (int64_t)Lx * gy + Lxy * gz;
            const int mu = smu[j];  // (stored blocks of row j)
            const double *v = sval + svptr[j];
            double rmax = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                double rs = 0.0;
                for (int kk = 0; kk < mu; ++kk)
#pragma unroll
                    for (int bb = 0; bb < 3; ++bb) rs += fabs(entry(j, v, a * 3 + bb, kk, mu));
                rmax = fmax(rmax, rs);
            }
            s += rmax;
        }
        wm = fmax(wm, s);
    }
    wred[threadIdx.x] = wm;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) wred[threadIdx.x] = fmax(wred[threadIdx.x], wred[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int e = -1000;  // (an all-zero brick)
        if (wred[0] > 0.0) (void)frexp(wred[0], &e);
        ebo[b] = e;
    }
}

// ---------------------------------------------------------------------------
// host side

// the ghost planes below (zo) and above (hp) the owned lattice (z slabs at N > 1)
struct BrickGhost { int zo, hp; };
static BrickGhost brick_ghost_planes(const kle_mat *A)
{
    const int64_t plane3 = 3 * A->row_lat[0] * A->row_lat[1];
    return {(int)(A->ghost_lo / plane3), (int)(A->ghost_hi / plane3)};
}

int brick_setup(kle_mat *A, const std::vector<int> &rb, const std::vector<int> &cnt, const std::vector<int> &srow,
                int P, std::vector<int64_t> &svptr_out, std::string &why, void **plan_out,
                const std::vector<unsigned char> &rbits)
{
    *plan_out = nullptr;
    if (A->ghost_lo + 3 * A->nrows + A->ghost_hi >= (int64_t)1 << 29) {  // (the fill's 32-bit byte offsets)
        why = "brick SpMV: 2^29 / 3 ext nodes or more";
        return 0;
    }
    auto bp = std::make_unique<BrickPlan>();
    // k whole rounds of one brick per CU, k from spmv_brick_rounds up to the
    // fewest whose largest region fits the LDS (config 4, p = 6 on one GPU:
    // 4 rounds; one round at p = 4 and for p = 6 z slabs of 8 ranks)
    for (int rounds = std::max(1, g_tune.spmv_brick_rounds); rounds <= BRICK_MAX_ROUNDS; ++rounds) {
        *bp = brick_plan_inputs(rbits);
        try {  // (no exception may cross the C ABI: a planner failure is a refusal)
            why = brick_plan((int)A->row_lat[0], (int)A->row_lat[1], (int)A->row_lat[2], brick_ghost_planes(A).hp,
                             std::max(1, A->ctx->num_cus), g_tune.spmv_brick_max, rounds, g_tune.spmv_brick_split, cnt,
                             srow, P, *bp);
        } catch (const std::exception &e) {
            why = std::string("brick planner: ") + e.what();
        }
        if (why.empty() || g_tune.spmv_brick_max > 0 || g_tune.spmv_brick_split > 0 ||
            why.find("fits the LDS") == std::string::npos)
            break;
    }
    if (!why.empty()) return 0;
    svptr_out = bp->svb;
    *plan_out = bp.release();
    return 0;
}

// ---------------------------------------------------------------------------
// Row dedup of the value stream.  On a box mesh every element is the same
// brick, so the assembled K repeats a few distinct rows (by the node's place
// in its element and the Dirichlet faces its elements touch; in the compact
// stream also by its role in a unit) over the whole lattice, once the
// assembly makes translated rows the same bits (kle_assemble.hip
// asm_box_uniform).  After the pack: a hash per bricked row
// proposes groups of equal rows, a word-by-word comparison with the group's
// first row (the smallest natural index: the same on every run) decides, and
// the kept rows are copied into a new, smaller array; the descriptors of the
// others point at their representative's copy.  The kernel reads the same
// values in the same order, so the product is what the full stream gives, bit
// for bit.

__device__ __forceinline__ unsigned long long dd_mix(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// one wave per listed row: two 64-bit sums of position-keyed mixes of its
// len[r] words from start[r] (sums: no order to fix)
__global__ __launch_bounds__(256) void k_brick_row_hash(int64_t nr, const int64_t *__restrict__ start,
                                                        const int *__restrict__ len, const double *__restrict__ sval,
                                                        unsigned long long *__restrict__ h)
{
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= nr) return;
    const unsigned long long *v = reinterpret_cast<const unsigned long long *>(sval + start[r]);
    unsigned long long a = 0, b = 0;
    for (int k = lane; k < len[r]; k += 64) {
        const unsigned long long w = v[k], p = (unsigned long long)(k + 1);
        a += dd_mix(w ^ (p * 0x9e3779b97f4a7c15ull));
        b += dd_mix((w + 0xd1b54a32d192ed03ull) ^ (p * 0xc2b2ae3d27d4eb4full));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    if (lane == 0) {
        h[2 * r] = a;
        h[2 * r + 1] = b;
    }
}

// one wave per listed row with a representative rep[r] != r: differs[r] = 1
// unless its len[r] words equal the representative's
__global__ __launch_bounds__(256) void k_brick_row_cmp(int64_t nr, const int64_t *__restrict__ start,
                                                       const int *__restrict__ len, const int *__restrict__ rep,
                                                       const double *__restrict__ sval, int *__restrict__ differs)
{
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= nr) return;
    const int q = rep[r];
    if (q < 0 || q >= nr || q == r) return;
    if (len[q] != len[r]) {
        if (lane == 0) differs[r] = 1;
        return;
    }
    const unsigned long long *v = reinterpret_cast<const unsigned long long *>(sval + start[r]);
    const unsigned long long *u = reinterpret_cast<const unsigned long long *>(sval + start[q]);
    bool d = false;
    for (int k = lane; k < len[r]; k += 64) d |= v[k] != u[k];
    if (__ballot(d) != 0ull && lane == 0) differs[r] = 1;
}

// one wave per listed row with dst[r] >= 0: its plen[r] doubles (the padding
// with them) from src + start[r] to out + dst[r]
__global__ __launch_bounds__(256) void k_brick_row_copy(int64_t nr, const int64_t *__restrict__ start,
                                                        const int *__restrict__ plen, const int64_t *__restrict__ dst,
                                                        const double *__restrict__ src, double *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= nr || dst[r] < 0) return;
    const double *s = src + start[r];
    double *o = out + dst[r];
    for (int k = lane; k < plen[r]; k += 64) o[k] = s[k];
}

// The dedup (spmv_brick_dedup), after the pack and before anything else of
// brick_finish: on success the plan's descriptors, bricks and svb, d_svptr,
// d_sval and snvals describe the unique array; where it does not pay (fewer
// than half of the bricked bytes saved), does not fit the descriptors' 23
// bits or the memory is short, everything stays as it was.
static int brick_dedup(kle_mat *A, BrickPlan &bp)
{
    kle_ctx *c = A->ctx;
    const int64_t n = A->nrows, Lx = A->row_lat[0], Ly = A->row_lat[1];
    const bool compact = !bp.rbits.empty();
    struct Row {
        int64_t i, rr;  // natural index, descriptor index
        int len, plen;
    };
    std::vector<Row> rows;
    for (const BrickDesc &D : bp.bricks)
        for (int r = 0; r < D.nr; ++r) {
            const int64_t rr = (int64_t)D.rstart + r;
            if (brick_row_null(bp.rowd.data(), rr)) continue;
            const int dw = brick_row_word(bp.rowd[2 * rr]);
            const int64_t len = compact ? brick_row_doubles(dw) : 9 * (int64_t)brick_row_box(dw, false).mu();
            const int64_t i = brick_ir_node(D, brick_row_ir(bp.rowd.data(), rr), Lx, Ly);
            if (i < 0 || i >= n || len < 1) return 0;  // (brick_validate names what is wrong)
            const int64_t v0 = D.vbase + brick_row_off(bp.rowd.data(), rr) * 16;
            const int64_t plen = (len + 15) & ~int64_t(15);
            if (v0 != bp.svb[i] || v0 < 0 || v0 + plen > A->snvals) return 0;
            rows.push_back({i, rr, (int)len, (int)plen});
        }
    const int64_t nr = (int64_t)rows.size();
    if (nr < 2 || nr > INT_MAX / 2) return 0;
    std::vector<int64_t> hstart(nr);
    std::vector<int> hlen(nr), hplen(nr);
    for (int64_t r = 0; r < nr; ++r) {
        hstart[r] = bp.svb[rows[r].i];
        hlen[r] = rows[r].len;
        hplen[r] = rows[r].plen;
    }
    DevTmp<int64_t> dstart, ddst;  // (freed on every way out)
    DevTmp<int> dlen, dplen, drep, ddiff;
    DevTmp<unsigned long long> dh;
    if (!dstart.alloc(nr) || !ddst.alloc(nr) || !dlen.alloc(nr) || !dplen.alloc(nr) || !drep.alloc(nr) ||
        !ddiff.alloc(nr) || !dh.alloc(2 * nr)) {
        (void)hipGetLastError();
        return 0;
    }
    const dim3 grid((unsigned)((nr + 3) / 4));
    KLE_TRY(h2d(dstart.p, hstart.data(), sizeof(int64_t) * nr));
    KLE_TRY(h2d(dlen.p, hlen.data(), sizeof(int) * nr));
    KLE_TRY(h2d(dplen.p, hplen.data(), sizeof(int) * nr));
    // 1. hash; equal keys (length, hash) grouped on the host, the smallest
    // natural index first.  A row's box and its role in its unit are not part
    // of the key: each row is read through its own descriptor, only the place
    // of its values is shared, so equal bytes are all the sharing needs (a
    // unit's second row of the compact stream, whose last partial pass comes
    // first, has other bytes than the same row as a first one)
    hipLaunchKernelGGL(k_brick_row_hash, grid, dim3(256), 0, c->stream, nr, dstart.p, dlen.p, A->d_sval, dh.p);
    KLE_HIP(hipGetLastError());
    std::vector<unsigned long long> hh(2 * nr);
    KLE_HIP(hipStreamSynchronize(c->stream));
    KLE_HIP(hipMemcpy(hh.data(), dh.p, sizeof(unsigned long long) * 2 * nr, hipMemcpyDeviceToHost));
    std::vector<int> ord(nr), rep(nr);
    for (int64_t r = 0; r < nr; ++r) ord[r] = (int)r;
    auto key_less = [&](int a, int b) {
        const Row &x = rows[a], &y = rows[b];
        if (x.len != y.len) return x.len < y.len;
        if (hh[2 * a] != hh[2 * b]) return hh[2 * a] < hh[2 * b];
        if (hh[2 * a + 1] != hh[2 * b + 1]) return hh[2 * a + 1] < hh[2 * b + 1];
        return x.i < y.i;
    };
    auto key_eq = [&](int a, int b) {
        const Row &x = rows[a], &y = rows[b];
        return x.len == y.len && hh[2 * a] == hh[2 * b] && hh[2 * a + 1] == hh[2 * b + 1];
    };
    std::sort(ord.begin(), ord.end(), key_less);
    for (int64_t k = 0, g = 0; k < nr; ++k) {
        if (!key_eq(ord[g], ord[k])) g = k;
        rep[ord[k]] = ord[g];
    }
    // 2. the comparison decides: a row that differs anywhere keeps its own storage
    KLE_TRY(h2d(drep.p, rep.data(), sizeof(int) * nr));
    KLE_HIP(hipMemsetAsync(ddiff.p, 0, sizeof(int) * nr, c->stream));
    hipLaunchKernelGGL(k_brick_row_cmp, grid, dim3(256), 0, c->stream, nr, dstart.p, dlen.p, drep.p, A->d_sval, ddiff.p);
    KLE_HIP(hipGetLastError());
    std::vector<int> diff(nr);
    KLE_HIP(hipStreamSynchronize(c->stream));
    KLE_HIP(hipMemcpy(diff.data(), ddiff.p, sizeof(int) * nr, hipMemcpyDeviceToHost));
    // 3. the unique array: the kept rows in brick order, each aligned to 16
    // doubles, then the one-block rows' values (9 doubles each) as before
    std::vector<int64_t> dst(nr, -1);
    int64_t cur = 0, before = 0, kept = 0;
    for (int64_t r = 0; r < nr; ++r) {
        before += rows[r].plen;
        if (rep[r] != r && !diff[r]) continue;
        rep[r] = (int)r;
        if ((cur >> 4) >= BRICK_ROW_NULL) return 0;  // (past what 23 bits x 16 doubles address: 1 GiB)
        dst[r] = cur;
        cur += rows[r].plen;
        ++kept;
    }
    if (2 * cur > before) return 0;  // (fewer than half of the bricked bytes saved)
    const int64_t ubytes = 8 * cur, ns = (int64_t)bp.srows.size();
    const int64_t s_old = ns ? bp.svb[bp.srows[0]] : 0, s_new = cur;
    for (int64_t k = 0; k < ns; ++k)
        if (bp.svb[bp.srows[k]] != s_old + 9 * k || s_old + 9 * ns > A->snvals) return 0;
    const int64_t total = (cur + 9 * ns + 15) & ~int64_t(15);
    double *old = A->d_sval;
    void *old_raw = A->sval_raw ? A->sval_raw : (void *)old;
    const size_t old_cap = A->sval_cap;
    if (sval_alloc(A, sizeof(double) * std::max<int64_t>(total, 1)) != 0) {
        A->d_sval = old;
        A->sval_raw = old_raw == (void *)old ? nullptr : old_raw;
        A->sval_cap = old_cap;
        return 0;
    }
    // (until the copy is done the matrix keeps its full stream: an error
    // return frees exactly one of the two arrays)
    DevTmp<double> nv(A->d_sval);
    A->d_sval = old;
    A->sval_raw = old_raw == (void *)old ? nullptr : old_raw;
    KLE_TRY(h2d(ddst.p, dst.data(), sizeof(int64_t) * nr));
    KLE_HIP(hipMemsetAsync(nv.p, 0, sizeof(double) * std::max<int64_t>(total, 1), c->stream));
    hipLaunchKernelGGL(k_brick_row_copy, grid, dim3(256), 0, c->stream, nr, dstart.p, dplen.p, ddst.p, old, nv.p);
    KLE_HIP(hipGetLastError());
    if (ns)
        KLE_HIP(hipMemcpyAsync(nv.p + s_new, old + s_old, sizeof(double) * 9 * ns, hipMemcpyDeviceToDevice, c->stream));
    // the tables: every row's place in the unique array
    std::vector<int64_t> svb(bp.svb);
    for (int64_t r = 0; r < nr; ++r) svb[rows[r].i] = dst[rep[r]];
    for (int64_t k = 0; k < ns; ++k) svb[bp.srows[k]] = s_new + 9 * k;
    svb[n] = total;
    KLE_TRY(h2d(A->d_svptr, svb.data(), sizeof(int64_t) * (n + 1)));
    KLE_HIP(hipStreamSynchronize(c->stream));
    (void)hipFree(old_raw);
    A->d_sval = nv.release();
    A->sval_raw = nullptr;
    A->sval_cap = 0;
    A->snvals = total;
    bp.svb.swap(svb);
    for (int64_t r = 0; r < nr; ++r) brick_row_set_off(bp.rowd.data(), rows[r].rr, dst[rep[r]] >> 4);
    for (BrickDesc &D : bp.bricks) D.vbase = 0;
    bp.dedup = true;
    // units class by class, handed out as runs (the full layout: a unit's
    // items depend on its rows' boxes and value offsets alone)
    if (!compact) {
        brick_runs_build(bp, BRICK_RUN_G);
        if (!brick_runs_pay(bp.run_item_loads, bp.run_items)) brick_runs_clear(bp);  // (too little repeats inside the bricks)
    }
    A->brick_dedup = 1;
    A->brick_unique_rows = kept;
    A->brick_unique_bytes = ubytes;
    if (const char *e = getenv("KLE_TIMING"))
        if (atoi(e))
            fprintf(stderr, "[kle brick r%d] dedup: %lld of %lld rows kept, %.1f of %.1f MB\n", c->rank, (long long)kept,
                    (long long)nr, ubytes * 1e-6, 8e-6 * before);
    return 0;
}

// ---------------------------------------------------------------------------
// brick_finish's steps, in its order

// the row descriptors, brick q's at row q rstride (the kernel's address needs
// no load); the rows past a brick's own repeat its last unit (never read:
// every read is of a unit < nr / 2)
static int brick_put_rows(kle_mat *A, const BrickPlan &bp, int rstride)
{
    const int NB = (int)bp.bricks.size();
    std::vector<int> pad((size_t)2 * std::max<int64_t>(1, (int64_t)NB * rstride), 0);
    for (int q = 0; q < NB; ++q) {
        const BrickDesc &D = bp.bricks[q];
        int *dst = pad.data() + 2 * (int64_t)q * rstride;
        std::copy(bp.rowd.begin() + 2 * (int64_t)D.rstart, bp.rowd.begin() + 2 * ((int64_t)D.rstart + D.nr), dst);
        for (int r = D.nr; r < rstride && D.nr >= 2; ++r) {
            dst[2 * r] = dst[2 * (D.nr - 2 + (r & 1))];
            dst[2 * r + 1] = dst[2 * (D.nr - 2 + (r & 1)) + 1];
        }
    }
    KLE_TRY(h2d(A->d_browd, pad.data(), sizeof(int) * pad.size()));
    A->brick_rstride = rstride;
    return 0;
}

// the runs' records, brick q's at q rs (as the row descriptors): the class's
// four descriptor words without their region-index bytes, the count, each
// unit's irA | irB << 16 -- all taken from the validated descriptors and
// runs; the slots past a brick's runs are never read (every read is of a
// run < nrun)
static int brick_put_runs(kle_mat *A, const BrickPlan &bp)
{
    const int NB = (int)bp.bricks.size(), G = bp.run_cap, RW = brick_run_words(G);
    const int *rowd = bp.rowd.data();
    int rs = 1;
    for (const BrickDesc &D : bp.bricks) rs = std::max(rs, D.nrun);
    std::vector<int> rec((size_t)NB * rs * RW, 0);
    for (int q = 0; q < NB; ++q) {
        const BrickDesc &D = bp.bricks[q];
        for (int r = 0; r < D.nrun; ++r) {
            int *o = rec.data() + ((size_t)q * rs + r) * RW;
            const int rv = bp.runs[bp.run_first[q] + r];
            const int first = brick_run_first(rv), cnt = brick_run_count(rv);
            const int *ord = bp.run_order.data() + D.rstart / 2 + first;
            const int64_t r0 = (int64_t)D.rstart + 2 * ord[0];
            for (int k = 0; k < 4; ++k) o[k] = brick_row_word(rowd[2 * r0 + k]);
            o[4] = cnt;
            for (int g = 0; g < cnt; ++g) {
                const int64_t ra = (int64_t)D.rstart + 2 * ord[g];
                const int irb = brick_row_null(rowd, ra + 1) ? 0 : brick_row_ir(rowd, ra + 1);
                o[5 + g] = brick_row_ir(rowd, ra) | irb << 16;
            }
        }
    }
    if (hipMalloc(&A->d_bruns, sizeof(int) * std::max<size_t>(rec.size(), 1)) != hipSuccess) {
        (void)hipGetLastError();
        A->d_bruns = nullptr;
        return fail(KLE_ERR_MEM, "out of device memory for the brick runs");
    }
    KLE_TRY(h2d(A->d_bruns, rec.data(), sizeof(int) * rec.size()));
    A->brick_run_cap = G;
    A->brick_run_stride = rs;
    A->brick_runs = (int64_t)bp.runs.size();
    A->brick_run_units = bp.run_units;
    A->brick_run_items = bp.run_items;
    A->brick_run_item_loads = bp.run_item_loads;
    return 0;
}

// the gather's run lists (kle_brick.hpp brick_gather_runs)
static int brick_put_gather(kle_mat *A, const BrickPlan &bp)
{
    const BrickGhost gp = brick_ghost_planes(A);
    std::vector<int> runptr, rstart;
    std::vector<unsigned long long> rmask;
    if (!brick_gather_runs(bp, A->row_lat[0], A->row_lat[1], A->row_lat[2], gp.zo, gp.hp, runptr, rstart, rmask))
        return fail(KLE_ERR_SUP, "brick sums beyond 2^31 doubles");
    const int64_t ns = (int64_t)runptr.size() - 1;
    if (hipMalloc(&A->d_sgptr, sizeof(int) * (ns + 1)) != hipSuccess ||
        hipMalloc(&A->d_sgidx, sizeof(int) * rstart.size()) != hipSuccess ||
        hipMalloc(&A->d_sgmask, sizeof(unsigned long long) * rmask.size()) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KLE_ERR_MEM, "out of device memory for the brick gather runs");
    }
    KLE_TRY(h2d(A->d_sgptr, runptr.data(), sizeof(int) * (ns + 1)));
    KLE_TRY(h2d(A->d_sgidx, rstart.data(), sizeof(int) * rstart.size()));
    KLE_TRY(h2d(A->d_sgmask, rmask.data(), sizeof(unsigned long long) * rmask.size()));
    A->brick_gparts = (int)(runptr[ns] / std::max<int64_t>(ns, 1));  // (runs per 64 rows, for the log)
    A->gather_rps = (int)((runptr[ns] + ns - 1) / std::max<int64_t>(ns, 1));
    return 0;
}

// the one-block rows per 64-row slice of the owned rows (the gather forms
// their B_ii x_i)
static int brick_put_singles(kle_mat *A, const BrickPlan &bp)
{
    const int64_t nso = (A->nrows + 63) / 64;
    std::vector<unsigned long long> sm(nso, 0ull);
    for (int64_t i : bp.srows) sm[i >> 6] |= 1ull << (i & 63);
    if (hipMalloc(&A->d_ssingle, sizeof(unsigned long long) * nso) != hipSuccess) {
        (void)hipGetLastError();
        A->d_ssingle = nullptr;
        return fail(KLE_ERR_MEM, "out of device memory for the brick gather's one-block rows");
    }
    return h2d(A->d_ssingle, sm.data(), sizeof(unsigned long long) * nso);
}

// the bound exponents (k_brick_bound) into the descriptors; dmu: 2 n ints of
// scratch, freed here
static int brick_put_bounds(kle_mat *A, BrickPlan &bp, DevTmp<int> &dmu)
{
    kle_ctx *c = A->ctx;
    const int NB = (int)bp.bricks.size();
    const int64_t n = A->nrows;
    const bool compact = !bp.rbits.empty();
    // stored blocks per row (the bound's direct sums) from the row
    // descriptors | owning brick per row (-1: a one-block row)
    std::vector<int> hmu(2 * n, 0);
    int *howner = hmu.data() + n;
    std::fill(howner, howner + n, -1);
    for (int64_t i : bp.srows) hmu[i] = 1;
    for (int q = 0; q < NB; ++q) {
        const BrickDesc &D = bp.bricks[q];
        for (int r = 0; r < D.nr; ++r) {
            const int64_t rr = (int64_t)D.rstart + r;
            if (brick_row_null(bp.rowd.data(), rr)) continue;
            const int64_t i = brick_ir_node(D, brick_row_ir(bp.rowd.data(), rr), A->row_lat[0], A->row_lat[1]);
            hmu[i] = brick_row_box(bp.rowd[2 * rr], compact).mu();
            howner[i] = q;
        }
    }
    KLE_TRY(h2d(dmu.p, hmu.data(), sizeof(int) * 2 * n));
    const BrickGhost gp = brick_ghost_planes(A);
    if (NB > 0)  // (every row of one block: no brick at all, the gather forms y)
        hipLaunchKernelGGL(k_brick_bound, dim3((unsigned)NB), dim3(256), 0, c->stream, (int)A->row_lat[0],
                           (int)A->row_lat[1], (int)A->row_lat[2], gp.zo, gp.hp,
                           reinterpret_cast<const BrickDesc *>(A->d_bdesc), A->d_rowbox, dmu.p, A->d_svptr, A->d_sval,
                           A->sym_P, dmu.p + n, A->d_stile_e, A->d_vptr, A->d_rowptr, A->d_rowcnt,
                           compact ? A->d_val : nullptr);
    KLE_HIP(hipGetLastError());
    std::vector<int> eb(NB);
    KLE_HIP(hipStreamSynchronize(c->stream));
    KLE_HIP(hipMemcpy(eb.data(), A->d_stile_e, sizeof(int) * NB, hipMemcpyDeviceToHost));
    (void)hipFree(dmu.release());
    for (int q = 0; q < NB; ++q) bp.bricks[q].eb = eb[q];
    return h2d(A->d_bdesc, bp.bricks.data(), sizeof(BrickDesc) * NB);
}

// what the matrix reports of its bricks
static int brick_put_stats(kle_mat *A, const BrickPlan &bp)
{
    const int NB = (int)bp.bricks.size();
    const bool compact = !bp.rbits.empty();
    A->nbricks = NB;
    std::vector<int> u[3];  // (bricks along each axis: distinct first coordinates)
    for (const BrickDesc &D : bp.bricks) {
        u[0].push_back(D.x0);
        u[1].push_back(D.y0);
        u[2].push_back(D.z0);
    }
    for (int k = 0; k < 3; ++k) {
        std::sort(u[k].begin(), u[k].end());
        A->brick_dims[k] = (int)(std::unique(u[k].begin(), u[k].end()) - u[k].begin());
    }
    A->brick_model_us = bp.model_us;
    A->brick_lds = (int)bp.lds;
    A->sws_entries = bp.ws_entries;
    A->sym_brick = 1;
    A->brick_compact = compact;
    A->brick_dropped = compact ? bp.dropped : 0;
    if (const char *e = getenv("KLE_TIMING"))
        if (atoi(e) && NB > 0) {
            const BrickDesc &D = bp.bricks[0];
            fprintf(stderr, "[kle brick] %d bricks (first %d x %d x %d rows, region %d x %d x %d), LDS %zu B, "
                            "region entries %lld (%.2f per row)\n",
                    NB, D.nx, D.ny, D.nz, D.RX, D.RY, D.RZ, bp.lds, (long long)bp.ws_entries,
                    (double)bp.ws_entries / A->nrows);
        }
    return 0;
}

// after the values are in place (d_sval, d_svptr in brick layout): the brick
// tables on the device, the workspace, the bound exponents
int brick_finish(kle_mat *A, void *plan)
{
    std::unique_ptr<BrickPlan> bp(reinterpret_cast<BrickPlan *>(plan));
    const int NB = (int)bp->bricks.size();
    if (g_tune.spmv_brick_dedup && NB > 0) KLE_TRY(brick_dedup(A, *bp));
    // every address the kernel forms from the tables, checked on the host
    // first (a bad plan is an error, never a launch)
    if (const char *bad = brick_validate(*bp, A->row_lat[0], A->row_lat[1], A->row_lat[2], A->snvals, (int64_t)bp->lds))
        return fail(KLE_ERR_SUP, "brick plan: %s", bad);
    int rstride = 0;  // rows per brick in the descriptor table (the most of any brick)
    for (const BrickDesc &D : bp->bricks) rstride = std::max(rstride, D.nr);
    rstride = std::max(2, (rstride + 1) & ~1);  // (whole units of two rows, at least one)
    DevTmp<int> dmu;
    const bool nomem = hipMalloc(&A->d_bdesc, sizeof(BrickDesc) * std::max(NB, 1)) != hipSuccess ||
                       hipMalloc(&A->d_browd, sizeof(int) * 2 * std::max<int64_t>(1, (int64_t)NB * rstride)) != hipSuccess ||
                       (A->ghost_hi && hipMalloc(&A->d_sgsend, sizeof(double) * A->ghost_hi) != hipSuccess) ||
                       (A->send_lo && hipMalloc(&A->d_sgrecv, sizeof(double) * A->send_lo) != hipSuccess) ||
                       hipMalloc(&A->d_sws, sizeof(double) * std::max<int64_t>(bp->ws_doubles, 1)) != hipSuccess ||
                       hipMalloc(&A->d_stile_e, sizeof(int) * std::max(NB, 1)) != hipSuccess || !dmu.alloc(2 * A->nrows);
    (void)hipGetLastError();
    if (nomem) return fail(KLE_ERR_MEM, "out of device memory for the symmetric SpMV bricks");
    A->sws_bytes = sizeof(double) * std::max<int64_t>(bp->ws_doubles, 1);
    KLE_TRY(h2d(A->d_bdesc, bp->bricks.data(), sizeof(BrickDesc) * NB));
    KLE_TRY(brick_put_rows(A, *bp, rstride));
    if (!bp->runs.empty()) KLE_TRY(brick_put_runs(A, *bp));
    KLE_TRY(brick_put_gather(A, *bp));
    if (!bp->srows.empty()) KLE_TRY(brick_put_singles(A, *bp));
    KLE_TRY(brick_put_bounds(A, *bp, dmu));
    return brick_put_stats(A, *bp);
}

void brick_plan_free(void *plan) { delete reinterpret_cast<BrickPlan *>(plan); }

void brick_pack_desc(const void *plan, const std::vector<int> &srow, std::vector<int> &pd)
{
    const BrickPlan *bp = reinterpret_cast<const BrickPlan *>(plan);
    const size_t n = srow.size();
    pd.assign(n, 0);
    for (size_t i = 0; i < n; ++i)
        pd[i] = brick_dw_bits(srow[i], bp->rbits.empty() ? 0 : bp->rbits[i]) | (bp->second.empty() ? 0 : bp->second[i] << 24);
    for (int64_t i : bp->srows) pd[i] |= 1 << 25;
}

void brick_drop(kle_mat *A)
{
    for (void *q : {A->d_bdesc, (void *)A->d_browd, (void *)A->d_bruns})
        if (q) (void)hipFree(q);
    brick_forget(A);
}

void brick_forget(kle_mat *A)
{
    A->d_bdesc = nullptr;
    A->d_browd = nullptr;
    A->d_bruns = nullptr;
    A->brick_run_cap = A->brick_run_stride = 0;
    A->brick_runs = A->brick_run_units = A->brick_run_items = A->brick_run_item_loads = 0;
    A->nbricks = 0;
    A->brick_gparts = 0;
    A->brick_dims[0] = A->brick_dims[1] = A->brick_dims[2] = 0;
    A->brick_model_us = 0.0;
    A->brick_lds = 0;
    A->sym_brick = 0;
    A->brick_compact = 0;
    A->brick_dropped = 0;
    A->brick_dedup = 0;
    A->brick_unique_rows = A->brick_unique_bytes = 0;
    A->sym_gbrick = 0;
    A->brick_lds_u = 0;
}

// the brick kernel of a matrix: compact or full stream; a deduplicated value
// array (its loads cached unless spmv_brick_dedup_nt); dot: (A x, x) shares
using BrickKern = void (*)(int, int, int, int, int, int, const BrickDesc *, const int2 *, const double *, const double *,
                           double *, double *, double *, const int *KLE_PROBE_PARAM);
// the product takes runs (G of the kernel): built for this matrix, and for the cap the kernel is compiled for
static bool brick_uses_runs(const kle_mat *A)
{
#ifdef KLE_PROBE_BUILD
    if (g_tune.spmv_sym_probe & 256) return false;  // (timing probe 256: unit by unit, as without the runs)
#endif
    return A->brick_dedup && !A->brick_compact && A->d_bruns && A->brick_run_cap == BRICK_RUN_G;
}
template <bool DOT, bool CP, bool DD, bool NTL, int G = 0>
constexpr BrickKern BRICK_KERN = k_nb_spmv_sym_brick<BRICK_WV, true, DOT, CP, DD, NTL, G>;
template <bool DOT>
static BrickKern brick_kernel_of(const kle_mat *A)
{
    const bool nt = g_tune.spmv_brick_dedup_nt != 0;
    if constexpr (!DOT)  // (runs of same-class units: the full layout, no DOT)
        if (brick_uses_runs(A))
            return nt ? BRICK_KERN<DOT, false, true, true, BRICK_RUN_G> : BRICK_KERN<DOT, false, true, false, BRICK_RUN_G>;
    // [shared, nontemporal loads | shared, cached loads | every row's own stream][compact | full]
    // (named in the order the code object has always held them: a reordering moves every kernel in it)
    static constexpr BrickKern kern[3][2] = {
        {BRICK_KERN<DOT, true, true, true>, BRICK_KERN<DOT, false, true, true>},
        {BRICK_KERN<DOT, true, true, false>, BRICK_KERN<DOT, false, true, false>},
        {BRICK_KERN<DOT, true, false, true>, BRICK_KERN<DOT, false, false, true>},
    };
    return kern[!A->brick_dedup ? 2 : nt ? 0 : 1][A->brick_compact ? 0 : 1];
}
// the bricks' launch; runs: the kernel takes the runs' records and their stride
static void brick_launch(kle_mat *A, BrickKern kern, bool runs, const kle_vec *x, kle_vec *y, double *dpart,
                         const int *istate)
{
    kle_ctx *c = A->ctx;
    const BrickGhost gp = brick_ghost_planes(A);
    dyn_lds(c, reinterpret_cast<const void *>(kern), (size_t)A->brick_lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)A->nbricks), dim3(64 * BRICK_WV), (size_t)A->brick_lds, c->stream,
                       (int)A->row_lat[0], (int)A->row_lat[1], (int)A->row_lat[2], gp.zo, gp.hp,
                       runs ? A->brick_run_stride : A->brick_rstride, reinterpret_cast<const BrickDesc *>(A->d_bdesc),
                       reinterpret_cast<const int2 *>(runs ? A->d_bruns : A->d_browd), A->d_sval, x->base, A->d_sws,
                       y->d, dpart, istate KLE_PROBE_ARG);
}

int brick_spmv(kle_mat *A, const kle_vec *x, kle_vec *y, const int *istate, double *dpart, bool split)
{
    kle_ctx *c = A->ctx;
    const bool dist = c->nranks > 1 && (A->lo_rank >= 0 || A->hi_rank >= 0);
    // N > 1 (z slabs): the x ghost planes first (every brick's region fill
    // may read them); after the bricks, the upper ghost nodes' sums go to the
    // upper neighbour (MPISBAIJ's reverse scatter) on the comm stream while
    // the owned rows are summed; the lower neighbour's sums for the lowest
    // rows are added last (fixed order: y stays bitwise reproducible).  All
    // RCCL calls in the same order on every rank: forward, then reverse halo.
    if (dist)
        KLE_TRY(halo_exchange(c, x->base, x->ghost_lo, x->n_local, x->ghost_hi, x->lo_rank, x->hi_rank, x->send_lo,
                              x->send_hi, c->stream, nullptr));
    if (A->nbricks == 0) {
        // (no brick: every row of one block, formed by the gather)
    } else {
        // (a split product's (A x, x): the bricks' shares, DOT; else the gather's)
        const bool dot = split && dpart && !dist;
        brick_launch(A, dot ? brick_kernel_of<true>(A) : brick_kernel_of<false>(A), !dot && brick_uses_runs(A), x, y, dpart,
                     istate);
    }
    KLE_HIP(hipGetLastError());
    // the gather (kle_sym.hip gsym_gather): per row its direct sum in y, then
    // the runs of the regions holding it, in ascending brick order
    const int64_t n = A->nrows, ntot = n + A->ghost_hi / 3, nlo = n / 64 * 64;
    const double *xs = A->d_ssingle ? x->d : nullptr;  // (rows of one stored block: the gather's)
    if (!dist) {
        if (split) return 0;  // (the consumer gathers every row: BrickGather)
        return gsym_gather(A, y->d, 0, n, istate, dpart ? x->d : nullptr, dpart, 1, c->stream, xs);
    }
    // the slices holding upper ghost rows first (their sums: d_sgsend)
    KLE_TRY(gsym_gather(A, y->d, nlo, ntot, istate, nullptr, nullptr, 1, c->stream, xs));
    const int64_t nrecv = A->lo_rank >= 0 ? A->send_lo : 0;
    const bool ovl = A->halo_overlap != 0;
    hipStream_t cs = ovl ? c->comm_stream : c->stream;
    if (ovl) {
        KLE_HIP(hipEventRecord(c->ev_x_ready, c->stream));
        KLE_HIP(hipStreamWaitEvent(cs, c->ev_x_ready, 0));
    }
    KLE_TRY(halo_reverse(c, A->d_sgsend, A->ghost_hi, A->hi_rank, A->d_sgrecv, nrecv, A->lo_rank, cs));
    if (ovl) KLE_HIP(hipEventRecord(c->ev_halo_done, cs));
    if (split) return 0;  // (the owned rows below nlo and the received sums: the consumer's)
    return brick_gather_rest(A, x, y, istate);
}

// The rank-local part of a box-brick product, for timing it
// (kle_mat_time_local_spmv): the bricks and the gather of every row they
// touch, owned and upper ghost, with no halo either way -- the ghost x as
// they are, the upper ghost rows' sums left in the send buffer.  A slab
// part's kernel time without its neighbours (ranks sharing one GPU take
// turns); on one rank the product itself.
int brick_spmv_local(kle_mat *A, const kle_vec *x, kle_vec *y)
{
    kle_ctx *c = A->ctx;
    if (A->nbricks > 0) {
        brick_launch(A, brick_kernel_of<false>(A), brick_uses_runs(A), x, y, nullptr, nullptr);
        KLE_HIP(hipGetLastError());
    }
    const int64_t ntot = A->nrows + A->ghost_hi / 3;
    return gsym_gather(A, y->d, 0, ntot, nullptr, nullptr, nullptr, 1, c->stream, A->d_ssingle ? x->d : nullptr);
}

// The rest of a split product (brick_spmv with split): the rows [0, nlo)
// (every row on one rank) gathered, then the received reverse-halo sums added
// last -- the same operations, in the same order, as the unsplit product
// (wps_force 1: each row's runs summed in k_pipe_iter_g's order).
int brick_gather_rest(kle_mat *A, const kle_vec *x, kle_vec *y, const int *istate, int wps_force)
{
    kle_ctx *c = A->ctx;
    const bool dist = c->nranks > 1 && (A->lo_rank >= 0 || A->hi_rank >= 0);
    const int64_t n = A->nrows, nlo = dist ? n / 64 * 64 : n;
    const double *xs = A->d_ssingle ? x->d : nullptr;
    KLE_TRY(gsym_gather(A, y->d, 0, nlo, istate, nullptr, nullptr, 1, c->stream, xs, wps_force));
    if (!dist) return 0;
    const int64_t nrecv = A->lo_rank >= 0 ? A->send_lo : 0;
    if (A->halo_overlap) KLE_HIP(hipStreamWaitEvent(c->stream, c->ev_halo_done, 0));
    if (nrecv)
        hipLaunchKernelGGL(k_brick_add_recv, dim3((unsigned)((nrecv + 255) / 256)), dim3(256), 0, c->stream, nrecv,
                           A->d_sgrecv, y->d, istate);
    KLE_HIP(hipGetLastError());
    return 0;
}

// What a consumer of a split product gathers itself (k_pipe_iter_g,
// kle_ksp.hip): the run lists of the rows [0, ng), the one-block rows, and
// the received sums of the lowest rows (after the reverse halo, which the
// consumer's stream must have waited for: see brick_split_wait)
BrickGather brick_gather_src(const kle_mat *A, const kle_vec *x)
{
    const kle_ctx *c = A->ctx;
    const bool dist = c->nranks > 1 && (A->lo_rank >= 0 || A->hi_rank >= 0);
    BrickGather g;
    g.runptr = A->d_sgptr;
    g.rstart = A->d_sgidx;
    g.rmask = A->d_sgmask;
    g.ws = A->d_sws;
    g.single = A->d_ssingle;
    g.sval = A->d_sval;
    g.svptr = A->d_svptr;
    g.xs = x->d;
    g.nrows = A->nrows;
    g.ng = dist ? A->nrows / 64 * 64 : A->nrows;
    g.recv = A->d_sgrecv;
    g.nrecv = dist && A->lo_rank >= 0 ? A->send_lo : 0;
    return g;
}

}  // namespace kle
