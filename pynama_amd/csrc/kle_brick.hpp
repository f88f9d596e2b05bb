// kle_brick.hpp -- the brick decomposition of the box symmetric SpMV
// (kle_brick.hip: kernels and device set-up; kle_brick_plan.cpp: the host
// planner, also reachable on a CPU through kle_brick_plan_box).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace kle {

// per brick (device, 80 B): the bounding box of its rows in owned-lattice
// coordinates (a box, or a ragged band piece whose first and last x planes /
// y lines are partial), its row count, the region (bounding box of its rows'
// upper triangles; z in owned coordinates), its first row descriptor, the
// bound exponent of its fixed-point sums, where its values and its region
// sums live
struct BrickDesc {
    int x0, y0, z0, nx, ny, nz;
    int ox, oy, oz, RX, RY, RZ;
    int rstart, eb, nr, nrun;  // (nrun: its runs of same-class units, 0 where none are used)
    long long vbase, wsoff;
};
static_assert(sizeof(BrickDesc) == 80, "BrickDesc layout");

// A row descriptor, two ints.  Word 0: the packed row box -- dbx, dby, dbz (the
// row's place in its box), bnx, bny, bnz (the box's size), 4 bits each from
// bit 0 -- and, in its top byte, the low byte of the row's region index.
// Word 1: the row's value offset / 16 doubles (23 bits), BRICK_ROW_NULL (a
// unit's absent second row) and, in its top byte, the high byte of the region
// index.  Rows come in units of two (kle_brick_plan.cpp).  The compact value
// stream (below) puts a boundary bit above each of dbx, dby, dbz, which are
// then 3 bits.  The functions from here to brick_row_set_null are the one
// definition of this layout; every shift is unsigned.
#if defined(__HIPCC__) || defined(__CUDACC__)
#define KLE_BRICK_HD __host__ __device__
#else
#define KLE_BRICK_HD
#endif
constexpr int BRICK_ROW_NULL = 1 << 23;
constexpr int BRICK_ROW_OFF = BRICK_ROW_NULL - 1;  // (word 1: the value offset's bits)
struct BrickRowBox {
    int dbx, dby, dbz, bnx, bny, bnz;
    KLE_BRICK_HD int k0() const { return dbx + bnx * (dby + bny * dbz); }  // the row's own (first stored) block
    KLE_BRICK_HD int mu() const { return bnx * bny * bnz - k0(); }         // its stored blocks
};
// the box of a packed box word (kle_sym.hip srow, or word 0 of a descriptor);
// compact: the word carries the boundary bits
KLE_BRICK_HD inline BrickRowBox brick_row_box(int dw, bool compact)
{
    const unsigned w = (unsigned)dw, dm = compact ? 7u : 15u;
    return {(int)(w & dm), (int)((w >> 4) & dm), (int)((w >> 8) & dm),
            (int)((w >> 12) & 15u), (int)((w >> 16) & 15u), (int)((w >> 20) & 15u)};
}
// a descriptor word without its region-index byte: the packed box of word 0,
// the value offset and the null bit of word 1
KLE_BRICK_HD inline int brick_row_word(int w) { return (int)((unsigned)w & 0xFFFFFFu); }
inline bool brick_row_null(const int *rowd, int64_t r) { return (rowd[2 * r + 1] & BRICK_ROW_NULL) != 0; }
// a row descriptor's region index (the low and high bytes of its two words)
inline int brick_row_ir(const int *rowd, int64_t r)
{
    return (int)(((unsigned)rowd[2 * r] >> 24) | (((unsigned)rowd[2 * r + 1] >> 24) << 8));
}
// its value offset in units of 16 doubles, read and rewritten (the null bit
// and the region byte stay)
inline int64_t brick_row_off(const int *rowd, int64_t r) { return rowd[2 * r + 1] & BRICK_ROW_OFF; }
inline void brick_row_set_off(int *rowd, int64_t r, int64_t off16)
{
    rowd[2 * r + 1] = (int)(((unsigned)rowd[2 * r + 1] & ~(unsigned)BRICK_ROW_OFF) | (unsigned)off16);
}
// a real row (packed box, region index, offset < 2^23) and the null row
inline void brick_row_set(int *rowd, int64_t r, int dw, int ir, int64_t off16)
{
    rowd[2 * r] = (int)((unsigned)brick_row_word(dw) | ((unsigned)(ir & 255) << 24));
    rowd[2 * r + 1] = (int)((unsigned)off16 | ((unsigned)((ir >> 8) & 255) << 24));
}
inline void brick_row_set_null(int *rowd, int64_t r) { rowd[2 * r] = 0, rowd[2 * r + 1] = BRICK_ROW_NULL; }
// the owned-lattice node of region index ir of brick D
inline int64_t brick_ir_node(const BrickDesc &D, int ir, int64_t Lx, int64_t Ly)
{
    const int rxy = D.RX * D.RY, rz = ir / rxy, rem = ir - rz * rxy, ry = rem / D.RX, rx = rem - ry * D.RX;
    return (D.ox + rx) + Lx * ((D.oy + ry) + Ly * (int64_t)(D.oz + rz));
}

// The compact value stream (spmv_brick_compact; a box K whose analytic zeros
// are stored as exact zeros, kle_assemble.hip box_zero_entry): word 0 of a
// row descriptor then carries, above each of dbx, dby, dbz (<= 7: 3 bits), one
// bit "the row's coordinate on this axis is not on a domain boundary plane".
// A block at (kx, ky, kz) of the row's box shares coordinate c with the row
// when k_c == db_c; the off-diagonal entries (a, b) and (b, a) are left out
// of the stream when the shared plane of a or of b counts.  Returned: bit 0
// the pair (0,1), bit 1 (0,2), bit 2 (1,2).  The one place that decides what
// the stream holds: the planner's sizes, the pack and the kernel's loads all
// come here.
KLE_BRICK_HD inline int brick_drop_bits(int dw, int kx, int ky, int kz)
{
    const int s0 = ((dw >> 3) & 1) & (int)(kx == (dw & 7));
    const int s1 = ((dw >> 7) & 1) & (int)(ky == ((dw >> 4) & 7));
    const int s2 = ((dw >> 11) & 1) & (int)(kz == ((dw >> 8) & 7));
    return (s0 | s1) | ((s0 | s2) << 1) | ((s1 | s2) << 2);
}
// the pair (class) of slot t = 3 a + b: 0 (0,1), 1 (0,2), 2 (1,2); -1 the diagonal
KLE_BRICK_HD inline int brick_slot_pair(int t) { return t == 1 || t == 3 ? 0 : t == 2 || t == 6 ? 1 : t == 5 || t == 7 ? 2 : -1; }
// doubles a row holds in the compact stream, and how many entries it leaves out
inline int64_t brick_row_doubles(int dw, int64_t *dropped = nullptr)
{
    const BrickRowBox b = brick_row_box(dw, true);
    const int bnx = b.bnx, bny = b.bny, k0 = b.k0(), m = bnx * bny * b.bnz;
    int64_t out = 0;
    for (int k = k0; k < m; ++k) {
        const int kz = k / (bnx * bny), ky = (k - kz * bnx * bny) / bnx, kx = k - kz * bnx * bny - ky * bnx;
        const int d = brick_drop_bits(dw, kx, ky, kz);
        out += 2 * ((d & 1) + ((d >> 1) & 1) + ((d >> 2) & 1));
    }
    if (dropped) *dropped += out;
    return 9 * (int64_t)(m - k0) - out;
}

constexpr int BRICK_MAX_ROUNDS = 8;        // bricks per CU the planner goes up to when fewer do not fit the LDS
constexpr int BRICK_WV = 16;            // waves per brick workgroup (one workgroup per CU)
constexpr size_t BRICK_LDS_CAP = 163840;  // LDS per CU
constexpr size_t BRICK_LDS_MIN = 82 * 1024;  // above half the CU's LDS: never two bricks on one CU

struct BrickPlan {
    std::vector<BrickDesc> bricks;  // the bricks (tail tiles last), in launch order
    std::vector<int> rowd;      // 2 ints per row, brick order
    std::vector<int64_t> svb;   // per row (natural index): first double of its values, brick layout
    int64_t ws_doubles = 0, ws_entries = 0;
    size_t lds = 0;
    double model_us = 0.0;  // the planner's time model of the product (us)
    int singles = 0;        // (in) rows of one stored block out of the bricks, to the gather (spmv_brick_singles)
    int pair = 0;           // (in) units of two rows sharing their tails' item (spmv_brick_pair)
    std::vector<int64_t> srows;  // (out) those rows, ascending; their values (9 doubles each) after the bricks'
    // the compact value stream: (in) per row the three "not on a boundary
    // plane" bits (x, y, z: bits 0..2), empty: the full layout; (out) per row
    // 1 if it is a unit's second row -- its last partial pass comes first in
    // its stream -- and the entries the stream leaves out
    std::vector<unsigned char> rbits, second;
    int64_t dropped = 0;
    // deduplicated values (kle_brick.hip brick_dedup): rows with bitwise equal
    // streams share one copy, every brick's vbase is 0, and a unit's second
    // row may lie anywhere in the value array
    bool dedup = false;
    // runs of same-class units (brick_runs_build, kle_brick_plan.cpp; full
    // layout on a deduplicated array only): run_order lists brick q's units
    // (indices into its units of rowd, from rstart / 2) class by class; its
    // runs are runs[run_first[q] .. run_first[q] + bricks[q].nrun), each
    // brick_run(first position in that order, count <= run_cap); empty: none.
    // rowd itself keeps its order: the kernels that take units (DOT, whose
    // lanes' shares of (A x, x) are summed in unit order) see what they saw.
    int run_cap = 0;
    std::vector<int> runs, run_order;
    std::vector<int64_t> run_first;
    int64_t run_units = 0, run_classes = 0, run_items = 0, run_item_loads = 0;
};
// A unit's class: two units of one class run the identical item sequence --
// same value loads, same lane layout, same s of the shared item -- and differ
// only in their rows' region indices.  The key: word 0 of row A without its
// region-index byte, A's value offset, B null or not, B's word 0 likewise and
// B's value offset.
#ifndef KLE_BRICK_RUN_G
#define KLE_BRICK_RUN_G 4  // (2 and 8 were measured slower or no faster: DESIGN 3; -DKLE_BRICK_RUN_G=n rebuilds for another)
#endif
constexpr int BRICK_RUN_G = KLE_BRICK_RUN_G;  // units per run the kernel is built for
struct BrickUnitKey {
    int a0, a1, b0, b1;
    bool operator==(const BrickUnitKey &o) const { return a0 == o.a0 && a1 == o.a1 && b0 == o.b0 && b1 == o.b1; }
    bool operator<(const BrickUnitKey &o) const
    {
        return a0 != o.a0 ? a0 < o.a0 : a1 != o.a1 ? a1 < o.a1 : b0 != o.b0 ? b0 < o.b0 : b1 < o.b1;
    }
};
inline BrickUnitKey brick_unit_key(const int *rowd, int64_t unit_row)  // (unit_row: the descriptor index of row A)
{
    const int *d = rowd + 2 * unit_row;
    if (brick_row_null(rowd, unit_row + 1)) return {brick_row_word(d[0]), brick_row_word(d[1]), 0, BRICK_ROW_NULL};
    return {brick_row_word(d[0]), brick_row_word(d[1]), brick_row_word(d[2]), brick_row_word(d[3])};
}
constexpr int BRICK_RUN_SHIFT = 20;  // a run: first unit | count << 20
inline int brick_run(int first, int count) { return first | count << BRICK_RUN_SHIFT; }
inline int brick_run_first(int r) { return r & ((1 << BRICK_RUN_SHIFT) - 1); }
inline int brick_run_count(int r) { return (int)((unsigned)r >> BRICK_RUN_SHIFT); }
// a run's record on the device (ints): the class's four descriptor words with
// the region-index bytes cleared, the count, then per unit irA | irB << 16
constexpr int brick_run_words(int G) { return (5 + G + 3) & ~3; }
// items a unit streams (A's passes, the shared item, B's full passes)
inline int brick_unit_items(const int *rowd, int64_t unit_row)
{
    const int ma = brick_row_box(rowd[2 * unit_row], false).mu();
    if (brick_row_null(rowd, unit_row + 1)) return (ma + 63) / 64;
    return ma / 64 + 1 + brick_row_box(rowd[2 * unit_row + 2], false).mu() / 64;
}
// Orders each brick's units so that a class is contiguous (heavier classes
// first: the brick's tail is short; inside a class the units keep their
// order) and cuts every class into runs of at most G units.  Which rows form a
// unit, and rowd, are untouched.  Full layout on a deduplicated array only.
void brick_runs_build(BrickPlan &bp, int G);
// ... and taken back (no runs: the units one by one, as without them)
void brick_runs_clear(BrickPlan &bp);
// Runs are kept where the items whose values are loaded are at most 3/4 of
// the items.  Per item the run loop saves the loads and the block positions
// and pays for its unit loop: measured at item_loads / items 0.370 (config 2)
// the product takes 0.742 of its time, at 0.948 (config 4: bricks about one
// element large) 1.05 -- linear in between, even at 0.85; 3/4 leaves a margin.
inline bool brick_runs_pay(int64_t item_loads, int64_t items) { return items > 0 && 4 * item_loads <= 3 * items; }
// a row's descriptor word 0 with its boundary bits (compact stream)
KLE_BRICK_HD inline int brick_dw_bits(int srow, int rb)
{
    return brick_row_word(srow) | ((rb & 1) << 3) | (((rb >> 1) & 1) << 7) | (((rb >> 2) & 1) << 11);
}

// the plan's tables checked against every address the brick kernel forms
// from them (kle_brick_plan.cpp); nullptr: consistent, else what is wrong
const char *brick_validate(const BrickPlan &bp, int64_t Lx, int64_t Ly, int64_t Lz, int64_t nvals, int64_t lds_cap);
// the LDS a brick of RN region nodes needs (x, the transposed sums and their
// dummy slots, wave maxima, the row counter)
inline size_t brick_lds(int RN) { return (size_t)(3 * RN + 3 * (RN + 64)) * 8 + 512; }
// an unstructured (graph) brick: rows [r0, r0 + nr), its dictionary of U
// entries from dict[d0] (its rows first), values from sval[vbase], 2-byte
// positions from slid[sbase], sums to ws[wsoff] ([entry][3]); eb its bound
// (kle_gbrick.hip)
struct GBrickDesc {
    int r0, nr, U, eb;
    long long d0, vbase, sbase, wsoff;
};
// dictionary entries a graph brick may hold (brick_lds <= BRICK_LDS_CAP)
constexpr int GB_UCAP = (int)((BRICK_LDS_CAP - 2048) / 48);

// bricks for the owned Lx x Ly x Lz lattice of a rank (rows x-fastest; per
// row its block count and packed box, kle_sym.hip srow; hp upper ghost
// planes, z slabs at N > 1) on ncu CUs: at
// most `rounds` bricks per CU, or at most nfix bricks (> 0); fs: forced
// split counts (0: planned).  "" or why not.
std::string brick_plan(int Lx, int Ly, int Lz, int hp, int ncu, int nfix, int rounds, int fs, const std::vector<int> &cnt,
                       const std::vector<int> &srow, int P, BrickPlan &bp);
// a plan with its inputs set: singles and pair from the tuning, rbits as given
BrickPlan brick_plan_inputs(const std::vector<unsigned char> &rbits = {});
// (diagnostics) the value offsets as the row dedup rewrites them for a K whose
// rows with equal packed boxes are equal: the first such row in brick order
// keeps its values, the others point at them, every brick's vbase is 0
struct BrickShared {
    int64_t rows = 0, kept = 0, total = 0, last = -1;  // rows in bricks, rows stored, doubles of the array, the last row
};
BrickShared brick_share_by_box(BrickPlan &bp);
// The gather's run lists (kle_sym.hip gsym_gather): per 64-row slice of
// [owned | hp upper ghost planes], per brick in ascending order, each stretch
// of a lattice line in the brick's region as (first sum, 64-bit row mask);
// zo: lower ghost planes.  False: sums beyond 2^31 doubles.
bool brick_gather_runs(const BrickPlan &bp, int64_t Lx, int64_t Ly, int64_t Lz, int64_t zo, int64_t hp,
                       std::vector<int> &runptr, std::vector<int> &rstart, std::vector<unsigned long long> &rmask);

}  // namespace kle
