// fec_solve.hpp — the elimination plan of a custom code matrix (fec_hip_matrix.h
// fec_ctx_set_custom_matrix, klauspost WithCustomMatrix), k + m <= 32. Host and device code: the plan
// kernels (fec_plan_solve.hip), the host self-test and the test hook (fec_selftest.cpp) all run the
// statements below.
//
// klauspost inverts the rows of the first k present shards. The code is systematic, so with
//   Pd  the present data shards, E the erased ones (e of them, ascending),
//   R   the first e present parity rows (the parity shards among the first k present),
// that inverse is the e x e problem A = P[R][E]: the rows are dependent exactly when A is singular,
// erased shard E_o takes (A^-1 P[R][Pd])[o][j] on present data shard j and (A^-1)[o][i] on parity
// shard R_i, and a missing parity shard q is P[q][Pd] ^ sum_c P[q][E_c] row(E_c) over the same inputs.
//
// The work is stated per column of the e x (k + e) matrix [P[R] | I], e bytes each: Gauss-Jordan
// with row pivoting turns the E columns into the identity, after which the Pd and the identity
// columns are the coefficient columns of the k inputs in index order (present data, then parity R).
// A plan kernel gives each column to a lane; the host loops over them (solve_block).
#pragma once

#include <stdint.h>

#include "fec_some.hpp"
#include "fec_status.hpp"

namespace fk {

constexpr uint32_t kSolveMaxE = 16;     // e <= min(k, m) <= 16 for k + m <= 32
constexpr uint32_t kSolveCols = 32;     // k + e <= k + m <= 32 columns
// Bytes between two columns: 5 dwords, so that the lanes of a group, each on its own column, spread
// over the LDS banks (a stride of 16 bytes would put every 8th lane on one bank).
constexpr uint32_t kSolveColStride = 20;
constexpr uint32_t kSolveColBytes = kSolveCols * kSolveColStride;

// ex: exp over [0, 510) at least (exp[i mod 255]); lg: the field's log table.
GF_HD inline uint32_t solve_mul(const uint8_t* ex, const uint8_t* lg, uint32_t x, uint32_t y) {
    return (x && y) ? ex[lg[x] + lg[y]] : 0u;
}

// Bits [0, n) set, n <= 32 (fec_kernels.hpp low_mask, restated for the host-only users).
GF_HD inline uint32_t solve_low(uint32_t n) { return n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u); }
GF_HD inline uint32_t solve_popc(uint32_t x) {
    uint32_t c = 0;
    for (; x; x &= x - 1) ++c;
    return c;
}

// Shard t's place in the block's sets (mask: the present shards, bits below n): an erased data shard
// is E[its rank among the erased data shards]; a present parity shard is R[its rank among the
// present parity shards], parity row t - k, if that rank is below e. One statement per shard.
GF_HD inline void solve_place(uint8_t* E, uint8_t* R, uint32_t t, uint32_t mask, uint32_t k, uint32_t e) {
    const uint32_t bit = (mask >> t) & 1u;
    if (t < k) {
        if (!bit) E[solve_popc(~mask & solve_low(t))] = (uint8_t)t;
    } else if (bit) {
        const uint32_t rank = solve_popc((mask >> k) & solve_low(t - k));
        if (rank < e) R[rank] = (uint8_t)(t - k);
    }
}

// Column j of [P[R] | I]: data column j < k, else column j - k of the identity.
GF_HD inline void solve_init_column(uint8_t* col, uint32_t j, const uint8_t* prows, const uint8_t* R, uint32_t k,
                                    uint32_t e) {
    for (uint32_t r = 0; r < e; ++r) col[r] = j < k ? prows[(uint32_t)R[r] * k + j] : (uint8_t)(j - k == r);
}

// The pivot of step c in the pivot column pc (column E_c): the lowest unused row, c or below it,
// with a nonzero entry; e when there is none (A is singular).
GF_HD inline uint32_t solve_pivot(const uint8_t* pc, uint32_t c, uint32_t e) {
    uint32_t p = c;
    while (p < e && !pc[p]) ++p;
    return p;
}

// Step c on one column other than the pivot column, which is read as it stood before the step: rows
// c and p change places, row c is scaled by 1 / pivot, and every other row r takes
// f_r * (the new row c), f_r its entry in the pivot column. The pivot column itself becomes the unit
// vector of row c, stays that in every later step and is never read again: nobody writes it.
GF_HD inline void solve_step(uint8_t* col, const uint8_t* pc, uint32_t c, uint32_t p, uint32_t e, const uint8_t* ex,
                             const uint8_t* lg) {
    const uint32_t x = solve_mul(ex, lg, col[p], ex[255u - lg[pc[p]]]);
    col[p] = col[c];
    col[c] = (uint8_t)x;
    for (uint32_t r = 0; r < e; ++r)
        if (r != c) col[r] ^= (uint8_t)solve_mul(ex, lg, r == p ? pc[c] : pc[r], x);
}

// The place of column j among the k inputs once the block is solved (present data shards in index
// order, then the parity shards R), and the shard it stands for; false for the column of an erased
// data shard.
GF_HD inline bool solve_input(uint32_t j, uint32_t mask, uint32_t k, uint32_t e, const uint8_t* R, uint32_t* pos,
                              uint32_t* shard) {
    if (j < k) {
        if (!((mask >> j) & 1u)) return false;
        *pos = solve_popc(mask & solve_low(j));
        *shard = j;
    } else {
        *pos = k - e + (j - k);
        *shard = k + R[j - k];
    }
    return true;
}

// The coefficient of one input column in shard o once the block is solved. col: the column's e
// solved bytes (row c = erased shard E_c); j: the column (j < k: a present data shard). An erased
// data shard's is its own row's byte; a parity shard's is P[o - k][j] (identity columns: 0) plus
// P[o - k][E_c] times row c.
GF_HD inline uint8_t solve_coef(const uint8_t* col, uint32_t j, uint32_t o, uint32_t mask, const uint8_t* prows,
                                const uint8_t* E, uint32_t k, uint32_t e, const uint8_t* ex, const uint8_t* lg) {
    if (o < k) return col[solve_popc(~mask & solve_low(o))];
    const uint8_t* row = prows + (o - k) * k;
    uint32_t v = j < k ? row[j] : 0u;
    for (uint32_t c = 0; c < e; ++c) v ^= solve_mul(ex, lg, row[E[c]], col[c]);
    return (uint8_t)v;
}

// One block on one thread: sets, columns, the e steps. cols: kSolveColBytes bytes; E, R:
// kSolveMaxE bytes each. mask has at least k of its low n bits set; e is its erased data shard count.
// False when A is singular.
GF_HD inline bool solve_block(uint8_t* cols, uint8_t* E, uint8_t* R, const uint8_t* prows, uint32_t mask, uint32_t k,
                              uint32_t n, uint32_t e, const uint8_t* ex, const uint8_t* lg) {
    for (uint32_t t = 0; t < n; ++t) solve_place(E, R, t, mask, k, e);
    for (uint32_t j = 0; j < k + e; ++j) solve_init_column(cols + j * kSolveColStride, j, prows, R, k, e);
    for (uint32_t c = 0; c < e; ++c) {
        const uint8_t* pc = cols + (uint32_t)E[c] * kSolveColStride;
        const uint32_t p = solve_pivot(pc, c, e);
        if (p == e) return false;
        for (uint32_t j = 0; j < k + e; ++j)
            if (j != E[c]) solve_step(cols + j * kSolveColStride, pc, c, p, e, ex, lg);
    }
    return true;
}

// The block classes of fec_status.hpp with the singular block after them: a block that passes
// classify_block() and whose rows are dependent rebuilds nothing.
struct SolveClass {
    int32_t status;
    uint32_t nout;
    int bit;
};

// The reconstruct / recover record of one block (PlanLayout: fec_kernels.hpp), on one thread: what
// rs_plan_solve_kernel writes with a lane per column. Scratch as solve_block.
GF_HD inline SolveClass solve_plan_record(uint8_t* P, const PlanLayout& lay, uint32_t present, uint32_t k, uint32_t n,
                                          uint32_t max_out, const uint8_t* prows, uint8_t* cols, uint8_t* E,
                                          uint8_t* R, const uint8_t* ex, const uint8_t* lg) {
    const uint32_t mask = present & solve_low(n);
    const uint32_t e = k - solve_popc(mask & solve_low(k));
    const BlockClass bc = classify_block(e, solve_popc(mask), k, max_out);
    SolveClass sc{bc.status, bc.nout, bc.bit};
    if (sc.nout && !solve_block(cols, E, R, prows, mask, k, n, e, ex, lg)) sc = {kStSingular, 0u, kStickySingular};
    P[lay.nout_off] = (uint8_t)sc.nout;
    if (!sc.nout) return sc;
    for (uint32_t r = 0; r < e; ++r) P[lay.out_off + r] = E[r];
    for (uint32_t j = 0; j < k + e; ++j) {
        uint32_t pos, shard;
        if (!solve_input(j, mask, k, e, R, &pos, &shard)) continue;
        P[lay.in_off + pos] = (uint8_t)shard;
        for (uint32_t r = 0; r < e; ++r) P[lay.coef_off + r * k + pos] = cols[j * kSolveColStride + r];
    }
    return sc;
}

// The reconstruct-some record of one block (WideLayout, rows = some_rows(n - k); fec_some.hpp
// some_plan_record states the record), on one thread: what rs_plan_solve_some_kernel writes. The
// outputs are the missing wanted shards, data and parity; a block with any of them and k shards
// present solves for all its erased data shards, wanted or not, as klauspost's Reconstruct does.
GF_HD inline SolveClass solve_some_record(uint8_t* P, const WideLayout& lay, uint32_t present, uint32_t want,
                                          uint32_t k, uint32_t n, const uint8_t* prows, uint8_t* cols, uint8_t* E,
                                          uint8_t* R, const uint8_t* ex, const uint8_t* lg) {
    const uint32_t mask = present & solve_low(n);
    const uint32_t miss = ~mask & want & solve_low(n);
    const uint32_t e = k - solve_popc(mask & solve_low(k)), eo = solve_popc(miss);
    SolveClass sc{0, 0u, 0};
    if (eo && solve_popc(mask) < k) sc = {kStTooFew, 0u, kStickyTooFew};
    else if (eo && !solve_block(cols, E, R, prows, mask, k, n, e, ex, lg)) sc = {kStSingular, 0u, kStickySingular};
    else sc.nout = eo;
    P[lay.nout_off] = (uint8_t)sc.nout;
    if (!sc.nout) return sc;
    uint8_t* O = P + lay.out_off;
    for (uint32_t t = 0; t < n; ++t)
        if ((miss >> t) & 1u) O[solve_popc(miss & solve_low(t))] = (uint8_t)t;
    for (uint32_t p = k; p < ((k + 7) & ~7u); ++p) P[lay.in_off + p] = 0;
    for (uint32_t j = 0; j < k + e; ++j) {
        uint32_t pos, shard;
        if (!solve_input(j, mask, k, e, R, &pos, &shard)) continue;
        P[lay.in_off + pos] = (uint8_t)shard;
        for (uint32_t r = 0; r < eo; ++r)
            P[lay.coef_off + r * k + pos] =
                solve_coef(cols + j * kSolveColStride, j, O[r], mask, prows, E, k, e, ex, lg);
    }
    return sc;
}

// The launch interface of fec_plan_solve.hip. The reconstruct-some form takes the parity rows beside
// the arguments of rs_plan_some_kernel (logv unused).
struct SolveSomeArgs {
    SomePlanArgs p;
    const uint8_t* prows;      // m x k parity rows, device memory
};
// Records in block order (plan_layout(k, maxe)) or sorted (plan_layout(k, maxe, true)): the records
// of launch_rs_plan and launch_rs_plan_sorted for a custom code (dall, logv unused).
hipError_t launch_rs_plan_solve(const PlanArgs& a, bool sorted, hipStream_t s);
hipError_t launch_rs_plan_solve_some(const SolveSomeArgs& a, hipStream_t s);

}  // namespace fk
