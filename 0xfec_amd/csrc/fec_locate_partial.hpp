// fec_locate_partial.hpp — locate corrupt shards in blocks that also have missing shards
// (fec_rs_locate_partial_batch): the arithmetic the kernels (fec_locate_partial.hip) and the host
// self-test both run, and the launch interface.
//
// fec_locate_multi.hpp's setting: shard r of a consistent block is the value at point r of one
// polynomial of degree < k, and every word y satisfies  V_l = sum_{r < n} u_r r^l y_r
// = sum_{i < m} A[l][i] s_i  for l < m, with the syndromes s_i = y_{k+i} ^ (row k+i applied to y's data)
// and A = locate_multi_table. Let X be a block's missing shards, e = |X| <= m, y the block with its
// missing shards taken as zeros, and lambda(x) = prod_{x_i in X} (x ^ x_i) = sum_j lambda_j x^j. The
// present shards are a code of the same kind with m - e checks and multipliers u'_r = u_r lambda(r):
//   W'_l = sum_{j <= e} lambda_j V_{l+j} = sum_{r present} u'_r r^l y_r          for l < m - e,
// all zero exactly when some codeword agrees with every present shard, and sum_{r in E} (u'_r eps_r) r^l
// for errors E among the present shards: what locate_multi_column (fec_locate_multi.hpp, the one solver
// of both calls) solves, with m - e for m.
// Since A[l][i] = u_{k+i} (k+i)^l,  sum_j lambda_j A[l+j][i] = A[l][i] lambda(k+i), so
//   W'_l = sum_{i < m} A[l][i] (lambda(k+i) s_i):
// a block's plan is the m bytes lambda(k+i), the kernels scale syndrome row i by its byte and then
// apply the first m - e rows of the code's own table. lambda(k+i) is zero for a missing parity shard,
// whose row counts for nothing. A root of a column's locator at a missing point is no shard the caller
// holds: such a candidate is rejected. The solve kernel and the self-test therefore call
// locate_multi_chunk<ROWS, true> with the scaled syndromes, m - e sums, the block's radius and its
// present mask (the solver's MASKED form); this header has no solver of its own.
#pragma once

#include "fec_locate_multi.hpp"

namespace fk {

// (the verdict kLocateTooFew: fec_status.hpp)

// A block's plan word: e in bits [0, 9), the radius T = min(max_bad, (m - e) / 2) in bits [16, 20), and
// bit 31 for a block of fewer than k present shards (e > m; no radius).
constexpr uint32_t kPartialTooFew = 1u << 31;
GF_HD inline uint32_t partial_missing(uint32_t plan) { return plan & 0x1FFu; }
GF_HD inline uint32_t partial_radius(uint32_t plan) { return (plan >> 16) & 0xFu; }

// The plan word of a block from its present mask; bits at and above n = k + m are ignored.
GF_HD inline uint32_t locate_partial_plan(const uint32_t* mask, uint32_t k, uint32_t m, uint32_t max_bad) {
    const uint32_t n = k + m;
    uint32_t e = 0;
    for (uint32_t w = 0; 32u * w < n; ++w)
        for (uint32_t v = ~mask[w] & low_mask(n - 32u * w); v; v &= v - 1) ++e;
    if (e > m) return e | kPartialTooFew;
    return e | locate_multi_radius(m - e, max_bad) << 16;
}

// lambda(k + i): the byte that scales syndrome row i of the block, a product over the missing shards
// (the clear bits below n, word by word).
GF_HD inline uint8_t locate_partial_scale(const uint32_t* mask, uint32_t k, uint32_t n, uint32_t i) {
    uint8_t prod = 1;
    for (uint32_t w = 0; 32u * w < n; ++w)
        for (uint32_t v = ~mask[w] & low_mask(n - 32u * w); v; v &= v - 1)
            prod = gf::mul_slow(prod, (uint8_t)((k + i) ^ (32u * w + (uint32_t)__builtin_ctz(v))));
    return prod;
}

// Syndrome row i times the block's byte lambda(k + i), by its PermTab L[i].
template <int ROWS>
GF_HD inline __attribute__((always_inline)) void locate_partial_scale_rows(uint32_t (&S)[ROWS][4], uint32_t m, const gf::PermTab* L) {
#pragma unroll
    for (int i = 0; i < ROWS; ++i)
        if (i < (int)m) {
            const gf::PermTab t = L[i];
#pragma unroll
            for (int d = 0; d < 4; ++d) S[i][d] = locate_mul4(t, S[i][d]);
        }
}

// A block's result: too few shards before anything else, then locate_multi_count with the block's radius.
GF_HD inline int32_t locate_partial_count(uint32_t plan, const uint32_t* bad, uint32_t words, bool unknown) {
    return plan & kPartialTooFew ? kLocateTooFew : locate_multi_count(bad, words, unknown, partial_radius(plan));
}

// A slice's workspace, in this order (every part a multiple of 16 bytes):
//   bitmap   one word per wave of the scan            } zero on entry to the scan:
//   blk      words + 1 words per block                } one memset clears the three
//   zeros    kPartialZeroBytes that stay zero         }
//   plan     one word per block                         (the plan launch writes every word)
//   ltabs    m PermTabs per block                       (written for blocks with 0 < e <= m only)
// A missing shard's loads are turned to `zeros`: the lane issues the same loads whatever its block's
// mask, reads no byte of a missing slot, and folds zeros.
constexpr size_t kPartialZeroBytes = 64;
struct PartialWs {
    size_t blk, zeros, plan, ltabs, end;   // byte offsets; the bitmap is at 0, `plan` bytes are cleared
};
inline PartialWs locate_partial_ws(uint64_t nblocks, uint32_t cps, uint32_t words, uint32_t m) {
    PartialWs w;
    w.blk = locate_multi_bitmap_bytes(nblocks * cps);
    w.zeros = w.blk + (size_t)((nblocks * (words + 1) * 4 + 15) & ~uint64_t(15));
    w.plan = w.zeros + kPartialZeroBytes;
    w.ltabs = w.plan + (size_t)((nblocks * 4 + 15) & ~uint64_t(15));
    w.end = w.ltabs + (size_t)nblocks * m * sizeof(gf::PermTab);
    return w;
}

// Launch 1, the plan: max(m, 1) lanes per block, lane i for the block's scaling table i, lane 0 for its word.
struct LocatePartialPlanArgs {
    const uint32_t* masks;  // mask_words per block
    uint32_t* plan;
    uint32_t* ltabs;
    uint32_t nblocks, k, m, max_bad, mask_words;
};

// Launch 2, the scan: locate-multi's (LocateMultiScanArgs) under the blocks' masks.
struct LocatePartialScanArgs : LocateMultiScanArgs {
    const uint32_t* masks;
    const uint32_t* plan;
    const uint32_t* ltabs;
    const uint32_t* atabs;  // locate_multi_table as m * m PermTabs
    const uint8_t* zeros;
    uint32_t mask_words;
};

// Launch 3, the solve: locate-multi's on the flagged chunks, each with its block's plan.
struct LocatePartialSolveArgs {
    LocatePartialScanArgs s;
    uint32_t nwords;
    uint32_t n, words;
    const uint8_t* ft;      // gf::Tables' bytes
    uint32_t* blk;
};

// Launch 4, the finalize: one lane per block. present may be the masks themselves: a lane reads its
// block's words before it writes them.
struct LocatePartialFinArgs {
    const uint32_t* blk;
    const uint32_t* plan;
    const uint32_t* masks;
    int32_t* bad_count;
    uint32_t* present;
    uint32_t* counts;       // optional: [0] located, [1] unknown, [2] too few
    uint32_t nblocks, n, words, mask_words;
};

hipError_t launch_rs_locate_partial_plan(const LocatePartialPlanArgs& a, hipStream_t s);
hipError_t launch_rs_locate_partial_scan(const LocatePartialScanArgs& a, int grid, hipStream_t s);
hipError_t launch_rs_locate_partial_solve(const LocatePartialSolveArgs& a, hipStream_t s);
hipError_t launch_rs_locate_partial_finalize(const LocatePartialFinArgs& a, hipStream_t s);

}  // namespace fk
