// fec_some.hpp — reconstruct-some (klauspost Reconstruct / ReconstructSome in place): the plan
// record of one block, built by a function the narrow plan kernel (k + m <= 32) and the host
// self-tests both run, and the launch interface of fec_some.hip. Wide codes (k + m <= 256) get the
// same records from the wide plan kernel (fec_wide.hip rs_plan_wide_kernel<true>), one wave per block. Records use the wide decode's layout and its
// Lagrange arithmetic (fec_wide.hpp): nothing in wide_coef assumes that the shard it evaluates is
// a data shard. The rebuild is the wide decode's tile itself (launch_rs_rebuild_wide, some = true).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "fec_wide.hpp"

namespace fk {

// Rows a record holds: a block that can be rebuilt has at least k of its n shards present, so it
// misses, and rebuilds, at most n - k = m.
GF_HD inline uint32_t some_rows(uint32_t m) { return m ? m : 1u; }

// Shard i's bit of a mask of words: bit i % 32 of word i / 32.
GF_HD inline uint32_t mask_bit(const uint32_t* w, uint32_t i) { return (w[i >> 5] >> (i & 31u)) & 1u; }

// Build block record P (layout `lay` = wide_layout(k, some_rows(n - k))) from the block's masks, each of
// (n + 31) / 32 words or more, shard i = bit i % 32 of word i / 32 (want null: every shard):
//   inputs   S = the first k present shards, ascending (zero padded to a multiple of 8)
//   outputs  O = the missing, wanted shards below n, ascending, shard indices 0 .. n-1 (data and
//                parity alike)
//   coef[r][p] = prod_{q != p} (O[r] ^ S[q]) / (S[p] ^ S[q])      (every row by Lagrange: the shard
//                of index o is the value at o of the polynomial through the k inputs)
// Returns the block's status: 0 (nout = |O|, or 0 when nothing is to rebuild) or
// kStTooFew (something to rebuild, fewer than k present: nout = 0).
// ex768: wide_exp768(0..767); lg: the field's log table. n <= 256.
GF_HD inline int32_t some_wide_plan_record(uint8_t* P, const WideLayout& lay, const uint32_t* present,
                                           const uint32_t* want, uint32_t k, uint32_t n, const uint8_t* ex768,
                                           const uint8_t* lg, const uint8_t* logv = nullptr) {
    P[lay.nout_off] = 0;
    uint8_t* S = P + lay.in_off;
    uint8_t* O = P + lay.out_off;
    // O has room for some_rows(n - k) shards: all that a block which can be rebuilt misses; one that
    // cannot may miss more, and nothing of its record but nout is read
    const uint32_t rows = some_rows(n - k);
    uint32_t np = 0, e = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (mask_bit(present, i)) {
            if (np < k) S[np] = (uint8_t)i;
            ++np;
        } else if (!want || mask_bit(want, i)) {
            if (e < rows) O[e] = (uint8_t)i;
            ++e;
        }
    }
    if (!e) return 0;
    if (np < k) return kStTooFew;
    for (uint32_t p = k; p < ((k + 7) & ~7u); ++p) S[p] = 0;
    // D_p waits in row 0 of the coefficients; rows go high to low, so row 0 replaces each D_p right
    // after reading it (as rs_plan_kernel, fec_decode.hip)
    uint8_t* C = P + lay.coef_off;
    for (uint32_t p = 0; p < k; ++p) C[p] = (uint8_t)wide_logsum(lg, S, k, S[p], p, logv);
    for (uint32_t r = e; r-- > 0;) {
        const uint32_t o = O[r];
        const uint32_t N = wide_logsum(lg, S, k, o, k, logv);
        for (uint32_t p = 0; p < k; ++p) C[r * k + p] = wide_coef(ex768, lg, N, C[p], o, S[p]);
    }
    P[lay.nout_off] = (uint8_t)e;
    return 0;
}

// The one-word form (k + m <= 32), which rs_plan_some_kernel runs.
GF_HD inline int32_t some_plan_record(uint8_t* P, const WideLayout& lay, uint32_t present, uint32_t want,
                                      uint32_t k, uint32_t n, const uint8_t* ex768, const uint8_t* lg,
                                      const uint8_t* logv = nullptr) {
    return some_wide_plan_record(P, lay, &present, &want, k, n, ex768, lg, logv);
}

struct SomePlanArgs {
    const uint32_t* masks;     // nblocks present masks
    const uint32_t* want;      // nblocks want masks (null: every shard)
    uint8_t* plans;            // nblocks * lay.stride bytes
    int32_t* status;           // optional
    int* err;                  // sticky error word
    uint32_t k, n, nblocks;
    WideLayout lay;
    const uint8_t* logv;       // n bytes, log v_r per shard (PlanArgs::logv); null for the default matrix
};

hipError_t launch_rs_plan_some(const SomePlanArgs& a, hipStream_t s);

}  // namespace fk
