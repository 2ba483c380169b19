// fec_some.hpp — reconstruct-some (klauspost Reconstruct / ReconstructSome in place, k + m <= 32):
// the plan record of one block, built by a function the plan kernel and the host self-test both
// run, and the launch interface of fec_some.hip. Records use the wide decode's layout and its
// Lagrange arithmetic (fec_wide.hpp): nothing in wide_coef assumes that the shard it evaluates is
// a data shard. The rebuild is the wide decode's tile itself (launch_rs_rebuild_wide, some = true).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "fec_wide.hpp"

namespace fk {

// The shards a block rebuilds: missing, wanted, and below n = k + m.
GF_HD inline uint32_t some_rebuild_set(uint32_t present, uint32_t want, uint32_t n) {
    return ~present & want & low_mask(n);
}

// Rows a record holds: a block that can be rebuilt has at least k of its n shards present, so it
// misses, and rebuilds, at most n - k = m.
GF_HD inline uint32_t some_rows(uint32_t m) { return m ? m : 1u; }

// Build block record P (layout `lay` = wide_layout(k, some_rows(n - k))) from the block's masks:
//   inputs   S = the first k present shards, ascending (zero padded to a multiple of 8)
//   outputs  O = some_rebuild_set(), ascending, shard indices 0 .. n-1 (data and parity alike)
//   coef[r][p] = prod_{q != p} (O[r] ^ S[q]) / (S[p] ^ S[q])      (every row by Lagrange: the shard
//                of index o is the value at o of the polynomial through the k inputs)
// Returns the block's status: 0 (nout = |O|, or 0 when nothing is to rebuild) or
// FEC_ERR_TOO_FEW_SHARDS = -4 (something to rebuild, fewer than k present: nout = 0).
// ex768: wide_exp768(0..767); lg: the field's log table.
GF_HD inline int32_t some_plan_record(uint8_t* P, const WideLayout& lay, uint32_t present, uint32_t want,
                                      uint32_t k, uint32_t n, const uint8_t* ex768, const uint8_t* lg) {
    present &= low_mask(n);
    const uint32_t R = some_rebuild_set(present, want, n);
    P[lay.nout_off] = 0;
    if (!R) return 0;
    uint8_t* S = P + lay.in_off;
    uint32_t np = 0;
    for (uint32_t i = 0; i < n && np < k; ++i)
        if ((present >> i) & 1u) S[np++] = (uint8_t)i;
    if (np < k) return -4;
    for (uint32_t p = k; p < ((k + 7) & ~7u); ++p) S[p] = 0;
    uint8_t* O = P + lay.out_off;
    uint32_t e = 0;
    for (uint32_t i = 0; i < n; ++i)
        if ((R >> i) & 1u) O[e++] = (uint8_t)i;
    // D_p waits in row 0 of the coefficients; rows go high to low, so row 0 replaces each D_p right
    // after reading it (as rs_plan_kernel, fec_decode.hip)
    uint8_t* C = P + lay.coef_off;
    for (uint32_t p = 0; p < k; ++p) C[p] = (uint8_t)wide_logsum(lg, S, k, S[p], p);
    for (uint32_t r = e; r-- > 0;) {
        const uint32_t o = O[r];
        const uint32_t N = wide_logsum(lg, S, k, o, k);
        for (uint32_t p = 0; p < k; ++p) C[r * k + p] = wide_coef(ex768, lg, N, C[p], o, S[p]);
    }
    P[lay.nout_off] = (uint8_t)e;
    return 0;
}

struct SomePlanArgs {
    const uint32_t* masks;     // nblocks present masks
    const uint32_t* want;      // nblocks want masks (null: every shard)
    uint8_t* plans;            // nblocks * lay.stride bytes
    int32_t* status;           // optional
    int* err;                  // sticky error word
    uint32_t k, n, nblocks;
    WideLayout lay;
};

hipError_t launch_rs_plan_some(const SomePlanArgs& a, hipStream_t s);

}  // namespace fk
