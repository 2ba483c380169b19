// fec_locate.hpp — locate the corrupt shard of a block that fails verify (fec_rs_locate_batch): the
// arithmetic the kernel (fec_locate.hip) and the host self-test both run, and the launch interface.
//
// With every shard present, the syndromes S_i = stored parity_i ^ computed parity_i name one corrupt
// shard when m >= 2. An error e in data shard j alone gives S_i = M[k+i][j] * e in every row, an
// error in parity shard k+i alone makes S_i the only nonzero row. Every entry of the parity rows M
// is nonzero and every 2 x 2 minor of them nonsingular (the code is MDS), so the ratios
// M[k+1][j] / M[k][j] are distinct over j: S_1 / S_0 at one corrupt byte names the column, and
//   M[k][j] * S_i == M[k+i][j] * S_0    for every row i and byte column
// confirms it without a division.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "fec_kernels.hpp"
#include "gf256.h"

namespace fk {

// (the verdicts kLocateClean and kLocateUnknown: fec_status.hpp)
constexpr int kLocateRows = 16;          // parity rows of a pass: row 0 and up to 15 further rows
constexpr uint32_t kLocateTabBytes = 512;

// The code's locate table, 512 bytes: [0, 256) ratio -> column (rho = M[k+1][j] / M[k][j] -> j, 0xFF
// for a ratio no column has; all 0xFF when m < 2: m >= 2 and k + m <= 256 leave 0xFF free),
// [256, 512) the field's inverses (inverse of 0 = 0). prows: the m x k parity rows. Returns false if
// an entry is zero or two columns share a ratio (which the code's matrix rules out).
GF_HD inline bool locate_table(uint8_t* tab, const uint8_t* prows, uint32_t k, uint32_t m) {
    for (uint32_t i = 0; i < 256; ++i) tab[i] = 0xFF, tab[256 + i] = 0;
    for (uint32_t a = 1; a < 256; ++a)
        for (uint32_t b = 1; b < 256; ++b)
            if (gf::mul_slow((uint8_t)a, (uint8_t)b) == 1) tab[256 + a] = (uint8_t)b;
    if (m < 2) return true;
    for (uint32_t j = 0; j < k; ++j) {
        if (!prows[j] || !prows[k + j]) return false;
        const uint8_t rho = gf::mul_slow(prows[k + j], tab[256 + prows[j]]);
        if (tab[rho] != 0xFF) return false;
        tab[rho] = (uint8_t)j;
    }
    return true;
}

// c * x for four packed bytes x, c by its PermTab (the kernels' v_perm product, gf256.h).
GF_HD inline uint32_t locate_mul4(const gf::PermTab& t, uint32_t x) {
    return gf::perm_b32(t.t0hi, t.t0lo, x & 0x07070707u) ^ gf::perm_b32(t.t1hi, t.t1lo, (x >> 3) & 0x07070707u) ^
           gf::perm_b32(t.t2, t.t2, (x >> 6) & 0x03030303u);
}

// The parity row that index i of a pass stands for: row 0, then the rows from r0.
GF_HD inline uint32_t locate_row(uint32_t i, uint32_t r0) { return i ? r0 + i - 1 : 0; }

// What one 16-byte column chunk of a block says about the block, from the chunk's syndromes (bytes at
// and past shard_len already zeroed): S[i] = parity row locate_row(i, r0) for i < rows. Pass 0 has
// r0 = 1 and finds its candidate column itself; a later pass (r0 > 1) takes `seen`, the block's
// verdict so far, which the earlier passes have completed.
//   every row zero                      kLocateClean (no proposal)
//   m < 2                               kLocateUnknown
//   one nonzero row                     parity shard k + that row
//   several, row 0 zero                 kLocateUnknown (a data error shows in every row)
//   several, row 0 nonzero              column j if M[k][j] * S_i == M[k+i][j] * S_0 for every row of
//                                       the pass over all 16 byte columns, else kLocateUnknown
// T: the pass's rows * k PermTabs, row i's at T + i * k; tab: locate_table's bytes.
template <int ROWS>
GF_HD inline int32_t locate_chunk(const uint32_t (&S)[ROWS][4], uint32_t rows, uint32_t r0, uint32_t k, uint32_t m,
                                  const gf::PermTab* T, const uint8_t* tab, int32_t seen) {
    uint32_t count = 0, only = 0;
#pragma unroll
    for (int i = 0; i < ROWS; ++i)
        if (i < (int)rows && (S[i][0] | S[i][1] | S[i][2] | S[i][3]) != 0) ++count, only = locate_row((uint32_t)i, r0);
    if (count == 0) return kLocateClean;
    if (m < 2) return kLocateUnknown;
    if (count == 1) return (int32_t)(k + only);
    if ((S[0][0] | S[0][1] | S[0][2] | S[0][3]) == 0) return kLocateUnknown;
    int32_t j = seen;
    if (r0 == 1) {
        // rho = S_1 / S_0 at the first nonzero byte of S_0 (rows >= 2 here: m >= 2)
        constexpr int ONE = ROWS > 1 ? 1 : 0;
        uint32_t s0 = 0, s1 = 0;
#pragma unroll
        for (int d = 3; d >= 0; --d)
#pragma unroll
            for (int sh = 24; sh >= 0; sh -= 8) {
                const uint32_t b = (S[0][d] >> sh) & 0xFFu;
                s0 = b ? b : s0;
                s1 = b ? (S[ONE][d] >> sh) & 0xFFu : s1;
            }
        const uint32_t col = tab[gf::mul_slow((uint8_t)s1, tab[256 + s0])];
        j = col == 0xFFu ? kLocateUnknown : (int32_t)col;
    }
    if (j < 0 || j >= (int32_t)k) return kLocateUnknown;
    const gf::PermTab A = T[j];
    bool ok = true;
#pragma unroll
    for (int i = 1; i < ROWS; ++i)
        if (i < (int)rows) {
            const gf::PermTab B = T[(uint32_t)i * k + (uint32_t)j];
#pragma unroll
            for (int d = 0; d < 4; ++d) ok = ok && locate_mul4(A, S[i][d]) == locate_mul4(B, S[0][d]);
        }
    return ok ? j : kLocateUnknown;
}

// A block's verdict after one more proposal: clean takes the proposal, a second proposal of the same
// shard changes nothing, a different one or an unknown makes it unknown, and unknown stays.
GF_HD inline int32_t locate_merge(int32_t cur, int32_t proposal) {
    if (proposal == kLocateClean || cur == proposal) return cur;
    return cur == kLocateClean ? proposal : kLocateUnknown;
}

// Flat launch as verify's (VerifyArgs): item = one 16-byte column chunk of one block. One launch
// takes parity row 0 and the rows - 1 <= 15 rows from r0; the caller walks longer codes in passes,
// r0 = 1, 16, 31, ...
struct LocateArgs {
    const uint8_t* in;      // data shard 0 of block 0
    const uint8_t* par;     // parity shard 0 of block 0
    uint64_t in_bs, par_bs, ss;
    uint32_t k, m;          // m: the code's parity rows (not the pass's)
    uint32_t r0, rows;      // rows: row 0 included
    uint32_t len, cps;
    uint32_t total;         // nblocks * cps (<= 2^31 per launch)
    FastDiv div_cps;
    // Row 0's k PermTabs and the (rows - 1) * k of the rows from r0, device memory. A pass whose
    // rows * k tables fit LDS (kMaxLdsTabs) stages both there, one after the other; a larger pass
    // reads them where they are, and tabs == tabs0 + k * 8 then (pass 0: the code's table itself;
    // later passes: locate_carry_tabs).
    const uint32_t* tabs0;
    const uint32_t* tabs;
    const uint8_t* loctab;  // the code's locate_table
    int32_t* verdict;       // nblocks words: kLocateClean on entry to pass 0
};

// Whether a pass of `rows` rows of a code of k data shards keeps its tables in LDS.
inline bool locate_lds_tabs(uint32_t k, uint32_t rows) { return rows * k <= (uint32_t)kMaxLdsTabs; }

// Codes whose later passes do not fit LDS (k > 128, m > 16) keep a second table for them: per later
// pass p = 1, 2, ... (r0 = 1 + 15 p) a slab of kLocateRows * k PermTabs, row 0's and then those of
// rows r0 .. (as many as the code has), so that the pass reads one contiguous table as pass 0 does.
inline bool locate_needs_carry_tabs(uint32_t k, uint32_t m) {
    return m > (uint32_t)kLocateRows && !locate_lds_tabs(k, (uint32_t)kLocateRows);
}
inline uint32_t locate_passes(uint32_t m) { return m == 0 ? 0u : 1u + (m > 16 ? (m - 16 + 14) / 15 : 0u); }

// The verdicts of nblocks blocks turned into present masks (optional: bits [0, n) of mask_words words
// per block, less the located shard's) and added to the two counts (optional: [0] located, [1] unknown).
struct LocateFinArgs {
    const int32_t* verdict;
    uint32_t* present;
    uint32_t* counts;
    uint32_t nblocks, n, mask_words;
};

hipError_t launch_rs_locate(const LocateArgs& a, int grid, hipStream_t s);
hipError_t launch_rs_locate_finalize(const LocateFinArgs& a, hipStream_t s);

}  // namespace fk
