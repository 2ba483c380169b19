// fec_locate_multi.hpp — locate up to m/2 corrupt shards of a block (fec_rs_locate_multi_batch): the
// arithmetic the solve kernel (fec_locate_multi.hip) and the host self-test both run, and the launch
// interface.
//
// Shard r of a consistent block is the value at point r (the field element r; subtraction is xor) of
// one polynomial of degree < k, for r = 0 .. n - 1, n = k + m. With u_r = 1 / prod_{j != r} (r ^ j)
// every consistent block satisfies  sum_r u_r r^l c_r = 0  for l = 0 .. m - 1 (0^0 = 1). From the
// syndromes s_i = stored parity_i ^ computed parity_i, the power sums are
//   W_l = sum_{i < m} u_{k+i} (k+i)^l s_i              (locate_multi_table: the m x m coefficients)
// and for corrupt shards E with error bytes e_r,  W_l = sum_{r in E} (u_r e_r) r^l. The monic locator
// sigma(x) = prod_{r in E} (x ^ r) = x^v + sum_{j < v} sigma_j x^j then satisfies
//   sum_{j < v} sigma_j W_{l+j} = W_{l+v}              for l = 0 .. m - 1 - v.
// Monic in x, not in 1/x: point 0 (shard 0) is a root like any other.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "fec_kernels.hpp"
#include "fec_locate.hpp"
#include "fec_verify.hpp"
#include "gf256.h"

namespace fk {

constexpr int kLocateMaxBad = 8;         // FEC_LOCATE_MAX_BAD
constexpr int kLocateMultiRows = 16;     // parity rows of a code the call takes: one pass of 16 rows
constexpr uint32_t kLocateMultiWords = 8;   // words of a block's set of corrupt shards (n <= 256)
constexpr size_t kLocateMultiSolveLds = 64 << 10;   // LDS of a solve workgroup: all its tables, if they fit

// The radius of a call: T = min(max_bad, m / 2).
GF_HD inline uint32_t locate_multi_radius(uint32_t m, uint32_t max_bad) { return m / 2 < max_bad ? m / 2 : max_bad; }

// a^-1 without tables (a != 0): a^254.
GF_HD inline uint8_t locate_multi_inv_slow(uint8_t a) {
    uint8_t r = 1;
    for (int i = 0; i < 254; ++i) r = gf::mul_slow(r, a);
    return r;
}

// The code's m x m coefficients, row l column i: u_{k+i} (k+i)^l. logv (null: all zero, the default
// matrix) holds log v_r for the n shards of a code whose shard r is v_r p(r) (rs_matrix.hpp grs_logv):
// then c_r / v_r takes the place of c_r in the sums above, the coefficients are
// (u_{k+i} / v_{k+i}) (k+i)^l, and a corrupt shard's error value is rescaled by the nonzero 1 / v_r:
// the locator, its recurrence and its roots are the same.
GF_HD inline void locate_multi_table(uint8_t* A, uint32_t k, uint32_t m, const uint8_t* logv = nullptr) {
    const uint32_t n = k + m;
    for (uint32_t i = 0; i < m; ++i) {
        const uint32_t r = k + i;
        uint8_t prod = 1;
        for (uint32_t j = 0; j < n; ++j)
            if (j != r) prod = gf::mul_slow(prod, (uint8_t)(r ^ j));
        if (logv) prod = gf::mul_slow(prod, gf::kTables.exp[logv[r]]);   // u_r / v_r = 1 / (prod * v_r)
        uint8_t c = locate_multi_inv_slow(prod);   // u_r; then u_r r^l
        for (uint32_t l = 0; l < m; ++l) A[l * m + i] = c, c = gf::mul_slow(c, (uint8_t)r);
    }
}

// Byte products by the field's tables, ft = gf::Tables' bytes: exp[512] then log[256]. FT: a pointer
// to bytes (the host's const uint8_t*, the solve kernel's pointer into LDS).
template <class FT>
GF_HD inline uint32_t lm_mul(FT ft, uint32_t a, uint32_t b) {
    return a && b ? ft[(uint32_t)ft[512 + a] + ft[512 + b]] : 0u;
}
template <class FT>
GF_HD inline uint32_t lm_inv(FT ft, uint32_t a) { return ft[255u - ft[512 + a]]; }   // a != 0

// Byte l of the 16 a column's power sums are packed in (W_l at byte l % 4 of word l / 4), by selects:
// the words stay in registers, where an indexed array would go through scratch memory.
struct LocateMultiSums {
    uint32_t w[4];
    GF_HD uint32_t operator[](uint32_t l) const {
        const uint32_t hi = l & 8u ? (l & 4u ? w[3] : w[2]) : (l & 4u ? w[1] : w[0]);
        return (hi >> (8u * (l & 3u))) & 0xFFu;
    }
};

// Bit r of a block's present mask (the wide calls' bit order).
GF_HD inline bool partial_has(const uint32_t* mask, uint32_t r) { return (mask[r >> 5] >> (r & 31u)) & 1u; }

// One byte column: its m power sums W, some of them nonzero. For v = 1 .. T: solve the v x v Hankel
// system [W_{i+j}] sigma = [W_{v+i}] (singular: next v), require the recurrence for every
// l <= m - 1 - v, and require v distinct roots among the points 0 .. n - 1. The first v that passes
// gives the column's unique error vector of weight <= T; its support is ORed into sup and the result
// is true. No v passes: false (the column has no explanation of weight <= T).
// v = 1, the common case, needs no elimination and no search: sigma_0 = W_1 / W_0 is the root itself.
// MASKED (locate-partial, fec_locate_partial.hpp: a block with missing shards): m is the number of
// sums the column has, m - e, and `mask` the block's present mask; a root counts only at a present
// shard, so a candidate with a root at a missing point, or too few roots among the present ones, is
// rejected. Not MASKED: `mask` is not read. (A compile-time flag and a defaulted trailing argument:
// the instances without the flag compile to the code they had before the flag existed.)
template <bool MASKED = false, class FT>
GF_HD inline bool locate_multi_column(const LocateMultiSums& W, uint32_t m, uint32_t n, uint32_t T, FT ft,
                                      uint32_t (&sup)[kLocateMultiWords], const uint32_t* mask = nullptr) {
    if (T >= 1 && W[0] != 0) {
        const uint32_t r = lm_mul(ft, W[1], lm_inv(ft, W[0]));
        bool ok = r < n;
        if constexpr (MASKED) ok = ok && partial_has(mask, r);
        for (uint32_t l = 1; l + 1 < m && ok; ++l) ok = lm_mul(ft, r, W[l]) == W[l + 1];
        if (ok) {
#pragma unroll
            for (uint32_t w = 0; w < kLocateMultiWords; ++w) sup[w] |= w == r >> 5 ? 1u << (r & 31u) : 0u;
            return true;
        }
    }
    for (uint32_t v = 2; v <= T; ++v) {   // 2 v - 1 <= m - 1: every W index below is in range
        uint8_t M[kLocateMaxBad][kLocateMaxBad + 1];
        for (uint32_t i = 0; i < v; ++i) {
            for (uint32_t j = 0; j < v; ++j) M[i][j] = W[i + j];
            M[i][v] = W[v + i];
        }
        bool singular = false;
        for (uint32_t c = 0; c < v && !singular; ++c) {   // Gauss-Jordan
            uint32_t p = c;
            while (p < v && M[p][c] == 0) ++p;
            if (p == v) {
                singular = true;
                break;
            }
            const uint32_t pi = lm_inv(ft, M[p][c]);
            for (uint32_t j = 0; j <= v; ++j) {
                const uint8_t t = (uint8_t)lm_mul(ft, M[p][j], pi);
                M[p][j] = M[c][j];
                M[c][j] = t;
            }
            for (uint32_t i = 0; i < v; ++i) {
                const uint32_t f = M[i][c];
                if (i == c || f == 0) continue;
                for (uint32_t j = 0; j <= v; ++j) M[i][j] ^= (uint8_t)lm_mul(ft, f, M[c][j]);
            }
        }
        if (singular) continue;
        bool ok = true;
        for (uint32_t l = v; l + v < m && ok; ++l) {
            uint32_t acc = W[l + v];
            for (uint32_t j = 0; j < v; ++j) acc ^= lm_mul(ft, M[j][v], W[l + j]);
            ok = acc == 0;
        }
        if (!ok) continue;
        uint32_t roots[kLocateMultiWords] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t count = 0;
        for (uint32_t r = 0; r < n; ++r) {
            uint32_t acc = 1;   // Horner, sigma_v = 1
            for (uint32_t j = v; j-- > 0;) acc = lm_mul(ft, acc, r) ^ M[j][v];
            bool root = acc == 0;
            if constexpr (MASKED) root = root && partial_has(mask, r);
            if (root) roots[r >> 5] |= 1u << (r & 31u), ++count;
        }
        if (count != v) continue;
        for (uint32_t w = 0; w < kLocateMultiWords; ++w) sup[w] |= roots[w];
        return true;
    }
    return false;
}

// One 16-byte column chunk of a block, from the chunk's m syndromes S (bytes at and past shard_len
// zeroed): the power sums by the code's coefficient PermTabs A (row l's at A + l * m), then every
// nonzero byte column. The supports found are ORed into sup; true if a column has no explanation of
// weight <= T (the block is unknown then).
// MASKED (a block with e missing shards, S its scaled syndromes: fec_locate_partial.hpp): only the
// first `sums` = m - e rows of A are applied, T is the block's own radius, and the columns are solved
// with `sums` sums under the block's present mask `mask`. Not MASKED: neither is read.
// (always inlined: as a called function it would take S through memory)
template <int ROWS, bool MASKED = false, class FT>
GF_HD inline __attribute__((always_inline)) bool locate_multi_chunk(const uint32_t (&S)[ROWS][4], uint32_t m, uint32_t n, uint32_t T,
                                     const gf::PermTab* A, FT ft, uint32_t (&sup)[kLocateMultiWords],
                                     uint32_t sums = 0, const uint32_t* mask = nullptr) {
    static_assert(ROWS <= 16, "a column's power sums are packed in 16 bytes");
    const uint32_t ns = MASKED ? sums : m;   // the column's sums
    // unrolled over ROWS with uniform predicates, so that S and the sums keep to registers
    uint32_t Wd[ROWS][4];
#pragma unroll
    for (int l = 0; l < ROWS; ++l) {
        uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
        if (l < (int)ns) {
#pragma unroll
            for (int i = 0; i < ROWS; ++i)
                if (i < (int)m) {
                    const gf::PermTab t = A[(uint32_t)l * m + (uint32_t)i];
                    w0 ^= locate_mul4(t, S[i][0]), w1 ^= locate_mul4(t, S[i][1]);
                    w2 ^= locate_mul4(t, S[i][2]), w3 ^= locate_mul4(t, S[i][3]);
                }
        }
        Wd[l][0] = w0, Wd[l][1] = w1, Wd[l][2] = w2, Wd[l][3] = w3;
    }
    bool unknown = false;
#pragma unroll
    for (int x = 0; x < 16; ++x) {
        LocateMultiSums W = {{0, 0, 0, 0}};
#pragma unroll
        for (int l = 0; l < ROWS; ++l) W.w[l >> 2] |= ((Wd[l][x >> 2] >> (8 * (x & 3))) & 0xFFu) << (8 * (l & 3));
        if ((W.w[0] | W.w[1] | W.w[2] | W.w[3]) != 0 && !locate_multi_column<MASKED>(W, ns, n, T, ft, sup, mask))
            unknown = true;
    }
    return unknown;
}

// A block's result from its merged set of corrupt shards (`words` words) and its unknown flag: the
// number of shards in the set, or kLocateUnknown if a chunk was unknown or the union exceeds T.
GF_HD inline int32_t locate_multi_count(const uint32_t* bad, uint32_t words, bool unknown, uint32_t T) {
    uint32_t count = 0;
    for (uint32_t w = 0; w < words; ++w)
        for (uint32_t v = bad[w]; v; v &= v - 1) ++count;
    return unknown || count > T ? kLocateUnknown : (int32_t)count;
}

// Launch 1, the scan (verify's flat launch, fec_verify.hpp SyndromeArgs, all m <= 16 rows of the code
// in one pass): wave w of the launch writes the ballot of its lanes that hold a nonzero syndrome into
// bitmap[w], and only if the ballot is nonzero. The bitmap is zero on entry.
struct LocateMultiScanArgs : SyndromeArgs {
    uint64_t* bitmap;       // one word per wave of the launch: 4 * grid
};

// Launch 2, the solve: walks the bitmap's nwords words; for every flagged item it reads the chunk
// again, forms the syndromes and the power sums, solves, and ORs the supports into the block's words
// blk[b * (words + 1) + w], an unknown into blk[b * (words + 1) + words]. The words are zero on entry.
struct LocateMultiSolveArgs {
    LocateMultiScanArgs s;
    uint32_t nwords;
    uint32_t n, T, words;
    const uint32_t* atabs;  // locate_multi_table as m * m PermTabs
    const uint8_t* ft;      // gf::Tables' bytes
    uint32_t* blk;
};

// Launch 3, the finalize: one lane per block turns its words into bad_count, the present mask
// (optional: bits [0, n) of mask_words words, less the set's; an unknown block keeps all n) and its
// part of the two counts (optional: [0] located, [1] unknown).
struct LocateMultiFinArgs {
    const uint32_t* blk;
    int32_t* bad_count;
    uint32_t* present;
    uint32_t* counts;
    uint32_t nblocks, n, T, words, mask_words;
};

// Words of the code's device table: m * m PermTabs, then gf::Tables.
inline size_t locate_multi_tab_words(uint32_t m) { return (size_t)m * m * 8 + sizeof(gf::Tables) / 4; }

// A slice's workspace: the bitmap of its scan launch (4 words per workgroup), then the blocks' words,
// each part a multiple of 16 bytes so that one memset clears both.
inline size_t locate_multi_bitmap_bytes(uint64_t total) {
    return (size_t)((total + kThreads - 1) / kThreads) * 4 * sizeof(uint64_t);
}
inline size_t locate_multi_ws_bytes(uint64_t nblocks, uint32_t cps, uint32_t words) {
    return locate_multi_bitmap_bytes(nblocks * cps) + (size_t)((nblocks * (words + 1) * 4 + 15) & ~uint64_t(15));
}

hipError_t launch_rs_locate_multi_scan(const LocateMultiScanArgs& a, int grid, hipStream_t s);
hipError_t launch_rs_locate_multi_solve(const LocateMultiSolveArgs& a, hipStream_t s);
hipError_t launch_rs_locate_multi_finalize(const LocateMultiFinArgs& a, hipStream_t s);

// The LDS of a solve workgroup (locate-multi's and locate-partial's): the field's tables and the m x m
// coefficient PermTabs, and the code's m x k PermTabs beside them (`tabs`) where all fit.
struct LocateSolveLds {
    size_t bytes;
    bool tabs;
};
inline LocateSolveLds locate_solve_lds(uint32_t k, uint32_t m) {
    const size_t fixed = sizeof(gf::Tables) + (size_t)m * m * sizeof(gf::PermTab);
    const size_t code = (size_t)m * k * sizeof(gf::PermTab);
    const bool tabs = fixed + code <= kLocateMultiSolveLds;
    return {tabs ? fixed + code : fixed, tabs};
}

}  // namespace fk
