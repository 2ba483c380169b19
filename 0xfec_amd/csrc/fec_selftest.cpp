// fec_selftest.cpp — device-free self-tests of the host-visible arithmetic the kernels share with
// the host (the fk:: / gf:: / rs:: functions of the headers below). The self-tests of file-local
// code stand beside it: fec__selftest_update_slices in fec_cores.cpp, fec__selftest_copypool in
// fec_host.cpp.
#include <string.h>

#include <algorithm>
#include <array>
#include <vector>

#include "../../include/fec_hip.h"
#include "fec_kernels.hpp"
#include "fec_locate.hpp"
#include "fec_locate_multi.hpp"
#include "fec_locate_partial.hpp"
#include "fec_ragged.hpp"
#include "fec_solve.hpp"
#include "fec_some.hpp"
#include "fec_wide.hpp"
#include "gf256.h"
#include "rs_matrix.hpp"

extern "C" {

// Internal self-test (not part of the public ABI, no device needed): the lane-arithmetic PermTab
// builder the kernels use equals the byte-wise one for every coefficient. 0 on success, else
// 1 + the first failing coefficient.
int fec__selftest_permtab(void) {
    for (uint32_t c = 0; c < 256; ++c) {
        const gf::PermTab a = gf::make_permtab((uint8_t)c), b = gf::make_permtab_fast(c);
        if (a.t0lo != b.t0lo || a.t0hi != b.t0hi || a.t1lo != b.t1lo || a.t1hi != b.t1hi || a.t2 != b.t2)
            return 1 + (int)c;
    }
    return 0;
}

// Internal self-test (not part of the public ABI, no device needed): the store policy of a call
// follows the hulls of its shard regions (fec_kernels.hpp regions_apart) for block-major and
// shard-major layouts. Addresses are only compared, never dereferenced. 0 on success, else
// 1 + the index of the first failing row.
int fec__selftest_store_policy(void) {
    const uint64_t S = 1216, L = 1202, B = 67, k = 8, m = 4;
    const uintptr_t base = 0x10000000;
    auto at = [&](uint64_t off) { return (const void*)(base + off); };
    struct Row {
        int st_pol;
        fk::ShardRegion data, parity;
        uint64_t nblocks;
        uint32_t want;
    };
    const Row rows[] = {
        // split, block-major [B][k][S] + [B][m][S]: apart (parity above data, and below it)
        {1, {at(0), k * S, S, k}, {at(B * k * S), m * S, S, m}, B, 1u},
        {1, {at(B * m * S), k * S, S, k}, {at(0), m * S, S, m}, B, 1u},
        // (those two touch); one 16-byte chunk into each other
        {1, {at(0), k * S, S, k}, {at(B * k * S - 16), m * S, S, m}, B, 0u},
        // interleaved [B][k+m][S]: parity slots among the data
        {1, {at(0), (k + m) * S, S, k}, {at(k * S), (k + m) * S, S, m}, B, 0u},
        // one block of it: its parity lies past its data
        {1, {at(0), (k + m) * S, S, k}, {at(k * S), (k + m) * S, S, m}, 1, 1u},
        // shard-major [k+m][B][S] in one region: parity rows after the last data row
        {1, {at(0), S, B * S, k}, {at(k * B * S), S, B * S, m}, B, 1u},
        // shard-major, parity rows in the gaps between the data rows
        {1, {at(0), S, 2 * B * S, k}, {at(B * S), S, 2 * B * S, m}, B, 0u},
        // shard-major data, block-major parity inside the data's second row
        {1, {at(0), S, B * S, k}, {at(B * S), m * S, S, m}, 8, 0u},
        // no blocks: nothing to claim
        {1, {at(0), k * S, S, k}, {at(B * k * S), m * S, S, m}, 0, 0u},
        // knob values: 0 nt whatever the layout, 2 sc1 whatever the layout
        {0, {at(0), k * S, S, k}, {at(B * k * S), m * S, S, m}, B, 0u},
        {2, {at(0), (k + m) * S, S, k}, {at(k * S), (k + m) * S, S, m}, B, 1u},
        {2, {at(0), k * S, S, k}, {at(B * k * S), m * S, S, m}, 0, 1u},
    };
    int i = 0;
    for (const Row& r : rows) {
        ++i;
        if (fk::encode_store_policy(r.st_pol, r.data, r.parity, L, r.nblocks) != r.want) return i;
        // symmetric in its two regions
        if (fk::encode_store_policy(r.st_pol, r.parity, r.data, L, r.nblocks) != r.want) return i;
    }
    // decode: nt sc1 (3) only into an out region apart from both the data and the parity read
    const fk::ShardRegion d{at(0), S, B * S, k}, p{at(k * B * S), S, B * S, m};
    const fk::ShardRegion out_far{at((k + m) * B * S), S, B * S, m}, out_in_parity{at((k + 1) * B * S), S, B * S, 1};
    const fk::ShardRegion out_rows_over_data{at(B * S - 16 * S), 16 * S, S, m}, none{nullptr, 0, 0, 0};
    if (fk::decode_store_policy(3, d, p, out_far, L, B) != 3u) return 101;
    if (fk::decode_store_policy(3, d, p, out_in_parity, L, B) != 0u) return 102;
    if (fk::decode_store_policy(3, d, p, out_rows_over_data, L, B) != 0u) return 103;
    if (fk::decode_store_policy(3, d, p, none, L, B) != 0u) return 104;       // in place
    if (fk::decode_store_policy(0, d, p, out_far, L, B) != 0u) return 105;    // knob: nt
    if (fk::decode_store_policy(3, d, p, out_far, L, 0) != 0u) return 106;
    return 0;
}

// Whether a record's status and row count are what the rule of fec_status.hpp (classify_block) gives
// an in-place block with e shards to rebuild (reconstruct-some: every wanted missing shard) and np
// shards present.
static bool some_as_rule(int32_t st, uint32_t nout, size_t e, size_t np, uint32_t k) {
    const fk::BlockClass c = fk::classify_block((uint32_t)e, (uint32_t)np, k, 0);
    return st == c.status && nout == c.nout;
}

// Internal self-test (not part of the public ABI, no device needed): the records some_plan_record
// builds (fec_some.hpp, the function rs_plan_some_kernel runs) against the systematic matrix. For
// 64 seeded recoverable masks per code, plus all parity lost and, where m >= k, exactly k present
// with all of them parity: want = every shard; the inputs are the first k present shards, the
// outputs every missing shard, ascending, and row r equals M[O[r]] * inverse(rows S of M), parity
// rows included. Then the same mask with a seeded want mask: the outputs are the wanted missing
// shards with the rows they had, a want mask naming nothing missing gives an empty record, and a
// mask with k - 1 present gives too-few exactly when something is to rebuild. Every status and row
// count is held to classify_block. 0 on success, else 1000 * (code index + 1) + mask index + 1.
int fec__selftest_some_plan(void) {
    static const int shapes[][2] = {{8, 4}, {2, 1}, {20, 10}, {10, 22}, {1, 31}, {31, 1}};
    uint8_t ex768[768];
    for (uint32_t i = 0; i < 768; ++i) ex768[i] = fk::wide_exp768(i);
    const uint8_t* lg = gf::kTables.log;
    uint64_t seed = 0xD1B54A32D192ED03ull;
    auto rnd = [&seed]() -> uint32_t {
        seed ^= seed << 13;
        seed ^= seed >> 7;
        seed ^= seed << 17;
        return (uint32_t)(seed >> 16);
    };
    int si = 0;
    for (auto& sh : shapes) {
        ++si;
        const uint32_t k = (uint32_t)sh[0], m = (uint32_t)sh[1], n = k + m;
        const std::vector<uint8_t> M = rs::build_matrix((int)k, (int)n);
        if (M.empty()) return 1000 * si;
        const fk::WideLayout lay = fk::wide_layout(k, fk::some_rows(m));
        const uint32_t all = fk::low_mask(n);
        // stray bits at and above n are set in both masks throughout: they are ignored
        const uint32_t stray = ~all;
        std::vector<uint8_t> rec(lay.stride), rec2(lay.stride);
        const int cases = 64 + 1 + (m >= k ? 1 : 0);
        for (int ci = 0; ci < cases; ++ci) {
            const int fail = 1000 * si + ci + 1;
            uint32_t pres = all;
            if (ci == 64) {
                pres = fk::low_mask(k);                    // all parity lost
            } else if (ci == 65) {
                pres = (fk::low_mask(k) << k) & all;       // exactly k present, all of them parity
            } else {
                for (uint32_t lose = rnd() % (m + 1); lose > 0;) {
                    const uint32_t i = rnd() % n;
                    if ((pres >> i) & 1u) {
                        pres &= ~(1u << i);
                        --lose;
                    }
                }
            }
            std::vector<uint8_t> S, O;
            for (uint32_t i = 0; i < n && S.size() < k; ++i)
                if ((pres >> i) & 1u) S.push_back((uint8_t)i);
            for (uint32_t i = 0; i < n; ++i)
                if (!((pres >> i) & 1u)) O.push_back((uint8_t)i);
            std::fill(rec.begin(), rec.end(), 0xEE);
            const size_t np = n - O.size();
            int32_t st = fk::some_plan_record(rec.data(), lay, pres | stray, 0xFFFFFFFFu, k, n, ex768, lg);
            if (!some_as_rule(st, rec[lay.nout_off], O.size(), np, k) || rec[lay.nout_off] != O.size()) return fail;
            if (O.empty()) continue;
            if (memcmp(&rec[lay.in_off], S.data(), k) || memcmp(&rec[lay.out_off], O.data(), O.size())) return fail;
            std::vector<uint8_t> inv((size_t)k * k);
            for (uint32_t p = 0; p < k; ++p) memcpy(&inv[(size_t)p * k], &M[(size_t)S[p] * k], k);
            if (!rs::invert((int)k, inv.data())) return fail;
            for (size_t r = 0; r < O.size(); ++r)
                for (uint32_t p = 0; p < k; ++p) {
                    uint8_t c = 0;   // (M[o] * inv)[p]
                    for (uint32_t t = 0; t < k; ++t) c ^= gf::mul(M[(size_t)O[r] * k + t], inv[(size_t)t * k + p]);
                    if (rec[lay.coef_off + r * k + p] != c) return fail;
                }
            // a want mask: only the wanted missing shards, each with the row it had
            const uint32_t want = rnd() & all;
            std::fill(rec2.begin(), rec2.end(), 0xEE);
            st = fk::some_plan_record(rec2.data(), lay, pres, want | stray, k, n, ex768, lg);
            uint32_t r2 = 0;
            for (size_t r = 0; r < O.size(); ++r) {
                if (!((want >> O[r]) & 1u)) continue;
                if (rec2[lay.out_off + r2] != O[r] ||
                    memcmp(&rec2[lay.coef_off + r2 * k], &rec[lay.coef_off + r * k], k))
                    return fail;
                ++r2;
            }
            if (!some_as_rule(st, rec2[lay.nout_off], r2, np, k)) return fail;
            st = fk::some_plan_record(rec2.data(), lay, pres, pres | stray, k, n, ex768, lg);
            if (!some_as_rule(st, rec2[lay.nout_off], 0, np, k)) return fail;
            // k - 1 present: too few exactly when something is to rebuild
            uint32_t few = 0;
            for (uint32_t p = 0; p + 1 < k; ++p) few |= 1u << S[p];
            st = fk::some_plan_record(rec2.data(), lay, few, 0xFFFFFFFFu, k, n, ex768, lg);
            if (st != FEC_ERR_TOO_FEW_SHARDS || !some_as_rule(st, rec2[lay.nout_off], n - (k - 1), k - 1, k))
                return fail;
            st = fk::some_plan_record(rec2.data(), lay, few, few, k, n, ex768, lg);
            if (!some_as_rule(st, rec2[lay.nout_off], 0, k - 1, k)) return fail;
        }
    }
    return 0;
}

// Internal self-test (not part of the public ABI, no device needed): fec__selftest_some_plan for the
// multi-word records of some_wide_plan_record (fec_some.hpp; wide_logsum / wide_coef are what
// rs_plan_wide_kernel<true> runs), masks of 8 words. Per code 64 masks: all parity lost; exactly k
// present, all of them parity (m >= k); shards 31, 32, 63 and 64 lost (those the code has, at most m);
// the rest seeded losses of 0..m shards. Checked as there: inputs, outputs and every row against
// M[O[r]] * inverse(rows S of M) with want = NULL, a seeded want subset, a want mask naming nothing
// missing, and k - 1 present; stray bits at and above n are set in both masks throughout. 0 on
// success, else 1000 * (code index + 1) + mask index + 1.
int fec__selftest_some_wide_plan(void) {
    static const int shapes[][2] = {{20, 13}, {33, 32}, {64, 16}, {16, 240}, {128, 128}, {1, 255}, {255, 1}};
    constexpr uint32_t W = fk::kWideMaskWords;
    using Mask = std::array<uint32_t, W>;
    uint8_t ex768[768];
    for (uint32_t i = 0; i < 768; ++i) ex768[i] = fk::wide_exp768(i);
    const uint8_t* lg = gf::kTables.log;
    uint64_t seed = 0xA0761D6478BD642Full;
    auto rnd = [&seed]() -> uint32_t {
        seed ^= seed << 13;
        seed ^= seed >> 7;
        seed ^= seed << 17;
        return (uint32_t)(seed >> 16);
    };
    auto get = [](const Mask& w, uint32_t i) { return (w[i >> 5] >> (i & 31u)) & 1u; };
    auto put = [](Mask& w, uint32_t i, bool v) {
        w[i >> 5] = (w[i >> 5] & ~(1u << (i & 31u))) | ((uint32_t)v << (i & 31u));
    };
    int si = 0;
    for (auto& sh : shapes) {
        ++si;
        const uint32_t k = (uint32_t)sh[0], m = (uint32_t)sh[1], n = k + m;
        const std::vector<uint8_t> M = rs::build_matrix((int)k, (int)n);
        if (M.empty()) return 1000 * si;
        const fk::WideLayout lay = fk::wide_layout(k, fk::some_rows(m));
        if (lay.coef_off > fk::kWideHdrMax) return 1000 * si;
        // bits [0, n) of `bits`, every bit from n on set
        auto with_stray = [&](const Mask& bits) {
            Mask w = bits;
            for (uint32_t i = n; i < 32 * W; ++i) put(w, i, true);
            return w;
        };
        std::vector<uint8_t> rec(lay.stride), rec2(lay.stride);
        for (int ci = 0; ci < 64; ++ci) {
            const int fail = 1000 * si + ci + 1;
            Mask pres{};
            for (uint32_t i = 0; i < n; ++i) put(pres, i, true);
            if (ci == 0) {
                for (uint32_t i = k; i < n; ++i) put(pres, i, false);          // all parity lost
            } else if (ci == 1 && m >= k) {
                for (uint32_t i = 0; i < n; ++i) put(pres, i, i >= k && i < 2 * k);   // k present, all parity
            } else if (ci == 2) {
                uint32_t lose = m;
                for (uint32_t i : {31u, 32u, 63u, 64u})
                    if (i < n && lose) put(pres, i, false), --lose;
            } else {
                for (uint32_t lose = rnd() % (m + 1); lose > 0;) {
                    const uint32_t i = rnd() % n;
                    if (get(pres, i)) put(pres, i, false), --lose;
                }
            }
            std::vector<uint8_t> S, O;
            for (uint32_t i = 0; i < n && S.size() < k; ++i)
                if (get(pres, i)) S.push_back((uint8_t)i);
            for (uint32_t i = 0; i < n; ++i)
                if (!get(pres, i)) O.push_back((uint8_t)i);
            std::fill(rec.begin(), rec.end(), 0xEE);
            const size_t np = n - O.size();
            int32_t st = fk::some_wide_plan_record(rec.data(), lay, with_stray(pres).data(), nullptr, k, n, ex768, lg);
            if (!some_as_rule(st, rec[lay.nout_off], O.size(), np, k) || rec[lay.nout_off] != O.size()) return fail;
            if (O.empty()) continue;
            if (memcmp(&rec[lay.in_off], S.data(), k) || memcmp(&rec[lay.out_off], O.data(), O.size())) return fail;
            std::vector<uint8_t> inv((size_t)k * k);
            for (uint32_t p = 0; p < k; ++p) memcpy(&inv[(size_t)p * k], &M[(size_t)S[p] * k], k);
            if (!rs::invert((int)k, inv.data())) return fail;
            for (size_t r = 0; r < O.size(); ++r)
                for (uint32_t p = 0; p < k; ++p) {
                    uint8_t c = 0;   // (M[o] * inv)[p]
                    for (uint32_t t = 0; t < k; ++t) c ^= gf::mul(M[(size_t)O[r] * k + t], inv[(size_t)t * k + p]);
                    if (rec[lay.coef_off + r * k + p] != c) return fail;
                }
            // a want mask: only the wanted missing shards, each with the row it had
            Mask want{};
            for (uint32_t& w : want) w = rnd();
            const Mask want_s = with_stray(want);
            std::fill(rec2.begin(), rec2.end(), 0xEE);
            st = fk::some_wide_plan_record(rec2.data(), lay, pres.data(), want_s.data(), k, n, ex768, lg);
            uint32_t r2 = 0;
            for (size_t r = 0; r < O.size(); ++r) {
                if (!get(want, O[r])) continue;
                if (rec2[lay.out_off + r2] != O[r] ||
                    memcmp(&rec2[lay.coef_off + r2 * k], &rec[lay.coef_off + r * k], k))
                    return fail;
                ++r2;
            }
            if (!some_as_rule(st, rec2[lay.nout_off], r2, np, k)) return fail;
            st = fk::some_wide_plan_record(rec2.data(), lay, pres.data(), with_stray(pres).data(), k, n, ex768, lg);
            if (!some_as_rule(st, rec2[lay.nout_off], 0, np, k)) return fail;
            // k - 1 present: too few exactly when something is to rebuild
            Mask few{};
            for (uint32_t p = 0; p + 1 < k; ++p) put(few, S[p], true);
            st = fk::some_wide_plan_record(rec2.data(), lay, few.data(), nullptr, k, n, ex768, lg);
            if (st != FEC_ERR_TOO_FEW_SHARDS || !some_as_rule(st, rec2[lay.nout_off], n - (k - 1), k - 1, k))
                return fail;
            st = fk::some_wide_plan_record(rec2.data(), lay, few.data(), few.data(), k, n, ex768, lg);
            if (!some_as_rule(st, rec2[lay.nout_off], 0, k - 1, k)) return fail;
        }
    }
    return 0;
}

// Internal self-test (not part of the public ABI, no device needed): the locate call's arithmetic
// (fec_locate.hpp: locate_table, locate_chunk, locate_merge, the functions rs_locate_kernel runs)
// against the brute-force definition, on syndromes. Per code: the table names column j at
// M[k+1][j] / M[k][j] and nothing else, and holds the field's inverses. Then seeded blocks of three
// 16-byte chunks in twelve corruption patterns (none; one data shard: one byte, bytes in several
// chunks, every byte; parity row 0, any parity row, the last one; two data shards in one chunk, in
// two chunks; a data and a parity shard in two chunks; for m > 16 a data shard whose rows 16 .. carry
// another error of the same column; t >= 2 random shards): the chunks are classified pass by pass
// (row 0 and 15 rows from r0 = 1, 16, ...) and merged into one word, in ascending and in descending
// chunk order, and the word must be what the definition gives: clean if every syndrome is zero, else
// (m >= 2) the one shard s for which some replacement of s alone explains every syndrome (a parity
// row that is the only nonzero one; a column j with S_i = M[k+i][j] * S_0 / M[k][j] in every row and
// byte), else unknown. 0 on success, else 1000 * (code index + 1) + case index + 1.
int fec__selftest_locate(void) {
    static const int shapes[][2] = {{1, 2}, {2, 2}, {8, 4}, {20, 10}, {3, 20}, {2, 33}, {254, 2}, {31, 1}};
    constexpr int R = fk::kLocateRows;
    constexpr uint32_t C = 3, W = 16 * C;   // chunks and bytes per shard
    uint64_t seed = 0xA0761D6478BD642Full;
    auto rnd = [&seed]() -> uint32_t {
        seed ^= seed << 13;
        seed ^= seed >> 7;
        seed ^= seed << 17;
        return (uint32_t)(seed >> 16);
    };
    auto nzbyte = [&rnd]() -> uint8_t { return (uint8_t)(1 + rnd() % 255); };
    int si = 0;
    for (auto& sh : shapes) {
        ++si;
        const uint32_t k = (uint32_t)sh[0], m = (uint32_t)sh[1];
        const std::vector<uint8_t> M = rs::build_matrix((int)k, (int)(k + m));
        if (M.empty()) return 1000 * si;
        const uint8_t* P = M.data() + (size_t)k * k;   // parity rows
        uint8_t tab[fk::kLocateTabBytes];
        if (!fk::locate_table(tab, P, k, m)) return 1000 * si;
        for (uint32_t a = 1; a < 256; ++a)
            if (gf::mul((uint8_t)a, tab[256 + a]) != 1) return 1000 * si;
        if (tab[256] != 0) return 1000 * si;
        uint32_t named = 0;
        for (uint32_t r = 0; r < 256; ++r) named += tab[r] != 0xFF;
        if (named != (m >= 2 ? k : 0)) return 1000 * si;
        for (uint32_t j = 0; m >= 2 && j < k; ++j)
            if (tab[gf::mul(P[k + j], gf::inv(P[j]))] != j) return 1000 * si;
        std::vector<gf::PermTab> T((size_t)m * k);
        for (size_t i = 0; i < T.size(); ++i) T[i] = gf::make_permtab(P[i]);

        for (int ci = 0; ci < 12 * 8; ++ci) {
            const int fail = 1000 * si + ci + 1;
            std::vector<uint8_t> S((size_t)m * W, 0);
            auto data_err = [&](uint32_t j, uint32_t x, uint8_t e, uint32_t row_lo = 0) {
                for (uint32_t r = row_lo; r < m; ++r) S[r * W + x] ^= gf::mul(P[r * k + j], e);
            };
            auto par_err = [&](uint32_t i, uint32_t x, uint8_t e) { S[i * W + x] ^= e; };
            const uint32_t j1 = rnd() % k, j2 = k > 1 ? (j1 + 1 + rnd() % (k - 1)) % k : j1;
            const uint32_t x1 = rnd() % 16, x2 = 16 + rnd() % 16, x3 = 32 + rnd() % 16;
            switch (ci % 12) {
                case 0: break;
                case 1: data_err(j1, x2, (uint8_t)(1u << (rnd() % 8))); break;
                case 2: data_err(j1, x1, nzbyte()), data_err(j1, x2, nzbyte()), data_err(j1, x3, nzbyte()); break;
                case 3:
                    for (uint32_t x = 0; x < W; ++x) data_err(j1, x, nzbyte());
                    break;
                case 4: par_err(0, x1, nzbyte()), par_err(0, x3, nzbyte()); break;
                case 5: par_err(rnd() % m, x2, nzbyte()); break;
                case 6: par_err(m - 1, x1, nzbyte()), par_err(m - 1, x2, nzbyte()); break;
                case 7:   // (k = 1: a data and a parity shard)
                    data_err(j1, x1, nzbyte());
                    if (k > 1) data_err(j2, (x1 + 1) % 16, nzbyte());
                    else par_err(rnd() % m, (x1 + 1) % 16, nzbyte());
                    break;
                case 8:
                    data_err(j1, x1, nzbyte());
                    if (k > 1) data_err(j2, x3, nzbyte());
                    else par_err(rnd() % m, x3, nzbyte());
                    break;
                case 9: data_err(j1, x1, nzbyte()), par_err(rnd() % m, x2, nzbyte()); break;
                case 10: {   // every pass agrees on the column, the passes disagree on the error
                    const uint8_t e = nzbyte();
                    data_err(j1, x2, e);
                    if (m > 16) data_err(j1, x2, nzbyte(), 16);   // rows 16 ..: e ^ another byte
                    break;
                }
                default:
                    for (uint32_t t = 2 + rnd() % (m + 1); t > 0; --t) {
                        const uint32_t s = rnd() % (k + m);
                        if (s < k) data_err(s, rnd() % W, nzbyte());
                        else par_err(s - k, rnd() % W, nzbyte());
                    }
            }
            // the definition
            int32_t want = fk::kLocateClean;
            if (std::any_of(S.begin(), S.end(), [](uint8_t v) { return v != 0; })) {
                int found = 0;
                want = fk::kLocateUnknown;
                for (uint32_t i = 0; m >= 2 && i < m; ++i) {
                    bool ok = true;
                    for (uint32_t r = 0; r < m; ++r)
                        for (uint32_t x = 0; x < W; ++x) ok = ok && (r == i || S[r * W + x] == 0);
                    if (ok) want = (int32_t)(k + i), ++found;
                }
                for (uint32_t j = 0; m >= 2 && j < k; ++j) {
                    bool ok = true;
                    for (uint32_t x = 0; x < W; ++x) {
                        const uint8_t e = gf::mul(gf::inv(P[j]), S[x]);
                        for (uint32_t r = 0; r < m; ++r) ok = ok && S[r * W + x] == gf::mul(P[r * k + j], e);
                    }
                    if (ok) want = (int32_t)j, ++found;
                }
                if (found > 1) return fail;   // (distance m + 1 >= 3 rules it out)
            }
            for (int order = 0; order < 2; ++order) {
                int32_t word = fk::kLocateClean;
                for (uint32_t r0 = 1; m > 0 && (r0 == 1 || r0 < m); r0 += R - 1) {
                    const uint32_t rows = 1 + std::min<uint32_t>(R - 1, m - r0);
                    std::vector<gf::PermTab> Tp(T.begin(), T.begin() + k);   // row 0's tables, then the pass's
                    Tp.insert(Tp.end(), T.begin() + (size_t)r0 * k, T.begin() + (size_t)(r0 + rows - 1) * k);
                    for (uint32_t cc = 0; cc < C; ++cc) {
                        const uint32_t c = order ? C - 1 - cc : cc;
                        uint32_t acc[R][4] = {};
                        for (uint32_t i = 0; i < rows; ++i)
                            memcpy(acc[i], &S[fk::locate_row(i, r0) * W + 16 * c], 16);
                        const int32_t p = fk::locate_chunk<R>(acc, rows, r0, k, m, Tp.data(), tab, word);
                        word = fk::locate_merge(word, p);
                    }
                }
                if (word != want) return fail;
            }
        }
    }
    // the merge rule, every pair
    const int32_t CL = fk::kLocateClean, UN = fk::kLocateUnknown;
    if (fk::locate_merge(CL, CL) != CL || fk::locate_merge(CL, 7) != 7 || fk::locate_merge(CL, UN) != UN) return 1;
    if (fk::locate_merge(7, CL) != 7 || fk::locate_merge(7, 7) != 7 || fk::locate_merge(7, 8) != UN) return 2;
    if (fk::locate_merge(7, UN) != UN || fk::locate_merge(UN, CL) != UN || fk::locate_merge(UN, 7) != UN) return 3;
    if (fk::locate_merge(UN, UN) != UN || fk::locate_merge(0, 255) != UN || fk::locate_merge(0, 0) != 0) return 4;
    return 0;
}

// Internal self-test (not part of the public ABI, no device needed): the locate-multi call's
// arithmetic (fec_locate_multi.hpp: locate_multi_table, locate_multi_chunk with its column solver,
// locate_multi_count, the functions the solve and finalize kernels run) against the brute-force
// definition, on syndromes. Per code and per max_bad = 1 .. 8 (T = min(max_bad, m / 2)): seeded blocks
// of three 16-byte chunks in fourteen error patterns (none; one byte; T shards in one byte column; T
// shards each in another chunk; supports {a,b} and {b,c} in two chunks; shard 0 among the corrupt;
// parity shards only; a data and a parity shard; one shard, every byte; T + 1 shards in one column;
// T + 1 shards spread so that no chunk holds more than T; t random shards, 0 <= t <= n; t random
// shards, T < t <= m - T; up to T shards with several bytes each). The syndromes are those of the
// errors under the code's own matrix; the chunks are solved one by one, their supports ORed, and the
// result must be
//   - where the subsets can be counted (n <= 12, and RS(16,24) at max_bad <= 2): what the definition
//     gives, by trying every set of at most T shards in ascending size and asking whether every
//     syndrome column lies in the span of those columns of [P | I] (at most one set of the smallest
//     size may pass);
//   - everywhere: exactly the t corrupt shards if t <= T, unknown if T < t <= m - T.
// With max_bad = 1 the result must also agree with locate_chunk / locate_merge (fec_locate.hpp). 0 on
// success, else 100000 * (code index + 1) + 1000 * max_bad + case index + 1.
int fec__selftest_locate_multi(void) {
    static const int shapes[][2] = {{1, 2},  {2, 2},   {6, 3},  {3, 5},    {8, 4},  {1, 8},
                                    {16, 8}, {20, 10}, {4, 16}, {240, 16}, {31, 1}, {32, 0}};
    constexpr int R = fk::kLocateMultiRows;
    constexpr uint32_t C = 3, W = 16 * C, NW = fk::kLocateMultiWords;
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto rnd = [&seed]() -> uint32_t {
        seed ^= seed << 13;
        seed ^= seed >> 7;
        seed ^= seed << 17;
        return (uint32_t)(seed >> 16);
    };
    auto nzbyte = [&rnd]() -> uint8_t { return (uint8_t)(1 + rnd() % 255); };
    const uint8_t* ft = reinterpret_cast<const uint8_t*>(&gf::kTables);
    int si = 0;
    for (auto& sh : shapes) {
        ++si;
        const uint32_t k = (uint32_t)sh[0], m = (uint32_t)sh[1], n = k + m;
        const std::vector<uint8_t> M = rs::build_matrix((int)k, (int)n);
        if (M.empty()) return 100000 * si;
        const uint8_t* P = M.data() + (size_t)k * k;   // parity rows
        uint8_t A[R * R] = {};
        fk::locate_multi_table(A, k, m);
        std::vector<gf::PermTab> At((size_t)m * m), Tp((size_t)m * k);
        for (size_t i = 0; i < At.size(); ++i) At[i] = gf::make_permtab(A[i]);
        for (size_t i = 0; i < Tp.size(); ++i) Tp[i] = gf::make_permtab(P[i]);
        uint8_t loctab[fk::kLocateTabBytes];
        if (m && !fk::locate_table(loctab, P, k, m)) return 100000 * si;
        // column r of [P | I]
        auto col = [&](uint32_t r, uint32_t i) -> uint8_t { return r < k ? P[i * k + r] : (uint8_t)(r - k == i); };

        for (uint32_t max_bad = 1; max_bad <= (uint32_t)fk::kLocateMaxBad; ++max_bad) {
            const uint32_t T = fk::locate_multi_radius(m, max_bad);
            if (T != std::min(max_bad, m / 2)) return 100000 * si + 1000 * (int)max_bad;
            const bool brute = n <= 12 || (k == 16 && m == 8 && max_bad <= 2);
            for (int ci = 0; ci < 14 * 3; ++ci) {
                const int fail = 100000 * si + 1000 * (int)max_bad + ci + 1;
                std::vector<uint8_t> S((size_t)m * W, 0);
                std::vector<uint8_t> hit(n, 0);
                auto err = [&](uint32_t r, uint32_t x, uint8_t e) {   // shard r, byte x ^= e: a second error of
                    if (hit[r] & (1u << (x / 16))) return;            // a shard stays out of a chunk it is in
                    hit[r] |= (uint8_t)(1u << (x / 16));
                    for (uint32_t i = 0; i < m; ++i) S[i * W + x] ^= gf::mul(col(r, i), e);
                };
                std::vector<uint32_t> perm(n);   // distinct random shards: perm[0], perm[1], ...
                for (uint32_t r = 0; r < n; ++r) perm[r] = r;
                for (uint32_t r = 0; r + 1 < n; ++r) std::swap(perm[r], perm[r + rnd() % (n - r)]);
                const uint32_t x0 = rnd() % 16, x1 = 16 + rnd() % 16;
                auto some = [&](uint32_t t) { return std::min(t, n); };
                switch (ci % 14) {
                    case 0: break;
                    case 1: err(perm[0], rnd() % W, (uint8_t)(1u << (rnd() % 8))); break;
                    case 2:
                        for (uint32_t i = 0; i < some(T); ++i) err(perm[i], x1, nzbyte());
                        break;
                    case 3:
                        for (uint32_t i = 0; i < some(T); ++i) err(perm[i], 16 * (i % C) + rnd() % 16, nzbyte());
                        break;
                    case 4:
                        err(perm[0], x0, nzbyte());
                        if (n > 1) err(perm[1], x0, nzbyte()), err(perm[1], x1, nzbyte());
                        if (n > 2) err(perm[2], x1, nzbyte());
                        break;
                    case 5:
                        err(0, x1, nzbyte());
                        for (uint32_t i = 0, left = T ? T - 1 : 0; i < n && left; ++i)
                            if (perm[i] != 0) err(perm[i], x1, nzbyte()), --left;
                        break;
                    case 6:
                        for (uint32_t i = 0; i < std::min(std::max(T, 1u), m); ++i) err(k + (perm[0] + i) % m, x0, nzbyte());
                        break;
                    case 7:
                        err(rnd() % k, x0, nzbyte());
                        if (m) err(k + rnd() % m, x1, nzbyte());
                        break;
                    case 8:
                        for (uint32_t x = 0; x < W; ++x) err(perm[0], x, nzbyte()), hit[perm[0]] = 0;
                        hit[perm[0]] = 7;
                        break;
                    case 9:
                        for (uint32_t i = 0; i < some(T + 1); ++i) err(perm[i], x0, nzbyte());
                        break;
                    case 10:
                        for (uint32_t i = 0; i < some(T + 1); ++i) err(perm[i], 16 * (i % C) + x0, nzbyte());
                        break;
                    case 11:
                        for (uint32_t i = 0, t = rnd() % (n + 1); i < t; ++i) err(perm[i], rnd() % W, nzbyte());
                        break;
                    case 12:
                        if (m >= 2 * T + 1)
                            for (uint32_t i = 0, t = T + 1 + rnd() % (m - 2 * T); i < some(t); ++i)
                                err(perm[i], x1, nzbyte());
                        break;
                    default:
                        for (uint32_t i = 0, t = T ? 1 + rnd() % T : 0; i < some(t); ++i)
                            for (uint32_t c = 0; c < C; ++c) err(perm[i], 16 * c + rnd() % 16, nzbyte());
                }
                uint32_t t = 0;
                uint32_t hitset[NW] = {};
                for (uint32_t r = 0; r < n; ++r)
                    if (hit[r]) ++t, hitset[r >> 5] |= 1u << (r & 31u);

                // the code under test: chunk by chunk, supports ORed, then the count
                uint32_t sup[NW] = {};
                bool unknown = false;
                for (uint32_t c = 0; c < C; ++c) {
                    uint32_t acc[R][4] = {};
                    for (uint32_t i = 0; i < m; ++i) memcpy(acc[i], &S[i * W + 16 * c], 16);
                    uint32_t cs[NW] = {};
                    if (fk::locate_multi_chunk<R>(acc, m, n, T, At.data(), ft, cs)) unknown = true;
                    for (uint32_t w = 0; w < NW; ++w) sup[w] |= cs[w];
                }
                const int32_t got = fk::locate_multi_count(sup, NW, unknown, T);
                const bool any = std::any_of(S.begin(), S.end(), [](uint8_t v) { return v != 0; });
                if ((got == 0) != !any) return fail;

                // the two guarantees
                if (t <= T && (got != (int32_t)t || memcmp(sup, hitset, sizeof(sup)) != 0)) return fail;
                if (t > T && t + T <= m && got != fk::kLocateUnknown) return fail;

                // the definition
                if (brute) {
                    int32_t want = fk::kLocateUnknown;
                    uint32_t wantset[NW] = {};
                    for (uint32_t v = 0; v <= T && want == fk::kLocateUnknown; ++v) {
                        std::vector<uint32_t> idx(v);   // combinations of v shards, ascending
                        for (uint32_t i = 0; i < v; ++i) idx[i] = i;
                        int found = 0;
                        for (bool more = v <= n; more;) {
                            // [H_E | S] reduced on H_E's columns; rows without a pivot must be zero in S
                            std::vector<uint8_t> G((size_t)m * (v + W));
                            for (uint32_t i = 0; i < m; ++i) {
                                for (uint32_t j = 0; j < v; ++j) G[i * (v + W) + j] = col(idx[j], i);
                                memcpy(&G[i * (v + W) + v], &S[i * W], W);
                            }
                            uint32_t row = 0;
                            for (uint32_t j = 0; j < v && row < m; ++j) {
                                uint32_t p = row;
                                while (p < m && G[p * (v + W) + j] == 0) ++p;
                                if (p == m) continue;
                                for (uint32_t x = 0; x < v + W; ++x) std::swap(G[p * (v + W) + x], G[row * (v + W) + x]);
                                const uint8_t pi = gf::inv(G[row * (v + W) + j]);
                                for (uint32_t i = row + 1; i < m; ++i) {
                                    const uint8_t f = gf::mul(G[i * (v + W) + j], pi);
                                    if (f)
                                        for (uint32_t x = j; x < v + W; ++x)
                                            G[i * (v + W) + x] ^= gf::mul(f, G[row * (v + W) + x]);
                                }
                                ++row;
                            }
                            bool ok = true;
                            for (uint32_t i = row; i < m && ok; ++i)
                                for (uint32_t x = v; x < v + W; ++x) ok = ok && G[i * (v + W) + x] == 0;
                            if (ok) {
                                ++found, want = (int32_t)v;
                                memset(wantset, 0, sizeof(wantset));
                                for (uint32_t j = 0; j < v; ++j) wantset[idx[j] >> 5] |= 1u << (idx[j] & 31u);
                            }
                            // the next combination
                            more = false;
                            for (uint32_t i = v; i-- > 0;)
                                if (idx[i] < n - v + i) {
                                    ++idx[i];
                                    for (uint32_t j = i + 1; j < v; ++j) idx[j] = idx[j - 1] + 1;
                                    more = true;
                                    break;
                                }
                        }
                        if (found > 1) return fail;   // (distance m + 1 > 2 T rules it out)
                    }
                    if (got != want) return fail;
                    if (want > 0 && memcmp(sup, wantset, sizeof(sup)) != 0) return fail;
                }

                // max_bad = 1 against the single-shard call's classifier and merge
                if (max_bad == 1) {
                    int32_t word = fk::kLocateClean;
                    for (uint32_t c = 0; m > 0 && c < C; ++c) {
                        uint32_t acc[R][4] = {};
                        for (uint32_t i = 0; i < m; ++i) memcpy(acc[i], &S[i * W + 16 * c], 16);
                        word = fk::locate_merge(word, fk::locate_chunk<R>(acc, m, 1, k, m, Tp.data(), loctab, word));
                    }
                    if (word == fk::kLocateClean && got != 0) return fail;
                    if (word == fk::kLocateUnknown && got != fk::kLocateUnknown) return fail;
                    if (word >= 0) {
                        uint32_t one[NW] = {};
                        one[word >> 5] = 1u << (word & 31);
                        if (got != 1 || memcmp(sup, one, sizeof(sup)) != 0) return fail;
                    }
                }
            }
        }
    }
    return 0;
}

// Internal self-test (not part of the public ABI, no device needed): the locate-partial call's
// arithmetic (fec_locate_partial.hpp: the plan word, the scaling bytes, the scaled rows, the count;
// fec_locate_multi.hpp: the per-chunk solver with a present set; the functions the plan, scan, solve
// and finalize kernels run) on real blocks. Per code one random codeword of three 16-byte chunks; per max_bad = 0 .. 8 and
// erasure count e = 0 .. m + 1, 24 seeded blocks: a set of e missing shards (random; with shard 0; data
// only; parity only, where there are enough), twelve error patterns on the present shards (none; one
// bit; T_b shards in one byte column; T_b shards each in another chunk; supports {a,b} and {b,c}; the
// first present shard among the corrupt; one shard, every byte; T_b + 1 in one column; T_b + 1 spread
// over the chunks; t random shards; T_b < t <= (m - e) - T_b shards; up to T_b shards with several bytes
// each), the missing shards then taken as zeros. The syndromes are those of that word under the code's
// matrix. The result must be
//   - too few for e > m, whatever the bytes;
//   - 0 exactly when no present shard was changed and t <= m - e (the punctured code's distance);
//   - exactly the t corrupt shards if t <= T_b, unknown if T_b < t <= (m - e) - T_b;
//   - for n <= 12 the definition by brute force against the punctured generator: every set E of at
//     most T_b present shards in ascending size, which explains the block if every byte column of the
//     present shards outside E lies in the column space of the generator's rows outside E and X (at
//     most one set of the smallest size may pass);
//   - with a full mask and max_bad >= 1, what locate_multi_chunk / locate_multi_count give.
// 0 on success, else 1000000 * (code index + 1) + 10000 * max_bad + 100 * e + case index + 1.
int fec__selftest_locate_partial(void) {
    static const int shapes[][2] = {{1, 2},   {2, 2},  {6, 3},    {3, 5},  {8, 4}, {16, 8},
                                    {20, 10}, {4, 16}, {240, 16}, {31, 1}, {32, 0}};
    constexpr int R = fk::kLocateMultiRows;
    constexpr uint32_t C = 3, W = 16 * C, NW = fk::kLocateMultiWords;
    uint64_t seed = 0xD1B54A32D192ED03ull;
    auto rnd = [&seed]() -> uint32_t {
        seed ^= seed << 13;
        seed ^= seed >> 7;
        seed ^= seed << 17;
        return (uint32_t)(seed >> 16);
    };
    auto nzbyte = [&rnd]() -> uint8_t { return (uint8_t)(1 + rnd() % 255); };
    const uint8_t* ft = reinterpret_cast<const uint8_t*>(&gf::kTables);
    int si = 0;
    for (auto& sh : shapes) {
        ++si;
        const uint32_t k = (uint32_t)sh[0], m = (uint32_t)sh[1], n = k + m;
        const std::vector<uint8_t> M = rs::build_matrix((int)k, (int)n);
        if (M.empty()) return 1000000 * si;
        const uint8_t* P = M.data() + (size_t)k * k;   // parity rows
        uint8_t A[R * R] = {};
        fk::locate_multi_table(A, k, m);
        std::vector<gf::PermTab> At((size_t)m * m);
        for (size_t i = 0; i < At.size(); ++i) At[i] = gf::make_permtab(A[i]);
        // one codeword: shard r's bytes at CW[r * W ..]
        std::vector<uint8_t> CW((size_t)n * W, 0);
        for (uint32_t j = 0; j < k; ++j)
            for (uint32_t x = 0; x < W; ++x) CW[j * W + x] = (uint8_t)rnd();
        for (uint32_t i = 0; i < m; ++i)
            for (uint32_t j = 0; j < k; ++j)
                for (uint32_t x = 0; x < W; ++x) CW[(k + i) * W + x] ^= gf::mul(P[i * k + j], CW[j * W + x]);
        // column r of [P | I]: what shard r's bytes add to the syndromes
        auto col = [&](uint32_t r, uint32_t i) -> uint8_t { return r < k ? P[i * k + r] : (uint8_t)(r - k == i); };

        for (uint32_t max_bad = 0; max_bad <= (uint32_t)fk::kLocateMaxBad; ++max_bad)
            for (uint32_t e = 0; e <= m + 1 && e <= n; ++e)
                for (int ci = 0; ci < 24; ++ci) {
                    const int fail = 1000000 * si + 10000 * (int)max_bad + 100 * (int)e + ci + 1;
                    // the missing shards
                    std::vector<uint32_t> perm(n);
                    for (uint32_t r = 0; r < n; ++r) perm[r] = r;
                    for (uint32_t r = 0; r + 1 < n; ++r) std::swap(perm[r], perm[r + rnd() % (n - r)]);
                    const int kind = ci / 6;   // 0 random, 1 with shard 0, 2 data first, 3 parity first
                    if (kind == 1) std::swap(perm[0], *std::find(perm.begin(), perm.end(), 0u));
                    if (kind == 2) std::stable_partition(perm.begin(), perm.end(), [&](uint32_t r) { return r < k; });
                    if (kind == 3) std::stable_partition(perm.begin(), perm.end(), [&](uint32_t r) { return r >= k; });
                    uint32_t mask[NW] = {};
                    for (uint32_t i = e; i < n; ++i) mask[perm[i] >> 5] |= 1u << (perm[i] & 31u);
                    if ((n & 31u) && (ci & 1)) mask[(n - 1) >> 5] |= ~fk::low_mask(n & 31u);   // bits at and above n: ignored
                    const std::vector<uint32_t> pres(perm.begin() + e, perm.end());   // random order
                    const uint32_t np = n - e;

                    const uint32_t plan = fk::locate_partial_plan(mask, k, m, max_bad);
                    if (fk::partial_missing(plan) != e || ((plan & fk::kPartialTooFew) != 0) != (e > m)) return fail;
                    if (e > m) {
                        uint32_t none[NW] = {};
                        if (fk::locate_partial_count(plan, none, NW, false) != fk::kLocateTooFew) return fail;
                        if (fk::locate_partial_count(plan, none, NW, true) != fk::kLocateTooFew) return fail;
                        continue;
                    }
                    const uint32_t sums = m - e, T = fk::partial_radius(plan);
                    if (T != std::min(max_bad, sums / 2)) return fail;

                    // the word: the codeword with errors on present shards
                    std::vector<uint8_t> Y(CW);
                    std::vector<uint8_t> hit(n, 0);
                    auto err = [&](uint32_t r, uint32_t x, uint8_t v) {   // present shard r, byte x ^= v
                        if (hit[r] & (1u << (x / 16))) return;
                        hit[r] |= (uint8_t)(1u << (x / 16));
                        Y[r * W + x] ^= v;
                    };
                    auto some = [&](uint32_t t) { return std::min(t, np); };
                    const uint32_t x0 = rnd() % 16, x1 = 16 + rnd() % 16;
                    switch (ci % 12) {
                        case 0: break;
                        case 1:
                            if (np) err(pres[0], rnd() % W, (uint8_t)(1u << (rnd() % 8)));
                            break;
                        case 2:
                            for (uint32_t i = 0; i < some(T); ++i) err(pres[i], x1, nzbyte());
                            break;
                        case 3:
                            for (uint32_t i = 0; i < some(T); ++i) err(pres[i], 16 * (i % C) + rnd() % 16, nzbyte());
                            break;
                        case 4:
                            if (np > 0) err(pres[0], x0, nzbyte());
                            if (np > 1) err(pres[1], x0, nzbyte()), err(pres[1], x1, nzbyte());
                            if (np > 2) err(pres[2], x1, nzbyte());
                            break;
                        case 5: {
                            const uint32_t first = *std::min_element(pres.begin(), pres.end());
                            err(first, x1, nzbyte());
                            for (uint32_t i = 0, left = T ? T - 1 : 0; i < np && left; ++i)
                                if (pres[i] != first) err(pres[i], x1, nzbyte()), --left;
                            break;
                        }
                        case 6:
                            for (uint32_t x = 0; x < W; ++x) err(pres[0], x, nzbyte()), hit[pres[0]] = 0;
                            hit[pres[0]] = 7;
                            break;
                        case 7:
                            for (uint32_t i = 0; i < some(T + 1); ++i) err(pres[i], x0, nzbyte());
                            break;
                        case 8:
                            for (uint32_t i = 0; i < some(T + 1); ++i) err(pres[i], 16 * (i % C) + x0, nzbyte());
                            break;
                        case 9:
                            for (uint32_t i = 0, t = rnd() % (np + 1); i < t; ++i) err(pres[i], rnd() % W, nzbyte());
                            break;
                        case 10:
                            if (sums >= 2 * T + 1)
                                for (uint32_t i = 0, t = T + 1 + rnd() % (sums - 2 * T); i < some(t); ++i)
                                    err(pres[i], x1, nzbyte());
                            break;
                        default:
                            for (uint32_t i = 0, t = T ? 1 + rnd() % T : 0; i < some(t); ++i)
                                for (uint32_t c = 0; c < C; ++c) err(pres[i], 16 * c + rnd() % 16, nzbyte());
                    }
                    uint32_t t = 0;
                    uint32_t hitset[NW] = {};
                    for (uint32_t r = 0; r < n; ++r)
                        if (hit[r]) ++t, hitset[r >> 5] |= 1u << (r & 31u);
                    for (uint32_t i = 0; i < e; ++i) memset(&Y[perm[i] * W], 0, W);   // missing: zeros

                    // the syndromes of the word: the codeword's are zero, so those of the shards that differ
                    std::vector<uint8_t> S((size_t)m * W, 0);
                    for (uint32_t r = 0; r < n; ++r)
                        if (hit[r] || !fk::partial_has(mask, r))
                            for (uint32_t i = 0; i < m; ++i)
                                for (uint32_t x = 0; x < W; ++x)
                                    S[i * W + x] ^= gf::mul(col(r, i), (uint8_t)(Y[r * W + x] ^ CW[r * W + x]));

                    // the code under test: the block's scaling tables, then chunk by chunk
                    gf::PermTab Lt[R] = {};
                    for (uint32_t i = 0; i < m; ++i) Lt[i] = gf::make_permtab_fast(fk::locate_partial_scale(mask, k, n, i));
                    uint32_t sup[NW] = {};
                    bool unknown = false, flagged = false;
                    for (uint32_t c = 0; c < C; ++c) {
                        uint32_t acc[R][4] = {};
                        for (uint32_t i = 0; i < m; ++i) memcpy(acc[i], &S[i * W + 16 * c], 16);
                        if (e) fk::locate_partial_scale_rows<R>(acc, m, Lt);
                        uint32_t cs[NW] = {};
                        if (fk::locate_multi_chunk<R, true>(acc, m, n, T, At.data(), ft, cs, sums, mask)) unknown = true;
                        for (uint32_t w = 0; w < NW; ++w) sup[w] |= cs[w];
                        // the scan's test: the OR of the first m - e sums of the scaled rows
                        uint32_t any = 0;
                        for (uint32_t l = 0; l < sums; ++l) {
                            uint32_t w[4] = {};
                            for (uint32_t i = 0; i < m; ++i)
                                for (uint32_t d = 0; d < 4; ++d) w[d] ^= fk::locate_mul4(At[l * m + i], acc[i][d]);
                            any |= w[0] | w[1] | w[2] | w[3];
                        }
                        flagged = flagged || any != 0;
                    }
                    const int32_t got = fk::locate_partial_count(plan, sup, NW, unknown);
                    if ((got == 0) != !flagged) return fail;   // an unflagged block is never solved

                    // the guarantees
                    if (t == 0 && got != 0) return fail;
                    if (t > 0 && t <= sums && got == 0) return fail;
                    if (t <= T && (got != (int32_t)t || memcmp(sup, hitset, sizeof(sup)) != 0)) return fail;
                    if (t > T && t + T <= sums && got != fk::kLocateUnknown) return fail;
                    for (uint32_t i = 0; i < e; ++i)
                        if (got > 0 && (sup[perm[i] >> 5] >> (perm[i] & 31u)) & 1u) return fail;   // never a missing shard

                    // the definition
                    if (n <= 12) {
                        // whether the columns of the rows `rows` of Y lie in the column space of those rows of M
                        auto explains = [&](const std::vector<uint32_t>& rows) -> bool {
                            const uint32_t nr = (uint32_t)rows.size(), wd = k + W;
                            std::vector<uint8_t> G((size_t)nr * wd);
                            for (uint32_t i = 0; i < nr; ++i) {
                                memcpy(&G[i * wd], &M[(size_t)rows[i] * k], k);
                                memcpy(&G[i * wd + k], &Y[rows[i] * W], W);
                            }
                            uint32_t row = 0;
                            for (uint32_t j = 0; j < k && row < nr; ++j) {
                                uint32_t p = row;
                                while (p < nr && G[p * wd + j] == 0) ++p;
                                if (p == nr) continue;
                                for (uint32_t x = 0; x < wd; ++x) std::swap(G[p * wd + x], G[row * wd + x]);
                                const uint8_t pi = gf::inv(G[row * wd + j]);
                                for (uint32_t i = row + 1; i < nr; ++i) {
                                    const uint8_t f = gf::mul(G[i * wd + j], pi);
                                    if (f)
                                        for (uint32_t x = j; x < wd; ++x) G[i * wd + x] ^= gf::mul(f, G[row * wd + x]);
                                }
                                ++row;
                            }
                            for (uint32_t i = row; i < nr; ++i)
                                for (uint32_t x = k; x < wd; ++x)
                                    if (G[i * wd + x]) return false;
                            return true;
                        };
                        std::vector<uint32_t> sorted(pres);
                        std::sort(sorted.begin(), sorted.end());
                        int32_t want = fk::kLocateUnknown;
                        uint32_t wantset[NW] = {};
                        for (uint32_t v = 0; v <= T && want == fk::kLocateUnknown; ++v) {
                            int found = 0;
                            for (uint32_t bits = 0; bits < (1u << np); ++bits) {   // np <= 12
                                uint32_t cnt = 0;
                                for (uint32_t b = bits; b; b &= b - 1) ++cnt;
                                if (cnt != v) continue;
                                std::vector<uint32_t> rows;
                                for (uint32_t i = 0; i < np; ++i)
                                    if (!((bits >> i) & 1u)) rows.push_back(sorted[i]);
                                if (!explains(rows)) continue;
                                ++found, want = (int32_t)v;
                                memset(wantset, 0, sizeof(wantset));
                                for (uint32_t i = 0; i < np; ++i)
                                    if ((bits >> i) & 1u) wantset[sorted[i] >> 5] |= 1u << (sorted[i] & 31u);
                            }
                            if (found > 1) return fail;   // (distance m - e + 1 > 2 T_b rules it out)
                        }
                        if (got != want) return fail;
                        if (want > 0 && memcmp(sup, wantset, sizeof(sup)) != 0) return fail;
                    }

                    // a full mask: the complete blocks' functions
                    if (e == 0 && max_bad >= 1) {
                        uint32_t sup2[NW] = {};
                        bool unk2 = false;
                        for (uint32_t c = 0; c < C; ++c) {
                            uint32_t acc[R][4] = {};
                            for (uint32_t i = 0; i < m; ++i) memcpy(acc[i], &S[i * W + 16 * c], 16);
                            if (fk::locate_multi_chunk<R>(acc, m, n, T, At.data(), ft, sup2)) unk2 = true;
                        }
                        const int32_t got2 = fk::locate_multi_count(sup2, NW, unk2, T);
                        if (got2 != got || (got > 0 && memcmp(sup, sup2, sizeof(sup)) != 0)) return fail;
                    }
                }
    }
    return 0;
}

// Internal self-test (not part of the public ABI, no device needed): the item arithmetic of the
// ragged kernels (fec_ragged.hpp), walked as the kernels walk it. For each row of a table of length
// vectors and tile sizes, every workgroup's tile and window are taken, its rounds of 256 lanes
// swept, and each item located in the tile's prefix: the items met, in order, must be exactly the
// (block, chunk) pairs of the batch in order, chunk below the block's count, each once, none
// missing; a window past its tile's item count must be empty, and no workgroup may run more than
// kRagRounds rounds. 0 on success, else 100 * (row + 1) + the failing check.
int fec__selftest_ragged_tiles(void) {
    struct Row {
        std::vector<uint32_t> lens;
        uint32_t max_len, g;
    };
    const uint32_t W = fk::kRagWindow, K16 = (uint32_t)fk::kChunk;
    std::vector<Row> rows;
    rows.push_back({std::vector<uint32_t>(40, 0), 1202, 8});                        // all-zero tiles
    {   // a zero run spanning a tile edge (blocks 5..10 of tiles of 8), an oversize block in it
        std::vector<uint32_t> l = {1202, 1, 16, 17, 50, 0, 0, 0, 0, 1203, 0, 33, 1202, 0, 15, 1200, 0xFFFFFFFFu, 7};
        rows.push_back({l, 1202, 8});
        rows.push_back({l, 1202, 3});
        rows.push_back({l, 1202, 1});
        rows.push_back({l, 1202, 256});
    }
    rows.push_back({{1202}, 1202, 16});                                             // a single block
    rows.push_back({{1}, 1202, 1});
    for (int d = -1; d <= 1; ++d) {   // a tile's sum = a multiple of 256, one less, one more
        rows.push_back({{16u * 200u, 0, 16u * (uint32_t)(56 + d), 16u * 256u}, 16u * 256u, 4});
        rows.push_back({{16u * (uint32_t)(256 + d)}, 16u * 300u, 1});
        rows.push_back({{16u * (W / 2), 16u * (uint32_t)((int)(W / 2) + d)}, 16u * W, 2});   // and of a window
    }
    rows.push_back({{70000, 1, 33333}, 70000, 1});                                  // several windows per tile
    rows.push_back({{70000, 1, 33333}, 70000, 16});
    rows.push_back({{5, 0, 1u << 30, 17}, 1u << 30, 64});                           // a 2^26-chunk shard
    int row = 0;
    for (const Row& r : rows) {
        const int fail = 100 * ++row;
        const uint32_t nblocks = (uint32_t)r.lens.size();
        const uint32_t cps_max = (r.max_len + K16 - 1) / K16;
        const uint32_t G = fk::rag_clamp_blocks(r.g, cps_max);
        if (G < 1 || G > fk::kRagMaxTileBlocks || (uint64_t)G * cps_max > fk::kRagMaxTileItems) return fail + 1;
        const uint32_t nwin = fk::rag_windows(G, cps_max);
        if ((uint64_t)nwin * W < (uint64_t)G * cps_max) return fail + 2;
        const uint32_t ntiles = (nblocks + G - 1) / G;
        uint32_t nb = 0, nc = 0;   // the next (block, chunk) the walk must meet
        auto skip_empty = [&] {
            while (nb < nblocks && nc >= fk::rag_chunks(r.lens[nb], r.max_len)) ++nb, nc = 0;
        };
        std::vector<uint32_t> prefix(G + 1);
        for (uint32_t wg = 0; wg < ntiles * nwin; ++wg) {
            const fk::RagTile T = fk::rag_tile(wg, G, nwin, nblocks);
            if (T.gt < 1 || T.gt > G || T.b0 + T.gt > nblocks || T.win >= nwin) return fail + 3;
            prefix[0] = 0;
            for (uint32_t g = 0; g < T.gt; ++g) prefix[g + 1] = prefix[g] + fk::rag_chunks(r.lens[T.b0 + g], r.max_len);
            const uint32_t total = prefix[T.gt];
            const fk::RagSpan sp = fk::rag_span(T.win, total);
            if (sp.hi > total || sp.lo > sp.hi) return fail + 4;
            if ((uint64_t)T.win * W >= total && sp.lo != sp.hi) return fail + 5;   // a window past the sum is empty
            uint32_t rounds = 0;
            for (uint32_t base = sp.lo; base < sp.hi; base += (uint32_t)fk::kThreads, ++rounds)
                for (uint32_t lane = 0; lane < (uint32_t)fk::kThreads; ++lane) {
                    const uint32_t t = base + lane;
                    if (t >= sp.hi) continue;
                    const uint32_t g = fk::rag_locate(prefix.data(), T.gt, t);
                    if (g >= T.gt) return fail + 6;
                    const uint32_t c = t - prefix[g];
                    if (c >= fk::rag_chunks(r.lens[T.b0 + g], r.max_len)) return fail + 7;
                    skip_empty();
                    if (nb != T.b0 + g || nc != c) return fail + 8;   // in order: each pair once
                    ++nc;
                }
            if (rounds > fk::kRagRounds) return fail + 9;
        }
        skip_empty();
        if (nb != nblocks) return fail + 10;   // every pair met
    }
    return 0;
}

// Internal self-test (not part of the public ABI, no device needed): the host-side arithmetic of the
// ragged reconstruct-some (fec_ragged.hpp rag_some_*), over every code k + m <= 32 (m = 0 included)
// and cps_max in {1, 76, 4375, 2^26}: the blocks per tile the launch is given (a full window's worth,
// and every forced rag_g of the tests, clamped as the core clamps them) are at least 1, at most one
// lane per block, keep a tile's local items within 32 bits and its LDS within the 64 KiB budget, and
// the largest tile is the largest that fits; a record's rows fall into rag_some_passes(rows) passes
// of at most kWideRowPass rows, each row of each possible output count in exactly one pass, and the
// rows a block keeps tables for cover every pass; the kernel instance compiled for a pass holds its
// rows. 0 on success, else 1000 * k + 10 * m + the failing check.
int fec__selftest_ragged_some(void) {
    static const uint32_t cpss[] = {1, 76, 4375, 1u << 26};
    static const uint32_t forced[] = {0, 1, 3, 16, 256, 100000};
    for (uint32_t k = 1; k <= 32; ++k)
        for (uint32_t m = 0; k + m <= 32; ++m) {
            const int fail = (int)(1000 * k + 10 * m);
            const uint32_t rows = fk::some_rows(m);
            const fk::WideLayout lay = fk::wide_layout(k, rows);
            const uint32_t gmax = fk::rag_some_max_blocks(k, rows, lay);
            if (gmax < 1 || gmax > fk::kRagMaxTileBlocks) return fail + 1;
            if (fk::rag_some_lds(gmax, k, rows, lay) > fk::kRagLdsBudget) return fail + 2;
            if (gmax < fk::kRagMaxTileBlocks && fk::rag_some_lds(gmax + 1, k, rows, lay) <= fk::kRagLdsBudget)
                return fail + 3;
            // the tables and the records of a tile lie behind one another, 16-byte aligned
            if (lay.stride % 16 || fk::rag_some_lds(1, k, rows, lay) % 16) return fail + 4;
            for (uint32_t cps : cpss)
                for (uint32_t f : forced) {
                    uint32_t G = f ? f : std::max<uint32_t>(1, fk::kRagWindow / cps);
                    G = fk::rag_clamp_blocks(std::min(G, gmax), cps);
                    if (G < 1 || G > gmax || (uint64_t)G * cps > fk::kRagMaxTileItems) return fail + 5;
                    if ((uint64_t)fk::rag_windows(G, cps) * fk::kRagWindow < (uint64_t)G * cps) return fail + 6;
                }
            const uint32_t passes = fk::rag_some_passes(rows), prow = fk::rag_some_pass_rows(rows);
            if (prow < 1 || prow > fk::kWideRowPass || passes * fk::kWideRowPass < rows ||
                (passes - 1) * fk::kWideRowPass >= rows)
                return fail + 7;
            for (uint32_t nout = 0; nout <= rows; ++nout) {
                uint32_t seen = 0;
                for (uint32_t p = 0; p < passes; ++p) {
                    const uint32_t my = fk::rag_some_rows_in_pass(nout, p * fk::kWideRowPass);
                    if (my > prow) return fail + 8;
                    seen += my;
                }
                if (seen != nout || fk::rag_some_rows_in_pass(nout, passes * fk::kWideRowPass)) return fail + 8;
            }
            const uint32_t maxe = fk::rag_some_instance(prow);
            if (maxe < prow || maxe > fk::kWideRowPass) return fail + 9;
        }
    return 0;
}

// Internal self-test (not part of the public ABI, no device needed): the wide plan's coefficient
// rows (fec_wide.hpp wide_logsum / wide_coef, the functions rs_plan_wide_kernel runs) equal the
// rows of the inverse of the first-k-present submatrix of the systematic matrix, for 64 seeded
// random recoverable masks per shape, plus all data lost where m >= k. 0 on success, else
// 1000 * (shape index + 1) + mask index + 1.
int fec__selftest_wide_plan(void) {
    static const int shapes[][2] = {{32, 1}, {20, 13}, {33, 31}, {64, 16}, {128, 128}, {255, 1}, {1, 255}, {8, 4}};
    uint8_t ex768[768];
    for (uint32_t i = 0; i < 768; ++i) ex768[i] = fk::wide_exp768(i);
    const uint8_t* lg = gf::kTables.log;
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto rnd = [&seed]() -> uint32_t {
        seed ^= seed << 13;
        seed ^= seed >> 7;
        seed ^= seed << 17;
        return (uint32_t)(seed >> 16);
    };
    int si = 0;
    for (auto& sh : shapes) {
        ++si;
        const int k = sh[0], m = sh[1], n = k + m;
        const std::vector<uint8_t> M = rs::build_matrix(k, n);
        if (M.empty()) return 1000 * si;
        const int cases = 64 + (m >= k ? 1 : 0);
        for (int ci = 0; ci < cases; ++ci) {
            std::vector<uint8_t> pres((size_t)n, 1);
            if (ci == 64) {
                for (int i = 0; i < k; ++i) pres[i] = 0;
            } else {
                for (int lose = (int)(rnd() % (uint32_t)(m + 1)); lose > 0;) {
                    const uint32_t i = rnd() % (uint32_t)n;
                    if (pres[i]) {
                        pres[i] = 0;
                        --lose;
                    }
                }
            }
            std::vector<uint8_t> S, O;
            for (int i = 0; i < n && (int)S.size() < k; ++i)
                if (pres[i]) S.push_back((uint8_t)i);
            for (int i = 0; i < k; ++i)
                if (!pres[i]) O.push_back((uint8_t)i);
            if (O.empty()) continue;
            std::vector<uint8_t> sub((size_t)k * k);
            for (int p = 0; p < k; ++p) memcpy(&sub[(size_t)p * k], &M[(size_t)S[p] * k], (size_t)k);
            if (!rs::invert(k, sub.data())) return 1000 * si + ci + 1;
            std::vector<uint32_t> D((size_t)k);
            for (int p = 0; p < k; ++p) D[p] = fk::wide_logsum(lg, S.data(), (uint32_t)k, S[p], (uint32_t)p);
            for (size_t r = 0; r < O.size(); ++r) {
                const uint32_t N = fk::wide_logsum(lg, S.data(), (uint32_t)k, O[r], (uint32_t)k);
                for (int p = 0; p < k; ++p)
                    if (fk::wide_coef(ex768, lg, N, D[p], O[r], S[p]) != sub[(size_t)O[r] * k + p])
                        return 1000 * si + ci + 1;
            }
        }
    }
    return 0;
}

// Internal self-test (not part of the public ABI, no device needed): the Cauchy matrix (rs_matrix.hpp
// build_cauchy_matrix) through the arithmetic the decode plans and the locate family run with its
// log v table (grs_logv).
// Plans, per shape 48 seeded recoverable masks plus all parity lost and, where m >= k, all data lost:
// with T = M[O] * inverse(rows S of M) by rs::invert, S the first k present shards and O every missing
// shard, data and parity,
//   - the narrow plan's sums as rs_plan_kernel forms them (D_p and N_r direct over S, + log v) and as
//     the sorted plans form them where n - k < k (dall, which holds log v, minus the others), n <= 32;
//   - the reconstruct-some record (some_wide_plan_record with logv);
//   - the wide plan's rows (wide_logsum with logv, wide_coef)
// must all give T; and without logv the record must differ from T somewhere (the table is needed).
// Locate, per shape with 1 <= m <= 16 and per max_bad: t <= T corrupt shards (shard 0 and a parity
// shard among them in turn) in every byte of a chunk, syndromes under the Cauchy rows; the column
// solver over locate_multi_table(logv) must return exactly the planted set, and with e missing shards
// (taken as zeros, rows scaled by locate_partial_scale) and t <= (m - e) / 2 likewise. 0 on success,
// else 100000 * part + 1000 * (shape index + 1) + case index + 1.
int fec__selftest_cauchy(void) {
    uint8_t ex768[768];
    for (uint32_t i = 0; i < 768; ++i) ex768[i] = fk::wide_exp768(i);
    const uint8_t* lg = gf::kTables.log;
    uint64_t seed = 0xC2B2AE3D27D4EB4Full;
    auto rnd = [&seed]() -> uint32_t {
        seed ^= seed << 13;
        seed ^= seed >> 7;
        seed ^= seed << 17;
        return (uint32_t)(seed >> 16);
    };
    auto nzbyte = [&rnd]() -> uint8_t { return (uint8_t)(1 + rnd() % 255); };
    {   // the matrix itself: identity on top, 1 / (r ^ c) below; kind 0 is build_matrix
        const std::vector<uint8_t> M = rs::build_matrix_kind(rs::kMatrixCauchy, 8, 12);
        static const uint8_t row0[8] = {0xad, 0x9d, 0xdd, 0x98, 0x3d, 0xaa, 0x5d, 0x96};
        if (M.size() != 96 || memcmp(&M[64], row0, 8)) return 1;
        for (int r = 0; r < 8; ++r)
            for (int c = 0; c < 8; ++c)
                if (M[(size_t)r * 8 + c] != (r == c)) return 2;
        if (rs::build_matrix_kind(rs::kMatrixVandermonde, 8, 12) != rs::build_matrix(8, 12)) return 3;
        if (!rs::build_matrix_kind(2, 8, 12).empty()) return 4;
    }
    static const int shapes[][2] = {{8, 4}, {2, 1}, {5, 3}, {20, 10}, {16, 8}, {1, 3}, {4, 8}, {3, 29},
                                    {33, 7}, {100, 20}, {100, 156}, {128, 128}};
    int si = 0;
    for (auto& sh : shapes) {
        ++si;
        const uint32_t k = (uint32_t)sh[0], m = (uint32_t)sh[1], n = k + m;
        const std::vector<uint8_t> M = rs::build_matrix_kind(rs::kMatrixCauchy, (int)k, (int)n);
        const std::vector<uint8_t> lv = rs::grs_logv(rs::kMatrixCauchy, (int)k, (int)n);
        if (M.empty() || lv.size() != n) return 100000 + 1000 * si;
        const fk::WideLayout lay = fk::wide_layout(k, fk::some_rows(m));
        std::vector<uint8_t> rec(lay.stride);
        std::vector<uint32_t> dall(n);   // as get_code builds it (fec_capi.cpp)
        for (uint32_t s = 0; s < n; ++s) {
            uint32_t d = lv[s];
            for (uint32_t t = 0; t < n; ++t)
                if (t != s) d += lg[s ^ t];
            dall[s] = d % 255u;
        }
        bool needed = false;
        const int cases = 48 + 1 + (m >= k ? 1 : 0);
        for (int ci = 0; ci < cases; ++ci) {
            const int fail = 100000 + 1000 * si + ci + 1;
            constexpr uint32_t W = fk::kWideMaskWords;
            std::array<uint32_t, W> pres{};
            std::vector<uint8_t> has(n, 1);
            if (ci == 48) {
                for (uint32_t i = k; i < n; ++i) has[i] = 0;
            } else if (ci == 49) {
                for (uint32_t i = 0; i < k; ++i) has[i] = 0;
            } else {
                for (uint32_t lose = 1 + rnd() % m; lose > 0;) {
                    const uint32_t i = rnd() % n;
                    if (has[i]) has[i] = 0, --lose;
                }
            }
            std::vector<uint8_t> S, O, X;   // inputs, missing, the n - k shards that are no input
            for (uint32_t i = 0; i < n; ++i) {
                if (has[i]) pres[i >> 5] |= 1u << (i & 31u);
                if (has[i] && S.size() < k) S.push_back((uint8_t)i);
                else X.push_back((uint8_t)i);
                if (!has[i]) O.push_back((uint8_t)i);
            }
            std::vector<uint8_t> inv((size_t)k * k);
            for (uint32_t p = 0; p < k; ++p) memcpy(&inv[(size_t)p * k], &M[(size_t)S[p] * k], k);
            if (!rs::invert((int)k, inv.data())) return fail;
            std::vector<uint8_t> T(O.size() * k, 0);
            for (size_t r = 0; r < O.size(); ++r)
                for (uint32_t p = 0; p < k; ++p)
                    for (uint32_t t = 0; t < k; ++t)
                        T[r * k + p] ^= gf::mul(M[(size_t)O[r] * k + t], inv[(size_t)t * k + p]);
            // reconstruct-some's record, with the table and without it
            if (fk::some_wide_plan_record(rec.data(), lay, pres.data(), nullptr, k, n, ex768, lg, lv.data()) != 0 ||
                rec[lay.nout_off] != O.size() || memcmp(&rec[lay.coef_off], T.data(), T.size()))
                return fail;
            (void)fk::some_wide_plan_record(rec.data(), lay, pres.data(), nullptr, k, n, ex768, lg);
            needed = needed || memcmp(&rec[lay.coef_off], T.data(), T.size()) != 0;
            // the wide plan's rows
            std::vector<uint32_t> D(k);
            for (uint32_t p = 0; p < k; ++p) D[p] = fk::wide_logsum(lg, S.data(), k, S[p], p, lv.data());
            for (size_t r = 0; r < O.size(); ++r) {
                const uint32_t N = fk::wide_logsum(lg, S.data(), k, O[r], k, lv.data());
                for (uint32_t p = 0; p < k; ++p)
                    if (fk::wide_coef(ex768, lg, N, D[p], O[r], S[p]) != T[r * k + p]) return fail;
            }
            if (n > FEC_MAX_DECODE_SHARDS) continue;
            // the narrow plans: rs_plan_kernel's direct sums, and the sorted plans' complement sums
            const bool comp = n - k < k;
            for (int form = 0; form < (comp ? 2 : 1); ++form) {
                auto sum = [&](uint32_t t) -> uint32_t {
                    uint32_t s = 0;
                    if (form == 0) {
                        for (uint32_t q = 0; q < k; ++q) s += t != S[q] ? lg[t ^ S[q]] : 0u;   // (t itself: no term)
                        return (s + lv[t]) % 255u;
                    }
                    for (uint32_t u = 0; u < n - k; ++u) s += t != X[u] ? lg[t ^ X[u]] : 0u;
                    return (dall[t] + 255u * 32u - s) % 255u;
                };
                for (size_t r = 0; r < O.size(); ++r) {
                    const uint32_t Nr = sum(O[r]);
                    for (uint32_t p = 0; p < k; ++p) {
                        const uint32_t v = Nr + 2u * 255u - lg[O[r] ^ S[p]] - sum(S[p]);
                        if (gf::kTables.exp[v % 255u] != T[r * k + p]) return fail;
                    }
                }
            }
        }
        if (!needed && k > 1) return 100000 + 1000 * si + 999;
    }

    // the locate family's column solver over Cauchy syndromes
    constexpr int R = fk::kLocateMultiRows;
    constexpr uint32_t NW = fk::kLocateMultiWords;
    const uint8_t* ft = reinterpret_cast<const uint8_t*>(&gf::kTables);
    static const int lshapes[][2] = {{8, 4}, {20, 10}, {64, 16}, {2, 2}, {1, 8}, {240, 16}, {3, 5}};
    si = 0;
    for (auto& sh : lshapes) {
        ++si;
        const uint32_t k = (uint32_t)sh[0], m = (uint32_t)sh[1], n = k + m;
        const std::vector<uint8_t> M = rs::build_matrix_kind(rs::kMatrixCauchy, (int)k, (int)n);
        const std::vector<uint8_t> lv = rs::grs_logv(rs::kMatrixCauchy, (int)k, (int)n);
        const uint8_t* P = M.data() + (size_t)k * k;
        uint8_t loctab[fk::kLocateTabBytes];
        if (!fk::locate_table(loctab, P, k, m)) return 200000 + 1000 * si;   // the single-shard call's table
        uint8_t A[R * R] = {};
        fk::locate_multi_table(A, k, m, lv.data());
        std::vector<gf::PermTab> At((size_t)m * m);
        for (size_t i = 0; i < At.size(); ++i) At[i] = gf::make_permtab(A[i]);
        auto col = [&](uint32_t r, uint32_t i) -> uint8_t { return r < k ? P[i * k + r] : (uint8_t)(r - k == i); };
        for (int ci = 0; ci < 96; ++ci) {
            const int fail = 200000 + 1000 * si + ci + 1;
            std::vector<uint32_t> perm(n);
            for (uint32_t r = 0; r < n; ++r) perm[r] = r;
            for (uint32_t r = 0; r + 1 < n; ++r) std::swap(perm[r], perm[r + rnd() % (n - r)]);
            // e missing shards first (none in the first half of the cases), then t corrupt ones
            const uint32_t e = ci < 48 ? 0 : (ci & 1) ? std::min(1u, m) : m / 2;
            const uint32_t sums = m - e, T = sums / 2 > (uint32_t)fk::kLocateMaxBad ? fk::kLocateMaxBad : sums / 2;
            const uint32_t t = (ci & 2) ? T : std::min(1u, T);
            if (t == 0) continue;   // (the solver is given columns with a nonzero sum only)
            if (ci % 3 == 1) std::swap(perm[e], *std::find(perm.begin(), perm.end(), 0u));       // shard 0 corrupt
            if (ci % 3 == 2) std::swap(perm[e], *std::find(perm.begin(), perm.end(), n - 1));   // a parity shard
            uint32_t mask[NW] = {}, hitset[NW] = {};
            for (uint32_t i = e; i < n; ++i) mask[perm[i] >> 5] |= 1u << (perm[i] & 31u);
            // a codeword's syndromes are zero: those of the word are its differences' (missing shards read
            // as zeros differ by the shard itself, random here)
            uint32_t acc[R][4] = {};
            uint8_t* S = reinterpret_cast<uint8_t*>(acc);
            for (uint32_t j = 0; j < e + t; ++j) {
                const uint32_t r = perm[j];
                if (j >= e) hitset[r >> 5] |= 1u << (r & 31u);
                for (uint32_t x = 0; x < 16; ++x) {
                    const uint8_t v = nzbyte();
                    for (uint32_t i = 0; i < m; ++i) S[i * 16 + x] ^= gf::mul(col(r, i), v);
                }
            }
            uint32_t sup[NW] = {};
            bool unknown;
            if (e == 0) {
                unknown = fk::locate_multi_chunk<R>(acc, m, n, T, At.data(), ft, sup);
            } else {
                gf::PermTab Lt[R] = {};
                for (uint32_t i = 0; i < m; ++i) Lt[i] = gf::make_permtab_fast(fk::locate_partial_scale(mask, k, n, i));
                fk::locate_partial_scale_rows<R>(acc, m, Lt);
                unknown = fk::locate_multi_chunk<R, true>(acc, m, n, T, At.data(), ft, sup, sums, mask);
            }
            if (unknown || memcmp(sup, hitset, sizeof(sup)) != 0) return fail;
        }
    }
    return 0;
}


}  // extern "C"

// ---------------------------------------------------------------- custom matrices (fec_solve.hpp)
namespace {

// The test matrices of tests/custom_model.py for (k, m), by their formulas: m x k parity rows.
// which: 0 the default matrix's own rows, 1 cauchy255 P[i][j] = 1 / ((255 - i) ^ j), 2 par1
// P[i][j] = (j + 1)^i, 3 lrc (8, 4): ones on columns 0-3, ones on columns 4-7, rows 0-1 of cauchy255.
std::vector<uint8_t> custom_test_rows(int which, int k, int m) {
    std::vector<uint8_t> P((size_t)m * k, 0);
    if (which == 0) {
        const std::vector<uint8_t> M = rs::build_matrix(k, k + m);
        std::copy(M.begin() + (size_t)k * k, M.end(), P.begin());
        return P;
    }
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < k; ++j) {
            const uint8_t c = gf::inv((uint8_t)((255 - i) ^ j));
            P[(size_t)i * k + j] = which == 1 ? c : which == 2 ? gf::exp_pow((uint8_t)(j + 1), i) : 0;
        }
    if (which == 3)
        for (int j = 0; j < k; ++j) {
            P[j] = j < 4, P[(size_t)k + j] = j >= 4;
            for (int i = 0; i < 2; ++i) P[(size_t)(2 + i) * k + j] = gf::inv((uint8_t)((255 - i) ^ j));
        }
    return P;
}

// What klauspost computes for one block, by another route than fec_solve.hpp: the rows of the first k
// present shards inverted whole (rs::invert, k x k). S: those shards; T: M[o] * inverse for every
// shard o < n (n x k). False when the rows are dependent.
bool custom_reference(const std::vector<uint8_t>& P, uint32_t k, uint32_t n, uint32_t mask, std::vector<uint8_t>& S,
                      std::vector<uint8_t>& T) {
    auto M = [&](uint32_t r, uint32_t c) -> uint8_t { return r < k ? (uint8_t)(r == c) : P[(size_t)(r - k) * k + c]; };
    S.clear();
    for (uint32_t i = 0; i < n && S.size() < k; ++i)
        if ((mask >> i) & 1u) S.push_back((uint8_t)i);
    std::vector<uint8_t> inv((size_t)k * k);
    for (uint32_t p = 0; p < k; ++p)
        for (uint32_t c = 0; c < k; ++c) inv[(size_t)p * k + c] = M(S[p], c);
    if (!rs::invert((int)k, inv.data())) return false;
    T.assign((size_t)n * k, 0);
    for (uint32_t o = 0; o < n; ++o)
        for (uint32_t p = 0; p < k; ++p)
            for (uint32_t t = 0; t < k; ++t) T[(size_t)o * k + p] ^= gf::mul(M(o, t), inv[(size_t)t * k + p]);
    return true;
}

// One mask of one matrix through both record builders against custom_reference: the reconstruct /
// recover record for 0, 1 and maxe output slots, the reconstruct-some record for the want masks
// given. 0, or the number of the check that failed. *singular: the rows were dependent.
int custom_check_mask(const std::vector<uint8_t>& P, uint32_t k, uint32_t m, uint32_t mask,
                      const std::vector<uint32_t>& wants, bool* singular) {
    const uint32_t n = k + m, all = fk::solve_low(n), kmask = fk::solve_low(k);
    const uint32_t maxe = std::max(1u, std::min(k, m));
    const uint8_t *ex = gf::kTables.exp, *lg = gf::kTables.log;
    uint8_t cols[fk::kSolveColBytes], E[fk::kSolveMaxE], R[fk::kSolveMaxE];
    const uint32_t np = fk::solve_popc(mask & all), e = k - fk::solve_popc(mask & kmask);
    std::vector<uint8_t> S, T;
    const bool ok = np >= k && custom_reference(P, k, n, mask, S, T);
    *singular = np >= k && !ok;
    for (uint32_t max_out : {0u, 1u, maxe}) {
        const fk::PlanLayout lay = fk::plan_layout(k, maxe, max_out == 1);
        std::vector<uint8_t> rec(lay.stride, 0xEE);
        const fk::SolveClass got =
            fk::solve_plan_record(rec.data(), lay, mask, k, n, max_out, P.data(), cols, E, R, ex, lg);
        fk::BlockClass want = fk::classify_block(e, np, k, max_out);
        if (want.nout && !ok) want = {fk::kStSingular, 0u, fk::kStickySingular};
        if (got.status != want.status || got.nout != want.nout || got.bit != want.bit) return 1;
        if (rec[lay.nout_off] != want.nout) return 2;
        if (!want.nout) continue;
        if (memcmp(&rec[lay.in_off], S.data(), k)) return 3;
        for (uint32_t i = 0, r = 0; i < k; ++i) {
            if ((mask >> i) & 1u) continue;
            if (rec[lay.out_off + r] != i || memcmp(&rec[lay.coef_off + (size_t)r * k], &T[(size_t)i * k], k)) return 4;
            ++r;
        }
    }
    const fk::WideLayout lay = fk::wide_layout(k, fk::some_rows(m));
    for (uint32_t want : wants) {
        std::vector<uint8_t> rec(lay.stride, 0xEE);
        const fk::SolveClass got =
            fk::solve_some_record(rec.data(), lay, mask, want, k, n, P.data(), cols, E, R, ex, lg);
        const uint32_t miss = ~mask & want & all, eo = fk::solve_popc(miss);
        const int32_t st = !eo ? 0 : np < k ? fk::kStTooFew : !ok ? fk::kStSingular : 0;
        const uint32_t nout = st ? 0u : eo;
        if (got.status != st || got.nout != nout || rec[lay.nout_off] != nout) return 5;
        if (got.bit != (st == fk::kStTooFew ? fk::kStickyTooFew : st ? fk::kStickySingular : 0)) return 6;
        if (!nout) continue;
        if (memcmp(&rec[lay.in_off], S.data(), k)) return 7;
        for (uint32_t i = 0, r = 0; i < n; ++i) {
            if (!((miss >> i) & 1u)) continue;
            if (rec[lay.out_off + r] != i || memcmp(&rec[lay.coef_off + (size_t)r * k], &T[(size_t)i * k], k)) return 8;
            ++r;
        }
    }
    return 0;
}

}  // namespace

extern "C" {

// Internal self-test (not part of the public ABI, no device needed): the elimination plan of a custom
// matrix (fec_solve.hpp: the statements the plan kernels of fec_plan_solve.hip run with a lane per
// column) against M[O] * inverse(M[S]) by rs::invert, a full k x k inversion. The four (8, 4) test
// matrices over every mask with 1..5 of the 12 shards missing (of those with 1..4 missing and a data
// shard among them, 778, the default rows and cauchy255 have no singular one, par1 8, lrc 172: counted
// here), each through the reconstruct / recover record for 0, 1 and 4 slots and the reconstruct-some
// record for want = every shard, data shard 0, parity shard 9, what is missing, and nothing; then
// cauchy255 of (20, 10), (16, 8), (16, 16), (1, 31), (31, 1) over 96 drawn masks each with 1..m + 1
// missing, none singular. 0 on success, else 100000 * (matrix or shape index + 1) + 10 * case + check.
int fec__selftest_custom_plan(void) {
    static const int want_singular[4] = {0, 0, 8, 172};
    for (int which = 0; which < 4; ++which) {
        const std::vector<uint8_t> P = custom_test_rows(which, 8, 4);
        int patterns = 0, singular = 0, ci = 0;
        for (uint32_t mask = 0; mask < (1u << 12); ++mask) {
            const uint32_t lost = 12 - fk::solve_popc(mask);
            if (lost < 1 || lost > 5) continue;
            ++ci;
            bool sing = false;
            const int rc = custom_check_mask(P, 8, 4, mask, {0xFFFFFFFFu, 1u, 1u << 9, ~mask, 0u}, &sing);
            if (rc) return 100000 * (which + 1) + 10 * ci + rc;
            if (lost <= 4 && (~mask & 0xFFu)) ++patterns, singular += sing;
        }
        if (patterns != 778 || singular != want_singular[which]) return 100000 * (which + 1) + 9;
    }
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto rnd = [&seed]() -> uint32_t {
        seed ^= seed << 13;
        seed ^= seed >> 7;
        seed ^= seed << 17;
        return (uint32_t)(seed >> 16);
    };
    static const int shapes[][2] = {{20, 10}, {16, 8}, {16, 16}, {1, 31}, {31, 1}};
    int si = 4;
    for (auto& sh : shapes) {
        ++si;
        const uint32_t k = (uint32_t)sh[0], m = (uint32_t)sh[1], n = k + m;
        const std::vector<uint8_t> P = custom_test_rows(1, (int)k, (int)m);
        for (int ci = 1; ci <= 96; ++ci) {
            uint32_t mask = fk::solve_low(n);
            for (uint32_t lose = 1 + rnd() % (m + 1); lose > 0;) {
                const uint32_t i = rnd() % n;
                if ((mask >> i) & 1u) mask &= ~(1u << i), --lose;
            }
            bool sing = false;
            const int rc = custom_check_mask(P, k, m, mask, {0xFFFFFFFFu, 1u << (rnd() % n), ~mask, 0u}, &sing);
            if (rc || sing) return 100000 * si + 10 * ci + (rc ? rc : 9);
        }
    }
    return 0;
}

// Internal, test-only like fec__set_tuning (not part of the public ABI, no device needed): the
// elimination plan of one block of the code with parity rows `rows` (m x k), k + m <= 32, by the
// statements the plan kernels run (solve_some_record). present, want: the block's masks (want
// 0xFFFFFFFF: every shard). Returns the number of shards the plan rebuilds (the missing wanted ones,
// ascending, into outputs_out: m bytes; their coefficient rows over the k inputs into coef_out:
// m * k bytes; the inputs into inputs_out: k bytes), or FEC_ERR_TOO_FEW_SHARDS / FEC_ERR_SINGULAR
// (nothing written), or FEC_ERR_INVALID_ARG.
int fec__custom_plan(int k, int m, const uint8_t* rows, uint32_t present, uint32_t want, uint8_t* inputs_out,
                     uint8_t* outputs_out, uint8_t* coef_out) {
    if (k <= 0 || m <= 0 || k + m > FEC_MAX_DECODE_SHARDS || !rows || !inputs_out || !outputs_out || !coef_out)
        return FEC_ERR_INVALID_ARG;
    const fk::WideLayout lay = fk::wide_layout((uint32_t)k, fk::some_rows((uint32_t)m));
    std::vector<uint8_t> rec(lay.stride, 0);
    uint8_t cols[fk::kSolveColBytes], E[fk::kSolveMaxE], R[fk::kSolveMaxE];
    const fk::SolveClass sc = fk::solve_some_record(rec.data(), lay, present, want, (uint32_t)k, (uint32_t)(k + m), rows,
                                                    cols, E, R, gf::kTables.exp, gf::kTables.log);
    if (sc.status) return sc.status;
    if (!sc.nout) return 0;
    memcpy(inputs_out, &rec[lay.in_off], (size_t)k);
    memcpy(outputs_out, &rec[lay.out_off], sc.nout);
    memcpy(coef_out, &rec[lay.coef_off], (size_t)sc.nout * k);
    return (int)sc.nout;
}

}  // extern "C"
