// fec_wide.hpp — wide RS decode (codes of up to 256 shards, present masks of 1..8 words): the
// plan record layout, the coefficient arithmetic shared by the plan kernel and the host self-test,
// and the launch interface of fec_wide.hip.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "fec_kernels.hpp"
#include "gf256.h"

namespace fk {

constexpr uint32_t kWideMaxShards = 256;
constexpr uint32_t kWideMaskWords = 8;     // 256 / 32
constexpr uint32_t kWideRowPass = 16;      // output rows accumulated per pass (uint32 acc[16][4])
constexpr uint32_t kWideTileTabs = 112;    // PermTab rows-of-16 a workgroup keeps: blocks * inputs per tile
constexpr uint32_t kWideMaxTileBlocks = 14;

// Wide plan record, one of `stride` bytes per block (in block order):
//   [in_off,   +rup8(k))  the first k present shards, ascending (zero padded)
//   [out_off,  +rows)     the shards to rebuild, ascending: erased data shards (reconstruct-some:
//                         the wanted missing shards, data and parity)
//   [nout_off]            shards to rebuild (0: nothing / failed); <= min(k, m) <= 128
//                         (reconstruct-some: <= m <= 255)
//   [coef_off, +rows*k)   GF coefficients, row r = output r, column p = input p
// [0, coef_off) is the record's header: the rebuild stages it in LDS and reads the coefficient
// bytes straight from the record.
struct WideLayout {
    uint32_t in_off, out_off, nout_off, coef_off, stride;
};
GF_HD inline WideLayout wide_layout(uint32_t k, uint32_t rows) {
    WideLayout l;
    l.in_off = 0;
    l.out_off = (k + 7) & ~7u;
    l.nout_off = l.out_off + rows;
    l.coef_off = (l.nout_off + 1 + 15) & ~15u;   // <= 272 for every k + m <= 256
    l.stride = (l.coef_off + rows * k + 15) & ~15u;
    return l;
}
constexpr uint32_t kWideHdrMax = 272;

// exp over the whole range of N_r + 510 - log - D_p (N_r, D_p, log <= 254): 768 entries, no
// reduction mod 255 at the lookup.
GF_HD inline uint8_t wide_exp768(uint32_t i) { return gf::kTables.exp[i % 255u]; }

// sum over q < k, q != skip of log(x ^ S[q]), mod 255 (skip >= k: every q). x ^ S[q] is nonzero
// for every term taken: the shard indices are distinct. logv (null: the default matrix) adds log v_x,
// the multiplier of shard x in a code whose shard r is v_r p(r) (rs_matrix.hpp grs_logv): D_p and N_r
// each take their own shard's, and wide_coef below is then exp(N_o + log v_o - log(o ^ s) - D_s - log v_s).
GF_HD inline uint32_t wide_logsum(const uint8_t* lg, const uint8_t* S, uint32_t k, uint32_t x, uint32_t skip,
                                  const uint8_t* logv = nullptr) {
    uint32_t d = logv ? logv[x] : 0u;
    for (uint32_t q = 0; q < k; ++q)
        if (q != skip) d += lg[x ^ S[q]];
    return d % 255u;
}

// The decode coefficient of input shard s (= S[p]) in erased data shard o (= O[r]), by Lagrange
// interpolation over the shard indices (fec_decode.hip, rs_plan_kernel):
//   coef[r][p] = prod_{q != p} (o ^ S[q]) / (S[p] ^ S[q]) = exp(N_r - log(o ^ s) - D_p)
// with N_r = wide_logsum(o, all q) and D_p = wide_logsum(S[p], q != p).
GF_HD inline uint8_t wide_coef(const uint8_t* ex768, const uint8_t* lg, uint32_t Nr, uint32_t Dp, uint32_t o,
                               uint32_t s) {
    return ex768[Nr + 510u - lg[o ^ s] - Dp];
}

struct WidePlanArgs {
    const uint32_t* masks;     // nblocks * mask_words
    uint32_t mask_words;
    const uint32_t* want;      // reconstruct-some: nblocks * mask_words want words (null: every shard)
    uint8_t* plans;            // nblocks * lay.stride bytes
    int32_t* status;           // optional
    int* err;                  // sticky error word
    uint32_t k, n, nblocks;
    uint32_t rows;             // output rows a record holds
    uint32_t max_out;          // recover: output slots per block (0: in place)
    WideLayout lay;
    FastDiv div_k;
    const uint8_t* logv;       // n bytes, log v_r per shard (PlanArgs::logv); null for the default matrix
};

// A workgroup rebuilds a tile of g consecutive blocks x c consecutive chunks (g * c <= 256, one
// lane per (block, chunk)); PermTabs of 16 rows x tk inputs of each block are in LDS at a time.
struct WideReconArgs {
    uint8_t* data;
    const uint8_t* parity;     // read only, but for reconstruct-some, which rebuilds parity shards too
    uint64_t dbs, pbs;
    uint32_t ss;
    const uint8_t* plans;
    WideLayout lay;
    uint32_t k, len, cps, nblocks;
    uint32_t g, c, tk;
    uint32_t nctiles;          // ceil(cps / c)
    uint32_t ntiles;           // ceil(nblocks / g) * nctiles
    FastDiv div_c, div_nct;
    uint8_t* out;              // recover: rebuilt shard r of block b at out + b*out_bs + r*ss
    uint64_t out_bs;
};

// Tile shape for shards of cps chunks of a code with k data shards.
inline void wide_tile_shape(uint32_t cps, uint32_t k, uint32_t* g, uint32_t* c, uint32_t* tk) {
    *c = cps < (uint32_t)kThreads ? cps : (uint32_t)kThreads;
    uint32_t G = (uint32_t)kThreads / *c;
    if (G > kWideMaxTileBlocks) G = kWideMaxTileBlocks;
    *g = G;
    uint32_t t = (kWideTileTabs / G) & ~7u;   // >= 8
    const uint32_t k8 = (k + 7) & ~7u;
    *tk = t < k8 ? t : k8;
}
inline size_t wide_recon_lds(uint32_t g, uint32_t tk, const WideLayout& lay) {
    return (size_t)g * kWideRowPass * tk * 32 + (size_t)g * lay.coef_off;
}

// some: the records of wide reconstruct-some (outputs: the wanted missing shards, data and parity;
// a.rows = some_rows(m), fec_some.hpp), else those of wide reconstruct / recover (a.want unused).
hipError_t launch_rs_plan_wide(const WidePlanArgs& a, bool some, hipStream_t s);
// some: the reconstruct-some form of the tile (records of fec_some.hpp; rebuilt shards go to their own
// slots in the data and the parity region, a.out unused), else the wide reconstruct / recover form.
hipError_t launch_rs_rebuild_wide(const WideReconArgs& a, bool some, hipStream_t s);

}  // namespace fk
