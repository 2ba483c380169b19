// fec_ragged.hpp — ragged batches (a shard length per block): the item arithmetic shared by the
// kernels of fec_ragged.hip and the host self-tests (fec__selftest_ragged_tiles and
// fec__selftest_ragged_some, fec_selftest.cpp), and
// the launch interface of fec_ragged.hip.
//
// A workgroup takes one window of one tile. A tile is G consecutive blocks; its items are the
// 16-byte column chunks of those blocks, numbered block after block: block g of the tile owns the
// local items [prefix[g], prefix[g + 1]), prefix = the exclusive prefix sum of the blocks' chunk
// counts (a block of length 0, or longer than the call's max_shard_len, counts zero chunks). A
// window is kRagWindow consecutive local items (kRagRounds rounds of one item per lane), so no
// workgroup runs more than kRagRounds rounds however long the shards are; the windows of a tile are
// sized for G full-length blocks, and a window that starts at or past the tile's item count exits.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "fec_kernels.hpp"
#include "fec_wide.hpp"
#include "gf256.h"

namespace fk {

constexpr uint32_t kRagMaxTileBlocks = 256;                    // one lane per block forms the prefix
constexpr uint32_t kRagRounds = 8;                             // rounds of a full window
constexpr uint32_t kRagWindow = kRagRounds * (uint32_t)kThreads;   // items per window
constexpr uint32_t kRagMaxTileItems = 1u << 31;                // local items are 32-bit

// 16-byte chunks block b contributes: none when it is empty or oversize (the comparison comes
// first: len + 15 would wrap for lengths near 2^32).
GF_HD inline uint32_t rag_chunks(uint32_t len, uint32_t max_len) {
    return len > max_len ? 0u : (len + (uint32_t)kChunk - 1u) / (uint32_t)kChunk;
}

// Blocks per tile: `want` bounded by one lane per block and by 32-bit local items of full-length
// blocks (cps_max = chunks of a shard of max_shard_len bytes, >= 1).
GF_HD inline uint32_t rag_clamp_blocks(uint32_t want, uint32_t cps_max) {
    uint32_t g = want < 1u ? 1u : want;
    if (g > kRagMaxTileBlocks) g = kRagMaxTileBlocks;
    const uint32_t by_items = kRagMaxTileItems / cps_max;      // >= 32 for shards of up to 2^30 bytes
    if (g > by_items) g = by_items;
    return g < 1u ? 1u : g;
}

// Windows per tile: enough for G full-length blocks, at least one.
GF_HD inline uint32_t rag_windows(uint32_t g, uint32_t cps_max) {
    const uint64_t items = (uint64_t)g * cps_max;
    const uint64_t w = (items + kRagWindow - 1) / kRagWindow;
    return w < 1 ? 1u : (uint32_t)w;
}

// Workgroup `wg` of a launch of ntiles * nwin workgroups: its tile's first block, the blocks the
// tile holds, and its window.
struct RagTile {
    uint32_t b0, gt, win;
};
GF_HD inline RagTile rag_tile(uint32_t wg, uint32_t g, uint32_t nwin, uint32_t nblocks) {
    RagTile t;
    const uint32_t bt = wg / nwin;
    t.win = wg - bt * nwin;
    t.b0 = bt * g;
    const uint32_t left = nblocks - t.b0;
    t.gt = left < g ? left : g;
    return t;
}

// The local items [lo, hi) of window `win` of a tile of `total` items (lo >= hi: nothing to do).
struct RagSpan {
    uint32_t lo, hi;
};
GF_HD inline RagSpan rag_span(uint32_t win, uint32_t total) {
    RagSpan s;
    const uint64_t lo = (uint64_t)win * kRagWindow;
    s.lo = lo < total ? (uint32_t)lo : total;
    const uint64_t hi = lo + kRagWindow;
    s.hi = hi < total ? (uint32_t)hi : total;
    return s;
}

// The block of local item t < prefix[gt]: the largest g < gt with prefix[g] <= t. Blocks of zero
// chunks repeat their prefix value and are never returned (prefix[g + 1] > t for the result).
GF_HD inline uint32_t rag_locate(const uint32_t* prefix, uint32_t gt, uint32_t t) {
    uint32_t lo = 0, hi = gt;   // the first index in (0, gt] whose prefix exceeds t is in (lo, hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct RagEncodeArgs {
    const uint8_t* in;         // data shard 0 of block 0
    uint8_t* out;              // parity shard 0 of this row pass, block 0
    uint64_t in_bs, out_bs, ss;
    uint32_t k, m;             // m: parity rows of this pass (<= 16)
    uint32_t max_len, nblocks;
    uint32_t g, nwin;          // blocks per tile, windows per tile
    const uint32_t* lens;      // nblocks shard lengths
    int32_t* status;           // optional; written by the pass with `report` set
    int* err;                  // sticky error word (bit 8: an oversize block)
    uint32_t report;
    const uint32_t* tabs;      // m * k PermTabs of this pass, device memory
};

struct RagReconArgs {
    ReconArgs r;               // r.g blocks per tile, r.plans in block order, r.status / r.err the
                               // per-block status (optional) and the sticky error word
    const uint32_t* lens;
    uint32_t max_len, nwin;
    uint32_t rows;             // rows a block can need: min(r.maxe, a recover's out slots)
};

// Ragged verify: one pass of m <= 16 parity rows over the encode's tiles and windows, the stored
// parity folded in (fec_verify.hpp VerifyArgs).
struct RagVerifyArgs {
    const uint8_t* in;         // data shard 0 of block 0
    const uint8_t* par;        // the pass's first parity shard of block 0
    uint64_t in_bs, par_bs, ss;
    uint32_t k, m;             // m: parity rows of this pass (<= 16)
    uint32_t max_len, nblocks;
    uint32_t g, nwin;
    const uint32_t* lens;
    int32_t* status;           // nblocks words, 1 on entry (or 0 from an earlier pass)
    uint32_t* count;           // optional: blocks whose status went from 1 to 0
    int* err;                  // sticky error word (an oversize block)
    uint32_t report;           // the first row pass: oversize blocks get their status
    const uint32_t* tabs;      // m * k PermTabs of this pass, device memory
};

// Ragged reconstruct-some: the records of fec_some.hpp (WideLayout, `rows` = some_rows(m) rows, block
// order), rebuilt shards into their own slots of the data and the parity region. Output rows go in
// passes of kWideRowPass; a block's tables of one pass take rag_some_pass_rows(rows) * k entries.
struct RagSomeArgs {
    uint8_t* data;
    uint8_t* parity;
    uint64_t dbs, pbs;
    uint32_t ss;
    const uint8_t* plans;
    WideLayout lay;
    uint32_t k, nblocks, max_len;
    uint32_t g, nwin;
    uint32_t rows;             // rows a record holds
    const uint32_t* lens;
    int32_t* status;           // optional; the plan kernel's, overridden for oversize blocks
    int* err;
};

// Table rows a block keeps in LDS at a time, and the row passes of a record of `rows` rows.
GF_HD inline uint32_t rag_some_pass_rows(uint32_t rows) { return rows < kWideRowPass ? rows : kWideRowPass; }
GF_HD inline uint32_t rag_some_passes(uint32_t rows) { return (rows + kWideRowPass - 1) / kWideRowPass; }
// The rows the kernel instance that serves passes of prow rows is compiled for (12: RS(20,30)'s ten
// rows, as the ragged rebuild's 12-row instance).
GF_HD inline uint32_t rag_some_instance(uint32_t prow) {
    return prow <= 1 ? 1u : prow <= 2 ? 2u : prow <= 4 ? 4u : prow <= 8 ? 8u : prow <= 12 ? 12u : kWideRowPass;
}
// The rows block-local pass p (from row p * kWideRowPass) rebuilds of a block with nout outputs.
GF_HD inline uint32_t rag_some_rows_in_pass(uint32_t nout, uint32_t r0) {
    return nout > r0 ? (nout - r0 < kWideRowPass ? nout - r0 : kWideRowPass) : 0u;
}

// Blocks per tile the rebuilds may hold in LDS beside their prefix arrays (64 KiB budget, so that more
// than one workgroup fits a CU): the reconstruct with `rows` table rows per block, reconstruct-some
// with one row pass of tables and the whole record per block; and the LDS a tile of g blocks takes.
uint32_t rag_recon_max_blocks(uint32_t k, uint32_t rows, const PlanLayout& lay);
uint32_t rag_some_max_blocks(uint32_t k, uint32_t rows, const WideLayout& lay);
size_t rag_some_lds(uint32_t g, uint32_t k, uint32_t rows, const WideLayout& lay);
constexpr size_t kRagLdsBudget = 64u * 1024u;

hipError_t launch_rs_encode_ragged(const RagEncodeArgs& a, hipStream_t s);
hipError_t launch_rs_reconstruct_ragged(const RagReconArgs& a, hipStream_t s);
hipError_t launch_rs_verify_ragged(const RagVerifyArgs& a, hipStream_t s);
hipError_t launch_rs_reconstruct_some_ragged(const RagSomeArgs& a, hipStream_t s);

}  // namespace fk
