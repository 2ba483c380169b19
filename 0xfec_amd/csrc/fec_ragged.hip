// fec_ragged.hip — RS encode and rebuild of ragged batches for gfx950: every block has its own
// shard length (the reference's shard is 2 + the block's biggest payload, reed_solomon.go:47,80),
// and lane work and HBM traffic follow the sum of the blocks' chunk counts instead of nblocks times
// the longest shard. A workgroup takes one window of one tile of G consecutive blocks
// (fec_ragged.hpp): it reads the G lengths, forms the exclusive prefix of their chunk counts in
// LDS (a wave scan and one add of the wave totals), and sweeps its window's local items in rounds
// of 256, each lane finding its (block, chunk) in the prefix by binary search. No global scan pass,
// no extra kernel. The encode body is rs_encode_kernel's (fec_encode.hip), the rebuild is
// rs_reconstruct_kernel's tile form around recon_item (fec_decode.hip, fec_recon.hpp) over the plan
// kernel's block-order records; a block's own length shapes its tail chunk. The verify is
// rs_verify_kernel's body (fec_verify.hip) on the encode's walk, and reconstruct-some the rebuild's
// walk over the records of fec_some.hpp with rs_rebuild_wide_kernel's row passes (fec_wide.hip).
//
// Control flow: every barrier is reached by all 256 lanes; what is tested before a barrier (the
// tile, the window, the tile's item count) is the same for the whole workgroup.
#include "fec_ragged.hpp"
#include "fec_recon.hpp"

namespace fk {

// LDS in front of each kernel's own: prefix[kRagMaxTileBlocks + 1], the blocks' lengths, the four
// wave totals of the scan and the four wave maxima of the row counts; rounded up so that the
// PermTabs behind it stay 32-byte aligned.
constexpr size_t kRagLds = ((2 * kRagMaxTileBlocks + 1 + 8) * 4 + 31) & ~(size_t)31;
static_assert(kRagMaxTileBlocks <= (uint32_t)kThreads, "one lane per block of a tile");

struct RagLds {
    uint32_t* prefix;   // gt + 1
    uint32_t* len;      // gt
    uint32_t* wsum;     // kThreads / 64
    uint32_t* wmax;     // kThreads / 64
};
__device__ __forceinline__ RagLds rag_lds(uint8_t* smem) {
    uint32_t* w = reinterpret_cast<uint32_t*>(smem);
    return {w, w + kRagMaxTileBlocks + 1, w + 2 * kRagMaxTileBlocks + 1, w + 2 * kRagMaxTileBlocks + 5};
}

__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v += o;
    }
    return v;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = max(v, (uint32_t)__shfl_xor(v, d, 64));
    return v;
}

// Lengths and prefix of tile T into LDS; returns the tile's item count and the largest `rows` of
// its blocks that have chunks. Lane i owns block i of the tile; `rows` is that block's row count
// (the rebuild: erased shards to rebuild; the encode: unused). With `report` (the tile's first
// window) an oversize block gets status kStShardSize and sets kStickyOversize, and with `zero`
// every other block gets status 0 (encode: no plan kernel wrote one). Two barriers, reached by
// every lane; LDS written by the caller before the call is visible after it.
struct TileSum {
    uint32_t total, rows;
};
__device__ __forceinline__ TileSum tile_prefix(const uint32_t* lens, const RagTile& T, uint32_t max_len,
                                               int32_t* status, int* err, bool report, bool zero, const RagLds& L,
                                               uint32_t rows = 0) {
    const uint32_t i = threadIdx.x;
    const bool mine = i < T.gt;
    const uint32_t len = mine ? lens[T.b0 + i] : 0u;
    if (report && mine) {
        if (len > max_len) {
            if (status) status[T.b0 + i] = kStShardSize;
            wave_flag(err, kStickyOversize);
        } else if (zero && status) {
            status[T.b0 + i] = 0;
        }
    }
    const uint32_t cnt = rag_chunks(len, max_len);
    const uint32_t incl = wave_inclusive_sum(cnt);
    const uint32_t wrows = wave_max(cnt ? rows : 0u);
    if ((i & 63u) == 63u) {
        L.wsum[i >> 6] = incl;
        L.wmax[i >> 6] = wrows;
    }
    if (mine) L.len[i] = len;
    __syncthreads();
    uint32_t off = 0;
    for (uint32_t w = 0; w < (i >> 6); ++w) off += L.wsum[w];
    if (mine) L.prefix[i + 1] = incl + off;
    if (i == 0) L.prefix[0] = 0;
    __syncthreads();
    return {L.prefix[T.gt], max(max(L.wmax[0], L.wmax[1]), max(L.wmax[2], L.wmax[3]))};
}

// ------------------------------------------------------------------ ragged RS encode
// One lane = one 16-byte column chunk of one block, all m parities of the row pass in VGPRs, runtime
// k, inputs 8 shards at a time: rs_encode_kernel's body. The pass's tables are staged in LDS while
// they fit 64 KiB (m * k <= kMaxLdsTabs), else read from global memory; the staging is issued
// before the lengths are read and is published by the prefix's barriers.
template <int MAXM, bool LDS_TABS>
__global__ __launch_bounds__(kThreads) void rs_encode_ragged_kernel(RagEncodeArgs a) {
    constexpr bool NTS = true;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const RagLds L = rag_lds(smem);
    const RagTile T = rag_tile(xcd_order(), a.g, a.nwin, a.nblocks);
    const gf::PermTab* tabs = stage_tabs<LDS_TABS>(a.tabs, a.m * a.k * 8, smem + kRagLds);
    const uint32_t total = tile_prefix(a.lens, T, a.max_len, a.status, a.err, a.report && T.win == 0, true, L).total;
    const RagSpan span = rag_span(T.win, total);
    if (span.lo >= span.hi) return;   // workgroup-uniform
    const uint32_t k = a.k, m = a.m;
    for (uint32_t base = span.lo; base < span.hi; base += kThreads) {
        const uint32_t t = base + threadIdx.x;
        if (t >= span.hi) continue;
        const uint32_t g = rag_locate(L.prefix, T.gt, t);
        const uint32_t c = t - L.prefix[g];
        const uint32_t b = T.b0 + g;
        const uint8_t* src = a.in + (uint64_t)b * a.in_bs + (uint64_t)c * kChunk;
        uint32_t acc[MAXM][4];
#pragma unroll
        for (int r = 0; r < MAXM; ++r) acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = 0;
        for (uint32_t j0 = 0; j0 < k; j0 += kInGroup) {
            uint4 x[kInGroup];
            load_shards(x, src, a.ss, j0, k);
            fold_group<MAXM>(acc, x, m, tabs, k, j0, k);
        }
        uint8_t* dst = a.out + (uint64_t)b * a.out_bs + (uint64_t)c * kChunk;
        const uint32_t nb = L.len[g] - c * kChunk;   // >= 1: chunk c starts below the block's length
#pragma unroll
        for (int r = 0; r < MAXM; ++r)
            if (r < (int)m) store_chunk<NTS>(dst + (uint64_t)r * a.ss, as_uint4(acc[r]), nb);
    }
}

// ------------------------------------------------------------------ ragged RS rebuild
// rs_reconstruct_kernel's tile form: the tile's plan records staged in LDS (issued before the
// lengths are read, published by the prefix's barriers), the coefficients expanded to PermTabs once
// per workgroup, then the window's items; each item loops to its wave's largest erasure count.
// Only the rows the tile needs are expanded: up to the largest erasure count among its blocks that
// have chunks (rows past a block's own count carry zero tables); a tile with nothing to rebuild, or
// a window with no items, returns after the prefix. ra.rows bounds a block's rows (the code's
// min(k, m), or a recover's out slots when fewer: the plan kernel leaves blocks with more erasures
// than slots at zero rows); a block's tables take ra.rows * k entries and MAXE >= ra.rows.
template <int MAXE>
__global__ __launch_bounds__(kThreads) void rs_reconstruct_ragged_kernel(RagReconArgs ra) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const ReconArgs& a = ra.r;
    const uint32_t k = a.k, G = a.g, tstride = ra.rows * k;
    const PlanLayout lay = a.lay;
    const RagLds L = rag_lds(smem);
    gf::PermTab* tabs = reinterpret_cast<gf::PermTab*>(smem + kRagLds);                 // G*rows*k
    uint8_t* plans = smem + kRagLds + (size_t)G * tstride * sizeof(gf::PermTab);        // G*stride
    const RagTile T = rag_tile(xcd_order(), G, ra.nwin, a.nblocks);
    const uint8_t* gplans = a.plans + (uint64_t)T.b0 * lay.stride;
    {
        const uint32_t nw = T.gt * lay.stride / 16;
        const uint4* src = reinterpret_cast<const uint4*>(gplans);
        uint4* dst = reinterpret_cast<uint4*>(plans);
        for (uint32_t i = threadIdx.x; i < nw; i += kThreads) dst[i] = src[i];
    }
    const uint32_t my_rows = threadIdx.x < T.gt ? gplans[threadIdx.x * lay.stride + lay.nout_off] : 0u;
    const TileSum ts = tile_prefix(ra.lens, T, ra.max_len, a.status, a.err, T.win == 0, false, L, my_rows);
    const RagSpan span = rag_span(T.win, ts.total);
    if (span.lo >= span.hi || ts.rows == 0) return;   // workgroup-uniform
    {
        const uint32_t trows = min(ts.rows, ra.rows);   // (a record never holds more than ra.rows)
        const uint32_t per = trows * k, ne = T.gt * per;
        for (uint32_t i = threadIdx.x; i < ne; i += kThreads) {
            const uint32_t g = i / per;
            const uint32_t rem = i - g * per;
            const uint32_t r = rem / k, j = rem - r * k;
            const uint8_t* P = plans + g * lay.stride;
            const uint8_t c = r < P[lay.nout_off] ? P[lay.coef_off + r * k + j] : 0;
            tabs[g * tstride + rem] = gf::make_permtab_fast(c);
        }
    }
    __syncthreads();
    for (uint32_t base = span.lo; base < span.hi; base += kThreads) {
        const uint32_t t = base + threadIdx.x;
        const bool inr = t < span.hi;
        const uint32_t g = inr ? rag_locate(L.prefix, T.gt, t) : 0;
        const uint32_t c = t - L.prefix[g];
        const uint8_t* P = plans + g * lay.stride;
        const uint32_t nout = inr ? P[lay.nout_off] : 0;
        const uint32_t rows = wave_rows<MAXE>(nout);
        if (nout == 0) continue;
        ReconArgs item = a;
        item.len = L.len[g];   // the tail chunk is the block's own
        recon_item<MAXE>(item, P, tabs + g * tstride, T.b0 + g, c, rows, nout);
    }
}

// ------------------------------------------------------------------ ragged RS verify
// rs_verify_kernel's body (fec_verify.hip) over the encode's tiles and windows: the accumulators
// start from the stored parity chunks, the k data chunks are folded in, and what is left, ORed over
// the pass's rows under the block's own tail mask, is the difference between stored and computed
// parity. The statuses are 1 on entry (oversize blocks: kStShardSize from the first pass's first
// window, after the memset in stream order; they have no items, so no lane meets them). A wave's
// lanes lie in as many blocks as the lengths make them: among the lanes that found a difference the
// first of each block exchanges 0 into the block's word and counts the block if it read back 1, so
// a block is counted once however many chunks, windows, workgroups or row passes find it bad, and
// a clean batch issues no atomics. Every lane of a wave reaches the ballots: the round loop's bounds
// are the workgroup's, and a lane past the window's end only skips its loads.
template <int MAXM, bool LDS_TABS>
__global__ __launch_bounds__(kThreads) void rs_verify_ragged_kernel(RagVerifyArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const RagLds L = rag_lds(smem);
    const RagTile T = rag_tile(xcd_order(), a.g, a.nwin, a.nblocks);
    const gf::PermTab* tabs = stage_tabs<LDS_TABS>(a.tabs, a.m * a.k * 8, smem + kRagLds);
    const uint32_t total = tile_prefix(a.lens, T, a.max_len, a.status, a.err, a.report && T.win == 0, false, L).total;
    const RagSpan span = rag_span(T.win, total);
    if (span.lo >= span.hi) return;   // workgroup-uniform
    const uint32_t k = a.k, m = a.m;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t base = span.lo; base < span.hi; base += kThreads) {
        const uint32_t t = base + threadIdx.x;
        const bool inr = t < span.hi;
        uint32_t b = 0;
        bool bad = false;
        if (inr) {
            const uint32_t g = rag_locate(L.prefix, T.gt, t);
            const uint32_t c = t - L.prefix[g];
            b = T.b0 + g;
            const uint8_t* src = a.in + (uint64_t)b * a.in_bs + (uint64_t)c * kChunk;
            const uint8_t* par = a.par + (uint64_t)b * a.par_bs + (uint64_t)c * kChunk;
            uint32_t acc[MAXM][4];
#pragma unroll
            for (int r = 0; r < MAXM; ++r) {
                const uint4 p = r < (int)m ? ld16<true>(par + (uint64_t)r * a.ss) : make_uint4(0, 0, 0, 0);
                acc[r][0] = p.x, acc[r][1] = p.y, acc[r][2] = p.z, acc[r][3] = p.w;
            }
            for (uint32_t j0 = 0; j0 < k; j0 += kInGroup) {
                uint4 x[kInGroup];
                load_shards(x, src, a.ss, j0, k);
                fold_group<MAXM>(acc, x, m, tabs, k, j0, k);
            }
            uint4 d = make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < MAXM; ++r)
                if (r < (int)m) d.x |= acc[r][0], d.y |= acc[r][1], d.z |= acc[r][2], d.w |= acc[r][3];
            d = keep_bytes(d, L.len[g] - c * kChunk);   // >= 1 byte: chunk c starts below the block's length
            bad = (d.x | d.y | d.z | d.w) != 0;
        }
        uint64_t todo = __ballot(bad);   // wave-uniform
        while (todo) {
            const uint32_t leader = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
            const uint32_t lb = (uint32_t)__shfl((int)b, (int)leader);
            todo &= ~__ballot(bad && b == lb);
            if (lane == leader)
                if (atomicExch(a.status + b, 0) == 1 && a.count) atomicAdd(a.count, 1u);
        }
    }
}

// ------------------------------------------------------------------ ragged RS reconstruct-some
// The ragged tile walk over reconstruct-some's records (fec_some.hpp; WideLayout, block order): the
// tile's records staged in LDS whole (issued before the lengths are read, published by the prefix's
// barriers), then, as rs_rebuild_wide_kernel, output rows in passes of kWideRowPass: for each pass
// the workgroup expands that pass's coefficient rows of its blocks into PermTabs (rows past a
// block's own count carry zero tables) and sweeps the window's items, each rebuilding the pass's
// rows of its block into the shards' own slots: the data region below k, the parity region from k
// on. A block's inputs (present shards) and outputs (missing ones) are disjoint slots and a lane
// reads and writes its own chunk column only, so a later pass reads what no earlier one wrote. The
// pass loop runs to the largest row count among the tile's blocks that have chunks: the same for
// every lane, as is the window, so every barrier is reached by all 256 lanes.
template <int MAXE>
__global__ __launch_bounds__(kThreads) void rs_reconstruct_some_ragged_kernel(RagSomeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t k = a.k, G = a.g, tstride = rag_some_pass_rows(a.rows) * k;
    const WideLayout lay = a.lay;
    const RagLds L = rag_lds(smem);
    gf::PermTab* tabs = reinterpret_cast<gf::PermTab*>(smem + kRagLds);                 // G*tstride
    uint8_t* plans = smem + kRagLds + (size_t)G * tstride * sizeof(gf::PermTab);        // G*stride
    const RagTile T = rag_tile(xcd_order(), G, a.nwin, a.nblocks);
    const uint8_t* gplans = a.plans + (uint64_t)T.b0 * lay.stride;
    {
        const uint32_t nw = T.gt * lay.stride / 16;
        const uint4* src = reinterpret_cast<const uint4*>(gplans);
        uint4* dst = reinterpret_cast<uint4*>(plans);
        for (uint32_t i = threadIdx.x; i < nw; i += kThreads) dst[i] = src[i];
    }
    const uint32_t my_rows = threadIdx.x < T.gt ? gplans[threadIdx.x * lay.stride + lay.nout_off] : 0u;
    const TileSum ts = tile_prefix(a.lens, T, a.max_len, a.status, a.err, T.win == 0, false, L, my_rows);
    const RagSpan span = rag_span(T.win, ts.total);
    if (span.lo >= span.hi || ts.rows == 0) return;   // workgroup-uniform
    const uint32_t trows = min(ts.rows, a.rows);      // (a record never holds more than a.rows)
    for (uint32_t r0 = 0; r0 < trows; r0 += kWideRowPass) {
        const uint32_t rp = min(kWideRowPass, trows - r0);   // <= rag_some_pass_rows(a.rows)
        if (r0) __syncthreads();   // the previous pass's tables are consumed
        {
            const uint32_t per = rp * k, ne = T.gt * per;
            for (uint32_t i = threadIdx.x; i < ne; i += kThreads) {
                const uint32_t g = i / per;
                const uint32_t rem = i - g * per;
                const uint32_t r = rem / k, j = rem - r * k;
                const uint8_t* P = plans + g * lay.stride;
                const uint8_t c = r0 + r < P[lay.nout_off] ? P[lay.coef_off + (r0 + r) * k + j] : 0;
                tabs[g * tstride + rem] = gf::make_permtab_fast(c);
            }
        }
        __syncthreads();
        for (uint32_t base = span.lo; base < span.hi; base += kThreads) {
            const uint32_t t = base + threadIdx.x;
            const bool inr = t < span.hi;
            const uint32_t g = inr ? rag_locate(L.prefix, T.gt, t) : 0;
            const uint32_t c = t - L.prefix[g];
            const uint8_t* P = plans + g * lay.stride;
            const uint32_t my = inr ? rag_some_rows_in_pass(P[lay.nout_off], r0) : 0u;
            const uint32_t rows = wave_rows<MAXE>(my);
            if (my == 0) continue;
            const uint32_t blk = T.b0 + g;
            uint8_t* dblk = a.data + (uint64_t)blk * a.dbs + (uint64_t)c * kChunk;
            uint8_t* pblk = a.parity + (uint64_t)blk * a.pbs + (uint64_t)c * kChunk;
            uint8_t* pbase = pblk - (uint64_t)k * a.ss;   // (parity_base: shard o >= k at pbase + o * ss)
            const gf::PermTab* Tb = tabs + g * tstride;
            uint32_t acc[MAXE][4];
#pragma unroll
            for (int r = 0; r < MAXE; ++r) acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = 0;
            for (uint32_t j0 = 0; j0 < k; j0 += kInGroup) {
                // the 8 input slots of this group (the list is zero padded to 8 bytes)
                const uint2 sl = *reinterpret_cast<const uint2*>(P + lay.in_off + j0);
                uint4 x[kInGroup];
#pragma unroll
                for (int jj = 0; jj < kInGroup; ++jj) {
                    const uint32_t w = jj < 4 ? sl.x : sl.y;
                    const uint32_t slot = (w >> (8 * (jj & 3))) & 0xFFu;
                    x[jj] = j0 + jj < k   // uniform predicate: no loads past input k-1
                                ? ld16<kNT>(slot_addr(dblk, pbase, slot, k, a.ss, a.ss))
                                : make_uint4(0, 0, 0, 0);
                }
                fold_group<MAXE>(acc, x, rows, Tb, k, j0, k);
            }
            const uint32_t nb = L.len[g] - c * kChunk;   // the tail chunk is the block's own
            const uint8_t* O = P + lay.out_off + r0;
#pragma unroll
            for (int r = 0; r < MAXE; ++r)
                if (r < (int)my) {
                    const uint32_t o = O[r];
                    store_chunk<kNT>((o < k ? dblk : pbase) + (uint64_t)o * a.ss, as_uint4(acc[r]), nb);
                }
        }
    }
}

// ------------------------------------------------------------------ launchers
static bool rag_grid(uint32_t nblocks, uint32_t g, uint32_t nwin, uint32_t* grid) {
    const uint64_t n = (uint64_t)((nblocks + g - 1) / g) * nwin;
    *grid = (uint32_t)n;
    return n > 0 && n < (uint64_t(1) << 31);
}

template <int MAXM>
static hipError_t rag_enc_dispatch(const RagEncodeArgs& a, uint32_t grid, hipStream_t s) {
    if (a.m * a.k <= (uint32_t)kMaxLdsTabs) {
        const size_t lds = occupancy_lds(g_tune.gen_wpc, kRagLds + (size_t)a.m * a.k * sizeof(gf::PermTab));
        hipLaunchKernelGGL((rs_encode_ragged_kernel<MAXM, true>), dim3(grid), dim3(kThreads), lds, s, a);
    } else {
        const size_t lds = occupancy_lds(g_tune.gen_wpc, kRagLds);
        hipLaunchKernelGGL((rs_encode_ragged_kernel<MAXM, false>), dim3(grid), dim3(kThreads), lds, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_rs_encode_ragged(const RagEncodeArgs& a, hipStream_t s) {
    if (a.nblocks == 0) return hipSuccess;
    uint32_t grid;
    if (a.g < 1 || a.g > kRagMaxTileBlocks || a.m > 16 || !rag_grid(a.nblocks, a.g, a.nwin, &grid))
        return hipErrorInvalidValue;
    if (a.m <= 1) return rag_enc_dispatch<1>(a, grid, s);
    if (a.m <= 2) return rag_enc_dispatch<2>(a, grid, s);
    if (a.m <= 4) return rag_enc_dispatch<4>(a, grid, s);
    if (a.m <= 8) return rag_enc_dispatch<8>(a, grid, s);
    if (a.m <= 12) return rag_enc_dispatch<12>(a, grid, s);
    return rag_enc_dispatch<16>(a, grid, s);   // caller splits m > 16
}

static size_t rag_recon_lds(uint32_t g, uint32_t k, uint32_t rows, const PlanLayout& lay) {
    return kRagLds + (size_t)g * rows * k * sizeof(gf::PermTab) + (size_t)g * lay.stride;
}

uint32_t rag_recon_max_blocks(uint32_t k, uint32_t rows, const PlanLayout& lay) {
    const size_t per_block = rag_recon_lds(1, k, rows, lay) - kRagLds;
    const size_t g = (kRagLdsBudget - kRagLds) / per_block;
    return g < 1 ? 1u : g > kRagMaxTileBlocks ? kRagMaxTileBlocks : (uint32_t)g;
}

hipError_t launch_rs_reconstruct_ragged(const RagReconArgs& ra, hipStream_t s) {
    const ReconArgs& a = ra.r;
    if (a.nblocks == 0) return hipSuccess;
    uint32_t grid;
    if (ra.rows < 1 || ra.rows > 16 || a.g < 1 || a.g > rag_recon_max_blocks(a.k, ra.rows, a.lay) ||
        !rag_grid(a.nblocks, a.g, ra.nwin, &grid))
        return hipErrorInvalidValue;
    const size_t lds = occupancy_lds(g_tune.dec_wpc, rag_recon_lds(a.g, a.k, ra.rows, a.lay));
#define FEC_RAG_LAUNCH(E) hipLaunchKernelGGL((rs_reconstruct_ragged_kernel<E>), dim3(grid), dim3(kThreads), lds, s, ra)
    if (ra.rows <= 1) FEC_RAG_LAUNCH(1);
    else if (ra.rows <= 2) FEC_RAG_LAUNCH(2);
    else if (ra.rows <= 4) FEC_RAG_LAUNCH(4);
    else if (ra.rows <= 8) FEC_RAG_LAUNCH(8);
    else if (ra.rows <= 12) FEC_RAG_LAUNCH(12);
    else FEC_RAG_LAUNCH(16);
#undef FEC_RAG_LAUNCH
    return hipGetLastError();
}

template <int MAXM>
static hipError_t rag_verify_dispatch(const RagVerifyArgs& a, uint32_t grid, hipStream_t s) {
    if (a.m * a.k <= (uint32_t)kMaxLdsTabs) {
        const size_t lds = occupancy_lds(g_tune.gen_wpc, kRagLds + (size_t)a.m * a.k * sizeof(gf::PermTab));
        hipLaunchKernelGGL((rs_verify_ragged_kernel<MAXM, true>), dim3(grid), dim3(kThreads), lds, s, a);
    } else {
        const size_t lds = occupancy_lds(g_tune.gen_wpc, kRagLds);
        hipLaunchKernelGGL((rs_verify_ragged_kernel<MAXM, false>), dim3(grid), dim3(kThreads), lds, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_rs_verify_ragged(const RagVerifyArgs& a, hipStream_t s) {
    if (a.nblocks == 0 || a.m == 0) return hipSuccess;
    uint32_t grid;
    if (a.g < 1 || a.g > kRagMaxTileBlocks || a.m > 16 || !rag_grid(a.nblocks, a.g, a.nwin, &grid))
        return hipErrorInvalidValue;
    if (a.m <= 1) return rag_verify_dispatch<1>(a, grid, s);
    if (a.m <= 2) return rag_verify_dispatch<2>(a, grid, s);
    if (a.m <= 4) return rag_verify_dispatch<4>(a, grid, s);
    if (a.m <= 8) return rag_verify_dispatch<8>(a, grid, s);
    return rag_verify_dispatch<16>(a, grid, s);   // the caller splits m > 16
}

size_t rag_some_lds(uint32_t g, uint32_t k, uint32_t rows, const WideLayout& lay) {
    return kRagLds + (size_t)g * rag_some_pass_rows(rows) * k * sizeof(gf::PermTab) + (size_t)g * lay.stride;
}

uint32_t rag_some_max_blocks(uint32_t k, uint32_t rows, const WideLayout& lay) {
    const size_t per_block = rag_some_lds(1, k, rows, lay) - kRagLds;
    const size_t g = (kRagLdsBudget - kRagLds) / per_block;
    return g < 1 ? 1u : g > kRagMaxTileBlocks ? kRagMaxTileBlocks : (uint32_t)g;
}

hipError_t launch_rs_reconstruct_some_ragged(const RagSomeArgs& a, hipStream_t s) {
    if (a.nblocks == 0) return hipSuccess;
    uint32_t grid;
    if (a.rows < 1 || a.g < 1 || a.g > rag_some_max_blocks(a.k, a.rows, a.lay) ||
        !rag_grid(a.nblocks, a.g, a.nwin, &grid))
        return hipErrorInvalidValue;
    const size_t lds = occupancy_lds(g_tune.dec_wpc, rag_some_lds(a.g, a.k, a.rows, a.lay));
#define FEC_RAG_LAUNCH(E) \
    case E: hipLaunchKernelGGL((rs_reconstruct_some_ragged_kernel<E>), dim3(grid), dim3(kThreads), lds, s, a); break
    switch (rag_some_instance(rag_some_pass_rows(a.rows))) {
        FEC_RAG_LAUNCH(1);
        FEC_RAG_LAUNCH(2);
        FEC_RAG_LAUNCH(4);
        FEC_RAG_LAUNCH(8);
        FEC_RAG_LAUNCH(12);
        default: FEC_RAG_LAUNCH(16);
    }
#undef FEC_RAG_LAUNCH
    return hipGetLastError();
}

}  // namespace fk
