// fec_wide.hip — wide RS decode for gfx950: codes of up to 256 shards (klauspost New(k, m) with
// k + m <= 256), present masks of 1..8 words per block. rs_plan_wide_kernel turns each block's mask
// into a record (inputs, shards to rebuild, e x k coefficient bytes, fec_wide.hpp): the erased data
// shards for wide reconstruct / recover, every wanted missing shard, parity included, for wide
// reconstruct-some. The rebuild is the generic encode's inner loop (fec_encode.hip rs_encode_kernel)
// over gathered inputs with a coefficient matrix per block.
#include "fec_recon.hpp"
#include "fec_wide.hpp"

namespace fk {

// ------------------------------------------------------------------ wide plan
// One wave per block, four blocks per workgroup. Lanes take shard indices lane, lane + 64, ..:
// ballots of the present and the to-rebuild bits give each shard its place in the input list S
// (the first k present, ascending) and the output list O (ascending). Lane p then builds D_p and
// lane r builds N_r (k-long sums over S in LDS), and the wave writes the e * k coefficient bytes,
// four per lane per store, straight into the record.
// The variable part is which shards go into O. SOME = false (wide reconstruct / recover): the
// missing data shards; recover (a.max_out set) reports their number and refuses more than its out
// slots. SOME = true (wide reconstruct-some): the missing shards below n that the block's want mask
// names (a.want null: every one), data and parity alike; in place, so a.max_out is not looked at.
// Either way a block that has something to rebuild and fewer than k shards present gets kStTooFew.
constexpr int kWidePlanWaves = kThreads / 64;

struct WidePlanWave {
    uint8_t hdr[kWideHdrMax];   // the record's header: S, O, nout
    uint8_t D[256];
    uint8_t N[256];             // up to 255 rows (reconstruct-some of RS(1,255))
};

template <bool SOME>
__global__ __launch_bounds__(kThreads) void rs_plan_wide_kernel(WidePlanArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_exp[768];
    __shared__ __attribute__((aligned(16))) uint8_t s_log[256];
    __shared__ __attribute__((aligned(16))) WidePlanWave s_w[kWidePlanWaves];
    for (uint32_t i = threadIdx.x; i < 768; i += kThreads) s_exp[i] = wide_exp768(i);
    for (uint32_t i = threadIdx.x; i < 256; i += kThreads) s_log[i] = gf::kTables.log[i];
    __syncthreads();   // the only workgroup barrier: waves part here
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t b = blockIdx.x * kWidePlanWaves + wave;
    if (b >= a.nblocks) return;
    WidePlanWave& W = s_w[wave];
    const WideLayout lay = a.lay;
    const uint32_t k = a.k, n = a.n;
    const uint32_t* mw = a.masks + (uint64_t)b * a.mask_words;
    const uint32_t* ww = SOME && a.want ? a.want + (uint64_t)b * a.mask_words : nullptr;
    const uint32_t max_out = SOME ? 0u : a.max_out;
    uint32_t* hdr32 = reinterpret_cast<uint32_t*>(W.hdr);
    const uint32_t hw = lay.coef_off / 4;
    for (uint32_t i = lane; i < hw; i += 64) hdr32[i] = 0;
    wave_sync();
    uint32_t npres = 0, e = 0;
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t idx = base + lane;
        // bits at and above n are ignored; idx < n implies idx / 32 < mask_words (checked by the host)
        const bool pres = idx < n && ((mw[idx >> 5] >> (idx & 31u)) & 1u);
        bool lost = idx < (SOME ? n : k) && !pres;
        if (SOME && ww) lost = lost && ((ww[idx >> 5] >> (idx & 31u)) & 1u);
        const uint64_t bp = __ballot(pres), bl = __ballot(lost);
        const uint32_t pp = npres + (uint32_t)__popcll(bp & below);
        const uint32_t pl = e + (uint32_t)__popcll(bl & below);
        if (pres && pp < k) W.hdr[lay.in_off + pp] = (uint8_t)idx;
        if (lost && pl < a.rows) W.hdr[lay.out_off + pl] = (uint8_t)idx;
        npres += (uint32_t)__popcll(bp);
        e += (uint32_t)__popcll(bl);
    }
    // statuses and the sticky word by the rule of fec_status.hpp (classify_block), as rs_plan_kernel
    int32_t st = max_out ? (int32_t)e : 0;   // recover reports the rebuilt count
    uint32_t nout = 0;
    if (e == 0) {
    } else if (npres < k) {
        st = kStTooFew;
        if (lane == 0) wave_flag(a.err, kStickyTooFew);
    } else if (max_out && e > max_out) {
        st = kStSlots;
        if (lane == 0) wave_flag(a.err, kStickySlots);
    } else {
        // <= rows: a recoverable block misses at most m shards, at most min(k, m) of them data, and
        // e <= max_out here
        nout = e;
    }
    if (lane == 0) {
        W.hdr[lay.nout_off] = (uint8_t)nout;
        if (a.status) a.status[b] = st;
    }
    wave_sync();
    uint8_t* rec = a.plans + (uint64_t)b * lay.stride;
    uint32_t* rec32 = reinterpret_cast<uint32_t*>(rec);
    for (uint32_t i = lane; i < hw; i += 64) rec32[i] = hdr32[i];
    if (nout == 0) return;
    const uint8_t* S = W.hdr + lay.in_off;
    const uint8_t* O = W.hdr + lay.out_off;
    for (uint32_t p = lane; p < k; p += 64) W.D[p] = (uint8_t)wide_logsum(s_log, S, k, S[p], p, a.logv);
    for (uint32_t r = lane; r < nout; r += 64) W.N[r] = (uint8_t)wide_logsum(s_log, S, k, O[r], k, a.logv);
    wave_sync();
    const uint32_t tot = nout * k;   // the record holds rows * k >= tot bytes, rounded up to 16
    uint32_t* C = reinterpret_cast<uint32_t*>(rec + lay.coef_off);
    for (uint32_t i4 = lane * 4; i4 < tot; i4 += 256) {
        uint32_t w = 0;
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) {
            const uint32_t idx = i4 + d;
            if (idx < tot) {
                const uint32_t r = fdiv(idx, a.div_k), p = idx - r * k;
                w |= (uint32_t)wide_coef(s_exp, s_log, W.N[r], W.D[p], O[r], S[p]) << (8 * d);
            }
        }
        C[i4 >> 2] = w;
    }
}

// ------------------------------------------------------------------ wide rebuild
// One lane owns one 16-byte chunk of one block. A workgroup takes a tile of g blocks x c chunks
// (g * c <= 256). Output rows go in passes of 16 accumulators; within a pass the k inputs go in
// tiles of tk, and for each (row pass, input tile) the workgroup expands the tile's coefficient
// bytes of its g blocks into PermTabs in LDS (16 rows x tk inputs x g blocks x 32 B <= 56 KiB, so
// two workgroups fit a CU's 160 KiB). Rows past a block's own erasure count carry zero tables;
// each wave folds only the rows some block of it needs (wave_rows), and a pass runs only while
// some block of the tile needs it. Every lane of the workgroup reaches every barrier.
// The one variable part is where rebuilt row r goes. SOME = false (wide reconstruct / recover; the
// outputs are erased data shards): a.out's slot r if a.out is set, else the shard's data slot.
// SOME = true (reconstruct-some, fec_some.hip; outputs are data and parity shards alike): shard o's
// own slot, in the data region below k and in the parity region from k on. A block's inputs
// (present shards) and outputs (missing ones) are disjoint slots and a lane reads and writes its own
// chunk column only, so a later row pass reads what no earlier one wrote.
template <bool SOME>
__global__ __launch_bounds__(kThreads) void rs_rebuild_wide_kernel(WideReconArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t k = a.k, G = a.g, TK = a.tk;
    const WideLayout lay = a.lay;
    gf::PermTab* tabs = reinterpret_cast<gf::PermTab*>(smem);                           // G * 16 * TK
    uint8_t* hdrs = smem + (size_t)G * kWideRowPass * TK * sizeof(gf::PermTab);         // G * coef_off
    const uint32_t tile = xcd_order();   // the grid is exactly ntiles workgroups
    if (tile >= a.ntiles) return;        // (workgroup-uniform)
    const uint32_t bt = fdiv(tile, a.div_nct), ct = tile - bt * a.nctiles;
    const uint32_t b0 = bt * G, gt = min(G, a.nblocks - b0), c0 = ct * a.c;
    {
        const uint32_t hw = lay.coef_off / 4, sw = lay.stride / 4;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.plans) + (uint64_t)b0 * sw;
        uint32_t* dst = reinterpret_cast<uint32_t*>(hdrs);
        for (uint32_t i = threadIdx.x; i < gt * hw; i += kThreads) {
            const uint32_t g = i / hw, w = i - g * hw;
            dst[i] = src[(uint64_t)g * sw + w];
        }
    }
    __syncthreads();
    uint32_t rows_max = 0;   // workgroup-uniform
    for (uint32_t g = 0; g < gt; ++g) rows_max = max(rows_max, (uint32_t)hdrs[g * lay.coef_off + lay.nout_off]);
    const uint32_t gi = fdiv(threadIdx.x, a.div_c), ci = threadIdx.x - gi * a.c;
    const uint32_t chunk = c0 + ci;
    const bool valid = gi < gt && chunk < a.cps;
    const uint8_t* H = hdrs + (valid ? gi : 0u) * lay.coef_off;
    const uint32_t nout = valid ? H[lay.nout_off] : 0u;
    const uint32_t blk = b0 + (valid ? gi : 0u);
    uint8_t* dblk = a.data + (uint64_t)blk * a.dbs + (uint64_t)chunk * kChunk;
    const uint8_t* pblk = a.parity + (uint64_t)blk * a.pbs + (uint64_t)chunk * kChunk;
    const uint8_t* pbase = parity_base(pblk, k, a.ss);
    const gf::PermTab* T = tabs + (size_t)(valid ? gi : 0u) * kWideRowPass * TK;
    for (uint32_t r0 = 0; r0 < rows_max; r0 += kWideRowPass) {
        const uint32_t rp = min(kWideRowPass, rows_max - r0);
        const uint32_t my = nout > r0 ? min(kWideRowPass, nout - r0) : 0u;
        const uint32_t rows = wave_rows<(int)kWideRowPass>(my);   // <= rp
        uint32_t acc[kWideRowPass][4];
#pragma unroll
        for (int r = 0; r < (int)kWideRowPass; ++r) acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = 0;
        for (uint32_t j0 = 0; j0 < k; j0 += TK) {
            const uint32_t tkc = min(TK, k - j0);
            __syncthreads();   // the previous tables are consumed
            {
                const uint32_t per = rp * tkc, ne = gt * per;
                for (uint32_t i = threadIdx.x; i < ne; i += kThreads) {
                    const uint32_t g = i / per, rem = i - g * per;
                    const uint32_t rr = rem / tkc, jj = rem - rr * tkc;
                    const uint32_t r = r0 + rr;
                    const uint8_t* rec = a.plans + (uint64_t)(b0 + g) * lay.stride;
                    const uint32_t c = r < hdrs[g * lay.coef_off + lay.nout_off]
                                           ? rec[lay.coef_off + r * k + j0 + jj] : 0u;
                    tabs[((size_t)g * kWideRowPass + rr) * TK + jj] = gf::make_permtab_fast(c);
                }
            }
            __syncthreads();
            if (my) {
                for (uint32_t jg = 0; jg < tkc; jg += kInGroup) {
                    // the 8 input slots of this group (the list is zero padded to 8 bytes)
                    const uint2 sl = *reinterpret_cast<const uint2*>(H + lay.in_off + j0 + jg);
                    uint4 x[kInGroup];
#pragma unroll
                    for (int jj = 0; jj < kInGroup; ++jj) {
                        const uint32_t w = jj < 4 ? sl.x : sl.y;
                        const uint32_t slot = (w >> (8 * (jj & 3))) & 0xFFu;
                        x[jj] = jg + jj < tkc   // uniform predicate: no loads past input k-1
                                    ? ld16<kNT>(slot_addr(dblk, pbase, slot, k, a.ss, a.ss))
                                    : make_uint4(0, 0, 0, 0);
                    }
                    fold_group<(int)kWideRowPass>(acc, x, rows, T, TK, jg, tkc);
                }
            }
        }
        if (my) {
            const uint32_t nb = a.len - chunk * kChunk;
            const uint8_t* O = H + lay.out_off + r0;
            uint8_t* oblk = !SOME && a.out
                                ? a.out + (uint64_t)blk * a.out_bs + (uint64_t)chunk * kChunk + (uint64_t)r0 * a.ss
                                : nullptr;
#pragma unroll
            for (int r = 0; r < (int)kWideRowPass; ++r)
                if (r < (int)my) {
                    uint8_t* dst;
                    if constexpr (SOME) {
                        const uint32_t o = O[r];   // (the parity region is the caller's to write here)
                        dst = (o < k ? dblk : const_cast<uint8_t*>(pbase)) + (uint64_t)o * a.ss;
                    } else {
                        dst = oblk ? oblk + (uint64_t)r * a.ss : dblk + (uint64_t)O[r] * a.ss;
                    }
                    store_chunk<kNT>(dst, as_uint4(acc[r]), nb);
                }
        }
    }
}

hipError_t launch_rs_plan_wide(const WidePlanArgs& a, bool some, hipStream_t s) {
    const int grid = (int)((a.nblocks + kWidePlanWaves - 1) / kWidePlanWaves);
    if (grid == 0) return hipSuccess;
    if (some) hipLaunchKernelGGL(rs_plan_wide_kernel<true>, dim3(grid), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL(rs_plan_wide_kernel<false>, dim3(grid), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_rs_rebuild_wide(const WideReconArgs& a, bool some, hipStream_t s) {
    if (a.ntiles == 0) return hipSuccess;
    const size_t lds = wide_recon_lds(a.g, a.tk, a.lay);
    if (some) hipLaunchKernelGGL(rs_rebuild_wide_kernel<true>, dim3(a.ntiles), dim3(kThreads), lds, s, a);
    else hipLaunchKernelGGL(rs_rebuild_wide_kernel<false>, dim3(a.ntiles), dim3(kThreads), lds, s, a);
    return hipGetLastError();
}

}  // namespace fk
