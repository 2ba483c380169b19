// fec_some.hip — reconstruct-some for gfx950 (klauspost Reconstruct / ReconstructSome, in place,
// k + m <= 32): every wanted missing shard of a block, data or parity, rebuilt into its own slot
// from the first k present shards. rs_plan_some_kernel turns each block's two masks into a record
// (fec_some.hpp some_plan_record); the rebuild is the wide decode's tile (fec_wide.hip
// rs_rebuild_wide_kernel: row passes of 16, so the up to 31 rows of RS(1,31) fit) with the store
// address of a row chosen between the data and the parity region by its shard index.
#include "fec_recon.hpp"
#include "fec_some.hpp"

namespace fk {

// ------------------------------------------------------------------ plan
// One lane per block, one wave per workgroup: each lane builds its record in LDS by the function
// the host self-test runs, then the wave copies the records out in 16-byte words.
constexpr int kSomePlanThreads = 64;
constexpr size_t kSomePlanTables = 768 + 256;   // exp768 | log

__global__ __launch_bounds__(kSomePlanThreads) void rs_plan_some_kernel(SomePlanArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t* s_exp = smem;
    uint8_t* s_log = smem + 768;
    uint8_t* recs = smem + kSomePlanTables;   // kSomePlanThreads * stride
    for (uint32_t i = threadIdx.x; i < 768; i += kSomePlanThreads) s_exp[i] = wide_exp768(i);
    for (uint32_t i = threadIdx.x; i < 256; i += kSomePlanThreads) s_log[i] = gf::kTables.log[i];
    __syncthreads();
    const WideLayout lay = a.lay;
    const uint32_t b0 = blockIdx.x * kSomePlanThreads;
    const uint32_t b = b0 + threadIdx.x;
    if (b < a.nblocks) {
        const uint32_t want = a.want ? a.want[b] : 0xFFFFFFFFu;
        const int32_t st = some_plan_record(recs + (size_t)threadIdx.x * lay.stride, lay, a.masks[b], want, a.k, a.n,
                                            s_exp, s_log);
        if (st) wave_flag(a.err, 1);   // too few shards, as rs_plan_kernel reports it
        if (a.status) a.status[b] = st;
    }
    __syncthreads();
    const uint32_t nrec = min((uint32_t)kSomePlanThreads, a.nblocks - b0);
    const uint32_t nw = nrec * lay.stride / 16;
    const uint4* src = reinterpret_cast<const uint4*>(recs);
    uint4* dst = reinterpret_cast<uint4*>(a.plans + (uint64_t)b0 * lay.stride);
    for (uint32_t i = threadIdx.x; i < nw; i += kSomePlanThreads) dst[i] = src[i];
}

// ------------------------------------------------------------------ rebuild
// rs_rebuild_wide_kernel's tile: one lane owns one 16-byte chunk of one block, a workgroup a tile
// of g blocks x c chunks; output rows in passes of 16 accumulators, inputs in tiles of tk, the
// tile's coefficient bytes expanded into PermTabs in LDS for each (row pass, input tile). A block's
// inputs (present shards) and outputs (missing ones) are disjoint slots and a lane reads and writes
// its own chunk column only, so a later row pass reads what no earlier one wrote.
__global__ __launch_bounds__(kThreads) void rs_rebuild_some_kernel(SomeReconArgs a) {
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
    uint8_t* pblk = a.parity + (uint64_t)blk * a.pbs + (uint64_t)chunk * kChunk;
    uint8_t* pbase = pblk - (uint64_t)k * a.ss;   // parity shard index i at pbase + i * ss
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
#pragma unroll
                    for (int jj = 0; jj < kInGroup; jj += 2) {
                        const uint32_t j = jg + jj;
                        if (j + 1 < tkc) {
                            Idx ia[4], ib[4];
                            split4(ia, x[jj]);
                            split4(ib, x[jj + 1]);
#pragma unroll
                            for (int r = 0; r < (int)kWideRowPass; ++r)
                                if (r < (int)rows) mac2(acc[r], ia, ib, T + r * TK + j, T + r * TK + j + 1);
                        } else if (j < tkc) {
                            Idx ia[4];
                            split4(ia, x[jj]);
#pragma unroll
                            for (int r = 0; r < (int)kWideRowPass; ++r)
                                if (r < (int)rows) mac1(acc[r], ia, T + r * TK + j);
                        }
                    }
                }
            }
        }
        if (my) {
            const uint32_t nb = a.len - chunk * kChunk;
            const uint8_t* O = H + lay.out_off + r0;
#pragma unroll
            for (int r = 0; r < (int)kWideRowPass; ++r)
                if (r < (int)my) {
                    // the one change against the data-only rebuilds: shard o lives in the data region
                    // below k, in the parity region from k on
                    const uint32_t o = O[r];
                    store_chunk<kNT>((o < k ? dblk : pbase) + (uint64_t)o * a.ss, as_uint4(acc[r]), nb);
                }
        }
    }
}

hipError_t launch_rs_plan_some(const SomePlanArgs& a, hipStream_t s) {
    const int grid = (int)((a.nblocks + kSomePlanThreads - 1) / kSomePlanThreads);
    if (grid == 0) return hipSuccess;
    const size_t lds = kSomePlanTables + (size_t)kSomePlanThreads * a.lay.stride;
    hipLaunchKernelGGL(rs_plan_some_kernel, dim3(grid), dim3(kSomePlanThreads), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_rs_rebuild_some(const SomeReconArgs& a, hipStream_t s) {
    if (a.ntiles == 0) return hipSuccess;
    const size_t lds = wide_recon_lds(a.g, a.tk, a.lay);
    hipLaunchKernelGGL(rs_rebuild_some_kernel, dim3(a.ntiles), dim3(kThreads), lds, s, a);
    return hipGetLastError();
}

}  // namespace fk
