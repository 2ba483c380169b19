// fec_plan_sort.hpp — what the sorted plan kernels share (fec_plan.hip: the Lagrange plans of the
// built-in matrices; fec_plan_solve.hip: the elimination plan of a custom matrix): the LDS layout of a
// plan workgroup, the sort window, and the step that stores a window's records in erasure-count order.
#pragma once

#include "fec_recon.hpp"

namespace fk {

constexpr uint32_t kPlanSortThreads = 256;
constexpr uint32_t kGroupScratch = 160;   // per block: S[32] slots, O[32] erased, X[32] others, D|N[64]

struct SortLds {
    size_t prows, dall, scratch, pos, rank, recs, total;
};
// Plan form 2 stages exp over [0, 768) (exp[i mod 255], so a sum of three logs needs no reduction),
// log over [768, 1024), then log of 0..31 in 4 copies (log 0 taken as 0): lane l reads copy l & 3,
// so the 32 lanes of a half-wave that look up log(i ^ j) for shard indices i, j < 32 never meet on
// a bank (32 banks of 4 bytes per half-wave).
constexpr uint32_t kV2Exp = 0, kV2Log = 768, kV2Log32 = 1024, kV2Tables = 1152;
constexpr uint32_t kRankBins = 33;   // erasure counts 0..32
// recs: the records of `win` segments of `groups` blocks, sorted together (sort window)
__host__ __device__ inline SortLds sort_lds(uint32_t m, uint32_t k, uint32_t groups, uint32_t stride,
                                            uint32_t win, uint32_t gscratch = kGroupScratch) {
    SortLds l;
    l.prows = kV2Tables;
    l.dall = l.prows + (size_t)m * k;
    l.scratch = (l.dall + 32 + 15) & ~(size_t)15;
    l.pos = l.scratch + (size_t)groups * gscratch;
    // ranking scratch: per wave of records and bin, a count (then its prefix), and per bin a start
    l.rank = l.pos + (size_t)groups * win * 4;
    l.recs = (l.rank + ((size_t)(groups * win + 63) / 64 + 1) * kRankBins * 4 + 15) & ~(size_t)15;
    l.total = l.recs + (size_t)groups * win * stride;
    return l;
}

// Segments sorted together: as many as make 64 blocks. A rebuild wave spans two neighbouring
// records, and its row count is the larger of their two erasure counts; sorted over one segment
// (16 blocks for RS(16,24), 8 for RS(20,30)) neighbours still differ by about one row. 64 blocks
// against 128 / 256 / 512 (r03y, r04s): the window's records in LDS cost the plan kernel
// residency that the rebuild does not win back.
__host__ __device__ inline uint32_t sort_window(uint32_t groups) { return groups < 64u ? 64u / groups : 1u; }

// The window's nw record slots (first block base0) from LDS to their storage order in a.plans:
// erasure count descending, then block order (stable). Workgroup-wide (barriers inside).
__device__ __forceinline__ void sort_window_out(const PlanArgs& a, uint8_t* smem, const SortLds& L, uint32_t nw,
                                                uint32_t base0) {
    const PlanLayout lay = a.lay;
    uint32_t* s_pos = reinterpret_cast<uint32_t*>(smem + L.pos);
    __syncthreads();   // every record of the window written
    const uint32_t nvalid = min(nw, a.nblocks - base0);
    // counting sort: position = records with a larger count + earlier records with the same
    // count (past-the-batch groups: nothing to rebuild, last indices, so they rank last).
    // Per wave of records and bin, a ballot gives the count and each record's rank in its wave.
    const uint32_t U = a.maxe + 1, nwv = (nw + 63) / 64;
    uint32_t* wc = reinterpret_cast<uint32_t*>(smem + L.rank);   // [nwv][U], then start[U]
    uint32_t* start = wc + nwv * U;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (uint32_t t = threadIdx.x; t < nwv * 64; t += kPlanSortThreads) {   // wave-uniform bound
        const uint32_t v = t < nw ? smem[L.recs + (size_t)t * lay.stride + lay.nout_off] : kRankBins;
        uint32_t rin = 0;
        for (uint32_t u = 0; u < U; ++u) {
            const uint64_t bm = __ballot(v == u);
            if (v == u) rin = (uint32_t)__popcll(bm & lt);
            if (lane == 0) wc[(t >> 6) * U + u] = (uint32_t)__popcll(bm);
        }
        if (t < nw) s_pos[t] = rin;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // bins in descending order; within a bin, waves in order: wc becomes each wave's offset
        uint32_t acc = 0;
        for (uint32_t u = U; u-- > 0;) {
            start[u] = acc;
            for (uint32_t w = 0; w < nwv; ++w) {
                const uint32_t c = wc[w * U + u];
                wc[w * U + u] = acc;
                acc += c;
            }
        }
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < nw; t += kPlanSortThreads) {
        const uint32_t v = smem[L.recs + (size_t)t * lay.stride + lay.nout_off];
        s_pos[t] += wc[(t >> 6) * U + v];
    }
    __syncthreads();
    const uint32_t per = lay.stride / 16;
    const uint4* src = reinterpret_cast<const uint4*>(smem + L.recs);
    uint4* dst = reinterpret_cast<uint4*>(a.plans + (uint64_t)base0 * lay.stride);
    for (uint32_t i = threadIdx.x; i < nvalid * per; i += kPlanSortThreads) {
        const uint32_t r = i / per, q = i - r * per;
        dst[(size_t)s_pos[r] * per + q] = src[(size_t)r * per + q];
    }
}

// The routed in-place form's word (fec_recover.hip): zero, no block needs a plan (workgroup-uniform).
__device__ __forceinline__ bool route_skips(const PlanArgs& a) {
    typedef __attribute__((address_space(4))) const uint32_t ConstU32;
    return a.route && *(ConstU32*)a.route == 0;
}

}  // namespace fk
