// fec_locate.hip — locate the corrupt shard of a block that fails verify, for gfx950
// (fec_rs_locate_batch). The verify kernel's body (fec_verify.hip): the accumulators start from the
// stored parity and the data chunks fold through the code's PermTabs, so they end as the syndromes.
// A lane whose syndromes are zero is done, as in verify; a lane that holds an anomaly classifies its
// chunk (fec_locate.hpp locate_chunk) and the block's verdict word collects the proposals.
#include "fec_flat.hpp"
#include "fec_locate.hpp"

namespace fk {

// One lane = one 16-byte column chunk of one block; accumulator 0 is parity row 0, accumulator i the
// row r0 + i - 1. Every pass compares its rows with the same S_0 (two passes can each agree with a
// data column on their own and still disagree on the error bytes), so row 0 rides along in each.
//
// The verdicts are kLocateClean on entry to pass 0. A wave's lanes may cover several blocks and a
// block may span waves and workgroups: the proposals of a wave's lanes are merged per block first
// (one shard if they all name it, else unknown), then the first lane of each block merges the result
// into the block's word by compare-and-swap (locate_merge). A clean batch issues no atomics and
// takes the branch below in no wave.
template <int ROWS, bool LDS_TABS>
__global__ __launch_bounds__(kThreads) void rs_locate_kernel(LocateArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t k = a.k, rows = a.rows;
    const gf::PermTab* tabs = stage_tabs<LDS_TABS>(a.tabs0, k * 8, smem);
    if constexpr (LDS_TABS) {
        stage_tabs<true>(a.tabs, (rows - 1) * k * 8, smem + (size_t)k * sizeof(gf::PermTab));
        __syncthreads();
    }
    const FlatItem f = flat_item(a.total, a.cps, a.div_cps);
    const uint32_t b = f.b, c = f.c;
    const uint8_t* src = a.in + (uint64_t)b * a.in_bs + (uint64_t)c * kChunk;
    const uint64_t poff = (uint64_t)b * a.par_bs + (uint64_t)c * kChunk;
    uint32_t acc[ROWS][4];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const uint8_t* par = a.par + poff + (uint64_t)locate_row((uint32_t)r, a.r0) * a.ss;
        const uint4 p = r < (int)rows ? ld16<true>(par) : make_uint4(0, 0, 0, 0);
        acc[r][0] = p.x, acc[r][1] = p.y, acc[r][2] = p.z, acc[r][3] = p.w;
    }
    for (uint32_t j0 = 0; j0 < k; j0 += kInGroup) {
        uint4 x[kInGroup];
        load_shards(x, src, a.ss, j0, k);
        fold_group<ROWS>(acc, x, rows, tabs, k, j0, k);
    }
    uint4 d = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
        if (r < (int)rows) d.x |= acc[r][0], d.y |= acc[r][1], d.z |= acc[r][2], d.w |= acc[r][3];
    const uint32_t nb = a.len - c * kChunk;
    d = keep_bytes(d, nb);
    const bool bad = f.live && (d.x | d.y | d.z | d.w) != 0;
    uint64_t todo = __ballot(bad);   // wave-uniform
    if (todo == 0) return;
    int32_t prop = kLocateClean;
    if (bad) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const uint4 s = keep_bytes(as_uint4(acc[r]), nb);
            acc[r][0] = s.x, acc[r][1] = s.y, acc[r][2] = s.z, acc[r][3] = s.w;
        }
        // a later pass checks the column the earlier passes left in the block's word
        const int32_t seen =
            a.r0 == 1 ? kLocateClean : __hip_atomic_load(a.verdict + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        prop = locate_chunk<ROWS>(acc, rows, a.r0, k, a.m, tabs, a.loctab, seen);
    }
    const uint32_t lane = threadIdx.x & 63u;
    while (todo) {
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
        const uint32_t lb = (uint32_t)__shfl((int)b, (int)leader);
        const int32_t lp = __shfl(prop, (int)leader);
        const bool mine = bad && b == lb;
        todo &= ~__ballot(mine);
        const bool split = __ballot(mine && prop != lp) != 0;
        if (lane == leader) {
            const int32_t v = split ? kLocateUnknown : lp;
            int32_t cur = kLocateClean;   // the likely word: one compare-and-swap settles it
            for (;;) {
                const int32_t next = locate_merge(cur, v);
                if (next == cur) break;
                const int32_t old = atomicCAS(a.verdict + b, cur, next);
                if (old == cur) break;
                cur = old;
            }
        }
    }
}

// One lane = one block: its present mask and its part in the two counts, one atomic per wave and
// count, and none for a wave that has nothing to count.
__global__ __launch_bounds__(kThreads) void rs_locate_finalize_kernel(LocateFinArgs a) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const bool live = i < a.nblocks;
    const int32_t v = live ? a.verdict[i] : kLocateClean;
    if (a.present && live)
        for (uint32_t w = 0; w < a.mask_words; ++w) {
            uint32_t bits = 32u * w < a.n ? low_mask(a.n - 32u * w) : 0u;
            if (v >= 0 && (uint32_t)v / 32u == w) bits &= ~(1u << ((uint32_t)v & 31u));
            a.present[(uint64_t)i * a.mask_words + w] = bits;
        }
    if (a.counts) {
        const uint64_t located = __ballot(v >= 0), unknown = __ballot(v == kLocateUnknown);
        if ((threadIdx.x & 63u) == 0) {
            if (located) atomicAdd(a.counts, (uint32_t)__popcll(located));
            if (unknown) atomicAdd(a.counts + 1, (uint32_t)__popcll(unknown));
        }
    }
}

template <int ROWS>
static hipError_t locate_dispatch(const LocateArgs& a, int grid, hipStream_t s) {
    if (locate_lds_tabs(a.k, a.rows)) {
        const size_t lds = (size_t)a.rows * a.k * sizeof(gf::PermTab);
        hipLaunchKernelGGL((rs_locate_kernel<ROWS, true>), dim3(grid), dim3(kThreads), lds, s, a);
    } else {
        hipLaunchKernelGGL((rs_locate_kernel<ROWS, false>), dim3(grid), dim3(kThreads), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_rs_locate(const LocateArgs& a, int grid, hipStream_t s) {
    if (a.total == 0 || a.rows == 0) return hipSuccess;
    if (a.rows <= 2) return locate_dispatch<2>(a, grid, s);
    if (a.rows <= 4) return locate_dispatch<4>(a, grid, s);
    if (a.rows <= 8) return locate_dispatch<8>(a, grid, s);
    return locate_dispatch<kLocateRows>(a, grid, s);   // the caller splits longer codes
}

hipError_t launch_rs_locate_finalize(const LocateFinArgs& a, hipStream_t s) {
    if (a.nblocks == 0 || (!a.present && !a.counts)) return hipSuccess;
    const uint32_t grid = (a.nblocks + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(rs_locate_finalize_kernel, dim3(grid), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace fk
