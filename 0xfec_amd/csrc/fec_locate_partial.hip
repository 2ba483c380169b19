// fec_locate_partial.hip — locate corrupt shards in blocks that also have missing shards, for gfx950
// (fec_rs_locate_partial_batch), in four launches: the plan (one word and, for a block with missing
// shards, m scaling PermTabs per block), then locate-multi's scan, solve and finalize
// (fec_locate_multi.hip) under the blocks' masks. The scan is the hot path. fec_locate_partial.hpp has
// the arithmetic.
#include "fec_flat.hpp"
#include "fec_locate_partial.hpp"

namespace fk {

// max(m, 1) lanes per block: lane i writes the PermTab of lambda(k + i) if the block has missing shards
// and enough present ones, lane 0 the block's plan word. A block with a full mask gets its word alone.
__global__ __launch_bounds__(kThreads) void rs_locate_partial_plan_kernel(LocatePartialPlanArgs a) {
    const uint32_t per = max(a.m, 1u);
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t b = t / per, i = t - b * per;
    if (b >= a.nblocks) return;
    const uint32_t* mask = a.masks + (uint64_t)b * a.mask_words;
    const uint32_t plan = locate_partial_plan(mask, a.k, a.m, a.max_bad);
    if (i == 0) a.plan[b] = plan;
    if (partial_missing(plan) == 0 || (plan & kPartialTooFew)) return;   // (m >= 1 here)
    reinterpret_cast<gf::PermTab*>(a.ltabs)[(uint64_t)b * a.m + i] =
        gf::make_permtab_fast(locate_partial_scale(mask, a.k, a.k + a.m, i));
}

// What a lane knows of its block before it loads a shard: the plan word, the parity shards' mask bits
// (bit r: parity shard r) and where the data shards' bits are read from. A block of too few shards
// has every bit clear: its lane loads from `zeros` alone and flags nothing.
struct PartialLane {
    uint32_t plan, pbits;
    const uint32_t* mask;
    bool few;
};
__device__ __forceinline__ PartialLane partial_lane(const LocatePartialScanArgs& a, uint32_t b) {
    PartialLane p;
    p.plan = a.plan[b];
    p.few = (p.plan & kPartialTooFew) != 0;
    p.mask = a.masks + (uint64_t)b * a.mask_words;
    p.pbits = 0;
    if (a.m != 0 && !p.few) {   // bits k .. k + m - 1 lie in one word or in two neighbours
        const uint64_t two = ((uint64_t)p.mask[(a.k + a.m - 1) >> 5] << 32) | p.mask[a.k >> 5];
        p.pbits = (uint32_t)(two >> (a.k & 31u));
    }
    return p;
}

// load_shards (fec_device.hpp) under the block's mask: `bits` holds the mask bits of shards j0 ..
// j0 + 7 in its low byte. The eight loads go out back to back whatever the mask says.
__device__ __forceinline__ void partial_load_shards(uint4 (&x)[kInGroup], const uint8_t* src, const uint8_t* zeros,
                                                    uint64_t ss, uint32_t j0, uint32_t k, uint32_t bits) {
#pragma unroll
    for (int jj = 0; jj < kInGroup; ++jj)
        x[jj] = j0 + jj < k ? ld16<true>((bits >> jj) & 1u ? src + (uint64_t)(j0 + jj) * ss : zeros)
                            : make_uint4(0, 0, 0, 0);
}

// rs_locate_multi_scan_kernel under the masks. A wave whose lanes all belong to complete blocks tests
// its syndromes as that kernel does. Otherwise the lanes of blocks with missing shards scale their
// rows and form the m - e sums W' one at a time, keeping only their OR; rows past a lane's m - e are
// formed with the wave and dropped by the lane.
template <int ROWS, bool LDS_TABS>
__global__ __launch_bounds__(kThreads) void rs_locate_partial_scan_kernel(LocatePartialScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const gf::PermTab* tabs = stage_tabs<LDS_TABS>(a.tabs, a.m * a.k * 8, smem);
    if constexpr (LDS_TABS) __syncthreads();
    const uint32_t k = a.k, m = a.m;
    const FlatItem f = flat_item(a.total, a.cps, a.div_cps);
    const uint32_t b = f.b, c = f.c;
    const PartialLane p = partial_lane(a, b);
    const uint8_t* src = a.in + (uint64_t)b * a.in_bs + (uint64_t)c * kChunk;
    const uint8_t* par = a.par + (uint64_t)b * a.par_bs + (uint64_t)c * kChunk;
    uint32_t acc[ROWS][4];
    // the stored parity of the present parity shards, zeros for the missing ones: a missing shard's load
    // goes to `zeros` (address select, no branch). (In the kernel's body: as a helper that takes acc by
    // reference, the 16-row instance holds 312 VGPRs, one wave per SIMD; here 213.)
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const uint4 v = r < (int)m ? ld16<true>((p.pbits >> r) & 1u ? par + (uint64_t)r * a.ss : a.zeros)
                                   : make_uint4(0, 0, 0, 0);
        acc[r][0] = v.x, acc[r][1] = v.y, acc[r][2] = v.z, acc[r][3] = v.w;
    }
    uint32_t mw = 0;
    for (uint32_t j0 = 0; j0 < k; j0 += kInGroup) {
        if ((j0 & 31u) == 0) mw = p.few ? 0u : p.mask[j0 >> 5];   // a group of 8 lies in one word
        uint4 x[kInGroup];
        partial_load_shards(x, src, a.zeros, a.ss, j0, k, mw >> (j0 & 31u));
        fold_group<ROWS>(acc, x, m, tabs, k, j0, k);
    }
    uint4 d = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
        if (r < (int)m) d.x |= acc[r][0], d.y |= acc[r][1], d.z |= acc[r][2], d.w |= acc[r][3];
    const bool part = partial_missing(p.plan) != 0 && !p.few;
    if (__ballot(part) != 0) {   // wave-uniform
        const uint32_t sums = part ? m - partial_missing(p.plan) : 0u;
        if (part) locate_partial_scale_rows<ROWS>(acc, m, reinterpret_cast<const gf::PermTab*>(a.ltabs) + (uint64_t)b * m);
        const gf::PermTab* A = reinterpret_cast<const gf::PermTab*>(a.atabs);   // uniform addresses
        uint4 dp = make_uint4(0, 0, 0, 0);
        // (a loop over the sums, not unrolled: l indexes the table alone, and one sum is live at a time)
#pragma unroll 1
        for (uint32_t l = 0; l < m && __ballot(l < sums) != 0; ++l) {
            uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
            for (int i = 0; i < ROWS; ++i)
                if (i < (int)m) {
                    const gf::PermTab t = A[l * m + (uint32_t)i];
                    w0 ^= locate_mul4(t, acc[i][0]), w1 ^= locate_mul4(t, acc[i][1]);
                    w2 ^= locate_mul4(t, acc[i][2]), w3 ^= locate_mul4(t, acc[i][3]);
                }
            if (l < sums) dp.x |= w0, dp.y |= w1, dp.z |= w2, dp.w |= w3;
        }
        if (part) d = dp;
    }
    d = keep_bytes(d, a.len - c * kChunk);
    const uint64_t flagged = __ballot(f.live && !p.few && (d.x | d.y | d.z | d.w) != 0);   // wave-uniform
    if (flagged != 0 && (threadIdx.x & 63u) == 0) a.bitmap[f.item >> 6] = flagged;
}

// rs_locate_multi_solve_kernel with each lane's own block plan: the syndromes again under the mask,
// scaled where the block has missing shards, then m - e sums solved to the block's radius with roots
// at present shards only (that kernel's solver, MASKED). The text around the lane's work repeats that
// kernel's: every shared form of it changed that kernel's machine code (Locate-partial).
template <bool LDS_TABS>
__global__ __launch_bounds__(kThreads) void rs_locate_partial_solve_kernel(LocatePartialSolveArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t w = blockIdx.x * kThreads + threadIdx.x;
    const uint64_t word = w < a.nwords ? a.s.bitmap[w] : 0;
    if (!__syncthreads_or(word != 0)) return;
    const uint32_t m = a.s.m;
    typedef __attribute__((address_space(3))) const uint8_t LdsByte;
    stage_tabs<true>(reinterpret_cast<const uint32_t*>(a.ft), sizeof(gf::Tables) / 4, smem);
    LdsByte* ft = (LdsByte*)smem;
    const gf::PermTab* atabs = stage_tabs<true>(a.s.atabs, m * m * 8, smem + sizeof(gf::Tables));
    const gf::PermTab* tabs =
        stage_tabs<LDS_TABS>(a.s.tabs, m * a.s.k * 8, smem + sizeof(gf::Tables) + (size_t)m * m * sizeof(gf::PermTab));
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stride = a.words + 1;
    uint64_t have = __ballot(word != 0);   // wave-uniform
    while (have) {
        const uint32_t src = (uint32_t)__ffsll((unsigned long long)have) - 1u;
        have &= have - 1;
        const uint64_t bits = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(word >> 32), (int)src) << 32) |
                              (uint32_t)__shfl((int)(uint32_t)word, (int)src);
        const bool mine = (bits >> lane) & 1u;   // the scan flags live items of blocks with >= k shards only
        uint32_t sup[kLocateMultiWords] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t b = 0;
        bool unknown = false;
        if (mine) {
            const uint32_t k = a.s.k;
            const uint32_t it = ((w - lane + src) << 6) + lane;
            b = fdiv(it, a.s.div_cps);
            const uint32_t c = it - b * a.s.cps;
            const PartialLane p = partial_lane(a.s, b);
            const uint8_t* in = a.s.in + (uint64_t)b * a.s.in_bs + (uint64_t)c * kChunk;
            const uint8_t* par = a.s.par + (uint64_t)b * a.s.par_bs + (uint64_t)c * kChunk;
            uint32_t acc[kLocateMultiRows][4];
#pragma unroll
            for (int r = 0; r < kLocateMultiRows; ++r) {
                const uint4 v = r < (int)m ? ld16<true>((p.pbits >> r) & 1u ? par + (uint64_t)r * a.s.ss : a.s.zeros)
                                           : make_uint4(0, 0, 0, 0);
                acc[r][0] = v.x, acc[r][1] = v.y, acc[r][2] = v.z, acc[r][3] = v.w;
            }
            uint32_t mw = 0;
            for (uint32_t j0 = 0; j0 < k; j0 += kInGroup) {
                if ((j0 & 31u) == 0) mw = p.mask[j0 >> 5];
                uint4 x[kInGroup];
                partial_load_shards(x, in, a.s.zeros, a.s.ss, j0, k, mw >> (j0 & 31u));
                fold_group<kLocateMultiRows>(acc, x, m, tabs, k, j0, k);
            }
            const uint32_t nb = a.s.len - c * kChunk;
#pragma unroll
            for (int r = 0; r < kLocateMultiRows; ++r) {
                const uint4 s = keep_bytes(as_uint4(acc[r]), nb);
                acc[r][0] = s.x, acc[r][1] = s.y, acc[r][2] = s.z, acc[r][3] = s.w;
            }
            if (partial_missing(p.plan) != 0)
                locate_partial_scale_rows<kLocateMultiRows>(acc, m, reinterpret_cast<const gf::PermTab*>(a.s.ltabs) + (uint64_t)b * m);
            unknown = locate_multi_chunk<kLocateMultiRows, true>(acc, m, a.n, partial_radius(p.plan), atabs, ft, sup,
                                                                 m - partial_missing(p.plan), p.mask);
        }
        uint64_t todo = bits;
        while (todo) {
            const uint32_t leader = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
            const uint32_t lb = (uint32_t)__shfl((int)b, (int)leader);
            const bool same = mine && b == lb;
            todo &= ~__ballot(same);
            const bool unk = __ballot(same && unknown) != 0;
            uint32_t* dst = a.blk + (uint64_t)lb * stride;
#pragma unroll
            for (uint32_t i = 0; i < kLocateMultiWords; ++i)
                if (i < a.words) {
                    uint32_t v = same ? sup[i] : 0u;
#pragma unroll
                    for (int off = 32; off; off >>= 1) v |= (uint32_t)__shfl_xor((int)v, off);
                    if (lane == leader && v) atomicOr(dst + i, v);
                }
            if (lane == leader && unk) atomicOr(dst + a.words, 1u);
        }
    }
}

// One lane = one block: its result (too few first), its present mask (the block's own present bits
// below n, read before they are written, less the located set) and its part in the three counts, one
// atomic per wave and count.
__global__ __launch_bounds__(kThreads) void rs_locate_partial_finalize_kernel(LocatePartialFinArgs a) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const bool live = i < a.nblocks;
    uint32_t bad[kLocateMultiWords] = {0, 0, 0, 0, 0, 0, 0, 0};
    int32_t v = 0;
    if (live) {
        const uint32_t* src = a.blk + (uint64_t)i * (a.words + 1);
#pragma unroll
        for (uint32_t w = 0; w < kLocateMultiWords; ++w)
            if (w < a.words) bad[w] = src[w];
        v = locate_partial_count(a.plan[i], bad, kLocateMultiWords, src[a.words] != 0);
        a.bad_count[i] = v;
        if (a.present) {
            uint32_t has[kLocateMultiWords];
#pragma unroll
            for (uint32_t w = 0; w < kLocateMultiWords; ++w)
                has[w] = w < a.mask_words && 32u * w < a.n ? a.masks[(uint64_t)i * a.mask_words + w] & low_mask(a.n - 32u * w)
                                                          : 0u;
#pragma unroll
            for (uint32_t w = 0; w < kLocateMultiWords; ++w)
                if (w < a.mask_words) a.present[(uint64_t)i * a.mask_words + w] = v > 0 ? has[w] & ~bad[w] : has[w];
        }
    }
    if (a.counts) {
        const uint64_t located = __ballot(v > 0), unknown = __ballot(v == kLocateUnknown),
                       few = __ballot(v == kLocateTooFew);
        if ((threadIdx.x & 63u) == 0) {
            if (located) atomicAdd(a.counts, (uint32_t)__popcll(located));
            if (unknown) atomicAdd(a.counts + 1, (uint32_t)__popcll(unknown));
            if (few) atomicAdd(a.counts + 2, (uint32_t)__popcll(few));
        }
    }
}

hipError_t launch_rs_locate_partial_plan(const LocatePartialPlanArgs& a, hipStream_t s) {
    if (a.nblocks == 0) return hipSuccess;
    // (a slice's workspace holds m PermTabs per block: nblocks * m stays far below 2^32)
    const uint32_t grid = (a.nblocks * std::max(a.m, 1u) + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(rs_locate_partial_plan_kernel, dim3(grid), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

template <int ROWS>
static hipError_t locate_partial_scan_dispatch(const LocatePartialScanArgs& a, int grid, hipStream_t s) {
    if (locate_lds_tabs(a.k, a.m)) {
        const size_t lds = (size_t)a.m * a.k * sizeof(gf::PermTab);
        hipLaunchKernelGGL((rs_locate_partial_scan_kernel<ROWS, true>), dim3(grid), dim3(kThreads), lds, s, a);
    } else {
        hipLaunchKernelGGL((rs_locate_partial_scan_kernel<ROWS, false>), dim3(grid), dim3(kThreads), 0, s, a);
    }
    return hipGetLastError();
}

// The instances of rs_locate_multi_scan_kernel: 2, 4, 8 and 16 rows.
hipError_t launch_rs_locate_partial_scan(const LocatePartialScanArgs& a, int grid, hipStream_t s) {
    if (a.total == 0 || a.m == 0) return hipSuccess;
    if (a.m <= 2) return locate_partial_scan_dispatch<2>(a, grid, s);
    if (a.m <= 4) return locate_partial_scan_dispatch<4>(a, grid, s);
    if (a.m <= 8) return locate_partial_scan_dispatch<8>(a, grid, s);
    return locate_partial_scan_dispatch<kLocateMultiRows>(a, grid, s);
}

hipError_t launch_rs_locate_partial_solve(const LocatePartialSolveArgs& a, hipStream_t s) {
    if (a.nwords == 0 || a.s.m == 0) return hipSuccess;
    const uint32_t grid = (a.nwords + kThreads - 1) / kThreads;
    const LocateSolveLds lds = locate_solve_lds(a.s.k, a.s.m);
    if (lds.tabs)
        hipLaunchKernelGGL(rs_locate_partial_solve_kernel<true>, dim3(grid), dim3(kThreads), lds.bytes, s, a);
    else
        hipLaunchKernelGGL(rs_locate_partial_solve_kernel<false>, dim3(grid), dim3(kThreads), lds.bytes, s, a);
    return hipGetLastError();
}

hipError_t launch_rs_locate_partial_finalize(const LocatePartialFinArgs& a, hipStream_t s) {
    if (a.nblocks == 0) return hipSuccess;
    const uint32_t grid = (a.nblocks + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(rs_locate_partial_finalize_kernel, dim3(grid), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace fk
