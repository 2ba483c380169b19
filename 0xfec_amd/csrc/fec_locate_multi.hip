// fec_locate_multi.hip — locate up to m/2 corrupt shards of a block, for gfx950
// (fec_rs_locate_multi_batch), in three launches. The scan is the hot path: verify's body
// (fec_verify.hip) that ends in one bitmap word per wave, written only where a lane holds a nonzero
// syndrome. The solve walks the bitmap and works on the flagged chunks alone (fec_locate_multi.hpp
// locate_multi_chunk); the finalize turns each block's merged words into its outputs.
#include "fec_flat.hpp"
#include "fec_locate_multi.hpp"

namespace fk {

// One lane = one 16-byte column chunk of one block, as in rs_verify_kernel. A wave's index in the
// launch's item order is its bitmap word's index, so no two waves share a word and a plain store
// serves; a wave without an anomaly writes nothing.
template <int ROWS, bool LDS_TABS>
__global__ __launch_bounds__(kThreads) void rs_locate_multi_scan_kernel(LocateMultiScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const gf::PermTab* tabs = stage_tabs<LDS_TABS>(a.tabs, a.m * a.k * 8, smem);
    if constexpr (LDS_TABS) __syncthreads();
    const uint32_t k = a.k, m = a.m;
    const FlatItem f = flat_item(a.total, a.cps, a.div_cps);
    const uint32_t b = f.b, c = f.c;
    const uint8_t* src = a.in + (uint64_t)b * a.in_bs + (uint64_t)c * kChunk;
    const uint8_t* par = a.par + (uint64_t)b * a.par_bs + (uint64_t)c * kChunk;
    uint32_t acc[ROWS][4];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const uint4 p = r < (int)m ? ld16<true>(par + (uint64_t)r * a.ss) : make_uint4(0, 0, 0, 0);
        acc[r][0] = p.x, acc[r][1] = p.y, acc[r][2] = p.z, acc[r][3] = p.w;
    }
    // (the loop stands in the kernel's own body: fec_device.hpp load_shards)
    for (uint32_t j0 = 0; j0 < k; j0 += kInGroup) {
        uint4 x[kInGroup];
        load_shards(x, src, a.ss, j0, k);
        fold_group<ROWS>(acc, x, m, tabs, k, j0, k);
    }
    uint4 d = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
        if (r < (int)m) d.x |= acc[r][0], d.y |= acc[r][1], d.z |= acc[r][2], d.w |= acc[r][3];
    d = keep_bytes(d, a.len - c * kChunk);
    const uint64_t flagged = __ballot(f.live && (d.x | d.y | d.z | d.w) != 0);   // wave-uniform
    if (flagged != 0 && (threadIdx.x & 63u) == 0) a.bitmap[f.item >> 6] = flagged;
}

// One lane reads one bitmap word; a workgroup whose 256 words are zero ends there. The waves then
// take their nonzero words one at a time: lane l of the wave works on item 64 * word + l if the word
// has bit l, so the lanes of a wave solve the chunks that one scan wave flagged. Their supports are
// merged per block within the wave first, then one lane per block ORs them into the block's words.
// A lane's solve is one long chain of dependent table reads, so a workgroup that has work stages
// what it reads into LDS first: the field's tables, the coefficient PermTabs, and the code's PermTabs
// where they fit beside those (LDS_TABS).
template <bool LDS_TABS>
__global__ __launch_bounds__(kThreads) void rs_locate_multi_solve_kernel(LocateMultiSolveArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t w = blockIdx.x * kThreads + threadIdx.x;
    const uint64_t word = w < a.nwords ? a.s.bitmap[w] : 0;
    if (!__syncthreads_or(word != 0)) return;
    const uint32_t m = a.s.m;
    // (read through an LDS-typed pointer: the solver's byte lookups are then ds_read_u8 with no test of
    // which memory a generic pointer names)
    typedef __attribute__((address_space(3))) const uint8_t LdsByte;
    stage_tabs<true>(reinterpret_cast<const uint32_t*>(a.ft), sizeof(gf::Tables) / 4, smem);
    LdsByte* ft = (LdsByte*)smem;
    const gf::PermTab* atabs = stage_tabs<true>(a.atabs, m * m * 8, smem + sizeof(gf::Tables));
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
        const bool mine = (bits >> lane) & 1u;   // the scan flags live items only
        uint32_t sup[kLocateMultiWords] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t b = 0;
        bool unknown = false;
        if (mine) {
            // the scan's syndromes again, every row in place whatever m is
            const uint32_t k = a.s.k;
            const uint32_t it = ((w - lane + src) << 6) + lane;
            b = fdiv(it, a.s.div_cps);
            const uint32_t c = it - b * a.s.cps;
            const uint8_t* in = a.s.in + (uint64_t)b * a.s.in_bs + (uint64_t)c * kChunk;
            const uint8_t* par = a.s.par + (uint64_t)b * a.s.par_bs + (uint64_t)c * kChunk;
            uint32_t acc[kLocateMultiRows][4];
#pragma unroll
            for (int r = 0; r < kLocateMultiRows; ++r) {
                const uint4 p = r < (int)m ? ld16<true>(par + (uint64_t)r * a.s.ss) : make_uint4(0, 0, 0, 0);
                acc[r][0] = p.x, acc[r][1] = p.y, acc[r][2] = p.z, acc[r][3] = p.w;
            }
            for (uint32_t j0 = 0; j0 < k; j0 += kInGroup) {
                uint4 x[kInGroup];
                load_shards(x, in, a.s.ss, j0, k);
                fold_group<kLocateMultiRows>(acc, x, m, tabs, k, j0, k);
            }
            const uint32_t nb = a.s.len - c * kChunk;
#pragma unroll
            for (int r = 0; r < kLocateMultiRows; ++r) {
                const uint4 s = keep_bytes(as_uint4(acc[r]), nb);
                acc[r][0] = s.x, acc[r][1] = s.y, acc[r][2] = s.z, acc[r][3] = s.w;
            }
            unknown = locate_multi_chunk<kLocateMultiRows>(acc, m, a.n, a.T, atabs, ft, sup);
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

// One lane = one block: its count, its present mask and its part in the two counts, one atomic per
// wave and count, and none for a wave that has nothing to count.
__global__ __launch_bounds__(kThreads) void rs_locate_multi_finalize_kernel(LocateMultiFinArgs a) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const bool live = i < a.nblocks;
    uint32_t bad[kLocateMultiWords] = {0, 0, 0, 0, 0, 0, 0, 0};
    int32_t v = 0;
    if (live) {
        const uint32_t* src = a.blk + (uint64_t)i * (a.words + 1);
#pragma unroll
        for (uint32_t w = 0; w < kLocateMultiWords; ++w)
            if (w < a.words) bad[w] = src[w];
        v = locate_multi_count(bad, kLocateMultiWords, src[a.words] != 0, a.T);
        a.bad_count[i] = v;
        if (a.present) {
#pragma unroll
            for (uint32_t w = 0; w < kLocateMultiWords; ++w)
                if (w < a.mask_words) {
                    const uint32_t bits = 32u * w < a.n ? low_mask(a.n - 32u * w) : 0u;
                    a.present[(uint64_t)i * a.mask_words + w] = v > 0 ? bits & ~bad[w] : bits;
                }
        }
    }
    if (a.counts) {
        const uint64_t located = __ballot(v > 0), unknown = __ballot(v == kLocateUnknown);
        if ((threadIdx.x & 63u) == 0) {
            if (located) atomicAdd(a.counts, (uint32_t)__popcll(located));
            if (unknown) atomicAdd(a.counts + 1, (uint32_t)__popcll(unknown));
        }
    }
}

template <int ROWS>
static hipError_t locate_multi_scan_dispatch(const LocateMultiScanArgs& a, int grid, hipStream_t s) {
    if (locate_lds_tabs(a.k, a.m)) {
        const size_t lds = (size_t)a.m * a.k * sizeof(gf::PermTab);
        hipLaunchKernelGGL((rs_locate_multi_scan_kernel<ROWS, true>), dim3(grid), dim3(kThreads), lds, s, a);
    } else {
        hipLaunchKernelGGL((rs_locate_multi_scan_kernel<ROWS, false>), dim3(grid), dim3(kThreads), 0, s, a);
    }
    return hipGetLastError();
}

// The instances of rs_locate_kernel (fec_locate.hip): 2, 4, 8 and 16 rows.
hipError_t launch_rs_locate_multi_scan(const LocateMultiScanArgs& a, int grid, hipStream_t s) {
    if (a.total == 0 || a.m == 0) return hipSuccess;
    if (a.m <= 2) return locate_multi_scan_dispatch<2>(a, grid, s);
    if (a.m <= 4) return locate_multi_scan_dispatch<4>(a, grid, s);
    if (a.m <= 8) return locate_multi_scan_dispatch<8>(a, grid, s);
    return locate_multi_scan_dispatch<kLocateMultiRows>(a, grid, s);
}

hipError_t launch_rs_locate_multi_solve(const LocateMultiSolveArgs& a, hipStream_t s) {
    if (a.nwords == 0 || a.s.m == 0) return hipSuccess;
    const uint32_t grid = (a.nwords + kThreads - 1) / kThreads;
    const LocateSolveLds lds = locate_solve_lds(a.s.k, a.s.m);
    if (lds.tabs)
        hipLaunchKernelGGL(rs_locate_multi_solve_kernel<true>, dim3(grid), dim3(kThreads), lds.bytes, s, a);
    else
        hipLaunchKernelGGL(rs_locate_multi_solve_kernel<false>, dim3(grid), dim3(kThreads), lds.bytes, s, a);
    return hipGetLastError();
}

hipError_t launch_rs_locate_multi_finalize(const LocateMultiFinArgs& a, hipStream_t s) {
    if (a.nblocks == 0) return hipSuccess;
    const uint32_t grid = (a.nblocks + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(rs_locate_multi_finalize_kernel, dim3(grid), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace fk
