// fec_verify.hip — RS verify for gfx950 (klauspost Encoder.Verify, batched): does the parity a
// block holds equal what the encode would write from its data? The generic encode's body
// (fec_encode.hip rs_encode_kernel) with the stored parity folded in and nothing written but one
// word per bad block.
#include "fec_flat.hpp"
#include "fec_verify.hpp"

namespace fk {

// One lane = one 16-byte column chunk of one block. The accumulators start from the stored parity
// chunks (their loads go out ahead of the data loads), so after the k data chunks are folded through
// the code's PermTabs each accumulator is the difference between the stored and the computed
// parity. Differences are ORed over rows under the tail mask: bytes at and past len of a slot, data
// or parity, meet only bytes of the same column, and those columns are masked off.
//
// The statuses are 1 on entry. A wave's lanes may cover several blocks (short shards), and a block
// may span waves and workgroups (long shards): among the lanes of a wave that found a difference,
// the first lane of each block exchanges 0 into the block's word, and counts the block if it read
// back 1. A clean batch issues no atomics.
template <int MAXM, bool LDS_TABS>
__global__ __launch_bounds__(kThreads) void rs_verify_kernel(VerifyArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const gf::PermTab* tabs = stage_tabs<LDS_TABS>(a.tabs, a.m * a.k * 8, smem);
    if constexpr (LDS_TABS) __syncthreads();
    const uint32_t k = a.k, m = a.m;
    const FlatItem f = flat_item(a.total, a.cps, a.div_cps);
    const uint32_t b = f.b, c = f.c;
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
    d = keep_bytes(d, a.len - c * kChunk);
    const bool bad = f.live && (d.x | d.y | d.z | d.w) != 0;
    uint64_t todo = __ballot(bad);   // wave-uniform
    const uint32_t lane = threadIdx.x & 63u;
    while (todo) {
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
        const uint32_t lb = (uint32_t)__shfl((int)b, (int)leader);
        todo &= ~__ballot(bad && b == lb);
        if (lane == leader)
            if (atomicExch(a.status + b, 0) == 1 && a.count) atomicAdd(a.count, 1u);
    }
}

template <int MAXM>
static hipError_t verify_dispatch(const VerifyArgs& a, int grid, hipStream_t s) {
    if (a.m * a.k <= (uint32_t)kMaxLdsTabs) {
        const size_t lds = (size_t)a.m * a.k * sizeof(gf::PermTab);
        hipLaunchKernelGGL((rs_verify_kernel<MAXM, true>), dim3(grid), dim3(kThreads), lds, s, a);
    } else {
        hipLaunchKernelGGL((rs_verify_kernel<MAXM, false>), dim3(grid), dim3(kThreads), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_rs_verify(const VerifyArgs& a, int grid, hipStream_t s) {
    if (a.total == 0 || a.m == 0) return hipSuccess;
    if (a.m <= 1) return verify_dispatch<1>(a, grid, s);
    if (a.m <= 2) return verify_dispatch<2>(a, grid, s);
    if (a.m <= 4) return verify_dispatch<4>(a, grid, s);
    if (a.m <= 8) return verify_dispatch<8>(a, grid, s);
    return verify_dispatch<16>(a, grid, s);   // the caller splits m > 16
}

}  // namespace fk
