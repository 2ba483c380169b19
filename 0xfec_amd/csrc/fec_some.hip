// fec_some.hip — reconstruct-some for gfx950 (klauspost Reconstruct / ReconstructSome, in place,
// k + m <= 32): every wanted missing shard of a block, data or parity, rebuilt into its own slot
// from the first k present shards. rs_plan_some_kernel turns each block's two masks into a record
// (fec_some.hpp some_plan_record), which is all this file holds: the rebuild is the wide decode's
// tile (fec_wide.hip rs_rebuild_wide_kernel<true>: row passes of 16, so the up to 31 rows of RS(1,31)
// fit) with the store address of a row chosen between the data and the parity region by its shard
// index.
#include "fec_device.hpp"
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
                                            s_exp, s_log, a.logv);
        if (st) wave_flag(a.err, kStickyTooFew);   // too few shards, as rs_plan_kernel reports it
        if (a.status) a.status[b] = st;
    }
    __syncthreads();
    const uint32_t nrec = min((uint32_t)kSomePlanThreads, a.nblocks - b0);
    const uint32_t nw = nrec * lay.stride / 16;
    const uint4* src = reinterpret_cast<const uint4*>(recs);
    uint4* dst = reinterpret_cast<uint4*>(a.plans + (uint64_t)b0 * lay.stride);
    for (uint32_t i = threadIdx.x; i < nw; i += kSomePlanThreads) dst[i] = src[i];
}

hipError_t launch_rs_plan_some(const SomePlanArgs& a, hipStream_t s) {
    const int grid = (int)((a.nblocks + kSomePlanThreads - 1) / kSomePlanThreads);
    if (grid == 0) return hipSuccess;
    const size_t lds = kSomePlanTables + (size_t)kSomePlanThreads * a.lay.stride;
    hipLaunchKernelGGL(rs_plan_some_kernel, dim3(grid), dim3(kSomePlanThreads), lds, s, a);
    return hipGetLastError();
}

}  // namespace fk
