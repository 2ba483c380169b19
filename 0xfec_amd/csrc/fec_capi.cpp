// fec_capi.cpp — C ABI of the MI355X FEC codec (include/fec_hip.h).
//
// Owns the per-device context: HIP stream, per-(k, m) code cache (systematic matrix,
// device parity rows, encode PermTabs), decode plan workspace, pinned staging for the
// FEC_HOST path. No CPU compute fallback exists: without a HIP device every compute
// entry point fails with FEC_ERR_NO_DEVICE / FEC_ERR_HIP.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <map>
#include <memory>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/fec_hip.h"
#include "fec_kernels.hpp"
#include "fec_ragged.hpp"
#include "fec_some.hpp"
#include "fec_update.hpp"
#include "fec_verify.hpp"
#include "fec_wide.hpp"
#include "gf256.h"
#include "rs_matrix.hpp"

namespace {

struct Code {
    int k = 0, m = 0;
    std::vector<uint8_t> matrix;   // n x k
    uint8_t* d_prows = nullptr;    // m x k
    uint32_t* d_tabs = nullptr;    // m x k PermTabs
    uint32_t* d_dytabs = nullptr;  // dyadic codes: leaf PermTabs of the split-recursive encode
    uint32_t* d_single = nullptr;  // single-erasure decode tables (fk::direct_table_words), when small
    uint32_t* d_single_coef = nullptr;   // their coefficient bytes, (k*m) rows of ceil(k/4) dwords
    std::vector<uint32_t> single_coef;   // host copy
    uint8_t* d_dall = nullptr;     // n bytes: sum_{t != s} log(s ^ t) mod 255 (sorted plans)
};

// Parity row r, column j of a dyadic code is g(r ^ j), g = parity row 0 (fec_kernels.hip,
// "dyadic encode"); k and m powers of two, m <= k. Returns the leaf constants of the recursion
// conv(C, D) = (P ^ Q, R ^ P ^ Q) for each group h of m columns, in the kernel's order (P's
// leaves, Q's, R's), or nothing when the matrix is not dyadic.
std::vector<uint8_t> dyadic_leaves(const std::vector<uint8_t>& matrix, int k, int m) {
    auto pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
    if (!pow2(k) || !pow2(m) || m > k) return {};
    const uint8_t* g = matrix.data() + (size_t)k * k;
    for (int r = 1; r < m; ++r)
        for (int j = 0; j < k; ++j)
            if (g[(size_t)r * k + j] != g[r ^ j]) return {};
    std::vector<uint8_t> out;
    std::function<void(const std::vector<uint8_t>&)> leaves = [&](const std::vector<uint8_t>& c) {
        if (c.size() == 1) {
            out.push_back(c[0]);
            return;
        }
        const size_t h = c.size() / 2;
        std::vector<uint8_t> lo(c.begin(), c.begin() + h), hi(c.begin() + h, c.end()), sum(h);
        for (size_t i = 0; i < h; ++i) sum[i] = (uint8_t)(lo[i] ^ hi[i]);
        leaves(lo);
        leaves(hi);
        leaves(sum);
    };
    for (int h = 0; h < k / m; ++h) leaves(std::vector<uint8_t>(g + (size_t)h * m, g + (size_t)(h + 1) * m));
    return out;
}


// Bytes of staged shards per FEC_HOST chunk (x2 buffers, in and out).
constexpr size_t kStageBytes = size_t(128) << 20;
// Upper bound on decode plan workspace.
constexpr size_t kPlanBytes = size_t(256) << 20;
// nblocks * chunks-per-shard must stay below 2^31 per launch (32-bit item ids).
constexpr uint64_t kMaxItems = uint64_t(1) << 31;

}  // namespace

// Device scratch of the kernels enqueued on one stream: decode plan records. Each stream the ctx
// launches on (its own / the caller's, and one per host-path staging set) has its own, so
// launches that overlap on different streams never share one (nor free one the other stream
// still reads).
struct Work {
    uint8_t* d_plans = nullptr;
    size_t plans_cap = 0;
    uint32_t* d_wflags = nullptr;   // routed in-place decode: the classify pass's route word
    size_t wflags_cap = 0;
    void release() {
        if (d_plans) (void)hipFree(d_plans);
        if (d_wflags) (void)hipFree(d_wflags);
        *this = Work{};
    }
};

// One staging set of the host-resident path: pinned host and device buffers for one chunk of
// blocks, and the events that carry that chunk through the pipeline's streams (HostPipe).
struct HostSet {
    uint8_t* h_in = nullptr;
    uint8_t* h_out = nullptr;
    uint8_t* d_in = nullptr;
    uint8_t* d_out = nullptr;
    uint32_t* h_masks = nullptr;
    uint32_t* d_masks = nullptr;
    int32_t* h_status = nullptr;
    int32_t* d_status = nullptr;
    uint8_t* d_raw_in = nullptr;    // FEC_HOST_PINNED: the caller's span, copied linearly (fec_pack.hip)
    uint8_t* d_raw_out = nullptr;   // FEC_HOST_PINNED: the packed image of the outputs, copied down linearly
    size_t in_cap = 0, out_cap = 0, blk_cap = 0, raw_in_cap = 0, raw_out_cap = 0;
    hipEvent_t up_done = nullptr;     // its H2D copies have landed
    hipEvent_t k_done = nullptr;      // its kernels are done (the device inputs are free)
    hipEvent_t down_done = nullptr;   // its D2H copies have landed (the set is free)
};

// The host-resident pipeline. Chunk c of a call uses set c % kHostSets and moves through three
// streams in order: H2D copies on `up`, kernels on `comp`, D2H copies on `down`, ordered by the
// set's events alone. PCIe's two directions and the kernels of different chunks therefore overlap,
// and the up direction (the larger one on every path) never waits for the host: the host blocks only
// to reuse a set, on its chunk kHostSets back, and at the end of a call. Measured on one MI355X
// (tools/pcie_duplex_probe.hip, profiles/r04/pcie_duplex_probe_r04b.log): H2D 57.6 GB/s, D2H 57.0,
// both at once 48.6 each way; this shape with 64 MiB chunks moved 53.8 GB/s up.
constexpr int kHostSets = 3;
struct HostPipe {
    hipStream_t up = nullptr, comp = nullptr, down = nullptr;
    Work w;   // scratch of the kernels on comp
    HostSet set[kHostSets];
};

struct fec_ctx {
    int device = 0;
    hipStream_t own = nullptr;
    hipStream_t stream = nullptr;
    std::map<std::pair<int, int>, Code> codes;
    Work main;               // scratch of the kernels on `own` / the caller's stream
    Work* work = &main;      // scratch of the kernels on `stream` (on_stream switches both)
    int* d_err = nullptr;    // [0] sticky device-path error, [1] host-path error
    uint8_t* h_stage = nullptr;
    uint8_t* d_stage = nullptr;
    size_t stage_cap = 0;
    uint32_t* d_masks = nullptr;
    int32_t* d_status = nullptr;
    size_t masks_cap = 0;
    HostPipe pipe;           // host-resident path (FEC_HOST / FEC_HOST_PINNED)
    hipEvent_t handoff = nullptr;   // orders a newly set stream after the previous one
};

#define HIP_TRY(expr)                      \
    do {                                   \
        if ((expr) != hipSuccess) {        \
            (void)hipGetLastError();       \
            return FEC_ERR_HIP;            \
        }                                  \
    } while (0)

static int select_device(fec_ctx* ctx) {
    if (!ctx) return FEC_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    return FEC_OK;
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

static int get_code(fec_ctx* ctx, int k, int m, Code** out) {
    if (k <= 0 || m < 0) return FEC_ERR_INV_SHARD_NUM;
    if (k + m > 256) return FEC_ERR_MAX_SHARD_NUM;
    auto key = std::make_pair(k, m);
    auto it = ctx->codes.find(key);
    if (it != ctx->codes.end()) {
        *out = &it->second;
        return FEC_OK;
    }
    Code c;
    c.k = k;
    c.m = m;
    c.matrix = rs::build_matrix(k, k + m);
    if (c.matrix.empty()) return FEC_ERR_INV_SHARD_NUM;
    if (m > 0) {
        std::vector<uint32_t> tabs((size_t)m * k * 8);
        for (int r = 0; r < m; ++r)
            for (int j = 0; j < k; ++j) {
                gf::PermTab t = gf::make_permtab(c.matrix[(size_t)(k + r) * k + j]);
                memcpy(&tabs[((size_t)r * k + j) * 8], &t, sizeof(t));
            }
        HIP_TRY(hipMalloc(&c.d_prows, (size_t)m * k));
        HIP_TRY(hipMalloc(&c.d_tabs, tabs.size() * 4));
        HIP_TRY(hipMemcpy(c.d_prows, c.matrix.data() + (size_t)k * k, (size_t)m * k, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c.d_tabs, tabs.data(), tabs.size() * 4, hipMemcpyHostToDevice));
        // single-erasure plans: data shard E0 lost, parity R0 the first present one; inputs are
        // the other data shards in order, then parity R0 (the first k present shards):
        // x_E0 = inv(A[R0][E0]) * (p_R0 ^ sum_{j != E0} A[R0][j] x_j)   (reed_solomon.go:124)
        if (k + m <= FEC_MAX_DECODE_SHARDS) {
            // the coefficient bytes of every single-erasure plan (small for every decodable code:
            // RS(20,30) 4 KB): the direct decode reads a wave's rows by scalar loads
            const size_t kw = ((size_t)k + 3) / 4;
            std::vector<uint32_t> sc((size_t)k * m * kw, 0);
            for (int e0 = 0; e0 < k; ++e0)
                for (int r0 = 0; r0 < m; ++r0) {
                    const uint8_t* row = c.matrix.data() + (size_t)(k + r0) * k;
                    const uint8_t inv = gf::inv(row[e0]);
                    uint8_t* dst = reinterpret_cast<uint8_t*>(&sc[((size_t)e0 * m + r0) * kw]);
                    for (int j = 0, pos = 0; j <= k; ++j)
                        if (j != e0) dst[pos++] = j < k ? gf::mul(inv, row[j]) : inv;
                }
            c.single_coef = sc;
            HIP_TRY(hipMalloc(&c.d_single_coef, sc.size() * 4));
            HIP_TRY(hipMemcpy(c.d_single_coef, sc.data(), sc.size() * 4, hipMemcpyHostToDevice));
        }
        if (k + m <= FEC_MAX_DECODE_SHARDS && fk::direct_table_words((uint32_t)k, (uint32_t)m) * 4 <= 16 * 1024) {
            // the same plans expanded to PermTabs (k*m*k*32 bytes; small codes only)
            std::vector<uint32_t> st(fk::direct_table_words((uint32_t)k, (uint32_t)m), 0);
            for (int e0 = 0; e0 < k; ++e0)
                for (int r0 = 0; r0 < m; ++r0) {
                    const uint8_t* row = c.matrix.data() + (size_t)(k + r0) * k;
                    const uint8_t inv = gf::inv(row[e0]);
                    for (int j = 0, pos = 0; j <= k; ++j) {
                        if (j == e0) continue;
                        const uint8_t coef = j < k ? gf::mul(inv, row[j]) : inv;
                        gf::PermTab t = gf::make_permtab(coef);
                        memcpy(&st[(((size_t)e0 * m + r0) * k + pos) * 8], &t, sizeof(t));
                        ++pos;
                    }
                }
            HIP_TRY(hipMalloc(&c.d_single, st.size() * 4));
            HIP_TRY(hipMemcpy(c.d_single, st.data(), st.size() * 4, hipMemcpyHostToDevice));
        }
        const std::vector<uint8_t> leaves = dyadic_leaves(c.matrix, k, m);
        if (!leaves.empty() && leaves.size() <= (size_t)m * k) {   // staged like m x k tables
            std::vector<uint32_t> dy((size_t)m * k * 8, 0);
            for (size_t i = 0; i < leaves.size(); ++i) {
                gf::PermTab t = gf::make_permtab(leaves[i]);
                memcpy(&dy[i * 8], &t, sizeof(t));
            }
            HIP_TRY(hipMalloc(&c.d_dytabs, dy.size() * 4));
            HIP_TRY(hipMemcpy(c.d_dytabs, dy.data(), dy.size() * 4, hipMemcpyHostToDevice));
        }
    }
    // (for m == 0 too: the sorted-plan kernels stage it whatever the code, and a reconstruct of a
    // code without parity, where every loss is a failed block, takes them on long shards)
    if (k + m <= FEC_MAX_DECODE_SHARDS) {
        uint8_t dall[FEC_MAX_DECODE_SHARDS] = {};
        for (int sidx = 0; sidx < k + m; ++sidx) {
            unsigned d = 0;
            for (int t = 0; t < k + m; ++t)
                if (t != sidx) d += gf::kTables.log[sidx ^ t];
            dall[sidx] = (uint8_t)(d % 255u);
        }
        HIP_TRY(hipMalloc(&c.d_dall, FEC_MAX_DECODE_SHARDS));
        HIP_TRY(hipMemcpy(c.d_dall, dall, FEC_MAX_DECODE_SHARDS, hipMemcpyHostToDevice));
    }
    auto res = ctx->codes.emplace(key, std::move(c));
    *out = &res.first->second;
    // the uploads above are plain hipMemcpy (null stream, and from pageable memory they may return
    // before the DMA lands): finish them before a kernel on a non-blocking ctx stream reads a table
    HIP_TRY(hipDeviceSynchronize());
    return FEC_OK;
}

// Grow the buffers that share capacity *cap (counted in units of `unit` bytes) to hold n units:
// pinned host memory where `pinned`, else device memory. The old buffers are freed only after
// ctx->stream, the only stream that reads them, has drained.
struct GrowBuf {
    void** p;
    bool pinned;
};
static int grow(fec_ctx* ctx, size_t* cap, size_t n, size_t unit, std::initializer_list<GrowBuf> bufs) {
    if (n <= *cap) return FEC_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *cap = 0;
    for (const GrowBuf& b : bufs) {
        void* old = *b.p;
        *b.p = nullptr;
        if (old) HIP_TRY(b.pinned ? hipHostFree(old) : hipFree(old));
    }
    for (const GrowBuf& b : bufs)
        HIP_TRY(b.pinned ? hipHostMalloc(b.p, n * unit, hipHostMallocDefault) : hipMalloc(b.p, n * unit));
    *cap = n;
    return FEC_OK;
}
static int grow_plans(fec_ctx* ctx, size_t bytes) {
    return grow(ctx, &ctx->work->plans_cap, bytes, 1, {{(void**)&ctx->work->d_plans, false}});
}
static int grow_wflags(fec_ctx* ctx, size_t n) {
    return grow(ctx, &ctx->work->wflags_cap, n, 4, {{(void**)&ctx->work->d_wflags, false}});
}
static int grow_stage(fec_ctx* ctx, size_t bytes) {
    return grow(ctx, &ctx->stage_cap, bytes, 1, {{(void**)&ctx->h_stage, true}, {(void**)&ctx->d_stage, false}});
}
static int grow_masks(fec_ctx* ctx, size_t n) {
    return grow(ctx, &ctx->masks_cap, n, 4, {{(void**)&ctx->d_masks, false}, {(void**)&ctx->d_status, false}});
}

static size_t round16(size_t x) { return (x + 15) & ~size_t(15); }

// Workgroups for a flat (block, chunk) item launch: one item per lane (total < 2^31).
static int flat_grid(uint32_t total) {
    return (int)std::max<uint64_t>(1, ((uint64_t)total + fk::kThreads - 1) / fk::kThreads);
}

// ---------------------------------------------------------------- device-memory cores

// A batch is cut into launches of consecutive blocks: fewer than kMaxItems items (block, chunk)
// each, and, where a launch keeps a plan record of `stride` bytes per block, at most kPlanBytes of
// records.
static uint32_t chunks_of(size_t len) { return (uint32_t)((len + fk::kChunk - 1) / fk::kChunk); }

static size_t blocks_per_launch(size_t nblocks, uint32_t cps, size_t stride = 0) {
    size_t per = (size_t)(kMaxItems / cps);
    if (stride) per = std::min(per, kPlanBytes / stride);
    return std::max<size_t>(1, std::min(per, nblocks));
}

// body(b0, nb) for each launch's blocks [b0, b0 + nb), until one fails.
template <class F>
static int for_slices(size_t nblocks, size_t per_launch, F body) {
    for (size_t b0 = 0; b0 < nblocks; b0 += per_launch) {
        const int rc = body(b0, std::min(per_launch, nblocks - b0));
        if (rc) return rc;
    }
    return FEC_OK;
}

// What EncodeArgs, VerifyArgs and RagEncodeArgs share: the data of the launch's first block and the
// tables of the pass of up to 16 parity rows from r0.
template <class Args>
static void fill_row_pass(Args& a, const Code* code, int r0, const uint8_t* data, size_t dbs, size_t ss) {
    a.in = data;
    a.in_bs = dbs;
    a.ss = ss;
    a.k = (uint32_t)code->k;
    a.m = (uint32_t)std::min(16, code->m - r0);
    a.tabs = code->d_tabs + (size_t)r0 * code->k * 8;
}

static int rs_encode_device(fec_ctx* ctx, Code* code, size_t len, size_t nblocks, const uint8_t* data,
                            size_t dbs, uint8_t* parity, size_t pbs, size_t ss) {
    const uint32_t cps = chunks_of(len);
    const int k = code->k;
    return for_slices(nblocks, blocks_per_launch(nblocks, cps), [&](size_t b0, size_t nb) -> int {
        for (int r0 = 0; r0 < code->m; r0 += 16) {
            fk::EncodeArgs a{};
            fill_row_pass(a, code, r0, data + b0 * dbs, dbs, ss);
            a.out = parity + b0 * pbs + (size_t)r0 * ss;
            a.out_bs = pbs;
            a.len = (uint32_t)len;
            a.cps = cps;
            a.total = (uint32_t)(nb * cps);
            a.div_cps = fk::make_fastdiv(cps);
            a.dytabs = (r0 == 0 && (int)a.m == code->m) ? code->d_dytabs : nullptr;
            a.sp = fk::encode_store_policy(fk::g_tune.st_pol, {data, dbs, ss, (uint64_t)k},
                                           {parity, pbs, ss, (uint64_t)code->m}, len, nblocks);
            if (fk::fixed_encode_applies((uint32_t)k, a.m, a.dytabs != nullptr)) {
                HIP_TRY(fk::launch_rs_encode_fixed(a, ctx->stream));
                continue;
            }
            HIP_TRY(fk::launch_rs_encode(a, flat_grid(a.total), ctx->stream));
        }
        return FEC_OK;
    });
}

// What a slice's PlanArgs and ReconArgs hold in the uniform and the ragged reconstruct alike: blocks
// [b0, b0 + nb) of the call, records of layout `lay` in the stream's workspace, tiles of G blocks.
struct ReconCall {
    uint8_t* data;
    size_t dbs;
    const uint8_t* parity;
    size_t pbs, ss, pss;
    const uint32_t* masks;
    int32_t* status;
    int* err;
    uint8_t* out;
    size_t out_bs;
    uint32_t out_slots;
};
static void fill_recon_slice(fk::PlanArgs& p, fk::ReconArgs& a, fec_ctx* ctx, const Code* code, const ReconCall& c,
                             size_t len, uint32_t cps, uint32_t maxe, const fk::PlanLayout& lay, uint32_t G,
                             size_t b0, size_t nb) {
    p.masks = c.masks + b0;
    p.plans = ctx->work->d_plans;
    p.status = c.status ? c.status + b0 : nullptr;
    p.err = c.err;
    p.prows = code->d_prows;
    p.k = (uint32_t)code->k;
    p.m = (uint32_t)code->m;
    p.nblocks = (uint32_t)nb;
    p.maxe = maxe;
    p.lay = lay;
    p.max_out = c.out ? c.out_slots : 0;
    p.dall = code->d_dall;   // (read by the sorted plans only)
    a.data = c.data + b0 * c.dbs;
    a.parity = c.parity + b0 * c.pbs;
    a.dbs = c.dbs;
    a.pbs = c.pbs;
    a.ss = c.ss;
    a.pss = c.pss;
    a.plans = ctx->work->d_plans;
    a.k = p.k;
    a.len = (uint32_t)len;
    a.cps = cps;
    a.nblocks = (uint32_t)nb;
    a.maxe = maxe;
    a.lay = lay;
    a.g = G;
    a.ntiles = (uint32_t)((nb + G - 1) / G);
    a.div_cps = fk::make_fastdiv(cps);
    a.out = c.out ? c.out + b0 * c.out_bs : nullptr;
    a.out_bs = c.out_bs;
}

static int rs_reconstruct_device(fec_ctx* ctx, Code* code, size_t len, size_t nblocks, uint8_t* data,
                                 size_t dbs, const uint8_t* parity, size_t pbs, size_t ss, const uint32_t* masks,
                                 int32_t* status, int* err, uint8_t* out = nullptr, size_t out_bs = 0,
                                 uint32_t out_slots = 0, size_t pss = 0) {
    if (pss == 0) pss = ss;
    if ((ss | pss) >> 32) return FEC_ERR_INVALID_ARG;   // the rebuild kernels take 32-bit shard strides
    const uint32_t k = (uint32_t)code->k, m = (uint32_t)code->m;
    const uint32_t maxe = std::max<uint32_t>(1, std::min(k, m));
    const uint32_t cps = chunks_of(len);
    const fk::PlanLayout lay_block = fk::plan_layout(k, maxe), lay_sorted = fk::plan_layout(k, maxe, true);
    // Three forms:
    //  * direct (fec_recover.hip): no plan kernel; single-erasure tables of the code, for calls
    //    where no block can need more (one output slot per block, or m = 1). Small codes (RS(2,3),
    //    RS(8,12)) and RS(16,24) / RS(20,30) (RS(20,30) single erasure +15 % over plan + rebuild,
    //    r03h);
    //  * shards of 32+ chunks: sorted plans (fec_plan.hip), then the wave-form rebuild
    //    (fec_rebuild.hip for RS(16,24) / RS(20,30) with 64+ chunks, else fec_decode.hip);
    //  * short shards: plans in block order, then the workgroup-tile rebuild.
    //  * routed (in-place calls of RS(8,12)): a classify pass reduces the masks to one word; the
    //    sorted plans run only if some block has two or more erased data shards, and one kernel
    //    runs the direct body or the wave rebuild by that word (fec_recover.hip).
    const bool single_slot = out && out_slots == 1;
    const bool direct = code->d_single_coef && fk::direct_recon_applies(k, m, cps, single_slot);
    const bool wave = !direct && fk::wave_recon_applies(cps, k, maxe, lay_sorted.stride);
    const bool routed = wave && !out && code->d_single_coef && !fk::rebuild_k_applies(k, maxe, cps) &&
                        fk::routed_recon_applies(k, m, cps, maxe, lay_sorted.stride);
    const fk::PlanLayout lay = wave ? lay_sorted : lay_block;
    const size_t per_launch = blocks_per_launch(nblocks, cps, direct ? 0 : lay.stride);
    if (!direct) {
        const int rc = grow_plans(ctx, per_launch * lay.stride);
        if (rc) return rc;
    }
    if (routed) {
        const int rc = grow_wflags(ctx, 1);
        if (rc) return rc;
    }
    const uint32_t G = fk::pick_tile_blocks(cps, k, maxe, lay);
    const ReconCall call{data, dbs, parity, pbs, ss, pss, masks, status, err, out, out_bs, out_slots};
    return for_slices(nblocks, per_launch, [&](size_t b0, size_t nb) -> int {
        fk::PlanArgs p{};
        fk::ReconArgs a{};
        fill_recon_slice(p, a, ctx, code, call, len, cps, maxe, lay, G, b0, nb);
        a.sorted = wave ? 1u : 0u;
        if (direct || routed) {
            a.masks = p.masks;
            a.status = p.status;
            a.err = p.err;
            a.prows = p.prows;
            a.m = m;
            a.max_out = p.max_out;
            a.single = code->d_single;
            a.single_coef = code->d_single_coef;
            a.single_coef_host = code->single_coef.data();
            a.sp = fk::decode_store_policy(fk::g_tune.dst_pol, {data, dbs, ss, k}, {parity, pbs, pss, m},
                                           {out, out_bs, ss, out_slots}, len, nblocks);
        }
        if (direct) {
            HIP_TRY(fk::launch_rs_recover_direct(a, ctx->stream));
        } else if (routed) {
            a.route = p.route = ctx->work->d_wflags;
            HIP_TRY(fk::launch_rs_route_classify(a, ctx->work->d_wflags, ctx->stream));
            HIP_TRY(fk::launch_rs_plan_sorted(p, ctx->stream));
            HIP_TRY(fk::launch_rs_reconstruct_routed(a, ctx->stream));
        } else if (wave) {
            HIP_TRY(fk::launch_rs_plan_sorted(p, ctx->stream));
            if (fk::rebuild_k_applies(k, maxe, cps)) HIP_TRY(fk::launch_rs_rebuild_k(a, ctx->stream));
            else HIP_TRY(fk::launch_rs_reconstruct_wave(a, ctx->stream));
        } else {
            HIP_TRY(fk::launch_rs_plan(p, ctx->stream));
            HIP_TRY(fk::launch_rs_reconstruct(a, (int)std::max<uint32_t>(1, a.ntiles), ctx->stream));
        }
        return FEC_OK;
    });
}

// The wide tile (fec_wide.hip rs_rebuild_wide_kernel) over a batch: records of `rows` output rows per
// block, cut into launches under kPlanBytes of records and kMaxItems items; for each, plan(b0, nb,
// lay) writes the launch's records into the stream's workspace, then the tile rebuilds from them:
// `some` false into out (if set) or the data region, true into the data and the parity region.
template <class Plan>
static int rs_rebuild_tiles(fec_ctx* ctx, uint32_t k, uint32_t rows, size_t len, size_t nblocks, uint8_t* data,
                            size_t dbs, const uint8_t* parity, size_t pbs, size_t ss, uint8_t* out, size_t out_bs,
                            bool some, Plan plan) {
    if (ss >> 32) return FEC_ERR_INVALID_ARG;   // the rebuild kernel takes 32-bit shard strides
    const uint32_t cps = chunks_of(len);
    const fk::WideLayout lay = fk::wide_layout(k, rows);
    const size_t per_launch = blocks_per_launch(nblocks, cps, lay.stride);
    const int rc = grow_plans(ctx, per_launch * lay.stride);
    if (rc) return rc;
    uint32_t G, C, TK;
    fk::wide_tile_shape(cps, k, &G, &C, &TK);
    return for_slices(nblocks, per_launch, [&](size_t b0, size_t nb) -> int {
        fk::WideReconArgs a{};
        a.data = data + b0 * dbs;
        a.parity = parity + b0 * pbs;
        a.dbs = dbs;
        a.pbs = pbs;
        a.ss = (uint32_t)ss;
        a.plans = ctx->work->d_plans;
        a.lay = lay;
        a.k = k;
        a.len = (uint32_t)len;
        a.cps = cps;
        a.nblocks = (uint32_t)nb;
        a.g = G;
        a.c = C;
        a.tk = TK;
        a.nctiles = (cps + C - 1) / C;
        a.ntiles = (uint32_t)((nb + G - 1) / G) * a.nctiles;
        a.div_c = fk::make_fastdiv(C);
        a.div_nct = fk::make_fastdiv(a.nctiles);
        a.out = out ? out + b0 * out_bs : nullptr;
        a.out_bs = out_bs;
        HIP_TRY(plan(b0, nb, lay));
        HIP_TRY(fk::launch_rs_rebuild_wide(a, some, ctx->stream));
        return FEC_OK;
    });
}

// Wide reconstruct / recover (fec_wide.hip): present masks of mask_words words per block, codes of
// up to 256 shards.
static int rs_reconstruct_wide_device(fec_ctx* ctx, int ki, int mi, size_t len, size_t nblocks, uint8_t* data,
                                      size_t dbs, const uint8_t* parity, size_t pbs, size_t ss,
                                      const uint32_t* masks, size_t mask_words, int32_t* status, int* err,
                                      uint8_t* out = nullptr, size_t out_bs = 0, uint32_t out_slots = 0) {
    const uint32_t k = (uint32_t)ki, m = (uint32_t)mi;
    uint32_t rows = std::max<uint32_t>(1, std::min(k, m));
    if (out) rows = std::min(rows, out_slots);
    return rs_rebuild_tiles(ctx, k, rows, len, nblocks, data, dbs, parity, pbs, ss, out, out_bs, false,
                            [&](size_t b0, size_t nb, const fk::WideLayout& lay) {
                                fk::WidePlanArgs p{};
                                p.masks = masks + b0 * mask_words;
                                p.mask_words = (uint32_t)mask_words;
                                p.plans = ctx->work->d_plans;
                                p.status = status ? status + b0 : nullptr;
                                p.err = err;
                                p.k = k;
                                p.n = k + m;
                                p.nblocks = (uint32_t)nb;
                                p.rows = rows;
                                p.max_out = out ? out_slots : 0;
                                p.lay = lay;
                                p.div_k = fk::make_fastdiv(k);
                                return fk::launch_rs_plan_wide(p, ctx->stream);
                            });
}

// Verify (fec_verify.hip): statuses pre-set to 1 and the count to 0 on the stream, then the encode's
// launches (cut under kMaxItems items, parity rows in passes of 16) with the stored parity folded
// in: a pass clears the word of a block it finds bad and counts it if no earlier pass had.
static int rs_verify_device(fec_ctx* ctx, Code* code, size_t len, size_t nblocks, const uint8_t* data, size_t dbs,
                            const uint8_t* parity, size_t pbs, size_t ss, int32_t* status, uint32_t* count) {
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)status, 1, nblocks, ctx->stream));
    if (count) HIP_TRY(hipMemsetAsync(count, 0, sizeof(uint32_t), ctx->stream));
    const uint32_t cps = chunks_of(len);
    return for_slices(nblocks, blocks_per_launch(nblocks, cps), [&](size_t b0, size_t nb) -> int {
        for (int r0 = 0; r0 < code->m; r0 += 16) {
            fk::VerifyArgs a{};
            fill_row_pass(a, code, r0, data + b0 * dbs, dbs, ss);
            a.par = parity + b0 * pbs + (size_t)r0 * ss;
            a.par_bs = pbs;
            a.len = (uint32_t)len;
            a.cps = cps;
            a.total = (uint32_t)(nb * cps);
            a.div_cps = fk::make_fastdiv(cps);
            a.status = status + b0;
            a.count = count;
            HIP_TRY(fk::launch_rs_verify(a, flat_grid(a.total), ctx->stream));
        }
        return FEC_OK;
    });
}

// Update and encode-idx (fec_update.hip): the regions and masks of one call. `in` is the data folded
// in (update: the new version), `old` the old version (encode-idx: null).
struct UpdateCall {
    const uint8_t* in;
    size_t in_bs;
    const uint8_t* old;
    size_t old_bs;
    uint8_t* parity;
    size_t pbs, ss;
    const uint32_t* masks;
    size_t mask_words;
};

// The arguments of one launch: blocks [b0, b0 + nb) of the call, the pass of up to 16 parity rows
// from r0. No device work (fec__selftest_update_slices calls it without one).
static void fill_update_launch(fk::UpdateArgs& a, const Code* code, int r0, size_t b0, size_t nb, size_t len,
                               const UpdateCall& u) {
    const uint32_t cps = chunks_of(len);
    fill_row_pass(a, code, r0, u.in + b0 * u.in_bs, u.in_bs, u.ss);
    a.old = u.old ? u.old + b0 * u.old_bs : nullptr;
    a.old_bs = u.old_bs;
    a.par = u.parity + b0 * u.pbs + (size_t)r0 * u.ss;
    a.par_bs = u.pbs;
    a.len = (uint32_t)len;
    a.cps = cps;
    a.total = (uint32_t)(nb * cps);
    a.nblocks = (uint32_t)nb;
    a.div_cps = fk::make_fastdiv(cps);
    a.masks = u.masks + b0 * u.mask_words;
    a.mask_words = (uint32_t)u.mask_words;
}

// emit(args) for every launch of a call: the encode's cut under kMaxItems items, parity rows in
// passes of 16 (each pass reads the masked columns again), until one fails.
template <class F>
static int update_launches(const Code* code, size_t len, size_t nblocks, const UpdateCall& u, F emit) {
    return for_slices(nblocks, blocks_per_launch(nblocks, chunks_of(len)), [&](size_t b0, size_t nb) -> int {
        for (int r0 = 0; r0 < code->m; r0 += 16) {
            fk::UpdateArgs a{};
            fill_update_launch(a, code, r0, b0, nb, len, u);
            const int rc = emit(a);
            if (rc) return rc;
        }
        return FEC_OK;
    });
}

static int rs_update_device(fec_ctx* ctx, const Code* code, size_t len, size_t nblocks, const UpdateCall& u) {
    return update_launches(code, len, nblocks, u, [&](const fk::UpdateArgs& a) -> int {
        HIP_TRY(fk::launch_rs_update(a, flat_grid(a.total), ctx->stream));
        return FEC_OK;
    });
}

// Reconstruct-some (fec_some.hip): plan records in block order from the present and want masks, then
// the wide tile, storing into both regions.
static int rs_reconstruct_some_device(fec_ctx* ctx, int ki, int mi, size_t len, size_t nblocks, uint8_t* data,
                                      size_t dbs, uint8_t* parity, size_t pbs, size_t ss, const uint32_t* masks,
                                      const uint32_t* want, int32_t* status, int* err) {
    const uint32_t k = (uint32_t)ki, m = (uint32_t)mi;
    return rs_rebuild_tiles(ctx, k, fk::some_rows(m), len, nblocks, data, dbs, parity, pbs, ss, nullptr, 0, true,
                            [&](size_t b0, size_t nb, const fk::WideLayout& lay) {
                                fk::SomePlanArgs p{};
                                p.masks = masks + b0;
                                p.want = want ? want + b0 : nullptr;
                                p.plans = ctx->work->d_plans;
                                p.status = status ? status + b0 : nullptr;
                                p.err = err;
                                p.k = k;
                                p.n = k + m;
                                p.nblocks = (uint32_t)nb;
                                p.lay = lay;
                                return fk::launch_rs_plan_some(p, ctx->stream);
                            });
}

// Ragged batches (fec_ragged.hip): block b's shards are lens[b] bytes long, at most max_len. Cut
// into launches as the uniform calls are, with cps_max = the chunks of a shard of max_len bytes.
static uint32_t ragged_encode_blocks(uint32_t cps_max) {
    const int forced = fk::g_tune.rag_g;
    // a tile of full-length blocks fills one window (kRagRounds rounds)
    const uint32_t want = forced > 0 ? (uint32_t)forced : std::max<uint32_t>(1, fk::kRagWindow / cps_max);
    return fk::rag_clamp_blocks(want, cps_max);
}

static int rs_encode_ragged_device(fec_ctx* ctx, Code* code, size_t max_len, size_t nblocks, const uint8_t* data,
                                   size_t dbs, uint8_t* parity, size_t pbs, size_t ss, const uint32_t* lens,
                                   int32_t* status, int* err) {
    const uint32_t cps = chunks_of(max_len);
    const uint32_t G = ragged_encode_blocks(cps);
    return for_slices(nblocks, blocks_per_launch(nblocks, cps), [&](size_t b0, size_t nb) -> int {
        for (int r0 = 0; r0 < code->m; r0 += 16) {
            fk::RagEncodeArgs a{};
            fill_row_pass(a, code, r0, data + b0 * dbs, dbs, ss);
            a.out = parity + b0 * pbs + (size_t)r0 * ss;
            a.out_bs = pbs;
            a.max_len = (uint32_t)max_len;
            a.nblocks = (uint32_t)nb;
            a.g = G;
            a.nwin = fk::rag_windows(G, cps);
            a.lens = lens + b0;
            a.status = status ? status + b0 : nullptr;
            a.err = err;
            a.report = r0 == 0;
            HIP_TRY(fk::launch_rs_encode_ragged(a, ctx->stream));
        }
        return FEC_OK;
    });
}

// Plans in block order by rs_plan_kernel (they do not depend on the length), then the ragged tile
// rebuild, which also overrides the status of oversize blocks.
static int rs_reconstruct_ragged_device(fec_ctx* ctx, Code* code, size_t max_len, size_t nblocks, uint8_t* data,
                                        size_t dbs, const uint8_t* parity, size_t pbs, size_t ss,
                                        const uint32_t* masks, const uint32_t* lens, int32_t* status, int* err,
                                        uint8_t* out = nullptr, size_t out_bs = 0, uint32_t out_slots = 0) {
    if (ss >> 32) return FEC_ERR_INVALID_ARG;   // the rebuild takes 32-bit shard strides
    const uint32_t k = (uint32_t)code->k, m = (uint32_t)code->m;
    const uint32_t maxe = std::max<uint32_t>(1, std::min(k, m));
    const uint32_t cps = chunks_of(max_len);
    const fk::PlanLayout lay = fk::plan_layout(k, maxe);
    const size_t per_launch = blocks_per_launch(nblocks, cps, lay.stride);
    const int rc = grow_plans(ctx, per_launch * lay.stride);
    if (rc) return rc;
    // rows a block can need: the plan kernel gives a block with more erasures than slots no rows
    const uint32_t rows = out ? std::min(maxe, out_slots) : maxe;
    // Blocks per tile: as the encode's, so that a tile of full-length blocks fills one window, within
    // what LDS holds. (pick_tile_blocks, the uniform tile form's choice, looks for the fewest blocks
    // that fill the lanes of a full-length tile: RS(20,30) 3. A ragged tile has fewer items than
    // that, and its fixed cost, two barriers for the prefix and one for the tables, is paid per
    // tile. Measured, the rebuild is indifferent between the two within the run-to-run spread; the
    // encode is 30-42 % slower at 3 blocks per tile: DESIGN.md 4b.)
    const int forced = fk::g_tune.rag_g;
    uint32_t G = forced > 0 ? (uint32_t)forced : std::max<uint32_t>(1, fk::kRagWindow / cps);
    G = fk::rag_clamp_blocks(std::min(G, fk::rag_recon_max_blocks(k, rows, lay)), cps);
    const ReconCall call{data, dbs, parity, pbs, ss, ss, masks, status, err, out, out_bs, out_slots};
    return for_slices(nblocks, per_launch, [&](size_t b0, size_t nb) -> int {
        fk::PlanArgs p{};
        fk::RagReconArgs ra{};
        fill_recon_slice(p, ra.r, ctx, code, call, max_len, cps, maxe, lay, G, b0, nb);
        ra.r.status = p.status;
        ra.r.err = err;
        ra.lens = lens + b0;
        ra.max_len = (uint32_t)max_len;
        ra.nwin = fk::rag_windows(G, cps);
        ra.rows = rows;
        HIP_TRY(fk::launch_rs_plan(p, ctx->stream));
        HIP_TRY(fk::launch_rs_reconstruct_ragged(ra, ctx->stream));
        return FEC_OK;
    });
}

// The XOR calls' launch arguments for blocks [b0, b0 + nb): the encode's, and the in-place
// reconstruct's (data rebuilt where it lies, parity read).
static fk::XorArgs xor_slice(int k, size_t len, uint32_t cps, const uint8_t* in, size_t in_bs, uint8_t* out,
                             size_t out_bs, size_t ss, size_t b0, size_t nb) {
    fk::XorArgs a{};
    a.in = in + b0 * in_bs;
    a.out = out + b0 * out_bs;
    a.in_bs = in_bs;
    a.out_bs = out_bs;
    a.ss = ss;
    a.k = (uint32_t)k;
    a.len = (uint32_t)len;
    a.cps = cps;
    a.total = (uint32_t)(nb * cps);
    a.div_cps = fk::make_fastdiv(cps);
    return a;
}

static int xor_encode_device(fec_ctx* ctx, int k, size_t len, size_t nblocks, const uint8_t* data, size_t dbs,
                             uint8_t* parity, size_t pbs, size_t ss) {
    const uint32_t cps = chunks_of(len);
    return for_slices(nblocks, blocks_per_launch(nblocks, cps), [&](size_t b0, size_t nb) -> int {
        const fk::XorArgs a = xor_slice(k, len, cps, data, dbs, parity, pbs, ss, b0, nb);
        HIP_TRY(fk::launch_xor_encode(a, flat_grid(a.total), ctx->stream));
        return FEC_OK;
    });
}

static int xor_reconstruct_device(fec_ctx* ctx, int k, size_t len, size_t nblocks, uint8_t* data, size_t dbs,
                                  const uint8_t* parity, size_t pbs, size_t ss, const uint32_t* masks,
                                  int32_t* status, int* err) {
    const uint32_t cps = chunks_of(len);
    return for_slices(nblocks, blocks_per_launch(nblocks, cps), [&](size_t b0, size_t nb) -> int {
        fk::XorArgs a = xor_slice(k, len, cps, data, dbs, data, dbs, ss, b0, nb);
        a.parity = parity + b0 * pbs;
        a.par_bs = pbs;
        a.masks = masks + b0;
        a.status = status ? status + b0 : nullptr;
        a.err = err;
        a.nblocks = (uint32_t)nb;
        HIP_TRY(fk::launch_xor_reconstruct(a, flat_grid(a.total), ctx->stream));
        return FEC_OK;
    });
}

// ---------------------------------------------------------------- validation helpers

// FEC_DEVICE masks and statuses are read and written as 4-byte words (the masks by scalar loads,
// which ignore the low two address bits: a misaligned mask array would be read wrong, silently).
static int check_device_words(const void* masks, const void* status) {
    return (((uintptr_t)masks | (uintptr_t)status) & 3u) ? FEC_ERR_ALIGNMENT : FEC_OK;
}

static int check_device_layout(const void* p, size_t bs, size_t ss, size_t len) {
    if (!p) return FEC_ERR_INVALID_ARG;
    if (!aligned16(p) || (bs & 15) || (ss & 15)) return FEC_ERR_ALIGNMENT;
    if (ss < len) return FEC_ERR_INVALID_ARG;
    return FEC_OK;
}

// ---------------------------------------------------------------- host-resident path
// FEC_HOST (pageable host memory): each chunk of blocks is staged by the calling thread into a
// pinned buffer, copied up with one hipMemcpyAsync, coded, copied down with one, and its results
// copied out once its set comes round again. FEC_HOST_PINNED (the caller's buffers are pinned or
// registered): no staging copies; the caller's span of a chunk goes up in one linear DMA and is
// repacked into 16-byte slots on the device (or one 2D DMA per shard column when the span is
// sparse), and packed outputs come down the same way. Only what the code needs crosses PCIe:
// encode sends the k data shards and returns the m parity shards; reconstruct sends the data
// shards and the parity planes its blocks read, and returns only the rebuilt shards. Chunks run
// through HostPipe's three streams (up / kernels / down), kHostSets at a time.

// Blocks per chunk of a host-path call of nblocks: at most kStageBytes of staged input (128 MiB:
// larger chunks gain nothing, r04o), and for a call of fewer than kHostSets such chunks, the call
// split over the sets, so its three sets together hold about the call rather than three full
// chunks; never below kMinChunkBlocks (chunks of 3072-4096 RS(8,12) blocks lose 10 % to their
// per-chunk overhead, 6144 and up do not: host_chunk_sweep_r04o.log).
constexpr size_t kMinChunkBlocks = 6144;
static size_t host_chunk_blocks(size_t nblocks, size_t bytes_per_block) {
    if (fk::g_tune.host_chunk > 0) return std::min(nblocks, (size_t)fk::g_tune.host_chunk);   // tests: many small chunks
    const size_t full = std::max<size_t>(1, kStageBytes / std::max<size_t>(1, bytes_per_block));
    const size_t split = std::max(kMinChunkBlocks, (nblocks + kHostSets - 1) / kHostSets);
    return std::max<size_t>(1, std::min({nblocks, full, split}));
}

// Copy workers made once per process for parallel_for: a chunk's staging or scatter copy then
// costs two condition-variable hand-offs instead of creating and joining a thread per part
// (tens of microseconds each, ~40 times per pageable bench step). One call at a time: a caller
// that finds the pool busy (another thread's FEC_HOST call) makes its own threads as before.
class CopyPool {
   public:
    static CopyPool& get() {
        static CopyPool* p = new CopyPool();   // never destroyed: workers may outlive static teardown
        return *p;
    }
    // false: busy, nothing run
    bool run(unsigned parts, size_t n, const std::function<void(size_t, size_t)>& fn) {
        std::unique_lock<std::mutex> call(call_mu_, std::try_to_lock);
        if (!call.owns_lock()) return false;
        std::unique_lock<std::mutex> lk(mu_);
        while (th_.size() + 1 < parts) th_.emplace_back([this] { work(); });
        fn_ = &fn;
        n_ = n;
        per_ = (n + parts - 1) / parts;
        parts_ = (unsigned)((n + per_ - 1) / per_);
        next_ = 1;   // part 0 is the caller's
        left_ = parts_;
        ++gen_;
        lk.unlock();
        cv_.notify_all();
        fn(0, std::min(n, per_));
        lk.lock();
        --left_;
        for (;;) {   // the caller takes parts too while any are unclaimed
            if (next_ >= parts_) break;
            const unsigned i = next_++;
            lk.unlock();
            fn(i * per_, std::min(n, (i + 1) * per_));
            lk.lock();
            --left_;
        }
        done_.wait(lk, [this] { return left_ == 0; });
        fn_ = nullptr;
        return true;
    }

   private:
    void work() {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return gen_ != seen; });
            seen = gen_;
            while (fn_ && next_ < parts_) {
                const unsigned i = next_++;
                const auto* fn = fn_;
                const size_t lo = i * per_, hi = std::min(n_, (i + 1) * per_);
                lk.unlock();
                (*fn)(lo, hi);
                lk.lock();
                if (--left_ == 0) done_.notify_all();
            }
        }
    }
    std::mutex call_mu_, mu_;
    std::condition_variable cv_, done_;
    std::vector<std::thread> th_;
    const std::function<void(size_t, size_t)>* fn_ = nullptr;
    size_t n_ = 0, per_ = 0;
    unsigned parts_ = 0, next_ = 0, left_ = 0;
    uint64_t gen_ = 0;
};

// fn(lo, hi) over [0, n) on up to host_threads threads (knob, 8): the staging and scatter copies
// of FEC_HOST (one core copies ~10 GB/s, a fifth of PCIe), on CopyPool's persistent workers (r04j:
// +0.7 to +1.6 GiB/s pageable over threads made per call); a caller that finds them busy makes
// its own.
template <class F>
static void parallel_for(size_t n, F fn) {
    const unsigned T = std::min<unsigned>((unsigned)std::max(1, (int)fk::g_tune.host_threads),
                                          std::max(1u, std::thread::hardware_concurrency()));
    if (n < 512 || T == 1) {
        fn((size_t)0, n);
        return;
    }
    if (CopyPool::get().run(T, n, std::function<void(size_t, size_t)>(fn))) return;
    std::vector<std::thread> th;
    const size_t per = (n + T - 1) / T;
    for (size_t lo = 0; lo < n; lo += per) th.emplace_back(fn, lo, std::min(n, lo + per));
    for (auto& t : th) t.join();
}

static int grow_dev(uint8_t** p, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return FEC_OK;
    if (*p) HIP_TRY(hipFree(*p));
    *p = nullptr;
    *cap = 0;
    HIP_TRY(hipMalloc(p, bytes));
    *cap = bytes;
    return FEC_OK;
}

// Bytes of the caller's span of nb blocks (shards of len bytes, cols per block).
static size_t span_bytes(size_t nb, size_t cols, size_t bs, size_t ss, size_t len) {
    return (nb - 1) * bs + (cols - 1) * ss + len;
}

// A span worth one linear copy: at most a quarter more bytes than the shards themselves.
static bool dense_span(size_t nb, size_t cols, size_t bs, size_t ss, size_t len) {
    return span_bytes(nb, cols, bs, ss, len) * 4 <= nb * cols * len * 5;
}

// Caller's columns [0, cols) of nb blocks toward the device stage [nb][st_bs/st_ss], on stream
// `up`: when the span of all span_cols >= cols columns is dense, one linear DMA of it into `raw`
// (a few unneeded columns ride along: one linear DMA beats narrow 2D rows) and *repack = true (the
// kernel stream then runs pinned_repack); else one 2D DMA per column straight into the stage.
static int pinned_up(hipStream_t up, uint8_t* stage, size_t st_bs, size_t st_ss, const uint8_t* src, size_t bs,
                     size_t ss, size_t nb, size_t cols, size_t len, uint8_t* raw, size_t span_cols, bool* repack) {
    *repack = dense_span(nb, span_cols, bs, ss, len);
    if (*repack) {
        HIP_TRY(hipMemcpyAsync(raw, src, span_bytes(nb, span_cols, bs, ss, len), hipMemcpyHostToDevice, up));
        return FEC_OK;
    }
    for (size_t j = 0; j < cols; ++j)
        HIP_TRY(hipMemcpy2DAsync(stage + j * st_ss, st_bs, src + j * ss, bs, len, nb, hipMemcpyHostToDevice, up));
    return FEC_OK;
}

// The caller layout's outputs are packed (no bytes between shards): the kernel stream packs the
// device stage into one image that goes down in one linear DMA.
static bool packed_out(size_t bs, size_t ss, size_t cols, size_t len) { return ss == len && bs == cols * len; }

// Device stage [nb][st_bs/st_ss] columns back to the caller, on stream `down`: the packed image
// (packed_out) in one linear DMA, else one 2D DMA per column, which writes exactly len bytes per
// shard.
static int pinned_down(hipStream_t down, uint8_t* dst, size_t bs, size_t ss, const uint8_t* stage, size_t st_bs,
                       size_t st_ss, size_t nb, size_t cols, size_t len, const uint8_t* raw) {
    if (packed_out(bs, ss, cols, len)) {
        HIP_TRY(hipMemcpyAsync(dst, raw, nb * cols * len, hipMemcpyDeviceToHost, down));
        return FEC_OK;
    }
    for (size_t j = 0; j < cols; ++j)
        HIP_TRY(hipMemcpy2DAsync(dst + j * ss, bs, stage + j * st_ss, st_bs, len, nb, hipMemcpyDeviceToHost, down));
    return FEC_OK;
}

static int host_pipe_init(HostPipe& p) {
    if (p.up) return FEC_OK;
    for (hipStream_t* q : {&p.up, &p.comp, &p.down}) HIP_TRY(hipStreamCreateWithFlags(q, hipStreamNonBlocking));
    for (HostSet& s : p.set)
        for (hipEvent_t* e : {&s.up_done, &s.k_done, &s.down_done})
            HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return FEC_OK;
}

// Buffers of every set for chunks of in / out staged bytes and `blocks` blocks (a call grows them
// before its first chunk, when no chunk of the pipe is in flight).
static int host_pipe_grow(HostPipe& p, size_t in_bytes, size_t out_bytes, size_t blocks) {
    int rc;
    if ((rc = host_pipe_init(p))) return rc;
    for (HostSet& s : p.set) {
        if (in_bytes > s.in_cap) {
            if (s.h_in) HIP_TRY(hipHostFree(s.h_in));
            if (s.d_in) HIP_TRY(hipFree(s.d_in));
            s.h_in = s.d_in = nullptr;
            s.in_cap = 0;
            HIP_TRY(hipHostMalloc(&s.h_in, in_bytes, hipHostMallocDefault));
            HIP_TRY(hipMalloc(&s.d_in, in_bytes));
            s.in_cap = in_bytes;
        }
        if (out_bytes > s.out_cap) {
            if (s.h_out) HIP_TRY(hipHostFree(s.h_out));
            if (s.d_out) HIP_TRY(hipFree(s.d_out));
            s.h_out = s.d_out = nullptr;
            s.out_cap = 0;
            HIP_TRY(hipHostMalloc(&s.h_out, out_bytes, hipHostMallocDefault));
            HIP_TRY(hipMalloc(&s.d_out, out_bytes));
            s.out_cap = out_bytes;
        }
        if (blocks > s.blk_cap) {
            for (void* q : {(void*)s.h_masks, (void*)s.h_status})
                if (q) HIP_TRY(hipHostFree(q));
            for (void* q : {(void*)s.d_masks, (void*)s.d_status})
                if (q) HIP_TRY(hipFree(q));
            s.h_masks = s.d_masks = nullptr;
            s.h_status = s.d_status = nullptr;
            s.blk_cap = 0;
            HIP_TRY(hipHostMalloc(&s.h_masks, blocks * 4, hipHostMallocDefault));
            HIP_TRY(hipHostMalloc(&s.h_status, blocks * 4, hipHostMallocDefault));
            HIP_TRY(hipMalloc(&s.d_masks, blocks * 4));
            HIP_TRY(hipMalloc(&s.d_status, blocks * 4));
            s.blk_cap = blocks;
        }
    }
    return FEC_OK;
}

// Run `fn` with the ctx's kernels enqueued on the pipe's kernel stream, with its scratch.
template <class F>
static int on_pipe(fec_ctx* ctx, F fn) {
    hipStream_t keep = ctx->stream;
    Work* keep_w = ctx->work;
    ctx->stream = ctx->pipe.comp;
    ctx->work = &ctx->pipe.w;
    const int rc = fn();
    ctx->stream = keep;
    ctx->work = keep_w;
    return rc;
}

// One chunk of a host-path call: blocks [b0, b0 + nb) and what its stages decided.
struct HostChunk {
    size_t b0 = 0, nb = 0;
    bool live = false;
    bool repack = false;      // pinned: the data span came up raw, the kernel stream repacks it
    size_t planes = 0;        // reconstruct: parity planes [0, planes) reach the device
    uint32_t gather = 0;      // reconstruct, pinned: planes the device pulls itself (bit r)
    size_t slots = 1;         // reconstruct: output slots per block
};

// Chunks of `chunk` blocks through the pipe. up(s, ch): host staging, then the H2D copies on
// p.up; kern(s, ch): kernels on p.comp; down(s, ch): D2H copies on p.down; finish(s, ch) on the
// host once the chunk's copies have landed. On any failure every stream is drained before the
// error returns, so no set is left in flight.
template <class Up, class Kern, class Down, class Finish>
static int host_pipeline(fec_ctx* ctx, size_t nblocks, size_t chunk, Up up, Kern kern, Down down, Finish finish) {
    HostPipe& p = ctx->pipe;
    HostChunk pend[kHostSets];
    auto run = [&]() -> int {
        int rc;
        size_t c = 0;
        for (size_t b0 = 0; b0 < nblocks; b0 += chunk, ++c) {
            const int i = (int)(c % kHostSets);
            HostSet& s = p.set[i];
            if (pend[i].live) {   // the set's chunk kHostSets back: all of its buffers are free after this
                HIP_TRY(hipEventSynchronize(s.down_done));
                pend[i].live = false;
                if ((rc = finish(s, pend[i]))) return rc;
            }
            HostChunk ch;
            ch.b0 = b0;
            ch.nb = std::min(chunk, nblocks - b0);
            if ((rc = up(s, ch))) return rc;
            HIP_TRY(hipEventRecord(s.up_done, p.up));
            HIP_TRY(hipStreamWaitEvent(p.comp, s.up_done, 0));
            if ((rc = kern(s, ch))) return rc;
            HIP_TRY(hipEventRecord(s.k_done, p.comp));
            HIP_TRY(hipStreamWaitEvent(p.down, s.k_done, 0));
            if ((rc = down(s, ch))) return rc;
            HIP_TRY(hipEventRecord(s.down_done, p.down));
            ch.live = true;
            pend[i] = ch;
        }
        for (size_t t = 0; t < (size_t)kHostSets; ++t) {   // oldest chunk first
            const int i = (int)((c + t) % kHostSets);
            if (!pend[i].live) continue;
            HIP_TRY(hipEventSynchronize(p.set[i].down_done));
            pend[i].live = false;
            if ((rc = finish(p.set[i], pend[i]))) return rc;
        }
        return FEC_OK;
    };
    const int rc = run();
    if (rc) {
        for (hipStream_t q : {p.up, p.comp, p.down})
            if (q) (void)hipStreamSynchronize(q);
        (void)hipGetLastError();
    }
    return rc;
}

// Encode (RS when code != nullptr, else XOR(k, 1)): host data -> host parity.
static int host_encode(fec_ctx* ctx, Code* code, int k, int m, size_t len, size_t nblocks, const uint8_t* data,
                       size_t dbs, uint8_t* parity, size_t pbs, size_t ss, bool pinned) {
    const size_t ssd = round16(len);
    const size_t chunk = host_chunk_blocks(nblocks, (size_t)k * ssd);
    HostPipe& p = ctx->pipe;
    int rc;
    if ((rc = host_pipe_grow(p, chunk * k * ssd, chunk * m * ssd, 1))) return rc;
    const bool pack = pinned && packed_out(pbs, ss, (size_t)m, len);
    if (pinned)
        for (HostSet& s : p.set) {
            if ((rc = grow_dev(&s.d_raw_in, &s.raw_in_cap, span_bytes(chunk, k, dbs, ss, len) + 16))) return rc;
            if (pack && (rc = grow_dev(&s.d_raw_out, &s.raw_out_cap, chunk * m * len + 16))) return rc;
        }
    auto up = [&](HostSet& s, HostChunk& ch) -> int {
        if (pinned)
            return pinned_up(p.up, s.d_in, (size_t)k * ssd, ssd, data + ch.b0 * dbs, dbs, ss, ch.nb, k, len, s.d_raw_in,
                             k, &ch.repack);
        parallel_for(ch.nb, [&](size_t lo, size_t hi) {
            for (size_t b = lo; b < hi; ++b)
                for (int j = 0; j < k; ++j) memcpy(s.h_in + (b * k + j) * ssd, data + (ch.b0 + b) * dbs + j * ss, len);
        });
        HIP_TRY(hipMemcpyAsync(s.d_in, s.h_in, ch.nb * k * ssd, hipMemcpyHostToDevice, p.up));
        return FEC_OK;
    };
    auto kern = [&](HostSet& s, HostChunk& ch) -> int {
        if (ch.repack)
            HIP_TRY(fk::launch_span_to_stage(s.d_in, (size_t)k * ssd, ssd, s.d_raw_in, dbs, ss, (uint32_t)ch.nb,
                                             (uint32_t)k, (uint32_t)len, p.comp));
        const int r = on_pipe(ctx, [&] {
            return code ? rs_encode_device(ctx, code, len, ch.nb, s.d_in, (size_t)k * ssd, s.d_out, (size_t)m * ssd, ssd)
                        : xor_encode_device(ctx, k, len, ch.nb, s.d_in, (size_t)k * ssd, s.d_out, ssd, ssd);
        });
        if (r) return r;
        if (pack)
            HIP_TRY(fk::launch_stage_to_packed(s.d_raw_out, s.d_out, (size_t)m * ssd, ssd, (uint32_t)ch.nb,
                                               (uint32_t)m, (uint32_t)len, p.comp));
        return FEC_OK;
    };
    auto down = [&](HostSet& s, HostChunk& ch) -> int {
        if (pinned)
            return pinned_down(p.down, parity + ch.b0 * pbs, pbs, ss, s.d_out, (size_t)m * ssd, ssd, ch.nb, m, len,
                               s.d_raw_out);
        HIP_TRY(hipMemcpyAsync(s.h_out, s.d_out, ch.nb * m * ssd, hipMemcpyDeviceToHost, p.down));
        return FEC_OK;
    };
    auto finish = [&](HostSet& s, HostChunk& ch) -> int {
        if (!pinned)
            parallel_for(ch.nb, [&](size_t lo, size_t hi) {
                for (size_t b = lo; b < hi; ++b)
                    for (int r = 0; r < m; ++r)
                        memcpy(parity + (ch.b0 + b) * pbs + r * ss, s.h_out + (b * m + r) * ssd, len);
            });
        return FEC_OK;
    };
    return host_pipeline(ctx, nblocks, chunk, up, kern, down, finish);
}

// RS reconstruct, in place in the caller's data slots: per chunk, the data shards and the parity
// planes its blocks read go up (P = 1 + the highest parity index any block of the chunk reads
// among its first k present shards); the recover kernel rebuilds each block's erased data shards
// into [block][slot] outputs (slots = the chunk's largest erasure count); only those come down
// and are scattered into the erased slots. Pinned callers: a parity plane that at least 3/4 of
// the chunk's blocks read goes up by one 2D DMA (tools/zerocopy_probe.hip: 52 GB/s for a 1202-B
// row of every 4808 B); a sparser one is pulled by the device, plane by plane and block by block,
// straight from the caller's buffer (gather_planes_kernel), which moves only what is read but runs
// slower beside a D2H copy (pcie_duplex_probe: a kernel reading host memory and a D2H DMA at once
// make 29.9 GB/s each way).
static int host_reconstruct_rs(fec_ctx* ctx, Code* code, int k, int m, size_t len, size_t nblocks, uint8_t* data,
                               size_t dbs, const uint8_t* parity, size_t pbs, size_t ss, const uint32_t* masks,
                               int32_t* block_status, bool pinned) {
    const size_t ssd = round16(len);
    const size_t n = (size_t)k + m;
    const uint32_t all = fk::low_mask((uint32_t)n), kmask = fk::low_mask((uint32_t)k);
    const size_t maxe = (size_t)std::max(1, std::min(k, m));
    const size_t chunk = host_chunk_blocks(nblocks, n * ssd);
    HostPipe& p = ctx->pipe;
    int rc;
    if ((rc = host_pipe_grow(p, chunk * n * ssd, chunk * maxe * ssd, chunk))) return rc;
    if (pinned)
        for (HostSet& s : p.set)
            if ((rc = grow_dev(&s.d_raw_in, &s.raw_in_cap, span_bytes(chunk, k, dbs, ss, len) + 16))) return rc;
    // the sticky device word of the host path: statuses report every per-block failure, but a plan
    // kernel that cannot run (fec_plan.hip form 3's LDS-alignment guard, bit 4) writes no statuses
    HIP_TRY(hipMemsetAsync(ctx->d_err + 1, 0, sizeof(int), p.comp));
    bool failed = false;
    auto up = [&](HostSet& s, HostChunk& ch) -> int {
        const size_t nb = ch.nb, b0 = ch.b0;
        // per block: the parity planes its first k present shards reach, its erasure count
        uint32_t needers[32] = {};
        for (size_t b = 0; b < nb; ++b) {
            const uint32_t mask = masks[b0 + b] & all;
            s.h_masks[b] = mask;
            const uint32_t e = (uint32_t)k - (uint32_t)__builtin_popcount(mask & kmask);
            if (e == 0 || (uint32_t)__builtin_popcount(mask) < (uint32_t)k) continue;
            uint32_t need = e;   // parities among the first k present: the first e present ones
            for (int r = 0; r < m && need; ++r)
                if ((mask >> (k + r)) & 1u) {
                    --need;
                    ++needers[r];
                    ch.planes = std::max(ch.planes, (size_t)r + 1);
                }
            ch.slots = std::max(ch.slots, (size_t)e);
        }
        uint8_t* d_par = s.d_in + nb * k * ssd;   // parity planes [P][nb][ssd]
        HIP_TRY(hipMemcpyAsync(s.d_masks, s.h_masks, nb * 4, hipMemcpyHostToDevice, p.up));
        if (pinned) {
            if ((rc = pinned_up(p.up, s.d_in, (size_t)k * ssd, ssd, data + b0 * dbs, dbs, ss, nb, k, len, s.d_raw_in, k,
                                &ch.repack)))
                return rc;
            // the device reads sparse planes straight out of the caller's pinned buffer (needs a
            // device mapping of it; otherwise every plane goes by DMA)
            const uint8_t* dpar = nullptr;
            const bool mapped = ch.planes &&
                                hipHostGetDevicePointer((void**)&dpar, (void*)(parity + b0 * pbs), 0) == hipSuccess &&
                                dpar;
            if (ch.planes && !mapped) (void)hipGetLastError();
            for (size_t r = 0; r < ch.planes; ++r) {
                const bool sparse = needers[r] * 4 < nb * 3;
                if (mapped && sparse) {
                    ch.gather |= 1u << r;
                    continue;
                }
                HIP_TRY(hipMemcpy2DAsync(d_par + r * nb * ssd, ssd, parity + b0 * pbs + r * ss, pbs, len, nb,
                                         hipMemcpyHostToDevice, p.up));
            }
            return FEC_OK;
        }
        const size_t P = ch.planes;
        parallel_for(nb, [&](size_t lo, size_t hi) {
            for (size_t b = lo; b < hi; ++b) {
                const uint32_t mask = s.h_masks[b];
                if ((mask & kmask) == kmask) continue;   // nothing to rebuild: nothing read
                for (int j = 0; j < k; ++j)
                    if ((mask >> j) & 1u) memcpy(s.h_in + (b * k + j) * ssd, data + (b0 + b) * dbs + j * ss, len);
                for (size_t r = 0; r < P; ++r)
                    if ((mask >> (k + r)) & 1u)
                        memcpy(s.h_in + nb * k * ssd + (r * nb + b) * ssd, parity + (b0 + b) * pbs + r * ss, len);
            }
        });
        HIP_TRY(hipMemcpyAsync(s.d_in, s.h_in, (nb * k + P * nb) * ssd, hipMemcpyHostToDevice, p.up));
        return FEC_OK;
    };
    auto kern = [&](HostSet& s, HostChunk& ch) -> int {
        const size_t nb = ch.nb;
        uint8_t* d_par = s.d_in + nb * k * ssd;
        if (ch.repack)
            HIP_TRY(fk::launch_span_to_stage(s.d_in, (size_t)k * ssd, ssd, s.d_raw_in, dbs, ss, (uint32_t)nb,
                                             (uint32_t)k, (uint32_t)len, p.comp));
        if (ch.gather) {
            const uint8_t* dpar = nullptr;
            HIP_TRY(hipHostGetDevicePointer((void**)&dpar, (void*)(parity + ch.b0 * pbs), 0));
            HIP_TRY(fk::launch_gather_planes(dpar, pbs, ss, (uint32_t)len, s.d_masks, (uint32_t)nb, (uint32_t)ch.planes,
                                             ch.gather, (uint32_t)k, d_par, ssd, p.comp));
        }
        return on_pipe(ctx, [&] {
            return rs_reconstruct_device(ctx, code, len, nb, s.d_in, (size_t)k * ssd, d_par, ssd, ssd, s.d_masks,
                                         s.d_status, ctx->d_err + 1, s.d_out, ch.slots * ssd, (uint32_t)ch.slots,
                                         nb * ssd);
        });
    };
    auto down = [&](HostSet& s, HostChunk& ch) -> int {
        HIP_TRY(hipMemcpyAsync(s.h_out, s.d_out, ch.nb * ch.slots * ssd, hipMemcpyDeviceToHost, p.down));
        HIP_TRY(hipMemcpyAsync(s.h_status, s.d_status, ch.nb * 4, hipMemcpyDeviceToHost, p.down));
        return FEC_OK;
    };
    auto finish = [&](HostSet& s, HostChunk& ch) -> int {
        for (size_t b = 0; b < ch.nb; ++b) {
            const int32_t st = s.h_status[b];
            if (block_status) block_status[ch.b0 + b] = st < 0 ? st : 0;
            if (st < 0) failed = true;
        }
        parallel_for(ch.nb, [&](size_t lo, size_t hi) {
            for (size_t b = lo; b < hi; ++b) {
                const int32_t st = s.h_status[b];
                const uint32_t mask = s.h_masks[b];
                for (int j = 0, r = 0; j < k && r < st; ++j)
                    if (!((mask >> j) & 1u))
                        memcpy(data + (ch.b0 + b) * dbs + j * ss, s.h_out + (b * ch.slots + r++) * ssd, len);
            }
        });
        return FEC_OK;
    };
    if ((rc = host_pipeline(ctx, nblocks, chunk, up, kern, down, finish))) return rc;
    int err = 0;
    HIP_TRY(hipMemcpyAsync(&err, ctx->d_err + 1, sizeof(int), hipMemcpyDeviceToHost, p.comp));
    HIP_TRY(hipStreamSynchronize(p.comp));
    if (err & 4) return FEC_ERR_HIP;
    return failed ? FEC_ERR_TOO_FEW_SHARDS : FEC_OK;
}

// FEC_HOST XOR(k,1) reconstruct (the scheme mirror's per-block recovery): the present shards of
// each chunk as [block][k+1][ssd], rebuilt in place on the device, the data slots copied back.
static int host_reconstruct_xor(fec_ctx* ctx, int k, size_t len, size_t nblocks, uint8_t* data, size_t dbs,
                                const uint8_t* parity, size_t pbs, size_t ss, const uint32_t* masks,
                                int32_t* block_status) {
    const size_t ssd = round16(len);
    const size_t n = (size_t)k + 1;
    const uint32_t all = fk::low_mask((uint32_t)n), kmask = fk::low_mask((uint32_t)k);
    const size_t chunk = host_chunk_blocks(nblocks, n * ssd);
    int rc;
    if ((rc = grow_stage(ctx, chunk * n * ssd))) return rc;
    if ((rc = grow_masks(ctx, chunk))) return rc;
    HIP_TRY(hipMemsetAsync(ctx->d_err + 1, 0, sizeof(int), ctx->stream));
    std::vector<int32_t> st;
    for (size_t b0 = 0; b0 < nblocks; b0 += chunk) {
        const size_t nb = std::min(chunk, nblocks - b0);
        for (size_t b = 0; b < nb; ++b) {
            const uint32_t mask = masks[b0 + b] & all;
            if ((mask & kmask) == kmask) continue;
            for (size_t i = 0; i < n; ++i)
                if ((mask >> i) & 1u)
                    memcpy(ctx->h_stage + (b * n + i) * ssd,
                           i < (size_t)k ? data + (b0 + b) * dbs + i * ss : parity + (b0 + b) * pbs, len);
        }
        HIP_TRY(hipMemcpyAsync(ctx->d_masks, masks + b0, nb * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(ctx->d_stage, ctx->h_stage, nb * n * ssd, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = xor_reconstruct_device(ctx, k, len, nb, ctx->d_stage, n * ssd, ctx->d_stage + k * ssd, n * ssd, ssd,
                                         ctx->d_masks, ctx->d_status, ctx->d_err + 1)))
            return rc;
        st.resize(nb);
        HIP_TRY(hipMemcpyAsync(st.data(), ctx->d_status, nb * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(ctx->h_stage, ctx->d_stage, nb * n * ssd, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (size_t b = 0; b < nb; ++b) {
            if (block_status) block_status[b0 + b] = st[b];
            if (st[b] != 0) continue;
            const uint32_t mask = masks[b0 + b] & all;
            for (int i = 0; i < k; ++i)
                if (!((mask >> i) & 1u)) memcpy(data + (b0 + b) * dbs + i * ss, ctx->h_stage + (b * n + i) * ssd, len);
        }
    }
    int err = 0;
    HIP_TRY(hipMemcpy(&err, ctx->d_err + 1, sizeof(int), hipMemcpyDeviceToHost));
    return err ? FEC_ERR_TOO_FEW_SHARDS : FEC_OK;
}

// FEC_HOST wide RS reconstruct: the plain form (it exists so that the scheme layer decodes wide
// codes; it is PCIe-bound, and not pipelined). Each slice of blocks goes as [block][k+m][ssd]
// through the ctx's pinned and device stage, is rebuilt in place on the device, and the rebuilt
// data shards of the blocks that succeeded are copied back.
static int host_reconstruct_wide(fec_ctx* ctx, int k, int m, size_t len, size_t nblocks, uint8_t* data, size_t dbs,
                                 const uint8_t* parity, size_t pbs, size_t ss, const uint32_t* masks,
                                 size_t mask_words, int32_t* block_status) {
    const size_t ssd = round16(len);
    const size_t n = (size_t)k + m;
    const size_t chunk = host_chunk_blocks(nblocks, n * ssd);
    int rc;
    if ((rc = grow_stage(ctx, chunk * n * ssd))) return rc;
    if ((rc = grow_masks(ctx, chunk * mask_words))) return rc;
    HIP_TRY(hipMemsetAsync(ctx->d_err + 1, 0, sizeof(int), ctx->stream));
    auto present = [&](size_t b, size_t i) { return (masks[b * mask_words + i / 32] >> (i % 32)) & 1u; };
    std::vector<int32_t> st;
    bool failed = false;
    for (size_t b0 = 0; b0 < nblocks; b0 += chunk) {
        const size_t nb = std::min(chunk, nblocks - b0);
        for (size_t b = 0; b < nb; ++b)
            for (size_t i = 0; i < n; ++i)
                if (present(b0 + b, i))
                    memcpy(ctx->h_stage + (b * n + i) * ssd,
                           i < (size_t)k ? data + (b0 + b) * dbs + i * ss : parity + (b0 + b) * pbs + (i - k) * ss, len);
        HIP_TRY(hipMemcpyAsync(ctx->d_masks, masks + b0 * mask_words, nb * mask_words * 4, hipMemcpyHostToDevice,
                               ctx->stream));
        HIP_TRY(hipMemcpyAsync(ctx->d_stage, ctx->h_stage, nb * n * ssd, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = rs_reconstruct_wide_device(ctx, k, m, len, nb, ctx->d_stage, n * ssd, ctx->d_stage + k * ssd, n * ssd,
                                             ssd, ctx->d_masks, mask_words, ctx->d_status, ctx->d_err + 1)))
            return rc;
        st.resize(nb);
        HIP_TRY(hipMemcpyAsync(st.data(), ctx->d_status, nb * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(ctx->h_stage, ctx->d_stage, nb * n * ssd, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (size_t b = 0; b < nb; ++b) {
            if (block_status) block_status[b0 + b] = st[b];
            if (st[b] != 0) {
                failed = true;
                continue;
            }
            for (size_t i = 0; i < (size_t)k; ++i)
                if (!present(b0 + b, i)) memcpy(data + (b0 + b) * dbs + i * ss, ctx->h_stage + (b * n + i) * ssd, len);
        }
    }
    return failed ? FEC_ERR_TOO_FEW_SHARDS : FEC_OK;
}

// ---------------------------------------------------------------- C ABI

extern "C" {

const char* fec_version(void) { return "0xfec-mi355x 0.1.0 (gfx950)"; }

const char* fec_strerror(int code) {
    switch (code) {
        case FEC_OK: return "ok";
        case FEC_ERR_INVALID_ARG: return "invalid argument";
        case FEC_ERR_INV_SHARD_NUM: return "cannot create Encoder with less than one data shard or less than zero parity shards";
        case FEC_ERR_MAX_SHARD_NUM: return "cannot create Encoder with more than 256 data+parity shards";
        case FEC_ERR_TOO_FEW_SHARDS: return "too few shards given";
        case FEC_ERR_SHARD_SIZE: return "shard sizes do not match";
        case FEC_ERR_SHARD_NO_DATA: return "no shard data";
        case FEC_ERR_ALIGNMENT: return "device shard layout must be 16-byte aligned";
        case FEC_ERR_HIP: return "HIP runtime error";
        case FEC_ERR_NOMEM: return "out of memory";
        case FEC_ERR_NO_DEVICE: return "no HIP device";
        case -21: return "EOF";   // FEC_ERR_EOF (fec_wire.h): io.EOF
        default: return "unknown error";
    }
}

int fec_device_count(int* count) {
    if (!count) return FEC_ERR_INVALID_ARG;
    *count = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return FEC_ERR_NO_DEVICE;
    }
    *count = n;
    return n > 0 ? FEC_OK : FEC_ERR_NO_DEVICE;
}

int fec_ctx_create(int device, fec_ctx** out) {
    if (!out) return FEC_ERR_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return FEC_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) return FEC_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(device));
    fec_ctx* ctx = new fec_ctx();
    ctx->device = device;
    if (hipStreamCreateWithFlags(&ctx->own, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&ctx->d_err, 2 * sizeof(int)) != hipSuccess ||
        hipMemset(ctx->d_err, 0, 2 * sizeof(int)) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {   // null-stream memsets done before any ctx stream runs
        (void)hipGetLastError();
        fec_ctx_destroy(ctx);
        return FEC_ERR_HIP;
    }
    ctx->stream = ctx->own;
    {   // LDS a workgroup may use (160 KiB on gfx950): bounds the wave-form rebuild's slices
        int lds = 0;
        if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && lds > 0)
            fk::g_max_lds = (size_t)lds;
    }
    *out = ctx;
    return FEC_OK;
}

void fec_ctx_destroy(fec_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (auto& kv : ctx->codes) {
        if (kv.second.d_prows) (void)hipFree(kv.second.d_prows);
        if (kv.second.d_tabs) (void)hipFree(kv.second.d_tabs);
        if (kv.second.d_dytabs) (void)hipFree(kv.second.d_dytabs);
        if (kv.second.d_single) (void)hipFree(kv.second.d_single);
        if (kv.second.d_single_coef) (void)hipFree(kv.second.d_single_coef);
        if (kv.second.d_dall) (void)hipFree(kv.second.d_dall);
    }
    if (ctx->own) (void)hipStreamSynchronize(ctx->own);
    if (ctx->stream && ctx->stream != ctx->own) (void)hipStreamSynchronize(ctx->stream);
    ctx->main.release();
    if (ctx->d_err) (void)hipFree(ctx->d_err);
    if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
    if (ctx->d_stage) (void)hipFree(ctx->d_stage);
    if (ctx->d_masks) (void)hipFree(ctx->d_masks);
    if (ctx->d_status) (void)hipFree(ctx->d_status);
    HostPipe& p = ctx->pipe;
    for (hipStream_t q : {p.up, p.comp, p.down})
        if (q) (void)hipStreamSynchronize(q);
    for (HostSet& s : p.set) {
        for (void* q : {(void*)s.h_in, (void*)s.h_out, (void*)s.h_masks, (void*)s.h_status})
            if (q) (void)hipHostFree(q);
        for (void* q : {(void*)s.d_in, (void*)s.d_out, (void*)s.d_masks, (void*)s.d_status, (void*)s.d_raw_in,
                        (void*)s.d_raw_out})
            if (q) (void)hipFree(q);
        for (hipEvent_t e : {s.up_done, s.k_done, s.down_done})
            if (e) (void)hipEventDestroy(e);
    }
    p.w.release();
    for (hipStream_t q : {p.up, p.comp, p.down})
        if (q) (void)hipStreamDestroy(q);
    if (ctx->handoff) (void)hipEventDestroy(ctx->handoff);
    if (ctx->own) (void)hipStreamDestroy(ctx->own);
    (void)hipGetLastError();
    delete ctx;
}

// Switch the ctx to `next`. The ctx's own / caller's stream share one workspace (`main`: plan
// records), so work already queued on the old
// stream must finish before anything on the new one touches it: the new stream waits on an
// event recorded on the old one (no host wait). grow_* then sync only the current stream,
// which by this wait covers the old one's kernels too.
static int switch_stream(fec_ctx* ctx, hipStream_t next) {
    if (next == ctx->stream) return FEC_OK;
    int rc = select_device(ctx);
    if (rc) return rc;
    if (!ctx->handoff) HIP_TRY(hipEventCreateWithFlags(&ctx->handoff, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ctx->handoff, ctx->stream));
    HIP_TRY(hipStreamWaitEvent(next, ctx->handoff, 0));
    ctx->stream = next;
    return FEC_OK;
}

int fec_ctx_release_staging(fec_ctx* ctx) {
    int rc = select_device(ctx);
    if (rc) return rc;
    HostPipe& p = ctx->pipe;
    for (hipStream_t q : {p.up, p.comp, p.down})
        if (q) HIP_TRY(hipStreamSynchronize(q));
    if (ctx->stream) HIP_TRY(hipStreamSynchronize(ctx->stream));
    // Every buffer is freed and forgotten even when a free fails (the first failure is returned),
    // so the ctx never keeps a pointer it has handed back.
    hipError_t first = hipSuccess;
    auto drop = [&first](hipError_t e) {
        if (e != hipSuccess && first == hipSuccess) first = e;
    };
    for (HostSet& s : p.set) {
        for (void* q : {(void*)s.h_in, (void*)s.h_out, (void*)s.h_masks, (void*)s.h_status})
            if (q) drop(hipHostFree(q));
        for (void* q : {(void*)s.d_in, (void*)s.d_out, (void*)s.d_masks, (void*)s.d_status, (void*)s.d_raw_in,
                        (void*)s.d_raw_out})
            if (q) drop(hipFree(q));
        s.h_in = s.h_out = s.d_in = s.d_out = s.d_raw_in = s.d_raw_out = nullptr;
        s.h_masks = s.d_masks = nullptr;
        s.h_status = s.d_status = nullptr;
        s.in_cap = s.out_cap = s.blk_cap = s.raw_in_cap = s.raw_out_cap = 0;
    }
    if (ctx->h_stage) drop(hipHostFree(ctx->h_stage));
    if (ctx->d_stage) drop(hipFree(ctx->d_stage));
    ctx->h_stage = ctx->d_stage = nullptr;
    ctx->stage_cap = 0;
    if (first != hipSuccess) {
        (void)hipGetLastError();
        return FEC_ERR_HIP;
    }
    return FEC_OK;
}

int fec_ctx_set_stream(fec_ctx* ctx, void* hip_stream) {
    if (!ctx) return FEC_ERR_INVALID_ARG;
    return switch_stream(ctx, (hipStream_t)hip_stream);
}

// Internal, test-only tuning entry point (not part of the public ABI): knob `key` of fk::Tuning
// (fec_kernels.hpp, keys 0..kTuningKeys-1 in declaration order) set to `value`, process-wide, for
// every ctx. Tests and tools set knobs while no other thread submits work. Returns the previous
// value, or FEC_ERR_INVALID_ARG for an unknown key.
int fec__set_tuning(fec_ctx* ctx, int key, int value) {
    if (!ctx) return FEC_ERR_INVALID_ARG;
    fk::Tuning& t = fk::g_tune;
    std::atomic<int>* slots[fk::kTuningKeys] = {&t.enc_wpc,   &t.gen_wpc,    &t.dec_wpc,      &t.dir_wpc,
                                                &t.enc_bwpc,  &t.enc_fixed,  &t.dec_wave,     &t.dec_direct,
                                                &t.host_chunk, &t.host_threads, &t.bat_zc,     &t.dec_route,
                                                &t.st_pol,     &t.dst_pol,    &t.route_wpc,
                                                &t.route_ww,   &t.xor_wpc,
                                                &t.enc_ww,     &t.rag_g};
    if (key < 0 || key >= fk::kTuningKeys) return FEC_ERR_INVALID_ARG;
    return slots[key]->exchange(value);
}

// Internal self-test (not part of the public ABI, no device needed): parallel_for covers [0, n)
// exactly once, for sizes around the part boundaries and part counts 2..16, with four threads
// calling at once (one holds the persistent copy workers, the others find them busy and make
// their own threads). 0 on success, else the failing case.
extern "C" int fec__selftest_copypool(void) {
    const int saved = fk::g_tune.host_threads;
    int fail = 0;
    const size_t sizes[] = {511, 512, 513, 1000, 4097, 65536, 100003};
    for (int T : {2, 3, 8, 16}) {
        fk::g_tune.host_threads = T;
        std::vector<std::thread> callers;
        std::vector<int> bad(4, 0);
        for (int t = 0; t < 4; ++t)
            callers.emplace_back([&, t] {
                for (size_t n : sizes) {
                    std::unique_ptr<std::atomic<uint32_t>[]> hits(new std::atomic<uint32_t>[n]);
                    for (size_t i = 0; i < n; ++i) hits[i].store(0);
                    parallel_for(n, [&](size_t lo, size_t hi) {
                        for (size_t i = lo; i < hi; ++i) hits[i].fetch_add(1);
                    });
                    for (size_t i = 0; i < n; ++i)
                        if (hits[i].load() != 1) bad[t] = 1;
                }
            });
        for (auto& th : callers) th.join();
        for (int b : bad)
            if (b) fail = 100 + T;
        if (fail) break;
    }
    fk::g_tune.host_threads = saved;
    return fail;
}

// Internal self-test (not part of the public ABI, no device needed): the lane-arithmetic PermTab
// builder the kernels use equals the byte-wise one for every coefficient. 0 on success, else
// 1 + the first failing coefficient.
int fec__selftest_permtab(void) {
    for (uint32_t c = 0; c < 256; ++c) {
        const gf::PermTab a = gf::make_permtab((uint8_t)c), b = gf::make_permtab_fast(c);
        if (a.t0lo != b.t0lo || a.t0hi != b.t0hi || a.t1lo != b.t1lo || a.t1hi != b.t1hi || a.t2 != b.t2)
            return 1 + (int)c;
    }
    return 0;
}

// Internal self-test (not part of the public ABI, no device needed): the store policy of a call
// follows the hulls of its shard regions (fec_kernels.hpp regions_apart) for block-major and
// shard-major layouts. Addresses are only compared, never dereferenced. 0 on success, else
// 1 + the index of the first failing row.
int fec__selftest_store_policy(void) {
    const uint64_t S = 1216, L = 1202, B = 67, k = 8, m = 4;
    const uintptr_t base = 0x10000000;
    auto at = [&](uint64_t off) { return (const void*)(base + off); };
    struct Row {
        int st_pol;
        fk::ShardRegion data, parity;
        uint64_t nblocks;
        uint32_t want;
    };
    const Row rows[] = {
        // split, block-major [B][k][S] + [B][m][S]: apart (parity above data, and below it)
        {1, {at(0), k * S, S, k}, {at(B * k * S), m * S, S, m}, B, 1u},
        {1, {at(B * m * S), k * S, S, k}, {at(0), m * S, S, m}, B, 1u},
        // (those two touch); one 16-byte chunk into each other
        {1, {at(0), k * S, S, k}, {at(B * k * S - 16), m * S, S, m}, B, 0u},
        // interleaved [B][k+m][S]: parity slots among the data
        {1, {at(0), (k + m) * S, S, k}, {at(k * S), (k + m) * S, S, m}, B, 0u},
        // one block of it: its parity lies past its data
        {1, {at(0), (k + m) * S, S, k}, {at(k * S), (k + m) * S, S, m}, 1, 1u},
        // shard-major [k+m][B][S] in one region: parity rows after the last data row
        {1, {at(0), S, B * S, k}, {at(k * B * S), S, B * S, m}, B, 1u},
        // shard-major, parity rows in the gaps between the data rows
        {1, {at(0), S, 2 * B * S, k}, {at(B * S), S, 2 * B * S, m}, B, 0u},
        // shard-major data, block-major parity inside the data's second row
        {1, {at(0), S, B * S, k}, {at(B * S), m * S, S, m}, 8, 0u},
        // no blocks: nothing to claim
        {1, {at(0), k * S, S, k}, {at(B * k * S), m * S, S, m}, 0, 0u},
        // knob values: 0 nt whatever the layout, 2 sc1 whatever the layout
        {0, {at(0), k * S, S, k}, {at(B * k * S), m * S, S, m}, B, 0u},
        {2, {at(0), (k + m) * S, S, k}, {at(k * S), (k + m) * S, S, m}, B, 1u},
        {2, {at(0), k * S, S, k}, {at(B * k * S), m * S, S, m}, 0, 1u},
    };
    int i = 0;
    for (const Row& r : rows) {
        ++i;
        if (fk::encode_store_policy(r.st_pol, r.data, r.parity, L, r.nblocks) != r.want) return i;
        // symmetric in its two regions
        if (fk::encode_store_policy(r.st_pol, r.parity, r.data, L, r.nblocks) != r.want) return i;
    }
    // decode: nt sc1 (3) only into an out region apart from both the data and the parity read
    const fk::ShardRegion d{at(0), S, B * S, k}, p{at(k * B * S), S, B * S, m};
    const fk::ShardRegion out_far{at((k + m) * B * S), S, B * S, m}, out_in_parity{at((k + 1) * B * S), S, B * S, 1};
    const fk::ShardRegion out_rows_over_data{at(B * S - 16 * S), 16 * S, S, m}, none{nullptr, 0, 0, 0};
    if (fk::decode_store_policy(3, d, p, out_far, L, B) != 3u) return 101;
    if (fk::decode_store_policy(3, d, p, out_in_parity, L, B) != 0u) return 102;
    if (fk::decode_store_policy(3, d, p, out_rows_over_data, L, B) != 0u) return 103;
    if (fk::decode_store_policy(3, d, p, none, L, B) != 0u) return 104;       // in place
    if (fk::decode_store_policy(0, d, p, out_far, L, B) != 0u) return 105;    // knob: nt
    if (fk::decode_store_policy(3, d, p, out_far, L, 0) != 0u) return 106;
    return 0;
}

int fec_ctx_reset_stream(fec_ctx* ctx) {
    if (!ctx) return FEC_ERR_INVALID_ARG;
    return switch_stream(ctx, ctx->own);
}

void* fec_ctx_stream(fec_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int fec_sync(fec_ctx* ctx) {
    int rc = select_device(ctx);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    int err = 0;
    HIP_TRY(hipMemcpy(&err, ctx->d_err, sizeof(int), hipMemcpyDeviceToHost));
    if (err) {
        HIP_TRY(hipMemsetAsync(ctx->d_err, 0, sizeof(int), ctx->stream));
        // 1: a block with too few shards; 2: more erasures than output slots; 4: internal (the
        // form-3 plan kernel's LDS-alignment guard); 8: a ragged call met a block longer than its
        // max_shard_len
        return (err & 1)   ? FEC_ERR_TOO_FEW_SHARDS
               : (err & 4) ? FEC_ERR_HIP
               : (err & 2) ? FEC_ERR_INVALID_ARG
                           : FEC_ERR_SHARD_SIZE;
    }
    return FEC_OK;
}

int fec_rs_matrix(int k, int m, uint8_t* out) {
    if (!out) return FEC_ERR_INVALID_ARG;
    if (k <= 0 || m < 0) return FEC_ERR_INV_SHARD_NUM;
    if (k + m > 256) return FEC_ERR_MAX_SHARD_NUM;
    std::vector<uint8_t> mat = rs::build_matrix(k, k + m);
    if (mat.empty()) return FEC_ERR_INV_SHARD_NUM;
    memcpy(out, mat.data(), mat.size());
    return FEC_OK;
}

int fec_rs_prepare(fec_ctx* ctx, int k, int m) {
    int rc = select_device(ctx);
    if (rc) return rc;
    Code* code = nullptr;
    return get_code(ctx, k, m, &code);
}

// The argument checks every batch call makes before it runs, in the documented order (fec_hip.h):
// shard counts, flags, shard_len, out_slots and mask_words; then the ctx and the code; an empty
// call; null pointers; and for FEC_DEVICE the layout of the data, parity and out regions, in that
// order, then the alignment of the word arrays. An entry point describes itself in a Call and gets
// kRun back when it has work to do, else the code to return.
struct Call {
    int k, m, max_n;           // max_n: the call's largest k + m (the XOR calls: m = 1)
    bool host_ok;              // FEC_HOST / FEC_HOST_PINNED accepted
    int flags;
    size_t len, nblocks;
    const uint8_t* data;
    size_t dbs;
    const uint8_t** parity;    // m == 0: set to data (never read: no parity slot exists)
    size_t pbs, ss;
    bool rs = true;            // the code's tables are needed (not for XOR)
    bool encode = false;       // m == 0 leaves nothing to do
    bool null_arg = false;     // some further pointer the call needs is null
    bool has_out = false;      // recover calls: the out region and its slot count (the update call: its
                               // third region, the old data)
    const uint8_t* out = nullptr;
    size_t obs = 0;
    int out_slots = 1;
    bool wide = false;         // wide calls: words per present mask
    size_t mask_words = 1;
    int mask_n = 0;            // the shards a mask covers (0: k + m; the update calls' column masks: k)
    struct {
        const void *a, *b;
    } words[2] = {};           // (mask, status)-like pairs of 4-byte arrays, either may be null
};
constexpr int kRun = 1;

static int check_call(fec_ctx* ctx, const Call& c, Code** code) {
    if (c.k <= 0 || c.m < 0) return FEC_ERR_INV_SHARD_NUM;
    if (c.k + c.m > c.max_n) return FEC_ERR_MAX_SHARD_NUM;
    if (c.flags != FEC_DEVICE && !(c.host_ok && (c.flags == FEC_HOST || c.flags == FEC_HOST_PINNED)))
        return FEC_ERR_INVALID_ARG;
    if (c.len == 0) return FEC_ERR_SHARD_NO_DATA;
    if (c.len > (size_t(1) << 30) || c.out_slots <= 0) return FEC_ERR_INVALID_ARG;
    if (c.wide && (c.mask_words < (size_t)FEC_MASK_WORDS(c.mask_n ? c.mask_n : c.k + c.m) || c.mask_words > 8))
        return FEC_ERR_INVALID_ARG;
    int rc = select_device(ctx);
    if (rc) return rc;
    if (c.rs && (rc = get_code(ctx, c.k, c.m, code))) return rc;
    if (c.nblocks == 0 || (c.encode && c.m == 0)) return FEC_OK;
    if (!c.data || c.null_arg || (c.m > 0 && !*c.parity)) return FEC_ERR_INVALID_ARG;
    if (c.m == 0) *c.parity = c.data;
    if (c.flags != FEC_DEVICE) return kRun;
    if ((rc = check_device_layout(c.data, c.dbs, c.ss, c.len))) return rc;
    if ((rc = check_device_layout(*c.parity, c.pbs, c.ss, c.len))) return rc;
    if (c.has_out && (rc = check_device_layout(c.out, c.obs, c.ss, c.len))) return rc;
    for (const auto& w : c.words)
        if ((rc = check_device_words(w.a, w.b))) return rc;
    return kRun;
}

int fec_rs_encode_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, const uint8_t* data,
                        size_t data_block_stride, uint8_t* parity, size_t parity_block_stride,
                        size_t shard_stride, int flags) {
    const uint8_t* par = parity;
    Call c{k, m, 256, true, flags, shard_len, nblocks, data, data_block_stride, &par, parity_block_stride, shard_stride};
    c.encode = true;
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    if (flags == FEC_DEVICE)
        return rs_encode_device(ctx, code, shard_len, nblocks, data, data_block_stride, parity,
                                parity_block_stride, shard_stride);
    return host_encode(ctx, code, k, m, shard_len, nblocks, data, data_block_stride, parity, parity_block_stride,
                       shard_stride, flags == FEC_HOST_PINNED);
}

int fec_rs_reconstruct_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, uint8_t* data,
                             size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                             size_t shard_stride, const uint32_t* present_mask, int32_t* block_status, int flags) {
    Call c{k, m, FEC_MAX_DECODE_SHARDS, true, flags, shard_len, nblocks, data, data_block_stride, &parity,
           parity_block_stride, shard_stride};
    c.null_arg = !present_mask;
    c.words[0] = {present_mask, block_status};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    if (flags == FEC_DEVICE)
        return rs_reconstruct_device(ctx, code, shard_len, nblocks, data, data_block_stride, parity,
                                     parity_block_stride, shard_stride, present_mask, block_status, ctx->d_err);
    return host_reconstruct_rs(ctx, code, k, m, shard_len, nblocks, data, data_block_stride, parity,
                               parity_block_stride, shard_stride, present_mask, block_status, flags == FEC_HOST_PINNED);
}

int fec_rs_recover_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, const uint8_t* data,
                         size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                         size_t shard_stride, const uint32_t* present_mask, uint8_t* out, size_t out_block_stride,
                         int out_slots, int32_t* block_status, int flags) {
    Call c{k, m, FEC_MAX_DECODE_SHARDS, false, flags, shard_len, nblocks, data, data_block_stride, &parity,
           parity_block_stride, shard_stride};
    c.null_arg = !present_mask || !out;
    c.has_out = true, c.out = out, c.obs = out_block_stride, c.out_slots = out_slots;
    c.words[0] = {present_mask, block_status};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_reconstruct_device(ctx, code, shard_len, nblocks, const_cast<uint8_t*>(data), data_block_stride,
                                 parity, parity_block_stride, shard_stride, present_mask, block_status, ctx->d_err,
                                 out, out_block_stride, (uint32_t)out_slots);
}

// The wide calls with one mask word and a narrow code are the narrow calls, bytes and errors
// unchanged (which make the same checks: one word is enough for k + m <= 32).
int fec_rs_reconstruct_wide_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, uint8_t* data,
                                  size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                                  size_t shard_stride, const uint32_t* present_mask, size_t mask_words,
                                  int32_t* block_status, int flags) {
    if (k + m <= FEC_MAX_DECODE_SHARDS && mask_words == 1)
        return fec_rs_reconstruct_batch(ctx, k, m, shard_len, nblocks, data, data_block_stride, parity,
                                        parity_block_stride, shard_stride, present_mask, block_status, flags);
    Call c{k, m, FEC_MAX_WIDE_SHARDS, true, flags, shard_len, nblocks, data, data_block_stride, &parity,
           parity_block_stride, shard_stride};
    c.null_arg = !present_mask;
    c.wide = true, c.mask_words = mask_words;
    c.words[0] = {present_mask, block_status};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    if (flags == FEC_DEVICE)
        return rs_reconstruct_wide_device(ctx, k, m, shard_len, nblocks, data, data_block_stride, parity,
                                          parity_block_stride, shard_stride, present_mask, mask_words, block_status,
                                          ctx->d_err);
    return host_reconstruct_wide(ctx, k, m, shard_len, nblocks, data, data_block_stride, parity, parity_block_stride,
                                 shard_stride, present_mask, mask_words, block_status);
}

int fec_rs_recover_wide_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, const uint8_t* data,
                              size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                              size_t shard_stride, const uint32_t* present_mask, size_t mask_words, uint8_t* out,
                              size_t out_block_stride, int out_slots, int32_t* block_status, int flags) {
    if (k + m <= FEC_MAX_DECODE_SHARDS && mask_words == 1)
        return fec_rs_recover_batch(ctx, k, m, shard_len, nblocks, data, data_block_stride, parity,
                                    parity_block_stride, shard_stride, present_mask, out, out_block_stride, out_slots,
                                    block_status, flags);
    Call c{k, m, FEC_MAX_WIDE_SHARDS, false, flags, shard_len, nblocks, data, data_block_stride, &parity,
           parity_block_stride, shard_stride};
    c.null_arg = !present_mask || !out;
    c.has_out = true, c.out = out, c.obs = out_block_stride, c.out_slots = out_slots;
    c.wide = true, c.mask_words = mask_words;
    c.words[0] = {present_mask, block_status};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_reconstruct_wide_device(ctx, k, m, shard_len, nblocks, const_cast<uint8_t*>(data), data_block_stride,
                                      parity, parity_block_stride, shard_stride, present_mask, mask_words,
                                      block_status, ctx->d_err, out, out_block_stride, (uint32_t)out_slots);
}

// ---------------------------------------------------------------- verify, reconstruct-some
int fec_rs_verify_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, const uint8_t* data,
                        size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                        size_t shard_stride, int32_t* block_status, uint32_t* mismatch_count, int flags) {
    Call c{k, m, 256, false, flags, shard_len, nblocks, data, data_block_stride, &parity, parity_block_stride,
           shard_stride};
    c.null_arg = !block_status;
    c.words[0] = {mismatch_count, block_status};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_verify_device(ctx, code, shard_len, nblocks, data, data_block_stride, parity, parity_block_stride,
                            shard_stride, block_status, mismatch_count);
}

int fec_rs_reconstruct_some_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, uint8_t* data,
                                  size_t data_block_stride, uint8_t* parity, size_t parity_block_stride,
                                  size_t shard_stride, const uint32_t* present_mask, const uint32_t* want_mask,
                                  int32_t* block_status, int flags) {
    const uint8_t* par = parity;   // (m == 0: neither read nor written)
    Call c{k, m, FEC_MAX_DECODE_SHARDS, false, flags, shard_len, nblocks, data, data_block_stride, &par,
           parity_block_stride, shard_stride};
    c.null_arg = !present_mask;
    c.words[0] = {present_mask, block_status};
    c.words[1] = {want_mask, nullptr};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_reconstruct_some_device(ctx, k, m, shard_len, nblocks, data, data_block_stride,
                                      const_cast<uint8_t*>(par), parity_block_stride, shard_stride, present_mask,
                                      want_mask, block_status, ctx->d_err);
}

// ---------------------------------------------------------------- update, encode-idx
// The two calls differ in the old region alone. The Call's data region is the data folded in (the
// new version), its out region the old version: the layouts are checked in the order new data,
// parity, old data.
static int rs_update_call(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, bool has_old,
                          const uint8_t* old_data, size_t old_block_stride, const uint8_t* data,
                          size_t data_block_stride, uint8_t* parity, size_t parity_block_stride, size_t shard_stride,
                          const uint32_t* mask, size_t mask_words, int flags) {
    const uint8_t* par = parity;
    Call c{k, m, 256, false, flags, shard_len, nblocks, data, data_block_stride, &par, parity_block_stride,
           shard_stride};
    c.encode = true;
    c.null_arg = !mask || (has_old && !old_data);
    if (has_old) c.has_out = true, c.out = old_data, c.obs = old_block_stride;
    c.wide = true, c.mask_words = mask_words, c.mask_n = k;
    c.words[0] = {mask, nullptr};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_update_device(ctx, code, shard_len, nblocks,
                            {data, data_block_stride, has_old ? old_data : nullptr, old_block_stride, parity,
                             parity_block_stride, shard_stride, mask, mask_words});
}

int fec_rs_update_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, const uint8_t* old_data,
                        size_t old_block_stride, const uint8_t* new_data, size_t new_block_stride, uint8_t* parity,
                        size_t parity_block_stride, size_t shard_stride, const uint32_t* changed_mask,
                        size_t mask_words, int flags) {
    return rs_update_call(ctx, k, m, shard_len, nblocks, true, old_data, old_block_stride, new_data, new_block_stride,
                          parity, parity_block_stride, shard_stride, changed_mask, mask_words, flags);
}

int fec_rs_encode_idx_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, const uint8_t* data,
                            size_t data_block_stride, uint8_t* parity, size_t parity_block_stride,
                            size_t shard_stride, const uint32_t* idx_mask, size_t mask_words, int flags) {
    return rs_update_call(ctx, k, m, shard_len, nblocks, false, nullptr, 0, data, data_block_stride, parity,
                          parity_block_stride, shard_stride, idx_mask, mask_words, flags);
}

// Internal self-test (not part of the public ABI, no device needed): the launches of an update call
// that the launch limit cuts. k = 5, m = 20, 70 000-byte shards (4375 chunks), one block more than
// kMaxItems / 4375: two launches (490 853 blocks, then one) of two row passes each (16 rows, then
// 4). Every launch's three region bases, mask pointer, item count, row count and table base are
// compared with values worked out here from the call's strides, without the functions under test.
// 0 on success, else 10 * (launch index + 1) + the failing field.
int fec__selftest_update_slices(void) {
    const int k = 5, m = 20;
    const size_t L = 70000, cps = 4375, per = 490853, B = per + 1, W = 3;
    if (per != (size_t)(kMaxItems / cps)) return 1;
    const size_t ss = 70016, in_bs = k * ss + 48, old_bs = k * ss + 16, pbs = m * ss + 32;
    const uintptr_t in0 = uintptr_t(1) << 40, old0 = uintptr_t(2) << 40, par0 = uintptr_t(3) << 40,
                    mask0 = uintptr_t(4) << 40, tab0 = uintptr_t(5) << 40;
    Code code;
    code.k = k;
    code.m = m;
    code.d_tabs = (uint32_t*)tab0;
    const UpdateCall u{(const uint8_t*)in0, in_bs, (const uint8_t*)old0, old_bs, (uint8_t*)par0, pbs, ss,
                       (const uint32_t*)mask0, W};
    std::vector<fk::UpdateArgs> got;
    const int rc = update_launches(&code, L, B, u, [&](const fk::UpdateArgs& a) -> int {
        got.push_back(a);
        return FEC_OK;
    });
    code.d_tabs = nullptr;
    if (rc != FEC_OK || got.size() != 4) return 2;
    for (size_t i = 0; i < 4; ++i) {
        const fk::UpdateArgs& a = got[i];
        const int fail = 10 * ((int)i + 1);
        const size_t b0 = (i / 2) * per, nb = i / 2 ? 1 : per, r0 = (i % 2) * 16;
        if ((uintptr_t)a.in != in0 + b0 * in_bs || a.in_bs != in_bs) return fail + 1;
        if ((uintptr_t)a.old != old0 + b0 * old_bs || a.old_bs != old_bs) return fail + 2;
        if ((uintptr_t)a.par != par0 + b0 * pbs + r0 * ss || a.par_bs != pbs || a.ss != ss) return fail + 3;
        if ((uintptr_t)a.masks != mask0 + b0 * W * 4 || a.mask_words != W) return fail + 4;
        if (a.total != nb * cps || a.nblocks != nb || a.cps != cps || a.len != L) return fail + 5;
        if (a.k != (uint32_t)k || a.m != (i % 2 ? 4u : 16u)) return fail + 6;
        if ((uintptr_t)a.tabs != tab0 + r0 * k * 8 * 4) return fail + 7;
        if (a.div_cps.d != cps) return fail + 8;
    }
    // encode-idx: no old region in any launch
    UpdateCall e = u;
    e.old = nullptr;
    fk::UpdateArgs a{};
    code.d_tabs = (uint32_t*)tab0;
    fill_update_launch(a, &code, 16, per, 1, L, e);
    code.d_tabs = nullptr;
    if (a.old != nullptr || (uintptr_t)a.in != in0 + per * in_bs) return 3;
    return 0;
}

// Internal self-test (not part of the public ABI, no device needed): the records some_plan_record
// builds (fec_some.hpp, the function rs_plan_some_kernel runs) against the systematic matrix. For
// 64 seeded recoverable masks per code, plus all parity lost and, where m >= k, exactly k present
// with all of them parity: want = every shard; the inputs are the first k present shards, the
// outputs every missing shard, ascending, and row r equals M[O[r]] * inverse(rows S of M), parity
// rows included. Then the same mask with a seeded want mask: the outputs are the wanted missing
// shards with the rows they had, a want mask naming nothing missing gives an empty record, and a
// mask with k - 1 present gives too-few exactly when something is to rebuild. 0 on success, else
// 1000 * (code index + 1) + mask index + 1.
int fec__selftest_some_plan(void) {
    static const int shapes[][2] = {{8, 4}, {2, 1}, {20, 10}, {10, 22}, {1, 31}, {31, 1}};
    uint8_t ex768[768];
    for (uint32_t i = 0; i < 768; ++i) ex768[i] = fk::wide_exp768(i);
    const uint8_t* lg = gf::kTables.log;
    uint64_t seed = 0xD1B54A32D192ED03ull;
    auto rnd = [&seed]() -> uint32_t {
        seed ^= seed << 13;
        seed ^= seed >> 7;
        seed ^= seed << 17;
        return (uint32_t)(seed >> 16);
    };
    int si = 0;
    for (auto& sh : shapes) {
        ++si;
        const uint32_t k = (uint32_t)sh[0], m = (uint32_t)sh[1], n = k + m;
        const std::vector<uint8_t> M = rs::build_matrix((int)k, (int)n);
        if (M.empty()) return 1000 * si;
        const fk::WideLayout lay = fk::wide_layout(k, fk::some_rows(m));
        const uint32_t all = fk::low_mask(n);
        // stray bits at and above n are set in both masks throughout: they are ignored
        const uint32_t stray = ~all;
        std::vector<uint8_t> rec(lay.stride), rec2(lay.stride);
        const int cases = 64 + 1 + (m >= k ? 1 : 0);
        for (int ci = 0; ci < cases; ++ci) {
            const int fail = 1000 * si + ci + 1;
            uint32_t pres = all;
            if (ci == 64) {
                pres = fk::low_mask(k);                    // all parity lost
            } else if (ci == 65) {
                pres = (fk::low_mask(k) << k) & all;       // exactly k present, all of them parity
            } else {
                for (uint32_t lose = rnd() % (m + 1); lose > 0;) {
                    const uint32_t i = rnd() % n;
                    if ((pres >> i) & 1u) {
                        pres &= ~(1u << i);
                        --lose;
                    }
                }
            }
            std::vector<uint8_t> S, O;
            for (uint32_t i = 0; i < n && S.size() < k; ++i)
                if ((pres >> i) & 1u) S.push_back((uint8_t)i);
            for (uint32_t i = 0; i < n; ++i)
                if (!((pres >> i) & 1u)) O.push_back((uint8_t)i);
            std::fill(rec.begin(), rec.end(), 0xEE);
            if (fk::some_plan_record(rec.data(), lay, pres | stray, 0xFFFFFFFFu, k, n, ex768, lg) != 0) return fail;
            if (rec[lay.nout_off] != O.size()) return fail;
            if (O.empty()) continue;
            if (memcmp(&rec[lay.in_off], S.data(), k) || memcmp(&rec[lay.out_off], O.data(), O.size())) return fail;
            std::vector<uint8_t> inv((size_t)k * k);
            for (uint32_t p = 0; p < k; ++p) memcpy(&inv[(size_t)p * k], &M[(size_t)S[p] * k], k);
            if (!rs::invert((int)k, inv.data())) return fail;
            for (size_t r = 0; r < O.size(); ++r)
                for (uint32_t p = 0; p < k; ++p) {
                    uint8_t c = 0;   // (M[o] * inv)[p]
                    for (uint32_t t = 0; t < k; ++t) c ^= gf::mul(M[(size_t)O[r] * k + t], inv[(size_t)t * k + p]);
                    if (rec[lay.coef_off + r * k + p] != c) return fail;
                }
            // a want mask: only the wanted missing shards, each with the row it had
            const uint32_t want = rnd() & all;
            std::fill(rec2.begin(), rec2.end(), 0xEE);
            if (fk::some_plan_record(rec2.data(), lay, pres, want | stray, k, n, ex768, lg) != 0) return fail;
            uint32_t r2 = 0;
            for (size_t r = 0; r < O.size(); ++r) {
                if (!((want >> O[r]) & 1u)) continue;
                if (rec2[lay.out_off + r2] != O[r] ||
                    memcmp(&rec2[lay.coef_off + r2 * k], &rec[lay.coef_off + r * k], k))
                    return fail;
                ++r2;
            }
            if (rec2[lay.nout_off] != r2) return fail;
            if (fk::some_plan_record(rec2.data(), lay, pres, pres | stray, k, n, ex768, lg) != 0 || rec2[lay.nout_off])
                return fail;
            // k - 1 present: too few exactly when something is to rebuild
            uint32_t few = 0;
            for (uint32_t p = 0; p + 1 < k; ++p) few |= 1u << S[p];
            if (fk::some_plan_record(rec2.data(), lay, few, 0xFFFFFFFFu, k, n, ex768, lg) != FEC_ERR_TOO_FEW_SHARDS ||
                rec2[lay.nout_off])
                return fail;
            if (fk::some_plan_record(rec2.data(), lay, few, few, k, n, ex768, lg) != 0 || rec2[lay.nout_off]) return fail;
        }
    }
    return 0;
}

// ---------------------------------------------------------------- ragged batches
// The uniform calls' checks, max_shard_len in place of shard_len.
int fec_rs_encode_ragged_batch(fec_ctx* ctx, int k, int m, size_t max_shard_len, size_t nblocks, const uint8_t* data,
                               size_t data_block_stride, uint8_t* parity, size_t parity_block_stride,
                               size_t shard_stride, const uint32_t* block_len, int32_t* block_status, int flags) {
    const uint8_t* par = parity;
    Call c{k, m, 256, false, flags, max_shard_len, nblocks, data, data_block_stride, &par, parity_block_stride,
           shard_stride};
    c.encode = true;
    c.null_arg = !block_len;
    c.words[0] = {block_len, block_status};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_encode_ragged_device(ctx, code, max_shard_len, nblocks, data, data_block_stride, parity,
                                   parity_block_stride, shard_stride, block_len, block_status, ctx->d_err);
}

int fec_rs_reconstruct_ragged_batch(fec_ctx* ctx, int k, int m, size_t max_shard_len, size_t nblocks, uint8_t* data,
                                    size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                                    size_t shard_stride, const uint32_t* present_mask, const uint32_t* block_len,
                                    int32_t* block_status, int flags) {
    Call c{k, m, FEC_MAX_DECODE_SHARDS, false, flags, max_shard_len, nblocks, data, data_block_stride, &parity,
           parity_block_stride, shard_stride};
    c.null_arg = !present_mask || !block_len;
    c.words[0] = {present_mask, block_status};
    c.words[1] = {block_len, nullptr};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_reconstruct_ragged_device(ctx, code, max_shard_len, nblocks, data, data_block_stride, parity,
                                        parity_block_stride, shard_stride, present_mask, block_len, block_status,
                                        ctx->d_err);
}

int fec_rs_recover_ragged_batch(fec_ctx* ctx, int k, int m, size_t max_shard_len, size_t nblocks, const uint8_t* data,
                                size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                                size_t shard_stride, const uint32_t* present_mask, const uint32_t* block_len,
                                uint8_t* out, size_t out_block_stride, int out_slots, int32_t* block_status,
                                int flags) {
    Call c{k, m, FEC_MAX_DECODE_SHARDS, false, flags, max_shard_len, nblocks, data, data_block_stride, &parity,
           parity_block_stride, shard_stride};
    c.null_arg = !present_mask || !block_len || !out;
    c.has_out = true, c.out = out, c.obs = out_block_stride, c.out_slots = out_slots;
    c.words[0] = {present_mask, block_status};
    c.words[1] = {block_len, nullptr};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_reconstruct_ragged_device(ctx, code, max_shard_len, nblocks, const_cast<uint8_t*>(data),
                                        data_block_stride, parity, parity_block_stride, shard_stride, present_mask,
                                        block_len, block_status, ctx->d_err, out, out_block_stride,
                                        (uint32_t)out_slots);
}

// Internal self-test (not part of the public ABI, no device needed): the item arithmetic of the
// ragged kernels (fec_ragged.hpp), walked as the kernels walk it. For each row of a table of length
// vectors and tile sizes, every workgroup's tile and window are taken, its rounds of 256 lanes
// swept, and each item located in the tile's prefix: the items met, in order, must be exactly the
// (block, chunk) pairs of the batch in order, chunk below the block's count, each once, none
// missing; a window past its tile's item count must be empty, and no workgroup may run more than
// kRagRounds rounds. 0 on success, else 100 * (row + 1) + the failing check.
int fec__selftest_ragged_tiles(void) {
    struct Row {
        std::vector<uint32_t> lens;
        uint32_t max_len, g;
    };
    const uint32_t W = fk::kRagWindow, K16 = (uint32_t)fk::kChunk;
    std::vector<Row> rows;
    rows.push_back({std::vector<uint32_t>(40, 0), 1202, 8});                        // all-zero tiles
    {   // a zero run spanning a tile edge (blocks 5..10 of tiles of 8), an oversize block in it
        std::vector<uint32_t> l = {1202, 1, 16, 17, 50, 0, 0, 0, 0, 1203, 0, 33, 1202, 0, 15, 1200, 0xFFFFFFFFu, 7};
        rows.push_back({l, 1202, 8});
        rows.push_back({l, 1202, 3});
        rows.push_back({l, 1202, 1});
        rows.push_back({l, 1202, 256});
    }
    rows.push_back({{1202}, 1202, 16});                                             // a single block
    rows.push_back({{1}, 1202, 1});
    for (int d = -1; d <= 1; ++d) {   // a tile's sum = a multiple of 256, one less, one more
        rows.push_back({{16u * 200u, 0, 16u * (uint32_t)(56 + d), 16u * 256u}, 16u * 256u, 4});
        rows.push_back({{16u * (uint32_t)(256 + d)}, 16u * 300u, 1});
        rows.push_back({{16u * (W / 2), 16u * (uint32_t)((int)(W / 2) + d)}, 16u * W, 2});   // and of a window
    }
    rows.push_back({{70000, 1, 33333}, 70000, 1});                                  // several windows per tile
    rows.push_back({{70000, 1, 33333}, 70000, 16});
    rows.push_back({{5, 0, 1u << 30, 17}, 1u << 30, 64});                           // a 2^26-chunk shard
    int row = 0;
    for (const Row& r : rows) {
        const int fail = 100 * ++row;
        const uint32_t nblocks = (uint32_t)r.lens.size();
        const uint32_t cps_max = (r.max_len + K16 - 1) / K16;
        const uint32_t G = fk::rag_clamp_blocks(r.g, cps_max);
        if (G < 1 || G > fk::kRagMaxTileBlocks || (uint64_t)G * cps_max > fk::kRagMaxTileItems) return fail + 1;
        const uint32_t nwin = fk::rag_windows(G, cps_max);
        if ((uint64_t)nwin * W < (uint64_t)G * cps_max) return fail + 2;
        const uint32_t ntiles = (nblocks + G - 1) / G;
        uint32_t nb = 0, nc = 0;   // the next (block, chunk) the walk must meet
        auto skip_empty = [&] {
            while (nb < nblocks && nc >= fk::rag_chunks(r.lens[nb], r.max_len)) ++nb, nc = 0;
        };
        std::vector<uint32_t> prefix(G + 1);
        for (uint32_t wg = 0; wg < ntiles * nwin; ++wg) {
            const fk::RagTile T = fk::rag_tile(wg, G, nwin, nblocks);
            if (T.gt < 1 || T.gt > G || T.b0 + T.gt > nblocks || T.win >= nwin) return fail + 3;
            prefix[0] = 0;
            for (uint32_t g = 0; g < T.gt; ++g) prefix[g + 1] = prefix[g] + fk::rag_chunks(r.lens[T.b0 + g], r.max_len);
            const uint32_t total = prefix[T.gt];
            const fk::RagSpan sp = fk::rag_span(T.win, total);
            if (sp.hi > total || sp.lo > sp.hi) return fail + 4;
            if ((uint64_t)T.win * W >= total && sp.lo != sp.hi) return fail + 5;   // a window past the sum is empty
            uint32_t rounds = 0;
            for (uint32_t base = sp.lo; base < sp.hi; base += (uint32_t)fk::kThreads, ++rounds)
                for (uint32_t lane = 0; lane < (uint32_t)fk::kThreads; ++lane) {
                    const uint32_t t = base + lane;
                    if (t >= sp.hi) continue;
                    const uint32_t g = fk::rag_locate(prefix.data(), T.gt, t);
                    if (g >= T.gt) return fail + 6;
                    const uint32_t c = t - prefix[g];
                    if (c >= fk::rag_chunks(r.lens[T.b0 + g], r.max_len)) return fail + 7;
                    skip_empty();
                    if (nb != T.b0 + g || nc != c) return fail + 8;   // in order: each pair once
                    ++nc;
                }
            if (rounds > fk::kRagRounds) return fail + 9;
        }
        skip_empty();
        if (nb != nblocks) return fail + 10;   // every pair met
    }
    return 0;
}

// Internal self-test (not part of the public ABI, no device needed): the wide plan's coefficient
// rows (fec_wide.hpp wide_logsum / wide_coef, the functions rs_plan_wide_kernel runs) equal the
// rows of the inverse of the first-k-present submatrix of the systematic matrix, for 64 seeded
// random recoverable masks per shape, plus all data lost where m >= k. 0 on success, else
// 1000 * (shape index + 1) + mask index + 1.
int fec__selftest_wide_plan(void) {
    static const int shapes[][2] = {{32, 1}, {20, 13}, {33, 31}, {64, 16}, {128, 128}, {255, 1}, {1, 255}, {8, 4}};
    uint8_t ex768[768];
    for (uint32_t i = 0; i < 768; ++i) ex768[i] = fk::wide_exp768(i);
    const uint8_t* lg = gf::kTables.log;
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto rnd = [&seed]() -> uint32_t {
        seed ^= seed << 13;
        seed ^= seed >> 7;
        seed ^= seed << 17;
        return (uint32_t)(seed >> 16);
    };
    int si = 0;
    for (auto& sh : shapes) {
        ++si;
        const int k = sh[0], m = sh[1], n = k + m;
        const std::vector<uint8_t> M = rs::build_matrix(k, n);
        if (M.empty()) return 1000 * si;
        const int cases = 64 + (m >= k ? 1 : 0);
        for (int ci = 0; ci < cases; ++ci) {
            std::vector<uint8_t> pres((size_t)n, 1);
            if (ci == 64) {
                for (int i = 0; i < k; ++i) pres[i] = 0;
            } else {
                for (int lose = (int)(rnd() % (uint32_t)(m + 1)); lose > 0;) {
                    const uint32_t i = rnd() % (uint32_t)n;
                    if (pres[i]) {
                        pres[i] = 0;
                        --lose;
                    }
                }
            }
            std::vector<uint8_t> S, O;
            for (int i = 0; i < n && (int)S.size() < k; ++i)
                if (pres[i]) S.push_back((uint8_t)i);
            for (int i = 0; i < k; ++i)
                if (!pres[i]) O.push_back((uint8_t)i);
            if (O.empty()) continue;
            std::vector<uint8_t> sub((size_t)k * k);
            for (int p = 0; p < k; ++p) memcpy(&sub[(size_t)p * k], &M[(size_t)S[p] * k], (size_t)k);
            if (!rs::invert(k, sub.data())) return 1000 * si + ci + 1;
            std::vector<uint32_t> D((size_t)k);
            for (int p = 0; p < k; ++p) D[p] = fk::wide_logsum(lg, S.data(), (uint32_t)k, S[p], (uint32_t)p);
            for (size_t r = 0; r < O.size(); ++r) {
                const uint32_t N = fk::wide_logsum(lg, S.data(), (uint32_t)k, O[r], (uint32_t)k);
                for (int p = 0; p < k; ++p)
                    if (fk::wide_coef(ex768, lg, N, D[p], O[r], S[p]) != sub[(size_t)O[r] * k + p])
                        return 1000 * si + ci + 1;
            }
        }
    }
    return 0;
}

int fec_xor_encode_batch(fec_ctx* ctx, int k, size_t shard_len, size_t nblocks, const uint8_t* data,
                         size_t data_block_stride, uint8_t* parity, size_t parity_block_stride, size_t shard_stride,
                         int flags) {
    const uint8_t* par = parity;
    Call c{k, 1, 256, true, flags, shard_len, nblocks, data, data_block_stride, &par, parity_block_stride, shard_stride};
    c.rs = false;
    const int rc = check_call(ctx, c, nullptr);
    if (rc != kRun) return rc;
    if (flags == FEC_DEVICE)
        return xor_encode_device(ctx, k, shard_len, nblocks, data, data_block_stride, parity, parity_block_stride,
                                 shard_stride);
    return host_encode(ctx, nullptr, k, 1, shard_len, nblocks, data, data_block_stride, parity, parity_block_stride,
                       shard_stride, flags == FEC_HOST_PINNED);
}

int fec_xor_reconstruct_batch(fec_ctx* ctx, int k, size_t shard_len, size_t nblocks, uint8_t* data,
                              size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                              size_t shard_stride, const uint32_t* present_mask, int32_t* block_status, int flags) {
    Call c{k, 1, FEC_MAX_DECODE_SHARDS, true, flags, shard_len, nblocks, data, data_block_stride, &parity,
           parity_block_stride, shard_stride};
    c.rs = false;
    c.null_arg = !present_mask;
    c.words[0] = {present_mask, block_status};
    const int rc = check_call(ctx, c, nullptr);
    if (rc != kRun) return rc;
    if (flags == FEC_DEVICE)
        return xor_reconstruct_device(ctx, k, shard_len, nblocks, data, data_block_stride, parity,
                                      parity_block_stride, shard_stride, present_mask, block_status, ctx->d_err);
    return host_reconstruct_xor(ctx, k, shard_len, nblocks, data, data_block_stride, parity, parity_block_stride,
                                shard_stride, present_mask, block_status);
}

}  // extern "C"
