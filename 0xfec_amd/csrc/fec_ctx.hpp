// fec_ctx.hpp — what the host translation units of the C ABI share (internal): the per-device
// context and its limits (fec_capi.cpp owns its lifecycle and the code cache), the device-memory
// cores (fec_cores.cpp) and the host-resident drivers (fec_host.cpp) that the entry points call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <map>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/fec_hip.h"

#pragma GCC visibility push(hidden)

// One device allocation that frees itself: move-only, null until upload() fills it.
template <class T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p, o.p);
        return *this;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    // hipMalloc of `bytes` and a host-to-device hipMemcpy of them (null stream) from src.
    hipError_t upload(const void* src, size_t bytes) {
        const hipError_t e = hipMalloc(&p, bytes);
        return e != hipSuccess ? e : hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
    }
    operator T*() const { return p; }
};

struct Code {
    int k = 0, m = 0;
    int kind = 0;                  // FEC_MATRIX_* (fec_hip_matrix.h)
    bool solve = false;            // a custom matrix: decode plans by elimination (fec_solve.hpp), no fixed-shape
                                   // encode; d_logv, d_dall, the locate tables and d_dytabs stay null
    std::vector<uint8_t> matrix;   // n x k
    std::vector<uint8_t> logv;     // n bytes: log of shard r's multiplier v_r (rs_matrix.hpp grs_logv; zeros for kind 0)
    DevBuf<uint8_t> d_logv;        // the same on the device; null for kind 0 (the plan kernels test it)
    DevBuf<uint8_t> d_prows;       // m x k
    DevBuf<uint32_t> d_tabs;       // m x k PermTabs
    DevBuf<uint32_t> d_dytabs;     // dyadic codes: leaf PermTabs of the split-recursive encode
    DevBuf<uint32_t> d_single;     // single-erasure decode tables (fk::direct_table_words), when small
    DevBuf<uint32_t> d_single_coef;      // their coefficient bytes, (k*m) rows of ceil(k/4) dwords
    std::vector<uint32_t> single_coef;   // host copy
    DevBuf<uint8_t> d_dall;        // n bytes: log v_s + sum_{t != s} log(s ^ t) mod 255 (sorted plans)
    DevBuf<uint8_t> d_loctab;      // m > 0: the locate call's table (fec_locate.hpp locate_table)
    DevBuf<uint32_t> d_loc_carry;  // k > 128, m > 16: PermTabs of locate's later passes, a slab per pass
    DevBuf<uint32_t> d_lmtab;      // 1 <= m <= 16: the locate-multi call's table (fec_locate_multi.hpp)
};

// The shards of one batch call, or of the blocks of it that one launch or one host chunk takes.
struct Shards {
    size_t len, nblocks;   // bytes per shard (ragged calls: max_shard_len), blocks
    uint8_t* data;         // data shard j of block b at data + b * dbs + j * ss
    size_t dbs;
    uint8_t* parity;       // parity shard r of block b at parity + b * pbs + r * pss
    size_t pbs;
    size_t ss, pss;        // pss == ss in every ABI layout; the host path's decode stage is parity-major
                           // (only the narrow reconstruct's kernels take a parity stride of their own)
    uint8_t* shard(size_t b, size_t j) const { return data + b * dbs + j * ss; }
    uint8_t* par(size_t b, size_t r) const { return parity + b * pbs + r * pss; }
    // The same batch, blocks [b0, b0 + nb).
    Shards blocks(size_t b0, size_t nb) const {
        Shards s = *this;
        s.nblocks = nb;
        s.data += b0 * dbs;
        s.parity += b0 * pbs;
        return s;
    }
};

// The out region of a recover call (`slots` shards per block, ss apart), or none; the update call's
// old data.
struct OutRegion {
    uint8_t* base = nullptr;
    size_t bs = 0;
    uint32_t slots = 0;
    OutRegion blocks(size_t b0) const { return {base ? base + b0 * bs : nullptr, bs, slots}; }
};

// The word arrays of a decode: mask_words present-mask words and a status (may be null) per block, and
// the sticky error word of the whole call.
struct DecodeWords {
    const uint32_t* masks;
    size_t mask_words;
    int32_t* status;
    int* err;
    DecodeWords blocks(size_t b0) const {
        return {masks + b0 * mask_words, mask_words, status ? status + b0 : nullptr, err};
    }
};

// Bytes of staged shards per FEC_HOST chunk (x2 buffers, in and out).
constexpr size_t kStageBytes = size_t(128) << 20;
// Upper bound on decode plan workspace.
constexpr size_t kPlanBytes = size_t(256) << 20;
// nblocks * chunks-per-shard must stay below 2^31 per launch (32-bit item ids).
constexpr uint64_t kMaxItems = uint64_t(1) << 31;

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
    int kind = 0;            // the matrix kind of the RS calls made from now on (fec_hip_matrix.h)
    // by (kind, k, m, registration: 0 for the built-in kinds); entries stay until the ctx goes
    std::map<std::tuple<int, int, int, int>, Code> codes;
    // fec_ctx_set_custom_matrix: every registration's parity rows (m x k; registration id = index + 1,
    // its k and m beside it), and the registration in force for each (k, m)
    struct CustomRows {
        int k, m;
        std::vector<uint8_t> rows;
    };
    std::vector<CustomRows> custom_rows;
    std::map<std::pair<int, int>, int> custom;
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

inline size_t round16(size_t x) { return (x + 15) & ~size_t(15); }

// ---------------------------------------------------------------- fec_capi.cpp
int select_device(fec_ctx* ctx);
// The ctx's code for (ctx->kind, k, m), built and cached on first use. Kind custom: the code of the
// matrix registered for (k, m), FEC_ERR_NO_MATRIX when there is none.
int get_code(fec_ctx* ctx, int k, int m, Code** out);
// Grow the buffers that share capacity *cap (counted in units of `unit` bytes) to hold n units:
// pinned host memory where `pinned`, else device memory. No stream may still use the old ones.
struct GrowBuf {
    void** p;
    bool pinned;
};
int grow_bufs(size_t* cap, size_t n, size_t unit, std::initializer_list<GrowBuf> bufs);
// The ctx's own buffers (of ctx->work: plans, wflags), grown once ctx->stream has drained.
int grow_plans(fec_ctx* ctx, size_t bytes);
int grow_wflags(fec_ctx* ctx, size_t n);
int grow_stage(fec_ctx* ctx, size_t bytes);
int grow_masks(fec_ctx* ctx, size_t n);

// ---------------------------------------------------------------- fec_cores.cpp: device-memory cores
// Each enqueues one call's launches on ctx->stream, with ctx->work as their scratch.
int rs_encode_device(fec_ctx* ctx, Code* code, const Shards& s);
// Reconstruct (no out region: in place in the data region) and recover.
struct ReconCall {
    Shards s;
    DecodeWords w;
    OutRegion out;
    ReconCall blocks(size_t b0, size_t nb) const { return {s.blocks(b0, nb), w.blocks(b0), out.blocks(b0)}; }
};
int rs_reconstruct_device(fec_ctx* ctx, Code* code, const ReconCall& c);
// (the wide and the reconstruct-some cores look their code up themselves, for its d_logv)
int rs_reconstruct_wide_device(fec_ctx* ctx, int k, int m, const ReconCall& c);
int rs_reconstruct_ragged_device(fec_ctx* ctx, Code* code, const ReconCall& c, const uint32_t* lens);
int rs_verify_device(fec_ctx* ctx, Code* code, const Shards& s, int32_t* status, uint32_t* count);
// Update and encode-idx (fec_update.hip): s.data is the data folded in (update: the new version),
// `old` the old version (encode-idx: none).
struct UpdateCall {
    Shards s;
    OutRegion old;
    const uint32_t* masks;
    size_t mask_words;
};
int rs_update_device(fec_ctx* ctx, const Code* code, const UpdateCall& u);
// Locate (fec_locate.hip): the outputs of one call (present and counts may be null).
struct LocateCall {
    Shards s;
    int32_t* verdict;
    uint32_t* present;
    size_t mask_words;
    uint32_t* counts;
};
int rs_locate_device(fec_ctx* ctx, const Code* code, const LocateCall& c);
// Locate-multi (fec_locate_multi.hip): the outputs of one call (present and counts may be null),
// m <= 16.
struct LocateMultiCall {
    Shards s;
    int max_bad;
    int32_t* bad_count;
    uint32_t* present;
    size_t mask_words;
    uint32_t* counts;
};
int rs_locate_multi_device(fec_ctx* ctx, const Code* code, const LocateMultiCall& c);
// Locate-partial (fec_locate_partial.hip): locate-multi's call with the blocks' present masks,
// mask_words apart like the masks written (present may be masks itself).
struct LocatePartialCall {
    LocateMultiCall c;
    const uint32_t* masks;
};
int rs_locate_partial_device(fec_ctx* ctx, const Code* code, const LocatePartialCall& c);
int rs_reconstruct_some_device(fec_ctx* ctx, int k, int m, const Shards& s, const DecodeWords& w,
                               const uint32_t* want);
// want: w.mask_words words per block, as the present masks
int rs_reconstruct_some_wide_device(fec_ctx* ctx, int k, int m, const Shards& s, const DecodeWords& w,
                                    const uint32_t* want);
int rs_encode_ragged_device(fec_ctx* ctx, Code* code, const Shards& s, const uint32_t* lens, int32_t* status,
                            int* err);
// The ragged forms of verify and reconstruct-some (s.len: max_shard_len; lens: nblocks lengths).
int rs_verify_ragged_device(fec_ctx* ctx, Code* code, const Shards& s, const uint32_t* lens, int32_t* status,
                            uint32_t* count, int* err);
int rs_reconstruct_some_ragged_device(fec_ctx* ctx, int k, int m, const Shards& s, const DecodeWords& w,
                                      const uint32_t* want, const uint32_t* lens);
int xor_encode_device(fec_ctx* ctx, int k, const Shards& s);
int xor_reconstruct_device(fec_ctx* ctx, int k, const Shards& s, const DecodeWords& w);

// ---------------------------------------------------------------- fec_host.cpp: host-resident path
// Encode (RS when code != nullptr, else XOR(k, 1)): host data -> host parity.
int host_encode(fec_ctx* ctx, Code* code, int k, int m, const Shards& s, bool pinned);
int host_reconstruct_rs(fec_ctx* ctx, Code* code, const Shards& s, const uint32_t* masks, int32_t* block_status,
                        bool pinned);
int host_reconstruct_xor(fec_ctx* ctx, int k, const Shards& s, const uint32_t* masks, int32_t* block_status);
int host_reconstruct_wide(fec_ctx* ctx, int k, int m, const Shards& s, const uint32_t* masks, size_t mask_words,
                          int32_t* block_status);
// Free every buffer of the set and forget it (pointers null, capacities 0), whatever a free
// returns; the first failure, or hipSuccess. The set's events stay.
hipError_t host_set_free(HostSet& s);

#pragma GCC visibility pop
