// fec_capi.cpp — C ABI of the MI355X FEC codec (include/fec_hip.h).
//
// Owns the per-device context (fec_ctx.hpp): HIP stream, per-(k, m) code cache (systematic matrix,
// device parity rows, encode PermTabs), decode plan workspace, pinned staging for the
// FEC_HOST path; checks every batch call's arguments and hands it to its device core
// (fec_cores.cpp) or its host-resident driver (fec_host.cpp). No CPU compute fallback exists:
// without a HIP device every compute entry point fails with FEC_ERR_NO_DEVICE / FEC_ERR_HIP.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <functional>

#include "../../include/fec_hip_matrix.h"
#include "../../include/fec_hip_ragged.h"
#include "../../include/fec_hip_some_wide.h"
#include "fec_ctx.hpp"
#include "fec_kernels.hpp"
#include "fec_locate.hpp"
#include "fec_locate_multi.hpp"
#include "gf256.h"
#include "rs_matrix.hpp"

namespace {

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

}  // namespace

int select_device(fec_ctx* ctx) {
    if (!ctx) return FEC_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    return FEC_OK;
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

int get_code(fec_ctx* ctx, int k, int m, Code** out) {
    if (k <= 0 || m < 0) return FEC_ERR_INV_SHARD_NUM;
    if (k + m > 256) return FEC_ERR_MAX_SHARD_NUM;
    int reg = 0;
    if (ctx->kind == FEC_MATRIX_CUSTOM) {
        const auto cu = ctx->custom.find({k, m});
        if (cu == ctx->custom.end()) return FEC_ERR_NO_MATRIX;
        reg = cu->second;
    }
    auto key = std::make_tuple(ctx->kind, k, m, reg);
    auto it = ctx->codes.find(key);
    if (it != ctx->codes.end()) {
        *out = &it->second;
        return FEC_OK;
    }
    Code c;
    c.k = k;
    c.m = m;
    c.kind = ctx->kind;
    c.solve = reg != 0;
    if (c.solve) {   // identity on top, the registered rows below
        const std::vector<uint8_t>& rows = ctx->custom_rows[(size_t)reg - 1].rows;
        c.matrix.assign((size_t)(k + m) * k, 0);
        for (int j = 0; j < k; ++j) c.matrix[(size_t)j * k + j] = 1;
        memcpy(c.matrix.data() + (size_t)k * k, rows.data(), rows.size());
    } else {
        c.matrix = rs::build_matrix_kind(c.kind, k, k + m);
    }
    if (c.matrix.empty()) return FEC_ERR_INV_SHARD_NUM;
    // a custom code keeps the single-erasure tables (the direct and the routed decode) only if every
    // entry of its parity rows is nonzero: only then is every single-erasure plan solvable
    const bool single_ok =
        !c.solve || std::find(c.matrix.begin() + (size_t)k * k, c.matrix.end(), (uint8_t)0) == c.matrix.end();
    c.logv = rs::grs_logv(c.kind, k, k + m);
    if (c.kind == rs::kMatrixCauchy) HIP_TRY(c.d_logv.upload(c.logv.data(), c.logv.size()));
    if (m > 0) {
        std::vector<uint32_t> tabs((size_t)m * k * 8);
        for (int r = 0; r < m; ++r)
            for (int j = 0; j < k; ++j) {
                gf::PermTab t = gf::make_permtab(c.matrix[(size_t)(k + r) * k + j]);
                memcpy(&tabs[((size_t)r * k + j) * 8], &t, sizeof(t));
            }
        HIP_TRY(c.d_prows.upload(c.matrix.data() + (size_t)k * k, (size_t)m * k));
        HIP_TRY(c.d_tabs.upload(tabs.data(), tabs.size() * 4));
        // single-erasure plans: data shard E0 lost, parity R0 the first present one; inputs are
        // the other data shards in order, then parity R0 (the first k present shards):
        // x_E0 = inv(A[R0][E0]) * (p_R0 ^ sum_{j != E0} A[R0][j] x_j)   (reed_solomon.go:124)
        if (k + m <= FEC_MAX_DECODE_SHARDS && single_ok) {
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
            HIP_TRY(c.d_single_coef.upload(sc.data(), sc.size() * 4));
        }
        if (k + m <= FEC_MAX_DECODE_SHARDS && single_ok &&
            fk::direct_table_words((uint32_t)k, (uint32_t)m) * 4 <= 16 * 1024) {
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
            HIP_TRY(c.d_single.upload(st.data(), st.size() * 4));
        }
        // (a custom code: no locate tables and no dyadic leaves; the locate calls are refused and the
        // encode is the generic fold, whatever its rows)
        if (!c.solve) {   // the locate call's ratio -> column table and the field's inverses (fec_locate.hpp)
            uint8_t lt[fk::kLocateTabBytes];
            if (!fk::locate_table(lt, c.matrix.data() + (size_t)k * k, (uint32_t)k, (uint32_t)m))
                return FEC_ERR_INVALID_ARG;
            HIP_TRY(c.d_loctab.upload(lt, sizeof(lt)));
        }
        if (!c.solve && fk::locate_needs_carry_tabs((uint32_t)k, (uint32_t)m)) {
            // locate's later passes, each row 0's tables followed by its own rows' (fec_locate.hpp)
            const size_t row = (size_t)k * 8, slab = fk::kLocateRows * row;
            const uint32_t later = fk::locate_passes((uint32_t)m) - 1;
            std::vector<uint32_t> carry(later * slab, 0);
            for (uint32_t p = 0; p < later; ++p) {
                const int r0 = 1 + (fk::kLocateRows - 1) * (int)(p + 1);
                const int rows = std::min(fk::kLocateRows - 1, m - r0);
                memcpy(&carry[p * slab], tabs.data(), row * 4);
                memcpy(&carry[p * slab + row], &tabs[r0 * row], rows * row * 4);
            }
            HIP_TRY(c.d_loc_carry.upload(carry.data(), carry.size() * 4));
        }
        if (!c.solve && m >= 1 && m <= fk::kLocateMultiRows) {
            // the locate-multi call's coefficients as PermTabs, then the field's tables
            // (fec_locate_multi.hpp)
            uint8_t A[fk::kLocateMultiRows * fk::kLocateMultiRows];
            fk::locate_multi_table(A, (uint32_t)k, (uint32_t)m, c.logv.data());
            std::vector<uint32_t> lm(fk::locate_multi_tab_words((uint32_t)m), 0);
            for (int i = 0; i < m * m; ++i) {
                const gf::PermTab t = gf::make_permtab(A[i]);
                memcpy(&lm[(size_t)i * 8], &t, sizeof(t));
            }
            memcpy(&lm[(size_t)m * m * 8], &gf::kTables, sizeof(gf::Tables));
            HIP_TRY(c.d_lmtab.upload(lm.data(), lm.size() * 4));
        }
        const std::vector<uint8_t> leaves = c.solve ? std::vector<uint8_t>() : dyadic_leaves(c.matrix, k, m);
        if (!leaves.empty() && leaves.size() <= (size_t)m * k) {   // staged like m x k tables
            std::vector<uint32_t> dy((size_t)m * k * 8, 0);
            for (size_t i = 0; i < leaves.size(); ++i) {
                gf::PermTab t = gf::make_permtab(leaves[i]);
                memcpy(&dy[i * 8], &t, sizeof(t));
            }
            HIP_TRY(c.d_dytabs.upload(dy.data(), dy.size() * 4));
        }
    }
    // (for m == 0 too: the sorted-plan kernels stage it whatever the code, and a reconstruct of a
    // code without parity, where every loss is a failed block, takes them on long shards)
    if (k + m <= FEC_MAX_DECODE_SHARDS && !c.solve) {
        uint8_t dall[FEC_MAX_DECODE_SHARDS] = {};
        for (int sidx = 0; sidx < k + m; ++sidx) {
            unsigned d = 0;
            for (int t = 0; t < k + m; ++t)
                if (t != sidx) d += gf::kTables.log[sidx ^ t];
            // (+ log v of the shard: the complement sums D_s and N_o both start from this entry)
            dall[sidx] = (uint8_t)((d + c.logv[(size_t)sidx]) % 255u);
        }
        HIP_TRY(c.d_dall.upload(dall, FEC_MAX_DECODE_SHARDS));
    }
    auto res = ctx->codes.emplace(key, std::move(c));
    *out = &res.first->second;
    // the uploads above are plain hipMemcpy (null stream, and from pageable memory they may return
    // before the DMA lands): finish them before a kernel on a non-blocking ctx stream reads a table
    HIP_TRY(hipDeviceSynchronize());
    return FEC_OK;
}

int grow_bufs(size_t* cap, size_t n, size_t unit, std::initializer_list<GrowBuf> bufs) {
    if (n <= *cap) return FEC_OK;
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
// The ctx's own buffers: the old ones are freed only after ctx->stream, the only stream that reads
// them, has drained.
static int grow(fec_ctx* ctx, size_t* cap, size_t n, size_t unit, std::initializer_list<GrowBuf> bufs) {
    if (n <= *cap) return FEC_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return grow_bufs(cap, n, unit, bufs);
}
int grow_plans(fec_ctx* ctx, size_t bytes) {
    return grow(ctx, &ctx->work->plans_cap, bytes, 1, {{(void**)&ctx->work->d_plans, false}});
}
int grow_wflags(fec_ctx* ctx, size_t n) {
    return grow(ctx, &ctx->work->wflags_cap, n, 4, {{(void**)&ctx->work->d_wflags, false}});
}
int grow_stage(fec_ctx* ctx, size_t bytes) {
    return grow(ctx, &ctx->stage_cap, bytes, 1, {{(void**)&ctx->h_stage, true}, {(void**)&ctx->d_stage, false}});
}
int grow_masks(fec_ctx* ctx, size_t n) {
    return grow(ctx, &ctx->masks_cap, n, 4, {{(void**)&ctx->d_masks, false}, {(void**)&ctx->d_status, false}});
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
        case FEC_ERR_SINGULAR: return "matrix is singular";   // klauspost errSingular
        case FEC_ERR_NO_MATRIX: return "no custom matrix registered for these shard counts, or a call custom matrices do not serve";
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
    ctx->codes.clear();   // (each code's device tables free themselves)
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
        (void)host_set_free(s);
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
    for (HostSet& s : p.set) drop(host_set_free(s));
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
// (fec_kernels.hpp FEC_TUNING_KNOBS, keys 0..kTuningKeys-1 in list order) set to `value`,
// process-wide, for every ctx. Tests and tools set knobs while no other thread submits work.
// Returns the previous value, or FEC_ERR_INVALID_ARG for an unknown key.
int fec__set_tuning(fec_ctx* ctx, int key, int value) {
    if (!ctx) return FEC_ERR_INVALID_ARG;
    fk::Tuning& t = fk::g_tune;
#define FEC_KNOB_SLOT(name, def) &t.name,
    std::atomic<int>* slots[fk::kTuningKeys] = {FEC_TUNING_KNOBS(FEC_KNOB_SLOT)};
#undef FEC_KNOB_SLOT
    if (key < 0 || key >= fk::kTuningKeys) return FEC_ERR_INVALID_ARG;
    return slots[key]->exchange(value);
}

// Internal, test-only like fec__set_tuning: the name of knob `key`, or null past the last key
// (the Python face builds Codec.TUNING_KEYS from it).
const char* fec__tuning_name(int key) {
#define FEC_KNOB_NAME(name, def) #name,
    static const char* const names[fk::kTuningKeys] = {FEC_TUNING_KNOBS(FEC_KNOB_NAME)};
#undef FEC_KNOB_NAME
    return key >= 0 && key < fk::kTuningKeys ? names[key] : nullptr;
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
        return fk::sticky_rc(err);
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

// The matrix kinds (fec_hip_matrix.h). Neither ctx call touches the device: the kind only chooses
// which cached Code the next RS call looks up (get_code); queued launches hold their own Code's tables.
int fec_rs_matrix_kind(int kind, int k, int m, uint8_t* out) {
    if (!out || kind < 0 || kind >= rs::kMatrixKinds) return FEC_ERR_INVALID_ARG;
    if (k <= 0 || m < 0) return FEC_ERR_INV_SHARD_NUM;
    if (k + m > 256) return FEC_ERR_MAX_SHARD_NUM;
    const std::vector<uint8_t> mat = rs::build_matrix_kind(kind, k, k + m);
    if (mat.empty()) return FEC_ERR_INV_SHARD_NUM;
    memcpy(out, mat.data(), mat.size());
    return FEC_OK;
}

int fec_ctx_set_matrix(fec_ctx* ctx, int kind) {
    if (!ctx || kind < 0 || (kind >= rs::kMatrixKinds && kind != FEC_MATRIX_CUSTOM)) return FEC_ERR_INVALID_ARG;
    ctx->kind = kind;
    return FEC_OK;
}

// A registration is its rows kept on the ctx; get_code builds the code's tables on first use, keyed
// by the registration, so a (k, m) registered again gets new tables and the old ones stay for the
// launches that hold them.
int fec_ctx_set_custom_matrix(fec_ctx* ctx, int k, int m, const uint8_t* parity_rows) {
    // (the shard counts first, as the batch calls check theirs before they look at the ctx)
    if (k <= 0 || m < 0) return FEC_ERR_INV_SHARD_NUM;
    if (k + m > 256) return FEC_ERR_MAX_SHARD_NUM;
    if (!ctx || !parity_rows || m == 0) return FEC_ERR_INVALID_ARG;
    const size_t bytes = (size_t)m * k;
    int reg = 0;
    for (size_t i = 0; i < ctx->custom_rows.size() && !reg; ++i) {
        const fec_ctx::CustomRows& r = ctx->custom_rows[i];
        if (r.k == k && r.m == m && !memcmp(r.rows.data(), parity_rows, bytes)) reg = (int)i + 1;
    }
    if (!reg) {
        ctx->custom_rows.push_back({k, m, std::vector<uint8_t>(parity_rows, parity_rows + bytes)});
        reg = (int)ctx->custom_rows.size();
    }
    ctx->custom[{k, m}] = reg;
    ctx->kind = FEC_MATRIX_CUSTOM;
    return FEC_OK;
}

int fec_ctx_get_matrix(fec_ctx* ctx, int* kind) {
    if (!ctx || !kind) return FEC_ERR_INVALID_ARG;
    *kind = ctx->kind;
    return FEC_OK;
}

int fec_rs_prepare(fec_ctx* ctx, int k, int m) {
    int rc = select_device(ctx);
    if (rc) return rc;
    Code* code = nullptr;
    return get_code(ctx, k, m, &code);
}

// The argument checks every batch call makes before it runs, in the documented order (fec_hip.h):
// shard counts (and the locate-multi call's limit on m), flags, shard_len, out_slots, max_bad and
// mask_words; then the ctx and the code; an empty
// call; null pointers; and for FEC_DEVICE the layout of the data, parity and out regions, in that
// order, then the alignment of the word arrays. An entry point describes itself in a Call and gets
// kRun back when it has work to do, else the code to return.
struct Call {
    int k, m, max_n;           // max_n: the call's largest k + m (the XOR calls: m = 1)
    bool host_ok;              // FEC_HOST / FEC_HOST_PINNED accepted
    int flags;
    Shards s;                  // m == 0: check_call sets parity to data (never read: no parity slot exists)
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
    int max_m = -1;            // the call's largest m (-1: none; the locate-multi call: 16)
    int max_bad = 1;           // the locate-multi call's max_bad, in [min_bad, FEC_LOCATE_MAX_BAD]
    int min_bad = 1;           // (the locate-partial call: 0)
    bool builtin_only = false; // not served under a custom matrix (fec_hip_matrix.h): FEC_ERR_NO_MATRIX
    struct {
        const void *a, *b;
    } words[2] = {};           // (mask, status)-like pairs of 4-byte arrays, either may be null
};
constexpr int kRun = 1;

// The one place where the ABI's pointers lose their const: which region a call writes is stated by
// fec_hip.h and by the const of the fk::*Args fields that the cores fill from these.
static uint8_t* region(const uint8_t* p) { return const_cast<uint8_t*>(p); }
static Shards shards(size_t shard_len, size_t nblocks, const uint8_t* data, size_t data_block_stride,
                     const uint8_t* parity, size_t parity_block_stride, size_t shard_stride) {
    return {shard_len,    nblocks,     region(data), data_block_stride, region(parity), parity_block_stride,
            shard_stride, shard_stride};
}

static int check_call(fec_ctx* ctx, Call& c, Code** code) {
    const Shards& s = c.s;
    if (c.k <= 0 || c.m < 0) return FEC_ERR_INV_SHARD_NUM;
    if (c.k + c.m > c.max_n) return FEC_ERR_MAX_SHARD_NUM;
    if (c.max_m >= 0 && c.m > c.max_m) return FEC_ERR_INVALID_ARG;
    if (c.flags != FEC_DEVICE && !(c.host_ok && (c.flags == FEC_HOST || c.flags == FEC_HOST_PINNED)))
        return FEC_ERR_INVALID_ARG;
    if (s.len == 0) return FEC_ERR_SHARD_NO_DATA;
    if (s.len > (size_t(1) << 30) || c.out_slots <= 0) return FEC_ERR_INVALID_ARG;
    if (c.max_bad < c.min_bad || c.max_bad > FEC_LOCATE_MAX_BAD) return FEC_ERR_INVALID_ARG;
    if (c.wide && (c.mask_words < (size_t)FEC_MASK_WORDS(c.mask_n ? c.mask_n : c.k + c.m) || c.mask_words > 8))
        return FEC_ERR_INVALID_ARG;
    int rc = select_device(ctx);
    if (rc) return rc;
    if (c.rs && c.builtin_only && ctx->kind == FEC_MATRIX_CUSTOM) return FEC_ERR_NO_MATRIX;
    if (c.rs && (rc = get_code(ctx, c.k, c.m, code))) return rc;
    if (s.nblocks == 0 || (c.encode && c.m == 0)) return FEC_OK;
    if (!s.data || c.null_arg || (c.m > 0 && !s.parity)) return FEC_ERR_INVALID_ARG;
    if (c.m == 0) c.s.parity = s.data;
    if (c.flags != FEC_DEVICE) return kRun;
    if ((rc = check_device_layout(s.data, s.dbs, s.ss, s.len))) return rc;
    if ((rc = check_device_layout(s.parity, s.pbs, s.ss, s.len))) return rc;
    if (c.has_out && (rc = check_device_layout(c.out, c.obs, s.ss, s.len))) return rc;
    for (const auto& w : c.words)
        if ((rc = check_device_words(w.a, w.b))) return rc;
    return kRun;
}

// A recover call is its reconstruct call with an out region, which must be given.
static OutRegion recover_out(Call& c, uint8_t* out, size_t out_block_stride, int out_slots) {
    c.null_arg = c.null_arg || !out;
    c.has_out = true, c.out = out, c.obs = out_block_stride, c.out_slots = out_slots;
    return {out, out_block_stride, (uint32_t)out_slots};
}

int fec_rs_encode_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, const uint8_t* data,
                        size_t data_block_stride, uint8_t* parity, size_t parity_block_stride,
                        size_t shard_stride, int flags) {
    Call c{k, m, 256, true, flags,
           shards(shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.encode = true;
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    if (flags == FEC_DEVICE) return rs_encode_device(ctx, code, c.s);
    return host_encode(ctx, code, k, m, c.s, flags == FEC_HOST_PINNED);
}

int fec_rs_reconstruct_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, uint8_t* data,
                             size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                             size_t shard_stride, const uint32_t* present_mask, int32_t* block_status, int flags) {
    Call c{k, m, FEC_MAX_DECODE_SHARDS, true, flags,
           shards(shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.null_arg = !present_mask;
    c.words[0] = {present_mask, block_status};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    if (flags == FEC_DEVICE)
        return rs_reconstruct_device(ctx, code, {c.s, {present_mask, 1, block_status, ctx->d_err}, {}});
    return host_reconstruct_rs(ctx, code, c.s, present_mask, block_status, flags == FEC_HOST_PINNED);
}

int fec_rs_recover_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, const uint8_t* data,
                         size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                         size_t shard_stride, const uint32_t* present_mask, uint8_t* out, size_t out_block_stride,
                         int out_slots, int32_t* block_status, int flags) {
    Call c{k, m, FEC_MAX_DECODE_SHARDS, false, flags,
           shards(shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.null_arg = !present_mask;
    const OutRegion o = recover_out(c, out, out_block_stride, out_slots);
    c.words[0] = {present_mask, block_status};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_reconstruct_device(ctx, code, {c.s, {present_mask, 1, block_status, ctx->d_err}, o});
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
    Call c{k, m, FEC_MAX_WIDE_SHARDS, true, flags,
           shards(shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.null_arg = !present_mask;
    c.wide = true, c.mask_words = mask_words;
    c.words[0] = {present_mask, block_status};
    c.builtin_only = true;
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    if (flags == FEC_DEVICE)
        return rs_reconstruct_wide_device(ctx, k, m, {c.s, {present_mask, mask_words, block_status, ctx->d_err}, {}});
    return host_reconstruct_wide(ctx, k, m, c.s, present_mask, mask_words, block_status);
}

int fec_rs_recover_wide_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, const uint8_t* data,
                              size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                              size_t shard_stride, const uint32_t* present_mask, size_t mask_words, uint8_t* out,
                              size_t out_block_stride, int out_slots, int32_t* block_status, int flags) {
    if (k + m <= FEC_MAX_DECODE_SHARDS && mask_words == 1)
        return fec_rs_recover_batch(ctx, k, m, shard_len, nblocks, data, data_block_stride, parity,
                                    parity_block_stride, shard_stride, present_mask, out, out_block_stride, out_slots,
                                    block_status, flags);
    Call c{k, m, FEC_MAX_WIDE_SHARDS, false, flags,
           shards(shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.null_arg = !present_mask;
    const OutRegion o = recover_out(c, out, out_block_stride, out_slots);
    c.wide = true, c.mask_words = mask_words;
    c.words[0] = {present_mask, block_status};
    c.builtin_only = true;
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_reconstruct_wide_device(ctx, k, m, {c.s, {present_mask, mask_words, block_status, ctx->d_err}, o});
}

// ---------------------------------------------------------------- verify, reconstruct-some
int fec_rs_verify_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, const uint8_t* data,
                        size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                        size_t shard_stride, int32_t* block_status, uint32_t* mismatch_count, int flags) {
    Call c{k, m, 256, false, flags,
           shards(shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.null_arg = !block_status;
    c.words[0] = {mismatch_count, block_status};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_verify_device(ctx, code, c.s, block_status, mismatch_count);
}

// (m == 0: the parity region is neither read nor written)
int fec_rs_reconstruct_some_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, uint8_t* data,
                                  size_t data_block_stride, uint8_t* parity, size_t parity_block_stride,
                                  size_t shard_stride, const uint32_t* present_mask, const uint32_t* want_mask,
                                  int32_t* block_status, int flags) {
    Call c{k, m, FEC_MAX_DECODE_SHARDS, false, flags,
           shards(shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.null_arg = !present_mask;
    c.words[0] = {present_mask, block_status};
    c.words[1] = {want_mask, nullptr};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_reconstruct_some_device(ctx, k, m, c.s, {present_mask, 1, block_status, ctx->d_err}, want_mask);
}

// Wide reconstruct-some (fec_hip_some_wide.h): one mask word and a narrow code is the narrow call, as
// for the two wide decode calls.
int fec_rs_reconstruct_some_wide_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, uint8_t* data,
                                       size_t data_block_stride, uint8_t* parity, size_t parity_block_stride,
                                       size_t shard_stride, const uint32_t* present_mask, const uint32_t* want_mask,
                                       size_t mask_words, int32_t* block_status, int flags) {
    if (k + m <= FEC_MAX_DECODE_SHARDS && mask_words == 1)
        return fec_rs_reconstruct_some_batch(ctx, k, m, shard_len, nblocks, data, data_block_stride, parity,
                                             parity_block_stride, shard_stride, present_mask, want_mask,
                                             block_status, flags);
    Call c{k, m, FEC_MAX_WIDE_SHARDS, false, flags,
           shards(shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.null_arg = !present_mask;
    c.wide = true, c.mask_words = mask_words;
    c.words[0] = {present_mask, block_status};
    c.words[1] = {want_mask, nullptr};
    c.builtin_only = true;
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_reconstruct_some_wide_device(ctx, k, m, c.s, {present_mask, mask_words, block_status, ctx->d_err},
                                           want_mask);
}

// ---------------------------------------------------------------- locate
// mask_words is checked whether or not present_out is given.
int fec_rs_locate_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, const uint8_t* data,
                        size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                        size_t shard_stride, int32_t* bad_shard, uint32_t* present_out, size_t mask_words,
                        uint32_t* counts, int flags) {
    Call c{k, m, 256, false, flags,
           shards(shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.null_arg = !bad_shard;
    c.wide = true, c.mask_words = mask_words;
    c.words[0] = {present_out, bad_shard};
    c.words[1] = {counts, nullptr};
    c.builtin_only = true;
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_locate_device(ctx, code, {c.s, bad_shard, present_out, mask_words, counts});
}

// Up to m/2 corrupt shards per block; m <= 16 (one pass of the scan's 16 rows).
int fec_rs_locate_multi_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, const uint8_t* data,
                              size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                              size_t shard_stride, int max_bad, int32_t* bad_count, uint32_t* present_out,
                              size_t mask_words, uint32_t* counts, int flags) {
    Call c{k, m, 256, false, flags,
           shards(shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.null_arg = !bad_count;
    c.max_m = fk::kLocateMultiRows, c.max_bad = max_bad;
    c.wide = true, c.mask_words = mask_words;
    c.words[0] = {present_out, bad_count};
    c.words[1] = {counts, nullptr};
    c.builtin_only = true;
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_locate_multi_device(ctx, code, {c.s, max_bad, bad_count, present_out, mask_words, counts});
}

// Locate-multi for blocks with missing shards: the same checks, max_bad = 0 allowed, the masks required.
int fec_rs_locate_partial_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, const uint8_t* data,
                                size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                                size_t shard_stride, const uint32_t* present_mask, size_t mask_words, int max_bad,
                                int32_t* bad_count, uint32_t* present_out, uint32_t* counts, int flags) {
    Call c{k, m, 256, false, flags,
           shards(shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.null_arg = !bad_count || !present_mask;
    c.max_m = fk::kLocateMultiRows, c.max_bad = max_bad, c.min_bad = 0;
    c.wide = true, c.mask_words = mask_words;
    c.words[0] = {present_mask, bad_count};
    c.words[1] = {present_out, counts};
    c.builtin_only = true;
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_locate_partial_device(ctx, code, {{c.s, max_bad, bad_count, present_out, mask_words, counts}, present_mask});
}

// ---------------------------------------------------------------- update, encode-idx
// The two calls differ in the old region alone, which the update call states before it comes here. The
// Call's data region is the data folded in (the new version), its out region the old version: the
// layouts are checked in the order new data, parity, old data.
static int rs_update_call(fec_ctx* ctx, Call& c, const uint32_t* mask, size_t mask_words) {
    c.encode = true;
    c.null_arg = !mask || (c.has_out && !c.out);
    c.wide = true, c.mask_words = mask_words, c.mask_n = c.k;
    c.words[0] = {mask, nullptr};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_update_device(ctx, code, {c.s, {region(c.out), c.obs}, mask, mask_words});
}

int fec_rs_update_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, const uint8_t* old_data,
                        size_t old_block_stride, const uint8_t* new_data, size_t new_block_stride, uint8_t* parity,
                        size_t parity_block_stride, size_t shard_stride, const uint32_t* changed_mask,
                        size_t mask_words, int flags) {
    Call c{k, m, 256, false, flags,
           shards(shard_len, nblocks, new_data, new_block_stride, parity, parity_block_stride, shard_stride)};
    c.has_out = true, c.out = old_data, c.obs = old_block_stride;
    return rs_update_call(ctx, c, changed_mask, mask_words);
}

int fec_rs_encode_idx_batch(fec_ctx* ctx, int k, int m, size_t shard_len, size_t nblocks, const uint8_t* data,
                            size_t data_block_stride, uint8_t* parity, size_t parity_block_stride,
                            size_t shard_stride, const uint32_t* idx_mask, size_t mask_words, int flags) {
    Call c{k, m, 256, false, flags,
           shards(shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    return rs_update_call(ctx, c, idx_mask, mask_words);
}

// ---------------------------------------------------------------- ragged batches
// The uniform calls' checks, max_shard_len in place of shard_len.
int fec_rs_encode_ragged_batch(fec_ctx* ctx, int k, int m, size_t max_shard_len, size_t nblocks, const uint8_t* data,
                               size_t data_block_stride, uint8_t* parity, size_t parity_block_stride,
                               size_t shard_stride, const uint32_t* block_len, int32_t* block_status, int flags) {
    Call c{k, m, 256, false, flags,
           shards(max_shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.encode = true;
    c.null_arg = !block_len;
    c.words[0] = {block_len, block_status};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_encode_ragged_device(ctx, code, c.s, block_len, block_status, ctx->d_err);
}

int fec_rs_reconstruct_ragged_batch(fec_ctx* ctx, int k, int m, size_t max_shard_len, size_t nblocks, uint8_t* data,
                                    size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                                    size_t shard_stride, const uint32_t* present_mask, const uint32_t* block_len,
                                    int32_t* block_status, int flags) {
    Call c{k, m, FEC_MAX_DECODE_SHARDS, false, flags,
           shards(max_shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.null_arg = !present_mask || !block_len;
    c.words[0] = {present_mask, block_status};
    c.words[1] = {block_len, nullptr};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_reconstruct_ragged_device(ctx, code, {c.s, {present_mask, 1, block_status, ctx->d_err}, {}}, block_len);
}

int fec_rs_recover_ragged_batch(fec_ctx* ctx, int k, int m, size_t max_shard_len, size_t nblocks, const uint8_t* data,
                                size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                                size_t shard_stride, const uint32_t* present_mask, const uint32_t* block_len,
                                uint8_t* out, size_t out_block_stride, int out_slots, int32_t* block_status,
                                int flags) {
    Call c{k, m, FEC_MAX_DECODE_SHARDS, false, flags,
           shards(max_shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.null_arg = !present_mask || !block_len;
    const OutRegion o = recover_out(c, out, out_block_stride, out_slots);
    c.words[0] = {present_mask, block_status};
    c.words[1] = {block_len, nullptr};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_reconstruct_ragged_device(ctx, code, {c.s, {present_mask, 1, block_status, ctx->d_err}, o}, block_len);
}

// Ragged verify and reconstruct-some (fec_hip_ragged.h): their uniform calls' checks, block_len among
// the pointers.
int fec_rs_verify_ragged_batch(fec_ctx* ctx, int k, int m, size_t max_shard_len, size_t nblocks, const uint8_t* data,
                               size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                               size_t shard_stride, const uint32_t* block_len, int32_t* block_status,
                               uint32_t* mismatch_count, int flags) {
    Call c{k, m, 256, false, flags,
           shards(max_shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.null_arg = !block_status || !block_len;
    c.words[0] = {mismatch_count, block_status};
    c.words[1] = {block_len, nullptr};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_verify_ragged_device(ctx, code, c.s, block_len, block_status, mismatch_count, ctx->d_err);
}

// (m == 0: the parity region is neither read nor written)
int fec_rs_reconstruct_some_ragged_batch(fec_ctx* ctx, int k, int m, size_t max_shard_len, size_t nblocks,
                                         uint8_t* data, size_t data_block_stride, uint8_t* parity,
                                         size_t parity_block_stride, size_t shard_stride,
                                         const uint32_t* present_mask, const uint32_t* want_mask,
                                         const uint32_t* block_len, int32_t* block_status, int flags) {
    Call c{k, m, FEC_MAX_DECODE_SHARDS, false, flags,
           shards(max_shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.null_arg = !present_mask || !block_len;
    c.words[0] = {present_mask, block_status};
    c.words[1] = {want_mask, block_len};
    Code* code = nullptr;
    const int rc = check_call(ctx, c, &code);
    if (rc != kRun) return rc;
    return rs_reconstruct_some_ragged_device(ctx, k, m, c.s, {present_mask, 1, block_status, ctx->d_err}, want_mask,
                                             block_len);
}

int fec_xor_encode_batch(fec_ctx* ctx, int k, size_t shard_len, size_t nblocks, const uint8_t* data,
                         size_t data_block_stride, uint8_t* parity, size_t parity_block_stride, size_t shard_stride,
                         int flags) {
    Call c{k, 1, 256, true, flags,
           shards(shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.rs = false;
    const int rc = check_call(ctx, c, nullptr);
    if (rc != kRun) return rc;
    if (flags == FEC_DEVICE) return xor_encode_device(ctx, k, c.s);
    return host_encode(ctx, nullptr, k, 1, c.s, flags == FEC_HOST_PINNED);
}

int fec_xor_reconstruct_batch(fec_ctx* ctx, int k, size_t shard_len, size_t nblocks, uint8_t* data,
                              size_t data_block_stride, const uint8_t* parity, size_t parity_block_stride,
                              size_t shard_stride, const uint32_t* present_mask, int32_t* block_status, int flags) {
    Call c{k, 1, FEC_MAX_DECODE_SHARDS, true, flags,
           shards(shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride)};
    c.rs = false;
    c.null_arg = !present_mask;
    c.words[0] = {present_mask, block_status};
    const int rc = check_call(ctx, c, nullptr);
    if (rc != kRun) return rc;
    if (flags == FEC_DEVICE) return xor_reconstruct_device(ctx, k, c.s, {present_mask, 1, block_status, ctx->d_err});
    return host_reconstruct_xor(ctx, k, c.s, present_mask, block_status);
}

}  // extern "C"
