// fec_host.cpp — the host-resident path of the C ABI (fec_ctx.hpp).
// FEC_HOST (pageable host memory): each chunk of blocks is staged by the calling thread into a
// pinned buffer, copied up with one hipMemcpyAsync, coded, copied down with one, and its results
// copied out once its set comes round again. FEC_HOST_PINNED (the caller's buffers are pinned or
// registered): no staging copies; the caller's span of a chunk goes up in one linear DMA and is
// repacked into 16-byte slots on the device (or one 2D DMA per shard column when the span is
// sparse), and packed outputs come down the same way. Only what the code needs crosses PCIe:
// encode sends the k data shards and returns the m parity shards; reconstruct sends the data
// shards and the parity planes its blocks read, and returns only the rebuilt shards. Chunks run
// through HostPipe's three streams (up / kernels / down), kHostSets at a time.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>

#include "fec_ctx.hpp"
#include "fec_kernels.hpp"

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

static int grow_dev(uint8_t** p, size_t* cap, size_t bytes) { return grow_bufs(cap, bytes, 1, {{(void**)p, false}}); }

// Bytes of the caller's span of nb blocks (shards of len bytes, cols per block).
static size_t span_bytes(size_t nb, size_t cols, size_t bs, size_t ss, size_t len) {
    return (nb - 1) * bs + (cols - 1) * ss + len;
}

// A span worth one linear copy: at most a quarter more bytes than the shards themselves.
static bool dense_span(size_t nb, size_t cols, size_t bs, size_t ss, size_t len) {
    return span_bytes(nb, cols, bs, ss, len) * 4 <= nb * cols * len * 5;
}

// The data columns [0, cols) of the caller's blocks `src` toward the device stage `st`, on stream
// `up`: when the span of all span_cols >= cols columns is dense, one linear DMA of it into `raw`
// (a few unneeded columns ride along: one linear DMA beats narrow 2D rows) and *repack = true (the
// kernel stream then runs pinned_repack); else one 2D DMA per column straight into the stage.
static int pinned_up(hipStream_t up, const Shards& st, const Shards& src, size_t cols, uint8_t* raw, size_t span_cols,
                     bool* repack) {
    *repack = dense_span(src.nblocks, span_cols, src.dbs, src.ss, src.len);
    if (*repack) {
        const size_t span = span_bytes(src.nblocks, span_cols, src.dbs, src.ss, src.len);
        HIP_TRY(hipMemcpyAsync(raw, src.data, span, hipMemcpyHostToDevice, up));
        return FEC_OK;
    }
    for (size_t j = 0; j < cols; ++j)
        HIP_TRY(hipMemcpy2DAsync(st.shard(0, j), st.dbs, src.shard(0, j), src.dbs, src.len, src.nblocks,
                                 hipMemcpyHostToDevice, up));
    return FEC_OK;
}

// The caller layout's outputs are packed (no bytes between shards): the kernel stream packs the
// device stage into one image that goes down in one linear DMA.
static bool packed_out(size_t bs, size_t ss, size_t cols, size_t len) { return ss == len && bs == cols * len; }

// The parity columns [0, cols) of the device stage `st` back to the caller's blocks `dst`, on stream
// `down`: the packed image (packed_out) in one linear DMA, else one 2D DMA per column, which writes
// exactly len bytes per shard.
static int pinned_down(hipStream_t down, const Shards& dst, const Shards& st, size_t cols, const uint8_t* raw) {
    if (packed_out(dst.pbs, dst.pss, cols, dst.len)) {
        HIP_TRY(hipMemcpyAsync(dst.parity, raw, dst.nblocks * cols * dst.len, hipMemcpyDeviceToHost, down));
        return FEC_OK;
    }
    for (size_t j = 0; j < cols; ++j)
        HIP_TRY(hipMemcpy2DAsync(dst.par(0, j), dst.pbs, st.par(0, j), st.pbs, dst.len, dst.nblocks,
                                 hipMemcpyDeviceToHost, down));
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
        if ((rc = grow_bufs(&s.in_cap, in_bytes, 1, {{(void**)&s.h_in, true}, {(void**)&s.d_in, false}}))) return rc;
        if ((rc = grow_bufs(&s.out_cap, out_bytes, 1, {{(void**)&s.h_out, true}, {(void**)&s.d_out, false}})))
            return rc;
        if ((rc = grow_bufs(&s.blk_cap, blocks, 4, {{(void**)&s.h_masks, true}, {(void**)&s.h_status, true},
                                                    {(void**)&s.d_masks, false}, {(void**)&s.d_status, false}})))
            return rc;
    }
    return FEC_OK;
}

hipError_t host_set_free(HostSet& s) {
    hipError_t first = hipSuccess;
    auto drop = [&first](hipError_t e) {
        if (e != hipSuccess && first == hipSuccess) first = e;
    };
    for (void* q : {(void*)s.h_in, (void*)s.h_out, (void*)s.h_masks, (void*)s.h_status})
        if (q) drop(hipHostFree(q));
    for (void* q : {(void*)s.d_in, (void*)s.d_out, (void*)s.d_masks, (void*)s.d_status, (void*)s.d_raw_in,
                    (void*)s.d_raw_out})
        if (q) drop(hipFree(q));
    s.h_in = s.h_out = s.d_in = s.d_out = s.d_raw_in = s.d_raw_out = nullptr;
    s.h_masks = s.d_masks = nullptr;
    s.h_status = s.d_status = nullptr;
    s.in_cap = s.out_cap = s.blk_cap = s.raw_in_cap = s.raw_out_cap = 0;
    return first;
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

// Encode (RS when code != nullptr, else XOR(k, 1)): host data -> host parity. A chunk is staged
// block-major, its data as [nb][k][ssd] in the set's in buffers and its parity as [nb][m][ssd] in the
// out buffers.
int host_encode(fec_ctx* ctx, Code* code, int k, int m, const Shards& s, bool pinned) {
    const size_t len = s.len, ssd = round16(len);
    const size_t chunk = host_chunk_blocks(s.nblocks, (size_t)k * ssd);
    HostPipe& p = ctx->pipe;
    int rc;
    if ((rc = host_pipe_grow(p, chunk * k * ssd, chunk * m * ssd, 1))) return rc;
    const bool pack = pinned && packed_out(s.pbs, s.pss, (size_t)m, len);
    if (pinned)
        for (HostSet& hs : p.set) {
            if ((rc = grow_dev(&hs.d_raw_in, &hs.raw_in_cap, span_bytes(chunk, k, s.dbs, s.ss, len) + 16))) return rc;
            if (pack && (rc = grow_dev(&hs.d_raw_out, &hs.raw_out_cap, chunk * m * len + 16))) return rc;
        }
    auto staged = [&](uint8_t* in, uint8_t* out, size_t nb) -> Shards {
        return {len, nb, in, (size_t)k * ssd, out, (size_t)m * ssd, ssd, ssd};
    };
    auto up = [&](HostSet& hs, HostChunk& ch) -> int {
        const Shards src = s.blocks(ch.b0, ch.nb);
        if (pinned) return pinned_up(p.up, staged(hs.d_in, hs.d_out, ch.nb), src, k, hs.d_raw_in, k, &ch.repack);
        const Shards h = staged(hs.h_in, hs.h_out, ch.nb);
        parallel_for(ch.nb, [&](size_t lo, size_t hi) {
            for (size_t b = lo; b < hi; ++b)
                for (int j = 0; j < k; ++j) memcpy(h.shard(b, j), src.shard(b, j), len);
        });
        HIP_TRY(hipMemcpyAsync(hs.d_in, hs.h_in, ch.nb * k * ssd, hipMemcpyHostToDevice, p.up));
        return FEC_OK;
    };
    auto kern = [&](HostSet& hs, HostChunk& ch) -> int {
        const Shards st = staged(hs.d_in, hs.d_out, ch.nb);
        if (ch.repack)
            HIP_TRY(fk::launch_span_to_stage(st.data, st.dbs, st.ss, hs.d_raw_in, s.dbs, s.ss, (uint32_t)ch.nb,
                                             (uint32_t)k, (uint32_t)len, p.comp));
        const int r =
            on_pipe(ctx, [&] { return code ? rs_encode_device(ctx, code, st) : xor_encode_device(ctx, k, st); });
        if (r) return r;
        if (pack)
            HIP_TRY(fk::launch_stage_to_packed(hs.d_raw_out, st.parity, st.pbs, st.pss, (uint32_t)ch.nb, (uint32_t)m,
                                               (uint32_t)len, p.comp));
        return FEC_OK;
    };
    auto down = [&](HostSet& hs, HostChunk& ch) -> int {
        if (pinned)
            return pinned_down(p.down, s.blocks(ch.b0, ch.nb), staged(hs.d_in, hs.d_out, ch.nb), m, hs.d_raw_out);
        HIP_TRY(hipMemcpyAsync(hs.h_out, hs.d_out, ch.nb * m * ssd, hipMemcpyDeviceToHost, p.down));
        return FEC_OK;
    };
    auto finish = [&](HostSet& hs, HostChunk& ch) -> int {
        if (pinned) return FEC_OK;
        const Shards dst = s.blocks(ch.b0, ch.nb), h = staged(hs.h_in, hs.h_out, ch.nb);
        parallel_for(ch.nb, [&](size_t lo, size_t hi) {
            for (size_t b = lo; b < hi; ++b)
                for (int r = 0; r < m; ++r) memcpy(dst.par(b, r), h.par(b, r), len);
        });
        return FEC_OK;
    };
    return host_pipeline(ctx, s.nblocks, chunk, up, kern, down, finish);
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
int host_reconstruct_rs(fec_ctx* ctx, Code* code, const Shards& s, const uint32_t* masks, int32_t* block_status,
                        bool pinned) {
    const int k = code->k, m = code->m;
    const size_t len = s.len, ssd = round16(len);
    const size_t n = (size_t)k + m;
    const uint32_t all = fk::low_mask((uint32_t)n), kmask = fk::low_mask((uint32_t)k);
    const size_t maxe = (size_t)std::max(1, std::min(k, m));
    const size_t chunk = host_chunk_blocks(s.nblocks, n * ssd);
    HostPipe& p = ctx->pipe;
    int rc;
    if ((rc = host_pipe_grow(p, chunk * n * ssd, chunk * maxe * ssd, chunk))) return rc;
    if (pinned)
        for (HostSet& hs : p.set)
            if ((rc = grow_dev(&hs.d_raw_in, &hs.raw_in_cap, span_bytes(chunk, k, s.dbs, s.ss, len) + 16))) return rc;
    // the sticky device word of the host path: statuses report every per-block failure, but a plan
    // kernel that cannot run (fec_plan.hip form 3's LDS-alignment guard, bit 4) writes no statuses
    HIP_TRY(hipMemsetAsync(ctx->d_err + 1, 0, sizeof(int), p.comp));
    bool failed = false, singular = false;   // (singular: blocks of a custom code, fec_solve.hpp)
    // A chunk's stage in a set's in buffer at `in`: the data block-major, [nb][k][ssd], then the parity
    // plane-major, [P][nb][ssd], so that only the planes a chunk reads cross PCIe.
    auto staged = [&](uint8_t* in, size_t nb) -> Shards {
        return {len, nb, in, (size_t)k * ssd, in + nb * k * ssd, /*pbs*/ ssd, /*ss*/ ssd, /*pss*/ nb * ssd};
    };
    auto up = [&](HostSet& hs, HostChunk& ch) -> int {
        const size_t nb = ch.nb;
        const Shards src = s.blocks(ch.b0, nb), st = staged(hs.d_in, nb);
        // per block: the parity planes its first k present shards reach, its erasure count
        uint32_t needers[32] = {};
        for (size_t b = 0; b < nb; ++b) {
            const uint32_t mask = masks[ch.b0 + b] & all;
            hs.h_masks[b] = mask;
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
        HIP_TRY(hipMemcpyAsync(hs.d_masks, hs.h_masks, nb * 4, hipMemcpyHostToDevice, p.up));
        if (pinned) {
            if ((rc = pinned_up(p.up, st, src, k, hs.d_raw_in, k, &ch.repack))) return rc;
            // the device reads sparse planes straight out of the caller's pinned buffer (needs a
            // device mapping of it; otherwise every plane goes by DMA)
            const uint8_t* dpar = nullptr;
            const bool mapped = ch.planes && hipHostGetDevicePointer((void**)&dpar, src.parity, 0) == hipSuccess && dpar;
            if (ch.planes && !mapped) (void)hipGetLastError();
            for (size_t r = 0; r < ch.planes; ++r) {
                const bool sparse = needers[r] * 4 < nb * 3;
                if (mapped && sparse) {
                    ch.gather |= 1u << r;
                    continue;
                }
                HIP_TRY(hipMemcpy2DAsync(st.par(0, r), st.pbs, src.par(0, r), src.pbs, len, nb, hipMemcpyHostToDevice,
                                         p.up));
            }
            return FEC_OK;
        }
        const size_t P = ch.planes;
        const Shards h = staged(hs.h_in, nb);
        parallel_for(nb, [&](size_t lo, size_t hi) {
            for (size_t b = lo; b < hi; ++b) {
                const uint32_t mask = hs.h_masks[b];
                if ((mask & kmask) == kmask) continue;   // nothing to rebuild: nothing read
                for (int j = 0; j < k; ++j)
                    if ((mask >> j) & 1u) memcpy(h.shard(b, j), src.shard(b, j), len);
                for (size_t r = 0; r < P; ++r)
                    if ((mask >> (k + r)) & 1u) memcpy(h.par(b, r), src.par(b, r), len);
            }
        });
        HIP_TRY(hipMemcpyAsync(hs.d_in, hs.h_in, (nb * k + P * nb) * ssd, hipMemcpyHostToDevice, p.up));
        return FEC_OK;
    };
    auto kern = [&](HostSet& hs, HostChunk& ch) -> int {
        const size_t nb = ch.nb;
        const Shards st = staged(hs.d_in, nb);
        if (ch.repack)
            HIP_TRY(fk::launch_span_to_stage(st.data, st.dbs, st.ss, hs.d_raw_in, s.dbs, s.ss, (uint32_t)nb, (uint32_t)k,
                                             (uint32_t)len, p.comp));
        if (ch.gather) {
            const uint8_t* dpar = nullptr;
            HIP_TRY(hipHostGetDevicePointer((void**)&dpar, s.blocks(ch.b0, nb).parity, 0));
            HIP_TRY(fk::launch_gather_planes(dpar, s.pbs, s.pss, (uint32_t)len, hs.d_masks, (uint32_t)nb,
                                             (uint32_t)ch.planes, ch.gather, (uint32_t)k, st.parity, st.pbs, p.comp));
        }
        return on_pipe(ctx, [&] {
            return rs_reconstruct_device(ctx, code,
                                         {st, {hs.d_masks, 1, hs.d_status, ctx->d_err + 1},
                                          {hs.d_out, ch.slots * ssd, (uint32_t)ch.slots}});
        });
    };
    auto down = [&](HostSet& hs, HostChunk& ch) -> int {
        HIP_TRY(hipMemcpyAsync(hs.h_out, hs.d_out, ch.nb * ch.slots * ssd, hipMemcpyDeviceToHost, p.down));
        HIP_TRY(hipMemcpyAsync(hs.h_status, hs.d_status, ch.nb * 4, hipMemcpyDeviceToHost, p.down));
        return FEC_OK;
    };
    auto finish = [&](HostSet& hs, HostChunk& ch) -> int {
        for (size_t b = 0; b < ch.nb; ++b) {
            const int32_t st = hs.h_status[b];
            if (block_status) block_status[ch.b0 + b] = st < 0 ? st : 0;
            if (st == fk::kStSingular) singular = true;
            else if (st < 0) failed = true;
        }
        const Shards dst = s.blocks(ch.b0, ch.nb);
        parallel_for(ch.nb, [&](size_t lo, size_t hi) {
            for (size_t b = lo; b < hi; ++b) {
                const int32_t st = hs.h_status[b];
                const uint32_t mask = hs.h_masks[b];
                for (int j = 0, r = 0; j < k && r < st; ++j)
                    if (!((mask >> j) & 1u)) memcpy(dst.shard(b, j), hs.h_out + (b * ch.slots + r++) * ssd, len);
            }
        });
        return FEC_OK;
    };
    if ((rc = host_pipeline(ctx, s.nblocks, chunk, up, kern, down, finish))) return rc;
    int err = 0;
    HIP_TRY(hipMemcpyAsync(&err, ctx->d_err + 1, sizeof(int), hipMemcpyDeviceToHost, p.comp));
    HIP_TRY(hipStreamSynchronize(p.comp));
    if ((rc = fk::sticky_rc(err & fk::kStickyInternal))) return rc;
    return failed ? FEC_ERR_TOO_FEW_SHARDS : singular ? FEC_ERR_SINGULAR : FEC_OK;
}

// The plain form of a FEC_HOST reconstruct, not pipelined: XOR(k,1) (the scheme mirror's per-block
// recovery) and wide RS (it exists so that the scheme layer decodes wide codes; it is PCIe-bound).
// Present masks of mask_words words per block, bits at and above n ignored. Each chunk of blocks
// goes as [block][n][ssd] through the ctx's pinned and device stage (a block with every data shard
// present is not staged: the kernels load a block's shards only to rebuild one of them), is rebuilt
// in place on the device by core(the device stage's layout, its masks and statuses), and the rebuilt
// data shards of the blocks that succeeded are copied back. A block fails exactly when its status is
// not 0 (fec_xor.hip and fec_wide.hip set the sticky word d_err[1] with such a status, never
// without).
template <class Core>
static int host_reconstruct_plain(fec_ctx* ctx, size_t k, size_t n, const Shards& s, const uint32_t* masks,
                                  size_t mask_words, int32_t* block_status, Core core) {
    const size_t len = s.len, ssd = round16(len);
    const size_t chunk = host_chunk_blocks(s.nblocks, n * ssd);
    int rc;
    if ((rc = grow_stage(ctx, chunk * n * ssd))) return rc;
    if ((rc = grow_masks(ctx, chunk * mask_words))) return rc;
    HIP_TRY(hipMemsetAsync(ctx->d_err + 1, 0, sizeof(int), ctx->stream));   // (the kernels OR into it)
    auto present = [&](size_t b, size_t i) { return (masks[b * mask_words + i / 32] >> (i % 32)) & 1u; };
    auto staged = [&](uint8_t* base, size_t nb) -> Shards {
        return {len, nb, base, n * ssd, base + k * ssd, n * ssd, ssd, ssd};
    };
    // shard i of the n of block b: data shard i, or parity shard i - k
    auto shard = [&](const Shards& x, size_t b, size_t i) { return i < k ? x.shard(b, i) : x.par(b, i - k); };
    std::vector<int32_t> st;
    bool failed = false;
    for (size_t b0 = 0; b0 < s.nblocks; b0 += chunk) {
        const size_t nb = std::min(chunk, s.nblocks - b0);
        const Shards src = s.blocks(b0, nb), h = staged(ctx->h_stage, nb);
        for (size_t b = 0; b < nb; ++b) {
            size_t have = 0;
            while (have < k && present(b0 + b, have)) ++have;
            if (have == k) continue;   // nothing to rebuild: nothing read
            for (size_t i = 0; i < n; ++i)
                if (present(b0 + b, i)) memcpy(shard(h, b, i), shard(src, b, i), len);
        }
        HIP_TRY(hipMemcpyAsync(ctx->d_masks, masks + b0 * mask_words, nb * mask_words * 4, hipMemcpyHostToDevice,
                               ctx->stream));
        HIP_TRY(hipMemcpyAsync(ctx->d_stage, ctx->h_stage, nb * n * ssd, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = core(staged(ctx->d_stage, nb), DecodeWords{ctx->d_masks, mask_words, ctx->d_status, ctx->d_err + 1})))
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
            for (size_t i = 0; i < k; ++i)
                if (!present(b0 + b, i)) memcpy(src.shard(b, i), h.shard(b, i), len);
        }
    }
    return failed ? FEC_ERR_TOO_FEW_SHARDS : FEC_OK;
}

int host_reconstruct_xor(fec_ctx* ctx, int k, const Shards& s, const uint32_t* masks, int32_t* block_status) {
    return host_reconstruct_plain(ctx, k, (size_t)k + 1, s, masks, 1, block_status,
                                  [&](const Shards& st, const DecodeWords& w) {
                                      return xor_reconstruct_device(ctx, k, st, w);
                                  });
}

int host_reconstruct_wide(fec_ctx* ctx, int k, int m, const Shards& s, const uint32_t* masks, size_t mask_words,
                          int32_t* block_status) {
    return host_reconstruct_plain(ctx, k, (size_t)k + m, s, masks, mask_words, block_status,
                                  [&](const Shards& st, const DecodeWords& w) {
                                      return rs_reconstruct_wide_device(ctx, k, m, {st, w, {}});
                                  });
}

extern "C" {

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

}  // extern "C"
