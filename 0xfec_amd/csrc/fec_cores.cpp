// fec_cores.cpp — the device-memory cores of the C ABI (fec_ctx.hpp): each cuts one call over device
// memory into launches and fills their arguments. The FEC_DEVICE entry points (fec_capi.cpp) call
// them on the caller's regions, the host-resident drivers (fec_host.cpp) on their staging buffers.
#include <string.h>

#include <algorithm>

#include "fec_ctx.hpp"
#include "fec_kernels.hpp"
#include "fec_locate.hpp"
#include "fec_locate_multi.hpp"
#include "fec_locate_partial.hpp"
#include "fec_ragged.hpp"
#include "fec_solve.hpp"
#include "fec_some.hpp"
#include "fec_update.hpp"
#include "fec_verify.hpp"
#include "fec_wide.hpp"

// Workgroups for a flat (block, chunk) item launch: one item per lane (total < 2^31), never an
// empty grid.
static int flat_grid_nonempty(uint32_t total) { return (int)std::max<uint64_t>(1, fk::flat_grid<uint64_t>(total)); }

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
static void fill_row_pass(Args& a, const Code* code, int r0, const Shards& sl) {
    a.in = sl.data;
    a.in_bs = sl.dbs;
    a.ss = sl.ss;
    a.k = (uint32_t)code->k;
    a.m = (uint32_t)std::min(16, code->m - r0);
    a.tabs = code->d_tabs + (size_t)r0 * code->k * 8;
}

// The item fields of a flat launch over the slice's blocks.
template <class Args>
static void fill_flat(Args& a, const Shards& sl) {
    a.len = (uint32_t)sl.len;
    a.cps = chunks_of(sl.len);
    a.total = (uint32_t)(sl.nblocks * a.cps);
    a.div_cps = fk::make_fastdiv(a.cps);
}

// A launch that starts from the stored parity (SyndromeArgs; UpdateArgs; LocateArgs, which then sets
// its own m and tables) over one slice of a call: the row pass from r0, the parity from that row, the
// item fields.
template <class Args>
static void fill_syndrome(Args& a, const Code* code, int r0, const Shards& sl) {
    fill_row_pass(a, code, r0, sl);
    a.par = sl.par(0, r0);
    a.par_bs = sl.pbs;
    fill_flat(a, sl);
}

// The slices of a batch whose launches keep no plan records: sl = s.blocks(b0, nb) for body(sl, b0).
template <class F>
static int for_flat_slices(const Shards& s, F body) {
    return for_slices(s.nblocks, blocks_per_launch(s.nblocks, chunks_of(s.len)),
                      [&](size_t b0, size_t nb) -> int { return body(s.blocks(b0, nb), b0); });
}

int rs_encode_device(fec_ctx* ctx, Code* code, const Shards& s) {
    const int k = code->k;
    return for_flat_slices(s, [&](const Shards& sl, size_t) -> int {
        for (int r0 = 0; r0 < code->m; r0 += 16) {
            fk::EncodeArgs a{};
            fill_row_pass(a, code, r0, sl);
            a.out = sl.par(0, r0);
            a.out_bs = sl.pbs;
            fill_flat(a, sl);
            a.dytabs = (r0 == 0 && (int)a.m == code->m) ? code->d_dytabs.p : nullptr;
            a.sp = fk::encode_store_policy(fk::g_tune.st_pol, {s.data, s.dbs, s.ss, (uint64_t)k},
                                           {s.parity, s.pbs, s.pss, (uint64_t)code->m}, s.len, s.nblocks);
            // (the fixed shapes are chosen by this code's own matrix: its kind, and for RS(2,3) its row)
            // (a custom code: none, whatever its rows are)
            const fk::FixedEncode fx = fk::fixed_encode((uint32_t)k, a.m, a.dytabs != nullptr, code->kind,
                                                        code->matrix.data() + (size_t)k * k);
            if (fx != fk::FixedEncode::none) {
                HIP_TRY(fk::launch_rs_encode_fixed(a, fx, code->kind, ctx->stream));
                continue;
            }
            HIP_TRY(fk::launch_rs_encode(a, flat_grid_nonempty(a.total), ctx->stream));
        }
        return FEC_OK;
    });
}

// The plan kernels of a code: a custom matrix takes its records from the elimination plan
// (fec_plan_solve.hip), the same records in the same order; the rebuild kernels do not tell.
static hipError_t launch_plan(const Code* code, const fk::PlanArgs& p, bool sorted, hipStream_t s) {
    if (code->solve) return fk::launch_rs_plan_solve(p, sorted, s);
    return sorted ? fk::launch_rs_plan_sorted(p, s) : fk::launch_rs_plan(p, s);
}

// What a slice's PlanArgs and ReconArgs hold in the uniform and the ragged reconstruct alike: the
// slice c of the call, records of layout `lay` in the stream's workspace, tiles of G blocks.
static void fill_recon_slice(fk::PlanArgs& p, fk::ReconArgs& a, fec_ctx* ctx, const Code* code, const ReconCall& c,
                             uint32_t maxe, const fk::PlanLayout& lay, uint32_t G) {
    p.masks = c.w.masks;
    p.plans = ctx->work->d_plans;
    p.status = c.w.status;
    p.err = c.w.err;
    p.prows = code->d_prows;
    p.k = (uint32_t)code->k;
    p.m = (uint32_t)code->m;
    p.nblocks = (uint32_t)c.s.nblocks;
    p.maxe = maxe;
    p.lay = lay;
    p.max_out = c.out.base ? c.out.slots : 0;
    p.dall = code->d_dall;   // (read by the sorted plans only)
    p.logv = code->d_logv;   // (null for the default matrix)
    a.data = c.s.data;
    a.parity = c.s.parity;
    a.dbs = c.s.dbs;
    a.pbs = c.s.pbs;
    a.ss = c.s.ss;
    a.pss = c.s.pss;
    a.plans = ctx->work->d_plans;
    a.k = p.k;
    a.len = (uint32_t)c.s.len;
    a.cps = chunks_of(c.s.len);
    a.nblocks = p.nblocks;
    a.maxe = maxe;
    a.lay = lay;
    a.g = G;
    a.ntiles = (uint32_t)((c.s.nblocks + G - 1) / G);
    a.div_cps = fk::make_fastdiv(a.cps);
    a.out = c.out.base;
    a.out_bs = c.out.bs;
}

int rs_reconstruct_device(fec_ctx* ctx, Code* code, const ReconCall& call) {
    const Shards& s = call.s;
    const OutRegion& out = call.out;
    if ((s.ss | s.pss) >> 32) return FEC_ERR_INVALID_ARG;   // the rebuild kernels take 32-bit shard strides
    const uint32_t k = (uint32_t)code->k, m = (uint32_t)code->m;
    const uint32_t maxe = std::max<uint32_t>(1, std::min(k, m));
    const uint32_t cps = chunks_of(s.len);
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
    // A custom code has the single-erasure tables, and so the direct and the routed form, only if no
    // entry of its parity rows is zero (get_code); its plans come from launch_plan.
    const bool single_slot = out.base && out.slots == 1;
    const bool direct = code->d_single_coef && fk::direct_recon_applies(k, m, cps, single_slot);
    const bool wave = !direct && fk::wave_recon_applies(cps, k, maxe, lay_sorted.stride);
    const bool routed = wave && !out.base && code->d_single_coef && !fk::rebuild_k_applies(k, maxe, cps) &&
                        fk::routed_recon_applies(k, m, cps, maxe, lay_sorted.stride);
    const fk::PlanLayout lay = wave ? lay_sorted : lay_block;
    const size_t per_launch = blocks_per_launch(s.nblocks, cps, direct ? 0 : lay.stride);
    if (!direct) {
        const int rc = grow_plans(ctx, per_launch * lay.stride);
        if (rc) return rc;
    }
    if (routed) {
        const int rc = grow_wflags(ctx, 1);
        if (rc) return rc;
    }
    const uint32_t G = fk::pick_tile_blocks(cps, k, maxe, lay);
    return for_slices(s.nblocks, per_launch, [&](size_t b0, size_t nb) -> int {
        fk::PlanArgs p{};
        fk::ReconArgs a{};
        fill_recon_slice(p, a, ctx, code, call.blocks(b0, nb), maxe, lay, G);
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
            a.sp = fk::decode_store_policy(fk::g_tune.dst_pol, {s.data, s.dbs, s.ss, k}, {s.parity, s.pbs, s.pss, m},
                                           {out.base, out.bs, s.ss, out.slots}, s.len, s.nblocks);
        }
        if (direct) {
            HIP_TRY(fk::launch_rs_recover_direct(a, ctx->stream));
        } else if (routed) {
            a.route = p.route = ctx->work->d_wflags;
            HIP_TRY(fk::launch_rs_route_classify(a, ctx->work->d_wflags, ctx->stream));
            HIP_TRY(launch_plan(code, p, true, ctx->stream));
            HIP_TRY(fk::launch_rs_reconstruct_routed(a, ctx->stream));
        } else if (wave) {
            HIP_TRY(launch_plan(code, p, true, ctx->stream));
            if (fk::rebuild_k_applies(k, maxe, cps)) HIP_TRY(fk::launch_rs_rebuild_k(a, ctx->stream));
            else HIP_TRY(fk::launch_rs_reconstruct_wave(a, ctx->stream));
        } else {
            HIP_TRY(launch_plan(code, p, false, ctx->stream));
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
static int rs_rebuild_tiles(fec_ctx* ctx, uint32_t k, uint32_t rows, const Shards& s, const OutRegion& out, bool some,
                            Plan plan) {
    if (s.ss >> 32) return FEC_ERR_INVALID_ARG;   // the rebuild kernel takes 32-bit shard strides
    const uint32_t cps = chunks_of(s.len);
    const fk::WideLayout lay = fk::wide_layout(k, rows);
    const size_t per_launch = blocks_per_launch(s.nblocks, cps, lay.stride);
    const int rc = grow_plans(ctx, per_launch * lay.stride);
    if (rc) return rc;
    uint32_t G, C, TK;
    fk::wide_tile_shape(cps, k, &G, &C, &TK);
    return for_slices(s.nblocks, per_launch, [&](size_t b0, size_t nb) -> int {
        const Shards sl = s.blocks(b0, nb);
        fk::WideReconArgs a{};
        a.data = sl.data;
        a.parity = sl.parity;
        a.dbs = sl.dbs;
        a.pbs = sl.pbs;
        a.ss = (uint32_t)sl.ss;
        a.plans = ctx->work->d_plans;
        a.lay = lay;
        a.k = k;
        a.len = (uint32_t)sl.len;
        a.cps = cps;
        a.nblocks = (uint32_t)nb;
        a.g = G;
        a.c = C;
        a.tk = TK;
        a.nctiles = (cps + C - 1) / C;
        a.ntiles = (uint32_t)((nb + G - 1) / G) * a.nctiles;
        a.div_c = fk::make_fastdiv(C);
        a.div_nct = fk::make_fastdiv(a.nctiles);
        a.out = out.blocks(b0).base;
        a.out_bs = out.bs;
        HIP_TRY(plan(b0, nb, lay));
        HIP_TRY(fk::launch_rs_rebuild_wide(a, some, ctx->stream));
        return FEC_OK;
    });
}

// The wide plan kernel (fec_wide.hip rs_plan_wide_kernel) for one launch slice of nb blocks from
// block b0: records of `rows` rows into the stream's workspace. some: the reconstruct-some form, with
// want masks (null: every shard) strided like the present masks; else the reconstruct / recover
// form with max_out output slots (0: in place).
static hipError_t plan_wide_slice(fec_ctx* ctx, uint32_t k, uint32_t m, uint32_t rows, const DecodeWords& words,
                                  const uint32_t* want, uint32_t max_out, bool some, size_t b0, size_t nb,
                                  const fk::WideLayout& lay, const uint8_t* logv) {
    const DecodeWords w = words.blocks(b0);
    fk::WidePlanArgs p{};
    p.masks = w.masks;
    p.mask_words = (uint32_t)w.mask_words;
    p.want = want ? want + b0 * w.mask_words : nullptr;
    p.plans = ctx->work->d_plans;
    p.status = w.status;
    p.err = w.err;
    p.k = k;
    p.n = k + m;
    p.nblocks = (uint32_t)nb;
    p.rows = rows;
    p.max_out = max_out;
    p.lay = lay;
    p.div_k = fk::make_fastdiv(k);
    p.logv = logv;
    return fk::launch_rs_plan_wide(p, some, ctx->stream);
}

// The log v table of the ctx's code for (k, m), for the plan kernels that take no Code (null for the
// default matrix). The entry points have looked the code up already, so this finds it cached.
static int code_logv(fec_ctx* ctx, int k, int m, const uint8_t** logv) {
    Code* code = nullptr;
    const int rc = get_code(ctx, k, m, &code);
    if (rc) return rc;
    *logv = code->d_logv;
    return FEC_OK;
}

// Wide reconstruct / recover (fec_wide.hip): present masks of mask_words words per block, codes of
// up to 256 shards.
int rs_reconstruct_wide_device(fec_ctx* ctx, int ki, int mi, const ReconCall& c) {
    const uint32_t k = (uint32_t)ki, m = (uint32_t)mi;
    const uint8_t* logv = nullptr;
    const int rc = code_logv(ctx, ki, mi, &logv);
    if (rc) return rc;
    uint32_t rows = std::max<uint32_t>(1, std::min(k, m));
    if (c.out.base) rows = std::min(rows, c.out.slots);
    const uint32_t max_out = c.out.base ? c.out.slots : 0;
    return rs_rebuild_tiles(ctx, k, rows, c.s, c.out, false,
                            [&](size_t b0, size_t nb, const fk::WideLayout& lay) {
                                return plan_wide_slice(ctx, k, m, rows, c.w, nullptr, max_out, false, b0, nb, lay,
                                                       logv);
                            });
}

// Verify (fec_verify.hip): statuses pre-set to 1 and the count to 0 on the stream, then the encode's
// launches (cut under kMaxItems items, parity rows in passes of 16) with the stored parity folded
// in: a pass clears the word of a block it finds bad and counts it if no earlier pass had.
int rs_verify_device(fec_ctx* ctx, Code* code, const Shards& s, int32_t* status, uint32_t* count) {
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)status, 1, s.nblocks, ctx->stream));
    if (count) HIP_TRY(hipMemsetAsync(count, 0, sizeof(uint32_t), ctx->stream));
    return for_flat_slices(s, [&](const Shards& sl, size_t b0) -> int {
        for (int r0 = 0; r0 < code->m; r0 += 16) {
            fk::VerifyArgs a{};
            fill_syndrome(a, code, r0, sl);
            a.status = status + b0;
            a.count = count;
            HIP_TRY(fk::launch_rs_verify(a, flat_grid_nonempty(a.total), ctx->stream));
        }
        return FEC_OK;
    });
}

// Update and encode-idx (fec_update.hip; UpdateCall, fec_ctx.hpp, holds a call's regions and masks).
// The arguments of one launch: blocks [b0, b0 + nb) of the call, the pass of up to 16 parity rows
// from r0. No device work (fec__selftest_update_slices calls it without one).
static void fill_update_launch(fk::UpdateArgs& a, const Code* code, int r0, const Shards& sl, size_t b0,
                               const UpdateCall& u) {
    fill_syndrome(a, code, r0, sl);
    a.old = u.old.blocks(b0).base;
    a.old_bs = u.old.bs;
    a.nblocks = (uint32_t)sl.nblocks;
    a.masks = u.masks + b0 * u.mask_words;
    a.mask_words = (uint32_t)u.mask_words;
}

// emit(args) for every launch of a call: the encode's cut under kMaxItems items, parity rows in
// passes of 16 (each pass reads the masked columns again), until one fails.
template <class F>
static int update_launches(const Code* code, const UpdateCall& u, F emit) {
    return for_flat_slices(u.s, [&](const Shards& sl, size_t b0) -> int {
        for (int r0 = 0; r0 < code->m; r0 += 16) {
            fk::UpdateArgs a{};
            fill_update_launch(a, code, r0, sl, b0, u);
            const int rc = emit(a);
            if (rc) return rc;
        }
        return FEC_OK;
    });
}

int rs_update_device(fec_ctx* ctx, const Code* code, const UpdateCall& u) {
    return update_launches(code, u, [&](const fk::UpdateArgs& a) -> int {
        HIP_TRY(fk::launch_rs_update(a, flat_grid_nonempty(a.total), ctx->stream));
        return FEC_OK;
    });
}

// Locate (fec_locate.hip; LocateCall, fec_ctx.hpp, holds a call's regions and outputs). pass(args)
// for every kernel launch of a call and fin(args) once per slice after its passes, until one fails:
// verify's cut under kMaxItems items; each pass takes parity row 0 and up to 15 rows from
// r0 = 1, 16, 31, ... (a code of one parity row: row 0 alone; of none: no pass). No device work
// (fec__selftest_locate_slices calls it without one).
template <class P, class F>
static int locate_launches(const Code* code, const LocateCall& c, P pass, F fin) {
    return for_flat_slices(c.s, [&](const Shards& sl, size_t b0) -> int {
        for (int r0 = 1; code->m > 0 && (r0 == 1 || r0 < code->m); r0 += fk::kLocateRows - 1) {
            fk::LocateArgs a{};
            fill_syndrome(a, code, 0, sl);
            a.m = (uint32_t)code->m;
            a.r0 = (uint32_t)r0;
            a.rows = 1u + (uint32_t)std::min(fk::kLocateRows - 1, code->m - r0);
            if (r0 > 1 && code->d_loc_carry) {   // the pass's slab: row 0's tables, then its rows'
                a.tabs0 = code->d_loc_carry + (size_t)(r0 / (fk::kLocateRows - 1) - 1) * fk::kLocateRows * code->k * 8;
                a.tabs = a.tabs0 + (size_t)code->k * 8;
            } else {
                a.tabs0 = code->d_tabs;
                a.tabs = code->d_tabs + (size_t)r0 * code->k * 8;
            }
            a.loctab = code->d_loctab;
            a.verdict = c.verdict + b0;
            const int rc = pass(a);
            if (rc) return rc;
        }
        fk::LocateFinArgs f{};
        f.verdict = c.verdict + b0;
        f.present = c.present ? c.present + b0 * c.mask_words : nullptr;
        f.counts = c.counts;
        f.nblocks = (uint32_t)sl.nblocks;
        f.n = (uint32_t)(code->k + code->m);
        f.mask_words = (uint32_t)c.mask_words;
        return fin(f);
    });
}

// Verdicts pre-set to clean and the counts to 0 on the stream, as verify presets its statuses.
int rs_locate_device(fec_ctx* ctx, const Code* code, const LocateCall& c) {
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)c.verdict, fk::kLocateClean, c.s.nblocks, ctx->stream));
    if (c.counts) HIP_TRY(hipMemsetAsync(c.counts, 0, 2 * sizeof(uint32_t), ctx->stream));
    return locate_launches(
        code, c,
        [&](const fk::LocateArgs& a) -> int {
            HIP_TRY(fk::launch_rs_locate(a, flat_grid_nonempty(a.total), ctx->stream));
            return FEC_OK;
        },
        [&](const fk::LocateFinArgs& f) -> int {
            HIP_TRY(fk::launch_rs_locate_finalize(f, ctx->stream));
            return FEC_OK;
        });
}

// Locate-multi (fec_locate_multi.hip; LocateMultiCall, fec_ctx.hpp) and locate-partial
// (fec_locate_partial.hip; LocatePartialCall). A batch is cut as the encode cuts it (kMaxItems items per
// slice), and so that a slice's workspace stays under kPlanBytes: locate_multi_ws_bytes (one bitmap bit
// per item, words + 1 words per block), and for locate-partial `block_extra` bytes per block and
// `slice_extra` per slice on top (fec_locate_partial.hpp locate_partial_ws).
static size_t locate_multi_per_launch(size_t nblocks, uint32_t cps, uint32_t words, size_t block_extra = 0,
                                      size_t slice_extra = 0) {
    const size_t per_block = (size_t)(words + 1) * 4 + (cps + 7) / 8 + block_extra;   // (+ 47 bytes of rounding per slice)
    return std::max<size_t>(1, std::min(blocks_per_launch(nblocks, cps), (kPlanBytes - 64 - slice_extra) / per_block));
}
// locate-partial's: a plan word and m PermTabs per block; the line of zeros and the plan words' rounding.
static size_t locate_partial_per_launch(size_t nblocks, uint32_t cps, uint32_t words, uint32_t m) {
    return locate_multi_per_launch(nblocks, cps, words, 4 + (size_t)m * sizeof(gf::PermTab), 128);
}

// What one slice of a locate-multi call runs, in order: `clear` bytes of the workspace set to zero, the
// scan, the solve, the finalize.
struct LocateMultiSlice {
    size_t clear;
    fk::LocateMultiScanArgs scan;
    fk::LocateMultiSolveArgs solve;
    fk::LocateMultiFinArgs fin;
};

// What one slice of a locate-partial call runs, in order: `clear` bytes of the workspace set to zero,
// the plan, the scan, the solve, the finalize.
struct LocatePartialSlice {
    size_t clear;
    fk::LocatePartialPlanArgs plan;
    fk::LocatePartialScanArgs scan;
    fk::LocatePartialSolveArgs solve;
    fk::LocatePartialFinArgs fin;
};

// What the slices of both calls hold alike, for blocks [b0, b0 + nb) of the call and the workspace at
// ws (the scan's bitmap first, the blocks' words behind it): the scan's flat launch and bitmap, the
// solve's and the finalize's fields but for the radius (locate-multi's) and the plan and masks
// (locate-partial's). solve.s is the caller's to copy from the scan once that is complete.
template <class Slice>
static void fill_locate_slice(Slice& sl, const Code* code, const LocateMultiCall& c, uint8_t* ws, size_t b0, size_t nb) {
    const uint32_t m = (uint32_t)code->m, n = (uint32_t)code->k + m, words = (n + 31) / 32;
    const size_t bitmap = fk::locate_multi_bitmap_bytes((uint64_t)nb * chunks_of(c.s.len));
    fill_syndrome(sl.scan, code, 0, c.s.blocks(b0, nb));   // (m <= 16)
    sl.scan.bitmap = (uint64_t*)ws;
    sl.solve.nwords = (uint32_t)(bitmap / sizeof(uint64_t));
    sl.solve.n = n;
    sl.solve.words = words;
    sl.solve.ft = code->d_lmtab ? (const uint8_t*)(code->d_lmtab + (size_t)m * m * 8) : nullptr;   // (m = 0)
    sl.solve.blk = (uint32_t*)(ws + bitmap);
    sl.fin.blk = sl.solve.blk;
    sl.fin.bad_count = c.bad_count + b0;
    sl.fin.present = c.present ? c.present + b0 * c.mask_words : nullptr;
    sl.fin.counts = c.counts;
    sl.fin.nblocks = (uint32_t)nb;
    sl.fin.n = n;
    sl.fin.words = words;
    sl.fin.mask_words = (uint32_t)c.mask_words;
}

// run(slice) for every slice of a call whose workspace is at ws, until one fails. No device work
// (fec__selftest_locate_multi_slices calls it without one).
template <class R>
static int locate_multi_launches(const Code* code, const LocateMultiCall& c, uint8_t* ws, R run) {
    const size_t nblocks = c.s.nblocks;
    const uint32_t cps = chunks_of(c.s.len);
    const uint32_t words = (uint32_t)(code->k + code->m + 31) / 32;
    const uint32_t T = fk::locate_multi_radius((uint32_t)code->m, (uint32_t)c.max_bad);
    return for_slices(nblocks, locate_multi_per_launch(nblocks, cps, words), [&](size_t b0, size_t nb) -> int {
        LocateMultiSlice sl{};
        sl.clear = fk::locate_multi_ws_bytes(nb, cps, words);
        fill_locate_slice(sl, code, c, ws, b0, nb);
        sl.solve.s = sl.scan;
        sl.solve.T = T;
        sl.solve.atabs = code->d_lmtab;
        sl.fin.T = T;
        return run(sl);
    });
}

// As locate_multi_launches, for a locate-partial call (fec__selftest_locate_partial_slices): on top of
// what both calls hold, the plan launch, the masks, and the workspace's parts behind the blocks' words.
template <class R>
static int locate_partial_launches(const Code* code, const LocatePartialCall& pc, uint8_t* ws, R run) {
    const LocateMultiCall& c = pc.c;
    const size_t nblocks = c.s.nblocks;
    const uint32_t cps = chunks_of(c.s.len);
    const uint32_t m = (uint32_t)code->m, words = (uint32_t)(code->k + code->m + 31) / 32;
    return for_slices(nblocks, locate_partial_per_launch(nblocks, cps, words, m), [&](size_t b0, size_t nb) -> int {
        const fk::PartialWs w = fk::locate_partial_ws(nb, cps, words, m);
        LocatePartialSlice sl{};
        sl.clear = w.plan;
        fill_locate_slice(sl, code, c, ws, b0, nb);
        fk::LocatePartialPlanArgs& p = sl.plan;
        p.masks = pc.masks + b0 * c.mask_words;
        p.plan = (uint32_t*)(ws + w.plan);
        p.ltabs = (uint32_t*)(ws + w.ltabs);
        p.nblocks = (uint32_t)nb;
        p.k = (uint32_t)code->k;
        p.m = m;
        p.max_bad = (uint32_t)c.max_bad;
        p.mask_words = (uint32_t)c.mask_words;
        fk::LocatePartialScanArgs& a = sl.scan;
        a.masks = p.masks;
        a.plan = p.plan;
        a.ltabs = p.ltabs;
        a.atabs = code->d_lmtab;
        a.zeros = ws + w.zeros;
        a.mask_words = p.mask_words;
        sl.solve.s = a;
        sl.fin.plan = p.plan;
        sl.fin.masks = p.masks;
        return run(sl);
    });
}

static int launch_locate_slice(const LocateMultiSlice& sl, hipStream_t s) {
    HIP_TRY(fk::launch_rs_locate_multi_scan(sl.scan, flat_grid_nonempty(sl.scan.total), s));
    HIP_TRY(fk::launch_rs_locate_multi_solve(sl.solve, s));
    HIP_TRY(fk::launch_rs_locate_multi_finalize(sl.fin, s));
    return FEC_OK;
}
static int launch_locate_slice(const LocatePartialSlice& sl, hipStream_t s) {
    HIP_TRY(fk::launch_rs_locate_partial_plan(sl.plan, s));
    HIP_TRY(fk::launch_rs_locate_partial_scan(sl.scan, flat_grid_nonempty(sl.scan.total), s));
    HIP_TRY(fk::launch_rs_locate_partial_solve(sl.solve, s));
    HIP_TRY(fk::launch_rs_locate_partial_finalize(sl.fin, s));
    return FEC_OK;
}

// A call on the device: the stream's workspace (ctx->work) grown to ws_bytes, the call's `ncounts`
// counts set to 0 on the stream, as verify presets its count, then launches(ws, run) with a run that
// clears the slice's part of the workspace and queues its launches. The workspace is the stream's, so
// slices and calls on one stream follow one another in it.
template <class L>
static int locate_slices_device(fec_ctx* ctx, size_t ws_bytes, uint32_t* counts, size_t ncounts, L launches) {
    const int rc = grow_plans(ctx, ws_bytes);
    if (rc) return rc;
    if (counts) HIP_TRY(hipMemsetAsync(counts, 0, ncounts * sizeof(uint32_t), ctx->stream));
    return launches(ctx->work->d_plans, [&](const auto& sl) -> int {
        HIP_TRY(hipMemsetAsync(ctx->work->d_plans, 0, sl.clear, ctx->stream));
        return launch_locate_slice(sl, ctx->stream);
    });
}

int rs_locate_multi_device(fec_ctx* ctx, const Code* code, const LocateMultiCall& c) {
    const uint32_t cps = chunks_of(c.s.len);
    const uint32_t words = (uint32_t)(code->k + code->m + 31) / 32;
    const size_t per = locate_multi_per_launch(c.s.nblocks, cps, words);
    return locate_slices_device(ctx, fk::locate_multi_ws_bytes(per, cps, words), c.counts, 2,
                                [&](uint8_t* ws, auto run) { return locate_multi_launches(code, c, ws, run); });
}

int rs_locate_partial_device(fec_ctx* ctx, const Code* code, const LocatePartialCall& pc) {
    const uint32_t cps = chunks_of(pc.c.s.len);
    const uint32_t m = (uint32_t)code->m, words = (uint32_t)(code->k + code->m + 31) / 32;
    const size_t per = locate_partial_per_launch(pc.c.s.nblocks, cps, words, m);
    return locate_slices_device(ctx, fk::locate_partial_ws(per, cps, words, m).end, pc.c.counts, 3,
                                [&](uint8_t* ws, auto run) { return locate_partial_launches(code, pc, ws, run); });
}

// Reconstruct-some's plan kernel for one launch slice of nb blocks from block b0: records of layout
// `lay` in block order into the stream's workspace, from the present and want masks (want null: every
// shard); a custom code's come from the elimination plan (fec_plan_solve.hip). They do not depend on
// the shard length: the uniform and the ragged call take the same.
static hipError_t plan_some_slice(fec_ctx* ctx, const Code* code, const DecodeWords& words, const uint32_t* want,
                                  size_t b0, size_t nb, const fk::WideLayout& lay) {
    const DecodeWords w = words.blocks(b0);
    fk::SomePlanArgs p{};
    p.masks = w.masks;
    p.want = want ? want + b0 : nullptr;
    p.plans = ctx->work->d_plans;
    p.status = w.status;
    p.err = w.err;
    p.k = (uint32_t)code->k;
    p.n = (uint32_t)(code->k + code->m);
    p.nblocks = (uint32_t)nb;
    p.lay = lay;
    p.logv = code->d_logv;
    if (code->solve) return fk::launch_rs_plan_solve_some({p, code->d_prows}, ctx->stream);
    return fk::launch_rs_plan_some(p, ctx->stream);
}

// Reconstruct-some (fec_some.hip): plan records in block order from the present and want masks, then
// the wide tile, storing into both regions.
int rs_reconstruct_some_device(fec_ctx* ctx, int ki, int mi, const Shards& s, const DecodeWords& words,
                               const uint32_t* want) {
    Code* code = nullptr;   // (the entry point has looked it up already: cached)
    const int rc = get_code(ctx, ki, mi, &code);
    if (rc) return rc;
    return rs_rebuild_tiles(ctx, (uint32_t)ki, fk::some_rows((uint32_t)mi), s, {}, true,
                            [&](size_t b0, size_t nb, const fk::WideLayout& lay) {
                                return plan_some_slice(ctx, code, words, want, b0, nb, lay);
                            });
}

// Wide reconstruct-some (k + m <= 256, masks of mask_words words): the same, with records from the
// wide plan kernel in its reconstruct-some form.
int rs_reconstruct_some_wide_device(fec_ctx* ctx, int ki, int mi, const Shards& s, const DecodeWords& words,
                                    const uint32_t* want) {
    const uint32_t k = (uint32_t)ki, m = (uint32_t)mi;
    const uint32_t rows = fk::some_rows(m);
    const uint8_t* logv = nullptr;
    const int rc = code_logv(ctx, ki, mi, &logv);
    if (rc) return rc;
    return rs_rebuild_tiles(ctx, k, rows, s, {}, true,
                            [&](size_t b0, size_t nb, const fk::WideLayout& lay) {
                                return plan_wide_slice(ctx, k, m, rows, words, want, 0, true, b0, nb, lay, logv);
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

int rs_encode_ragged_device(fec_ctx* ctx, Code* code, const Shards& s, const uint32_t* lens, int32_t* status,
                            int* err) {
    const uint32_t cps = chunks_of(s.len);
    const uint32_t G = ragged_encode_blocks(cps);
    return for_flat_slices(s, [&](const Shards& sl, size_t b0) -> int {
        for (int r0 = 0; r0 < code->m; r0 += 16) {
            fk::RagEncodeArgs a{};
            fill_row_pass(a, code, r0, sl);
            a.out = sl.par(0, r0);
            a.out_bs = sl.pbs;
            a.max_len = (uint32_t)sl.len;
            a.nblocks = (uint32_t)sl.nblocks;
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
int rs_reconstruct_ragged_device(fec_ctx* ctx, Code* code, const ReconCall& call, const uint32_t* lens) {
    const Shards& s = call.s;
    if (s.ss >> 32) return FEC_ERR_INVALID_ARG;   // the rebuild takes 32-bit shard strides
    const uint32_t k = (uint32_t)code->k, m = (uint32_t)code->m;
    const uint32_t maxe = std::max<uint32_t>(1, std::min(k, m));
    const uint32_t cps = chunks_of(s.len);
    const fk::PlanLayout lay = fk::plan_layout(k, maxe);
    const size_t per_launch = blocks_per_launch(s.nblocks, cps, lay.stride);
    const int rc = grow_plans(ctx, per_launch * lay.stride);
    if (rc) return rc;
    // rows a block can need: the plan kernel gives a block with more erasures than slots no rows
    const uint32_t rows = call.out.base ? std::min(maxe, call.out.slots) : maxe;
    // Blocks per tile: as the encode's, so that a tile of full-length blocks fills one window, within
    // what LDS holds. (pick_tile_blocks, the uniform tile form's choice, looks for the fewest blocks
    // that fill the lanes of a full-length tile: RS(20,30) 3. A ragged tile has fewer items than
    // that, and its fixed cost, two barriers for the prefix and one for the tables, is paid per
    // tile. Measured, the rebuild is indifferent between the two within the run-to-run spread; the
    // encode is 30-42 % slower at 3 blocks per tile: DESIGN.md 4b.)
    const int forced = fk::g_tune.rag_g;
    uint32_t G = forced > 0 ? (uint32_t)forced : std::max<uint32_t>(1, fk::kRagWindow / cps);
    G = fk::rag_clamp_blocks(std::min(G, fk::rag_recon_max_blocks(k, rows, lay)), cps);
    return for_slices(s.nblocks, per_launch, [&](size_t b0, size_t nb) -> int {
        fk::PlanArgs p{};
        fk::RagReconArgs ra{};
        fill_recon_slice(p, ra.r, ctx, code, call.blocks(b0, nb), maxe, lay, G);
        ra.r.status = p.status;
        ra.r.err = p.err;
        ra.lens = lens + b0;
        ra.max_len = (uint32_t)s.len;
        ra.nwin = fk::rag_windows(G, cps);
        ra.rows = rows;
        HIP_TRY(launch_plan(code, p, false, ctx->stream));
        HIP_TRY(fk::launch_rs_reconstruct_ragged(ra, ctx->stream));
        return FEC_OK;
    });
}

// Ragged verify: rs_verify_device's presets (statuses 1, the count 0, on the stream), then the ragged
// encode's launches with the stored parity folded in; the first row pass gives oversize blocks their
// status, after the memset in stream order.
int rs_verify_ragged_device(fec_ctx* ctx, Code* code, const Shards& s, const uint32_t* lens, int32_t* status,
                            uint32_t* count, int* err) {
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)status, 1, s.nblocks, ctx->stream));
    if (count) HIP_TRY(hipMemsetAsync(count, 0, sizeof(uint32_t), ctx->stream));
    const uint32_t cps = chunks_of(s.len);
    const uint32_t G = ragged_encode_blocks(cps);
    return for_flat_slices(s, [&](const Shards& sl, size_t b0) -> int {
        for (int r0 = 0; r0 < code->m; r0 += 16) {
            fk::RagVerifyArgs a{};
            fill_row_pass(a, code, r0, sl);
            a.par = sl.par(0, r0);
            a.par_bs = sl.pbs;
            a.max_len = (uint32_t)sl.len;
            a.nblocks = (uint32_t)sl.nblocks;
            a.g = G;
            a.nwin = fk::rag_windows(G, cps);
            a.lens = lens + b0;
            a.status = status + b0;
            a.count = count;
            a.err = err;
            a.report = r0 == 0;
            HIP_TRY(fk::launch_rs_verify_ragged(a, ctx->stream));
        }
        return FEC_OK;
    });
}

// Ragged reconstruct-some: the uniform call's records (plan_some_slice), then the ragged tile over
// them, which also overrides the status of oversize blocks. Blocks per tile as the ragged rebuild's,
// within what LDS holds of one row pass of tables and the record per block.
int rs_reconstruct_some_ragged_device(fec_ctx* ctx, int ki, int mi, const Shards& s, const DecodeWords& words,
                                      const uint32_t* want, const uint32_t* lens) {
    if (s.ss >> 32) return FEC_ERR_INVALID_ARG;   // the rebuild takes 32-bit shard strides
    Code* code = nullptr;   // (the entry point has looked it up already: cached)
    const int rc0 = get_code(ctx, ki, mi, &code);
    if (rc0) return rc0;
    const uint32_t k = (uint32_t)ki, rows = fk::some_rows((uint32_t)mi);
    const uint32_t cps = chunks_of(s.len);
    const fk::WideLayout lay = fk::wide_layout(k, rows);
    const size_t per_launch = blocks_per_launch(s.nblocks, cps, lay.stride);
    const int rc = grow_plans(ctx, per_launch * lay.stride);
    if (rc) return rc;
    const int forced = fk::g_tune.rag_g;
    uint32_t G = forced > 0 ? (uint32_t)forced : std::max<uint32_t>(1, fk::kRagWindow / cps);
    G = fk::rag_clamp_blocks(std::min(G, fk::rag_some_max_blocks(k, rows, lay)), cps);
    return for_slices(s.nblocks, per_launch, [&](size_t b0, size_t nb) -> int {
        const Shards sl = s.blocks(b0, nb);
        const DecodeWords w = words.blocks(b0);
        fk::RagSomeArgs a{};
        a.data = sl.data;
        a.parity = sl.parity;
        a.dbs = sl.dbs;
        a.pbs = sl.pbs;
        a.ss = (uint32_t)sl.ss;
        a.plans = ctx->work->d_plans;
        a.lay = lay;
        a.k = k;
        a.nblocks = (uint32_t)nb;
        a.max_len = (uint32_t)s.len;
        a.g = G;
        a.nwin = fk::rag_windows(G, cps);
        a.rows = rows;
        a.lens = lens + b0;
        a.status = w.status;
        a.err = w.err;
        HIP_TRY(plan_some_slice(ctx, code, words, want, b0, nb, lay));
        HIP_TRY(fk::launch_rs_reconstruct_some_ragged(a, ctx->stream));
        return FEC_OK;
    });
}

// The XOR calls' launch arguments for one slice: the encode's, or the in-place reconstruct's (data
// rebuilt where it lies, parity read).
static fk::XorArgs xor_slice(int k, const Shards& sl, bool encode) {
    fk::XorArgs a{};
    a.in = sl.data;
    a.out = encode ? sl.parity : sl.data;
    a.in_bs = sl.dbs;
    a.out_bs = encode ? sl.pbs : sl.dbs;
    a.ss = sl.ss;
    a.k = (uint32_t)k;
    fill_flat(a, sl);
    return a;
}

int xor_encode_device(fec_ctx* ctx, int k, const Shards& s) {
    return for_flat_slices(s, [&](const Shards& sl, size_t) -> int {
        const fk::XorArgs a = xor_slice(k, sl, true);
        HIP_TRY(fk::launch_xor_encode(a, flat_grid_nonempty(a.total), ctx->stream));
        return FEC_OK;
    });
}

int xor_reconstruct_device(fec_ctx* ctx, int k, const Shards& s, const DecodeWords& words) {
    return for_flat_slices(s, [&](const Shards& sl, size_t b0) -> int {
        const DecodeWords w = words.blocks(b0);
        fk::XorArgs a = xor_slice(k, sl, false);
        a.parity = sl.parity;
        a.par_bs = sl.pbs;
        a.masks = w.masks;
        a.status = w.status;
        a.err = w.err;
        a.nblocks = (uint32_t)sl.nblocks;
        HIP_TRY(fk::launch_xor_reconstruct(a, flat_grid_nonempty(a.total), ctx->stream));
        return FEC_OK;
    });
}

// A Code for the self-tests below, whose tables are fake addresses: it forgets them before its owners
// would free them.
struct FakeCode : Code {
    ~FakeCode() { d_tabs.p = d_loc_carry.p = d_lmtab.p = nullptr, d_loctab.p = nullptr; }
};

extern "C" {

// Internal self-test (not part of the public ABI, no device needed): blocks() of Shards, OutRegion and
// DecodeWords (fec_ctx.hpp), the one place where a region is moved to a launch's or a chunk's first
// block. A decode call of B = 1000 blocks whose strides all differ (ss != pss, dbs != pbs != out.bs,
// 3 mask words), cut at (b0, nb) = (0, 1), (0, B), (7, 1), (B - 1, 1): the data, parity, out, mask and
// status bases move by b0 times their own stride, nblocks is nb, and nothing else changes (the sticky
// error word and the slot count among it). 0 on success, else 100 * (cut index + 1) + the failing field.
int fec__selftest_batch_slices(void) {
    const size_t B = 1000, W = 3;
    const uintptr_t d0 = uintptr_t(1) << 40, p0 = uintptr_t(2) << 40, o0 = uintptr_t(3) << 40, m0 = uintptr_t(4) << 40,
                    st0 = uintptr_t(5) << 40, e0 = uintptr_t(6) << 40;
    const size_t len = 70000, dbs = 350128, pbs = 1400352, ss = 70016, pss = 70048, obs = 140064;
    const ReconCall c{{len, B, (uint8_t*)d0, dbs, (uint8_t*)p0, pbs, ss, pss},
                      {(const uint32_t*)m0, W, (int32_t*)st0, (int*)e0},
                      {(uint8_t*)o0, obs, 2}};
    const size_t cuts[][2] = {{0, 1}, {0, B}, {7, 1}, {B - 1, 1}};
    int fail = 0;
    for (auto& cut : cuts) {
        fail += 100;
        const size_t b0 = cut[0], nb = cut[1];
        const ReconCall g = c.blocks(b0, nb);
        if ((uintptr_t)g.s.data != d0 + b0 * dbs) return fail + 1;
        if ((uintptr_t)g.s.parity != p0 + b0 * pbs) return fail + 2;
        if (g.s.nblocks != nb) return fail + 3;
        if (g.s.len != len || g.s.dbs != dbs || g.s.pbs != pbs || g.s.ss != ss || g.s.pss != pss) return fail + 4;
        if ((uintptr_t)g.out.base != o0 + b0 * obs) return fail + 5;
        if (g.out.bs != obs || g.out.slots != 2) return fail + 6;
        if ((uintptr_t)g.w.masks != m0 + b0 * W * 4 || g.w.mask_words != W) return fail + 7;
        if ((uintptr_t)g.w.status != st0 + b0 * 4) return fail + 8;
        if ((uintptr_t)g.w.err != e0) return fail + 9;
        // a shard of the slice is that shard of the call
        if (g.s.shard(0, 4) != c.s.shard(b0, 4) || g.s.par(0, 3) != c.s.par(b0, 3)) return fail + 10;
        if ((uintptr_t)c.s.par(b0, 3) != p0 + b0 * pbs + 3 * pss) return fail + 11;
    }
    // no out region and no statuses: none in any slice
    ReconCall n = c;
    n.out = {};
    n.w.status = nullptr;
    const ReconCall g = n.blocks(7, 1);
    return g.out.base || g.w.status ? 1 : 0;
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
    FakeCode code;
    code.k = k;
    code.m = m;
    code.d_tabs.p = (uint32_t*)tab0;
    const UpdateCall u{{L, B, (uint8_t*)in0, in_bs, (uint8_t*)par0, pbs, ss, ss}, {(uint8_t*)old0, old_bs},
                       (const uint32_t*)mask0, W};
    std::vector<fk::UpdateArgs> got;
    const int rc = update_launches(&code, u, [&](const fk::UpdateArgs& a) -> int {
        got.push_back(a);
        return FEC_OK;
    });
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
    e.old = {};
    fk::UpdateArgs a{};
    fill_update_launch(a, &code, 16, e.s.blocks(per, 1), per, e);
    if (a.old != nullptr || (uintptr_t)a.in != in0 + per * in_bs) return 3;
    return 0;
}

// Internal self-test (not part of the public ABI, no device needed): the launches of a locate call
// that the launch limit cuts, for m = 2, 16, 17, 31, 32, 40 (and 1 and 0: one pass of row 0 alone,
// and none). k = 5, 70 000-byte shards, one block more than kMaxItems / 4375: two slices (490 853
// blocks, then one), each its passes and then its finalize. Pass p takes row 0 and the rows from
// r0 = 1 + 15 p: min(15, m - r0) of them. Every launch's data and parity bases, rows, tables, item
// count and verdict pointer, and every finalize's verdict, mask and count pointers, are compared
// with values worked out here from the call's strides. 0 on success, else
// 1000 * (index of m + 1) + 10 * (launch index + 1) + the failing field.
int fec__selftest_locate_slices(void) {
    const int k = 5;
    const size_t L = 70000, cps = 4375, per = 490853, B = per + 1, W = 3;
    if (per != (size_t)(kMaxItems / cps)) return 1;
    const size_t ss = 70016, dbs = k * ss + 48;
    const uintptr_t in0 = uintptr_t(1) << 40, par0 = uintptr_t(3) << 40, mask0 = uintptr_t(4) << 40,
                    tab0 = uintptr_t(5) << 40, ver0 = uintptr_t(6) << 40, cnt0 = uintptr_t(7) << 40,
                    loc0 = uintptr_t(8) << 40;
    static const int ms[] = {2, 16, 17, 31, 32, 40, 1, 0};
    static const int want_passes[] = {1, 1, 2, 2, 3, 3, 1, 0};
    int mi = 0;
    for (int m : ms) {
        const int base = 1000 * ++mi;
        const size_t pbs = (size_t)m * ss + 32;
        FakeCode code;
        code.k = k;
        code.m = m;
        code.d_tabs.p = (uint32_t*)tab0;
        code.d_loctab.p = (uint8_t*)loc0;
        const LocateCall c{{L, B, (uint8_t*)in0, dbs, (uint8_t*)par0, pbs, ss, ss}, (int32_t*)ver0,
                           (uint32_t*)mask0, W, (uint32_t*)cnt0};
        std::vector<fk::LocateArgs> got;
        std::vector<fk::LocateFinArgs> fins;
        std::vector<size_t> fin_after;   // launches emitted before each finalize
        const int rc = locate_launches(
            &code, c,
            [&](const fk::LocateArgs& a) -> int {
                got.push_back(a);
                return FEC_OK;
            },
            [&](const fk::LocateFinArgs& f) -> int {
                fins.push_back(f);
                fin_after.push_back(got.size());
                return FEC_OK;
            });
        const size_t np = (size_t)want_passes[mi - 1];
        if (rc != FEC_OK || got.size() != 2 * np || fins.size() != 2) return base + 2;
        for (size_t i = 0; i < got.size(); ++i) {
            const fk::LocateArgs& a = got[i];
            const int fail = base + 10 * ((int)i + 1);
            const size_t b0 = (i / np) * per, nb = i / np ? 1 : per, r0 = 1 + 15 * (i % np);
            const size_t rows = 1 + std::min<size_t>(15, (size_t)m - r0);   // row 0 among them
            if ((uintptr_t)a.in != in0 + b0 * dbs || a.in_bs != dbs || a.ss != ss) return fail + 1;
            if ((uintptr_t)a.par != par0 + b0 * pbs || a.par_bs != pbs) return fail + 2;
            if (a.r0 != r0 || a.rows != rows || a.k != (uint32_t)k || a.m != (uint32_t)m) return fail + 4;
            if (a.total != nb * cps || a.cps != cps || a.len != L || a.div_cps.d != cps) return fail + 5;
            if ((uintptr_t)a.tabs0 != tab0 || (uintptr_t)a.tabs != tab0 + r0 * k * 8 * 4) return fail + 6;
            if ((uintptr_t)a.loctab != loc0) return fail + 7;
            if ((uintptr_t)a.verdict != ver0 + b0 * 4) return fail + 8;
        }
        for (size_t s = 0; s < 2; ++s) {
            const fk::LocateFinArgs& f = fins[s];
            const int fail = base + 500 + 10 * (int)s;
            const size_t b0 = s * per, nb = s ? 1 : per;
            if (fin_after[s] != (s + 1) * np) return fail + 1;   // after its slice's passes, before the next's
            if ((uintptr_t)f.verdict != ver0 + b0 * 4 || f.nblocks != nb) return fail + 2;
            if ((uintptr_t)f.present != mask0 + b0 * W * 4 || f.mask_words != W) return fail + 3;
            if ((uintptr_t)f.counts != cnt0 || f.n != (uint32_t)(k + m)) return fail + 4;
        }
    }
    // no masks asked for: none in any finalize
    FakeCode code;
    code.k = k;
    code.m = 2;
    code.d_tabs.p = (uint32_t*)tab0;
    LocateCall c{{L, B, (uint8_t*)in0, dbs, (uint8_t*)par0, 2 * ss, ss, ss}, (int32_t*)ver0, nullptr, W, nullptr};
    int bad = 0;
    (void)locate_launches(
        &code, c, [&](const fk::LocateArgs&) -> int { return FEC_OK; },
        [&](const fk::LocateFinArgs& f) -> int {
            if (f.present || f.counts) ++bad;
            return FEC_OK;
        });
    if (bad) return 3;
    // a code with a table for its later passes (k > 128, m > 16): pass 0 reads the code's table, pass p
    // slab p - 1 of 16 * k PermTabs, row 0's first
    const uintptr_t car0 = uintptr_t(9) << 40;
    code.k = 130;
    code.m = 40;
    code.d_loc_carry.p = (uint32_t*)car0;
    c.s.len = 16, c.s.nblocks = 1;
    std::vector<fk::LocateArgs> got;
    (void)locate_launches(
        &code, c,
        [&](const fk::LocateArgs& a) -> int {
            got.push_back(a);
            return FEC_OK;
        },
        [&](const fk::LocateFinArgs&) -> int { return FEC_OK; });
    if (got.size() != 3 || (uintptr_t)got[0].tabs0 != tab0 || (uintptr_t)got[0].tabs != tab0 + 130 * 8 * 4) return 4;
    for (size_t p = 1; p < 3; ++p)
        if ((uintptr_t)got[p].tabs0 != car0 + (p - 1) * 16 * 130 * 8 * 4 ||
            (uintptr_t)got[p].tabs != (uintptr_t)got[p].tabs0 + 130 * 8 * 4)
            return 5;
    return 0;
}

// Internal self-test (not part of the public ABI, no device needed): the slices of a locate-multi call
// that the limits cut, for (k, m) = (5, 4), (5, 16), (5, 1), (5, 0) and (40, 16) (two mask words).
// 70 000-byte shards (4375 chunks): a slice's workspace holds one bitmap bit per item and words + 1
// words per block, and kPlanBytes of it are fewer blocks than kMaxItems items are, so a batch of one
// block more than that has two slices. Every slice's clear size, data, parity and output bases, item
// count, bitmap and block-word pointers, word count, radius and tables are compared with values worked
// out here from the call's strides. Then 16-byte shards, where kMaxItems cuts nothing and the
// workspace alone does. 0 on success, else 1000 * (code index + 1) + 100 * slice + the failing field.
int fec__selftest_locate_multi_slices(void) {
    const size_t L = 70000, cps = 4375, W = 3;
    const size_t ss = 70016;
    const uintptr_t in0 = uintptr_t(1) << 40, par0 = uintptr_t(3) << 40, mask0 = uintptr_t(4) << 40,
                    tab0 = uintptr_t(5) << 40, cnt0 = uintptr_t(6) << 40, out0 = uintptr_t(7) << 40,
                    lm0 = uintptr_t(8) << 40, ws0 = uintptr_t(9) << 40;
    static const int codes[][3] = {{5, 4, 8}, {5, 16, 3}, {5, 1, 1}, {5, 0, 2}, {40, 16, 8}};   // k, m, max_bad
    static const uint32_t want_T[] = {2, 3, 0, 0, 8};
    int ci = 0;
    for (auto& cd : codes) {
        const int base = 1000 * ++ci;
        const int k = cd[0], m = cd[1];
        const size_t words = (size_t)(k + m + 31) / 32;
        const size_t per = std::min<size_t>(kMaxItems / cps, (kPlanBytes - 64) / ((words + 1) * 4 + (cps + 7) / 8));
        const size_t B = per + 1, dbs = k * ss + 48, pbs = (size_t)m * ss + 32;
        if (per >= (size_t)(kMaxItems / cps)) return base + 1;   // the workspace is the tighter limit here
        FakeCode code;
        code.k = k;
        code.m = m;
        code.d_tabs.p = (uint32_t*)tab0;
        code.d_lmtab.p = (uint32_t*)lm0;
        const LocateMultiCall c{{L, B, (uint8_t*)in0, dbs, (uint8_t*)par0, pbs, ss, ss}, cd[2], (int32_t*)out0,
                                (uint32_t*)mask0, W, (uint32_t*)cnt0};
        std::vector<LocateMultiSlice> got;
        const int rc = locate_multi_launches(&code, c, (uint8_t*)ws0, [&](const LocateMultiSlice& sl) -> int {
            got.push_back(sl);
            return FEC_OK;
        });
        if (rc != FEC_OK || got.size() != 2) return base + 2;
        for (size_t s = 0; s < 2; ++s) {
            const LocateMultiSlice& sl = got[s];
            const int fail = base + 100 * (int)s;
            const size_t b0 = s * per, nb = s ? 1 : per;
            const size_t bm = (nb * cps + 255) / 256 * 32, bw = (nb * (words + 1) * 4 + 15) / 16 * 16;
            if (sl.clear != bm + bw || sl.clear > kPlanBytes) return fail + 3;
            const fk::LocateMultiScanArgs& a = sl.scan;
            if ((uintptr_t)a.in != in0 + b0 * dbs || a.in_bs != dbs || a.ss != ss) return fail + 4;
            if ((uintptr_t)a.par != par0 + b0 * pbs || a.par_bs != pbs) return fail + 5;
            if (a.k != (uint32_t)k || a.m != (uint32_t)m || a.len != L || a.cps != cps) return fail + 6;
            if (a.total != nb * cps || a.div_cps.d != cps) return fail + 7;
            if ((uintptr_t)a.tabs != tab0 || (uintptr_t)a.bitmap != ws0) return fail + 8;
            const fk::LocateMultiSolveArgs& v = sl.solve;
            if (memcmp(&v.s, &a, sizeof(a)) != 0) return fail + 9;
            if (v.nwords != bm / 8 || v.n != (uint32_t)(k + m) || v.T != want_T[ci - 1] || v.words != words)
                return fail + 10;
            if ((uintptr_t)v.atabs != lm0 || (uintptr_t)v.ft != lm0 + (size_t)m * m * 32) return fail + 11;
            if ((uintptr_t)v.blk != ws0 + bm) return fail + 12;
            const fk::LocateMultiFinArgs& f = sl.fin;
            if ((uintptr_t)f.blk != ws0 + bm || (uintptr_t)f.bad_count != out0 + b0 * 4) return fail + 13;
            if ((uintptr_t)f.present != mask0 + b0 * W * 4 || f.mask_words != W) return fail + 14;
            if ((uintptr_t)f.counts != cnt0 || f.nblocks != nb || f.n != v.n || f.T != v.T || f.words != words)
                return fail + 15;
        }
    }
    // no masks and no counts asked for: none in any finalize; 16-byte shards: 2^31 items fit a launch
    // but their workspace does not (10 bytes a block)
    Code code;
    code.k = 5;
    code.m = 4;
    const size_t per = (kPlanBytes - 64) / 9, B = 2 * per + 5;
    const LocateMultiCall c{{16, B, (uint8_t*)in0, 128, (uint8_t*)par0, 64, 16, 16}, 1, (int32_t*)out0, nullptr, 1,
                            nullptr};
    size_t slices = 0, blocks = 0;
    int bad = 0;
    (void)locate_multi_launches(&code, c, (uint8_t*)ws0, [&](const LocateMultiSlice& sl) -> int {
        if (sl.fin.present || sl.fin.counts || sl.solve.T != 1 || sl.clear > kPlanBytes) ++bad;
        if (sl.scan.total != sl.fin.nblocks || (uintptr_t)sl.scan.in != in0 + blocks * 128) ++bad;
        ++slices, blocks += sl.fin.nblocks;
        return FEC_OK;
    });
    if (bad || slices != 3 || blocks != B) return 3;
    return 0;
}

// Internal self-test (not part of the public ABI, no device needed): the slices of a locate-partial
// call, for (k, m) = (5, 4), (5, 16), (5, 0) and (40, 16), 70 000-byte shards and one block more than
// kPlanBytes of workspace holds (so two slices). Every slice's clear size, workspace parts (bitmap,
// block words, zeros, plan words, scaling tables: each where the parts before it end), mask, data,
// parity and output bases and the records' fields are compared with values worked out here. Then a
// call without masks written or counts. 0 on success, else 1000 * (code index + 1) + 100 * slice + the
// failing field.
int fec__selftest_locate_partial_slices(void) {
    const size_t L = 70000, cps = 4375, W = 3;
    const size_t ss = 70016;
    const uintptr_t in0 = uintptr_t(1) << 40, par0 = uintptr_t(3) << 40, mask0 = uintptr_t(4) << 40,
                    tab0 = uintptr_t(5) << 40, cnt0 = uintptr_t(6) << 40, out0 = uintptr_t(7) << 40,
                    lm0 = uintptr_t(8) << 40, ws0 = uintptr_t(9) << 40, pm0 = uintptr_t(10) << 40;
    static const int codes[][3] = {{5, 4, 8}, {5, 16, 0}, {5, 0, 2}, {40, 16, 8}};   // k, m, max_bad
    int ci = 0;
    for (auto& cd : codes) {
        const int base = 1000 * ++ci;
        const int k = cd[0], m = cd[1];
        const size_t words = (size_t)(k + m + 31) / 32;
        const size_t per = std::min<size_t>(kMaxItems / cps,
                                            (kPlanBytes - 192) / ((words + 2) * 4 + (cps + 7) / 8 + (size_t)m * 32));
        const size_t B = per + 1, dbs = k * ss + 48, pbs = (size_t)m * ss + 32;
        if (per >= (size_t)(kMaxItems / cps)) return base + 1;   // the workspace is the tighter limit here
        FakeCode code;
        code.k = k;
        code.m = m;
        code.d_tabs.p = (uint32_t*)tab0;
        code.d_lmtab.p = (uint32_t*)lm0;
        const LocatePartialCall c{{{L, B, (uint8_t*)in0, dbs, (uint8_t*)par0, pbs, ss, ss}, cd[2], (int32_t*)out0,
                                   (uint32_t*)mask0, W, (uint32_t*)cnt0},
                                  (const uint32_t*)pm0};
        std::vector<LocatePartialSlice> got;
        const int rc = locate_partial_launches(&code, c, (uint8_t*)ws0, [&](const LocatePartialSlice& sl) -> int {
            got.push_back(sl);
            return FEC_OK;
        });
        if (rc != FEC_OK || got.size() != 2) return base + 2;
        for (size_t s = 0; s < 2; ++s) {
            const LocatePartialSlice& sl = got[s];
            const int fail = base + 100 * (int)s;
            const size_t b0 = s * per, nb = s ? 1 : per;
            const size_t bm = (nb * cps + 255) / 256 * 32, bw = (nb * (words + 1) * 4 + 15) / 16 * 16;
            const size_t pw = (nb * 4 + 15) / 16 * 16;
            const uintptr_t zero = ws0 + bm + bw, plan = zero + 64, lt = plan + pw;
            if (sl.clear != bm + bw + 64 || lt - ws0 + nb * m * 32 > kPlanBytes) return fail + 3;
            const fk::LocatePartialPlanArgs& p = sl.plan;
            if ((uintptr_t)p.masks != pm0 + b0 * W * 4 || p.mask_words != W || p.nblocks != nb) return fail + 4;
            if ((uintptr_t)p.plan != plan || (uintptr_t)p.ltabs != lt) return fail + 5;
            if (p.k != (uint32_t)k || p.m != (uint32_t)m || p.max_bad != (uint32_t)cd[2]) return fail + 6;
            const fk::LocatePartialScanArgs& a = sl.scan;
            if ((uintptr_t)a.in != in0 + b0 * dbs || a.in_bs != dbs || a.ss != ss) return fail + 7;
            if ((uintptr_t)a.par != par0 + b0 * pbs || a.par_bs != pbs) return fail + 8;
            if (a.k != (uint32_t)k || a.m != (uint32_t)m || a.len != L || a.cps != cps) return fail + 9;
            if (a.total != nb * cps || a.div_cps.d != cps) return fail + 10;
            if ((uintptr_t)a.tabs != tab0 || (uintptr_t)a.bitmap != ws0 || (uintptr_t)a.atabs != lm0) return fail + 11;
            if (a.masks != p.masks || a.plan != p.plan || a.ltabs != p.ltabs || a.mask_words != W) return fail + 12;
            if ((uintptr_t)a.zeros != zero) return fail + 13;
            const fk::LocatePartialSolveArgs& v = sl.solve;
            if (memcmp(&v.s, &a, sizeof(a)) != 0) return fail + 14;
            if (v.nwords != bm / 8 || v.n != (uint32_t)(k + m) || v.words != words) return fail + 15;
            if ((uintptr_t)v.ft != lm0 + (size_t)m * m * 32 || (uintptr_t)v.blk != ws0 + bm) return fail + 16;
            const fk::LocatePartialFinArgs& f = sl.fin;
            if (f.blk != v.blk || f.plan != p.plan || f.masks != p.masks) return fail + 17;
            if ((uintptr_t)f.bad_count != out0 + b0 * 4 || (uintptr_t)f.present != mask0 + b0 * W * 4) return fail + 18;
            if ((uintptr_t)f.counts != cnt0 || f.nblocks != nb || f.n != v.n || f.words != words || f.mask_words != W)
                return fail + 19;
        }
    }
    // no masks written and no counts: none in any finalize; the masks read stride by mask_words
    Code code;
    code.k = 5;
    code.m = 4;
    const size_t per = (kPlanBytes - 192) / (12 + 1 + 128), B = per + 7;
    const LocatePartialCall c{{{16, B, (uint8_t*)in0, 128, (uint8_t*)par0, 64, 16, 16}, 1, (int32_t*)out0, nullptr, 2,
                               nullptr},
                              (const uint32_t*)pm0};
    size_t slices = 0, blocks = 0;
    int bad = 0;
    (void)locate_partial_launches(&code, c, (uint8_t*)ws0, [&](const LocatePartialSlice& sl) -> int {
        if (sl.fin.present || sl.fin.counts || sl.plan.max_bad != 1 || sl.clear > kPlanBytes) ++bad;
        if ((uintptr_t)sl.fin.masks != pm0 + blocks * 8 || (uintptr_t)sl.scan.in != in0 + blocks * 128) ++bad;
        ++slices, blocks += sl.fin.nblocks;
        return FEC_OK;
    });
    if (bad || slices != 2 || blocks != B) return 3;
    return 0;
}

}  // extern "C"
