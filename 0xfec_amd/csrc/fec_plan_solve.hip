// fec_plan_solve.hip — the elimination plan of a custom code matrix for gfx950 (fec_hip_matrix.h
// fec_ctx_set_custom_matrix; the arithmetic and what it computes: fec_solve.hpp). The built-in
// matrices never invert anything (fec_plan.hip: Lagrange over the shard indices); rows of the caller's
// own have no such structure, so these kernels do what klauspost does, Gauss-Jordan on the rows of the
// first k present shards, and write the records the rebuild kernels already read: PlanLayout records
// in block order or sorted by erasure count (reconstruct, recover, their ragged forms), WideLayout
// records for reconstruct-some.
//
// A group of 32 lanes, half a wave, shares a block. Lane j owns column j of the e x (k + e) matrix
// [P[R] | I], e <= 16 bytes in the group's LDS scratch (columns 20 bytes apart: lanes on different
// banks). Step c reads the pivot column E_c, which every lane of the group scans for the pivot row
// itself (the same LDS bytes: a broadcast read, no ballot needed), and updates its own column
// (solve_step); the pivot column's owner sits the step out, so one wave-level sync per step orders
// everything. After e steps the lanes of the present data columns and of the identity columns hold
// the coefficient columns of their input and store them into the record.
#include <algorithm>

#include "fec_plan_sort.hpp"
#include "fec_solve.hpp"

namespace fk {

namespace {

constexpr uint32_t kSolveLanes = 32;                                // lanes per block
constexpr uint32_t kSolveGroups = kPlanSortThreads / kSolveLanes;   // blocks per workgroup segment
// group scratch: the columns, then E and R
constexpr uint32_t kSolveE = kSolveColBytes, kSolveR = kSolveE + kSolveMaxE, kSolveScratch = kSolveR + kSolveMaxE;
static_assert(kSolveScratch % 16 == 0 && kSolveCols == kSolveLanes, "a lane per column, scratch in 16-byte units");
// tables: exp over [0, 512), then log (inside the table area of sort_lds)
constexpr uint32_t kSolveExp = 0, kSolveLog = 512;
static_assert(kSolveLog + 256 <= kV2Tables, "the tables fit sort_lds's table area");

__device__ __forceinline__ void stage_tables(uint8_t* smem, uint8_t* s_prows, const uint8_t* prows, uint32_t mk) {
    for (uint32_t i = threadIdx.x; i < 768; i += kPlanSortThreads)
        smem[i] = i < kSolveLog ? gf::kTables.exp[i] : gf::kTables.log[i - kSolveLog];
    for (uint32_t i = threadIdx.x; i < mk; i += kPlanSortThreads) s_prows[i] = prows[i];
}

// The largest of the wave's two groups' step counts: the step loop runs to it, so that its syncs are
// wave-uniform.
__device__ __forceinline__ uint32_t wave_steps(uint32_t e) {
    const uint32_t o = (uint32_t)__shfl_xor((int)e, (int)kSolveLanes);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)max(e, o));
}

// The group's block solved in its scratch: sets, columns, steps (solve_block, a lane per shard and per
// column). e: the block's erased data shard count, 0 for a group with nothing to solve. False when
// the rows are dependent (group-uniform). Wave-uniform control flow around every sync.
__device__ __forceinline__ bool solve_group(uint8_t* grp, uint32_t gl, uint32_t mask, uint32_t k, uint32_t n,
                                            uint32_t e, const uint8_t* s_prows, const uint8_t* s_exp,
                                            const uint8_t* s_log) {
    uint8_t* E = grp + kSolveE;
    uint8_t* R = grp + kSolveR;
    uint8_t* col = grp + gl * kSolveColStride;
    if (e && gl < n) solve_place(E, R, gl, mask, k, e);
    wave_sync();
    if (gl < k + e) solve_init_column(col, gl, s_prows, R, k, e);
    wave_sync();
    bool ok = true;
    const uint32_t steps = wave_steps(e);
    for (uint32_t c = 0; c < steps; ++c) {
        if (c < e && ok) {
            const uint32_t ec = E[c];
            const uint8_t* pc = grp + ec * kSolveColStride;
            const uint32_t p = solve_pivot(pc, c, e);
            if (p == e) ok = false;
            else if (gl < k + e && gl != ec) solve_step(col, pc, c, p, e, s_exp, s_log);
        }
        wave_sync();
    }
    return ok;
}

// The group's record from LDS to block b's place in a.plans (block order), 16 bytes per lane and turn.
__device__ __forceinline__ void record_out(uint8_t* plans, const uint8_t* P, uint32_t stride, uint32_t b,
                                           uint32_t gl) {
    const uint4* src = reinterpret_cast<const uint4*>(P);
    uint4* dst = reinterpret_cast<uint4*>(plans + (uint64_t)b * stride);
    for (uint32_t i = gl; i < stride / 16; i += kSolveLanes) dst[i] = src[i];
}

// Reconstruct / recover records. SORTED: the records of a window of 64 blocks stored in erasure-count
// order, each naming its block (sort_window_out, as fec_plan.hip stores them); else in block order.
// The block head is the rule of fec_status.hpp (classify_block), in place as in the other plan
// kernels, with the singular block after it.
template <bool SORTED>
__global__ __launch_bounds__(kPlanSortThreads) void rs_plan_solve_kernel(PlanArgs a, uint32_t segs, uint32_t win) {
    constexpr uint32_t G = kSolveGroups;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if (route_skips(a)) return;
    const PlanLayout lay = a.lay;
    const SortLds L = sort_lds(a.m, a.k, G, lay.stride, win, kSolveScratch);
    const uint8_t* s_exp = smem + kSolveExp;
    const uint8_t* s_log = smem + kSolveLog;
    uint8_t* s_prows = smem + L.prows;
    const uint32_t k = a.k, m = a.m, n = k + m;
    const uint32_t gb = threadIdx.x / kSolveLanes, gl = threadIdx.x % kSolveLanes;
    stage_tables(smem, s_prows, a.prows, m * k);
    uint8_t* grp = smem + L.scratch + gb * kSolveScratch;
    const uint32_t all = low_mask(n), kmask = low_mask(k);
    const uint32_t seg0 = blockIdx.x * segs;
    for (uint32_t sg = 0; sg < segs; ++sg) {
        const uint32_t base = (seg0 + sg) * G;
        if (base >= a.nblocks) break;   // workgroup-uniform
        const uint32_t b = base + gb;
        const bool valid = b < a.nblocks;
        const uint32_t wl = SORTED ? sg % win : 0u;   // segment within the sort window
        // a window's first segment (block order: the first segment) waits for the workgroup: tables
        // staged, the previous window's records copied out; later ones reuse only the group's own LDS
        if (sg == 0 || (SORTED && wl == 0)) __syncthreads();
        else wave_sync();
        uint8_t* P = smem + L.recs + ((size_t)wl * G + gb) * lay.stride;
        const uint32_t mask = valid ? a.masks[b] & all : all;   // past the batch: nothing to rebuild
        const uint32_t e = k - __popc(mask & kmask);
        int32_t st = a.max_out ? (int32_t)e : 0;
        uint32_t nout = 0;
        if (e != 0) {
            if ((uint32_t)__popc(mask) < k) {
                st = kStTooFew;
                if (gl == 0) wave_flag(a.err, kStickyTooFew);
            } else if (a.max_out && e > a.max_out) {
                st = kStSlots;
                if (gl == 0) wave_flag(a.err, kStickySlots);
            } else {
                nout = e;
            }
        }
        if (!solve_group(grp, gl, mask, k, n, nout, s_prows, s_exp, s_log)) {
            nout = 0;
            st = kStSingular;
            if (gl == 0) wave_flag(a.err, kStickySingular);
        }
        if (gl == 0) {
            P[lay.nout_off] = (uint8_t)nout;
            if (SORTED) *reinterpret_cast<uint32_t*>(P + lay.blk_off) = b;
            if (valid && a.status) a.status[b] = st;
        }
        if (nout) {
            if (gl < nout) P[lay.out_off + gl] = grp[kSolveE + gl];
            uint32_t pos, shard;
            if (gl < k + nout && solve_input(gl, mask, k, nout, grp + kSolveR, &pos, &shard)) {
                const uint8_t* col = grp + gl * kSolveColStride;
                P[lay.in_off + pos] = (uint8_t)shard;
                for (uint32_t r = 0; r < nout; ++r) P[lay.coef_off + r * k + pos] = col[r];
            }
        }
        if constexpr (SORTED) {
            const bool last = sg + 1 == segs || base + G >= a.nblocks;
            if (wl + 1 < win && !last) continue;   // workgroup-uniform
            sort_window_out(a, smem, L, (wl + 1) * G, base - wl * G);
        } else {
            wave_sync();
            if (valid) record_out(a.plans, P, lay.stride, b, gl);
        }
    }
}

// Reconstruct-some records (WideLayout, block order): solve_some_record with a lane per column.
__global__ __launch_bounds__(kPlanSortThreads) void rs_plan_solve_some_kernel(SolveSomeArgs sa, uint32_t segs) {
    constexpr uint32_t G = kSolveGroups;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const SomePlanArgs& a = sa.p;
    const WideLayout lay = a.lay;
    const uint32_t k = a.k, n = a.n, m = n - k;
    const SortLds L = sort_lds(m, k, G, lay.stride, 1, kSolveScratch);
    const uint8_t* s_exp = smem + kSolveExp;
    const uint8_t* s_log = smem + kSolveLog;
    uint8_t* s_prows = smem + L.prows;
    const uint32_t gb = threadIdx.x / kSolveLanes, gl = threadIdx.x % kSolveLanes;
    stage_tables(smem, s_prows, sa.prows, m * k);
    uint8_t* grp = smem + L.scratch + gb * kSolveScratch;
    uint8_t* P = smem + L.recs + (size_t)gb * lay.stride;
    const uint32_t all = low_mask(n), kmask = low_mask(k);
    const uint32_t seg0 = blockIdx.x * segs;
    for (uint32_t sg = 0; sg < segs; ++sg) {
        const uint32_t base = (seg0 + sg) * G;
        if (base >= a.nblocks) break;   // workgroup-uniform
        const uint32_t b = base + gb;
        const bool valid = b < a.nblocks;
        if (sg == 0) __syncthreads();
        else wave_sync();
        const uint32_t mask = valid ? a.masks[b] & all : all;
        const uint32_t miss = ~mask & (a.want && valid ? a.want[b] : 0xFFFFFFFFu) & all;
        const uint32_t e = k - __popc(mask & kmask), eo = __popc(miss);
        int32_t st = 0;
        uint32_t nout = 0;
        if (eo != 0) {
            if ((uint32_t)__popc(mask) < k) {
                st = kStTooFew;
                if (gl == 0) wave_flag(a.err, kStickyTooFew);
            } else {
                nout = eo;
            }
        }
        const uint32_t es = nout ? e : 0u;   // erased data shards to solve for
        if (!solve_group(grp, gl, mask, k, n, es, s_prows, s_exp, s_log)) {
            nout = 0;
            st = kStSingular;
            if (gl == 0) wave_flag(a.err, kStickySingular);
        }
        if (gl == 0) {
            P[lay.nout_off] = (uint8_t)nout;
            if (valid && a.status) a.status[b] = st;
        }
        uint8_t* O = P + lay.out_off;
        if (nout && gl < n && ((miss >> gl) & 1u)) O[__popc(miss & low_mask(gl))] = (uint8_t)gl;
        if (nout && gl >= k && gl < ((k + 7) & ~7u)) P[lay.in_off + gl] = 0;
        wave_sync();
        uint32_t pos, shard;
        if (nout && gl < k + es && solve_input(gl, mask, k, es, grp + kSolveR, &pos, &shard)) {
            const uint8_t* col = grp + gl * kSolveColStride;
            P[lay.in_off + pos] = (uint8_t)shard;
            for (uint32_t r = 0; r < nout; ++r)
                P[lay.coef_off + r * k + pos] =
                    solve_coef(col, gl, O[r], mask, s_prows, grp + kSolveE, k, es, s_exp, s_log);
        }
        wave_sync();
        if (valid) record_out(a.plans, P, lay.stride, b, gl);
    }
}

// Segments per workgroup: enough workgroups to fill the chip several times over, each staging the
// tables once for all its segments; a sort window never spans two workgroups.
uint32_t solve_segments(uint32_t nseg, uint32_t win) {
    uint32_t segs = std::max<uint32_t>(1, nseg / 4096);
    segs = std::min<uint32_t>(segs, std::max<uint32_t>(64, win));
    return (segs + win - 1) / win * win;
}

}  // namespace

hipError_t launch_rs_plan_solve(const PlanArgs& a, bool sorted, hipStream_t s) {
    constexpr uint32_t G = kSolveGroups;
    const uint32_t nseg = (a.nblocks + G - 1) / G;
    if (nseg == 0) return hipSuccess;
    const uint32_t win = sorted ? sort_window(G) : 1u, segs = solve_segments(nseg, win);
    const uint32_t grid = (nseg + segs - 1) / segs;
    const size_t lds = sort_lds(a.m, a.k, G, a.lay.stride, win, kSolveScratch).total;
    if (sorted) hipLaunchKernelGGL(rs_plan_solve_kernel<true>, dim3(grid), dim3(kPlanSortThreads), lds, s, a, segs, win);
    else hipLaunchKernelGGL(rs_plan_solve_kernel<false>, dim3(grid), dim3(kPlanSortThreads), lds, s, a, segs, win);
    return hipGetLastError();
}

hipError_t launch_rs_plan_solve_some(const SolveSomeArgs& a, hipStream_t s) {
    constexpr uint32_t G = kSolveGroups;
    const uint32_t nseg = (a.p.nblocks + G - 1) / G;
    if (nseg == 0) return hipSuccess;
    const uint32_t segs = solve_segments(nseg, 1);
    const uint32_t grid = (nseg + segs - 1) / segs;
    const size_t lds = sort_lds(a.p.n - a.p.k, a.p.k, G, a.p.lay.stride, 1, kSolveScratch).total;
    hipLaunchKernelGGL(rs_plan_solve_some_kernel, dim3(grid), dim3(kPlanSortThreads), lds, s, a, segs);
    return hipGetLastError();
}

}  // namespace fk
