// fec_plan.hip — sorted decode plans for gfx950 (reed_solomon.go:124 ReconstructData: which shards
// to read and with which coefficients to rebuild the erased data shards of each block).
//
// rs_plan_kernel (fec_decode.hip) gives one block to one lane: its k^2 + 3ek table lookups run
// one after another (~0.2 ms for 2^19 RS(16,24) blocks with 1-8 losses). Here a group of
// plan_lanes(k) lanes of one wave shares a block: lane p builds input slot p, the Lagrange
// denominator D_p and coefficient column p; lane r < e the numerator N_r — k-long chains instead
// of k^2.
//
// The records of a window of 64 blocks are then stored ordered by erasure count (descending,
// blocks with nothing to rebuild last), each naming its block. The rebuild kernel walks records
// in storage order, so the <= 3 blocks a rebuild wave touches have (nearly always) the same
// erasure count: its wave-uniform row count is the blocks' own, not the maximum of unrelated
// neighbours (RS(16,24) with 1-8 losses: 3.8 -> 3.1 rows per wave).
//
// Two forms: rs_plan_code_kernel (form 3) compiled for RS(16,24) / RS(20,30), and
// rs_plan_sorted_kernel (form 2) for every other code.
#include <algorithm>

#include "fec_plan_sort.hpp"

namespace fk {

namespace {

// ---- the parts of a segment walk that forms 2 and 3 share. Each form keeps its own index scatter,
// sums and coefficient rows; the block head (classification by the rule of fec_status.hpp, record
// fields, status) and the window end also stay written out in both: as helpers they changed both
// forms' machine code.

// The segment step, two parts that each form calls in its own order. The mask of block b's
// successor in the workgroup's next segment (0: none), loaded a segment ahead of its use:
template <uint32_t G>
__device__ __forceinline__ uint32_t next_mask(const PlanArgs& a, uint32_t b, uint32_t sg, uint32_t segs) {
    const uint32_t bn = b + G;
    return (sg + 1 < segs && bn < a.nblocks) ? a.masks[bn] : 0u;
}
// and the barrier before segment wl of a sort window. A window's first segment waits for the
// workgroup: tables staged (first pass), the previous window's records copied out; within a
// window a block group's scratch is its own lanes' (wave-local).
__device__ __forceinline__ void window_sync(uint32_t wl) {
    if (wl == 0) __syncthreads();
    else wave_sync();
}

// The coefficient row of a block with one erased data shard E0, inputs S:
// x_E0 = inv(A[R0][E0]) * (p_R0 ^ sum_j A[R0][j] x_j), R0 the first present parity (e = 1 with k
// present shards: there is one, k < 32).
__device__ __forceinline__ void one_erasure_row(uint8_t* C, const uint8_t* S, uint32_t E0, uint32_t mask, uint32_t k,
                                                uint32_t gl, const uint8_t* s_prows, const uint8_t* s_exp,
                                                const uint8_t* s_log) {
    const uint32_t R0 = __ffs(mask >> k) - 1;
    const uint8_t* row = s_prows + R0 * k;
    const uint32_t inv = s_exp[255 - s_log[row[E0]]];
    if (gl < k) {
        const uint32_t sj = S[gl];
        C[gl] = (uint8_t)(sj < k ? (row[sj] ? s_exp[s_log[inv] + s_log[row[sj]]] : 0u) : inv);
    }
}

template <uint32_t LPB>
__global__ __launch_bounds__(kPlanSortThreads) void rs_plan_sorted_kernel(PlanArgs a, uint32_t segs, uint32_t win) {
    constexpr uint32_t G = kPlanSortThreads / LPB;   // blocks per workgroup segment
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if (route_skips(a)) return;
    const PlanLayout lay = a.lay;
    const SortLds L = sort_lds(a.m, a.k, G, lay.stride, win);
    uint8_t* s_exp = smem + kV2Exp;
    uint8_t* s_log = smem + kV2Log;
    // this lane's copy of log(0..31)
    const uint8_t* s_l32 = smem + kV2Log32 + (threadIdx.x & 3u) * 32u;
    uint8_t* s_prows = smem + L.prows;
    const uint32_t k = a.k, m = a.m, n = k + m;
    const uint32_t gb = threadIdx.x / LPB, gl = threadIdx.x % LPB;   // block group, lane in group
    // the tables (the layout above), the parity rows and dall: staged once per workgroup, which
    // then plans `segs` consecutive segments of G blocks
    for (uint32_t i = threadIdx.x; i < kV2Tables; i += kPlanSortThreads) {
        const uint32_t j = i - kV2Log32;
        smem[i] = i < kV2Log ? gf::kTables.exp[i % 255u]
                : i < kV2Log32 ? gf::kTables.log[i - kV2Log]
                : (j & 31u) ? gf::kTables.log[j & 31u] : (uint8_t)0;
    }
    for (uint32_t i = threadIdx.x; i < m * k; i += kPlanSortThreads) s_prows[i] = a.prows[i];
    uint8_t* s_dall = smem + L.dall;
    if (threadIdx.x < n) s_dall[threadIdx.x] = a.dall[threadIdx.x];
    uint8_t* S = smem + L.scratch + gb * kGroupScratch;   // first k present shards
    uint8_t* O = S + 32;                                  // erased data shards, ascending
    uint8_t* X = S + 64;                                  // the other n - k shard indices
    uint8_t* Dt = S + 96;                                 // D_p (k bytes), then N_r (maxe bytes)
    uint8_t* Nt = Dt + k;
    const uint32_t all = low_mask(n), kmask = low_mask(k);
    const uint32_t seg0 = blockIdx.x * segs;
    // the first segment's masks in flight while the tables stage
    uint32_t mask_next = seg0 * G + gb < a.nblocks ? a.masks[seg0 * G + gb] : 0u;
    for (uint32_t sg = 0; sg < segs; ++sg) {
        const uint32_t base = (seg0 + sg) * G;
        if (base >= a.nblocks) break;   // workgroup-uniform
        const uint32_t b = base + gb;
        const bool valid = b < a.nblocks;
        const uint32_t wl = sg % win;   // segment within the sort window
        const uint32_t mask_in = mask_next;
        mask_next = next_mask<G>(a, b, sg, segs);   // loads before this segment's work
        window_sync(wl);
        uint8_t* P = smem + L.recs + ((size_t)wl * G + gb) * lay.stride;
        const uint32_t mask = valid ? mask_in & all : all;   // past the batch: nothing to rebuild
        const uint32_t e = k - __popc(mask & kmask);
        // the block head: the rule of fec_status.hpp (classify_block) in place, then the record's fields
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
        if (gl == 0) {
            P[lay.nout_off] = (uint8_t)nout;
            *reinterpret_cast<uint32_t*>(P + lay.blk_off) = b;
            if (valid && a.status) a.status[b] = st;
        }
        if (nout) {
            for (uint32_t t = gl; t < n; t += LPB) {
                const uint32_t pos = __popc(mask & low_mask(t));
                if (((mask >> t) & 1u) && pos < k) {
                    S[pos] = (uint8_t)t;
                } else {
                    X[t - min(pos, k)] = (uint8_t)t;   // not an input: erased, or present past the first k
                    if (t < k && !((mask >> t) & 1u)) O[__popc(~mask & kmask & low_mask(t))] = (uint8_t)t;
                }
            }
        }
        wave_sync();
        uint8_t* C = P + lay.coef_off;
        if (nout) {
            if (gl < k) P[lay.in_off + gl] = S[gl];
            if (gl < nout) P[lay.out_off + gl] = O[gl];
            if (e == 1) {
                one_erasure_row(C, S, O[0], mask, k, gl, s_prows, s_exp, s_log);
            } else {
                // D_p and N_r are the same sum for the shard t = s_p or i_r, over the set Y = the
                // others X (complement form, n - k < k: sum over all n indices, dall, minus the n - k
                // others) or the inputs S; log32(0) = 0 drops the t = y term. Lane q of the group
                // takes t = S[q] (q < k) or O[q - k]: RS(20,30) both sets in one pass over 30 lanes;
                // Nt = Dt + k. coef[r][p] = exp(N_r - log(i_r ^ s_p) - D_p) (Lagrange over the shard
                // indices, rs_plan_kernel).
                const bool comp = n - k < k;
                const uint32_t ny = comp ? n - k : k;
                const uint8_t* Y = comp ? X : S;
                for (uint32_t q = gl; q < k + e; q += LPB) {
                    const uint32_t t = q < k ? S[q] : O[q - k];
                    uint32_t s = 0;
                    for (uint32_t u = 0; u < ny; ++u) s += s_l32[t ^ Y[u]];
                    if (comp) s = s_dall[t] + 255u * 32u - s;   // (dall holds logv[t] already)
                    else if (a.logv) s += a.logv[t];            // direct sums: PlanArgs::logv
                    Dt[q] = (uint8_t)(s % 255u);
                }
            }
        }
        wave_sync();
        if (nout >= 2 && gl < k) {
            const uint32_t sp = S[gl], dp = Dt[gl];
            for (uint32_t r = 0; r < nout; ++r) {
                // < 765: exp needs no reduction
                const uint32_t v = Nt[r] + 2u * 255u - s_l32[O[r] ^ sp] - dp;
                C[r * k + gl] = s_exp[v];
            }
        }
        // at the end of a sort window (or of the work): storage order of the window's records,
        // erasure count descending, then block order (stable)
        const bool last = sg + 1 == segs || base + G >= a.nblocks;
        if (wl + 1 < win && !last) continue;   // workgroup-uniform
        sort_window_out(a, smem, L, (wl + 1) * G, base - wl * G);
    }
}

// Form 3: the same plans for one code known at compile time, K data and M parity shards with
// M < K (the complement sums: RS(16,24), RS(20,30)), so every loop is unrolled and the sums are built
// for the fewest instructions (r04d/e: VALU per plan wave 3171 -> 2064 for RS(20,30), 2176 -> 1380
// for RS(16,24), decode +0.8-0.9 % over form 2):
//   * tables: exp over [0, 768), then 255 - log j for j < 32 in 4 copies (j = 0: 255, i.e. log 0 = 0),
//     then log; lane l reads copy l & 3, and its table address t ^ y ^ (copy << 5) is one XOR of
//     a shard index y with the lane's t ^ (copy << 5);
//   * with nl(j) = 255 - log j the complement sum D = dall[t] + 255*32 - sum_y log(t ^ y) is
//     dall[t] + sum_y nl(t ^ y) mod 255: no compare, no subtraction;
//   * the others X, the erased O and the numerators N sit in dword scratch, read into registers
//     by wide LDS loads, and coef = exp(N_r + nl(O_r ^ s_p) + (255 - D_p)) is one three-input add
//     (the argument < 765: exp needs no reduction).
// (Two segments interleaved per wave, r04i, and a window ranked from the masks first, r04t, left
// the decode within +-0.4 % and 0.8-2 % slower: not kept.)
constexpr uint32_t kV3Exp = 0, kV3NLog32 = 768, kV3Log = 896, kV3Tables = 1152;
typedef const __attribute__((address_space(3))) uint8_t lds_cu8;
// LDS address of a pointer into the kernel's LDS, and a byte load from one: lets the table
// address be formed as one XOR (the compiler, given generic pointers, adds the LDS base per load)
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}
__device__ __forceinline__ uint32_t lds_ld8(uint32_t addr) { return *(lds_cu8*)(uintptr_t)addr; }
static_assert(kV3Tables == kV2Tables, "forms 2 and 3 share sort_lds's table area");
// group scratch: S bytes [0, 32), X dwords [32, 80), O dwords [80, 128), N dwords [128, 176), 255 - D_p
// bytes [176, 208)
constexpr uint32_t kV3S = 0, kV3X = 32, kV3O = 80, kV3N = 128, kV3D = 176, kGroupScratch3 = 208;
// lanes per block of form 3
constexpr uint32_t code_lanes(uint32_t K) { return K <= 16 ? 16u : 32u; }

template <uint32_t K, uint32_t M>
__global__ __launch_bounds__(kPlanSortThreads) void rs_plan_code_kernel(PlanArgs a, uint32_t segs, uint32_t win) {
    constexpr uint32_t N = K + M, LPB = code_lanes(K), G = kPlanSortThreads / LPB, MAXE = M;
    static_assert(M < K && M <= 12 && K <= LPB && N <= 32, "complement-sum codes with the scratch above");
    extern __shared__ __attribute__((aligned(128))) uint8_t smem[];
    const PlanLayout lay = a.lay;
    const SortLds L = sort_lds(M, K, G, lay.stride, win, kGroupScratch3);
    const uint8_t* s_exp = smem + kV3Exp;
    const uint8_t* s_log = smem + kV3Log;
    const uint8_t* s_nl = smem + kV3NLog32;
    const uint32_t copy5 = (threadIdx.x & 3u) << 5;
    // nl(t ^ y) of the lane's copy at nlb ^ y, nlb = the table's LDS address + (t ^ copy << 5): one
    // XOR per term, exact while the table starts on a 128-byte boundary: smem is declared 128-byte
    // aligned and the table sits 768 bytes into it (the check below cannot fire; if it ever did,
    // the sticky error fails the call, device and host paths alike)
    const uint32_t nl_base = lds_addr(s_nl);
    if (nl_base & 127u) {
        if (threadIdx.x == 0) atomicOr(a.err, kStickyInternal);
        return;
    }
    uint8_t* s_prows = smem + L.prows;
    const uint32_t gb = threadIdx.x / LPB, gl = threadIdx.x % LPB;
    for (uint32_t i = threadIdx.x; i < kV3Tables; i += kPlanSortThreads) {
        const uint32_t j = (i - kV3NLog32) & 31u;
        smem[i] = i < kV3NLog32 ? gf::kTables.exp[i % 255u]
                : i < kV3Log ? (uint8_t)(j ? 255u - gf::kTables.log[j] : 255u)
                : gf::kTables.log[i - kV3Log];
    }
    for (uint32_t i = threadIdx.x; i < M * K; i += kPlanSortThreads) s_prows[i] = a.prows[i];
    uint8_t* s_dall = smem + L.dall;
    if (threadIdx.x < N) s_dall[threadIdx.x] = a.dall[threadIdx.x];
    // the group scratch starts zeroed: the coefficient rows below read O and N past a block's own
    // erasure count (stale or zero shard indices and sums, always table-range values)
    for (uint32_t i = threadIdx.x; i < G * kGroupScratch3 / 4; i += kPlanSortThreads)
        reinterpret_cast<uint32_t*>(smem + L.scratch)[i] = 0u;
    uint8_t* grp = smem + L.scratch + gb * kGroupScratch3;
    uint8_t* S = grp + kV3S;
    uint32_t* Xd = reinterpret_cast<uint32_t*>(grp + kV3X);
    uint32_t* Od = reinterpret_cast<uint32_t*>(grp + kV3O);
    uint32_t* Nd = reinterpret_cast<uint32_t*>(grp + kV3N);
    uint8_t* Dn = grp + kV3D;
    constexpr uint32_t all = N >= 32 ? 0xFFFFFFFFu : (1u << N) - 1u, kmask = (1u << K) - 1u;
    const uint32_t seg0 = blockIdx.x * segs;
    // the first segment's masks in flight while the tables stage
    uint32_t mask_next = seg0 * G + gb < a.nblocks ? a.masks[seg0 * G + gb] : 0u;
    for (uint32_t sg = 0; sg < segs; ++sg) {
        const uint32_t base = (seg0 + sg) * G;
        if (base >= a.nblocks) break;   // workgroup-uniform
        const uint32_t wl = sg % win;
        window_sync(wl);
        const uint32_t b = base + gb;
        const bool valid = b < a.nblocks;
        const uint32_t mask_in = mask_next;
        mask_next = next_mask<G>(a, b, sg, segs);
        uint8_t* P = smem + L.recs + ((size_t)wl * G + gb) * lay.stride;
        const uint32_t mask = valid ? mask_in & all : all;   // past the batch: nothing to rebuild
        const uint32_t e = K - __popc(mask & kmask);
        // the block head: the rule of fec_status.hpp (classify_block) in place, then the record's fields
        int32_t st = a.max_out ? (int32_t)e : 0;
        uint32_t nout = 0;
        if (e != 0) {
            if ((uint32_t)__popc(mask) < K) {
                st = kStTooFew;
                if (gl == 0) wave_flag(a.err, kStickyTooFew);
            } else if (a.max_out && e > a.max_out) {
                st = kStSlots;
                if (gl == 0) wave_flag(a.err, kStickySlots);
            } else {
                nout = e;
            }
        }
        if (gl == 0) {
            P[lay.nout_off] = (uint8_t)nout;
            *reinterpret_cast<uint32_t*>(P + lay.blk_off) = b;
            if (valid && a.status) a.status[b] = st;
        }
        if (nout) {
#pragma unroll
            for (uint32_t t0 = 0; t0 < N; t0 += LPB) {
                const uint32_t t = t0 + gl;
                if (t < N) {
                    const uint32_t below = mask & ((1u << t) - 1u);   // t < 32
                    const uint32_t pos = __popc(below);
                    if (((mask >> t) & 1u) && pos < K) {
                        S[pos] = (uint8_t)t;
                    } else {
                        Xd[t - min(pos, K)] = t;   // not an input: erased, or present past the first K
                        if (t < K && !((mask >> t) & 1u)) Od[t - pos] = t;   // erased data shards below t: t - pos
                    }
                }
            }
        }
        wave_sync();
        if (nout) {
            if (gl < K) P[lay.in_off + gl] = S[gl];
            if (gl < nout) P[lay.out_off + gl] = (uint8_t)Od[gl];
            if (e == 1) {
                one_erasure_row(P + lay.coef_off, S, Od[0], mask, K, gl, s_prows, s_exp, s_log);
            } else {
                uint32_t x[M];
#pragma unroll
                for (uint32_t u = 0; u < M; ++u) x[u] = Xd[u];
#pragma unroll
                for (uint32_t q0 = 0; q0 < K + MAXE; q0 += LPB) {
                    const uint32_t q = q0 + gl;
                    if (q < K + e) {
                        const uint32_t t = q < K ? (uint32_t)S[q] : Od[q - K];
                        const uint32_t tb = nl_base + (t ^ copy5);
                        uint32_t sum = s_dall[t];
#pragma unroll
                        for (uint32_t u = 0; u < M; ++u) sum += lds_ld8(tb ^ x[u]);
                        sum %= 255u;
                        if (q < K) Dn[q] = (uint8_t)(255u - sum);
                        else Nd[q - K] = sum;
                    }
                }
            }
        }
        wave_sync();
        // coefficient rows in chunks of 4, each chunk computed whole (rows past a block's count read
        // stale but in-range scratch, and are not stored) so its 12 LDS loads are in flight together;
        // a chunk runs while some block of the wave needs it
        uint32_t nw = nout;
#pragma unroll
        for (uint32_t o = LPB; o < 64; o <<= 1) nw = max(nw, (uint32_t)__shfl_xor((int)nw, (int)o));
        nw = (uint32_t)__builtin_amdgcn_readfirstlane((int)nw);
        const uint32_t exp_base = lds_addr(s_exp);
#pragma unroll
        for (uint32_t r0 = 0; r0 < MAXE; r0 += 4) {
            if (r0 >= nw || nw < 2 || gl >= K) continue;   // wave-uniform but for gl
            const uint32_t sb = nl_base + ((uint32_t)S[gl] ^ copy5), dn = Dn[gl];
            uint32_t c[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (r0 + j < MAXE) c[j] = lds_ld8(exp_base + Nd[r0 + j] + lds_ld8(sb ^ Od[r0 + j]) + dn);
            uint8_t* C = P + lay.coef_off + gl;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (r0 + j < MAXE && r0 + j < nout && nout >= 2) C[(r0 + j) * K] = (uint8_t)c[j];
        }
        const bool last = sg + 1 >= segs || base + G >= a.nblocks;
        if (wl + 1 < win && !last) continue;   // workgroup-uniform
        sort_window_out(a, smem, L, (wl + 1) * G, base - wl * G);
    }
}

// Segments per workgroup: enough workgroups to fill the chip several times over, each staging the
// tables once for all its segments; a sort window never spans two workgroups.
inline uint32_t plan_segments(uint32_t nseg, uint32_t win) {
    uint32_t segs = std::max<uint32_t>(1, nseg / 4096);
    segs = std::min<uint32_t>(segs, std::max<uint32_t>(64, win));
    return (segs + win - 1) / win * win;
}

// Either form's launch: LPB lanes per block, gscratch bytes of group scratch per block.
template <uint32_t LPB>
hipError_t sorted_launch(const PlanArgs& a, hipStream_t s, uint32_t gscratch,
                         void (*kernel)(PlanArgs, uint32_t, uint32_t)) {
    constexpr uint32_t G = kPlanSortThreads / LPB;
    const uint32_t nseg = (a.nblocks + G - 1) / G;
    if (nseg == 0) return hipSuccess;
    const uint32_t win = sort_window(G), segs = plan_segments(nseg, win);
    const uint32_t grid = (nseg + segs - 1) / segs;
    const size_t lds = sort_lds(a.m, a.k, G, a.lay.stride, win, gscratch).total;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kPlanSortThreads), lds, s, a, segs, win);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_rs_plan_sorted(const PlanArgs& a, hipStream_t s) {
    if (a.k == 16 && a.m == 8 && a.maxe == 8)
        return sorted_launch<code_lanes(16)>(a, s, kGroupScratch3, rs_plan_code_kernel<16, 8>);
    if (a.k == 20 && a.m == 10 && a.maxe == 10)
        return sorted_launch<code_lanes(20)>(a, s, kGroupScratch3, rs_plan_code_kernel<20, 10>);
    switch (plan_lanes(a.k)) {
        case 2: return sorted_launch<2>(a, s, kGroupScratch, rs_plan_sorted_kernel<2>);
        case 4: return sorted_launch<4>(a, s, kGroupScratch, rs_plan_sorted_kernel<4>);
        case 8: return sorted_launch<8>(a, s, kGroupScratch, rs_plan_sorted_kernel<8>);
        case 16: return sorted_launch<16>(a, s, kGroupScratch, rs_plan_sorted_kernel<16>);
        default: return sorted_launch<32>(a, s, kGroupScratch, rs_plan_sorted_kernel<32>);
    }
}

}  // namespace fk
