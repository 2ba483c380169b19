// fec_update.hip — RS parity update for gfx950 (klauspost Encoder.Update and Encoder.EncodeIdx,
// batched): parity_i ^= sum over a block's masked columns j of M[k+i][j] * delta_j, with delta_j =
// old_j ^ new_j (update) or data_j (encode-idx). The verify kernel's body (fec_verify.hip): the
// accumulators start from the stored parity; here only the masked columns are folded in, and the
// accumulators are stored back.
#include "fec_flat.hpp"
#include "fec_update.hpp"

namespace fk {

// Word w of the column masks of the wave's <= 3 blocks (bfirst, +1, +2, clamped to the launch), by
// scalar loads as wave_masks() (fec_device.hpp) loads one-word masks.
__device__ __forceinline__ WaveMasks wave_mask_words(const uint32_t* masks, uint32_t words, uint32_t w,
                                                     uint32_t bfirst, uint32_t nblocks) {
    typedef __attribute__((address_space(4))) const uint32_t ConstU32;
    ConstU32* cm = (ConstU32*)masks;
    const uint32_t last = nblocks - 1;
    const uint32_t b1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(bfirst + 1, last));
    const uint32_t b2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(bfirst + 2, last));
    return {cm[(uint64_t)bfirst * words + w], cm[(uint64_t)b1 * words + w], cm[(uint64_t)b2 * words + w]};
}

// One lane = one 16-byte column chunk of one block. Each lane walks the set bits of its own block's
// mask, a word at a time and G columns at a time (G loads in flight per lane; two per column with
// HAS_OLD, so half as many columns); the walk of a word goes on while any lane of the wave has a
// bit left, and a lane that has none loads nothing and folds zeros. The column index is per lane,
// so the PermTab addresses are (lanes of one block share them: an LDS broadcast).
//
// A block with an empty mask is neither read nor written: the mask comes first, and the parity
// loads, which go out ahead of the data loads, are predicated on it. Masks of long shards (a wave
// spans at most 3 blocks when cps >= 32) come by scalar loads, else by one vector load per lane.
template <int MAXM, bool HAS_OLD, bool LDS_TABS>
__global__ __launch_bounds__(kThreads) void rs_update_kernel(UpdateArgs a) {
    // 8 or 16 rows with 8 columns in flight take 174 / 256 VGPRs (2 / 1 waves per SIMD), with 4
    // columns 154 / 244 (3 / 2): chosen by the register count, not by a timing
    constexpr int G = (HAS_OLD || MAXM >= 8) ? kInGroup / 2 : kInGroup;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const gf::PermTab* tabs = stage_tabs<LDS_TABS>(a.tabs, a.m * a.k * 8, smem);
    if constexpr (LDS_TABS) __syncthreads();
    const uint32_t k = a.k, m = a.m, kw = (k + 31u) >> 5;
    const FlatItem f = flat_item(a.total, a.cps, a.div_cps);
    const uint32_t b = f.b, c = f.c;
    const bool scalar = a.cps >= 32u;   // uniform
    const uint32_t bfirst = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
    auto word = [&](uint32_t w) -> uint32_t {   // the lane's block's columns 32 w .. 32 w + 31 below k
        const uint32_t v = scalar ? wave_mask_words(a.masks, a.mask_words, w, bfirst, a.nblocks).of(b - bfirst)
                                  : a.masks[(uint64_t)b * a.mask_words + w];
        return v & low_mask(k - 32u * w);
    };
    const uint32_t w0 = word(0);
    uint32_t any = w0;
    for (uint32_t w = 1; w < kw; ++w) any |= word(w);
    const bool go = any != 0;
    if (__ballot(go) == 0) return;   // wave-uniform; no barrier follows

    const uint8_t* src = a.in + (uint64_t)b * a.in_bs + (uint64_t)c * kChunk;
    const uint8_t* old = HAS_OLD ? a.old + (uint64_t)b * a.old_bs + (uint64_t)c * kChunk : nullptr;
    uint8_t* par = a.par + (uint64_t)b * a.par_bs + (uint64_t)c * kChunk;
    uint32_t acc[MAXM][4];
#pragma unroll
    for (int r = 0; r < MAXM; ++r) {
        const uint4 p = (r < (int)m && go) ? ld16<true>(par + (uint64_t)r * a.ss) : make_uint4(0, 0, 0, 0);
        acc[r][0] = p.x, acc[r][1] = p.y, acc[r][2] = p.z, acc[r][3] = p.w;
    }
    for (uint32_t w = 0; w < kw; ++w) {
        uint32_t bits = w == 0 ? w0 : word(w);   // zero in every lane of a block with an empty mask
        while (__ballot(bits != 0) != 0) {
            uint4 x[G];
            uint32_t j[G];
            bool has[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                has[g] = bits != 0;
                j[g] = has[g] ? 32u * w + (uint32_t)__ffs((int)bits) - 1u : 0u;
                bits &= bits - 1u;
                x[g] = has[g] ? ld16<true>(src + (uint64_t)j[g] * a.ss) : make_uint4(0, 0, 0, 0);
            }
            if constexpr (HAS_OLD) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const uint4 o = has[g] ? ld16<true>(old + (uint64_t)j[g] * a.ss) : make_uint4(0, 0, 0, 0);
                    x[g].x ^= o.x, x[g].y ^= o.y, x[g].z ^= o.z, x[g].w ^= o.w;
                }
            }
            // a lane without column g holds zeros and table 0 of the row: its product is zero
#pragma unroll
            for (int g = 0; g < G; g += 2) {
                if (__ballot(has[g + 1]) != 0) {
                    Idx ia[4], ib[4];
                    split4(ia, x[g]);
                    split4(ib, x[g + 1]);
#pragma unroll
                    for (int r = 0; r < MAXM; ++r)
                        if (r < (int)m) mac2(acc[r], ia, ib, tabs + r * k + j[g], tabs + r * k + j[g + 1]);
                } else if (__ballot(has[g]) != 0) {
                    Idx ia[4];
                    split4(ia, x[g]);
#pragma unroll
                    for (int r = 0; r < MAXM; ++r)
                        if (r < (int)m) mac1(acc[r], ia, tabs + r * k + j[g]);
                }
            }
        }
    }
    if (f.live && go) {
#pragma unroll
        for (int r = 0; r < MAXM; ++r)
            if (r < (int)m) store_chunk<true>(par + (uint64_t)r * a.ss, as_uint4(acc[r]), a.len - c * kChunk);
    }
}

template <int MAXM, bool HAS_OLD>
static hipError_t update_dispatch(const UpdateArgs& a, int grid, hipStream_t s) {
    if (a.m * a.k <= (uint32_t)kMaxLdsTabs) {
        const size_t lds = (size_t)a.m * a.k * sizeof(gf::PermTab);
        hipLaunchKernelGGL((rs_update_kernel<MAXM, HAS_OLD, true>), dim3(grid), dim3(kThreads), lds, s, a);
    } else {
        hipLaunchKernelGGL((rs_update_kernel<MAXM, HAS_OLD, false>), dim3(grid), dim3(kThreads), 0, s, a);
    }
    return hipGetLastError();
}

template <int MAXM>
static hipError_t update_rows(const UpdateArgs& a, int grid, hipStream_t s) {
    return a.old ? update_dispatch<MAXM, true>(a, grid, s) : update_dispatch<MAXM, false>(a, grid, s);
}

hipError_t launch_rs_update(const UpdateArgs& a, int grid, hipStream_t s) {
    if (a.total == 0 || a.m == 0) return hipSuccess;
    if (a.m <= 1) return update_rows<1>(a, grid, s);
    if (a.m <= 2) return update_rows<2>(a, grid, s);
    if (a.m <= 4) return update_rows<4>(a, grid, s);
    if (a.m <= 8) return update_rows<8>(a, grid, s);
    return update_rows<16>(a, grid, s);   // the caller splits m > 16
}

}  // namespace fk
