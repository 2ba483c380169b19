// fec_status.hpp — the decode convention every kernel and both host decoders share: the per-block
// status values, the bits of the sticky error word, the one step from a sticky word to a return
// code, and the classification of a block from its erasure counts. Host and device code.
#pragma once

#include <stdint.h>

#include "../../include/fec_hip.h"

#if defined(__HIPCC__)
#define FEC_HD __host__ __device__
#else
#define FEC_HD
#endif

namespace fk {

// ------------------------------------------------------------------ per-block statuses
// What a decode writes into a block's status word when the block fails (a block that succeeds gets
// 0, or from a recover call its rebuilt count e).
constexpr int32_t kStTooFew = -4;     // fewer than k shards present and something to rebuild
constexpr int32_t kStSlots = -1;      // recover: more erased data shards than output slots
constexpr int32_t kStShardSize = -5;  // ragged: the block is longer than the call's max_shard_len
constexpr int32_t kStSingular = -11;  // custom matrix: enough shards and slots, but the rows are dependent
// The locate calls' verdicts (fec_locate.hpp, fec_locate_partial.hpp).
constexpr int32_t kLocateClean = -1;
constexpr int32_t kLocateUnknown = -2;
constexpr int32_t kLocateTooFew = -3;

static_assert(kStTooFew == FEC_ERR_TOO_FEW_SHARDS && kStSlots == FEC_ERR_INVALID_ARG &&
                  kStShardSize == FEC_ERR_SHARD_SIZE && kStSingular == FEC_ERR_SINGULAR,
              "block statuses are the public return codes");
static_assert(kLocateClean == FEC_LOCATE_CLEAN && kLocateUnknown == FEC_LOCATE_UNKNOWN &&
                  kLocateTooFew == FEC_LOCATE_TOO_FEW,
              "locate verdicts are the public values");

// ------------------------------------------------------------------ sticky error bits
// A ctx's sticky error word: kernels OR bits into it (fec_device.hpp wave_flag), fec_sync() reads
// and clears it.
constexpr int kStickyTooFew = 1;    // a block with too few shards
constexpr int kStickySlots = 2;     // a recover block with more erasures than output slots
constexpr int kStickyInternal = 4;  // internal (the form-3 plan kernel's LDS-alignment guard)
constexpr int kStickyOversize = 8;  // a ragged call met a block longer than its max_shard_len
constexpr int kStickySingular = 16; // a block of a custom code whose rows are dependent (fec_solve.hpp)

// The return code of a sticky word (0: FEC_OK). Too few shards comes first, then the internal
// error, then too few slots, then the oversize ragged block, then the singular block.
inline int sticky_rc(int err) {
    if (!err) return FEC_OK;
    return (err & kStickyTooFew)    ? FEC_ERR_TOO_FEW_SHARDS
           : (err & kStickyInternal) ? FEC_ERR_HIP
           : (err & kStickySlots)    ? FEC_ERR_INVALID_ARG
           : (err & kStickyOversize) ? FEC_ERR_SHARD_SIZE
                                     : FEC_ERR_SINGULAR;
}

// ------------------------------------------------------------------ classification
// A block with e erased data shards (to rebuild), npresent shards present in all, of a code with k
// data shards, in a call with max_out output slots per block (0: in place, no limit):
//   e == 0                       nothing to do: status 0
//   npresent < k                 too few shards (this wins over the slot limit)
//   max_out and e > max_out      too few slots
//   else                         nout = e rows to rebuild; recover reports e, in place reports 0
// `bit` is the sticky bit to flag (0: none).
// The kernels that report statuses (rs_plan_kernel, the two sorted plan kernels, the wide plan
// kernel, the direct status pass) spell this rule out in place with the names above: written as a
// call to classify_block() each of them compiled to different machine code. This is
// the statement they are held to: its cases are checked below at compile time, and the host
// self-tests of the reconstruct-some records (fec_selftest.cpp) compare every status and row count
// with it. The code that only chooses what to rebuild (the direct body's row choice, the route
// classify pass) calls block_rebuilds().
struct BlockClass {
    int32_t status;
    uint32_t nout;
    int bit;
};
// The rule's predicate alone: the block is rebuilt (nout = e).
FEC_HD constexpr bool block_rebuilds(uint32_t e, uint32_t npresent, uint32_t k, uint32_t max_out) {
    return e != 0 && npresent >= k && !(max_out && e > max_out);
}
FEC_HD constexpr BlockClass classify_block(uint32_t e, uint32_t npresent, uint32_t k, uint32_t max_out) {
    return block_rebuilds(e, npresent, k, max_out) ? BlockClass{max_out ? (int32_t)e : 0, e, 0}
           : e == 0                                ? BlockClass{0, 0u, 0}
           : npresent < k                          ? BlockClass{kStTooFew, 0u, kStickyTooFew}
                                                   : BlockClass{kStSlots, 0u, kStickySlots};
}
constexpr bool same_class(BlockClass a, int32_t status, uint32_t nout, int bit) {
    return a.status == status && a.nout == nout && a.bit == bit;
}
// RS(4,2): whole; one lost, recover and in place; three lost (a present count below k wins over
// the slot limit); two lost into one slot
static_assert(same_class(classify_block(0, 6, 4, 1), 0, 0, 0) && same_class(classify_block(1, 5, 4, 1), 1, 1, 0) &&
                  same_class(classify_block(1, 5, 4, 0), 0, 1, 0) &&
                  same_class(classify_block(3, 3, 4, 1), kStTooFew, 0, kStickyTooFew) &&
                  same_class(classify_block(2, 4, 4, 1), kStSlots, 0, kStickySlots) &&
                  same_class(classify_block(2, 4, 4, 0), 0, 2, 0),
              "the classification rule");

}  // namespace fk
