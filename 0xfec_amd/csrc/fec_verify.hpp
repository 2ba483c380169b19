// fec_verify.hpp — launch interface of the RS verify kernel (fec_verify.hip).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "fec_kernels.hpp"

namespace fk {

// Flat launch as the encode's (EncodeArgs): item = one 16-byte column chunk of one block. What the
// launches that form a chunk's syndromes take (verify, the locate-multi scan and solve): one pass of
// m <= 16 parity rows.
struct SyndromeArgs {
    const uint8_t* in;     // data shard 0 of block 0
    const uint8_t* par;    // the pass's first parity shard of block 0
    uint64_t in_bs, par_bs, ss;
    uint32_t k, m, len, cps;
    uint32_t total;        // nblocks * cps (<= 2^31 per launch)
    FastDiv div_cps;
    const uint32_t* tabs;  // the pass's m * k PermTabs, device memory
};

// One launch checks m <= 16 parity rows; the caller walks longer codes in row passes.
struct VerifyArgs : SyndromeArgs {
    int32_t* status;       // nblocks words, 1 on entry (or 0 from an earlier pass)
    uint32_t* count;       // optional: blocks whose status went from 1 to 0
};

hipError_t launch_rs_verify(const VerifyArgs& a, int grid, hipStream_t s);

}  // namespace fk
