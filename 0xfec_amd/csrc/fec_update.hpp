// fec_update.hpp — launch interface of the RS parity-update kernel (fec_update.hip).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "fec_kernels.hpp"

namespace fk {

// Flat launch as the encode's (EncodeArgs): item = one 16-byte column chunk of one block. One
// launch folds the masked columns into m <= 16 parity rows; the caller walks longer codes in row
// passes, each of which reads the masked columns again.
struct UpdateArgs {
    const uint8_t* in;     // shard 0 of block 0 of the folded data (update: the new version)
    const uint8_t* old;    // update: shard 0 of block 0 of the old version; encode-idx: null
    uint8_t* par;          // the pass's first parity shard of block 0
    uint64_t in_bs, old_bs, par_bs, ss;
    uint32_t k, m, len, cps;
    uint32_t total;        // nblocks * cps (<= 2^31 per launch)
    uint32_t nblocks;      // blocks of this launch (total / cps)
    FastDiv div_cps;
    const uint32_t* tabs;  // the pass's m * k PermTabs, device memory
    const uint32_t* masks; // mask_words words per block, the launch's first block first
    uint32_t mask_words;
};

hipError_t launch_rs_update(const UpdateArgs& a, int grid, hipStream_t s);

}  // namespace fk
