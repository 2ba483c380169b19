// fec_flat.hpp — the prologue of the flat launches that end in wave-wide votes (fec_verify.hip,
// fec_locate.hip, fec_locate_multi.hip, fec_update.hip): device only.
#pragma once

#include "fec_device.hpp"

namespace fk {

// A lane's item of a flat launch: 16-byte column chunk c of block b.
struct FlatItem {
    uint32_t item, b, c;
    bool live;
};

// The grid is exactly the items' workgroups; a lane past the end (not live) repeats the last item
// and reports or stores nothing, so every lane of a wave reaches the kernel's ballots.
__device__ __forceinline__ FlatItem flat_item(uint32_t total, uint32_t cps, const FastDiv& div_cps) {
    FlatItem f;
    f.item = xcd_order() * kThreads + threadIdx.x;
    f.live = f.item < total;
    const uint32_t it = min(f.item, total - 1u);
    f.b = fdiv(it, div_cps);
    f.c = it - f.b * cps;
    return f;
}

}  // namespace fk
