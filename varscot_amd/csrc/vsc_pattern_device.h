// vsc_pattern_device.h - device helpers that the kernels of vsc_pattern.hip share with those of
// vsc_pattern_bulge.hip (4.19): the front end's start mask of one table (the wave and cell helpers: vsc_cells_device.h).
#pragma once

#include "vsc_cells_device.h"
#include "vsc_device.h"
#include "vsc_pattern.h"

namespace vsc {

// The start mask of one strand: bit b = the site that starts at bit b of the lane's word satisfies the table.
__device__ __forceinline__ uint32_t pattern_starts(const PatFront &f, uint32_t H0, uint32_t H1, uint32_t L0, uint32_t L1)
{
    uint32_t ok = ~0u;
    for (uint32_t i = 0; i < f.n; ++i) {
        const uint32_t e = f.ent[i], j = e & 31u;  // wave-uniform
        const uint32_t h = funnel(H1, H0, j), l = funnel(L1, L0, j);
        const uint32_t tA = 0u - ((e >> 8) & 1u), tC = 0u - ((e >> 9) & 1u), tG = 0u - ((e >> 10) & 1u), tT = 0u - ((e >> 11) & 1u);
        ok &= (~h & ~l & tA) | (~h & l & tC) | (h & ~l & tG) | (h & l & tT);
    }
    return ok;
}

typedef uint32_t v16u __attribute__((ext_vector_type(16)));
typedef const __attribute__((address_space(4))) v16u *const_v16u_ptr;

}  // namespace vsc
