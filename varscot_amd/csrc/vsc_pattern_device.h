// vsc_pattern_device.h - device helpers that the kernels of vsc_pattern.hip share with those of
// vsc_pattern_bulge.hip (4.19): the front end's start mask of one table, the wave's prefix and sum, a wave's run of tiles.
#pragma once

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

// exclusive prefix of v over the lanes of the wave; *total = the wave's sum (enum_kernel's)
__device__ __forceinline__ uint32_t wave_exclusive(uint32_t v, uint32_t lane, uint32_t *total)
{
    uint32_t s = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)s, d, kWave);
        if (lane >= (uint32_t)d) s += o;
    }
    *total = uniform((uint32_t)__shfl((int)s, kWave - 1, kWave));
    return s - v;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, kWave);
    return v;
}

typedef uint32_t v16u __attribute__((ext_vector_type(16)));
typedef const __attribute__((address_space(4))) v16u *const_v16u_ptr;

// tiles [*t0, *t1) of wave `w` of `n_waves`: runs of consecutive tiles, so that the cells a wave stores lie side by side
__device__ __forceinline__ void pattern_tile_run(uint32_t n_tiles, uint32_t w, uint32_t n_waves, uint32_t *t0, uint32_t *t1)
{
    const uint32_t per = (n_tiles + n_waves - 1u) / n_waves;
    const uint64_t first = (uint64_t)w * per;
    *t0 = first < n_tiles ? (uint32_t)first : n_tiles;
    *t1 = first + per < n_tiles ? (uint32_t)(first + per) : n_tiles;
}

}  // namespace vsc
