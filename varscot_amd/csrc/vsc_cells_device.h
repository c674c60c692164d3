// vsc_cells_device.h - device helpers of the count / scan / write searches (vsc_bulge.hip, vsc_pattern.hip,
// vsc_pattern_bulge.hip): the wave's sum and prefix, a wave's run of tiles, the launch grid over the tiles and
// the offset of a cell (guide of the round, strand, tile) behind one or two levels of sums.  vsc_enum.hip keeps a prefix of
// its own: its total stays in a vector register, and enum_kernel's instructions change with the one below.
#pragma once

#include "vsc_device.h"

namespace vsc {

constexpr uint32_t kCellChunk = kWave;  // cells per chunk, chunks per group (kBulgeChunk, kPatChunk): one load per lane

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, kWave);
    return v;
}

// exclusive prefix of v over the lanes of the wave
__device__ __forceinline__ uint32_t wave_exclusive(uint32_t v, uint32_t lane)
{
    uint32_t s = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)s, d, kWave);
        if (lane >= (uint32_t)d) s += o;
    }
    return s - v;
}

// ... and *total = the wave's sum
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

// exclusive prefix of v over the workgroup's threads and *total = the sum; ws: kWavesPerGroup words of LDS (the selection
// walks of vsc_pattern.hip and vsc_bulge_table.hip)
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t *ws, uint32_t *total)
{
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    uint32_t wave_total;
    const uint32_t in_wave = wave_exclusive(v, lane, &wave_total);
    block_sync();  // (the last step's readers of ws are done)
    if (lane == 0) ws[wave] = wave_total;
    block_sync();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kWavesPerGroup; ++k) {
        const uint32_t t = ws[k];
        before += k < wave ? t : 0u;
        all += t;
    }
    *total = all;
    return before + in_wave;
}

// tiles [*t0, *t1) of wave `w` of `n_waves`: runs of consecutive tiles, so that the cells a wave stores lie side by side
__device__ __forceinline__ void cell_tile_run(uint32_t n_tiles, uint32_t w, uint32_t n_waves, uint32_t *t0, uint32_t *t1)
{
    const uint32_t per = (n_tiles + n_waves - 1u) / n_waves;
    const uint64_t first = (uint64_t)w * per;
    *t0 = first < n_tiles ? (uint32_t)first : n_tiles;
    *t1 = first + per < n_tiles ? (uint32_t)(first + per) : n_tiles;
}

// hits of all cells before `cell`, one level of sums: the chunk's offset + the cells of the chunk in front of it (one load
// per lane)
__device__ __forceinline__ unsigned long long cell_offset(const uint32_t *count, const unsigned long long *chunk_off, unsigned long long cell,
                                                          uint32_t lane)
{
    const unsigned long long first = cell & ~(unsigned long long)(kCellChunk - 1u);
    const uint32_t before = wave_sum(lane < (uint32_t)(cell - first) ? count[first + lane] : 0u);
    return chunk_off[cell / kCellChunk] + before;
}

// ... two levels: the offset of its group of 64 chunks + the chunks of the group in front of its own + the cells of the chunk
// in front of it (two loads per lane)
__device__ __forceinline__ unsigned long long cell_offset(const uint32_t *count, const uint32_t *chunk_sum, const unsigned long long *group_off,
                                                          unsigned long long cell, uint32_t lane)
{
    const unsigned long long chunk = cell / kCellChunk, group = chunk / kCellChunk;
    const unsigned long long first_chunk = group * kCellChunk, first_cell = chunk * kCellChunk;
    const uint32_t chunks = wave_sum(lane < (uint32_t)(chunk - first_chunk) ? chunk_sum[first_chunk + lane] : 0u);
    const uint32_t cells = wave_sum(lane < (uint32_t)(cell - first_cell) ? count[first_cell + lane] : 0u);
    return group_off[group] + chunks + cells;
}

// 8 workgroups of 4 waves per CU fill every SIMD's 8 wave slots; fewer when the tiles do not need them
static inline dim3 cell_grid(uint32_t n_tiles, int n_cus)
{
    const uint32_t want = (n_tiles + kWavesPerGroup - 1) / kWavesPerGroup;
    const uint32_t cap = (uint32_t)(n_cus > 0 ? n_cus : 256) * 8u;
    return dim3(want < cap ? want : cap);
}

}  // namespace vsc
