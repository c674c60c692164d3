// vsc_pick_device.h - what the host code of vsc_*_pick (vsc_api.cpp) shares with the kernels of vsc_pick.hip: the
// kernels' arguments and their launch wrappers.  The definition itself is vsc_pick.h.
#pragma once

#include "vsc_enum.h"
#include "vsc_pick.h"

namespace vsc {

constexpr int kPickPerLane = 4;                      // records a lane keeps in registers: a wave selects segments of <= 256 from them
constexpr uint32_t kPickWaveCap = kWave * kPickPerLane;
constexpr uint32_t kPickTile = 1024;                 // candidates per tile of the `picked` passes (run_enumeration)

struct PickArgs {
    PickShape shape;
    const uint4 *loci;                   // [n] vsc_locus
    unsigned long long n;
    const unsigned long long *key;       // [n]
    const uint32_t *target;              // [n], or null: the target comes from the regions
    uint32_t n_targets;
    RegionsView reg;                     // target == null: start[] and the class table ...
    LocateView loc;                      // ... and the label structure
    const uint32_t *group;               // [n_group] target of every input interval (kPickNone: of none); null: the label is the target
    uint32_t n_group;
    const uint32_t *contig_off, *contig_end;  // the genome's table
    uint32_t n_contigs;
    uint32_t *tgt;                       // [n] mark: the target of an eligible candidate, kPickNone for every other
    uint32_t *count;                     // [n_targets] zeroed: eligible candidates per target
    unsigned long long *stats;           // [kPickStats] zeroed
    const unsigned long long *seg_off;   // [n_targets + 1] exclusive scan of count[]
    uint32_t *cursor;                    // [n_targets] zeroed: records appended to the target's segment so far
    uint4 *rec;                          // [n_rec] per eligible candidate (key low, key high, cut coordinate, contig) ...
    uint32_t *rec_index;                 // ... and its index
    unsigned long long n_rec;
    uint32_t *picks;                     // [n_targets * k]
    uint32_t *counts;                    // [n_targets]
    uint32_t *rank;                      // [n] all ones before pick_rank_kernel
};

// the `picked` object: run_enumeration's two passes over tiles of kPickTile candidates, keep = rank[i] != kPickNone
struct PickGatherArgs {
    const unsigned long long *in_codes;  // [n]
    const uint4 *in_loci;
    const uint32_t *rank;
    unsigned long long n;
    const uint32_t *work;                // null: tiles 0 .. n_work - 1
    uint32_t n_work;
    uint32_t *tile_count;
    const unsigned long long *tile_off;
    unsigned long long *codes;
    uint4 *loci;
};

hipError_t launch_pick_mark(const PickArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_pick_scatter(const PickArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_pick_select(const PickArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_pick_rank(const PickArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_pick_gather(const PickGatherArgs &args, bool write, hipStream_t stream);

}  // namespace vsc
