// vsc_enum.h - what the host code of vsc_guides_enumerate (vsc_api.cpp) shares with its kernels (vsc_enum.hip).  A header of
// its own, so that the structs of vsc_internal.h - and with them the other kernels' translation units - stay what they were.
#pragma once

#include "vsc_internal.h"

namespace vsc {

struct EnumArgs {
    const uint32_t *hi, *lo, *nm;  // device planes, as ScanArgs
    uint32_t first_pos;            // global position of bit 0 of element 0
    const uint32_t *work;          // [n_work] ascending tiles of the shard to visit; null: tile i is work item i
    uint32_t n_work;
    PamMasks pam;                  // the guide's PAM
    uint32_t keep_fwd, keep_rev;   // all ones / zero: the strand is wanted
    uint32_t filter;               // non-zero: a GC bound or a T-run limit is set (else no window is looked at one by one)
    uint32_t gc_min, gc_max;       // G / C among the 20 protospacer bases (gc_max = 20: no upper bound)
    uint32_t max_t_run;            // 0: no limit
    RegionsView reg;               // kRegions kernels only
    const uint32_t *contig_off, *contig_end;
    uint32_t n_contigs;
    uint32_t *tile_count;          // [n_work] count pass: candidates kept per work item
    const unsigned long long *tile_off;  // [n_work + 1] write pass: candidates of all earlier work items
    unsigned long long *codes;     // out: vsc_pack_guide codes
    uint4 *loci;                   // out: vsc_locus {contig, pos, strand, 0}
};

hipError_t launch_enum(const EnumArgs &args, bool write, bool regions, hipStream_t stream);
hipError_t launch_enum_scan(const uint32_t *tile_count, uint32_t n, unsigned long long *tile_off, hipStream_t stream);

}  // namespace vsc
