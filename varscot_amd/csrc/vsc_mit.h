// vsc_mit.h - calcMitScore on the device, shared by the kernels that score hits where they lie (vsc_kernels.hip: scores, summary,
// selection; vsc_variants.hip: the variant merge).  Device code only: include it from a .hip file.
#pragma once

#include "vsc_internal.h"

namespace vsc {

// variant_processing/mit_score.h:42 - position weights
static __constant__ double kMitWeights[20] = {0,     0,     0.014, 0,     0,     0.395, 0.317, 0,     0.389, 0.079,
                                       0.445, 0.508, 0.613, 0.851, 0.732, 0.828, 0.615, 0.804, 0.685, 0.583};

// calcMitScore (variant_processing/mit_score.h:12-68) on the set bits of `mask` (ascending positions,
// forward-genome window coordinates - merge_output_bam.h:549 passes the MD-derived positions as is).
// fp64 with the reference's operation order; contraction off so no multiply-add is fused.
__device__ inline double mit_score(uint32_t mask, int *ub)
{
#pragma clang fp contract(off)
    *ub = 0;
    const int n = __popc(mask);
    if (n == 0) return 100.0;  // perfectMatch {-1}, :19-22,38-41
    const int last = 31 - __clz(mask);
    const unsigned nm = last < 20 ? (unsigned)n : (unsigned)n - 1u;  // :26-33
    if (nm == 0) return 100.0;                                       // :38-41
    const double s3 = (double)1 / ((double)nm * (double)nm);        // :35, pow(nm, 2) is exact
    double s1 = 1;
    int dist_sum = 0, prev = 0;
    uint32_t rest = mask;
    for (unsigned i = 0; i < nm; ++i) {  // :48-55
        const int p = __ffs(rest) - 1;
        rest &= rest - 1u;
        double wgt = 0;
        if (p < 20) wgt = kMitWeights[p]; else *ub = 1;  // the reference reads past its 20-entry table here
        s1 *= (1 - wgt);
        if (i > 0) dist_sum += p - prev;
        prev = p;
    }
    double s2;
    if (nm < 2) {  // :57-60
        s2 = 1;
    } else {
        const double avg = (double)dist_sum / (double)(nm - 1u);  // :63
        s2 = 1 / (((19 - avg) / 19) * 4 + 1);                      // :64
    }
    return s1 * s2 * s3 * 100;  // :66
}

}  // namespace vsc
