// mh_host.hpp - the -H and -m options of guide_summary and pattern_search: the microhomology and out-of-frame scores of the
// guides that -E finds (include/varscot_hip.h "microhomology and out-of-frame scores"; tools/README.md).
//   -H FLANK[,CUT]     the window: FLANK bases (8 .. 32) on either side of the break, which lies between read positions CUT - 1
//                      and CUT of the site (default: the tool's - 17 for the 23-mers of guide_summary)
//   -m MIN_OOF[,MIN_MH] floors: the out-of-frame share in per cent (0 .. 100) and the microhomology score; needs -H
// The per cent become per mille and the score tenths HERE, once: round(10 * MIN_OOF), ceil(10 * MIN_MH).  Host C++ only.
#pragma once

#include <cmath>

#include "eff_model_host.hpp"

namespace vsc_host {

struct MhOptions {
    bool on = false, floored = false;
    vsc_mh_shape shape{};
    uint32_t min_sum = 0, min_oof_permille = 0;
};

// "" and *o filled, or the message of a refusal
inline std::string parse_mh_options(bool h_set, const std::string &h, bool m_set, const std::string &m, bool enumerating, uint32_t site_len,
                                    uint32_t default_cut, MhOptions *o)
{
    if (m_set && !h_set) return "-m is a floor on the scores of the -H window: give -H";
    if (!h_set) return "";
    if (!enumerating) return "-H scores the guides that -E finds: give -E";
    const auto numbers = [](const std::string &v, double *a, double *b, bool *two) {
        char *e = nullptr;
        *a = std::strtod(v.c_str(), &e);
        if (e == v.c_str() || std::isnan(*a)) return false;
        *two = *e == ',';
        if (!*two) return *e == 0;
        const char *second = e + 1;
        *b = std::strtod(second, &e);
        return e != second && *e == 0 && !std::isnan(*b);
    };
    double a = 0, b = 0;
    bool two = false;
    if (!numbers(h, &a, &b, &two) || a != std::floor(a) || a < 8 || a > 32 || (two && (b != std::floor(b) || b < 0 || b > site_len)))
        return "-H takes FLANK[,CUT]: 8 .. 32 bases on either side of the break, the break in front of read position 0 .. " +
               std::to_string(site_len) + ", not '" + h + "'";
    o->on = true;
    o->shape = vsc_mh_shape{site_len, two ? (uint32_t)b : default_cut, (uint32_t)a, 0};
    if (m_set) {
        if (!numbers(m, &a, &b, &two) || a < 0 || a > 100 || (two && (b < 0 || b > 400000)))
            return "-m takes MIN_OOF[,MIN_MH]: the out-of-frame share in per cent, 0 .. 100, and the microhomology score, not '" + m + "'";
        o->floored = true;
        o->min_oof_permille = (uint32_t)std::llround(10.0 * a);
        o->min_sum = two ? (uint32_t)std::ceil(10.0 * b - 1e-9) : 0u;
    }
    return "";
}

// "\tmhScore\toofScore" of a (sum, oof) pair: %.17g, NA where the pair is undefined
inline std::string mh_columns(const uint32_t *pair)
{
    double mh = 0, oof = 0;
    if (vsc_mh_scores(pair[0], pair[1], &mh, &oof) != VSC_OK) throw std::runtime_error("a microhomology pair with oof > sum");
    return '\t' + eff_text(mh) + '\t' + eff_text(oof);
}

}  // namespace vsc_host
