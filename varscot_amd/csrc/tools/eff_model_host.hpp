// eff_model_host.hpp - the -Y option of guide_summary and pattern_search: an on-target efficiency model (include/varscot_hip.h
// "on-target efficiency") read from the text file that varscot_amd.EfficiencyModel.to_tsv writes (tools/README.md):
//   shape up site_len down | link identity|logistic | intercept x | gc_range start length | mono pos X w | di pos XY w | gc count w
// one entry per line, tab- or blank-separated, '#' starts a comment; `shape` comes before every weight, `gc_range` before every
// `gc`; what the file does not name weighs 0.  Everything else is refused with the line number.  Host C++ only.
#pragma once

#include <cmath>
#include <set>
#include <sstream>

#include "vsc_host.hpp"

namespace vsc_host {

// the model of `path` (freed with vsc_eff_model_free); *shape = its shape
inline vsc_eff_model *load_eff_model(const std::string &path, vsc_eff_shape *shape)
{
    std::ifstream in(path);
    if (!in) throw std::runtime_error("Could not open the -Y file.");
    vsc_eff_shape s{};
    bool have_shape = false, have_range = false;
    double intercept = 0.0;
    std::vector<double> mono, di, gc;
    std::set<std::string> once;
    std::string line;
    size_t n = 0;
    auto base = [](char c) { return c == 'A' || c == 'a' ? 0 : c == 'C' || c == 'c' ? 1 : c == 'G' || c == 'g' ? 2 : c == 'T' || c == 't' || c == 'U' || c == 'u' ? 3 : -1; };
    while (std::getline(in, line)) {
        ++n;
        const auto bad = [&](const std::string &what) { return std::runtime_error("-Y: " + path + ":" + std::to_string(n) + ": " + what); };
        std::istringstream is(line.substr(0, line.find('#')));
        std::vector<std::string> f;
        for (std::string w; is >> w;) f.push_back(w);
        if (f.empty()) continue;
        const std::string &key = f[0];
        const auto integer = [&](const std::string &v, long *out) {
            char *e = nullptr;
            *out = std::strtol(v.c_str(), &e, 10);
            if (e == v.c_str() || *e) throw bad("'" + v + "' is no integer");
        };
        const auto number = [&](const std::string &v) {
            char *e = nullptr;
            const double x = std::strtod(v.c_str(), &e);
            if (e == v.c_str() || *e || !std::isfinite(x)) throw bad("'" + v + "' is no finite number");
            return x;
        };
        if (key == "shape" || key == "link" || key == "intercept" || key == "gc_range") {
            if (!once.insert(key).second) throw bad("'" + key + "' is given twice");
        } else if ((key == "mono" || key == "di" || key == "gc") && !have_shape) {
            throw bad("'" + key + "' before the 'shape' line");
        }
        long a = 0, b = 0, c = 0;
        if (key == "shape" && f.size() == 4) {
            integer(f[1], &a), integer(f[2], &b), integer(f[3], &c);
            if (a < 0 || a > 16 || c < 0 || c > 16 || b < 16 || b > 32 || a + b + c > 64)
                throw bad("a shape has flanks of 0 .. 16, a site of 16 .. 32 and a context of at most 64 bases");
            s.up = (uint32_t)a, s.site_len = (uint32_t)b, s.down = (uint32_t)c;
            have_shape = true;
            mono.assign(4 * (size_t)(a + b + c), 0.0);
            di.assign(16 * (size_t)(a + b + c - 1), 0.0);
        } else if (key == "link" && f.size() == 2) {
            if (f[1] != "identity" && f[1] != "logistic") throw bad("link must be 'identity' or 'logistic'");
            s.link = f[1] == "logistic" ? VSC_EFF_LOGISTIC : VSC_EFF_IDENTITY;
        } else if (key == "intercept" && f.size() == 2) {
            intercept = number(f[1]);
        } else if (key == "gc_range" && f.size() == 3) {
            integer(f[1], &a), integer(f[2], &b);
            if (a < 0 || b < 0 || a > 64 || b > 64) throw bad("a G/C range lies inside the context");
            if (!gc.empty()) throw bad("'gc_range' behind a 'gc' line");
            s.gc_start = (uint32_t)a, s.gc_len = (uint32_t)b;
            have_range = true;
            gc.assign((size_t)b + 1, 0.0);
        } else if ((key == "mono" || key == "di") && f.size() == 4) {
            const size_t letters = key == "mono" ? 1 : 2;
            integer(f[1], &a);
            const long C = (long)(s.up + s.site_len + s.down);
            if (f[2].size() != letters) throw bad("'" + key + "' takes " + (letters == 1 ? "one letter" : "two letters"));
            if (a < 0 || a > C - (long)letters) throw bad("position " + f[1] + " lies outside the context of " + std::to_string(C));
            int code = 0;
            std::string canon = key + ' ' + std::to_string(a) + ' ';
            for (char ch : f[2]) {
                if (base(ch) < 0) throw bad("'" + f[2] + "' holds a letter that is no base");
                code = 4 * code + base(ch);
                canon += "ACGT"[base(ch)];
            }
            if (!once.insert(canon).second) throw bad("feature (" + f[1] + ", " + f[2] + ") is given twice");
            (letters == 1 ? mono[4 * (size_t)a + (size_t)code] : di[16 * (size_t)a + (size_t)code]) = number(f[3]);
        } else if (key == "gc" && f.size() == 3) {
            if (!have_range) throw bad("'gc' before the 'gc_range' line");
            integer(f[1], &a);
            if (a < 0 || a > (long)s.gc_len || !once.insert("gc " + std::to_string(a)).second)
                throw bad("G/C count " + f[1] + " is given twice or lies outside 0.." + std::to_string(s.gc_len));
            gc[(size_t)a] = number(f[2]);
        } else {
            throw bad("unknown key or wrong number of fields: '" + line + "'");
        }
    }
    if (!have_shape) throw std::runtime_error("-Y: " + path + ": no 'shape' line");
    if (!s.gc_len) s.gc_start = 0;
    vsc_eff_model *model = nullptr;
    if (vsc_eff_model_build(&s, intercept, mono.data(), di.data(), s.gc_len ? gc.data() : nullptr, &model) != VSC_OK)
        throw std::runtime_error("-Y: " + path + ": the library refuses this model (a G/C range that leaves the context?)");
    *shape = s;
    return model;
}

// "%.17g" of a predictor, NA when it is undefined
inline std::string eff_text(double x)
{
    if (std::isnan(x)) return "NA";
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.17g", x);
    return buf;
}

}  // namespace vsc_host
