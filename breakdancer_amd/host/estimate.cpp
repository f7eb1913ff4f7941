#include "estimate.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>

#include "../csrc/bdx_estimate.h"

namespace bdhost {

namespace {

std::string two_decimals(double v) {
    char buf[64];
    snprintf(buf, sizeof buf, "%.2f", v);
    return buf;
}

struct Printed { std::string lower, upper, mean, std; };

// one line of the configuration with the four insert-size fields replaced
std::string rewrite_line(const std::string& line, const Printed& p, uint64_t n_kept) {
    std::vector<std::string> fields;
    size_t b = 0;
    while (true) {
        const size_t e = line.find('\t', b);
        const std::string f = line.substr(b, e == std::string::npos ? std::string::npos : e - b);
        const size_t colon = f.find(':');
        bool keep = true;
        std::string field = f;
        if (colon != std::string::npos) {
            const std::string key = f.substr(0, colon);
            const Field fn = translate_token(key);
            keep = fn != INSERT_SIZE_MEAN && fn != INSERT_SIZE_STDDEV && fn != INSERT_SIZE_UPPER_CUTOFF && fn != INSERT_SIZE_LOWER_CUTOFF;
            if (keep && key == "num") field = "num:" + std::to_string(n_kept);
        }
        if (keep) fields.push_back(field);
        if (e == std::string::npos) break;
        b = e + 1;
    }
    for (const std::string& f : {"lower:" + p.lower, "upper:" + p.upper, "mean:" + p.mean, "std:" + p.std}) fields.push_back(f);
    std::string out;
    for (size_t i = 0; i < fields.size(); ++i) out += (i ? "\t" : "") + fields[i];
    return out;
}

// the library a line names, as the parser resolves it (config.cpp: lib\w*$, else samp\w*$; the last field of a kind wins)
std::string library_of_line(const std::string& line) {
    std::map<Field, std::string> dir;
    size_t b = 0;
    while (true) {
        const size_t e = line.find('\t', b);
        const std::string f = line.substr(b, e == std::string::npos ? std::string::npos : e - b);
        const size_t colon = f.find(':');
        if (colon != std::string::npos) {
            const Field fn = translate_token(f.substr(0, colon));
            if (fn != UNKNOWN_FIELD) dir[fn] = f.substr(colon + 1);
        }
        if (e == std::string::npos) break;
        b = e + 1;
    }
    if (dir.count(LIBRARY_NAME)) return dir[LIBRARY_NAME];
    if (dir.count(SAMPLE_NAME)) return dir[SAMPLE_NAME];
    return "";
}

}  // namespace

EstimatePlan plan_estimate(const BamConfig& cfg, const std::string& config_text, int cut_sd, const uint64_t* hist, const uint64_t* n_over) {
    EstimatePlan plan;
    const size_t nlibs = cfg.num_libs();
    plan.est.resize(nlibs);
    plan.n_over.assign(n_over, n_over + nlibs);
    plan.libs = cfg.abi_libs();
    std::map<std::string, size_t> index;
    std::vector<Printed> printed(nlibs);
    for (size_t i = 0; i < nlibs; ++i) {
        const LibraryConfig& lc = cfg.library_config(i);
        index[lc.name] = i;
        bdx_insert_estimate& e = plan.est[i];
        bdx::estimate_insert_size(hist + i * (size_t)BDX_ISIZE_BINS, &e);
        if (!e.valid) {
            plan.warnings.push_back("--estimate: library " + lc.name + " has no valid estimate (n_kept=" + std::to_string(e.n_kept) +
                                    "): it keeps the configuration's values");
            if (!lc.has_mean && !lc.has_std && plan.fatal.empty())
                plan.fatal = "--estimate: library " + lc.name + " has no valid estimate (n_kept=" + std::to_string(e.n_kept) +
                             ") and its configuration line gives neither mean nor std";
            continue;
        }
        const double upper = e.mean + cut_sd * e.sd_plus;
        const double lower = std::max(0.0, e.mean - cut_sd * e.sd_minus);
        Printed& p = printed[i];
        p.lower = two_decimals(lower); p.upper = two_decimals(upper); p.mean = two_decimals(e.mean); p.std = two_decimals(e.sd);
        bdx_lib& l = plan.libs[i];
        l.mean_insertsize = strtof(p.mean.c_str(), nullptr); l.std_insertsize = strtof(p.std.c_str(), nullptr);
        l.uppercutoff = strtof(p.upper.c_str(), nullptr); l.lowercutoff = strtof(p.lower.c_str(), nullptr);
    }
    int w = 100000000;
    for (const bdx_lib& l : plan.libs) {
        const int t = l.mean_insertsize - l.readlens * 2;   // (float arithmetic, truncated: config.cpp's)
        w = std::min(w, t);
    }
    plan.window = std::max(w, 50);
    // the text: the parser stops at the first empty line, what follows it is kept as it is
    size_t b = 0;
    bool live = true;
    while (b <= config_text.size()) {
        const size_t e = config_text.find('\n', b);
        const std::string line = config_text.substr(b, e == std::string::npos ? std::string::npos : e - b);
        if (line.empty()) live = false;
        std::string out = line;
        if (live) {
            const auto it = index.find(library_of_line(line));
            if (it != index.end() && plan.est[it->second].valid) out = rewrite_line(line, printed[it->second], plan.est[it->second].n_kept);
        }
        plan.config_text += out;
        if (e == std::string::npos) break;
        plan.config_text += '\n';
        b = e + 1;
    }
    return plan;
}

std::string estimate_summary(const BamConfig& cfg, const EstimatePlan& plan) {
    std::string s;
    for (size_t i = 0; i < plan.est.size(); ++i) {
        const bdx_insert_estimate& e = plan.est[i];
        const bdx_lib& l = plan.libs[i];
        char buf[512];
        snprintf(buf, sizeof buf, "%slibrary %s: n=%llu n_over=%llu n_kept=%llu mean=%.2f std=%.2f lower=%.2f upper=%.2f %s", i ? "; " : "",
                 cfg.library_config(i).name.c_str(), (unsigned long long)e.n, (unsigned long long)plan.n_over[i], (unsigned long long)e.n_kept,
                 l.mean_insertsize, l.std_insertsize, l.lowercutoff, l.uppercutoff, e.valid ? "valid" : "not valid");
        s += buf;
    }
    return s;
}

}  // namespace bdhost
