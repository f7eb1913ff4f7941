#include "exclude.h"

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <unordered_map>

namespace bdhost {

namespace {

// a non-negative decimal integer, clamped to 2^31 - 1; false: not one
bool parse_coordinate(const std::string& s, bool* negative, int32_t* out) {
    *negative = false;
    size_t i = 0;
    if (i < s.size() && (s[i] == '+' || s[i] == '-')) { *negative = s[i] == '-'; ++i; }
    if (i == s.size()) return false;
    int64_t v = 0;
    for (; i < s.size(); ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        v = std::min<int64_t>(v * 10 + (s[i] - '0'), (int64_t)1 << 40);
    }
    if (v == 0) *negative = false;
    *out = (int32_t)std::min<int64_t>(v, 0x7FFFFFFF);
    return true;
}

}  // namespace

void read_exclude_bed(const std::string& path, const std::vector<std::string>& targets, ExcludeTable& out) {
    std::ifstream in(path.c_str());
    if (!in.is_open()) throw std::runtime_error("unable to open exclude file '" + path + "'");
    std::unordered_map<std::string, int32_t> tid_of;
    for (size_t t = 0; t < targets.size(); ++t) tid_of.emplace(targets[t], (int32_t)t);   // (the first of equal names, as tid_of of the readers)
    out.path = path;
    out.unknown_lines = 0;
    std::vector<bdx_interval> raw;
    std::string line;
    size_t lineno = 0;
    auto bad = [&](const std::string& what) { return std::runtime_error(path + ":" + std::to_string(lineno) + ": " + what); };
    while (std::getline(in, line)) {
        ++lineno;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        std::vector<std::string> f;
        for (size_t i = 0; i < line.size() && f.size() < 3;) {
            while (i < line.size() && (line[i] == '\t' || line[i] == ' ')) ++i;
            size_t j = i;
            while (j < line.size() && line[j] != '\t' && line[j] != ' ') ++j;
            if (j > i) f.push_back(line.substr(i, j - i));
            i = j;
        }
        if (f.empty() || line[0] == '#' || line.compare(0, 5, "track") == 0 || line.compare(0, 7, "browser") == 0) continue;
        if (f.size() < 3) throw bad("fewer than three fields");
        int32_t b = 0, e = 0;
        bool nb = false, ne = false;
        if (!parse_coordinate(f[1], &nb, &b) || !parse_coordinate(f[2], &ne, &e)) throw bad("a coordinate is not an integer");
        if (nb || ne) throw bad("a coordinate is negative");
        if (e < b) throw bad("end before begin");
        auto t = tid_of.find(f[0]);
        if (t == tid_of.end()) { ++out.unknown_lines; continue; }
        if (b == e) continue;   // (an empty interval)
        raw.push_back(bdx_interval{t->second, b, e});
    }
    if (in.bad()) throw std::runtime_error("unable to read exclude file '" + path + "'");
    const size_t n = bdx::exclude_build(raw.data(), raw.size(), out.first, out.beg, out.end);
    if (n > bdx::kMaxExcludeIntervals) throw std::runtime_error(path + ": more than 2^24 intervals after merging (" + bdx_strerror(BDX_ELIMIT) + ")");
    out.intervals.clear();
    for (size_t t = 0; t + 1 < out.first.size(); ++t)
        for (uint32_t i = out.first[t]; i < out.first[t + 1]; ++i) out.intervals.push_back(bdx_interval{(int32_t)t, out.beg[i], out.end[i]});
}

void print_exclude_timing(const ExcludeTable& t) {
    fprintf(stderr, "[bdx timing] excluded %llu records in %zu intervals (%zu BED lines on unknown sequences ignored)\n",
            (unsigned long long)t.dropped.load(), t.beg.size(), t.unknown_lines);
}

}  // namespace bdhost
