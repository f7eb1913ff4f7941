#include "sites.h"

#include <algorithm>
#include <fstream>
#include <stdexcept>
#include <unordered_map>

namespace bdhost {

const char* const kSiteTypes[5] = {"DEL", "INS", "INV", "ITX", "CTX"};

namespace {

// a decimal integer with an optional sign, |value| clamped to 2^40; false: not one
bool parse_integer(const std::string& s, long long* out) {
    size_t i = 0;
    bool negative = false;
    if (i < s.size() && (s[i] == '+' || s[i] == '-')) { negative = s[i] == '-'; ++i; }
    if (i == s.size()) return false;
    long long v = 0;
    for (; i < s.size(); ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        v = std::min<long long>(v * 10 + (s[i] - '0'), 1LL << 40);
    }
    *out = negative ? -v : v;
    return true;
}

}  // namespace

void read_sites(const std::string& path, const std::vector<std::string>& targets, const std::vector<std::pair<std::string, uint32_t>>& type_masks,
                SiteTable& out) {
    std::ifstream in(path.c_str());
    if (!in.is_open()) throw std::runtime_error("unable to open sites file '" + path + "'");
    std::unordered_map<std::string, int32_t> tid_of;
    for (size_t t = 0; t < targets.size(); ++t) tid_of.emplace(targets[t], (int32_t)t);   // (the first of equal names, as tid_of of the readers)
    out.path = path;
    out.sites.clear();
    out.unknown_lines = 0;
    std::string line;
    size_t lineno = 0;
    auto bad = [&](const std::string& what) { return std::runtime_error(path + ":" + std::to_string(lineno) + ": " + what); };
    while (std::getline(in, line)) {
        ++lineno;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#' || line.find_first_not_of(" \t") == std::string::npos) continue;
        std::vector<std::string> f;
        for (size_t i = 0; f.size() < 8;) {
            const size_t j = line.find('\t', i);
            f.push_back(line.substr(i, j == std::string::npos ? std::string::npos : j - i));
            if (j == std::string::npos) break;
            i = j + 1;
        }
        if (f.size() < 7) throw bad("fewer than seven fields (Chr1 Pos1 Orientation1 Chr2 Pos2 Orientation2 Type)");
        long long p1 = 0, p2 = 0;
        if (!parse_integer(f[1], &p1) || !parse_integer(f[4], &p2) || p1 < 1 || p2 < 1 || p1 > 0x7FFFFFFF || p2 > 0x7FFFFFFF)
            throw bad("a position is not an integer >= 1");
        SiteLine s;
        s.type = f[6];
        bool known = false;
        for (const char* t : kSiteTypes) known = known || s.type == t;
        if (!known) throw bad("type '" + s.type + "' is not one of DEL INS INV ITX CTX");
        uint32_t mask = 0;
        for (auto const& tm : type_masks)
            if (tm.first == s.type) mask = tm.second;
        if (!mask) throw bad("no read class maps to type " + s.type + " with this run's -l setting");
        if ((s.type == "CTX") == (f[0] == f[3]))
            throw bad(s.type == "CTX" ? "CTX with both ends on one sequence" : "type " + s.type + " with its ends on two sequences");
        if (f.size() > 7) s.has_size = parse_integer(f[7], &s.size);
        auto t1 = tid_of.find(f[0]), t2 = tid_of.find(f[3]);
        if (t1 == tid_of.end() || t2 == tid_of.end()) { ++out.unknown_lines; continue; }
        s.chr1 = t1->second; s.pos1 = (int32_t)p1; s.chr2 = t2->second; s.pos2 = (int32_t)p2;
        const bool swap = s.chr1 > s.chr2 || (s.chr1 == s.chr2 && s.pos1 > s.pos2);
        s.site = swap ? bdx_site{s.chr2, s.pos2, s.chr1, s.pos1, mask} : bdx_site{s.chr1, s.pos1, s.chr2, s.pos2, mask};
        out.sites.push_back(s);
    }
    if (in.bad()) throw std::runtime_error("unable to read sites file '" + path + "'");
}

}  // namespace bdhost
