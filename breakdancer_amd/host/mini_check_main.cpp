// bdx-mini-check ROWS --n N0,N1,.. --mu M0,M1,.. --window W --step S [--min-pairs P] [--score T] --contig NAME:LEN [--contig ...]:
// the host half of --mini on rows given as text.  ROWS holds lines "window lib n n_over saturated sum t_plus t_minus": the rows of
// bdx_window_insert_shift that are not all zero, in any order; `window` counts the grid windows of the contigs one behind the other, in the
// order the contigs are given (mini.h GRID).  --n and --mu are the libraries' null counts and means.  Through the functions the CLI calls
// (mini.cpp, csrc/bdx_mini.h) it prints, tab separated,
//   row        window lib score D          (every line of ROWS in its order; doubles with 17 digits)
//   threshold  T scoring W saturated S     (the threshold used, the windows with a scoring row, the saturated windows)
// and then the merged table as --mini writes it, from its #Chr line on.  Exit 2 for a malformed argument or line.
// bdx-mini-check --scoring-windows W [--scoring-windows ...] alone prints "default-threshold W T" per W: the threshold --mini uses when W
// windows had a scoring row (mini_default_threshold), for counts no rows file could reasonably hold.
// Test tooling: it links no libbdx and needs no GPU (tests/test_mini.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../csrc/bdx_mini.h"
#include "mini.h"

namespace {

int usage() {
    fprintf(stderr, "usage: bdx-mini-check ROWS --n N0,N1,.. --mu M0,M1,.. --window W --step S [--min-pairs P] [--score T] --contig NAME:LEN [--contig ...]\n");
    return 2;
}

std::vector<std::string> split(const std::string& s, char sep) {
    std::vector<std::string> out;
    size_t p = 0;
    for (;;) {
        const size_t q = s.find(sep, p);
        out.push_back(s.substr(p, q == std::string::npos ? std::string::npos : q - p));
        if (q == std::string::npos) return out;
        p = q + 1;
    }
}

}  // namespace

int main(int argc, char** argv) {
    using namespace bdhost;
    std::string rows_path;
    MiniParams p;
    MiniNull null;
    std::vector<std::string> names;
    std::vector<uint32_t> lengths;
    if (argc > 1 && !strcmp(argv[1], "--scoring-windows")) {   // the threshold alone: nothing but pairs "--scoring-windows W"
        for (int i = 1; i < argc; i += 2) {
            char* end = nullptr;
            if (strcmp(argv[i], "--scoring-windows") || i + 1 >= argc || argv[i + 1][0] < '0' || argv[i + 1][0] > '9') return usage();
            const unsigned long long w = strtoull(argv[i + 1], &end, 10);
            if (*end) return usage();
            printf("default-threshold\t%llu\t%d\n", w, mini_default_threshold(w));
        }
        return 0;
    }
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const bool more = i + 1 < argc;
        if (a == "--n" && more) { for (auto& t : split(argv[++i], ',')) null.N.push_back(strtoull(t.c_str(), nullptr, 10)); }
        else if (a == "--mu" && more) { for (auto& t : split(argv[++i], ',')) null.mu.push_back(strtod(t.c_str(), nullptr)); }
        else if (a == "--window" && more) p.window = atoll(argv[++i]);
        else if (a == "--step" && more) p.step = atoll(argv[++i]);
        else if (a == "--min-pairs" && more) p.min_pairs = atoi(argv[++i]);
        else if (a == "--score" && more) p.score = atoi(argv[++i]);
        else if (a == "--contig" && more) {
            const std::string c = argv[++i];
            const size_t q = c.rfind(':');
            if (q == std::string::npos) return usage();
            names.push_back(c.substr(0, q));
            lengths.push_back((uint32_t)strtoul(c.c_str() + q + 1, nullptr, 10));
        } else if (rows_path.empty() && a.compare(0, 2, "--") != 0) rows_path = a;
        else return usage();
    }
    const size_t nlibs = null.N.size();
    if (rows_path.empty() || !nlibs || null.mu.size() != nlibs || p.window < 1 || p.step < 1 || p.min_pairs < 2 || names.empty()) return usage();
    for (size_t l = 0; l < nlibs; ++l) null.usable.push_back(null.N[l] >= kMiniUsable);
    std::vector<uint64_t> first(names.size() + 1, 0);   // the first window of every contig
    for (size_t c = 0; c < names.size(); ++c) first[c + 1] = first[c] + mini_grid(lengths[c], p.step);

    std::ifstream rf(rows_path.c_str());
    if (!rf.is_open()) { fprintf(stderr, "unable to open rows file '%s'\n", rows_path.c_str()); return 2; }
    std::map<uint64_t, std::vector<bdx_insert_shift>> windows;
    std::string line;
    while (std::getline(rf, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        unsigned long long w, lib, n, n_over, sat, sum;
        long long tp, tm;
        std::string rest;
        if (!(in >> w >> lib >> n >> n_over >> sat >> sum >> tp >> tm) || (in >> rest) || lib >= nlibs || w >= first.back()) {
            fprintf(stderr, "not 'window lib n n_over saturated sum t_plus t_minus' with a window of the grid and a library: '%s'\n", line.c_str());
            return 2;
        }
        bdx_insert_shift r{};
        r.n = (uint32_t)n; r.n_over = (uint32_t)n_over; r.saturated = (uint32_t)sat; r.sum = sum; r.t_plus = tp; r.t_minus = tm;
        double sc, d;
        bdx::insert_shift_score(r, null.N[lib], &sc, &d);
        printf("row\t%llu\t%llu\t%.17g\t%.17g\n", w, lib, sc, d);
        auto& rows = windows[w];
        rows.resize(nlibs);
        rows[lib] = r;
    }
    std::vector<MiniKept> kept;
    uint64_t scoring = 0, saturated = 0;
    size_t c = 0;
    for (auto const& kv : windows) {   // (ascending window index: contig by contig, window by window)
        while (kv.first >= first[c + 1]) ++c;
        const MiniWindow w = mini_window(kv.second.data(), null, p.min_pairs);
        scoring += w.scoring;
        saturated += w.saturated;
        if (w.scoring) kept.push_back(MiniKept{(int32_t)c, (int64_t)(kv.first - first[c]), w});
    }
    const int threshold = p.score >= 0 ? p.score : mini_default_threshold(scoring);
    printf("threshold\t%d\tscoring\t%llu\tsaturated\t%llu\n", threshold, (unsigned long long)scoring, (unsigned long long)saturated);
    fflush(stdout);
    mini_write_table(std::cout, mini_merge(kept, threshold, p, lengths), names);
    std::cout.flush();
    return 0;
}
