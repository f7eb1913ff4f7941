// bdx-anchor-check ROWS --min M --contig NAME [--contig ...]: the host half of --anchor on rows given as text.  ROWS holds lines
// "seq n_fwd n_rev n_low n_left n_right u_left u_right split last_left first_right": rows of bdx_window_anchor_split in grid order, `seq`
// the index of a contig given.  Through the functions the CLI calls (anchor.cpp) it prints "calls N" (the rows that call) and then the merged
// table as --anchor writes it, from its #Chr line on.
// bdx-anchor-check --cutoffs U0,U1,.. [--window W] [--step S] [--length LEN] prints "window W step S" as the CLI settles them from the
// libraries' uppercutoffs (nan and inf are read as such) and the options given, and with --length the number of grid windows of a sequence of
// that length behind them ("window W step S windows N"); "error TEXT" and exit 1 when no window can be derived.
// Exit 2 for a malformed argument or line.  Test tooling: it links no libbdx and needs no GPU (tests/test_anchor.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "anchor.h"
#include "mini.h"

namespace {

int usage() {
    fprintf(stderr, "usage: bdx-anchor-check ROWS --min M --contig NAME [--contig ...]\n       bdx-anchor-check --cutoffs U0,U1,.. [--window W] [--step S] [--length LEN]\n");
    return 2;
}

}  // namespace

int main(int argc, char** argv) {
    using namespace bdhost;
    std::string rows_path, cutoffs;
    AnchorParams p;
    long long length = -1;
    std::vector<std::string> names;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const bool more = i + 1 < argc;
        if (a == "--min" && more) p.min = atoi(argv[++i]);
        else if (a == "--window" && more) p.window = atoll(argv[++i]);
        else if (a == "--step" && more) p.step = atoll(argv[++i]);
        else if (a == "--length" && more) length = atoll(argv[++i]);
        else if (a == "--cutoffs" && more) cutoffs = argv[++i];
        else if (a == "--contig" && more) names.push_back(argv[++i]);
        else if (rows_path.empty() && a.compare(0, 2, "--") != 0) rows_path = a;
        else return usage();
    }
    if (!cutoffs.empty()) {
        if (!rows_path.empty() || p.window < 0 || p.step < 0) return usage();
        std::vector<bdx_lib> libs;
        std::istringstream in(cutoffs);
        std::string tok;
        while (std::getline(in, tok, ',')) {
            char* end = nullptr;
            bdx_lib l{};
            l.uppercutoff = strtof(tok.c_str(), &end);
            if (end == tok.c_str() || *end) return usage();
            libs.push_back(l);
        }
        try {
            const int64_t window = p.window > 0 ? p.window : anchor_default_window(libs);
            const int64_t step = p.step > 0 ? p.step : anchor_default_step(window);
            printf("window\t%lld\tstep\t%lld", (long long)window, (long long)step);
            if (length >= 0) printf("\twindows\t%llu", (unsigned long long)mini_grid((uint64_t)length, step));
            printf("\n");
        } catch (const std::runtime_error& e) {
            printf("error\t%s\n", e.what());
            return 1;
        }
        return 0;
    }
    if (rows_path.empty() || p.min < 1 || names.empty()) return usage();
    std::ifstream rf(rows_path.c_str());
    if (!rf.is_open()) { fprintf(stderr, "unable to open rows file '%s'\n", rows_path.c_str()); return 2; }
    std::vector<AnchorCall> called;
    std::string line;
    while (std::getline(rf, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        unsigned long long seq, f[7];
        long long split, ll, fr;
        std::string rest;
        bool ok = (bool)(in >> seq);
        for (int k = 0; ok && k < 7; ++k) ok = (bool)(in >> f[k]) && f[k] <= 0xFFFFFFFFull;
        if (!ok || !(in >> split >> ll >> fr) || (in >> rest) || seq >= names.size() || split < 0 || split > 2147483647ll || ll < -1 || ll > 2147483647ll ||
            fr < -1 || fr > 2147483647ll) {
            fprintf(stderr, "not 'seq n_fwd n_rev n_low n_left n_right u_left u_right split last_left first_right' with a contig given: '%s'\n", line.c_str());
            return 2;
        }
        bdx_anchor_split r{};
        r.n_fwd = (uint32_t)f[0]; r.n_rev = (uint32_t)f[1]; r.n_low = (uint32_t)f[2]; r.n_left = (uint32_t)f[3]; r.n_right = (uint32_t)f[4];
        r.u_left = (uint32_t)f[5]; r.u_right = (uint32_t)f[6]; r.split = (int32_t)split; r.last_left = (int32_t)ll; r.first_right = (int32_t)fr;
        if (anchor_calls(r, p.min)) called.push_back(AnchorCall{(int32_t)seq, r, 1});
    }
    printf("calls\t%zu\n", called.size());
    fflush(stdout);
    anchor_write_table(std::cout, anchor_merge(std::move(called)), names);
    std::cout.flush();
    return 0;
}
