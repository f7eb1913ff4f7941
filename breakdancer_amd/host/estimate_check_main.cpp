// bdx-estimate-check HIST CONFIG [-c N] [--out FILE]: the host half of --estimate on a histogram given as text.  HIST holds lines
// "lib x count" (library index in the configuration's sorted-name order, insert size, observations; x of BDX_ISIZE_BINS and beyond counts
// in n_over; counts of one bin add up), CONFIG is a configuration.  Through the functions the CLI calls (estimate.cpp, csrc/bdx_estimate.h)
// it prints, tab separated,
//   estimate  i name n n_over n_kept n_minus n_plus valid mean_all sd_all mean sd sd_minus sd_plus     (doubles with 17 digits)
//   library   i name mean std upper lower readlen min_mapq bam_index                                   (floats with 9 digits)
//   window    W
//   warning   text                                                                                     (one per library that is not valid)
// and then the rewritten configuration, behind a line "config" on stdout or into FILE.  Exit 1 when the run would end (a library
// without a valid estimate whose line gives neither mean nor std), 2 for a malformed argument or line.
// Test tooling: it links no libbdx and needs no GPU (tests/test_estimate.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "config.h"
#include "estimate.h"

int main(int argc, char** argv) {
    std::string hist_path, config_path, out_path;
    int cut_sd = 3;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "-c") && i + 1 < argc) cut_sd = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--out") && i + 1 < argc) out_path = argv[++i];
        else if (hist_path.empty()) hist_path = argv[i];
        else if (config_path.empty()) config_path = argv[i];
        else { fprintf(stderr, "usage: bdx-estimate-check HIST CONFIG [-c N] [--out FILE]\n"); return 2; }
    }
    if (config_path.empty()) { fprintf(stderr, "usage: bdx-estimate-check HIST CONFIG [-c N] [--out FILE]\n"); return 2; }
    try {
        std::ifstream cf(config_path.c_str());
        if (!cf.is_open()) { fprintf(stderr, "unable to open config file '%s'\n", config_path.c_str()); return 2; }
        std::stringstream ss;
        ss << cf.rdbuf();
        const std::string text = ss.str();
        std::istringstream parsed(text);
        const bdhost::BamConfig cfg(parsed, cut_sd);
        const size_t nlibs = cfg.num_libs();
        std::vector<uint64_t> hist(nlibs * (size_t)BDX_ISIZE_BINS, 0), n_over(nlibs, 0);
        std::ifstream hf(hist_path.c_str());
        if (!hf.is_open()) { fprintf(stderr, "unable to open histogram file '%s'\n", hist_path.c_str()); return 2; }
        std::string line;
        while (std::getline(hf, line)) {
            if (line.empty()) continue;
            std::istringstream in(line);
            long long lib, x;
            unsigned long long count;
            std::string rest;
            if (!(in >> lib >> x >> count) || (in >> rest) || lib < 0 || (size_t)lib >= nlibs || x < 0) {
                fprintf(stderr, "not 'lib x count' with a library of the configuration: '%s'\n", line.c_str());
                return 2;
            }
            if (x >= BDX_ISIZE_BINS) n_over[lib] += count;
            else hist[(size_t)lib * BDX_ISIZE_BINS + (size_t)x] += count;
        }
        const bdhost::EstimatePlan plan = bdhost::plan_estimate(cfg, text, cut_sd, hist.data(), n_over.data());
        for (size_t i = 0; i < nlibs; ++i) {
            const bdx_insert_estimate& e = plan.est[i];
            printf("estimate\t%zu\t%s\t%llu\t%llu\t%llu\t%llu\t%llu\t%d\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\n", i, cfg.library_config(i).name.c_str(),
                   (unsigned long long)e.n, (unsigned long long)plan.n_over[i], (unsigned long long)e.n_kept, (unsigned long long)e.n_minus,
                   (unsigned long long)e.n_plus, e.valid, e.mean_all, e.sd_all, e.mean, e.sd, e.sd_minus, e.sd_plus);
        }
        for (size_t i = 0; i < nlibs; ++i) {
            const bdx_lib& l = plan.libs[i];
            printf("library\t%zu\t%s\t%.9g\t%.9g\t%.9g\t%.9g\t%.9g\t%d\t%d\n", i, cfg.library_config(i).name.c_str(), l.mean_insertsize, l.std_insertsize,
                   l.uppercutoff, l.lowercutoff, l.readlens, l.min_mapping_quality, l.bam_index);
        }
        printf("window\t%d\n", plan.window);
        for (const std::string& w : plan.warnings) printf("warning\t%s\n", w.c_str());
        if (!plan.fatal.empty()) {
            fprintf(stderr, "ERROR: %s\n", plan.fatal.c_str());
            return 1;
        }
        if (out_path.empty()) {
            printf("config\n%s", plan.config_text.c_str());
        } else {
            std::ofstream of(out_path.c_str());
            if (!of.is_open()) { fprintf(stderr, "unable to open '%s' for writing\n", out_path.c_str()); return 2; }
            of << plan.config_text;
        }
    } catch (std::exception const& e) {
        fprintf(stderr, "ERROR: %s\n", e.what());
        return 2;
    }
    return 0;
}
