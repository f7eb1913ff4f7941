// --estimate: from the insert-size histograms of the records a run holds (bdx_insert_size_histogram) to the libraries it runs with, its
// initial window and the configuration rewritten with them.  Nothing here touches the GPU: the arithmetic of one library is
// csrc/bdx_estimate.h's, and bin/bdx-estimate-check runs these functions on a histogram given as text (tests/test_estimate.py).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "bdx.h"
#include "config.h"

namespace bdhost {

struct EstimatePlan {
    std::vector<bdx_insert_estimate> est;   // [nlibs]
    std::vector<uint64_t> n_over;           // [nlibs] observations of BDX_ISIZE_BINS and beyond
    // The run's libraries.  A library with a valid estimate: mean and std the estimate's, upper = mean + c sd_plus,
    // lower = max(0, mean - c sd_minus) with the run's -c -- also where its line gave cutoffs of its own --, each printed with %.2f and
    // read back as float: exactly what the configuration parser makes of the rewritten file.  Read length, minimum quality and BAM index
    // stay the configuration's.  A library without one keeps the configuration's values.
    std::vector<bdx_lib> libs;
    int window = 0;                         // max(50, min over the libraries of int(mean - readlen * 2)), as the parser's (config.cpp)
    std::string config_text;                // the configuration as read; on every line of a library with a valid estimate the mean, std and
                                            // cutoff fields are dropped, "lower: upper: mean: std:" appended and a num: field set to n_kept
    std::vector<std::string> warnings;      // one per library without a valid estimate
    std::string fatal;                      // not empty: such a library's line gave neither mean nor std -- the run cannot go on
};

// hist[nlibs][BDX_ISIZE_BINS], n_over[nlibs]
EstimatePlan plan_estimate(const BamConfig& cfg, const std::string& config_text, int cut_sd, const uint64_t* hist, const uint64_t* n_over);

// "library NAME: n=.. n_over=.. n_kept=.. mean=.. std=.. lower=.. upper=.. valid" for BDX_TIMING's --estimate line
std::string estimate_summary(const BamConfig& cfg, const EstimatePlan& plan);

}  // namespace bdhost
