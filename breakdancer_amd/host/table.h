// The table breakdancer-max prints: the #Library Statistics block, the column line and one row per printed SV
// (BreakDancerMax.cpp:83-137, BreakDancer.cpp:395-497).  Nothing here touches the GPU: the rows are formatted from what the run
// fetched (bdx_get_svs, bdx_get_sv_lists), so bin/bdx-table-check holds this file to the CPU oracle's text (tests/test_table.py).
#pragma once
#include <cstdint>
#include <ostream>
#include <string>
#include <vector>

#include "bdx.h"
#include "config.h"
#include "options.h"

namespace bdhost {

// the flat lists the bdx_sv rows index (bdx_get_sv_lists): lib_* by lib_begin / lib_count, cn_* by cn_begin / cn_count
struct SvLists {
    std::vector<int32_t> lib_index, lib_pairs, cn_key;
    std::vector<float> cn_value;
};

// pass-1 statistics of the run (bdx_get_summary, bdx_get_counters), as the header prints them
struct TableCounters {
    uint32_t covered_ref_len = 0;
    std::vector<uint32_t> lib_count, bam_count, flag_hist;   // [nlibs], [nbams], [nlibs * BDX_NUM_FLAGS]
    std::vector<float> seqcov, density;                      // [nlibs]
};

// The sample columns of the table and of the VCFs: the libraries with -a, else the BAM files' base names.
std::vector<std::string> sample_names(const Options& opts, const BamConfig& cfg);

class TableFormat {
public:
    // (keeps references: all three outlive the formatter)
    TableFormat(const Options& opts, const BamConfig& cfg, const std::vector<std::string>& targets) : opts_(opts), cfg_(cfg), targets_(targets) {}
    // "#Software" ... "#Library Statistics:" and the column line
    void header(std::ostream& os, const TableCounters& c) const;
    // one row of the table (BreakDancer.cpp:395-497) into `os`; the stream's manipulators carry over to the next row
    void row(std::ostream& os, const bdx_sv& s, const SvLists& l) const;
    // does this row leave the stream printing fixed with two decimals (see row)?
    bool sets_fixed(const bdx_sv& s, const SvLists& l) const;
    // the rows svs[printed_rows[k]] in order, formatted by `threads` threads (1: straight into os), and os left in the state the
    // sequential loop leaves it in
    void write_rows(std::ostream& os, const std::vector<bdx_sv>& svs, const std::vector<size_t>& printed_rows, const SvLists& l, size_t threads) const;
    // sequence name of a reference id (the id itself where the header has none)
    std::string target_name(int t) const { return (t >= 0 && (size_t)t < targets_.size()) ? targets_[t] : std::to_string(t); }

private:
    const Options& opts_;
    const BamConfig& cfg_;
    const std::vector<std::string>& targets_;
};

}  // namespace bdhost
