// --mini: small insertions and deletions from the insert sizes of the pairs that start inside sliding windows, each window tested against
// its libraries' genome-wide distributions with Kolmogorov-Smirnov (bdx_window_insert_shift on the GPU, include/bdx.h; the score is
// csrc/bdx_mini.h).  Here: what the CLI and bdx-mini-check share behind the rows the GPU returns -- the null's figures, a window's call,
// the threshold, the merge and the file.  No GPU, no libbdx.
//
//   NULL       N_L = the histogram's total, mu_L = its mean (double, bins ascending, count * x).  A library is USABLE when N_L >= 1000.
//   GRID       window j of a sequence of length len is [j step, j step + window), for every j with j step < len.
//   WINDOW     its SCORING rows are those of usable libraries with n >= min-pairs and saturated == 0.  Score = the sum of their scores
//              (libraries are independent, as the table's own score adds them); Pairs = the sum of their n;
//              Shift = sum_L (sum_L - n_L mu_L) / Pairs, the terms added in library order in double; D = that of the row with the largest
//              score (the first such row).  Type DEL for Shift > 0, INS otherwise.
//   THRESHOLD  --mini-score, or 20 + ceil(10 log10 W) with W = the windows that have a scoring row (W = 0: 20).  This is Bonferroni: at
//              most 0.01 expected false windows under the asymptotic null.
//   MERGE      maximal runs of consecutive windows of one sequence that have a scoring row, reach the threshold (Score >= threshold) and share
//              their Type are one call: Beg = the first window's start + 1, End = the last window's end clamped to the sequence,
//              Shift / Score / Pairs / D of the run's best window (the largest Score, the first such), Windows = the run's length.
//   FILE       tab separated: #Chr Beg End Type Shift Score Pairs D Windows; Shift "%.1f", D "%.3f", Score floor(Score + 0.5) capped at 99999.
#pragma once
#include <cstdint>
#include <iosfwd>
#include <string>
#include <vector>

#include "bdx.h"

namespace bdhost {

struct MiniParams {
    int64_t window = 0, step = 0;
    int min_pairs = 20;
    int score = -1;                    // -1: the default threshold
};

// the default window: the ceiling of the largest finite positive library mean insert size; throws std::runtime_error when there is none
int64_t mini_mean_window(const std::vector<bdx_lib>& libs);

struct MiniNull {
    std::vector<uint64_t> N;
    std::vector<double> mu;
    std::vector<char> usable;
};
MiniNull mini_null(const uint64_t* hist, size_t nlibs);   // hist[nlibs][BDX_ISIZE_BINS]
constexpr uint64_t kMiniUsable = 1000;

struct MiniWindow {
    bool scoring = false, saturated = false, del = false;   // saturated: some row of the window is
    double score = 0, shift = 0, D = 0;
    uint64_t pairs = 0;
};
MiniWindow mini_window(const bdx_insert_shift* rows, const MiniNull& null, int min_pairs);

int mini_default_threshold(uint64_t scoring_windows);
// windows of a sequence
inline uint64_t mini_grid(uint64_t len, int64_t step) { return len ? (len - 1) / (uint64_t)step + 1 : 0; }

struct MiniKept {                      // a window worth keeping: it has a scoring row and may reach the threshold
    int32_t seq;
    int64_t j;
    MiniWindow w;
};
struct MiniCall {
    int32_t seq;
    int64_t beg, end;                  // 1-based, inclusive end
    bool del;
    double shift, score, D;
    uint64_t pairs, windows;
};
// kept: in (seq, j) order
std::vector<MiniCall> mini_merge(const std::vector<MiniKept>& kept, int threshold, const MiniParams& p, const std::vector<uint32_t>& lengths);

void mini_write_table(std::ostream& out, const std::vector<MiniCall>& calls, const std::vector<std::string>& names);

}  // namespace bdhost
