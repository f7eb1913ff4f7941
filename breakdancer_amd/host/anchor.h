// --anchor: insertion sites from the one-end-anchored reads (mapped, mate unmapped) that start inside sliding windows: right-pointing
// anchors pile up left of a junction, left-pointing ones right of it (bdx_window_anchor_split on the GPU; the rule is in include/bdx.h).
// Here: what the CLI and bdx-anchor-check share behind the rows the GPU returns -- the default window and step, a window's call, the merge
// and the file.  No GPU, no libbdx.
//
//   WINDOW     --anchor-window, or 2 x the ceiling of the largest finite library uppercutoff (at most 2^30); an error when that is not
//              positive.  STEP: --anchor-step, or half the window, at least 1.  With these every junction lies in the middle half of some
//              window.
//   GRID       --mini's: window j of a sequence of length len is [j step, j step + window) clamped to len, for every j with j step < len.
//   CALL       a window calls when u_left >= min and u_right >= min (--anchor-min): distinct starts, because duplicates of these reads are
//              never marked.
//   MERGE      calls in (sequence, split) order; two calls of one sequence belong together when their closed intervals
//              [last_left, first_right] intersect, transitively.  The row kept has the largest u_left + u_right, then the largest
//              n_left + n_right, then the smallest split; Windows = the calls it stands for.
//   FILE       tab separated, in sequence and position order: #Chr Pos1 Pos2 Type Left Right DistinctLeft DistinctRight LowQual Windows with
//              Pos1 = last_left + 1 and Pos2 = first_right + 1 (1-based: the junction lies right of the read starting at Pos1 and not right
//              of Pos2), Type INS, and n_left, n_right, u_left, u_right, n_low of the row kept.
#pragma once
#include <cstdint>
#include <iosfwd>
#include <string>
#include <vector>

#include "bdx.h"

namespace bdhost {

struct AnchorParams {
    int64_t window = 0, step = 0;
    int min = 3;
    int mapq = -1;                     // bdx_window_anchor_split's min_qual
};

// the default window from the libraries' uppercutoffs; throws std::runtime_error when no cutoff gives a window of at least 1
int64_t anchor_default_window(const std::vector<bdx_lib>& libs);
inline int64_t anchor_default_step(int64_t window) { return window / 2 > 1 ? window / 2 : 1; }

inline bool anchor_calls(const bdx_anchor_split& r, int min) { return r.u_left >= (uint32_t)min && r.u_right >= (uint32_t)min; }

struct AnchorCall {
    int32_t seq;
    bdx_anchor_split row;
    uint64_t windows;
};
// called: rows that call, in any order; returns the merged calls in (seq, split) order
std::vector<AnchorCall> anchor_merge(std::vector<AnchorCall> called);

void anchor_write_table(std::ostream& out, const std::vector<AnchorCall>& calls, const std::vector<std::string>& names);

}  // namespace bdhost
