// --exclude FILE: a BED file of regions whose read pairs the readers drop (no counterpart in the reference, whose -x drops a region after
// its reads have been counted).  The rule itself is csrc/bdx_exclude.h, shared with the device decode; this is the file's parser and
// the table the three readers are handed: ColumnReader and Stream::advance on the host, bdx_bamdec_set_exclude on the device.
#pragma once
#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "bdx.h"
#include "../csrc/bdx_exclude.h"

namespace bdhost {

struct ExcludeTable {
    std::string path;
    std::vector<bdx_interval> intervals;   // sorted and merged: what the device decoder is given
    std::vector<uint32_t> first;           // the same as the table of csrc/bdx_exclude.h, for the host readers
    std::vector<int32_t> beg, end;
    size_t unknown_lines = 0;              // BED lines naming a sequence the header does not have (ignored)
    mutable std::atomic<uint64_t> dropped{0};   // records the run's reader dropped, over all files and ranks (the BDX_TIMING line)
    bdx::ExcludeMask mask() const {
        return bdx::ExcludeMask{first.data(), beg.data(), end.data(), first.empty() ? 0 : (int32_t)first.size() - 1};
    }
};

// Fields split on tabs or spaces, the first three used; blank lines and lines starting with '#', "track" or "browser" skipped; names
// resolved against `targets` (the first BAM's header, the one -o is resolved against), unknown ones ignored and counted; end clamped to
// 2^31 - 1.  Throws std::runtime_error with FILE:LINE for fewer than three fields, a coordinate that is not an integer or is negative,
// end < beg; with FILE for an unreadable file; and for more than 2^24 merged intervals.
void read_exclude_bed(const std::string& path, const std::vector<std::string>& targets, ExcludeTable& out);

// the summary line of a BDX_TIMING=1 run
void print_exclude_timing(const ExcludeTable& t);

}  // namespace bdhost
