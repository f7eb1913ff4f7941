// --sites FILE: SV sites to genotype over the records the run holds (no counterpart in the reference).  FILE is the tool's own table, so
// that a run's stdout -- or several runs' merged -- can be fed back; this is its parser.  The counting rule is include/bdx.h
// (bdx_count_site_pairs); the output goes through VcfWriter (vcf.h).
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "bdx.h"

namespace bdhost {

// the table's Type column: what a site may be
extern const char* const kSiteTypes[5];   // DEL INS INV ITX CTX

struct SiteLine {
    int32_t chr1 = 0, pos1 = 0, chr2 = 0, pos2 = 0;   // as the file gave them (the VCF prints these)
    std::string type;
    bool has_size = false;     // a numeric 8th field
    long long size = 0;
    bdx_site site{};           // the same, ends swapped where needed so that (tid1, pos1) <= (tid2, pos2), with the type's flag mask
};

struct SiteTable {
    std::string path;
    std::vector<SiteLine> sites;   // the kept lines, in file order (SITE<k>: k = index + 1)
    size_t unknown_lines = 0;      // lines naming a sequence the header does not have (ignored)
};

// Fields split on tabs; blank lines and lines starting with '#' skipped; at least seven fields Chr1 Pos1 Orientation1 Chr2 Pos2
// Orientation2 Type, a numeric eighth (Size) kept, everything further ignored.  Names are resolved against `targets` (the first BAM's
// header), a line with an unknown one is ignored and counted.  type_masks: for each of kSiteTypes the ReadFlags that map to it under the
// run's -l setting (Options::sv_flag_mask; 0: none).  Throws std::runtime_error with FILE:LINE for fewer than seven fields, a position
// that is not an integer in [1, 2^31 - 1], a type outside kSiteTypes or with mask 0, CTX with Chr1 == Chr2 or another type with
// Chr1 != Chr2; with FILE for an unreadable file.
void read_sites(const std::string& path, const std::vector<std::string>& targets, const std::vector<std::pair<std::string, uint32_t>>& type_masks,
                SiteTable& out);

}  // namespace bdhost
