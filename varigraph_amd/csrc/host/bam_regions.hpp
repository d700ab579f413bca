// bam_regions.hpp -- the regions of a BAM file as the command line gives them, and their resolution against a file's header
// (bam_reader.cpp); the rule they feed is condition 5 of ../vgmi_bam_filter.h.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../vgmi_bam_filter.h"

namespace vgh {

// The regions of `genotype --bam-regions LIST --bam-regions-file BED --bam-regions-unplaced` as the options give them; resolved per BAM
// file, whose header assigns the reference ids.
struct BamRegionSpec {
    std::string list;      // NAME | NAME:BEG | NAME:BEG-END, comma-separated, 1-based inclusive
    std::string bed;       // a BED file's path: columns 1 to 3, 0-based half-open
    bool unplaced = false;
    bool on() const { return !list.empty() || !bed.empty(); }
};
// The spec against the reference names of `path`'s header: the normalised list.  An item of LIST that equals a reference name as a
// whole is that reference, [0, 2^31); else it is split at its last ':'.  Throws "'<path>': reference '<name>' of region '<item>' is
// not in the header", and for a malformed item; for a BED line whose start or end is not a number or has start >= end, naming the
// line; for more than 2^20 merged intervals; for a list that comes out empty (a BED file none of whose lines names a reference of the header).  BED lines whose name the header lacks are skipped and counted in *bed_skipped.
std::vector<BamInterval> resolve_bam_regions(const BamRegionSpec& spec, const std::vector<std::string>& ref_names, const std::string& path,
                                             uint64_t* bed_skipped = nullptr);

}  // namespace vgh
